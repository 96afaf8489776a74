// Depths from bone lengths: 2-D detections without a depth network.
// Included from errors.hip, behind keypoints.h (kp_usable, kp_camera2world).
//
//   gem_bone_depths  per frame, the 15 depths d_j along the detections' unit rays r_j that meet the skeleton's bone lengths:
//                    14 bone residuals |d_j r_j - d_p r_p| - L_j, the neck's anchor sqrt(w_n) (d_0 - neck_depth), and a weak prior
//                    sqrt(w_m) (d_j - dbar_j) that settles each bone's near / far choice; Levenberg-Marquardt from dbar, a fixed
//                    number of iterations, no state between frames.
//
// The normal matrix has the skeleton's tree as its graph: a bone row touches j and p(j) only, anchor and prior are diagonal, and
// p(j) < j, so eliminating joints 14 .. 1 into their parents produces no fill.  A step is a diagonal D[15], one off-diagonal per joint
// and a right-hand side: O(15), no dense factorisation.
//
// Layout: ONE THREAD PER FRAME, one wavefront per workgroup, everything in registers (the parent table is a compile-time constant and
// every joint loop is unrolled, so rays, depths and the three vectors of the system are named registers: about 125 doubles).  The
// other candidate, one lane per joint with four frames per wavefront, shortens the dependent chain per iteration from 14 joints to
// 5 tree levels but pays two cross-lane exchanges per level in each of the two sweeps and a 16-lane reduction for the cost of every
// trial point, all on the critical path of a loop that cannot overlap its iterations; a recording is a few thousand frames, so both
// layouts leave most of the device idle, and the per-frame thread needs no LDS, no barrier and no cross-lane order to keep fixed.
// Being alone in its thread also makes a frame's bytes independent of the frames beside it by construction.
//
// float64 throughout, no fused multiply-adds in the solver (the numpy twin of the tests rounds the same way), every sum in a fixed
// order, no atomics.  The ray is kp_camera2world at depth 1 -- the very function gem_lift_keypoints calls, so depth * ray there has the
// bits of d_j r_j here.
#pragma once
#include "keypoints.h"

namespace gem {

constexpr int BD_J = 15;
constexpr int BD_THREADS = 64;                    // one wavefront per workgroup: a recording's frames spread over as many CUs as they fill
constexpr double BD_FLOOR = 0.01;                 // depths are floored at 1 cm
constexpr double BD_LAMBDA0 = 1e-3, BD_LAMBDA_MIN = 1e-12, BD_LAMBDA_MAX = 1e12;
__device__ constexpr int BD_PARENT[BD_J] = {0, 0, 1, 2, 0, 4, 5, 1, 7, 8, 9, 4, 11, 12, 13};
static const int BD_PARENT_HOST[BD_J] = {0, 0, 1, 2, 0, 4, 5, 1, 7, 8, 9, 4, 11, 12, 13};

struct BoneDepthArgs {
    KpLiftArgs cam;            // kp, n, n_poly, poly, cx, cy: what kp_camera2world reads (the other members are unused here)
    gem_bone_depth_opts o;
    double* depth;             // [n,15] or nullptr
    unsigned char* solved;     // [n,15] or nullptr
    double* rms;               // [n] or nullptr
};

// residual of bone j at depths d, and (want_jac) its two derivatives: a = d e / d d_j, b = d e / d d_p; a bone of zero extent has none
__device__ __forceinline__ double bd_bone(const double (&r)[BD_J][3], const double (&d)[BD_J], int j, int p, double L, double& a, double& b) {
#pragma clang fp contract(off)
    const double v0 = d[j] * r[j][0] - d[p] * r[p][0], v1 = d[j] * r[j][1] - d[p] * r[p][1], v2 = d[j] * r[j][2] - d[p] * r[p][2];
    const double len = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
    const double dj = v0 * r[j][0] + v1 * r[j][1] + v2 * r[j][2], dp = v0 * r[p][0] + v1 * r[p][1] + v2 * r[p][2];
    a = len > 0.0 ? dj / len : 0.0;
    b = len > 0.0 ? -(dp / len) : 0.0;
    return len - L;
}

// anchor, then the priors of the joints that take part (ascending), then the bones (ascending); `bones`: the bones' share alone
__device__ __forceinline__ double bd_cost(const gem_bone_depth_opts& o, const double (&r)[BD_J][3], const double (&d)[BD_J],
                                          const bool (&on)[BD_J], double& bones) {
#pragma clang fp contract(off)
    const double t0 = d[0] - o.neck_depth;
    double c = o.w_n * (t0 * t0);
#pragma unroll
    for (int j = 0; j < BD_J; ++j) {
        const double t = d[j] - o.dbar[j];
        c += on[j] ? o.w_m * (t * t) : 0.0;
    }
    bones = 0.0;
#pragma unroll
    for (int j = 1; j < BD_J; ++j) {
        double a, b;
        const double e = bd_bone(r, d, j, BD_PARENT[j], o.bone[j], a, b);
        bones += on[j] ? e * e : 0.0;
    }
    return c + bones;
}

__global__ __launch_bounds__(BD_THREADS) void bone_depths_kernel(BoneDepthArgs A) {
#pragma clang fp contract(off)
    const int f = blockIdx.x * BD_THREADS + threadIdx.x;
    if (f >= A.cam.n) return;
    const gem_bone_depth_opts& o = A.o;
    const double* kp = A.cam.kp + (size_t)f * BD_J * 3;
    double r[BD_J][3], d[BD_J];
    bool on[BD_J];                                // SOLVED: usable, and so is every joint on the path to the neck
    int n_bones = 0;
#pragma unroll
    for (int j = 0; j < BD_J; ++j) {
        const double u = kp[j * 3], v = kp[j * 3 + 1], conf = kp[j * 3 + 2];
        const bool ok = kp_usable(u, v, conf);
        on[j] = ok && (j == 0 || on[BD_PARENT[j]]);
        r[j][0] = r[j][1] = r[j][2] = 0.0;
        if (ok) kp_camera2world(A.cam, u, v, 1.0, r[j]);
        d[j] = o.dbar[j];
        if (j > 0 && on[j]) ++n_bones;
    }
    double bones = 0.0;
    if (on[0]) {                                  // (a frame without its neck keeps every prior depth)
        double cost = bd_cost(o, r, d, on, bones), lam = BD_LAMBDA0;
        for (int it = 0; it < o.iters; ++it) {
            // the normal equations at d: diagonal D, off-diagonal off[j] = A[j][p(j)], right-hand side g = J^T residual
            double D[BD_J], off[BD_J], g[BD_J];
            D[0] = o.w_n + o.w_m;
            g[0] = o.w_n * (d[0] - o.neck_depth) + o.w_m * (d[0] - o.dbar[0]);
            off[0] = 0.0;
#pragma unroll
            for (int j = 1; j < BD_J; ++j) {
                D[j] = on[j] ? o.w_m : 1.0;
                g[j] = on[j] ? o.w_m * (d[j] - o.dbar[j]) : 0.0;
            }
#pragma unroll
            for (int j = 1; j < BD_J; ++j) {
                const int p = BD_PARENT[j];
                double a, b;
                const double e = bd_bone(r, d, j, p, o.bone[j], a, b);
                const bool t = on[j];
                D[j] += t ? a * a : 0.0;
                D[p] += t ? b * b : 0.0;
                off[j] = t ? a * b : 0.0;
                g[j] += t ? a * e : 0.0;
                g[p] += t ? b * e : 0.0;
            }
            const double damp = 1.0 + lam;
#pragma unroll
            for (int j = 0; j < BD_J; ++j) D[j] = on[j] ? D[j] * damp : 1.0;
            // leaves into parents: no fill
#pragma unroll
            for (int j = BD_J - 1; j >= 1; --j) {
                const int p = BD_PARENT[j];
                const double m = off[j] / D[j];
                D[p] -= m * off[j];
                g[p] -= m * g[j];
            }
            // ... and back: g becomes the step
            g[0] = -g[0] / D[0];
#pragma unroll
            for (int j = 1; j < BD_J; ++j) g[j] = (-g[j] - off[j] * g[BD_PARENT[j]]) / D[j];
            double dn[BD_J];
#pragma unroll
            for (int j = 0; j < BD_J; ++j) dn[j] = on[j] ? fmax(d[j] + g[j], BD_FLOOR) : d[j];
            double bones_n;
            const double cost_n = bd_cost(o, r, dn, on, bones_n);
            const bool take = cost_n < cost;      // (a NaN is not taken)
#pragma unroll
            for (int j = 0; j < BD_J; ++j) d[j] = take ? dn[j] : d[j];
            cost = take ? cost_n : cost;
            bones = take ? bones_n : bones;
            lam = take ? fmax(lam * 0.1, BD_LAMBDA_MIN) : fmin(lam * 10.0, BD_LAMBDA_MAX);
        }
    }
#pragma unroll
    for (int j = 0; j < BD_J; ++j) {
        if (A.depth) A.depth[(size_t)f * BD_J + j] = d[j];
        if (A.solved) A.solved[(size_t)f * BD_J + j] = on[j] ? 1 : 0;
    }
    if (A.rms) A.rms[f] = n_bones > 0 ? sqrt(bones / (double)n_bones) : 0.0;
}

}  // namespace gem

extern "C" {

int gem_bone_depths(gem_handle* h, const double* d_kp, int64_t n_frames, const double* h_poly_c2w, int n_poly, const gem_bone_depth_opts* opts,
                    double* d_depth, unsigned char* d_solved, double* d_rms, void* stream) {
    using namespace gem;
    if (!h) { set_error("gem_bone_depths: null handle"); return 1; }
    if (n_frames < 0 || n_frames > 0x7fffffff / MAXJ_ERR || n_poly < 1 || n_poly > GEM_MAX_POLY) {
        set_error("gem_bone_depths: need 0 <= n_frames < 2^27 and 1 <= n_poly <= 16"); return 1;
    }
    bool tree = h->J == BD_J;
    for (int j = 0; tree && j < BD_J; ++j) tree = h->cfg.parents[j] == BD_PARENT_HOST[j];
    if (!tree) { set_error("gem_bone_depths: the handle's skeleton is not the 15-joint egocentric tree"); return 1; }
    if (!opts || !h_poly_c2w) { set_error("gem_bone_depths: null argument"); return 1; }
    bool ok = opts->bone[0] == 0.0 && std::isfinite(opts->neck_depth) && opts->neck_depth > 0.0 && std::isfinite(opts->w_n) && opts->w_n >= 0.0 &&
              std::isfinite(opts->w_m) && opts->w_m > 0.0;
    for (int j = 0; j < BD_J; ++j)
        ok = ok && std::isfinite(opts->bone[j]) && opts->bone[j] >= 0.0 && std::isfinite(opts->dbar[j]) && opts->dbar[j] >= BD_FLOOR;
    if (!ok) {
        set_error("gem_bone_depths: need finite bone lengths >= 0 with bone[0] = 0, prior depths >= 0.01, neck_depth > 0, w_n >= 0 and w_m > 0");
        return 1;
    }
    if (opts->iters < 1 || opts->iters > 1000) { set_error("gem_bone_depths: need 1 <= iters <= 1000"); return 1; }
    if (n_frames == 0) return 0;
    if (!d_kp || (!d_depth && !d_solved && !d_rms)) { set_error("gem_bone_depths: null argument"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    BoneDepthArgs a;
    a.cam.kp = d_kp; a.cam.depth = nullptr; a.cam.prev = nullptr; a.cam.out64 = nullptr; a.cam.out32 = nullptr; a.cam.valid = nullptr;
    a.cam.n = (int)n_frames; a.cam.J = BD_J; a.cam.n_poly = n_poly;
    for (int i = 0; i < GEM_MAX_POLY; ++i) a.cam.poly[i] = i < n_poly ? h_poly_c2w[i] : 0.0;
    a.cam.cx = h->cfg.cx; a.cam.cy = h->cfg.cy;
    a.o = *opts;
    a.depth = d_depth; a.solved = d_solved; a.rms = d_rms;
    hipLaunchKernelGGL(bone_depths_kernel, dim3((unsigned)((n_frames + BD_THREADS - 1) / BD_THREADS)), dim3(BD_THREADS), 0,
                       static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
