// The SLAM scale of a recording without ground truth, from foot contacts.  Included from errors.hip.
//
//   gem_slam_scale_work  bytes of scratch a call needs (no GPU)
//   gem_slam_scale       feet -> pairs -> 513 candidate costs -> argmin -> four refit rounds -> the report, all on the caller's stream
//
// A foot that stands does not move in the world, so R_t x_t,foot + s c_t is constant over a stance phase: with q = R x the foot
// point carried along the camera's rotation, a = q[t+k] - q[t] and b = c[t+k] - c[t], a stance pair has a = -s b.  Everything is
// float64, written as the numpy twin writes it (no fused multiply-adds), and every sum has a fixed order -- per-lane partial sums
// in pair order, DPP wavefront sums, the wavefronts of a workgroup in order, the workgroups / tiles in order by a later launch --
// so two calls give the same bits; there are no floating-point atomics.
//
//   scale_feet_kernel    one thread per (frame, side): the chunk's own allocation through the pointer table, q = R (ankle + foot) / 2
//   scale_pairs_kernel   one thread per pair: validity from the frame ids, a (two sides) and b, nine doubles; an invalid pair is
//                        stored as zeros (it adds +0.0 to every sum); per-workgroup sums of |a|^2, |b|^2 and the count
//   scale_ref_kernel     the workgroups' sums in order -> s_ref
//   scale_cost_kernel    one workgroup per tile of SC_TILE pairs, staged in LDS (18 KB); a thread owns three candidates and walks the
//                        tile in order -- every LDS read is a broadcast, and is used three times -- -> [n_tiles, 513] partial costs
//   scale_argmin_kernel  the tiles in order per candidate, then the smallest cost (the smallest g of equal ones)
//   scale_fit_kernel     ONE workgroup of 1024: four rounds of (side, inlier, s <- -sum<a,b> / sum<b,b>) and the report round, each
//                        round's s feeding the next on the device; then a wavefront per chunk for the per-chunk sums
#pragma once
#include "gem_internal.h"
#include <cmath>

namespace gem {

constexpr int SC_THREADS = 256;          // feet / pairs kernels
constexpr int SC_TILE = GEM_SCALE_TILE;  // pairs per workgroup of the cost kernel
constexpr int SC_CAND = GEM_SCALE_CANDIDATES;
constexpr int SC_COST_THREADS = 192;     // x 3 candidates each = 576 >= 513
constexpr int SC_FIT_THREADS = 1024;
constexpr int SC_ROUNDS = 4;
constexpr int SC_MAX_FRAMES = 1 << 24;
static_assert(SC_COST_THREADS * 3 >= SC_CAND && (SC_CAND & 1) == 1, "three candidates per thread cover them all");

struct ScaleArgs {
    const int64_t* chunks;     // device: [n_chunks] addresses of the chunks' [n,J,3] f64 poses, then [n_chunks + 1] first rows
    const double* rot;         // [N,3,3]
    const double* trans;       // [N,3]
    const int64_t* ids;        // [N]
    int n_chunks, J, N, P, lag, min_pairs, nb, n_tiles;
    int feet[4];               // right ankle, right foot, left ankle, left foot
    double tau, tau2;
    double* q;                 // [N,2,3]
    double* pair;              // [P,9]: a right, a left, b
    int* flag;                 // [P]
    double* part;              // [nb,3]
    double* sums;              // [8]: sum |a|^2, sum |b|^2, s_ref, pairs, s0, g0, status
    double* tile_cost;         // [n_tiles,513]
    double* costs;             // [513]
    double* report;            // [16 + 3 n_chunks]
    double* out_costs;         // [513] or nullptr
};

__device__ __forceinline__ double sc_candidate(double s_ref, int g) { return s_ref * exp2((double)(g - SC_CAND / 2) / 32.0); }

// |a + s b|^2 as the twin writes it: the product rounded, the sum rounded, three squares added left to right
__device__ __forceinline__ double sc_residual(const double* a, const double* b, double s) {
#pragma clang fp contract(off)
    const double d0 = a[0] + s * b[0], d1 = a[1] + s * b[1], d2 = a[2] + s * b[2];
    return d0 * d0 + d1 * d1 + d2 * d2;
}
__device__ __forceinline__ double sc_dot(const double* u, const double* v) {
#pragma clang fp contract(off)
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
}

// the workgroup's total of NV values per thread, in every thread: wavefront sums, then the wavefronts in order
template <int NW, int NV>
__device__ __forceinline__ void sc_block_sum(double (&v)[NV], double (*red)[NV], int tid) {
    __syncthreads();          // (the previous use of `red` is over)
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const double w = wave_sum_dpp(v[c]);
        if ((tid & 63) == 0) red[tid >> 6][c] = w;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        double t = 0.0;
        for (int w = 0; w < NW; ++w) t += red[w][c];
        v[c] = t;
    }
}

__global__ __launch_bounds__(SC_THREADS) void scale_feet_kernel(ScaleArgs a) {
    const int i = blockIdx.x * SC_THREADS + threadIdx.x;
    if (i >= 2 * a.N) return;
    const int t = i >> 1, side = i & 1;
    const int64_t* start = a.chunks + a.n_chunks;
    int lo = 0, hi = a.n_chunks - 1;          // the last chunk that begins at or before row t (start[0] = 0, start[n_chunks] = N > t)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const double* x = reinterpret_cast<const double*>(a.chunks[lo]) + (size_t)(t - start[lo]) * a.J * 3;
    const double* xa = x + a.feet[2 * side] * 3;
    const double* xf = x + a.feet[2 * side + 1] * 3;
    const double* R = a.rot + (size_t)t * 9;
    double* q = a.q + (size_t)i * 3;
    {
#pragma clang fp contract(off)
        const double m0 = 0.5 * (xa[0] + xf[0]), m1 = 0.5 * (xa[1] + xf[1]), m2 = 0.5 * (xa[2] + xf[2]);
        for (int r = 0; r < 3; ++r) q[r] = R[r * 3] * m0 + R[r * 3 + 1] * m1 + R[r * 3 + 2] * m2;
    }
}

__global__ __launch_bounds__(SC_THREADS) void scale_pairs_kernel(ScaleArgs a) {
    __shared__ double red[SC_THREADS / 64][3];
    const int tid = threadIdx.x, p = blockIdx.x * SC_THREADS + tid;
    double v[3] = {0.0, 0.0, 0.0};
    if (p < a.P) {
        const bool ok = a.ids[p + a.lag] - a.ids[p] == (int64_t)a.lag;
        double w[9];
        for (int c = 0; c < 6; ++c) w[c] = ok ? a.q[(size_t)(p + a.lag) * 6 + c] - a.q[(size_t)p * 6 + c] : 0.0;
        for (int c = 0; c < 3; ++c) w[6 + c] = ok ? a.trans[(size_t)(p + a.lag) * 3 + c] - a.trans[(size_t)p * 3 + c] : 0.0;
        for (int c = 0; c < 9; ++c) a.pair[(size_t)p * 9 + c] = w[c];
        a.flag[p] = ok ? 1 : 0;
        {
#pragma clang fp contract(off)
            v[0] = sc_dot(w, w) + sc_dot(w + 3, w + 3);
            v[1] = sc_dot(w + 6, w + 6);
        }
        v[2] = ok ? 1.0 : 0.0;
    }
    sc_block_sum<SC_THREADS / 64, 3>(v, red, tid);
    if (tid < 3) a.part[(size_t)blockIdx.x * 3 + tid] = v[tid];
}

__global__ __launch_bounds__(64) void scale_ref_kernel(ScaleArgs a) {
    __shared__ double tot[3];
    const int c = threadIdx.x;
    if (c < 3) {
        double t = 0.0;
        for (int b = 0; b < a.nb; ++b) t += a.part[(size_t)b * 3 + c];
        tot[c] = t;
    }
    __syncthreads();
    if (c == 0) {
        a.sums[0] = tot[0]; a.sums[1] = tot[1]; a.sums[3] = tot[2];
        a.sums[2] = sqrt(tot[0] / (2.0 * tot[1]));
        a.sums[6] = (tot[2] == 0.0 || tot[1] == 0.0) ? (double)GEM_SCALE_NO_PAIRS : 0.0;
    }
}

__global__ __launch_bounds__(SC_COST_THREADS) void scale_cost_kernel(ScaleArgs a) {
    __shared__ double tile[SC_TILE * 9];
    const int tid = threadIdx.x, p0 = blockIdx.x * SC_TILE, n = min(SC_TILE, a.P - p0);
    for (int i = tid; i < n * 9; i += SC_COST_THREADS) tile[i] = a.pair[(size_t)p0 * 9 + i];
    __syncthreads();
    const double s_ref = a.sums[2], tau2 = a.tau2;
    double s[3], acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] = sc_candidate(s_ref, min(tid + SC_COST_THREADS * j, SC_CAND - 1));
    for (int p = 0; p < n; ++p) {
        double w[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) w[c] = tile[p * 9 + c];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double r0 = sc_residual(w, w + 6, s[j]), r1 = sc_residual(w + 3, w + 6, s[j]);
            const double m = r1 < r0 ? r1 : r0;
            acc[j] += m < tau2 ? m : tau2;
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int g = tid + SC_COST_THREADS * j;
        if (g < SC_CAND) a.tile_cost[(size_t)blockIdx.x * SC_CAND + g] = acc[j];
    }
}

__global__ __launch_bounds__(SC_THREADS) void scale_argmin_kernel(ScaleArgs a) {
    __shared__ double cost[SC_CAND];
    const int tid = threadIdx.x;
    for (int g = tid; g < SC_CAND; g += SC_THREADS) {
        double t = 0.0;
        for (int k = 0; k < a.n_tiles; ++k) t += a.tile_cost[(size_t)k * SC_CAND + g];
        cost[g] = t;
        a.costs[g] = t;
        if (a.out_costs) a.out_costs[g] = t;
    }
    __syncthreads();
    if (tid == 0) {
        int g0 = 0;
        for (int g = 1; g < SC_CAND; ++g)
            if (cost[g] < cost[g0]) g0 = g;
        a.sums[4] = sc_candidate(a.sums[2], g0);
        a.sums[5] = (double)g0;
    }
}

// one pair at scale s: which side, its residual, whether it is an inlier.  -> false for a pair that does not count
struct ScPair { double ab, bb, rs, nb; int side; bool inl; };
__device__ __forceinline__ bool sc_pair_at(const ScaleArgs& a, int p, double s, ScPair* o) {
    if (!a.flag[p]) return false;
    double w[9];
    for (int c = 0; c < 9; ++c) w[c] = a.pair[(size_t)p * 9 + c];
    const double r0 = sc_residual(w, w + 6, s), r1 = sc_residual(w + 3, w + 6, s);
    o->side = r1 < r0 ? 1 : 0;          // (a tie takes the right foot)
    o->rs = o->side ? r1 : r0;
    o->inl = o->rs < a.tau2;
    o->ab = sc_dot(w + 3 * o->side, w + 6);
    o->bb = sc_dot(w + 6, w + 6);
    o->nb = sqrt(o->bb);
    return true;
}

__global__ __launch_bounds__(SC_FIT_THREADS) void scale_fit_kernel(ScaleArgs a) {
    constexpr int NW = SC_FIT_THREADS / 64;
    __shared__ double red[NW][7];
    const int tid = threadIdx.x;
    double s = a.sums[4];
    double v[7];
    for (int round = 0; round <= SC_ROUNDS; ++round) {
        // numerator, denominator, inliers, of them on the left foot, informative ones, their squared residuals, sum |b| of all pairs
        for (int c = 0; c < 7; ++c) v[c] = 0.0;
        for (int p = tid; p < a.P; p += SC_FIT_THREADS) {
            ScPair k;
            if (!sc_pair_at(a, p, s, &k)) continue;
            v[6] += k.nb;
            if (!k.inl) continue;
            v[0] += k.ab; v[1] += k.bb; v[2] += 1.0; v[3] += (double)k.side; v[5] += k.rs;
            if (s * k.nb > a.tau) v[4] += 1.0;
        }
        sc_block_sum<NW, 7>(v, red, tid);
        if (round < SC_ROUNDS) s = -v[0] / v[1];
    }
    // per chunk: a wavefront sums the inlier pairs whose first frame lies in the chunk, at the final s
    const int64_t* start = a.chunks + a.n_chunks;
    for (int ch = tid >> 6; ch < a.n_chunks; ch += NW) {
        const int p1 = (int)min(start[ch + 1], (int64_t)a.P);
        double num = 0.0, den = 0.0;
        for (int p = (int)start[ch] + (tid & 63); p < p1; p += 64) {
            ScPair k;
            if (sc_pair_at(a, p, s, &k) && k.inl) { num += k.ab; den += k.bb; }
        }
        num = wave_sum_dpp(num); den = wave_sum_dpp(den);
        if ((tid & 63) == 0) {
            double* o = a.report + GEM_SCALE_REPORT_DOUBLES + (size_t)ch * 3;
            o[0] = num; o[1] = den; o[2] = -num / den;
        }
    }
    if (tid == 0) {
        double status = a.sums[6];
        if (status == 0.0 && !(isfinite(s) && s > 0.0)) status = (double)GEM_SCALE_BAD_SCALE;
        if (status == 0.0 && v[4] < (double)a.min_pairs) status = (double)GEM_SCALE_TOO_FEW;
        double* o = a.report;
        o[0] = s; o[1] = a.sums[4]; o[2] = a.sums[2]; o[3] = a.sums[5]; o[4] = a.sums[3]; o[5] = v[2]; o[6] = v[4];
        o[7] = sqrt(v[5] / v[2]);
        o[8] = s * v[6] / (double)a.lag;
        o[9] = (v[2] - v[3]) / v[2]; o[10] = v[3] / v[2];
        o[11] = status; o[12] = (double)a.lag; o[13] = a.tau; o[14] = (double)a.min_pairs; o[15] = (double)a.n_chunks;
    }
}

inline int64_t scale_work_doubles(int64_t N, int lag, int n_chunks, int64_t* off) {
    const int64_t P = N - lag, nb = (P + SC_THREADS - 1) / SC_THREADS, nt = (P + SC_TILE - 1) / SC_TILE;
    int64_t at = 0;
    const int64_t sizes[7] = {6 * N, 9 * P, (P + 1) / 2, 3 * nb, 8, nt * SC_CAND, SC_CAND};      // q, pair, flag, part, sums, tile_cost, costs
    for (int i = 0; i < 7; ++i) { if (off) off[i] = at; at += sizes[i]; }
    (void)n_chunks;
    return at;
}

}  // namespace gem

extern "C" {

int64_t gem_slam_scale_work(int64_t n_frames, int lag, int n_chunks) {
    using namespace gem;
    if (n_frames < 1 || n_frames > SC_MAX_FRAMES || lag < 1 || n_chunks < 1) {
        set_error("gem_slam_scale_work: need 1 <= n_frames <= 2^24, lag >= 1 and n_chunks >= 1"); return -1;
    }
    if (n_frames <= lag) return 8;          // (nothing is launched for such a call)
    return scale_work_doubles(n_frames, lag, n_chunks, nullptr) * (int64_t)sizeof(double);
}

int gem_slam_scale(const int64_t* h_chunks, const int64_t* d_chunks, int n_chunks, int n_joints, const int* h_feet, const double* d_rot,
                   const double* d_trans, const int64_t* d_ids, int64_t n_frames, int lag, double tau, int min_pairs, void* d_work,
                   int64_t work_bytes, double* d_report, double* d_costs, double* h_report, void* stream) {
    using namespace gem;
    if (n_frames < 1 || n_frames > SC_MAX_FRAMES || lag < 1 || n_chunks < 1 || n_chunks > (1 << 20) || n_joints < 1 || n_joints > 64 ||
        min_pairs < 0 || !(tau > 0.0) || !std::isfinite(tau)) {
        set_error("gem_slam_scale: need 1 <= n_frames <= 2^24, lag >= 1, 1 .. 2^20 chunks, 1 .. 64 joints, min_pairs >= 0 and a positive tau");
        return 1;
    }
    if (!h_chunks || !d_chunks || !h_feet || !d_rot || !d_trans || !d_ids || !d_work || !d_report) { set_error("gem_slam_scale: null argument"); return 1; }
    for (int i = 0; i < 4; ++i)
        if (h_feet[i] < 0 || h_feet[i] >= n_joints) { set_error("gem_slam_scale: a foot joint outside the skeleton"); return 1; }
    const int64_t* start = h_chunks + n_chunks;
    bool ok = start[0] == 0 && start[n_chunks] == n_frames;
    for (int k = 0; k < n_chunks && ok; ++k) ok = start[k + 1] >= start[k] && (start[k + 1] == start[k] || (h_chunks[k] != 0 && (h_chunks[k] & 7) == 0));
    if (!ok) { set_error("gem_slam_scale: the chunks' first rows must rise from 0 to n_frames, and every chunk with frames needs an 8-byte aligned address"); return 1; }
    if ((reinterpret_cast<uintptr_t>(d_work) | reinterpret_cast<uintptr_t>(d_report) | reinterpret_cast<uintptr_t>(d_costs) |
         reinterpret_cast<uintptr_t>(d_rot) | reinterpret_cast<uintptr_t>(d_trans) | reinterpret_cast<uintptr_t>(d_ids) |
         reinterpret_cast<uintptr_t>(d_chunks)) & 7) { set_error("gem_slam_scale: device arrays must be 8-byte aligned"); return 1; }
    if (n_frames <= lag) {          // decided here: no grid of zero workgroups is ever launched
        set_error("gem_slam_scale: no pairs: " + std::to_string(n_frames) + " frames cannot hold two that are " + std::to_string(lag) + " apart");
        return GEM_SCALE_NO_PAIRS;
    }
    int64_t off[7];
    const int64_t need = scale_work_doubles(n_frames, lag, n_chunks, off) * (int64_t)sizeof(double);
    if (work_bytes < need) { set_error("gem_slam_scale: d_work holds " + std::to_string(work_bytes) + " bytes, " + std::to_string(need) + " are needed"); return 1; }
    ScaleArgs a;
    a.chunks = d_chunks; a.rot = d_rot; a.trans = d_trans; a.ids = d_ids;
    a.n_chunks = n_chunks; a.J = n_joints; a.N = (int)n_frames; a.P = (int)(n_frames - lag); a.lag = lag; a.min_pairs = min_pairs;
    a.nb = (a.P + SC_THREADS - 1) / SC_THREADS; a.n_tiles = (a.P + SC_TILE - 1) / SC_TILE;
    for (int i = 0; i < 4; ++i) a.feet[i] = h_feet[i];
    a.tau = tau; a.tau2 = tau * tau;
    double* w = static_cast<double*>(d_work);
    a.q = w + off[0]; a.pair = w + off[1]; a.flag = reinterpret_cast<int*>(w + off[2]); a.part = w + off[3]; a.sums = w + off[4];
    a.tile_cost = w + off[5]; a.costs = w + off[6];
    a.report = d_report; a.out_costs = d_costs;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(scale_feet_kernel, dim3((unsigned)((2 * a.N + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, s, a);
    GEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(scale_pairs_kernel, dim3((unsigned)a.nb), dim3(SC_THREADS), 0, s, a);
    GEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(scale_ref_kernel, dim3(1), dim3(64), 0, s, a);
    GEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(scale_cost_kernel, dim3((unsigned)a.n_tiles), dim3(SC_COST_THREADS), 0, s, a);
    GEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(scale_argmin_kernel, dim3(1), dim3(SC_THREADS), 0, s, a);
    GEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(scale_fit_kernel, dim3(1), dim3(SC_FIT_THREADS), 0, s, a);
    GEM_HIP(hipGetLastError());
    if (!h_report) return 0;
    GEM_HIP(hipMemcpyAsync(h_report, d_report, (GEM_SCALE_REPORT_DOUBLES + 3 * (size_t)n_chunks) * sizeof(double), hipMemcpyDeviceToHost, s));
    GEM_HIP(hipStreamSynchronize(s));
    const int status = (int)h_report[11];
    if (status == 0) return 0;
    const std::string counts = std::to_string((long long)h_report[4]) + " pairs, " + std::to_string((long long)h_report[5]) + " inliers, " +
                               std::to_string((long long)h_report[6]) + " informative";
    if (status == GEM_SCALE_NO_PAIRS) set_error("gem_slam_scale: no pairs of frames " + std::to_string(lag) + " apart with a camera translation between them (" + counts + ")");
    else if (status == GEM_SCALE_BAD_SCALE) set_error("gem_slam_scale: the fitted scale is not a positive number (" + counts + ")");
    else set_error("gem_slam_scale: the wearer did not walk enough to fix the scale: " + counts + ", " + std::to_string(min_pairs) + " informative pairs are needed");
    return status;
}

}  // extern "C"
