// The ground plane of a pose sequence from its foot contacts, the foot figures and the upright transform.
// Included from errors.hip.
//
//   gem_ground_plane_work    the work-buffer offsets of the sequences too long for LDS, and the bytes they need (no GPU)
//   gem_ground_plane         a table of sequences -> one 48-double record each, ONE launch, a workgroup of 1024 per sequence
//   gem_similarity_compose   (c, R, t) records a, then b -> one record
//
// A foot that stands does not move, and the places where the feet stand lie on the floor.  q[f,side] = (ankle + foot) / 2; foot point
// (f, side) is a CANDIDATE when |q[f+lag] - q[f]| < tau_v.  The plane: centroid and scatter of the candidates, the normal the
// singular vector of the smallest singular value (svd3 on the symmetric scatter), its sign the body's; four rounds of refit on the
// candidates within tau_h of the plane.  Where the candidates span no plane the normal is the body's direction and the offset the
// candidates' height along it (from their lower median, four rounds of refit); where there are too few, the offset is the lowest
// foot point.  Then the foot figures over all frames and the rigid transform into the upright frame.  tests/ground_twin.py is the
// specification, step for step.
//
// Everything is float64.  A sequence's foot points (48 bytes per frame) are kept in LDS up to GEM_GROUND_LDS_FRAMES frames (48 KB);
// a longer sequence keeps them in its part of the work buffer and every pass reads them from there, with the same arithmetic.  The
// candidates are not stored: a pass tests the pair again (six loads and a square root).  Every sum has a fixed order -- a thread's
// points in order, DPP wavefront sums, the sixteen wavefronts in order (block_sums) -- and there are no floating-point atomics:
// two calls give the same bytes.  The lower median is found exactly, by a radix selection over the heights' bit patterns: 64 counting
// passes.
#pragma once
#include "umeyama_device.h"
#include <cmath>

namespace gem {

constexpr int GR_LDS_FRAMES = GEM_GROUND_LDS_FRAMES;
constexpr int GR_REC = GEM_GROUND_RECORD_DOUBLES;
constexpr int GR_MAX_FRAMES = 1 << 24;
constexpr int GR_ROUNDS = 4;
constexpr int GR_J = 15, GR_NECK = 0, GR_RHIP = 7, GR_LHIP = 11;
static_assert(GR_LDS_FRAMES * 48 + 2 * 16 * ERR_NW * 8 + 256 <= 64 * 1024, "the foot points and the sums' partials fit a workgroup's static LDS");

struct GroundArgs {
    const int64_t* table;      // device: [n] sequence addresses, [n] frames, [n] addresses of a (c, R, t) applied first or 0, [n] work offsets (doubles) or -1
    int n, lag, min_points;
    double tau_v, tau_h, min_spread, foot_height;
    double* work;
    double* rec;               // [n, GR_REC]
};

__device__ __forceinline__ double gr_dot(const double* u, const double* v) {
#pragma clang fp contract(off)
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
}

// whether foot point i = 2 f + side is a candidate: the earlier frame of a still pair
__device__ __forceinline__ bool gr_candidate(const double* q, int i, int F, int lag, double tau_v) {
#pragma clang fp contract(off)
    if ((i >> 1) + lag >= F) return false;
    const double* a = q + (size_t)i * 3;
    const double* b = q + (size_t)(i + 2 * lag) * 3;
    const double d0 = b[0] - a[0], d1 = b[1] - a[1], d2 = b[2] - a[2];
    return sqrt(d0 * d0 + d1 * d1 + d2 * d2) < tau_v;
}

// whether foot point i = 2 f + side is in contact: a candidate within tau_h of the plane (n, d)
__device__ __forceinline__ bool gr_contact(const double* q, int i, int F, int lag, double tau_v, double tau_h, const double* n, double d) {
    return gr_candidate(q, i, F, lag, tau_v) && fabs(gr_dot(q + (size_t)i * 3, n) - d) < tau_h;
}

// the workgroup's largest value, in every thread (NaN wins); two barriers
__device__ inline double gr_block_max(double v, double* mx) {
    const double w = wave_max_dpp(v);
    if ((threadIdx.x & 63) == 0) mx[threadIdx.x >> 6] = w;
    __syncthreads();
    double t = mx[0];
    for (int i = 1; i < ERR_NW; ++i) t = nan_max(t, mx[i]);
    __syncthreads();
    return t;
}

// a double's bits as an unsigned number that orders as the double does
__device__ __forceinline__ unsigned long long gr_key(double h) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(h);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double gr_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// centroid and scatter of the candidates (every one, or those within tau_h of the plane (n, d)), then the plane through them:
// -> the count; with at least min_points of them m, lam (unsorted singular values), n and d are replaced
__device__ inline double gr_fit(const double* q, int F, const GroundArgs& a, bool inliers_only, const double* u0, double* red, int& parity,
                                double* n, double& d, double* lam) {
    const int tid = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < 2 * F; i += ERR_ST) {
        if (!gr_candidate(q, i, F, a.lag, a.tau_v)) continue;
        const double* p = q + (size_t)i * 3;
        if (inliers_only && !(fabs(gr_dot(n, p) - d) < a.tau_h)) continue;
        s[0] += 1.0; s[1] += p[0]; s[2] += p[1]; s[3] += p[2];
    }
    block_sums<4>(s, red, parity);
    if (s[0] < (double)a.min_points) return s[0];
    const double m[3] = {s[1] / s[0], s[2] / s[0], s[3] / s[0]};
    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};          // xx xy xz yy yz zz
    for (int i = tid; i < 2 * F; i += ERR_ST) {
        if (!gr_candidate(q, i, F, a.lag, a.tau_v)) continue;
        const double* p = q + (size_t)i * 3;
        if (inliers_only && !(fabs(gr_dot(n, p) - d) < a.tau_h)) continue;
        const double e0 = p[0] - m[0], e1 = p[1] - m[1], e2 = p[2] - m[2];
        c[0] += e0 * e0; c[1] += e0 * e1; c[2] += e0 * e2; c[3] += e1 * e1; c[4] += e1 * e2; c[5] += e2 * e2;
    }
    block_sums<6>(c, red, parity);
    for (int k = 0; k < 6; ++k) c[k] /= s[0];
    const double S[9] = {c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]};
    double U[9], V[9];
    svd3(S, U, lam, V);
    int kmin = 0;
    for (int k = 1; k < 3; ++k)
        if (lam[k] < lam[kmin]) kmin = k;
    double nn[3] = {V[kmin], V[3 + kmin], V[6 + kmin]};
    const double len = sqrt(gr_dot(nn, nn));
    const double sign = gr_dot(nn, u0) < 0.0 ? -1.0 : 1.0;
    for (int k = 0; k < 3; ++k) n[k] = sign * nn[k] / len;
    d = gr_dot(n, m);
    return s[0];
}

__global__ __launch_bounds__(ERR_ST) void ground_plane_kernel(GroundArgs a) {
    __shared__ double qs[GR_LDS_FRAMES * 6];
    __shared__ double red[2 * 16 * ERR_NW];
    __shared__ double mx[ERR_NW];
    const int tid = threadIdx.x, seq = blockIdx.x;
    int parity = 0;
    double* rec = a.rec + (size_t)seq * GR_REC;
    const int64_t addr = a.table[seq], frames = a.table[a.n + seq], crt_addr = a.table[2 * a.n + seq], work_at = a.table[3 * a.n + seq];
    for (int k = tid; k < GR_REC; k += ERR_ST) rec[k] = 0.0;
    __syncthreads();
    const bool in_lds = frames <= GR_LDS_FRAMES;
    if (addr == 0 || (addr & 7) || (crt_addr & 7) || frames < 1 || frames > GR_MAX_FRAMES || (!in_lds && work_at < 0)) {
        if (tid == 0) rec[0] = (double)GEM_GROUND_BAD_SEQUENCE;
        return;
    }
    const int F = (int)frames;
    const double* x = reinterpret_cast<const double*>(addr);
    double* q = in_lds ? qs : a.work + work_at;
    double cin[13] = {1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    const bool moved = crt_addr != 0;
    if (moved)
        for (int k = 0; k < 13; ++k) cin[k] = reinterpret_cast<const double*>(crt_addr)[k];
    auto joint = [&](int f, int j, double* o) {          // c * (p . R) + t, as every writer moves a joint
        const double* p = x + ((size_t)f * GR_J + j) * 3;
        if (!moved) { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; return; }
        for (int dd = 0; dd < 3; ++dd) o[dd] = cin[0] * (p[0] * cin[1 + dd] + p[1] * cin[4 + dd] + p[2] * cin[7 + dd]) + cin[10 + dd];
    };
    // 1. foot points and body up
    double body[3] = {0.0, 0.0, 0.0};
    for (int f = tid; f < F; f += ERR_ST) {
        double ra[3], rf[3], la[3], lf[3], nk[3];
        joint(f, 9, ra); joint(f, 10, rf); joint(f, 13, la); joint(f, 14, lf); joint(f, GR_NECK, nk);
        double* o = q + (size_t)f * 6;
        {
#pragma clang fp contract(off)
            for (int dd = 0; dd < 3; ++dd) {
                o[dd] = 0.5 * (ra[dd] + rf[dd]);
                o[3 + dd] = 0.5 * (la[dd] + lf[dd]);
                body[dd] += nk[dd] - 0.5 * (o[dd] + o[3 + dd]);
            }
        }
    }
    __threadfence();          // (a long sequence's foot points lie in global memory: visible to the workgroup behind the sums' barrier)
    block_sums<3>(body, red, parity);
    double hr[3], hl[3];
    joint(0, GR_RHIP, hr); joint(0, GR_LHIP, hl);
    const double norm = sqrt(gr_dot(body, body));
    bool fine = isfinite(norm) && norm >= 1e-6 * (double)F;
    for (int dd = 0; dd < 3; ++dd) fine = fine && isfinite(hr[dd] + hl[dd]);
    if (!fine) {
        if (tid == 0) { rec[0] = (double)GEM_GROUND_NO_BODY; rec[21] = (double)F; rec[22] = (double)a.lag; }
        return;
    }
    const double u0[3] = {body[0] / norm, body[1] / norm, body[2] / norm};
    // 2. - 6. the plane
    double n[3] = {u0[0], u0[1], u0[2]}, d = 0.0, lam[3] = {0.0, 0.0, 0.0};
    double points = gr_fit(q, F, a, false, u0, red, parity, n, d, lam);
    int source = GEM_GROUND_SOURCE_BODY;
    double inliers = 0.0, rms = 0.0, spread = 0.0, extent = 0.0;
    if (points >= (double)a.min_points) {
        bool ok = true;
        for (int round = 0; round < GR_ROUNDS && ok; ++round)
            ok = gr_fit(q, F, a, true, u0, red, parity, n, d, lam) >= (double)a.min_points;
        double lo = lam[0], mid = lam[1], hi = lam[2], t;
        if (lo > mid) { t = lo; lo = mid; mid = t; }
        if (mid > hi) { t = mid; mid = hi; hi = t; }
        if (lo > mid) { t = lo; lo = mid; mid = t; }
        spread = sqrt(mid > 0.0 ? mid : 0.0); extent = sqrt(hi > 0.0 ? hi : 0.0);
        if (ok && spread >= a.min_spread) {
            source = GEM_GROUND_SOURCE_PLANE;
        } else {          // the candidates span no plane: the body's direction, the height from the candidates
            source = GEM_GROUND_SOURCE_BODY_NORMAL;
            for (int k = 0; k < 3; ++k) n[k] = u0[k];
            // the lower median of the heights: the value of rank (points - 1) / 2, bit by bit from the top
            double rank = floor((points - 1.0) * 0.5);
            unsigned long long prefix = 0ull;
            for (int bit = 63; bit >= 0; --bit) {
                double zero[1] = {0.0};
                const unsigned long long above = bit == 63 ? 0ull : (~0ull << (bit + 1));
                for (int i = tid; i < 2 * F; i += ERR_ST) {
                    if (!gr_candidate(q, i, F, a.lag, a.tau_v)) continue;
                    const unsigned long long key = gr_key(gr_dot(q + (size_t)i * 3, u0));
                    if ((key & above) == prefix && !((key >> bit) & 1ull)) zero[0] += 1.0;
                }
                block_sums<1>(zero, red, parity);
                if (!(rank < zero[0])) { rank -= zero[0]; prefix |= 1ull << bit; }
            }
            d = gr_unkey(prefix);
            for (int round = 0; round < GR_ROUNDS; ++round) {
                double s[2] = {0.0, 0.0};
                for (int i = tid; i < 2 * F; i += ERR_ST) {
                    if (!gr_candidate(q, i, F, a.lag, a.tau_v)) continue;
                    const double h = gr_dot(q + (size_t)i * 3, u0);
                    if (fabs(h - d) < a.tau_h) { s[0] += 1.0; s[1] += h; }
                }
                block_sums<2>(s, red, parity);
                if (s[0] > 0.0) d = s[1] / s[0];
            }
        }
        // 5. the final pass at the final (n, d)
        double s[2] = {0.0, 0.0};
        for (int i = tid; i < 2 * F; i += ERR_ST) {
            if (!gr_candidate(q, i, F, a.lag, a.tau_v)) continue;
            const double r = gr_dot(q + (size_t)i * 3, n) - d;
            if (fabs(r) < a.tau_h) { s[0] += 1.0; s[1] += r * r; }
        }
        block_sums<2>(s, red, parity);
        inliers = s[0];
        rms = sqrt(s[1] / (s[0] > 1.0 ? s[0] : 1.0));
    } else {          // too few candidates: the lowest foot point along the body's direction
        for (int k = 0; k < 3; ++k) n[k] = u0[k];
        double low = -INFINITY;
        for (int i = tid; i < 2 * F; i += ERR_ST) low = nan_max(low, -gr_dot(q + (size_t)i * 3, u0));
        d = -gr_block_max(low, mx);
    }
    // 7. the foot figures, over all frames
    double fig[4] = {0.0, 0.0, 0.0, 0.0};          // contact frames right, left; the skate's sum and its pairs
    double hmin = INFINITY, hmax = -INFINITY;
    for (int i = tid; i < 2 * F; i += ERR_ST) {
        const double* p = q + (size_t)i * 3;
        const double h = gr_dot(p, n) - d;
        hmin = h < hmin ? h : hmin; hmax = h > hmax ? h : hmax;
        if (!gr_contact(q, i, F, a.lag, a.tau_v, a.tau_h, n, d)) continue;
        fig[i & 1] += 1.0;
        if ((i >> 1) + 1 < F && gr_contact(q, i + 2, F, a.lag, a.tau_v, a.tau_h, n, d)) {
#pragma clang fp contract(off)
            double v[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
            const double along = gr_dot(v, n);
            for (int k = 0; k < 3; ++k) v[k] = v[k] - along * n[k];
            fig[2] += sqrt(gr_dot(v, v)); fig[3] += 1.0;
        }
    }
    block_sums<4>(fig, red, parity);
    hmin = -gr_block_max(-hmin, mx);
    hmax = gr_block_max(hmax, mx);
    if (tid != 0) return;
    // 8. the upright transform: Y = n, X the hips' left made level, Z = X x Y; frame 0's hip midpoint above the origin
    double X[3], l[3] = {hl[0] - hr[0], hl[1] - hr[1], hl[2] - hr[2]};
    double along = gr_dot(l, n);
    for (int k = 0; k < 3; ++k) X[k] = l[k] - along * n[k];
    if (sqrt(gr_dot(X, X)) < 1e-6) {
        int e = 0;
        for (int k = 1; k < 3; ++k)
            if (fabs(n[k]) < fabs(n[e])) e = k;
        for (int k = 0; k < 3; ++k) X[k] = (k == e ? 1.0 : 0.0) - n[e] * n[k];
    }
    const double xl = sqrt(gr_dot(X, X));
    for (int k = 0; k < 3; ++k) X[k] /= xl;
    const double Z[3] = {X[1] * n[2] - X[2] * n[1], X[2] * n[0] - X[0] * n[2], X[0] * n[1] - X[1] * n[0]};
    double o[3] = {0.5 * (hr[0] + hl[0]), 0.5 * (hr[1] + hl[1]), 0.5 * (hr[2] + hl[2])};
    const double off = gr_dot(o, n) - (d - a.foot_height);
    for (int k = 0; k < 3; ++k) o[k] -= off * n[k];
    rec[0] = 0.0; rec[1] = (double)source;
    for (int k = 0; k < 3; ++k) { rec[2 + k] = n[k]; rec[6 + k] = u0[k]; }
    rec[5] = d; rec[9] = gr_dot(n, u0);
    rec[10] = points; rec[11] = inliers; rec[12] = rms; rec[13] = spread; rec[14] = extent;
    rec[15] = fig[0]; rec[16] = fig[1]; rec[17] = fig[3] > 0.0 ? fig[2] / fig[3] : 0.0;
    rec[18] = hmin < 0.0 ? -hmin : 0.0; rec[19] = hmax; rec[20] = fig[3]; rec[21] = (double)F; rec[22] = (double)a.lag;
    double* crt = rec + 23;
    crt[0] = 1.0;
    for (int k = 0; k < 3; ++k) { crt[1 + 3 * k] = X[k]; crt[2 + 3 * k] = n[k]; crt[3 + 3 * k] = Z[k]; }
    crt[10] = -gr_dot(o, X); crt[11] = -gr_dot(o, n); crt[12] = -gr_dot(o, Z);
}

__global__ __launch_bounds__(64) void similarity_compose_kernel(const double* a, const double* b, double* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double A[13], B[13], o[13];
    for (int k = 0; k < 13; ++k) { A[k] = a[i * 13 + k]; B[k] = b[i * 13 + k]; }
    {
#pragma clang fp contract(off)
        o[0] = A[0] * B[0];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) o[1 + 3 * r + c] = A[1 + 3 * r] * B[1 + c] + A[2 + 3 * r] * B[4 + c] + A[3 + 3 * r] * B[7 + c];
        for (int c = 0; c < 3; ++c) o[10 + c] = B[0] * (A[10] * B[1 + c] + A[11] * B[4 + c] + A[12] * B[7 + c]) + B[10 + c];
    }
    for (int k = 0; k < 13; ++k) out[i * 13 + k] = o[k];
}

// the work offsets (doubles) of the sequences that do not fit LDS, -1 for the others; -> doubles in all
inline int64_t ground_work_doubles(const int64_t* frames, int n, int64_t* offsets) {
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        const bool big = frames[i] > GR_LDS_FRAMES && frames[i] <= GR_MAX_FRAMES;
        if (offsets) offsets[i] = big ? at : -1;
        if (big) at += 6 * frames[i];
    }
    return at;
}

}  // namespace gem

extern "C" {

int64_t gem_ground_plane_work(const int64_t* h_frames, int n_sequences, int64_t* h_offsets) {
    using namespace gem;
    if (!h_frames || n_sequences < 1 || n_sequences > (1 << 20)) { set_error("gem_ground_plane_work: need the frame counts of 1 .. 2^20 sequences"); return -1; }
    return ground_work_doubles(h_frames, n_sequences, h_offsets) * (int64_t)sizeof(double);
}

int gem_ground_plane(const int64_t* h_table, const int64_t* d_table, int n_sequences, int lag, double tau_v, double tau_h, double min_spread,
                     int min_points, double foot_height, double* d_work, int64_t work_bytes, double* d_records, void* stream) {
    using namespace gem;
    if (n_sequences < 1) { set_error("gem_ground_plane: an empty table of sequences"); return 1; }          // (no grid of zero workgroups)
    if (n_sequences > (1 << 20) || lag < 1 || min_points < 3 || !(tau_v > 0.0) || !std::isfinite(tau_v) || !(tau_h > 0.0) || !std::isfinite(tau_h) ||
        !(min_spread >= 0.0) || !std::isfinite(min_spread) || !std::isfinite(foot_height)) {
        set_error("gem_ground_plane: need at most 2^20 sequences, lag >= 1, min_points >= 3, positive finite tau_v and tau_h, a finite min_spread >= 0 and a finite foot_height");
        return 1;
    }
    if (!h_table || !d_table || !d_records) { set_error("gem_ground_plane: null argument"); return 1; }
    if ((reinterpret_cast<uintptr_t>(d_table) | reinterpret_cast<uintptr_t>(d_records) | reinterpret_cast<uintptr_t>(d_work)) & 7) {
        set_error("gem_ground_plane: device arrays must be 8-byte aligned"); return 1;
    }
    // the work offsets of the long sequences must be the ones gem_ground_plane_work gives: parts that do not overlap, inside d_work
    int64_t at = 0;
    for (int i = 0; i < n_sequences; ++i) {
        const int64_t frames = h_table[n_sequences + i], given = h_table[3 * (int64_t)n_sequences + i];
        const bool big = frames > GR_LDS_FRAMES && frames <= GR_MAX_FRAMES;
        if (given != (big ? at : -1)) { set_error("gem_ground_plane: sequence " + std::to_string(i) + ": its work offset is not the one gem_ground_plane_work gives"); return 1; }
        if (big) at += 6 * frames;
    }
    const int64_t need = at * (int64_t)sizeof(double);
    if (need > 0 && (!d_work || work_bytes < need)) {
        set_error("gem_ground_plane: d_work holds " + std::to_string(d_work ? work_bytes : 0) + " bytes, " + std::to_string(need) + " are needed"); return 1;
    }
    GroundArgs a;
    a.table = d_table; a.n = n_sequences; a.lag = lag; a.min_points = min_points;
    a.tau_v = tau_v; a.tau_h = tau_h; a.min_spread = min_spread; a.foot_height = foot_height;
    a.work = d_work; a.rec = d_records;
    hipLaunchKernelGGL(ground_plane_kernel, dim3((unsigned)n_sequences), dim3(ERR_ST), 0, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_similarity_compose(const double* d_a, const double* d_b, double* d_out, int64_t n, void* stream) {
    using namespace gem;
    if (n < 1 || n > (1 << 24)) { set_error("gem_similarity_compose: need 1 .. 2^24 records"); return 1; }
    if (!d_a || !d_b || !d_out) { set_error("gem_similarity_compose: null argument"); return 1; }
    if ((reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_b) | reinterpret_cast<uintptr_t>(d_out)) & 7) {
        set_error("gem_similarity_compose: device arrays must be 8-byte aligned"); return 1;
    }
    hipLaunchKernelGGL(similarity_compose_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), d_a, d_b, d_out, n);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
