// A SLAM scale that drifts within a recording, followed from foot contacts, and the camera track in metres.
// Included from errors.hip behind slam_scale.h, whose foot-point, pair, candidate and fit kernels give the start value.
//
//   gem_slam_drift_work  bytes of scratch a call needs (no GPU)
//   gem_slam_drift       the global estimate -> four rounds of (assembly, solve) -> the final statistics -> the metric track
//
// The scale is piecewise linear over K knots `knot` frames apart.  Pair p (first row t) lives at ids[t] + lag / 2, in interval
// k_p with fraction u_p; all of that is integer arithmetic on 2 (tau - A), so the twin and the device place every pair alike.
// Everything is float64 without fused multiply-adds and every sum has a fixed order; there are no floating-point atomics.
//
//   drift_init_kernel      s_k = the global scale; the global verdict is copied so that a refused call writes no output
//   drift_assemble_kernel  one workgroup per interval: the pairs are ordered by their first row, so an interval's pairs are one
//                          run of the pair table, found by binary search over the frame ids; nine sums per interval (the five of
//                          the normal equations, sum <b,b>, count, informative count, squared residuals), per-lane partial sums in
//                          pair order, DPP wavefront sums, the wavefronts in order
//   drift_solve_kernel     ONE workgroup: the five bands in LDS (5 K doubles, 80 KB at 2048 knots), lambda D^T D added, then one
//                          thread factors L D L^T and substitutes in index order; a pivot that is not positive and finite keeps
//                          the previous curve and sets GEM_DRIFT_NOT_SOLVED
//   drift_steps_kernel     a block of 256 rows: the scaled steps and their inclusive scan in LDS (Hillis-Steele: the order is
//                          the block size's), the block's total and its two path lengths
//   drift_finish_kernel    ONE workgroup: the blocks' totals in order -> every block's offset; the report and the knot table
//   drift_offset_kernel    adds its block's offset to every row behind the first block
#pragma once
#include "slam_scale.h"

namespace gem {

constexpr int DR_THREADS = 256;
constexpr int DR_ROUNDS = 4;
constexpr int DR_SUMS = 9;          // A_kk, A_k,k+1, A_k+1,k+1, g_k, g_k+1, sum <b,b>, count, informative, squared residuals
constexpr int DR_MAX_KNOTS = GEM_DRIFT_MAX_KNOTS;

struct DriftArgs {
    ScaleArgs sc;
    const double* scale_report;   // the global estimate's record
    int K, knot;
    int64_t first_id;
    double stiffness;
    int n_blocks;
    double* curve;                // [K]
    double* sums;                 // [K-1, DR_SUMS]
    double* block_tot;            // [n_blocks, 5]: the block's summed step, its metric and its SLAM path length
    double* block_off;            // [n_blocks, 3]
    double* misc;                 // [8]: global status, drift status, lambda, first bad pivot, intervals with a moving camera
    double* knots;                // [K,4] out
    double* metric;               // [N,3] out
    double* report;               // [16] out
};

// interval and fraction of the time whose doubled distance from the first knot is m2
__device__ __forceinline__ int dr_place(int64_t m2, int knot, int K, double* u) {
    const int64_t two = 2 * (int64_t)knot;
    int64_t k = m2 / two;
    k = k < 0 ? 0 : (k > K - 2 ? K - 2 : k);
    *u = (double)(m2 - two * k) / (double)two;
    return (int)k;
}
__device__ __forceinline__ double dr_curve(const double* s, int k, double u) {
#pragma clang fp contract(off)
    return (1.0 - u) * s[k] + u * s[k + 1];
}

__global__ __launch_bounds__(DR_THREADS) void drift_init_kernel(DriftArgs a) {
    const double s = a.scale_report[0];
    for (int k = threadIdx.x; k < a.K; k += DR_THREADS) a.curve[k] = s;
    if (threadIdx.x == 0) {
        a.misc[0] = a.scale_report[11]; a.misc[1] = 0.0; a.misc[2] = 0.0; a.misc[3] = -1.0; a.misc[4] = 0.0;
    }
}

// the first pair row in [0, P] whose time lies at or behind the left end of interval k (k = K - 1: P)
__device__ __forceinline__ int dr_run_start(const DriftArgs& a, int k) {
    if (k <= 0) return 0;
    if (k >= a.K - 1) return a.sc.P;
    const int64_t want = 2 * (int64_t)a.knot * k;
    int lo = 0, hi = a.sc.P;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (2 * (a.sc.ids[mid] - a.first_id) + a.sc.lag >= want) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(DR_THREADS) void drift_assemble_kernel(DriftArgs a) {
    __shared__ double red[DR_THREADS / 64][DR_SUMS];
    const int tid = threadIdx.x, k = blockIdx.x;
    const int p0 = dr_run_start(a, k), p1 = dr_run_start(a, k + 1);
    const double s0 = a.curve[k], s1 = a.curve[k + 1];
    double v[DR_SUMS];
    for (int c = 0; c < DR_SUMS; ++c) v[c] = 0.0;
    for (int p = p0 + tid; p < p1; p += DR_THREADS) {
        double u;
        (void)dr_place(2 * (a.sc.ids[p] - a.first_id) + a.sc.lag, a.knot, a.K, &u);
        ScPair q;
        {
#pragma clang fp contract(off)
            const double w0 = 1.0 - u, w1 = u, sp = w0 * s0 + w1 * s1;
            if (!sc_pair_at(a.sc, p, sp, &q) || !q.inl) continue;
            v[0] += w0 * w0 * q.bb; v[1] += w0 * w1 * q.bb; v[2] += w1 * w1 * q.bb;
            v[3] += w0 * q.ab; v[4] += w1 * q.ab;
            v[5] += q.bb; v[6] += 1.0; v[8] += q.rs;
            if (sp * q.nb > a.sc.tau) v[7] += 1.0;
        }
    }
    sc_block_sum<DR_THREADS / 64, DR_SUMS>(v, red, tid);
    if (tid < DR_SUMS) a.sums[(size_t)k * DR_SUMS + tid] = v[tid];
}

__global__ __launch_bounds__(DR_THREADS) void drift_solve_kernel(DriftArgs a) {
    extern __shared__ double dr_lds[];          // M0 -> d, M1 -> e1 / l1, M2 -> l2, rhs -> y -> s, and the diagonal count of D^T D
    __shared__ double lam_s;
    const int tid = threadIdx.x, K = a.K;
    double *M0 = dr_lds, *M1 = dr_lds + K, *M2 = dr_lds + 2 * K, *rh = dr_lds + 3 * K, *L1 = dr_lds + 4 * K;
    if (tid == 0) {
#pragma clang fp contract(off)
        double tot = 0.0;
        int informed = 0;
        for (int j = 0; j < K - 1; ++j) { tot += a.sums[(size_t)j * DR_SUMS + 5]; informed += a.sums[(size_t)j * DR_SUMS + 5] > 0.0 ? 1 : 0; }
        lam_s = a.stiffness * tot / (double)(K - 1);
        a.misc[2] = lam_s; a.misc[4] = (double)informed;
    }
    __syncthreads();
    const double lam = lam_s;
    for (int k = tid; k < K; k += DR_THREADS) {
#pragma clang fp contract(off)
        // D^T D of the second differences at rows 1 .. K - 2
        double d0 = 0.0, d1 = 0.0, d2 = 0.0;
        for (int j = k - 1; j <= k + 1; ++j)
            if (j >= 1 && j <= K - 2) d0 += j == k ? 4.0 : 1.0;
        if (k >= 1 && k <= K - 2) d1 += -2.0;
        if (k + 1 >= 1 && k + 1 <= K - 2) d1 += -2.0;
        if (k + 1 >= 1 && k + 1 <= K - 2) d2 = 1.0;
        double m0 = 0.0, g0 = 0.0;
        if (k > 0) { m0 = m0 + a.sums[(size_t)(k - 1) * DR_SUMS + 2]; g0 = g0 + a.sums[(size_t)(k - 1) * DR_SUMS + 4]; }
        if (k < K - 1) { m0 = m0 + a.sums[(size_t)k * DR_SUMS + 0]; g0 = g0 + a.sums[(size_t)k * DR_SUMS + 3]; }
        M0[k] = m0 + lam * d0;
        rh[k] = -g0;
        M1[k] = k < K - 1 ? a.sums[(size_t)k * DR_SUMS + 1] + lam * d1 : 0.0;
        M2[k] = k < K - 2 ? lam * d2 : 0.0;
        L1[k] = 0.0;
    }
    __syncthreads();
    if (tid == 0) {
#pragma clang fp contract(off)
        int bad = -1;
        bool enough = K == 2 || a.misc[4] >= 2.0;
        // L D L^T in index order.  M2[i-2] and M1[i-1] hold the matrix until row i has used them; d overwrites M0, l1 goes to L1
        // and l2 overwrites M2 one row late (M2[i-2] is read by row i alone)
        for (int i = 0; i < K && enough && bad < 0; ++i) {
            const double e2 = i >= 2 ? M2[i - 2] : 0.0;
            const double l2 = i >= 2 ? e2 / M0[i - 2] : 0.0;
            double e1 = 0.0;
            if (i >= 2) e1 = M1[i - 1] - l2 * (L1[i - 1] * M0[i - 2]);
            else if (i == 1) e1 = M1[0];
            const double l1 = i >= 1 ? e1 / M0[i - 1] : 0.0;
            const double d = M0[i] - l1 * e1 - l2 * e2;
            if (!(isfinite(d) && d > 0.0)) { bad = i; break; }
            M0[i] = d; L1[i] = l1;
            if (i >= 2) M2[i - 2] = l2;
        }
        if (!enough || bad >= 0) {
            if (a.misc[1] == 0.0) { a.misc[1] = (double)GEM_DRIFT_NOT_SOLVED; a.misc[3] = (double)bad; }
        } else {
            for (int i = 0; i < K; ++i) {
                double v = rh[i];
                if (i >= 1) v = v - L1[i] * rh[i - 1];
                if (i >= 2) v = v - M2[i - 2] * rh[i - 2];
                rh[i] = v;
            }
            for (int i = K - 1; i >= 0; --i) {
                double v = rh[i] / M0[i];
                if (i + 1 < K) v = v - L1[i + 1] * rh[i + 1];
                if (i + 2 < K) v = v - M2[i] * rh[i + 2];
                rh[i] = v;
            }
        }
    }
    __syncthreads();
    if (a.misc[1] == 0.0)
        for (int k = tid; k < K; k += DR_THREADS) a.curve[k] = rh[k];
}

__global__ __launch_bounds__(DR_THREADS) void drift_steps_kernel(DriftArgs a) {
    __shared__ double scan[2][3][DR_THREADS];
    __shared__ double red[DR_THREADS / 64][2];
    const int tid = threadIdx.x, i = blockIdx.x * DR_THREADS + tid;
    const bool live = a.misc[0] == 0.0 && a.misc[1] == 0.0;
    double st[3] = {0.0, 0.0, 0.0}, len[2] = {0.0, 0.0};
    if (i >= 1 && i < a.sc.N) {
#pragma clang fp contract(off)
        double u;
        const int k = dr_place(a.sc.ids[i - 1] + a.sc.ids[i] - 2 * a.first_id, a.knot, a.K, &u);
        const double s = dr_curve(a.curve, k, u);
        double dc[3];
        for (int c = 0; c < 3; ++c) { dc[c] = a.sc.trans[(size_t)i * 3 + c] - a.sc.trans[(size_t)(i - 1) * 3 + c]; st[c] = s * dc[c]; }
        const double l = sqrt(sc_dot(dc, dc));
        len[0] = s * l; len[1] = l;
    }
    for (int c = 0; c < 3; ++c) scan[0][c][tid] = st[c];
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < DR_THREADS; off <<= 1) {
        for (int c = 0; c < 3; ++c) scan[cur ^ 1][c][tid] = tid >= off ? scan[cur][c][tid - off] + scan[cur][c][tid] : scan[cur][c][tid];
        cur ^= 1;
        __syncthreads();
    }
    if (live && i < a.sc.N)
        for (int c = 0; c < 3; ++c) a.metric[(size_t)i * 3 + c] = scan[cur][c][tid];
    if (tid < 3) a.block_tot[(size_t)blockIdx.x * 5 + tid] = scan[cur][tid][DR_THREADS - 1];
    sc_block_sum<DR_THREADS / 64, 2>(len, red, tid);
    if (tid < 2) a.block_tot[(size_t)blockIdx.x * 5 + 3 + tid] = len[tid];
}

__global__ __launch_bounds__(DR_THREADS) void drift_finish_kernel(DriftArgs a) {
    __shared__ double tot[5];
    const int tid = threadIdx.x, K = a.K;
    if (tid < 5) {
        double t = 0.0;
        for (int b = 0; b < a.n_blocks; ++b) {
            if (tid < 3) a.block_off[(size_t)b * 3 + tid] = t;
            t += a.block_tot[(size_t)b * 5 + tid];
        }
        tot[tid] = t;
    }
    __syncthreads();
    const bool accepted = a.misc[0] == 0.0;
    if (accepted)
        for (int k = tid; k < K; k += DR_THREADS) {
            double* o = a.knots + (size_t)k * 4;
            o[0] = a.curve[k];
            o[1] = k < K - 1 ? a.sums[(size_t)k * DR_SUMS + 6] : 0.0;
            o[2] = k < K - 1 ? a.sums[(size_t)k * DR_SUMS + 5] : 0.0;
            o[3] = 0.0;
        }
    if (tid == 0) {
        double inl = 0.0, info = 0.0, rss = 0.0, lo = a.curve[0], hi = a.curve[0];
        for (int j = 0; j < K - 1; ++j) { inl += a.sums[(size_t)j * DR_SUMS + 6]; info += a.sums[(size_t)j * DR_SUMS + 7]; rss += a.sums[(size_t)j * DR_SUMS + 8]; }
        for (int k = 1; k < K; ++k) { lo = a.curve[k] < lo ? a.curve[k] : lo; hi = a.curve[k] > hi ? a.curve[k] : hi; }
        double* o = a.report;
        o[0] = a.misc[0] != 0.0 ? a.misc[0] : a.misc[1];
        o[1] = (double)K; o[2] = (double)a.knot; o[3] = a.stiffness; o[4] = inl; o[5] = info; o[6] = sqrt(rss / inl);
        o[7] = lo; o[8] = hi; o[9] = tot[3] / tot[4]; o[10] = tot[3]; o[11] = tot[4]; o[12] = a.misc[2]; o[13] = (double)a.first_id;
        o[14] = a.misc[3]; o[15] = a.misc[4];
    }
}

__global__ __launch_bounds__(DR_THREADS) void drift_offset_kernel(DriftArgs a) {
    const int i = (blockIdx.x + 1) * DR_THREADS + threadIdx.x;          // (the first block's offset is zero: its rows stay as they are)
    if (!(a.misc[0] == 0.0 && a.misc[1] == 0.0) || i >= a.sc.N) return;
    for (int c = 0; c < 3; ++c) a.metric[(size_t)i * 3 + c] = a.block_off[(size_t)(blockIdx.x + 1) * 3 + c] + a.metric[(size_t)i * 3 + c];
}

inline int64_t drift_work_doubles(int64_t N, int lag, int K, int64_t* off) {
    const int64_t nblk = (N + DR_THREADS - 1) / DR_THREADS;
    int64_t at = scale_work_doubles(N, lag, 1, nullptr);
    const int64_t sizes[5] = {K, (int64_t)(K - 1) * DR_SUMS, nblk * 5, nblk * 3, 8};      // curve, sums, block_tot, block_off, misc
    for (int i = 0; i < 5; ++i) { if (off) off[i] = at; at += sizes[i]; }
    return at;
}

inline int64_t drift_knot_count(int64_t first_id, int64_t last_id, int knot) {
    const int64_t span = last_id - first_id, k = (span + knot - 1) / knot + 1;
    return k < 2 ? 2 : k;
}

}  // namespace gem

extern "C" {

int64_t gem_slam_drift_work(int64_t n_frames, int lag, int n_knots) {
    using namespace gem;
    if (n_frames < 1 || n_frames > SC_MAX_FRAMES || lag < 1 || n_knots < 2 || n_knots > DR_MAX_KNOTS) {
        set_error("gem_slam_drift_work: need 1 <= n_frames <= 2^24, lag >= 1 and 2 <= n_knots <= " + std::to_string(DR_MAX_KNOTS)); return -1;
    }
    if (n_frames <= lag) return 8;          // (nothing is launched for such a call)
    return drift_work_doubles(n_frames, lag, n_knots, nullptr) * (int64_t)sizeof(double);
}

int gem_slam_drift(const int64_t* h_chunks, const int64_t* d_chunks, int n_chunks, int n_joints, const int* h_feet, const double* d_rot,
                   const double* d_trans, const int64_t* d_ids, int64_t n_frames, int64_t first_id, int64_t last_id, int lag, double tau,
                   int min_pairs, int knot, double stiffness, void* d_work, int64_t work_bytes, double* d_scale_report, double* d_costs,
                   double* d_knots, double* d_metric, double* d_report, double* h_scale_report, double* h_knots, double* h_metric,
                   double* h_report, void* stream) {
    using namespace gem;
    if (!d_knots || !d_metric || !d_report || !d_scale_report) { set_error("gem_slam_drift: null output (d_scale_report, d_knots, d_metric and d_report are needed)"); return 1; }
    if (!h_report && (h_scale_report || h_knots || h_metric)) { set_error("gem_slam_drift: host copies need h_report, which carries the verdict"); return 1; }
    if (lag < 1 || knot < lag + 1) { set_error("gem_slam_drift: knot = " + std::to_string(knot) + " frames, at least lag + 1 = " + std::to_string((long long)lag + 1) + " are needed"); return 1; }
    if (!(stiffness >= 0.0) || !std::isfinite(stiffness)) { set_error("gem_slam_drift: stiffness must be a finite number >= 0"); return 1; }
    if (n_frames >= 1 && (last_id < first_id || last_id - first_id > ((int64_t)1 << 40))) { set_error("gem_slam_drift: the frame ids must rise from first_id to last_id"); return 1; }
    const int64_t K64 = n_frames >= 1 ? drift_knot_count(first_id, last_id, knot) : 2;
    if (K64 > DR_MAX_KNOTS) {
        set_error("gem_slam_drift: too many knots: " + std::to_string(K64) + " at " + std::to_string(knot) + " frames apart, at most " + std::to_string(DR_MAX_KNOTS) + " are possible");
        return 1;
    }
    if ((reinterpret_cast<uintptr_t>(d_knots) | reinterpret_cast<uintptr_t>(d_metric) | reinterpret_cast<uintptr_t>(d_report) |
         reinterpret_cast<uintptr_t>(d_scale_report)) & 7) { set_error("gem_slam_drift: device arrays must be 8-byte aligned"); return 1; }
    if (n_frames >= 1 && n_frames <= SC_MAX_FRAMES && n_frames > lag && d_work) {
        const int64_t need = drift_work_doubles(n_frames, lag, (int)K64, nullptr) * (int64_t)sizeof(double);
        if (work_bytes < need) { set_error("gem_slam_drift: d_work holds " + std::to_string(work_bytes) + " bytes, " + std::to_string(need) + " are needed"); return 1; }
    }
    // the global estimate: gem_slam_scale's own checks and kernels, enqueued only
    const int rc = gem_slam_scale(h_chunks, d_chunks, n_chunks, n_joints, h_feet, d_rot, d_trans, d_ids, n_frames, lag, tau, min_pairs, d_work,
                                  work_bytes, d_scale_report, d_costs, nullptr, stream);
    if (rc) return rc;
    int64_t soff[7], off[5];
    scale_work_doubles(n_frames, lag, n_chunks, soff);
    drift_work_doubles(n_frames, lag, (int)K64, off);
    DriftArgs a;
    ScaleArgs& sc = a.sc;
    sc.chunks = d_chunks; sc.rot = d_rot; sc.trans = d_trans; sc.ids = d_ids;
    sc.n_chunks = n_chunks; sc.J = n_joints; sc.N = (int)n_frames; sc.P = (int)(n_frames - lag); sc.lag = lag; sc.min_pairs = min_pairs;
    sc.nb = (sc.P + SC_THREADS - 1) / SC_THREADS; sc.n_tiles = (sc.P + SC_TILE - 1) / SC_TILE;
    for (int i = 0; i < 4; ++i) sc.feet[i] = h_feet[i];
    sc.tau = tau; sc.tau2 = tau * tau;
    double* w = static_cast<double*>(d_work);
    sc.q = w + soff[0]; sc.pair = w + soff[1]; sc.flag = reinterpret_cast<int*>(w + soff[2]); sc.part = w + soff[3]; sc.sums = w + soff[4];
    sc.tile_cost = w + soff[5]; sc.costs = w + soff[6];
    sc.report = d_scale_report; sc.out_costs = d_costs;
    a.scale_report = d_scale_report; a.K = (int)K64; a.knot = knot; a.first_id = first_id; a.stiffness = stiffness;
    a.n_blocks = (int)((n_frames + DR_THREADS - 1) / DR_THREADS);
    a.curve = w + off[0]; a.sums = w + off[1]; a.block_tot = w + off[2]; a.block_off = w + off[3]; a.misc = w + off[4];
    a.knots = d_knots; a.metric = d_metric; a.report = d_report;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = 5 * (size_t)a.K * sizeof(double);
    static PerDeviceOnce once;
    int device = -1;
    GEM_HIP(hipGetDevice(&device));
    if (once.need(device))
        GEM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(drift_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    5 * DR_MAX_KNOTS * (int)sizeof(double)));
    hipLaunchKernelGGL(drift_init_kernel, dim3(1), dim3(DR_THREADS), 0, s, a);
    GEM_HIP(hipGetLastError());
    for (int round = 0; round <= DR_ROUNDS; ++round) {
        hipLaunchKernelGGL(drift_assemble_kernel, dim3((unsigned)(a.K - 1)), dim3(DR_THREADS), 0, s, a);
        GEM_HIP(hipGetLastError());
        if (round == DR_ROUNDS) break;
        hipLaunchKernelGGL(drift_solve_kernel, dim3(1), dim3(DR_THREADS), lds, s, a);
        GEM_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(drift_steps_kernel, dim3((unsigned)a.n_blocks), dim3(DR_THREADS), 0, s, a);
    GEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(drift_finish_kernel, dim3(1), dim3(DR_THREADS), 0, s, a);
    GEM_HIP(hipGetLastError());
    if (a.n_blocks > 1) {
        hipLaunchKernelGGL(drift_offset_kernel, dim3((unsigned)(a.n_blocks - 1)), dim3(DR_THREADS), 0, s, a);
        GEM_HIP(hipGetLastError());
    }
    if (!h_report) return 0;
    GEM_HIP(hipMemcpyAsync(h_report, d_report, GEM_DRIFT_REPORT_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, s));
    if (h_scale_report) GEM_HIP(hipMemcpyAsync(h_scale_report, d_scale_report, (GEM_SCALE_REPORT_DOUBLES + 3 * (size_t)n_chunks) * sizeof(double), hipMemcpyDeviceToHost, s));
    if (h_knots) GEM_HIP(hipMemcpyAsync(h_knots, d_knots, 4 * (size_t)a.K * sizeof(double), hipMemcpyDeviceToHost, s));
    if (h_metric) GEM_HIP(hipMemcpyAsync(h_metric, d_metric, 3 * (size_t)n_frames * sizeof(double), hipMemcpyDeviceToHost, s));
    GEM_HIP(hipStreamSynchronize(s));
    const int status = (int)h_report[0];
    if (status == 0) return 0;
    if (status == GEM_DRIFT_NOT_SOLVED) {
        set_error("gem_slam_drift: the recording does not fix the scale curve: " + std::to_string((long long)h_report[15]) + " of " +
                  std::to_string(a.K - 1) + " knot intervals hold inlier pairs with a moving camera" +
                  (h_report[14] >= 0.0 ? ", pivot " + std::to_string((long long)h_report[14]) + " is not positive" : std::string()));
        return status;
    }
    // the global estimate's refusals, with its text and counts: read its record
    double head[GEM_SCALE_REPORT_DOUBLES];
    GEM_HIP(hipMemcpy(head, d_scale_report, sizeof(head), hipMemcpyDeviceToHost));
    const std::string counts = std::to_string((long long)head[4]) + " pairs, " + std::to_string((long long)head[5]) + " inliers, " +
                               std::to_string((long long)head[6]) + " informative";
    if (status == GEM_SCALE_NO_PAIRS) set_error("gem_slam_scale: no pairs of frames " + std::to_string(lag) + " apart with a camera translation between them (" + counts + ")");
    else if (status == GEM_SCALE_BAD_SCALE) set_error("gem_slam_scale: the fitted scale is not a positive number (" + counts + ")");
    else set_error("gem_slam_scale: the wearer did not walk enough to fix the scale: " + counts + ", " + std::to_string(min_pairs) + " informative pairs are needed");
    return status;
}

}  // extern "C"
