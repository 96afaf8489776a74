// Looking at a trained motion VAE: the two device steps between the encoder / decoder and the files that
// meshes.py / render.py write.  Included from errors.hip.
//
//   gem_latent_paths   S latent points from za to zb per pair, straight (the reference's networks/interpolant.py:126, in numpy's
//                      fp32 arithmetic) or along the great circle between the two directions
//   gem_latent_report  per window: sum mu^2, sum (sigma - 1)^2 (networks/get_latent.py:57-58), the KL divergence to N(0, I), the
//                      reconstruction's mean and maximal joint distance; per latent dimension, added to the caller's accumulators
//                      over as many calls as the data set has batches: sum mu, sum mu^2, sum sigma^2
//
// Both are streaming kernels (a 2048-D batch of 256 windows is 4 MB in, 10 KB out) whose point is that the numbers stay on the
// device between the batches of a pass.  Sums are float64 in a fixed order -- a thread's strided terms in order, DPP wavefront
// sums, the wavefronts of a workgroup in order -- so two calls give the same bits; there are no floating-point atomics.
#pragma once
#include "gem_internal.h"

namespace gem {

constexpr int LT_THREADS = 256;
constexpr int LT_WAVES = LT_THREADS / 64;

// the workgroup's total of N per-thread values, the same in every thread: wavefront sums, then the wavefronts in order
template <int N>
__device__ inline void lt_block_sums(double (&v)[N], double (*red)[LT_WAVES]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const double w = wave_sum_dpp(v[c]);
        if ((tid & 63) == 0) red[c][tid >> 6] = w;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; ++c) {
        double t = red[c][0];
        for (int w = 1; w < LT_WAVES; ++w) t += red[c][w];
        v[c] = t;
    }
    __syncthreads();
}

// interpolant.py:126 on float32 arrays, `first_z + (i / (S - 1.)) * (second_z - first_z)`: numpy rounds the Python float to
// float32, then the difference, the product and the sum each once.  (The library is built with -ffp-contract=on: written as one
// expression the product and the sum would fuse.)
__device__ __forceinline__ float lt_lerp(float a, float b, float t) {
    const float d = __fsub_rn(b, a);
    const float m = __fmul_rn(t, d);
    return __fadd_rn(a, m);
}

constexpr int LT_STEPS = 256;      // steps whose coefficients are held in LDS at a time

// One workgroup per pair.  Thread tid owns the dimensions tid, tid + 256, ...: it reads a and b once and writes the S points.
__global__ __launch_bounds__(LT_THREADS) void latent_paths_kernel(const float* __restrict__ za, const float* __restrict__ zb,
                                                                  float* __restrict__ out, int D, int S, int mode) {
    __shared__ double red[3][LT_WAVES];
    __shared__ double coef[LT_STEPS][2];
    __shared__ float tf[LT_STEPS];
    const int tid = threadIdx.x;
    const size_t p = blockIdx.x;
    const float* a = za + p * D;
    const float* b = zb + p * D;
    float* o = out + p * (size_t)S * D;
    bool slerp = false;
    double omega = 0.0, sin_omega = 1.0;
    if (mode == 1) {
        double v[3] = {0.0, 0.0, 0.0};      // <a,b>, <a,a>, <b,b>
        for (int d = tid; d < D; d += LT_THREADS) {
            const double x = (double)a[d], y = (double)b[d];
            v[0] += x * y; v[1] += x * x; v[2] += y * y;
        }
        lt_block_sums<3>(v, red);
        const double na = sqrt(v[1]), nb = sqrt(v[2]);
        if (na != 0.0 && nb != 0.0) {
            double c = v[0] / (na * nb);
            c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
            omega = acos(c);
            sin_omega = sin(omega);
            slerp = sin_omega >= 1e-6;      // (parallel, opposite or NaN directions: the straight line)
        }
    }
    for (int s0 = 0; s0 < S; s0 += LT_STEPS) {
        const int ns = S - s0 < LT_STEPS ? S - s0 : LT_STEPS;
        if (tid < ns) {
            const double t = (double)(s0 + tid) / (double)(S - 1);
            tf[tid] = (float)t;
            if (slerp) {
                coef[tid][0] = sin((1.0 - t) * omega);
                coef[tid][1] = sin(t * omega);
            }
        }
        __syncthreads();
        for (int d = tid; d < D; d += LT_THREADS) {
            const float x = a[d], y = b[d];
            for (int k = 0; k < ns; ++k) {
                const int s = s0 + k;
                float r;
                if (s == 0) r = x;                      // the end points are the inputs themselves: in fp32 a + 1.0 * (b - a) is not b
                else if (s == S - 1) r = y;
                else if (slerp) {
#pragma clang fp contract(off)
                    r = (float)((coef[k][0] * (double)x + coef[k][1] * (double)y) / sin_omega);
                } else r = lt_lerp(x, y, tf[k]);
                o[(size_t)s * D + d] = r;
            }
        }
        __syncthreads();
    }
}

struct LatentReportArgs {
    const float* mu;          // [B,D]
    const float* logvar;      // [B,D]
    const float* x;           // [B,n_coords] or nullptr
    const float* rec;         // likewise
    double* rows;             // [B][5]
    double* cols;             // [3][D] or nullptr
    int64_t* count;           // or nullptr
    int64_t B;
    int D, n_points;
};

// One workgroup per window: the three latent sums over D, the joint distances over the window's n_points = T * J points.
__global__ __launch_bounds__(LT_THREADS) void latent_report_rows_kernel(LatentReportArgs a) {
    __shared__ double red[4][LT_WAVES];
    __shared__ double red_max[LT_WAVES];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const float* mu = a.mu + b * a.D;
    const float* lv = a.logvar + b * a.D;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    double far = 0.0;
    {          // plain IEEE float64 operations, like the numpy they are checked against: no fused multiply-add
#pragma clang fp contract(off)
        for (int d = tid; d < a.D; d += LT_THREADS) {
            const double m = (double)mu[d], l = (double)lv[d];
            const double sd = exp(0.5 * l) - 1.0;
            v[0] += m * m;
            v[1] += sd * sd;
            v[2] += 1.0 + l - m * m - exp(l);
        }
        if (a.x && a.rec) {
            const float* X = a.x + b * (size_t)a.n_points * 3;
            const float* R = a.rec + b * (size_t)a.n_points * 3;
            for (int i = tid; i < a.n_points; i += LT_THREADS) {
                const double dx = (double)R[3 * i] - (double)X[3 * i], dy = (double)R[3 * i + 1] - (double)X[3 * i + 1],
                             dz = (double)R[3 * i + 2] - (double)X[3 * i + 2];
                const double dist = sqrt(dx * dx + dy * dy + dz * dz);
                v[3] += dist;
                far = nan_max(far, dist);
            }
        }
    }
    lt_block_sums<4>(v, red);
    far = wave_max_dpp(far);
    if ((tid & 63) == 0) red_max[tid >> 6] = far;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < LT_WAVES; ++w) far = nan_max(far, red_max[w]);
        double* row = a.rows + b * 5;
        const bool have = a.x && a.rec;
        row[0] = v[0];
        row[1] = v[1];
        row[2] = -0.5 * v[2];
        row[3] = have ? v[3] / (double)a.n_points : __builtin_nan("");
        row[4] = have ? far : __builtin_nan("");
        if (b == 0 && a.count) *a.count += a.B;
    }
}

// The batch's contribution to the per-dimension accumulators.  A workgroup owns 16 neighbouring dimensions; its 16 row groups
// take the rows g, g + 16, g + 32, ... of the batch each (independent loads, one running sum per group), then the groups are
// added in order and the total goes onto the accumulator: the order of the additions depends on a row's index in the batch only.
constexpr int LT_COLS = 16, LT_GROUPS = LT_THREADS / LT_COLS;

__global__ __launch_bounds__(LT_THREADS) void latent_report_cols_kernel(LatentReportArgs a) {
    __shared__ double red[3][LT_GROUPS][LT_COLS];
    const int tid = threadIdx.x, c = tid & (LT_COLS - 1), g = tid / LT_COLS;
    const int d = blockIdx.x * LT_COLS + c;
    double v[3] = {0.0, 0.0, 0.0};
    if (d < a.D) {
#pragma clang fp contract(off)
#pragma unroll 4
        for (int64_t r = g; r < a.B; r += LT_GROUPS) {
            const double m = (double)a.mu[(size_t)r * a.D + d], l = (double)a.logvar[(size_t)r * a.D + d];
            v[0] += m;
            v[1] += m * m;
            v[2] += exp(l);
        }
    }
    for (int k = 0; k < 3; ++k) red[k][g][c] = v[k];
    __syncthreads();
    if (tid < 3 * LT_COLS) {
        const int k = tid / LT_COLS, cc = tid % LT_COLS, dd = blockIdx.x * LT_COLS + cc;
        if (dd < a.D) {
            double t = red[k][0][cc];
            for (int q = 1; q < LT_GROUPS; ++q) t += red[k][q][cc];
            a.cols[(size_t)k * a.D + dd] += t;
        }
    }
}

}  // namespace gem

extern "C" {

int gem_latent_paths(const float* d_za, const float* d_zb, int64_t n_pairs, int latent_dim, int n_steps, int mode, float* d_out,
                     void* stream) {
    using namespace gem;
    if (n_pairs < 1 || latent_dim < 1 || n_steps < 2) {
        set_error("gem_latent_paths: need n_pairs >= 1, latent_dim >= 1 and n_steps >= 2"); return 1;
    }
    if (mode != GEM_PATH_LINEAR && mode != GEM_PATH_SPHERICAL) {
        set_error("gem_latent_paths: unknown mode " + std::to_string(mode) + " (0 linear, 1 spherical)"); return 1;
    }
    if (n_pairs > 0x7fffffffLL) { set_error("gem_latent_paths: at most 2^31 - 1 pairs per call"); return 1; }
    if (!d_za || !d_zb || !d_out) { set_error("gem_latent_paths: null argument"); return 1; }
    hipLaunchKernelGGL(latent_paths_kernel, dim3((unsigned)n_pairs), dim3(LT_THREADS), 0, static_cast<hipStream_t>(stream), d_za, d_zb,
                       d_out, latent_dim, n_steps, mode);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_latent_report(const float* d_mu, const float* d_logvar, const float* d_x, const float* d_rec, int64_t n_windows, int latent_dim,
                      int n_coords, int n_joints, double* d_rows, double* d_cols, int64_t* d_count, void* stream) {
    using namespace gem;
    if (n_windows < 1 || latent_dim < 1) { set_error("gem_latent_report: need n_windows >= 1 and latent_dim >= 1"); return 1; }
    if (n_windows > 0x7fffffffLL) { set_error("gem_latent_report: at most 2^31 - 1 windows per call"); return 1; }
    if (!d_mu || !d_logvar || !d_rows) { set_error("gem_latent_report: null argument"); return 1; }
    const bool have = d_x && d_rec;
    if (have && (n_joints < 1 || n_coords < 3 * n_joints || n_coords % (3 * n_joints))) {
        set_error("gem_latent_report: n_coords must be frames * n_joints * 3 with n_joints >= 1"); return 1;
    }
    LatentReportArgs a;
    a.mu = d_mu; a.logvar = d_logvar; a.x = have ? d_x : nullptr; a.rec = have ? d_rec : nullptr;
    a.rows = d_rows; a.cols = d_cols; a.count = d_count; a.B = n_windows; a.D = latent_dim; a.n_points = have ? n_coords / 3 : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(latent_report_rows_kernel, dim3((unsigned)n_windows), dim3(LT_THREADS), 0, s, a);
    GEM_HIP(hipGetLastError());
    if (d_cols) {
        hipLaunchKernelGGL(latent_report_cols_kernel, dim3((unsigned)((latent_dim + LT_COLS - 1) / LT_COLS)), dim3(LT_THREADS), 0, s, a);
        GEM_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
