// Heat-maps without a depth network: the maps' peaks as sub-pixel detections (u, v, confidence).
// Included from errors.hip, behind keypoints.h (the detections' convention) and the lifting kernels (lift_better).
//
//   gem_heatmap_peaks  per frame and joint the integer maximum of the map (numpy's argmax: NaN is maximal, the first occurrence wins)
//                      and, from it, eight iterations of a Gaussian-windowed mean shift over the 9 x 9 texels around it:
//                      m <- sum w k x / sum w k, w = max(value, 0), k = exp(-(x - m_x)^2 / 2 tau^2) exp(-(y - m_y)^2 / 2 tau^2), tau = 1.5.
//                      The fixed point is the centre of a Gaussian blob whatever its own width; it is a sum, so texel noise averages
//                      out, and it takes no logarithm of small values.
//
// One 256-thread workgroup per frame, two passes.
//
// Pass 1 is gem_lift_skeleton's scan: the frame in its [H,W,J] layout, 16-byte non-temporal loads, a wavefront's load 1 KB contiguous,
// the running maxima in registers (a thread's four lanes of every load hold the same four joints, the stride 4 A being a multiple of
// J); the candidates are combined per joint by 16 lanes.  A frame that is no whole number of 16-byte words, or a tensor that does not
// start on a 16-byte boundary, takes the generic scan (thread (g, j) walks pixels g, g + 16, ... of joint j).
//
// Pass 2, layout: 16 LANES PER JOINT, the window in registers.  Lane r < 9 of a joint's group holds row sy - 4 + r of the window (nine
// texels, zero outside the map: clipping the window and adding zeros are the same sum) and the coordinate r of both separable tables:
// per iteration it takes ONE exponential for column sx - 4 + r and ONE for its row (9 + 9 per joint), the nine column weights go round
// by lane broadcasts, the lane sums its row in ascending x, and the three row totals (sum w k, sum w k x, sum w k y) are added over
// the 16 lanes by an xor butterfly (8, 4, 2, 1; a float add commutes, so every lane ends with the same bits).  One lane per joint
// would run 8 x (18 exponentials + 81 x 3 multiply-adds) in a row behind the stream of the frame -- a serial tail of the order of the
// streaming time itself; one lane per texel needs the window in LDS and a 128-lane reduction per sum.  Sixteen lanes cut the chain to
// 2 exponentials + 9 row terms + 4 butterfly levels per iteration and need no LDS and no barrier.
//
// float64 throughout pass 2, no fused multiply-adds (the numpy twin of the tests rounds the same way), every sum in a fixed order, no
// atomics, plain vector stores; a frame has its own workgroup, so its bytes do not depend on the frames beside it.
#pragma once
#include "keypoints.h"

namespace gem {

constexpr int HP_THREADS = 256;
constexpr int HP_R = 4, HP_N = 2 * HP_R + 1;              // the window: texels within 4 of the maximum
constexpr int HP_ITERS = 8;
constexpr int HP_SLOTS = 80;                              // candidates per joint in LDS (the streaming scan leaves 4 A / J <= 80)
constexpr double HP_INV2T2 = 1.0 / (2.0 * 1.5 * 1.5);      // 1 / (2 tau^2), tau = 1.5 texels
constexpr int HP_NONE = 0x7fffffff;
typedef float hp_f4 __attribute__((ext_vector_type(4)));

struct PeakArgs {
    const float* heat;     // [n,H,W,J]
    double* kp;            // [n,J,3] or nullptr
    int32_t* arg;          // [n,J] or nullptr
    int H, W, J;
    double su, sv;         // upscale W / (W - 1), upscale H / (H - 1)
    double pad_x, pad_y, min_peak;
};

// the sum of v over the 16 lanes of a joint's group, in every lane: levels 8, 4, 2, 1
__device__ __forceinline__ double hp_sum16(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 16);
    return v;
}

template <bool STREAM>
__global__ __launch_bounds__(HP_THREADS) void heatmap_peaks_kernel(PeakArgs a, int A) {
#pragma clang fp contract(off)
    __shared__ float c_val[16 * HP_SLOTS];
    __shared__ int c_idx[16 * HP_SLOTS];
    const int f = blockIdx.x, tid = threadIdx.x, J = a.J, H = a.H, W = a.W;
    const int j = tid >> 4, part = tid & 15;             // pass 2 and the end of pass 1: 16 lanes per joint
    const float* frame = a.heat + (size_t)f * H * W * J;
    // ------------------------------------------------------------------------------------------------ pass 1: the integer maximum
    float b = -INFINITY;
    int i = HP_NONE;
    if (STREAM) {
        const int n4 = H * W * J / 4, n_slots = 4 * A / J;
        const hp_f4* base = reinterpret_cast<const hp_f4*>(frame);
        if (tid < A) {
            float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            int bi[4] = {HP_NONE, HP_NONE, HP_NONE, HP_NONE};
#pragma unroll 8
            for (int q = tid; q < n4; q += A) {
                const hp_f4 v = __builtin_nontemporal_load(base + q);
#pragma unroll
                for (int c = 0; c < 4; ++c)          // ascending scan: a strict improvement (or the first NaN) takes over
                    if (v[c] > best[c] || (v[c] != v[c] && best[c] == best[c])) { best[c] = v[c]; bi[c] = (4 * q + c) / J; }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int e = 4 * tid + c, jj = e % J, slot = e / J;
                c_val[jj * HP_SLOTS + slot] = best[c];
                c_idx[jj * HP_SLOTS + slot] = bi[c];
            }
        }
        __syncthreads();
        if (j < J)
            for (int sl = part; sl < n_slots; sl += 16)
                if (lift_better(c_val[j * HP_SLOTS + sl], c_idx[j * HP_SLOTS + sl], b, i)) { b = c_val[j * HP_SLOTS + sl]; i = c_idx[j * HP_SLOTS + sl]; }
    } else {
        const int g = tid >> 4, jj = tid & 15, P = H * W;          // thread (g, jj): pixels g, g + 16, ... of joint jj
        float best = -INFINITY;
        int bi = HP_NONE;
        if (jj < J)
            for (int p = g; p < P; p += 16) {
                const float v = frame[(size_t)p * J + jj];
                if (lift_better(v, p, best, bi)) { best = v; bi = p; }
            }
        c_val[jj * HP_SLOTS + g] = best;
        c_idx[jj * HP_SLOTS + g] = bi;
        __syncthreads();
        if (j < J) { b = c_val[j * HP_SLOTS + part]; i = c_idx[j * HP_SLOTS + part]; }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const float ob = __shfl_xor(b, o, 16);
        const int oi = __shfl_xor(i, o, 16);
        if (lift_better(ob, oi, b, i)) { b = ob; i = oi; }
    }
    if (i == HP_NONE) i = 0;          // (a map of -inf alone never improves on the start: its first maximum is texel 0)
    // ------------------------------------------------------------------------------------------------ pass 2: the mean shift
    const bool act = j < J;
    const int sx = i % W, sy = i / W;
    const int y = sy - HP_R + part;                      // this lane's row of the window (lanes 9 .. 15 hold zeros)
    double w[HP_N];
#pragma unroll
    for (int c = 0; c < HP_N; ++c) {
        const int x = sx - HP_R + c;
        float t = 0.f;
        if (act && part < HP_N && y >= 0 && y < H && x >= 0 && x < W) t = frame[((size_t)y * W + x) * J + j];
        w[c] = fmax((double)t, 0.0);                     // (a NaN texel weighs nothing)
    }
    const double xc = (double)(sx - HP_R + part), yc = (double)y;          // the column and the row whose table entry this lane makes
    double mx = (double)sx, my = (double)sy;
    for (int it = 0; it < HP_ITERS; ++it) {
        const double dx = xc - mx, dy = yc - my;
        const double kx = exp(-(dx * dx) * HP_INV2T2), ky = exp(-(dy * dy) * HP_INV2T2);
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int c = 0; c < HP_N; ++c) {
            const double t = w[c] * __shfl(kx, c, 16);
            s0 = s0 + t;
            s1 = s1 + t * (double)(sx - HP_R + c);
        }
        const double r0 = ky * s0, r1 = ky * s1, r2 = r0 * yc;
        const double t0 = hp_sum16(r0), t1 = hp_sum16(r1), t2 = hp_sum16(r2);
        mx = t1 / t0;
        my = t2 / t0;
    }
    if (act && part == 0) {
        const size_t at = (size_t)f * J + j;
        const bool ok = b > 0.f && !((double)b < a.min_peak);          // (NaN > 0 is false)
        if (a.kp) {
            a.kp[at * 3] = ok ? a.pad_x + mx * a.su : 0.0;
            a.kp[at * 3 + 1] = ok ? a.pad_y + my * a.sv : 0.0;
            a.kp[at * 3 + 2] = ok ? (double)fminf(b, 1.f) : 0.0;
        }
        if (a.arg) a.arg[at] = i;
    }
}

}  // namespace gem

extern "C" {

int gem_heatmap_peaks(gem_handle* h, const float* d_heat, int64_t n_frames, int upscale, int pad_x, int pad_y, double min_peak,
                      double* d_kp, int32_t* d_arg, void* stream) {
    using namespace gem;
    if (!h) { set_error("gem_heatmap_peaks: null handle"); return 1; }
    if (!d_kp && !d_arg) { set_error("gem_heatmap_peaks: null argument (one of d_kp and d_arg is needed)"); return 1; }
    if (n_frames < 0 || n_frames > 0x7fffffff / MAXJ_ERR || upscale < 1 || pad_x < 0 || pad_y < 0) {
        set_error("gem_heatmap_peaks: need 0 <= n_frames < 2^27, upscale >= 1, pads >= 0"); return 1;
    }
    if (!(min_peak >= 0.0) || !std::isfinite(min_peak)) { set_error("gem_heatmap_peaks: min_peak must be a finite number >= 0"); return 1; }
    const int H = h->cfg.heat_h, W = h->cfg.heat_w, J = h->J;
    if (J < 1 || J > 16 || H < 2 || W < 2 || (int64_t)H * W * J >= (int64_t)1 << 30) {
        set_error("gem_heatmap_peaks: need 1 .. 16 joints and maps of at least 2 x 2 texels, fewer than 2^30 floats per frame"); return 1;
    }
    if (n_frames == 0) return 0;
    if (!d_heat) { set_error("gem_heatmap_peaks: null argument"); return 1; }
    if (reinterpret_cast<uintptr_t>(d_heat) & 3) { set_error("gem_heatmap_peaks: d_heat must be 4-byte aligned"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    PeakArgs a;
    a.heat = d_heat; a.kp = d_kp; a.arg = d_arg; a.H = H; a.W = W; a.J = J;
    a.su = (double)upscale * (double)W / (double)(W - 1);
    a.sv = (double)upscale * (double)H / (double)(H - 1);
    a.pad_x = (double)pad_x; a.pad_y = (double)pad_y; a.min_peak = min_peak;
    const int Jr = J / (J % 4 == 0 ? 4 : J % 2 == 0 ? 2 : 1);      // J / gcd(J, 4)
    const int A = HP_THREADS / Jr * Jr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((H * W * J) % 4 == 0 && 4 * A / J <= HP_SLOTS && (reinterpret_cast<uintptr_t>(d_heat) & 15) == 0)
        hipLaunchKernelGGL(heatmap_peaks_kernel<true>, dim3((unsigned)n_frames), dim3(HP_THREADS), 0, s, a, A);
    else
        hipLaunchKernelGGL(heatmap_peaks_kernel<false>, dim3((unsigned)n_frames), dim3(HP_THREADS), 0, s, a, A);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
