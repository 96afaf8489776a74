// Recordings given as 2-D joint detections: one (u, v, confidence) per joint and frame instead of a heat-map.
// Included from errors.hip.
//
//   gem_keypoint_heatmaps  the detections splatted into the heat-maps every consumer takes: unit-peak Gaussians times the confidence
//   gem_lift_keypoints     FishEyeCalibrated.camera2world at the sub-pixel detection (float64), and which detections were usable
//   gem_fill_missing       unusable joints of a finished recording: linear interpolation in time inside their chunk
//
// A detection is usable when its confidence is > 0 (a NaN is not) and u and v are finite.  An unusable joint gets an all-zero map:
// the blank heat-map whose reprojection term contributes nothing.
//
// The splat is the only kernel here with any volume: 245 KB out per frame for 360 bytes in.  One workgroup per frame builds the two
// separable tables exp(-(x - ix)^2 / 2 sigma^2) and exp(-(y - iy)^2 / 2 sigma^2) in LDS -- J (H + W) exponentials, float64, so that
// the product rounded to float32 is the float64 Gaussian rounded to float32 -- and then walks the frame's flat run of H W J floats in
// 16-byte stores; lane l of a wavefront writes bytes [16 l, 16 l + 16) of a 1 KB run.  J = 15: a store straddles pixels, so the walk
// is by flat element.  The x table is kept as [x][j]: its index is the element's offset inside its row, so consecutive elements read
// consecutive doubles; the y table as [y][j].  A frame whose run does not start on a 16-byte boundary or is no multiple of four floats
// has up to three scalar stores in front and behind.  No division in the loop: (row, offset in row, joint) advance by the stride's
// constants.
#pragma once
#include "gem_internal.h"

namespace gem {

constexpr int KP_THREADS = 256;
typedef float kp_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool kp_usable(double u, double v, double conf) {
    return conf > 0.0 && isfinite(u) && isfinite(v);          // (NaN > 0 is false)
}

struct SplatArgs {
    const double* kp;      // [n,J,3]
    float* heat;           // [n,H,W,J]
    int H, W, J;
    double inv2s2;         // 1 / (2 sigma^2)
    double sx, sy;         // (W - 1) / 1024, (H - 1) / 1024
};

// one element of the frame: row y, offset r = x J + j inside the row, joint j
__device__ __forceinline__ float splat_value(const double* tx, const double* ty, int y, int r, int j, int J) {
    return (float)(tx[r] * ty[y * J + j]);
}

__global__ __launch_bounds__(KP_THREADS) void keypoint_heatmaps_kernel(SplatArgs a) {
    extern __shared__ double kp_lds[];
    const int f = blockIdx.x, tid = threadIdx.x, H = a.H, W = a.W, J = a.J;
    const int RW = W * J, N = H * RW;          // floats per row, per frame (the host has checked N < 2^30)
    double* tx = kp_lds;                       // [W][J]: amplitude * exp(-(x - ix)^2 / 2 sigma^2)
    double* ty = kp_lds + RW;                  // [H][J]
    const double* kp = a.kp + (size_t)f * J * 3;
    for (int i = tid; i < RW + H * J; i += KP_THREADS) {
        const bool is_x = i < RW;
        const int k = is_x ? i : i - RW, c = k / J, j = k - c * J;
        const double u = kp[j * 3], v = kp[j * 3 + 1], conf = kp[j * 3 + 2];
        double val = 0.0;
        if (kp_usable(u, v, conf)) {
            const double d = is_x ? (double)c - (u - 128.0) * a.sx : (double)c - v * a.sy;
            val = exp(-(d * d) * a.inv2s2);
            if (is_x) val *= fmin(conf, 1.0);          // (conf > 0 here: the clamp's lower end is the usable rule)
        }
        kp_lds[i] = val;
    }
    __syncthreads();
    float* out = a.heat + (size_t)f * N;
    const int head = min((int)((4 - ((reinterpret_cast<uintptr_t>(out) >> 2) & 3)) & 3), N);
    const int n4 = (N - head) >> 2, tail0 = head + 4 * n4;
    // scalar stores in front of the first and behind the last 16-byte boundary (at most three each)
    if (tid < head) {
        const int y = tid / RW, r = tid - y * RW;
        out[tid] = splat_value(tx, ty, y, r, r % J, J);
    }
    if (tid >= 32 && tid - 32 < N - tail0) {
        const int e = tail0 + tid - 32, y = e / RW, r = e - y * RW;
        out[e] = splat_value(tx, ty, y, r, r % J, J);
    }
    // the 16-byte stores: vector q holds elements head + 4 q .. + 3
    constexpr int STEP = 4 * KP_THREADS;
    const int dy = STEP / RW, dr = STEP - dy * RW, dj = STEP % J;
    int e = head + 4 * tid;
    int y = e / RW, r = e - y * RW, j = r % J;
    kp_f4* out4 = reinterpret_cast<kp_f4*>(out + head);
    for (int q = tid; q < n4; q += KP_THREADS) {
        kp_f4 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            int rc = r + c, yc = y, jc = j + c;
            if (rc >= RW) { rc -= RW; ++yc; }          // (RW >= 4: checked on the host)
            if (jc >= J) jc -= J;
            if (jc >= J) jc -= J;                      // (J < 4: c may pass it twice; J >= 2 by the host's check)
            v[c] = splat_value(tx, ty, yc, rc, jc, J);
        }
        out4[q] = v;
        y += dy; r += dr; j += dj;
        if (r >= RW) { r -= RW; ++y; }
        if (j >= J) j -= J;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------- lifting
struct KpLiftArgs {
    const double* kp;      // [n,J,3]
    const double* depth;   // [n,J]
    double* prev;          // [J,3] or nullptr
    double* out64;         // [n,J,3] or nullptr
    float* out32;          // [n,J,3] or nullptr
    unsigned char* valid;  // [n,J] or nullptr
    int n, J, n_poly;
    double poly[GEM_MAX_POLY];
    double cx, cy;
};

// camera2world at image point (X, Y), the expressions of lift_skeleton_kernel: the same bits for the same point
__device__ __forceinline__ void kp_camera2world(const KpLiftArgs& a, double X, double Y, double d, double o[3]) {
    const double x = X - a.cx, y = Y - a.cy;
    const double r = sqrt(x * x + y * y);
    double z = a.poly[a.n_poly - 1];
    for (int k = a.n_poly - 2; k >= 0; --k) z = z * r + a.poly[k];
    const double v[3] = {x, y, -z};
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int c = 0; c < 3; ++c) o[c] = v[c] / n * d;
}

__device__ __forceinline__ void kp_lift_one(const KpLiftArgs& a, int f, int j, double held[3]) {
    const size_t at = (size_t)f * a.J + j;
    const double u = a.kp[at * 3], v = a.kp[at * 3 + 1], conf = a.kp[at * 3 + 2];
    const bool ok = kp_usable(u, v, conf);
    double o[3] = {held[0], held[1], held[2]};
    if (ok) {
        kp_camera2world(a, u, v, a.depth[at], o);
        for (int c = 0; c < 3; ++c) held[c] = o[c];
    }
    for (int c = 0; c < 3; ++c) {
        if (a.out64) a.out64[at * 3 + c] = o[c];
        if (a.out32) a.out32[at * 3 + c] = (float)o[c];
    }
    if (a.valid) a.valid[at] = ok ? 1 : 0;
}

// without `prev`: one thread per (frame, joint), an unusable joint is written as zeros (gem_fill_missing replaces it)
__global__ __launch_bounds__(KP_THREADS) void lift_keypoints_kernel(KpLiftArgs a) {
    const size_t i = (size_t)blockIdx.x * KP_THREADS + threadIdx.x;
    if (i >= (size_t)a.n * a.J) return;
    double held[3] = {0.0, 0.0, 0.0};
    kp_lift_one(a, (int)(i / a.J), (int)(i % a.J), held);
}

// with `prev`: one thread per joint walks the frames in order, holding the last usable value
__global__ __launch_bounds__(64) void lift_keypoints_hold_kernel(KpLiftArgs a) {
    const int j = threadIdx.x;
    if (j >= a.J) return;
    double held[3] = {a.prev[j * 3], a.prev[j * 3 + 1], a.prev[j * 3 + 2]};
    for (int f = 0; f < a.n; ++f) kp_lift_one(a, f, j, held);
    for (int c = 0; c < 3; ++c) a.prev[j * 3 + c] = held[c];
}

// ---------------------------------------------------------------------------------------------------------------------------- filling
// one thread per (chunk, joint): the frames in order; a run of invalid frames between valid frames lo and hi becomes
// seq[lo] + (seq[hi] - seq[lo]) (f - lo) / (hi - lo), a run at either end the nearest valid value
__global__ __launch_bounds__(KP_THREADS) void fill_missing_kernel(double* seq, const unsigned char* valid, int n_chunks, int fpc, int J) {
    const int i = blockIdx.x * KP_THREADS + threadIdx.x;
    if (i >= n_chunks * J) return;
    const int chunk = i / J, j = i - chunk * J;
    const size_t base = (size_t)chunk * fpc;
    int lo = -1, f = 0;
    while (f < fpc) {
        if (valid[(base + f) * J + j]) { lo = f++; continue; }
        int hi = f + 1;
        while (hi < fpc && !valid[(base + hi) * J + j]) ++hi;
        if (lo >= 0 || hi < fpc) {          // (a joint with no valid frame in the chunk is left as it is: the caller refuses it)
            for (int g = f; g < hi; ++g)
                for (int c = 0; c < 3; ++c) {
                    double* dst = seq + ((base + g) * J + j) * 3 + c;
                    if (lo < 0) *dst = seq[((base + hi) * J + j) * 3 + c];
                    else if (hi >= fpc) *dst = seq[((base + lo) * J + j) * 3 + c];
                    else {
                        const double p = seq[((base + lo) * J + j) * 3 + c], q = seq[((base + hi) * J + j) * 3 + c];
                        const double w = (double)(g - lo) / (double)(hi - lo);
                        *dst = p + (q - p) * w;
                    }
                }
        }
        f = hi;
    }
}

}  // namespace gem

extern "C" {

int gem_keypoint_heatmaps(const double* d_kp, int64_t n_frames, int n_joints, int heat_h, int heat_w, double sigma, float* d_heat,
                          void* stream) {
    using namespace gem;
    if (n_frames < 0 || n_frames > 0x7fffffff) { set_error("gem_keypoint_heatmaps: n_frames out of range"); return 1; }
    if (n_joints < 2 || n_joints > MAXJ_ERR || heat_h < 1 || heat_w < 2 || heat_h > 4096 || heat_w > 4096) {
        set_error("gem_keypoint_heatmaps: need 2 .. " + std::to_string(MAXJ_ERR) + " joints and maps of 1 .. 4096 rows, 2 .. 4096 columns"); return 1;
    }
    if (!(sigma > 0.0) || !std::isfinite(sigma)) { set_error("gem_keypoint_heatmaps: sigma must be a positive number"); return 1; }
    const size_t lds = (size_t)n_joints * (heat_h + heat_w) * sizeof(double);
    if (lds > 64 * 1024) { set_error("gem_keypoint_heatmaps: the two tables of J (H + W) doubles must fit 64 KB of LDS"); return 1; }
    if (n_frames == 0) return 0;
    if (!d_kp || !d_heat) { set_error("gem_keypoint_heatmaps: null argument"); return 1; }
    if (reinterpret_cast<uintptr_t>(d_heat) & 3) { set_error("gem_keypoint_heatmaps: d_heat must be 4-byte aligned"); return 1; }
    SplatArgs a;
    a.kp = d_kp; a.heat = d_heat; a.H = heat_h; a.W = heat_w; a.J = n_joints;
    a.inv2s2 = 1.0 / (2.0 * sigma * sigma);
    a.sx = (double)(heat_w - 1) / 1024.0; a.sy = (double)(heat_h - 1) / 1024.0;
    hipLaunchKernelGGL(keypoint_heatmaps_kernel, dim3((unsigned)n_frames), dim3(KP_THREADS), lds, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_lift_keypoints(gem_handle* h, const double* d_kp, const double* d_depth, int64_t n_frames, const double* h_poly_c2w, int n_poly,
                       double* d_prev, double* d_out64, float* d_out32, unsigned char* d_valid, void* stream) {
    using namespace gem;
    if (!h) { set_error("gem_lift_keypoints: null handle"); return 1; }
    if (n_frames < 0 || n_frames > 0x7fffffff / MAXJ_ERR || n_poly < 1 || n_poly > GEM_MAX_POLY) {
        set_error("gem_lift_keypoints: need 0 <= n_frames < 2^27 and 1 <= n_poly <= 16"); return 1;
    }
    if (h->J > 64) { set_error("gem_lift_keypoints: at most 64 joints"); return 1; }
    if (n_frames == 0) return 0;
    if (!d_kp || !d_depth || !h_poly_c2w || (!d_out64 && !d_out32 && !d_valid)) { set_error("gem_lift_keypoints: null argument"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    KpLiftArgs a;
    a.kp = d_kp; a.depth = d_depth; a.prev = d_prev; a.out64 = d_out64; a.out32 = d_out32; a.valid = d_valid;
    a.n = (int)n_frames; a.J = h->J; a.n_poly = n_poly;
    for (int i = 0; i < GEM_MAX_POLY; ++i) a.poly[i] = i < n_poly ? h_poly_c2w[i] : 0.0;
    a.cx = h->cfg.cx; a.cy = h->cfg.cy;
    if (d_prev)
        hipLaunchKernelGGL(lift_keypoints_hold_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL(lift_keypoints_kernel, dim3((unsigned)(((size_t)a.n * a.J + KP_THREADS - 1) / KP_THREADS)), dim3(KP_THREADS), 0,
                           static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_fill_missing(double* d_seq, const unsigned char* d_valid, int n_chunks, int frames_per_chunk, int n_joints, void* stream) {
    using namespace gem;
    if (n_chunks < 0 || frames_per_chunk < 0 || n_joints < 1 || n_joints > 64 ||
        (int64_t)n_chunks * frames_per_chunk > 0x7fffffff / 64) {
        set_error("gem_fill_missing: need n_chunks >= 0, frames_per_chunk >= 0, 1 .. 64 joints and fewer than 2^25 frames"); return 1;
    }
    if (n_chunks == 0 || frames_per_chunk == 0) return 0;
    if (!d_seq || !d_valid) { set_error("gem_fill_missing: null argument"); return 1; }
    const int n = n_chunks * n_joints;
    hipLaunchKernelGGL(fill_missing_kernel, dim3((unsigned)((n + KP_THREADS - 1) / KP_THREADS)), dim3(KP_THREADS), 0,
                       static_cast<hipStream_t>(stream), d_seq, d_valid, n_chunks, frames_per_chunk, n_joints);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
