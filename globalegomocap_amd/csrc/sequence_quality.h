// A report on merged sequences that needs no ground truth: what the reference's own energy terms say
// about a sequence, evaluated on the chunk's merged frames instead of per window.  Included from
// errors.hip.
//
//   gem_sequence_quality  per chunk four numbers: the mean heat-map response under the re-projected joints, the RMS deviation of
//                         the bone lengths from the chunk's mean bone lengths, the mean joint acceleration and the mean distance
//                         to a second sequence
//
// The heat-maps stay where they are (246 KB per frame): one thread per (frame, joint) gathers its four texels.  About 1500
// samples per chunk: a latency / gather kernel.  The projection and the sampling are energy_device.h's, so a joint sees the
// very fp32 arithmetic the optimiser's reprojection term applied to it.  Sums are float64 and fixed-order -- DPP wavefront sums,
// the wavefronts of a workgroup in order, the workgroups of a chunk in order by a second small launch -- so two calls give
// bitwise the same row; there are no floating-point atomics.
#pragma once
#include "energy_device.h"

namespace gem {

constexpr int SQ_FRAMES = 16;            // frames per workgroup, 16 lanes each (lane = joint; MAXJ_ERR == 16)
constexpr int SQ_THREADS = SQ_FRAMES * 16;
static_assert(MAXJ_ERR <= 16, "sequence_quality_kernel gives a frame 16 lanes");

struct SeqQualityArgs {
    const double* seq;         // [n_chunks*fpc, J, 3]
    const double* ref;         // the same shape, or nullptr
    const double* cams;        // [F,4,4]
    const float* heat;         // [F,H,W,J]
    const int64_t* frame0;     // [n_chunks]
    const float* mean_bone;    // [n_chunks, J]
    double* partial;           // [n_chunks][n_blocks][4]
    double* out;               // [n_chunks][4]
    int64_t F;
    int fpc, J, H, W, n_poly, n_blocks, n_bones;
    float poly[GEM_MAX_POLY];
    float cx, cy;
    int parents[MAXJ_ERR];
};

__global__ __launch_bounds__(SQ_THREADS) void sequence_quality_kernel(SeqQualityArgs a) {
    __shared__ double red[SQ_THREADS / 64][4];
    const int chunk = blockIdx.y, tid = threadIdx.x, j = tid & 15, f = blockIdx.x * SQ_FRAMES + (tid >> 4);
    const int J = a.J, fpc = a.fpc;
    double v[4] = {0.0, 0.0, 0.0, 0.0};      // this (frame, joint)'s terms of the four sums
    if (f < fpc && j < J) {
        const size_t at = (((size_t)chunk * fpc + f) * J + j) * 3;
        const double* X = a.seq + at;
        const double x[3] = {X[0], X[1], X[2]};
        {          // the float64 columns are plain IEEE operations, like the numpy they are checked against: no fused multiply-add
#pragma clang fp contract(off)
            const int par = a.parents[j];
            if (par != j) {
                const double* P = a.seq + (((size_t)chunk * fpc + f) * J + par) * 3;
                const double bx = x[0] - P[0], by = x[1] - P[1], bz = x[2] - P[2];
                const double d = sqrt(bx * bx + by * by + bz * bz) - (double)a.mean_bone[(size_t)chunk * J + j];
                v[1] = d * d;
            }
            if (f >= 1 && f <= fpc - 2) {
                const double* Xm = X - (size_t)J * 3;
                const double* Xp = X + (size_t)J * 3;
                const double ax = Xm[0] - 2.0 * x[0] + Xp[0], ay = Xm[1] - 2.0 * x[1] + Xp[1], az = Xm[2] - 2.0 * x[2] + Xp[2];
                v[2] = sqrt(ax * ax + ay * ay + az * az);
            }
            if (a.ref) {
                const double* R = a.ref + at;
                const double dx = x[0] - R[0], dy = x[1] - R[1], dz = x[2] - R[2];
                v[3] = sqrt(dx * dx + dy * dy + dz * dz);
            }
        }
        const int64_t g = a.frame0[chunk] + f;
        if (g < 0 || g >= a.F) {
            v[0] = __builtin_nan("");          // a frame outside the buffers is never read
        } else {
            float xc[3];
            {          // X_cam = C^-1 X for a rigid C = [R | t]: R^T (X - t), float64, rounded once
#pragma clang fp contract(off)
                const double* M = a.cams + (size_t)g * 16;
                const double d0 = x[0] - M[3], d1 = x[1] - M[7], d2 = x[2] - M[11];
                for (int r = 0; r < 3; ++r) xc[r] = (float)(M[r] * d0 + M[4 + r] * d1 + M[8 + r] * d2);
            }
            const FisheyeUV q = fisheye_uv(a.poly, a.n_poly, a.cx, a.cy, xc[0], xc[1], xc[2]);
            const HeatTap k = heat_tap(q.u, q.v, a.H, a.W);
            const float* hm = a.heat + ((size_t)g * a.H * a.W) * J + j;
            float nw = hm[((size_t)k.ya * a.W + k.xa) * J];
            float ne = hm[((size_t)k.ya * a.W + k.xb) * J];
            float sw = hm[((size_t)k.yc * a.W + k.xa) * J];
            float se = hm[((size_t)k.yc * a.W + k.xb) * J];
            const float val = heat_bilinear(k, nw, ne, sw, se);
            v[0] = q.nn == 0.f ? __builtin_nan("") : (double)val;      // a joint on the optical axis: NaN, like the energy
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double w = wave_sum(v[c]);
        if ((tid & 63) == 0) red[tid >> 6][c] = w;
    }
    __syncthreads();
    if (tid < 4) {
        double t = 0.0;
        for (int w = 0; w < SQ_THREADS / 64; ++w) t += red[w][tid];
        a.partial[((size_t)chunk * a.n_blocks + blockIdx.x) * 4 + tid] = t;
    }
}

// the workgroups' partial sums in block order, then the means: thread c of chunk blockIdx.x finishes column c
__global__ __launch_bounds__(64) void sequence_quality_finish_kernel(SeqQualityArgs a) {
    const int chunk = blockIdx.x, c = threadIdx.x;
    if (c >= 4) return;
    double t = 0.0;
    for (int b = 0; b < a.n_blocks; ++b) t += a.partial[((size_t)chunk * a.n_blocks + b) * 4 + c];
    const double pairs = (double)a.fpc * a.J;
    double r;
    if (c == 0) r = t / pairs;
    else if (c == 1) r = sqrt(t / ((double)a.fpc * a.n_bones));
    else if (c == 2) r = t / ((double)(a.fpc > 2 ? a.fpc - 2 : 0) * a.J);          // fewer than three frames: 0 / 0
    else r = a.ref ? t / pairs : __builtin_nan("");
    a.out[(size_t)chunk * 4 + c] = r;
}

}  // namespace gem

extern "C" {

int gem_sequence_quality(gem_handle* h, const double* d_seq, const double* d_cams, const float* d_heat, int64_t n_frames,
                         const int64_t* d_frame0, const float* d_mean_bone, const double* d_ref, int n_chunks, int frames_per_chunk,
                         double* d_out, void* stream) {
    using namespace gem;
    if (!h) { set_error("gem_sequence_quality: null handle"); return 1; }
    if (n_chunks < 0 || frames_per_chunk < 1 || n_frames < 0) {
        set_error("gem_sequence_quality: need n_chunks >= 0, frames_per_chunk >= 1 and n_frames >= 0"); return 1;
    }
    if (n_chunks == 0) return 0;
    if (!d_seq || !d_cams || !d_heat || !d_frame0 || !d_mean_bone || !d_out) { set_error("gem_sequence_quality: null argument"); return 1; }
    if (n_chunks > 65535) { set_error("gem_sequence_quality: at most 65535 chunks per call"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    SeqQualityArgs a;
    a.seq = d_seq; a.ref = d_ref; a.cams = d_cams; a.heat = d_heat; a.frame0 = d_frame0; a.mean_bone = d_mean_bone; a.out = d_out;
    a.F = n_frames; a.fpc = frames_per_chunk; a.J = h->J; a.H = h->cfg.heat_h; a.W = h->cfg.heat_w; a.n_poly = h->cfg.n_poly;
    a.n_blocks = (frames_per_chunk + SQ_FRAMES - 1) / SQ_FRAMES;
    for (int i = 0; i < GEM_MAX_POLY; ++i) a.poly[i] = i < a.n_poly ? (float)h->cfg.poly[i] : 0.f;
    a.cx = (float)h->cfg.cx; a.cy = (float)h->cfg.cy;
    a.n_bones = 0;
    for (int j = 0; j < MAXJ_ERR; ++j) {
        a.parents[j] = j < h->J ? h->cfg.parents[j] : j;
        if (j < h->J && a.parents[j] != j) ++a.n_bones;
    }
    if (post_scratch(h, (size_t)n_chunks * a.n_blocks * 4)) return 1;
    a.partial = h->post_work;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sequence_quality_kernel, dim3((unsigned)a.n_blocks, (unsigned)n_chunks), dim3(SQ_THREADS), 0, s, a);
    GEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(sequence_quality_finish_kernel, dim3((unsigned)n_chunks), dim3(64), 0, s, a);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
