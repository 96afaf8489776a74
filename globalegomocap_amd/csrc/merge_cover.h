// A recording optimised as one continuous motion: the merge of windows that are NOT equally spaced.
//
//   gem_merge_cover   every frame the mean of all windows that cover it, for any ascending table of window starts (the last window of
//                     a recording is anchored to its end); per frame the number of covering windows and how far they disagree about
//                     the frame; optionally the Gaussian smoothing of the merged sequence (gauss_smooth_kernel, errors.hip)
//
// `sequence.merge_cover` is the definition.  Sums run over the covering windows oldest first, one lane per coordinate, no atomics and
// no shared memory: a frame's bytes depend on nothing but its own windows.
#include "gem_internal.h"

namespace gem {

constexpr int COVER_THREADS = 256;                       // four wavefronts = four frames per workgroup
constexpr int COVER_FRAMES = COVER_THREADS / 64;

struct MergeCoverArgs {
    const double* win;         // [n_windows, T, JC]
    const int32_t* starts;     // [n_windows]
    double* merged;            // [n_frames, JC]
    int32_t* count;            // [n_frames] or null
    double* spread;            // [n_frames] or null
    int64_t n_windows, n_frames;
    int T, JC;
};

// max that keeps a NaN once it has one, like numpy's
__device__ inline double cover_max(double m, double s) { return (s > m || s != s) ? s : m; }

// One wavefront per frame, lane c < JC owns coordinate c = 3 j + d.  The first covering window is the first one with
// starts[w] > f - T (binary search: the table ascends); the covering windows are those from there on with starts[w] <= f, at most T
// of them.  Every read is guarded by 0 <= w < n_windows and 0 <= f - starts[w] < T: whatever the table holds, nothing outside the
// arrays is touched and the walk ends after T windows.
__global__ __launch_bounds__(COVER_THREADS) void merge_cover_kernel(MergeCoverArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * COVER_FRAMES + (threadIdx.x >> 6);
    if (f >= a.n_frames) return;                         // (the whole wavefront leaves)
    const int T = a.T, JC = a.JC;
    const bool mine = lane < JC;
    int64_t lo = 0, hi = a.n_windows;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)a.starts[mid] + T > f) hi = mid; else lo = mid + 1;
    }
    const int64_t first = lo;
    double sum = 0.0;
    int n = 0;
    for (int k = 0; k < T && first + k < a.n_windows; ++k) {
        const int64_t t = f - (int64_t)a.starts[first + k];
        if (t < 0) break;
        if (t >= T) continue;
        if (mine) {
            const double x = a.win[((size_t)(first + k) * T + (size_t)t) * JC + lane];
            sum = n == 0 ? x : sum + x;                  // the first one as it is: 0 + x would lose the sign of -0
        }
        ++n;
    }
    const double mean = n ? sum / (double)n : __longlong_as_double(0x7ff8000000000000LL);
    if (mine) a.merged[(size_t)f * JC + lane] = mean;
    if (lane == 0 && a.count) a.count[f] = n;
    if (!a.spread) return;
    // the second walk: the largest distance between a window's joint and the merged joint.  A joint's three lanes exchange their
    // squared deviations; the maximum over joints and windows is taken on the squares (the square root is monotonic).
    const int j3 = mine ? lane - lane % 3 : lane;
    double worst = 0.0;
    for (int k = 0; k < T && first + k < a.n_windows; ++k) {
        const int64_t t = f - (int64_t)a.starts[first + k];
        if (t < 0) break;
        if (t >= T) continue;
        double sq = 0.0;
        if (mine) {
            const double d = a.win[((size_t)(first + k) * T + (size_t)t) * JC + lane] - mean;
            sq = d * d;
        }
        const double x2 = __shfl(sq, j3), y2 = __shfl(sq, mine ? j3 + 1 : lane), z2 = __shfl(sq, mine ? j3 + 2 : lane);
        if (mine) worst = cover_max(worst, (x2 + y2) + z2);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) worst = cover_max(worst, __shfl_xor(worst, o));
    if (lane == 0) a.spread[f] = n == 0 ? mean : (n == 1 ? 0.0 : sqrt(worst));
}

}  // namespace gem

extern "C" {

int gem_merge_cover(const double* d_windows, const int32_t* d_starts, int64_t n_windows, int T, int n_joints, int64_t n_frames,
                    double* d_merged, double* d_smooth, int32_t* d_count, double* d_spread, void* stream) {
    using namespace gem;
    if (!d_windows || !d_starts || !d_merged) { set_error("gem_merge_cover: null argument"); return 1; }
    if (T < 1) { set_error("gem_merge_cover: a window has at least one frame, got T = " + std::to_string(T)); return 1; }
    if (n_joints < 1 || n_joints > GEM_MAX_JOINTS) {
        set_error("gem_merge_cover: n_joints is between 1 and " + std::to_string(GEM_MAX_JOINTS) + ", got " + std::to_string(n_joints)); return 1;
    }
    if (n_windows < 0 || n_frames < 0) { set_error("gem_merge_cover: negative size"); return 1; }
    const int JC = 3 * n_joints;
    // (with the input below 2^40 doubles no index in the kernel overflows)
    if (n_windows > (((int64_t)1 << 40) / T) / JC) { set_error("gem_merge_cover: too many windows for one call"); return 1; }
    const int64_t blocks = (n_frames + COVER_FRAMES - 1) / COVER_FRAMES;
    if (blocks > 0x7fffffffLL) { set_error("gem_merge_cover: too many frames for one call"); return 1; }
    // (the smoothing kernel counts frames and elements in 32 bits)
    if (d_smooth && (n_frames >= ((int64_t)1 << 30) || (n_frames * JC + 255) / 256 > 0x7fffffffLL)) {
        set_error("gem_merge_cover: too many frames to smooth in one call"); return 1;
    }
    if (n_frames == 0) return 0;
    MergeCoverArgs a;
    a.win = d_windows; a.starts = d_starts; a.merged = d_merged; a.count = d_count; a.spread = d_spread;
    a.n_windows = n_windows; a.n_frames = n_frames; a.T = T; a.JC = JC;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(merge_cover_kernel, dim3((unsigned)blocks), dim3(COVER_THREADS), 0, s, a);
    GEM_HIP(hipGetLastError());
    if (d_smooth) {
        hipLaunchKernelGGL(gauss_smooth_kernel, dim3((unsigned)((n_frames * JC + 255) / 256)), dim3(256), 0, s, (const double*)d_merged, d_smooth,
                           1, (int)n_frames, JC);
        GEM_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
