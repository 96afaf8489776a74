// Live mode: a stream optimised window by window as its frames arrive.  Included from errors.hip.
//
//   gem_live_push    k <= 8 new frames into the frame rings, their bone lengths onto the running sums
//   gem_live_window  the frames [8w, 8w + 10) from the rings into the buffers of fixed address that the optimiser's call reads
//                    (fixed addresses: one captured graph serves every window), and the mean bone lengths the call is given
//   gem_live_emit    the window's result merged with the two frames held from the window before (sequence.merge_batches' expression),
//                    the estimated sequence cams . pose, the causal One-Euro filter, 8 final frames out, two frames held
//   gem_one_euro     the same filter over whole sequences (chunks x coordinates in parallel, frames in order)
//   gem_live_window_at, gem_live_emit_dense, gem_merge_dense   a window every k <= 8 frames and dense merging: the file's second half
//
// A frame of heat-maps is 245 KB and a window 2.4 MB: the two copy kernels move 16-byte vectors with one workgroup per (frame, row).
// Everything else is a few hundred doubles handled by one workgroup; all state lives in the caller's block (gem_hip.h has its
// layout).  Sums and recurrences run in frame order in one thread per joint / coordinate: the same bits on every call.
#pragma once
#include "gem_internal.h"

namespace gem {

constexpr int LIVE_T = GEM_LIVE_WINDOW, LIVE_STRIDE = GEM_LIVE_STRIDE, LIVE_HOLD = LIVE_T - LIVE_STRIDE, LIVE_RING = GEM_LIVE_RING;
constexpr int LIVE_MAXC = 48;                // coordinates per frame the state block has room for (J <= 16)
constexpr int LIVE_THREADS = 256;
// the state block (gem_hip.h)
constexpr int LS_BONE = 0, LS_COUNT = 16, LS_PUSHED = 17, LS_WINDOWS = 18, LS_EMITTED = 19, LS_TPREV = 20, LS_HAVE_PREV = 21, LS_TAIL_T = 22,
              LS_HAVE_TAIL = 24, LS_XPREV = 32, LS_DXPREV = LS_XPREV + LIVE_MAXC, LS_TAIL_OPT = LS_DXPREV + LIVE_MAXC,
              LS_TAIL_EST = LS_TAIL_OPT + LIVE_HOLD * LIVE_MAXC;
static_assert(LS_TAIL_EST + LIVE_HOLD * LIVE_MAXC == GEM_LIVE_STATE_DOUBLES, "the state block's layout and its size disagree");
static_assert(3 * MAXJ_ERR <= LIVE_MAXC && MAXJ_ERR <= LS_COUNT, "the state block holds 16 joints");
static_assert(LIVE_T + GEM_LIVE_PUSH_MAX <= LIVE_RING, "the rings hold a window plus a full push");

typedef float live_f4 __attribute__((ext_vector_type(4)));

// n floats by the workgroup: 16-byte vectors when `vec` (n a multiple of 4, both pointers 16-byte aligned)
__device__ __forceinline__ void live_copy(const float* __restrict__ src, float* __restrict__ dst, int n, bool vec) {
    if (vec) {
        const live_f4* s = reinterpret_cast<const live_f4*>(src);
        live_f4* d = reinterpret_cast<live_f4*>(dst);
        for (int q = threadIdx.x; q < n / 4; q += LIVE_THREADS) d[q] = s[q];
    } else {
        for (int q = threadIdx.x; q < n; q += LIVE_THREADS) dst[q] = src[q];
    }
}

struct LiveArgs {
    gem_live_buffers b;
    const float* heat;         // push: [k,H,W,J]        window: the window buffer [T,H,W,J] (written)
    const float* pose;         // push: [k,J,3]          window / emit: the window buffer [T,J,3]
    const double* cams;        // push: [k,4,4]          window / emit: the window buffer [T,4,4]
    const double* times;       // push: [k]
    const float* bone_fixed;   // window: [J] or nullptr
    float* mean_bone;          // window: [J]
    const double* global;      // emit: [T,J,3]
    double* out;               // emit: [2][STRIDE][JC]
    int64_t first;             // push: the first frame's number        window / emit: the window's first frame, 8w
    int k, H, W, J, vec, final, filter;
    double euro[3];            // min_cutoff, beta, d_cutoff
    int parents[MAXJ_ERR];
};

// grid (k, H + 1): workgroup (i, y < H) copies row y of pushed frame i into its ring slot; (i, H) the frame's skeleton, camera and
// timestamp, and (0, H) adds the k frames' bone lengths to the sums, in frame order, one thread per joint.
__global__ __launch_bounds__(LIVE_THREADS) void live_push_kernel(LiveArgs a) {
    const int i = blockIdx.x, y = blockIdx.y, tid = threadIdx.x, J = a.J;
    const int slot = (int)((a.first + i) % LIVE_RING);
    const int row = a.W * J;
    if (y < a.H) {
        live_copy(a.heat + ((size_t)i * a.H + y) * row, a.b.ring_heat + ((size_t)slot * a.H + y) * row, row, a.vec != 0);
        return;
    }
    if (tid < J * 3) a.b.ring_pose[(size_t)slot * J * 3 + tid] = a.pose[(size_t)i * J * 3 + tid];
    if (tid < 16) a.b.ring_cams[(size_t)slot * 16 + tid] = a.cams[(size_t)i * 16 + tid];
    if (tid == 0) a.b.ring_times[slot] = a.times[i];
    if (i != 0) return;
    double* st = a.b.state;
    if (tid < J) {
        const int par = a.parents[tid];
        double sum = st[LS_BONE + tid];
        for (int f = 0; f < a.k; ++f) {
            const float* p = a.pose + ((size_t)f * J + tid) * 3;
            const float* q = a.pose + ((size_t)f * J + par) * 3;
            const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
            sum += (double)sqrtf(dx * dx + dy * dy + dz * dz);          // (the expression of mean_bone_kernel)
        }
        st[LS_BONE + tid] = sum;
    }
    if (tid == 64) { st[LS_COUNT] += (double)a.k; st[LS_PUSHED] += (double)a.k; }
}

// grid (T, H + 1): workgroup (i, y < H) copies row y of ring frame first + i into the window buffer; (i, H) the frame's skeleton and
// camera, and (0, H) writes the mean bone lengths of the call.
__global__ __launch_bounds__(LIVE_THREADS) void live_window_kernel(LiveArgs a, float* win_heat, float* win_pose, double* win_cams) {
    const int i = blockIdx.x, y = blockIdx.y, tid = threadIdx.x, J = a.J;
    const int slot = (int)((a.first + i) % LIVE_RING);
    const int row = a.W * J;
    if (y < a.H) {
        live_copy(a.b.ring_heat + ((size_t)slot * a.H + y) * row, win_heat + ((size_t)i * a.H + y) * row, row, a.vec != 0);
        return;
    }
    if (tid < J * 3) win_pose[(size_t)i * J * 3 + tid] = a.b.ring_pose[(size_t)slot * J * 3 + tid];
    if (tid < 16) win_cams[(size_t)i * 16 + tid] = a.b.ring_cams[(size_t)slot * 16 + tid];
    if (i == 0 && tid < J)
        a.mean_bone[tid] = a.bone_fixed ? a.bone_fixed[tid] : (float)(a.b.state[LS_BONE + tid] / a.b.state[LS_COUNT]);
}

// utils/one_euro_filter.py, operation by operation in IEEE float64 (no fused multiply-add): the step shared by the live kernel and
// gem_one_euro.  -> x_hat; x_prev / dx_prev are updated, the caller keeps t_prev.
__device__ __forceinline__ double one_euro_factor(double t_e, double cutoff) {
#pragma clang fp contract(off)
    const double r = 2 * 3.141592653589793 * cutoff * t_e;
    return r / (r + 1);
}

__device__ __forceinline__ double one_euro_step(const double* euro, double t, double t_prev, double x, double& x_prev, double& dx_prev) {
#pragma clang fp contract(off)
    const double t_e = t - t_prev;
    const double a_d = one_euro_factor(t_e, euro[2]);
    const double dx = (x - x_prev) / t_e;
    const double dx_hat = a_d * dx + (1 - a_d) * dx_prev;
    const double cutoff = euro[0] + euro[1] * fabs(dx_hat);
    const double a = one_euro_factor(t_e, cutoff);
    const double x_hat = a * x + (1 - a) * x_prev;
    x_prev = x_hat;
    dx_prev = dx_hat;
    return x_hat;
}

// One workgroup; thread c owns coordinate c = 3 j + d of every frame.
__global__ __launch_bounds__(64) void live_emit_kernel(LiveArgs a) {
    const int c = threadIdx.x, J = a.J, JC = J * 3;
    double* st = a.b.state;
    const bool have_prev0 = st[LS_HAVE_PREV] != 0.0;
    const double t_prev0 = st[LS_TPREV];
    __syncthreads();          // (thread 0 writes those two at the end)
    const int n_out = a.final ? LIVE_HOLD : LIVE_STRIDE;
    double t_last = t_prev0;
    bool have_prev = have_prev0;
    if (c < JC) {
        const int j = c / 3, d = c % 3;
        double x_prev = st[LS_XPREV + c], dx_prev = st[LS_DXPREV + c], t_prev = t_prev0;
        double* out_opt = a.out + c;
        double* out_est = a.out + (size_t)LIVE_STRIDE * JC + c;
        double est_hold[LIVE_HOLD], opt_hold[LIVE_HOLD];
        for (int i = 0; i < (a.final ? LIVE_HOLD : LIVE_T); ++i) {
            double x, e, t;
            if (a.final) {
                x = st[LS_TAIL_OPT + i * LIVE_MAXC + c];
                e = st[LS_TAIL_EST + i * LIVE_MAXC + c];
                t = st[LS_TAIL_T + i];
            } else {
#pragma clang fp contract(off)
                const double* M = a.cams + (size_t)i * 16 + 4 * d;
                const float* p = a.pose + ((size_t)i * J + j) * 3;
                e = M[0] * (double)p[0] + M[1] * (double)p[1] + M[2] * (double)p[2] + M[3];
                x = a.global[(size_t)i * JC + c];
                t = a.b.ring_times[(a.first + i) % LIVE_RING];
                if (i >= LIVE_STRIDE) { opt_hold[i - LIVE_STRIDE] = x; est_hold[i - LIVE_STRIDE] = e; continue; }
                // merge_batches: (w[i][-overlap:] + w[i + 1][:overlap]) / 2
                if (i < LIVE_HOLD && a.first > 0) x = (st[LS_TAIL_OPT + i * LIVE_MAXC + c] + x) / 2;
            }
            if (a.filter) {
                if (!have_prev) { x_prev = x; dx_prev = 0.0; have_prev = true; }          // the first frame passes through
                else x = one_euro_step(a.euro, t, t_prev, x, x_prev, dx_prev);
                t_prev = t;
            }
            out_opt[(size_t)i * JC] = x;
            out_est[(size_t)i * JC] = e;
        }
        t_last = t_prev;
        st[LS_XPREV + c] = x_prev;
        st[LS_DXPREV + c] = dx_prev;
        if (!a.final)
            for (int i = 0; i < LIVE_HOLD; ++i) {
                st[LS_TAIL_OPT + i * LIVE_MAXC + c] = opt_hold[i];
                st[LS_TAIL_EST + i * LIVE_MAXC + c] = est_hold[i];
            }
    }
    if (c == 0) {
        st[LS_TPREV] = t_last;
        st[LS_HAVE_PREV] = have_prev ? 1.0 : 0.0;
        st[LS_EMITTED] += (double)n_out;
        if (a.final) st[LS_HAVE_TAIL] = 0.0;
        else {
            for (int i = 0; i < LIVE_HOLD; ++i) st[LS_TAIL_T + i] = a.b.ring_times[(a.first + LIVE_STRIDE + i) % LIVE_RING];
            st[LS_HAVE_TAIL] = 1.0;
            st[LS_WINDOWS] += 1.0;
        }
    }
}

struct OneEuroArgs {
    const double* seq;
    const double* times;
    double* out;
    int64_t F;
    int n_chunks, JC;
    double euro[3];
};

// one thread per (chunk, coordinate), frames in order
__global__ __launch_bounds__(LIVE_THREADS) void one_euro_kernel(OneEuroArgs a) {
    const int64_t id = (int64_t)blockIdx.x * LIVE_THREADS + threadIdx.x;
    if (id >= (int64_t)a.n_chunks * a.JC) return;
    const int64_t chunk = id / a.JC;
    const int c = (int)(id % a.JC);
    const double* x = a.seq + (size_t)chunk * a.F * a.JC + c;
    const double* t = a.times + (size_t)chunk * a.F;
    double* o = a.out + (size_t)chunk * a.F * a.JC + c;
    double x_prev = x[0], dx_prev = 0.0, t_prev = t[0];
    o[0] = x_prev;
    for (int64_t f = 1; f < a.F; ++f) {
        o[(size_t)f * a.JC] = one_euro_step(a.euro, t[f], t_prev, x[(size_t)f * a.JC], x_prev, dx_prev);
        t_prev = t[f];
    }
}

inline bool live_buffers_ok(const gem_live_buffers* b) {
    return b && b->ring_pose && b->ring_cams && b->ring_times && b->ring_heat && b->state;
}

// the handle's part of a launch: sizes, parents, whether heat-map rows can move as 16-byte vectors
inline int live_args(gem_handle* h, const gem_live_buffers* b, const char* who, LiveArgs* a) {
    if (!h) { set_error(std::string(who) + ": null handle"); return 1; }
    if (!live_buffers_ok(b)) { set_error(std::string(who) + ": null buffer"); return 1; }
    if (h->T != LIVE_T) {
        set_error(std::string(who) + ": live mode works on windows of " + std::to_string(LIVE_T) + " frames, this handle has seq_len " +
                  std::to_string(h->T));
        return 1;
    }
    if (h->J > MAXJ_ERR) { set_error(std::string(who) + ": at most 16 joints"); return 1; }
    *a = LiveArgs();
    a->b = *b;
    a->H = h->cfg.heat_h; a->W = h->cfg.heat_w; a->J = h->J;
    for (int j = 0; j < MAXJ_ERR; ++j) a->parents[j] = j < h->J ? h->cfg.parents[j] : j;
    a->vec = (a->W * a->J) % 4 == 0 && (reinterpret_cast<uintptr_t>(b->ring_heat) & 15) == 0;
    return 0;
}

// the launch of gem_live_window and gem_live_window_at for the frames [first, first + T): the caller has checked them against the ring
inline int live_window_launch(gem_handle* h, LiveArgs& a, int64_t first, const float* d_bone_fixed, float* d_win_pose, double* d_win_cams,
                              float* d_win_heat, float* d_mean_bone, void* stream) {
    GEM_HIP(hipSetDevice(h->cfg.device));
    a.first = first; a.bone_fixed = d_bone_fixed; a.mean_bone = d_mean_bone;
    a.vec = a.vec && (reinterpret_cast<uintptr_t>(d_win_heat) & 15) == 0;
    hipLaunchKernelGGL(live_window_kernel, dim3((unsigned)LIVE_T, (unsigned)a.H + 1), dim3(LIVE_THREADS), 0, static_cast<hipStream_t>(stream), a,
                       d_win_heat, d_win_pose, d_win_cams);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // namespace gem

extern "C" {

int gem_live_push(gem_handle* h, const gem_live_buffers* b, int64_t first_frame, int k, int64_t oldest_needed, const float* d_heat,
                  const float* d_pose, const double* d_cams, const double* d_times, void* stream) {
    using namespace gem;
    LiveArgs a;
    if (live_args(h, b, "gem_live_push", &a)) return 1;
    if (!d_heat || !d_pose || !d_cams || !d_times) { set_error("gem_live_push: null argument"); return 1; }
    if (k < 1 || k > GEM_LIVE_PUSH_MAX) {
        set_error("gem_live_push: between 1 and " + std::to_string(GEM_LIVE_PUSH_MAX) + " frames per call, got " + std::to_string(k)); return 1;
    }
    if (first_frame < 0 || oldest_needed < 0 || oldest_needed > first_frame) {
        set_error("gem_live_push: need 0 <= oldest_needed <= first_frame"); return 1;
    }
    if (first_frame + k - oldest_needed > LIVE_RING) {
        set_error("gem_live_push: ring overrun: frames " + std::to_string(oldest_needed) + " .. " + std::to_string(first_frame + k - 1) +
                  " do not fit the " + std::to_string(LIVE_RING) + " slots (a window still to come reads the oldest)");
        return 1;
    }
    GEM_HIP(hipSetDevice(h->cfg.device));
    a.heat = d_heat; a.pose = d_pose; a.cams = d_cams; a.times = d_times; a.first = first_frame; a.k = k;
    a.vec = a.vec && (reinterpret_cast<uintptr_t>(d_heat) & 15) == 0;
    hipLaunchKernelGGL(live_push_kernel, dim3((unsigned)k, (unsigned)a.H + 1), dim3(LIVE_THREADS), 0, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_live_window(gem_handle* h, const gem_live_buffers* b, int64_t window, int64_t n_pushed, const float* d_bone_fixed,
                    float* d_win_pose, double* d_win_cams, float* d_win_heat, float* d_mean_bone, void* stream) {
    using namespace gem;
    LiveArgs a;
    if (live_args(h, b, "gem_live_window", &a)) return 1;
    if (!d_win_pose || !d_win_cams || !d_win_heat || !d_mean_bone) { set_error("gem_live_window: null argument"); return 1; }
    if (window < 0 || window > (INT64_MAX - LIVE_T) / LIVE_STRIDE) { set_error("gem_live_window: window out of range"); return 1; }
    const int64_t first = window * LIVE_STRIDE;
    if (n_pushed < first + LIVE_T) {
        set_error("gem_live_window: window " + std::to_string(window) + " ends at frame " + std::to_string(first + LIVE_T - 1) + ", only " +
                  std::to_string(n_pushed) + " frames have been pushed");
        return 1;
    }
    if (n_pushed - first > LIVE_RING) {
        set_error("gem_live_window: ring overrun: frame " + std::to_string(first) + " has been overwritten (" + std::to_string(n_pushed) +
                  " frames pushed, " + std::to_string(LIVE_RING) + " slots)");
        return 1;
    }
    return live_window_launch(h, a, first, d_bone_fixed, d_win_pose, d_win_cams, d_win_heat, d_mean_bone, stream);
}

int gem_live_emit(gem_handle* h, const gem_live_buffers* b, int64_t window, int final, const double* d_global, const float* d_win_pose,
                  const double* d_win_cams, const double* h_one_euro, double* d_out, void* stream) {
    using namespace gem;
    LiveArgs a;
    if (live_args(h, b, "gem_live_emit", &a)) return 1;
    if (!d_out || (!final && (!d_global || !d_win_pose || !d_win_cams))) { set_error("gem_live_emit: null argument"); return 1; }
    if (window < 0 || window > (INT64_MAX - LIVE_T) / LIVE_STRIDE) { set_error("gem_live_emit: window out of range"); return 1; }
    if (h_one_euro) {
        for (int i = 0; i < 3; ++i) {
            if (!(h_one_euro[i] >= 0.0) || h_one_euro[i] > 1e300) { set_error("gem_live_emit: the filter's parameters must be finite and not negative"); return 1; }
            a.euro[i] = h_one_euro[i];
        }
        a.filter = 1;
    }
    GEM_HIP(hipSetDevice(h->cfg.device));
    a.first = window * LIVE_STRIDE; a.final = final ? 1 : 0; a.global = d_global; a.pose = d_win_pose; a.cams = d_win_cams; a.out = d_out;
    hipLaunchKernelGGL(live_emit_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_one_euro(const double* d_seq, const double* d_times, int n_chunks, int64_t frames_per_chunk, int n_coords, const double* h_params,
                 double* d_out, void* stream) {
    using namespace gem;
    if (n_chunks < 0 || frames_per_chunk < 0 || n_coords < 1) {
        set_error("gem_one_euro: need n_chunks >= 0, frames_per_chunk >= 0 and n_coords >= 1"); return 1;
    }
    if (n_chunks == 0 || frames_per_chunk == 0) return 0;
    if (!d_seq || !d_times || !d_out || !h_params) { set_error("gem_one_euro: null argument"); return 1; }
    if ((int64_t)n_chunks * n_coords > 0x7fffffffLL * LIVE_THREADS / 2) { set_error("gem_one_euro: too many chunks x coordinates for one call"); return 1; }
    OneEuroArgs a;
    a.seq = d_seq; a.times = d_times; a.out = d_out; a.F = frames_per_chunk; a.n_chunks = n_chunks; a.JC = n_coords;
    for (int i = 0; i < 3; ++i) {
        if (!(h_params[i] >= 0.0) || h_params[i] > 1e300) { set_error("gem_one_euro: the filter's parameters must be finite and not negative"); return 1; }
        a.euro[i] = h_params[i];
    }
    const int64_t n = (int64_t)n_chunks * n_coords;
    hipLaunchKernelGGL(one_euro_kernel, dim3((unsigned)((n + LIVE_THREADS - 1) / LIVE_THREADS)), dim3(LIVE_THREADS), 0,
                       static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------- dense live mode
// Live mode at a stride k below 8, and the `now` stream ("Dense live mode"; gem_live_dense.h has the layout of
// the dense state block).
//
//   gem_live_window_at    gem_live_window for any first frame (the same kernel, the same ring checks)
//   gem_live_emit_dense   the window's 10 frames onto the per-frame sums, the `now` frames (the window's newest k, all 10 of window 0;
//                         One-Euro filtered in frame order when asked), the k frames no later window covers as sum / count, their
//                         estimated frames; `final`: the 10 - k frames still held, each over its own count
//   gem_merge_dense       the offline twin: every frame the mean of all windows that cover it, at any stride 1 .. T
//
// Sums run over the covering windows oldest first, one thread per coordinate, no atomics: the same bits on every call.
namespace gem {

constexpr int LIVE_SLOTS = GEM_LIVE_DENSE_SLOTS;
constexpr int LD_TPREV = 0, LD_HAVE_PREV = 1, LD_WINDOWS = 2, LD_SETTLED = 3, LD_NOW = 4, LD_COUNT = 16, LD_XPREV = LD_COUNT + LIVE_SLOTS,
              LD_DXPREV = LD_XPREV + LIVE_MAXC, LD_SUM = LD_DXPREV + LIVE_MAXC, LD_EST = LD_SUM + LIVE_SLOTS * LIVE_MAXC;
static_assert(LD_EST + LIVE_SLOTS * LIVE_MAXC == GEM_LIVE_DENSE_DOUBLES, "the dense state block's layout and its size disagree");
static_assert((LIVE_SLOTS & (LIVE_SLOTS - 1)) == 0 && LIVE_T <= LIVE_SLOTS, "a window's frames lie in distinct slots, slot = frame mod a power of two");

struct LiveDenseArgs {
    const double* ring_times;  // the session's ring of timestamps
    double* st;                // the dense state block
    const double* global;      // [T,J,3] the window's result
    const float* pose;         // [T,J,3] the window buffer
    const double* cams;        // [T,4,4] the window buffer
    double* out;               // [3][T][JC]: settled, estimated, now
    int64_t first;             // the window's first frame, stride * window
    int stride, J, final, filter, all_now;
    double euro[3];
};

// One workgroup; thread c owns coordinate c = 3 j + d of every frame.
__global__ __launch_bounds__(64) void live_emit_dense_kernel(LiveDenseArgs a) {
    const int c = threadIdx.x, J = a.J, JC = J * 3, k = a.stride;
    double* st = a.st;
    const bool have_prev0 = st[LD_HAVE_PREV] != 0.0;
    const double t_prev0 = st[LD_TPREV];
    const int n_frames = a.final ? LIVE_T - k : LIVE_T;
    double cnt[LIVE_T];
    for (int i = 0; i < n_frames; ++i) cnt[i] = st[LD_COUNT + (int)((a.first + i) & (LIVE_SLOTS - 1))];
    __syncthreads();          // (thread 0 writes the counts and the filter's two scalars at the end)
    double t_last = t_prev0;
    bool have_prev = have_prev0;
    const int n_now = a.final ? 0 : (a.all_now ? LIVE_T : k);
    if (c < JC) {
        const int j = c / 3, d = c % 3;
        double* out_set = a.out + c;
        double* out_est = a.out + (size_t)LIVE_T * JC + c;
        double* out_now = a.out + (size_t)2 * LIVE_T * JC + c;
        if (a.final) {
            for (int i = 0; i < n_frames; ++i) {
                const int slot = (int)((a.first + i) & (LIVE_SLOTS - 1));
                out_set[(size_t)i * JC] = st[LD_SUM + slot * LIVE_MAXC + c] / cnt[i];
                out_est[(size_t)i * JC] = st[LD_EST + slot * LIVE_MAXC + c];
                st[LD_SUM + slot * LIVE_MAXC + c] = 0.0;
            }
        } else {
            double x_prev = st[LD_XPREV + c], dx_prev = st[LD_DXPREV + c], t_prev = t_prev0;
            for (int i = 0; i < LIVE_T; ++i) {
#pragma clang fp contract(off)
                const int slot = (int)((a.first + i) & (LIVE_SLOTS - 1));
                const double* M = a.cams + (size_t)i * 16 + 4 * d;
                const float* p = a.pose + ((size_t)i * J + j) * 3;
                const double e = M[0] * (double)p[0] + M[1] * (double)p[1] + M[2] * (double)p[2] + M[3];
                double x = a.global[(size_t)i * JC + c];
                // the covering windows oldest first: the first one is taken as it is (no 0 + x, which would lose the sign of -0)
                const double sum = cnt[i] == 0.0 ? x : st[LD_SUM + slot * LIVE_MAXC + c] + x;
                if (i < k) {          // no later window covers frame first + i
                    out_set[(size_t)i * JC] = sum / (cnt[i] + 1.0);
                    out_est[(size_t)i * JC] = e;
                    st[LD_SUM + slot * LIVE_MAXC + c] = 0.0;
                } else {
                    st[LD_SUM + slot * LIVE_MAXC + c] = sum;
                    st[LD_EST + slot * LIVE_MAXC + c] = e;
                }
                if (i >= LIVE_T - n_now) {
                    if (a.filter) {
                        const double t = a.ring_times[(a.first + i) % LIVE_RING];
                        if (!have_prev) { x_prev = x; dx_prev = 0.0; have_prev = true; }          // the first frame passes through
                        else x = one_euro_step(a.euro, t, t_prev, x, x_prev, dx_prev);
                        t_prev = t;
                    }
                    out_now[(size_t)(i - (LIVE_T - n_now)) * JC] = x;
                }
            }
            t_last = t_prev;
            st[LD_XPREV + c] = x_prev;
            st[LD_DXPREV + c] = dx_prev;
        }
    }
    if (c == 0) {
        for (int i = 0; i < n_frames; ++i)
            st[LD_COUNT + (int)((a.first + i) & (LIVE_SLOTS - 1))] = (a.final || i < k) ? 0.0 : cnt[i] + 1.0;
        st[LD_TPREV] = t_last;
        st[LD_HAVE_PREV] = have_prev ? 1.0 : 0.0;
        st[LD_SETTLED] += (double)(a.final ? LIVE_T - k : k);
        st[LD_NOW] += (double)n_now;
        if (!a.final) st[LD_WINDOWS] += 1.0;
    }
}

struct MergeDenseArgs {
    const double* win;
    double* out;
    int64_t n;                 // n_chunks * frames_per_chunk * JC
    int64_t fpc;
    int wpc, T, JC, stride;
};

// one thread per (chunk, frame, coordinate): the covering windows in ascending order
__global__ __launch_bounds__(LIVE_THREADS) void merge_dense_kernel(MergeDenseArgs a) {
    const int64_t id = (int64_t)blockIdx.x * LIVE_THREADS + threadIdx.x;
    if (id >= a.n) return;
    const int c = (int)(id % a.JC);
    const int64_t f = (id / a.JC) % a.fpc, chunk = id / a.JC / a.fpc;
    const int64_t lo = f < a.T ? 0 : (f - a.T) / a.stride + 1;          // the first window with lo * stride + T > f
    const int64_t hi = f / a.stride < a.wpc - 1 ? f / a.stride : a.wpc - 1;
    const double* w = a.win + (size_t)chunk * a.wpc * a.T * a.JC + c;
    double sum = w[((size_t)lo * a.T + (size_t)(f - lo * a.stride)) * a.JC];
    for (int64_t i = lo + 1; i <= hi; ++i) sum += w[((size_t)i * a.T + (size_t)(f - i * a.stride)) * a.JC];
    a.out[id] = sum / (double)(hi - lo + 1);
}

}  // namespace gem

extern "C" {

int gem_live_window_at(gem_handle* h, const gem_live_buffers* b, int64_t first_frame, int64_t n_pushed, const float* d_bone_fixed,
                       float* d_win_pose, double* d_win_cams, float* d_win_heat, float* d_mean_bone, void* stream) {
    using namespace gem;
    LiveArgs a;
    if (live_args(h, b, "gem_live_window_at", &a)) return 1;
    if (!d_win_pose || !d_win_cams || !d_win_heat || !d_mean_bone) { set_error("gem_live_window_at: null argument"); return 1; }
    if (first_frame < 0 || first_frame > INT64_MAX - LIVE_T) { set_error("gem_live_window_at: first frame out of range"); return 1; }
    if (n_pushed < first_frame + LIVE_T) {
        set_error("gem_live_window_at: the window ends at frame " + std::to_string(first_frame + LIVE_T - 1) + ", only " +
                  std::to_string(n_pushed) + " frames have been pushed");
        return 1;
    }
    if (n_pushed - first_frame > LIVE_RING) {
        set_error("gem_live_window_at: ring overrun: frame " + std::to_string(first_frame) + " has been overwritten (" +
                  std::to_string(n_pushed) + " frames pushed, " + std::to_string(LIVE_RING) + " slots)");
        return 1;
    }
    return live_window_launch(h, a, first_frame, d_bone_fixed, d_win_pose, d_win_cams, d_win_heat, d_mean_bone, stream);
}

int gem_live_emit_dense(gem_handle* h, const gem_live_buffers* b, double* d_dense_state, int stride, int64_t window, int final,
                        const double* d_global, const float* d_win_pose, const double* d_win_cams, const double* h_one_euro, double* d_out,
                        void* stream) {
    using namespace gem;
    LiveArgs la;
    if (live_args(h, b, "gem_live_emit_dense", &la)) return 1;
    if (!d_dense_state || !d_out || (!final && (!d_global || !d_win_pose || !d_win_cams))) { set_error("gem_live_emit_dense: null argument"); return 1; }
    if (stride < 1 || stride > LIVE_STRIDE) {
        set_error("gem_live_emit_dense: the stride is between 1 and " + std::to_string(LIVE_STRIDE) + " frames, got " + std::to_string(stride)); return 1;
    }
    if (window < 0 || window > (INT64_MAX - LIVE_T) / LIVE_STRIDE) { set_error("gem_live_emit_dense: window out of range"); return 1; }
    LiveDenseArgs a = LiveDenseArgs();
    if (h_one_euro) {
        for (int i = 0; i < 3; ++i) {
            if (!(h_one_euro[i] >= 0.0) || h_one_euro[i] > 1e300) { set_error("gem_live_emit_dense: the filter's parameters must be finite and not negative"); return 1; }
            a.euro[i] = h_one_euro[i];
        }
        a.filter = 1;
    }
    GEM_HIP(hipSetDevice(h->cfg.device));
    a.ring_times = b->ring_times; a.st = d_dense_state; a.global = d_global; a.pose = d_win_pose; a.cams = d_win_cams; a.out = d_out;
    a.first = window * stride; a.stride = stride; a.J = la.J; a.final = final ? 1 : 0; a.all_now = window == 0;
    hipLaunchKernelGGL(live_emit_dense_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_merge_dense(const double* d_windows, int n_chunks, int windows_per_chunk, int T, int n_coords, int stride, double* d_out, void* stream) {
    using namespace gem;
    if (n_chunks < 0 || windows_per_chunk < 1 || T < 1 || n_coords < 1 || stride < 1 || stride > T) {
        set_error("gem_merge_dense: need n_chunks >= 0, windows_per_chunk >= 1, n_coords >= 1 and 1 <= stride <= T"); return 1;
    }
    if (n_chunks == 0) return 0;
    if (!d_windows || !d_out) { set_error("gem_merge_dense: null argument"); return 1; }
    MergeDenseArgs a;
    a.win = d_windows; a.out = d_out; a.wpc = windows_per_chunk; a.T = T; a.JC = n_coords; a.stride = stride;
    a.fpc = (int64_t)(windows_per_chunk - 1) * stride + T;
    // (the input is the larger of the two arrays: with it below 2^40 doubles no index above overflows)
    if ((int64_t)n_chunks * windows_per_chunk > (((int64_t)1 << 40) / T) / n_coords) { set_error("gem_merge_dense: too many windows for one call"); return 1; }
    a.n = (int64_t)n_chunks * a.fpc * n_coords;
    if ((a.n + LIVE_THREADS - 1) / LIVE_THREADS > 0x7fffffffLL) { set_error("gem_merge_dense: too many frames x coordinates for one call"); return 1; }
    hipLaunchKernelGGL(merge_dense_kernel, dim3((unsigned)((a.n + LIVE_THREADS - 1) / LIVE_THREADS)), dim3(LIVE_THREADS), 0,
                       static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
