// Training windows of the motion VAEs cut on the device from resident source frames (the reference cuts
// them on the host: networks/dataset/global_dataset.py:82-110, local_dataset.py:82-98).
//   gem_motion_cameras   once at load time: every frame's {'loc', 'rot'} -> the float64 rigid matrix [R(q) | loc] of
//                        utils/utils.py:33-42 (scipy's Rotation.from_quat: the quaternion, x y z w, divided by its norm first)
//   gem_motion_windows   per batch (or once over every window): window ids -> [B, T, 45] f32 straight into the caller's buffer.
//                        The sequence of an id comes from a binary search over the [S+1] window prefix (no per-window table).
//                        Global: inv(C_i) . C_{i+k*timer} . [x; 1] in float64 (rigid inverse), every windows_size-th of the
//                        frame_num * windows_size frames; local: the frame_num * windows_size frames as they are.  One rounding
//                        to float32, at the store.
// Included from train.hip (the build's source list stays as it is).
#pragma once

namespace gem {

constexpr int MW_ROWS = 256;           // output rows (window, frame) per workgroup: one per thread in the first phase

// Source frame k * timer of window `id` (-1: no such window).  Its sequence is the largest s < n_seq with window0[s] <= id (empty
// sequences repeat the prefix value and are skipped); windows start every `interval` frames, or every total * timer[s] (interval 0)
__device__ inline int64_t mw_frame_of(int64_t id, const int64_t* __restrict__ frame0, const int64_t* __restrict__ window0,
                                      const int32_t* __restrict__ timer, int n_seq, int64_t interval, int64_t total, int64_t k,
                                      int64_t* first) {
    if (id < 0 || id >= window0[n_seq]) return -1;
    int lo = 0, hi = n_seq;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (window0[mid] <= id) lo = mid; else hi = mid;
    }
    const int64_t base = frame0[lo] + (id - window0[lo]) * (interval > 0 ? interval : total * timer[lo]);
    *first = base;
    return base + k * (int64_t)timer[lo];
}

// scipy's from_quat(q).as_matrix() (normalised first), float64, with its own operation order; cam34 [n][3][4] = [R | loc]
__global__ __launch_bounds__(256) void motion_cameras_kernel(const double* __restrict__ loc, const double* __restrict__ quat,
                                                             int64_t n, double* __restrict__ cam) {
#pragma clang fp contract(off)
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    const double qx = quat[f * 4], qy = quat[f * 4 + 1], qz = quat[f * 4 + 2], qw = quat[f * 4 + 3];
    const double nrm = sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
    const double x = qx / nrm, y = qy / nrm, z = qz / nrm, w = qw / nrm;
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    double* c = cam + f * 12;
    c[0] = x2 - y2 - z2 + w2;   c[1] = 2 * (xy - zw);        c[2] = 2 * (xz + yw);         c[3] = loc[f * 3];
    c[4] = 2 * (xy + zw);       c[5] = -x2 + y2 - z2 + w2;   c[6] = 2 * (yz - xw);         c[7] = loc[f * 3 + 1];
    c[8] = 2 * (xz - yw);       c[9] = 2 * (yz + xw);        c[10] = -x2 - y2 + z2 + w2;   c[11] = loc[f * 3 + 2];
}

// grid ceil(B * T / MW_ROWS), 256 threads.  Phase 1: thread r owns output row r0 + r = (window b, frame t): its source frame and (global)
// the composed [A | b] = inv(C_first) . C_frame as float64 in LDS.  Phase 2: the workgroup's rows * 45 floats, one per thread per
// pass, consecutive threads on consecutive floats.  Rows of an id outside [0, n_windows) are NaN.
template <bool GLOBAL>
__global__ __launch_bounds__(256) void motion_windows_kernel(const double* __restrict__ pose, const double* __restrict__ cam,
                                                             const int64_t* __restrict__ frame0, const int64_t* __restrict__ window0,
                                                             const int32_t* __restrict__ timer, int n_seq, int64_t interval, int T,
                                                             int step, const int64_t* __restrict__ ids, int64_t B,
                                                             float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double mat[GLOBAL ? MW_ROWS * 12 : 1];
    __shared__ int64_t src[MW_ROWS];
    const int64_t rows = B * T, r0 = (int64_t)blockIdx.x * MW_ROWS;
    const int nr = (int)(rows - r0 < MW_ROWS ? rows - r0 : MW_ROWS);
    if ((int)threadIdx.x < nr) {
        const int64_t row = r0 + threadIdx.x, b = row / T, t = row - b * T;
        int64_t first = 0;
        const int64_t f = mw_frame_of(ids[b], frame0, window0, timer, n_seq, interval, (int64_t)T * step, t * step, &first);
        src[threadIdx.x] = f;
        if (GLOBAL && f >= 0) {
            // inverse of the rigid [R0 | l0]: [R0^T | -R0^T l0]; composed with [Ri | li]: A = R0^T Ri, b = R0^T li - R0^T l0
            const double* c0 = cam + first * 12;
            const double* ci = cam + f * 12;
            double* m = mat + threadIdx.x * 12;
            for (int r = 0; r < 3; ++r) {
                const double a0 = c0[r], a1 = c0[4 + r], a2 = c0[8 + r];          // row r of R0^T = column r of R0
                for (int c = 0; c < 4; ++c) m[r * 4 + c] = a0 * ci[c] + a1 * ci[4 + c] + a2 * ci[8 + c];
                m[r * 4 + 3] = m[r * 4 + 3] + (-(a0 * c0[3] + a1 * c0[7] + a2 * c0[11]));
            }
        }
    }
    __syncthreads();
    const int64_t e0 = r0 * 45, ne = (int64_t)nr * 45;
    for (int e = threadIdx.x; e < ne; e += 256) {
        const int r = e / 45, jc = e - r * 45;
        const int64_t f = src[r];
        float v;
        if (f < 0) {
            v = __builtin_nanf("");
        } else if (GLOBAL) {
            const int c = jc % 3;
            const double* x = pose + f * 45 + (jc - c);
            const double* m = mat + r * 12 + c * 4;
            v = (float)(m[0] * x[0] + m[1] * x[1] + m[2] * x[2] + m[3]);
        } else {
            v = (float)pose[f * 45 + jc];
        }
        out[e0 + e] = v;
    }
}

}  // namespace gem

extern "C" {

int gem_motion_cameras(const double* d_loc, const double* d_quat, int64_t n_frames, double* d_cam34, void* stream) {
    if (n_frames == 0) return 0;
    if (!d_loc || !d_quat || !d_cam34 || n_frames < 0) { gem::set_error("gem_motion_cameras: bad argument"); return 1; }
    if (n_frames > (int64_t)0xffffffff * 256) { gem::set_error("gem_motion_cameras: too many frames for one launch"); return 1; }
    hipLaunchKernelGGL(gem::motion_cameras_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_loc, d_quat, n_frames, d_cam34);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_motion_windows(const double* d_pose, const double* d_cam34, const int64_t* d_seq_frame0, const int64_t* d_seq_window0,
                       const int32_t* d_seq_timer, int n_seq, int64_t interval, int frame_num, int windows_size,
                       const int64_t* d_ids, int64_t B, float* d_out, void* stream) {
    if (B == 0) return 0;
    if (!d_pose || !d_seq_frame0 || !d_seq_window0 || !d_seq_timer || !d_ids || !d_out || B < 0 || n_seq < 1) {
        gem::set_error("gem_motion_windows: bad argument"); return 1;
    }
    if (interval < 0 || frame_num < 1 || windows_size < 1 || (int64_t)frame_num * windows_size > 65536) {
        gem::set_error("gem_motion_windows: need interval >= 0, frame_num >= 1, windows_size >= 1, frame_num * windows_size <= 65536");
        return 1;
    }
    if (reinterpret_cast<uintptr_t>(d_out) & 3) { gem::set_error("gem_motion_windows: the output must be 4-byte aligned"); return 1; }
    // global: frame_num frames, every windows_size-th; local: all frame_num * windows_size frames (local_dataset.py:93-96)
    const int T = d_cam34 ? frame_num : frame_num * windows_size, step = d_cam34 ? windows_size : 1;
    const int64_t blocks = (B * T + gem::MW_ROWS - 1) / gem::MW_ROWS;
    if (B > ((int64_t)1 << 40) / T || blocks > 0x7fffffff) { gem::set_error("gem_motion_windows: too many windows for one launch"); return 1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d_cam34)
        hipLaunchKernelGGL(gem::motion_windows_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, d_pose, d_cam34, d_seq_frame0,
                           d_seq_window0, d_seq_timer, n_seq, interval, T, step, d_ids, B, d_out);
    else
        hipLaunchKernelGGL(gem::motion_windows_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, d_pose, d_cam34, d_seq_frame0,
                           d_seq_window0, d_seq_timer, n_seq, interval, T, step, d_ids, B, d_out);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
