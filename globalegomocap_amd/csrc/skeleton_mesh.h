// Skeleton meshes as PLY files from the device: what the reference's --save writes frame by frame with
// open3d (optimizer.py:485-504 -> save_mesh -> Skeleton.joints_2_mesh, utils/skeleton.py:142-158, utils/pose_visualization_utils.py).
// Included from errors.hip.
//
//   gem_skeleton_mesh_layout    the counts and byte sizes of one file                                        (host)
//   gem_skeleton_mesh_constant  the header and the face block, the same for every frame                      (host)
//   gem_sequence_align          (c, R, t) of the similarity that takes one sequence onto another, all frames at once
//   gem_skeleton_mesh           the vertex block of every frame: 12 960 records of 27 bytes (3 x f64 + 3 x u8), as the file holds them
//
// A frame is 15 spheres (radius 0.02 m, 762 vertices) on the joints and 15 cylinders (radius 0.005 m, 102 vertices) along
// MESH_LINES.  The kernel turns 360 bytes of joints into 349 920 bytes of file: it is bound by its stores.  The 27-byte records
// are not aligned to anything, so no record is stored as such: a thread computes FOUR consecutive vertices -- 108 bytes, 27 whole
// 32-bit words, every field's shift known at compile time -- and puts the words into LDS; a workgroup's 480 vertices are 12 960
// bytes = 810 x 16, which all its threads then stream out as aligned 16-byte stores, a wavefront's stores contiguous.  One frame
// is 27 such workgroups, so that a sequence of ten frames already occupies every CU.  The two unit templates (sphere directions,
// the cylinder's ring) are a 19 KB table that the host fills once with libm's sin / cos and every workgroup reads through L2.
#pragma once
#include <cmath>
#include <cstring>
#include <mutex>

#include "umeyama_device.h"

namespace gem {

constexpr int MESH_J = 15, MESH_L = 15;                     // joints, lines
constexpr int SPH_V = 762, SPH_T = 1520;                    // create_sphere(resolution 20)
constexpr int CYL_V = 102, CYL_T = 200;                     // create_cylinder(resolution 20, split 4)
constexpr int MESH_V = MESH_J * SPH_V + MESH_L * CYL_V;     // 12 960
constexpr int MESH_T = MESH_J * SPH_T + MESH_L * CYL_T;     // 25 800
constexpr int MESH_REC = 27, MESH_FACE = 13;
constexpr int64_t MESH_VERTEX_BYTES = (int64_t)MESH_V * MESH_REC;        // 349 920
constexpr int64_t MESH_FACE_BYTES = (int64_t)MESH_T * MESH_FACE;         // 335 400
constexpr double SPH_R = 0.02, CYL_R = 0.005;
constexpr uint32_t SPH_RGB = 26u | (26u << 8) | (179u << 16);           // (0.1, 0.1, 0.7) * 255, rounded half up
constexpr uint32_t CYL_RGB = 26u | (230u << 8) | (26u << 16);           // (0.1, 0.9, 0.1)
// Skeleton.lines (utils/skeleton.py:20-21): the 14 bones and (7, 11); skeleton.py's MESH_LINES
constexpr int MESH_LINES[MESH_L][2] = {{0, 1}, {0, 4}, {1, 2}, {2, 3}, {4, 5}, {5, 6}, {1, 7}, {4, 11}, {7, 8}, {8, 9}, {9, 10},
                                       {11, 12}, {12, 13}, {13, 14}, {7, 11}};
static const char MESH_HEADER[] =
    "ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\nelement vertex 12960\nproperty double x\nproperty double y\n"
    "property double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face 25800\n"
    "property list uchar uint vertex_indices\nend_header\n";
constexpr int64_t MESH_HEADER_BYTES = sizeof(MESH_HEADER) - 1;

constexpr int MESH_GROUP = 4;                               // vertices per thread: 4 x 27 bytes = 27 words
constexpr int MESH_SLICE_V = 480;                           // vertices per workgroup: 12 960 bytes = 810 x 16
constexpr int MESH_SLICES = MESH_V / MESH_SLICE_V;          // 27
constexpr int MESH_THREADS = 128;
constexpr int MESH_SLICE_WORDS = MESH_SLICE_V * MESH_REC / 4;
static_assert(MESH_V % MESH_SLICE_V == 0 && MESH_SLICE_V % MESH_GROUP == 0 && (MESH_SLICE_V * MESH_REC) % 16 == 0, "slices are whole 16-byte runs");
static_assert(MESH_SLICE_V / MESH_GROUP <= MESH_THREADS && MESH_VERTEX_BYTES % 16 == 0, "one group per thread");

// unit sphere [762][3], then the ring (cos, sin) [20][2]
constexpr int MESH_TABLE = SPH_V * 3 + 40;
__device__ double mesh_table[MESH_TABLE];

inline void mesh_fill_table(double* t) {
    t[0] = 0.0; t[1] = 0.0; t[2] = 1.0;
    t[3] = 0.0; t[4] = 0.0; t[5] = -1.0;
    for (int i = 1; i <= 19; ++i)
        for (int j = 0; j < 40; ++j) {
            double* v = t + 3 * (2 + 40 * (i - 1) + j);
            const double th = i * M_PI / 20, ph = j * M_PI / 20;
            v[0] = std::sin(th) * std::cos(ph);
            v[1] = std::sin(th) * std::sin(ph);
            v[2] = std::cos(th);
        }
    for (int j = 0; j < 20; ++j) {
        t[SPH_V * 3 + 2 * j] = std::cos(j * 2 * M_PI / 20);
        t[SPH_V * 3 + 2 * j + 1] = std::sin(j * 2 * M_PI / 20);
    }
}

struct MeshArgs {
    const double* seq;         // [F,15,3]
    const double* crt;         // [13] c, R row-major, t -- or nullptr
    unsigned char* out;
    int64_t stride;
    int lines[MESH_L][2];
};

// The cylinder of the line from joint s to joint e: bone = its rotation R (row-major, takes +z onto the line) and its centre, *bh its height
__device__ inline void mesh_bone(const double* s, const double* e, double* bone, double* bh) {
    const double d[3] = {e[0] - s[0], e[1] - s[1], e[2] - s[2]};
    const double h = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (h != 0.0) {          // (a zero-length bone keeps the identity: the reference divides 0 by 0 here)
        const double bx = d[0] / h, by = d[1] / h, bz = d[2] / h;
        const double c1 = 1.0 + bz;
        if (c1 <= 0x1p-40) {          // along -z: a half turn about x (the reference: 0 / 0)
            R[4] = -1.0; R[8] = -1.0;
        } else {
            // rotation_matrix_from_vectors((0,0,1), b): v = z x b = (-by, bx, 0), K = [v]x, R = I + K + K K / (1 + c)
            // (the reference's (1 - c) / s^2 is 1 / (1 + c), without its 0 / 0 on the axis); NaN passes through
            const double k = 1.0 / c1;
            R[0] = 1.0 - bx * bx * k; R[1] = -(bx * by) * k;     R[2] = bx;
            R[3] = -(bx * by) * k;    R[4] = 1.0 - by * by * k;  R[5] = by;
            R[6] = -bx;               R[7] = -by;                R[8] = 1.0 - (bx * bx + by * by) * k;
        }
    }
    for (int i = 0; i < 9; ++i) bone[i] = R[i];
    for (int i = 0; i < 3; ++i) bone[9 + i] = (s[i] + e[i]) / 2;
    *bh = h;
}

// Vertex v of a frame: its position and its colour word.  jt: the frame's joints; bone: per line R (row-major) and the centre; bh: heights.
__device__ inline void mesh_vertex(int v, const double (*jt)[3], const double (*bone)[12], const double* bh, double* o, uint32_t* rgb) {
    if (v < MESH_J * SPH_V) {
        const int j = v / SPH_V, k = v - j * SPH_V;
        const double* u = mesh_table + 3 * k;
        for (int d = 0; d < 3; ++d) o[d] = SPH_R * u[d] + jt[j][d];
        *rgb = SPH_RGB;
    } else {
        const int w = v - MESH_J * SPH_V, l = w / CYL_V, k = w - l * CYL_V;
        const double h = bh[l];
        double x = 0.0, y = 0.0, z;
        if (k < 2) {
            z = k == 0 ? h / 2 : -h / 2;
        } else {
            const int i = (k - 2) / 20, j = (k - 2) - 20 * i;
            x = CYL_R * mesh_table[SPH_V * 3 + 2 * j];
            y = CYL_R * mesh_table[SPH_V * 3 + 2 * j + 1];
            z = h / 2 - i * h / 4;
        }
        const double* R = bone[l];
        for (int d = 0; d < 3; ++d) o[d] = R[3 * d] * x + R[3 * d + 1] * y + R[3 * d + 2] * z + R[9 + d];
        *rgb = CYL_RGB;
    }
}

__global__ __launch_bounds__(MESH_THREADS) void skeleton_mesh_kernel(MeshArgs a) {
    __shared__ double jt[MESH_J][3];
    __shared__ double bone[MESH_L][12];
    __shared__ double bh[MESH_L];
    __shared__ __attribute__((aligned(16))) uint32_t rec[MESH_SLICE_WORDS];
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x / MESH_SLICES;
    const int slice = blockIdx.x - (int)f * MESH_SLICES;
    if (tid < MESH_J) {
        const double* p = a.seq + (f * MESH_J + tid) * 3;
        double q[3] = {p[0], p[1], p[2]};
        if (a.crt) {          // c * (p . R) + t, the row-vector convention of errors.align_sequence
            const double c = a.crt[0];
            const double* R = a.crt + 1;
            const double* t = a.crt + 10;
            const double p0 = q[0], p1 = q[1], p2 = q[2];
            for (int d = 0; d < 3; ++d) q[d] = c * (p0 * R[d] + p1 * R[3 + d] + p2 * R[6 + d]) + t[d];
        }
        for (int d = 0; d < 3; ++d) jt[tid][d] = q[d];
    }
    __syncthreads();
    if (tid < MESH_L) mesh_bone(jt[a.lines[tid][0]], jt[a.lines[tid][1]], bone[tid], &bh[tid]);
    __syncthreads();
    if (tid < MESH_SLICE_V / MESH_GROUP) {
        uint32_t w[MESH_GROUP * MESH_REC / 4 + 1];          // 27 words (+ one that only ever receives zeros)
#pragma unroll
        for (int i = 0; i < MESH_GROUP * MESH_REC / 4 + 1; ++i) w[i] = 0u;
        const int v0 = slice * MESH_SLICE_V + tid * MESH_GROUP;
#pragma unroll
        for (int k = 0; k < MESH_GROUP; ++k) {
            double o[3];
            uint32_t dw[7];
            mesh_vertex(v0 + k, jt, bone, bh, o, &dw[6]);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(o[d]);
                dw[2 * d] = (uint32_t)bits;
                dw[2 * d + 1] = (uint32_t)(bits >> 32);
            }
            const int at = MESH_REC * k, base = at / 4, sh = 8 * (at % 4);          // compile-time after unrolling
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                w[base + i] |= dw[i] << sh;
                if (sh != 0) w[base + i + 1] |= dw[i] >> (32 - sh);
            }
        }
#pragma unroll
        for (int i = 0; i < MESH_GROUP * MESH_REC / 4; ++i) rec[tid * (MESH_GROUP * MESH_REC / 4) + i] = w[i];          // stride 27 words: no bank conflicts
    }
    __syncthreads();
    typedef uint32_t mesh_u4 __attribute__((ext_vector_type(4)));
    mesh_u4* dst = reinterpret_cast<mesh_u4*>(a.out + f * a.stride + (int64_t)slice * (MESH_SLICE_V * MESH_REC));
    const mesh_u4* src = reinterpret_cast<const mesh_u4*>(rec);
    for (int i = tid; i < MESH_SLICE_WORDS / 4; i += MESH_THREADS) __builtin_nontemporal_store(src[i], dst + i);
}

// (c, R, t) of calculate_errors.global_align_skeleton_seq: the sums of errors_sequence_kernel, one workgroup
__global__ __launch_bounds__(ERR_ST) void sequence_align_kernel(const double* P, const double* Q, size_t N, double* crt) {
    __shared__ double red[2 * 16 * ERR_NW];
    int parity = 0;
    double m[6], c[10];
    sequence_moments(P, Q, N, threadIdx.x, red, parity, m, c);
    if (threadIdx.x == 0) {
        Sim3 sim;
        double s, R[9];
        umeyama_moments_t<true>(m, m + 3, c, c[9], &sim, &s, R);          // (its t: what the error report applies)
        crt[0] = s;
        for (int i = 0; i < 9; ++i) crt[1 + i] = R[i];
        for (int i = 0; i < 3; ++i) crt[10 + i] = sim.t[i];
    }
}

inline void mesh_put_triangle(unsigned char*& p, uint32_t off, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t v[3] = {off + a, off + b, off + c};
    *p++ = 3;
    std::memcpy(p, v, 12);          // (little-endian host, like every reader of this library's files)
    p += 12;
}

// the unit templates on the current device: filled once on the host (libm), uploaded once per device
inline int mesh_upload_table() {
    static std::mutex mu;
    static bool uploaded[64] = {};
    static double table[MESH_TABLE];
    static bool filled = false;
    int dev = 0;
    GEM_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (!filled) { mesh_fill_table(table); filled = true; }
    if (dev < 0 || dev >= 64 || !uploaded[dev]) {
        GEM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(mesh_table), table, sizeof(table)));
        if (dev >= 0 && dev < 64) uploaded[dev] = true;
    }
    return 0;
}

}  // namespace gem

extern "C" {

int gem_skeleton_mesh_layout(int64_t* out) {
    using namespace gem;
    if (!out) { set_error("gem_skeleton_mesh_layout: null argument"); return 1; }
    out[0] = MESH_V; out[1] = MESH_T; out[2] = MESH_HEADER_BYTES; out[3] = MESH_VERTEX_BYTES; out[4] = MESH_FACE_BYTES;
    out[5] = MESH_HEADER_BYTES + MESH_VERTEX_BYTES + MESH_FACE_BYTES;
    return 0;
}

int gem_skeleton_mesh_constant(void* h_header, void* h_faces) {
    using namespace gem;
    if (!h_header || !h_faces) { set_error("gem_skeleton_mesh_constant: null argument"); return 1; }
    std::memcpy(h_header, MESH_HEADER, (size_t)MESH_HEADER_BYTES);
    unsigned char* p = static_cast<unsigned char*>(h_faces);
    uint32_t off = 0;
    for (int s = 0; s < MESH_J; ++s, off += SPH_V) {          // create_sphere: the two caps, then the 18 bands
        for (uint32_t j = 0; j < 40; ++j) {
            const uint32_t j1 = (j + 1) % 40;
            mesh_put_triangle(p, off, 0, 2 + j, 2 + j1);
            mesh_put_triangle(p, off, 1, 2 + 40 * 18 + j1, 2 + 40 * 18 + j);
        }
        for (uint32_t i = 1; i <= 18; ++i) {
            const uint32_t b1 = 2 + 40 * (i - 1), b2 = b1 + 40;
            for (uint32_t j = 0; j < 40; ++j) {
                const uint32_t j1 = (j + 1) % 40;
                mesh_put_triangle(p, off, b2 + j, b1 + j1, b1 + j);
                mesh_put_triangle(p, off, b2 + j, b2 + j1, b1 + j1);
            }
        }
    }
    for (int l = 0; l < MESH_L; ++l, off += CYL_V) {          // create_cylinder: top and bottom fans, then the 4 bands
        for (uint32_t j = 0; j < 20; ++j) {
            const uint32_t j1 = (j + 1) % 20;
            mesh_put_triangle(p, off, 0, 2 + j, 2 + j1);
            mesh_put_triangle(p, off, 1, 82 + j1, 82 + j);
        }
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t b1 = 2 + 20 * i, b2 = b1 + 20;
            for (uint32_t j = 0; j < 20; ++j) {
                const uint32_t j1 = (j + 1) % 20;
                mesh_put_triangle(p, off, b2 + j, b1 + j1, b1 + j);
                mesh_put_triangle(p, off, b2 + j, b2 + j1, b1 + j1);
            }
        }
    }
    if (p - static_cast<unsigned char*>(h_faces) != MESH_FACE_BYTES || off != (uint32_t)MESH_V) {
        set_error("gem_skeleton_mesh_constant: the face block does not add up"); return 1;
    }
    return 0;
}

int gem_sequence_align(const double* d_src, const double* d_dst, int64_t n_points, double* d_crt, void* stream) {
    using namespace gem;
    if (!d_src || !d_dst || !d_crt) { set_error("gem_sequence_align: null argument"); return 1; }
    if (n_points < 1) { set_error("gem_sequence_align: need at least one point"); return 1; }
    hipLaunchKernelGGL(sequence_align_kernel, dim3(1), dim3(ERR_ST), 0, static_cast<hipStream_t>(stream), d_src, d_dst, (size_t)n_points, d_crt);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_skeleton_mesh(const double* d_seq, int64_t n_frames, const double* d_crt, void* d_vertex_blocks, int64_t frame_stride_bytes,
                      void* stream) {
    using namespace gem;
    if (n_frames < 0) { set_error("gem_skeleton_mesh: n_frames < 0"); return 1; }
    if (frame_stride_bytes < MESH_VERTEX_BYTES || frame_stride_bytes % 16) {
        set_error("gem_skeleton_mesh: the frame stride must be at least the vertex block (349920 bytes) and a multiple of 16"); return 1;
    }
    if (reinterpret_cast<uintptr_t>(d_vertex_blocks) % 16) { set_error("gem_skeleton_mesh: the vertex blocks must be 16-byte aligned"); return 1; }
    if (n_frames == 0) return 0;
    if (!d_seq || !d_vertex_blocks) { set_error("gem_skeleton_mesh: null argument"); return 1; }
    if (n_frames > 0x7fffffffll / MESH_SLICES) { set_error("gem_skeleton_mesh: too many frames for one launch"); return 1; }
    if (int rc = gem::mesh_upload_table()) return rc;
    MeshArgs a;
    a.seq = d_seq; a.crt = d_crt; a.out = static_cast<unsigned char*>(d_vertex_blocks); a.stride = frame_stride_bytes;
    for (int l = 0; l < MESH_L; ++l) { a.lines[l][0] = MESH_LINES[l][0]; a.lines[l][1] = MESH_LINES[l][1]; }
    hipLaunchKernelGGL(skeleton_mesh_kernel, dim3((unsigned)(n_frames * MESH_SLICES)), dim3(MESH_THREADS), 0, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
