// Results as one glTF 2.0 binary file: skinned, animated skeletons: `gltf=DIR` / `--gltf DIR`.  Included from
// errors.hip behind bvh.h and skeleton_mesh.h, whose device functions it shares.
//
//   gem_gltf_layout     the counts of the file's skeleton and mesh, the byte offsets of an animation block's 17 arrays       (host)
//   gem_gltf_animation  the animation block of a sequence: times, the Hips' translation, 15 local rotations as unit quaternions
//   gem_gltf_rest_mesh  the rest-pose mesh of a skeleton with its skinning: 12 960 vertices of 32 bytes, and their bounds
//
// The rotations are the local rotation matrices of the BVH route's tree walk (bvh_walk_frame with another receiver), turned into
// quaternions by Shepperd's method and given a canonical sign.  A player interpolates between keys, and q and -q, the same rotation,
// are far apart for it: the sign must not change from one key to the next unless the rotation does.  With c[f] the canonical
// quaternions, s[f] = -s[f-1] where c[f] . c[f-1] < 0, else s[f-1]: a prefix parity over the frames, 15 of them side by side.
// Three launches, no scratch buffer, no read-back:
//   gltf_walk_kernel   one wavefront per 63 frames, one thread per frame, in 64 columns of LDS like gem_bvh_channels: column 0 holds
//                      the frame BEFORE the workgroup's first, so that every flip c[f] . c[f-1] < 0 is known inside the workgroup.  The
//                      flips of a node are one ballot, a thread's parity is the popcount below it: the quaternions are written with
//                      the sign relative to the workgroup's start, and the workgroup's own parities (15 bits) go, for the moment,
//                      into the slot of times[] of its first frame;
//   gltf_sign_kernel   workgroup g folds the words of the workgroups before it (in index order) and negates its frames' quaternions
//                      of the nodes whose bit is set.  It reads times[] and writes rotations only: no workgroup waits for another;
//   gltf_times_kernel  times[f] = f / fps.
// Everything is float64 without fused multiply-adds, rounded once to float32 at the store; negation is exact, so the bytes are
// round(s[f] c[f]) whatever the order the workgroups ran in.
#pragma once
#include <cmath>

#include "bvh.h"
#include "skeleton_mesh.h"

namespace gem {

constexpr bool gltf_has_child(int n) {
    for (int c = 0; c < BVH_NODES; ++c)
        if (BVH_PARENT[c] == n) return true;
    return false;
}
constexpr int gltf_rot_index(int n) {          // the how-manieth rotating node: the root and every node with a child
    int k = 0;
    for (int i = 0; i < n; ++i) k += gltf_has_child(i) ? 1 : 0;
    return k;
}
constexpr int GLTF_ROT = gltf_rot_index(BVH_NODES);                        // 15
constexpr int GLTF_ARRAYS = 2 + GLTF_ROT;                                  // times, translation, the rotations
constexpr int GLTF_FRAME_BYTES = 4 + 12 + 16 * GLTF_ROT;                   // 256
constexpr int GLTF_FO = BVH_FT - 1;                                        // frames a workgroup of gltf_walk_kernel writes
constexpr int GLTF_QS = 4 * GLTF_ROT;                                      // numbers per frame in LDS, [number][thread]
constexpr int GLTF_VERTEX = 32;                                            // position f32 x 3, normal f32 x 3, JOINTS_0 u8 x 4, WEIGHTS_0 u8 x 4
constexpr int64_t GLTF_VERTEX_BYTES = (int64_t)MESH_V * GLTF_VERTEX;       // 414 720
constexpr int GLTF_LAYOUT = 6 + GLTF_ROT + GLTF_ARRAYS + 2;                // the numbers of gem_gltf_layout: 40
constexpr int GLTF_TORSO[2] = {6, 7};                                      // the MESH_LINES that join two branches: (1, 7) and (4, 11)
constexpr int GLTF_HIP_LINE = 14;                                          // (7, 11): turns with Hips
static_assert(GLTF_ROT == 15 && GLTF_FRAME_BYTES == 256 && BVH_FT == 64, "one wavefront per workgroup: its ballot is the workgroup's");
static_assert(MESH_V <= 65536, "the file's indices are uint16");

// where the arrays of a block of n frames begin: every array tightly packed, every start on a 16-byte boundary
struct GltfBlock {
    unsigned char* base;
    int64_t times, translation, rotation;          // rotation k begins at rotation + k * 16 * n_frames
};

inline int64_t gltf_block_layout(int64_t n, int64_t* off) {
    int64_t at = 0;
    off[0] = at; at += (4 * n + 15) / 16 * 16;
    off[1] = at; at += (12 * n + 15) / 16 * 16;
    for (int k = 0; k < GLTF_ROT; ++k) { off[2 + k] = at; at += 16 * n; }
    return at;
}

// R (row-major, v' = R v) -> the canonical unit quaternion (x, y, z, w) into a thread's column: Shepperd's method on the largest of
// (trace, R00, R11, R22), the first on ties; then the sign that makes the first non-zero of (w, x, y, z) positive
__device__ inline void gltf_quaternion(const double* R, double* out) {
#pragma clang fp contract(off)
    const double t = (R[0] + R[4]) + R[8];
    double w, x, y, z;
    if (t >= R[0] && t >= R[4] && t >= R[8]) {
        const double r = sqrt(1.0 + t), d = 2.0 * r;
        w = r / 2; x = (R[7] - R[5]) / d; y = (R[2] - R[6]) / d; z = (R[3] - R[1]) / d;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        const double r = sqrt(((1.0 + R[0]) - R[4]) - R[8]), d = 2.0 * r;
        x = r / 2; w = (R[7] - R[5]) / d; y = (R[1] + R[3]) / d; z = (R[2] + R[6]) / d;
    } else if (R[4] >= R[8]) {
        const double r = sqrt(((1.0 - R[0]) + R[4]) - R[8]), d = 2.0 * r;
        y = r / 2; w = (R[2] - R[6]) / d; x = (R[1] + R[3]) / d; z = (R[5] + R[7]) / d;
    } else {
        const double r = sqrt(((1.0 - R[0]) - R[4]) + R[8]), d = 2.0 * r;
        z = r / 2; w = (R[3] - R[1]) / d; x = (R[2] + R[6]) / d; y = (R[5] + R[7]) / d;
    }
    const double lead = w != 0.0 ? w : x != 0.0 ? x : y != 0.0 ? y : z;
    if (lead < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    out[0] = x; out[BVH_FT] = y; out[2 * BVH_FT] = z; out[3 * BVH_FT] = w;
}

// the receiver of bvh_walk_frame that keeps the root's position and makes quaternions of the rotating nodes' matrices (a thread's column in LDS)
struct GltfQuatOut {
    double* q;
    double P[3];
    __device__ void position(const double* p) { P[0] = p[0]; P[1] = p[1]; P[2] = p[2]; }
    template <int N>
    __device__ void rotation(const double* R) { gltf_quaternion(R, q + 4 * gltf_rot_index(N) * BVH_FT); }
    template <int N>
    __device__ void leaf() { static_assert(!gltf_has_child(N), "a leaf has no channel in the file"); }
};

__device__ inline bool gltf_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }          // (false for NaN)

typedef float gltf_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t gltf_u4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(BVH_FT) void gltf_walk_kernel(const double* seq, int64_t n_frames, const double* crt, double fps, GltfBlock b,
                                                           unsigned long long* bad) {
    __shared__ double xs[BVH_XS * BVH_FT];
    __shared__ double qs[GLTF_QS * BVH_FT];
    const int tx = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * GLTF_FO;          // the first frame this workgroup writes; column c holds frame first - 1 + c
    for (int i = tx; i < BVH_FT * BVH_J; i += BVH_FT) {
        const int fl = i / BVH_J, j = i - fl * BVH_J;
        const int64_t fi = first - 1 + fl;
        if (fi < 0 || fi >= n_frames) continue;
        double q[3];
        bvh_moved_joint(seq + fi * (BVH_J * 3), crt, j, q);
#pragma unroll
        for (int d = 0; d < 3; ++d) xs[(3 * j + d) * BVH_FT + fl] = q[d];
    }
    __syncthreads();
    const int64_t f = first - 1 + tx;
    const bool valid = f >= 0 && f < n_frames;
    GltfQuatOut out;
    out.q = qs + tx;
    out.P[0] = out.P[1] = out.P[2] = 0.0;
    if (valid) bvh_walk_frame(BvhLdsFrame{xs + tx}, out);
    __syncthreads();
    const bool writes = valid && tx >= 1;
    const unsigned long long below = tx == 63 ? ~0ull : ((1ull << (tx + 1)) - 1ull);          // this lane and the lanes before it
    uint32_t group = 0;
    bool is_bad = false;
#pragma unroll
    for (int k = 0; k < GLTF_ROT; ++k) {
#pragma clang fp contract(off)
        const double* c = qs + (4 * k) * BVH_FT + tx;
        const double x = c[0], y = c[BVH_FT], z = c[2 * BVH_FT], w = c[3 * BVH_FT];
        bool flip = false;
        if (writes && f >= 1) {          // (column tx - 1 holds frame f - 1; a dot of 0 or NaN does not flip)
            const double dot = ((w * c[3 * BVH_FT - 1] + x * c[-1]) + y * c[BVH_FT - 1]) + z * c[2 * BVH_FT - 1];
            flip = dot < 0.0;
        }
        const unsigned long long flips = __ballot(flip ? 1 : 0);
        group |= (uint32_t)(__popcll(flips) & 1) << k;
        if (writes) {
            const bool neg = __popcll(flips & below) & 1;
            gltf_f4 v;
            v[0] = (float)(neg ? -x : x); v[1] = (float)(neg ? -y : y); v[2] = (float)(neg ? -z : z); v[3] = (float)(neg ? -w : w);
            is_bad = is_bad || !(gltf_finite(v[0]) && gltf_finite(v[1]) && gltf_finite(v[2]) && gltf_finite(v[3]));
            reinterpret_cast<gltf_f4*>(b.base + b.rotation + (int64_t)k * 16 * n_frames)[f] = v;
        }
    }
    if (writes) {
#pragma clang fp contract(off)
        float* t = reinterpret_cast<float*>(b.base + b.translation) + 3 * f;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float v = (float)out.P[d];
            is_bad = is_bad || !gltf_finite(v);
            t[d] = v;
        }
        is_bad = is_bad || !gltf_finite((float)((double)f / fps));
        if (is_bad) {
            atomicAdd(bad, 1ull);
            atomicMin(bad + 1, (unsigned long long)f);          // (-1 as the caller set it is the largest unsigned value)
        }
        if (tx == 1) reinterpret_cast<uint32_t*>(b.base + b.times)[first] = group;          // (until gltf_times_kernel: read by gltf_sign_kernel)
    }
}

__global__ __launch_bounds__(BVH_FT) void gltf_sign_kernel(int64_t n_frames, GltfBlock b) {
    __shared__ uint32_t part[BVH_FT];
    const int tx = threadIdx.x;
    const int64_t g = blockIdx.x;
    if (g == 0) return;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(b.base + b.times);
    uint32_t m = 0;
    for (int64_t h = tx; h < g; h += BVH_FT) m ^= words[h * GLTF_FO];
    part[tx] = m;
    __syncthreads();
    uint32_t before = 0;
    for (int i = 0; i < BVH_FT; ++i) before ^= part[i];
    const int64_t f = g * GLTF_FO + tx;
    if (before == 0 || tx >= GLTF_FO || f >= n_frames) return;
#pragma unroll
    for (int k = 0; k < GLTF_ROT; ++k) {
        if (!((before >> k) & 1u)) continue;
        gltf_f4* p = reinterpret_cast<gltf_f4*>(b.base + b.rotation + (int64_t)k * 16 * n_frames) + f;
        const gltf_f4 v = *p;
        *p = -v;
    }
}

__global__ __launch_bounds__(256) void gltf_times_kernel(int64_t n_frames, double fps, float* times) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f < n_frames) times[f] = (float)((double)f / fps);
}

// ---------------------------------------------------------------------------------------------------  the rest-pose mesh
struct GltfMeshArgs {
    const double* rest;
    unsigned char* out;
    float* bounds;
    int parent[BVH_NODES];
    double dirs[BVH_NODES][3];
    int node_of_joint[MESH_J];
    int lines[MESH_L][2];
    int bind[MESH_L][2];          // the node a line turns with and -1, or for a torso line the nodes of its second and of its first joint
};

constexpr int GLTF_MESH_THREADS = 256;

// One workgroup: the static mesh is made once per skeleton, and its bounds are the minimum and maximum over all of it.
__global__ __launch_bounds__(GLTF_MESH_THREADS) void gltf_rest_mesh_kernel(GltfMeshArgs a) {
    __shared__ double nodes[BVH_NODES][3];
    __shared__ double jt[MESH_J][3];
    __shared__ double bone[MESH_L][12];
    __shared__ double bh[MESH_L];
    __shared__ float red[6][GLTF_MESH_THREADS];
    const int tid = threadIdx.x;
    if (tid == 0) {          // the rest joints: Hips at the origin, every node its rest direction times its rest length from its parent
#pragma clang fp contract(off)
        for (int d = 0; d < 3; ++d) nodes[0][d] = 0.0;
        for (int n = 1; n < BVH_NODES; ++n)
            for (int d = 0; d < 3; ++d) nodes[n][d] = nodes[a.parent[n]][d] + a.dirs[n][d] * a.rest[n];
        for (int j = 0; j < MESH_J; ++j)
            for (int d = 0; d < 3; ++d) jt[j][d] = nodes[a.node_of_joint[j]][d];
    }
    __syncthreads();
    if (tid < MESH_L) mesh_bone(jt[a.lines[tid][0]], jt[a.lines[tid][1]], bone[tid], &bh[tid]);
    __syncthreads();
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int v = tid; v < MESH_V; v += GLTF_MESH_THREADS) {
#pragma clang fp contract(off)
        double o[3], nr[3];
        uint32_t unused, joints, weights;
        mesh_vertex(v, jt, bone, bh, o, &unused);
        if (v < MESH_J * SPH_V) {          // a sphere: radial normals, bound to its joint's node
            const int j = v / SPH_V, k = v - j * SPH_V;
            for (int d = 0; d < 3; ++d) nr[d] = mesh_table[3 * k + d];
            joints = (uint32_t)a.node_of_joint[j];
            weights = 255u;
        } else {
            const int w = v - MESH_J * SPH_V, l = w / CYL_V, k = w - l * CYL_V;
            const double* R = bone[l];
            int ring = -1;
            if (k < 2) {          // the cap centres: + the bone at the line's second joint, - the bone at its first
                const double sg = k == 0 ? 1.0 : -1.0;
                for (int d = 0; d < 3; ++d) nr[d] = sg * R[3 * d + 2];
            } else {
                ring = (k - 2) / 20;
                const int j = (k - 2) - 20 * ring;
                const double cs = mesh_table[SPH_V * 3 + 2 * j], sn = mesh_table[SPH_V * 3 + 2 * j + 1];
                for (int d = 0; d < 3; ++d) nr[d] = R[3 * d] * cs + R[3 * d + 1] * sn;
            }
            const int n0 = a.bind[l][0], n1 = a.bind[l][1];
            if (n1 < 0) {
                joints = (uint32_t)n0;
                weights = 255u;
            } else {          // a torso line: ring 0 and cap 0 lie on its second joint (n0), ring 4 and cap 1 on its first (n1)
                const uint32_t w1 = ring < 0 ? (k == 0 ? 0u : 255u) : ring == 0 ? 0u : ring == 1 ? 64u : ring == 2 ? 128u : ring == 3 ? 191u : 255u;
                const uint32_t w0 = 255u - w1;
                joints = (w0 ? (uint32_t)n0 : 0u) | ((w1 ? (uint32_t)n1 : 0u) << 8);          // (a weight of zero names node 0)
                weights = w0 | (w1 << 8);
            }
        }
        const float p[3] = {(float)o[0], (float)o[1], (float)o[2]};
        for (int d = 0; d < 3; ++d) {
            if (p[d] < lo[d]) lo[d] = p[d];
            if (p[d] > hi[d]) hi[d] = p[d];
        }
        gltf_u4 rec0, rec1;
        rec0[0] = __float_as_uint(p[0]); rec0[1] = __float_as_uint(p[1]); rec0[2] = __float_as_uint(p[2]); rec0[3] = __float_as_uint((float)nr[0]);
        rec1[0] = __float_as_uint((float)nr[1]); rec1[1] = __float_as_uint((float)nr[2]); rec1[2] = joints; rec1[3] = weights;
        gltf_u4* dst = reinterpret_cast<gltf_u4*>(a.out) + 2 * (int64_t)v;
        dst[0] = rec0;
        dst[1] = rec1;
    }
    for (int d = 0; d < 3; ++d) { red[d][tid] = lo[d]; red[3 + d][tid] = hi[d]; }
    __syncthreads();
    if (tid < 6) {
        float r = red[tid][0];
        for (int i = 1; i < GLTF_MESH_THREADS; ++i) {
            const float c = red[tid][i];
            if (tid < 3 ? c < r : c > r) r = c;
        }
        a.bounds[tid] = r;
    }
}

}  // namespace gem

extern "C" {

int gem_gltf_layout(int64_t n_frames, int64_t* out) {
    using namespace gem;
    if (!out) { set_error("gem_gltf_layout: null argument"); return 1; }
    if (n_frames < 0) { set_error("gem_gltf_layout: n_frames < 0"); return 1; }
    if (n_frames > (int64_t)1 << 40) { set_error("gem_gltf_layout: too many frames"); return 1; }
    int at = 0;
    out[at++] = BVH_NODES; out[at++] = GLTF_ROT; out[at++] = MESH_V; out[at++] = MESH_T; out[at++] = GLTF_VERTEX; out[at++] = GLTF_VERTEX_BYTES;
    for (int n = 0; n < BVH_NODES; ++n)
        if (gltf_has_child(n)) out[at++] = n;
    const int64_t size = gltf_block_layout(n_frames, out + at);
    at += GLTF_ARRAYS;
    out[at++] = size;
    out[at++] = GLTF_FRAME_BYTES;
    if (at != GLTF_LAYOUT) { set_error("gem_gltf_layout: the layout does not add up"); return 1; }
    return 0;
}

int gem_gltf_animation(const double* d_seq, int64_t n_frames, const double* d_crt, double fps, void* d_block, int64_t* d_bad, void* stream) {
    using namespace gem;
    if (n_frames < 0) { set_error("gem_gltf_animation: n_frames < 0"); return 1; }
    if (!(fps > 0.0) || !std::isfinite(fps)) { set_error("gem_gltf_animation: fps must be a finite positive number"); return 1; }
    if (reinterpret_cast<uintptr_t>(d_block) % 16) { set_error("gem_gltf_animation: the block must be 16-byte aligned"); return 1; }
    if (n_frames == 0) return 0;
    if (!d_seq || !d_block || !d_bad) { set_error("gem_gltf_animation: null argument"); return 1; }
    if (n_frames > 0x7fffffffll * GLTF_FO) { set_error("gem_gltf_animation: too many frames for one launch"); return 1; }
    int64_t off[GLTF_ARRAYS];
    gltf_block_layout(n_frames, off);
    GltfBlock b;
    b.base = static_cast<unsigned char*>(d_block); b.times = off[0]; b.translation = off[1]; b.rotation = off[2];
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned groups = (unsigned)((n_frames + GLTF_FO - 1) / GLTF_FO);
    hipLaunchKernelGGL(gltf_walk_kernel, dim3(groups), dim3(BVH_FT), 0, s, d_seq, n_frames, d_crt, fps, b, reinterpret_cast<unsigned long long*>(d_bad));
    GEM_HIP(hipGetLastError());
    if (groups > 1) {
        hipLaunchKernelGGL(gltf_sign_kernel, dim3(groups), dim3(BVH_FT), 0, s, n_frames, b);
        GEM_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(gltf_times_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, s, n_frames, fps,
                       reinterpret_cast<float*>(b.base + b.times));
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_gltf_rest_mesh(const double* d_rest, void* d_vertices, float* d_bounds, void* stream) {
    using namespace gem;
    if (!d_rest || !d_vertices || !d_bounds) { set_error("gem_gltf_rest_mesh: null argument"); return 1; }
    if (reinterpret_cast<uintptr_t>(d_vertices) % 16) { set_error("gem_gltf_rest_mesh: the vertices must be 16-byte aligned"); return 1; }
    if (int rc = mesh_upload_table()) return rc;
    GltfMeshArgs a;
    a.rest = d_rest; a.out = static_cast<unsigned char*>(d_vertices); a.bounds = d_bounds;
    for (int n = 0; n < BVH_NODES; ++n) {
        a.parent[n] = BVH_PARENT[n];
        for (int d = 0; d < 3; ++d) a.dirs[n][d] = BVH_REST[n][d];
        if (BVH_JOINT[n] >= 0) a.node_of_joint[BVH_JOINT[n]] = n;
    }
    for (int l = 0; l < MESH_L; ++l) {
        a.lines[l][0] = MESH_LINES[l][0]; a.lines[l][1] = MESH_LINES[l][1];
        const int first = a.node_of_joint[MESH_LINES[l][0]], second = a.node_of_joint[MESH_LINES[l][1]];
        if (l == GLTF_TORSO[0] || l == GLTF_TORSO[1]) { a.bind[l][0] = second; a.bind[l][1] = first; }
        else { a.bind[l][0] = l == GLTF_HIP_LINE ? 0 : BVH_PARENT[second]; a.bind[l][1] = -1; }
    }
    hipLaunchKernelGGL(gltf_rest_mesh_kernel, dim3(1), dim3(GLTF_MESH_THREADS), 0, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
