// Skeleton sequences as BVH animation from the device: `bvh=DIR` / `--bvh DIR`.  Included from errors.hip.
//
//   gem_bvh_layout     nodes, channels per frame, bytes per field, bytes per frame                              (host)
//   gem_bvh_tables     the tree: parents, the skeleton joint under every node, the rest directions             (host)
//   gem_bvh_rest       the rest length of every bone: the mean of its length over the sequence's frames
//   gem_bvh_channels   the 60 channels of every frame: the root's position, then (Z, X, Y) Euler angles of 19 local rotations
//   gem_format_fields  float64 values as "%15.6f" text, 16 bytes each, correctly rounded
//
// The tree has 19 nodes on the 15 joints: Hips sits on the midpoint of the two hip joints, Spine and the two collars are helpers
// with a zero offset (a joint with several children cannot point at all of them with one rotation; with the helpers every bone is
// reproduced exactly, up to its length).  Rest directions are axis-aligned: Y up, Z forward, +X the character's left.  The inverse
// kinematics are position-only: the root's frame comes from the hip line and the direction to the neck, the neck's from the shoulder
// line and the spine, every other node turns its rest direction onto its one bone by the shortest arc; 15 points say nothing about
// the twist about a bone.  The rest lengths are one workgroup's fixed-order sums (16 lanes per frame, one per bone): the same bits on
// every call, no atomics, no scratch buffer.  For the channels one thread per frame walks the tree (float64, no fused multiply-adds), its joints and its channels in
// LDS so that a workgroup's loads and stores are contiguous; the walk hands the root's position and every local rotation matrix to a
// receiver (BvhEulerOut: the channels; gltf.h walks the same tree into quaternions).  The text is one thread per field: the decimal digits come from the
// value's exact binary expansion in integer arithmetic (mantissa x 15625 in 128 bits, a shift, the remainder against one half, ties
// to even), which is what C's printf and Python's % give; every field is one aligned 16-byte store.
#pragma once
#include <cmath>

#include "umeyama_device.h"

namespace gem {

constexpr int BVH_NODES = 19, BVH_J = 15, BVH_CHANNELS = 6 + 3 * (BVH_NODES - 1);          // 60
constexpr int BVH_FIELD = 16;                                                               // "%15.6f" and one separator
constexpr int BVH_FRAME_BYTES = BVH_CHANNELS * BVH_FIELD;                                   // 960
constexpr int BVH_HIP_R = 7, BVH_HIP_L = 11;                                                // Hips = their midpoint
//                                      Hips Spine Neck | R: collar shoulder elbow wrist | L: collar shoulder elbow wrist | R: hip knee ankle foot | L
constexpr int BVH_PARENT[BVH_NODES] = {-1, 0, 1, 2, 3, 4, 5, 2, 7, 8, 9, 0, 11, 12, 13, 0, 15, 16, 17};
constexpr int BVH_JOINT[BVH_NODES] = {-1, -1, 0, -1, 1, 2, 3, -1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14};          // -1: no joint of its own
constexpr double BVH_REST[BVH_NODES][3] = {{0, 0, 0}, {0, 0, 0}, {0, 1, 0},
                                           {0, 0, 0}, {-1, 0, 0}, {-1, 0, 0}, {-1, 0, 0}, {0, 0, 0}, {1, 0, 0}, {1, 0, 0}, {1, 0, 0},
                                           {-1, 0, 0}, {0, -1, 0}, {0, -1, 0}, {0, 0, 1}, {1, 0, 0}, {0, -1, 0}, {0, -1, 0}, {0, 0, 1}};
constexpr int BVH_BONES = 15;                                                               // nodes with a rest direction
constexpr double BVH_TINY = 1e-12;                                                          // below it a cross product has no direction
constexpr double BVH_GIMBAL = 1.0 - 1e-10;
constexpr double BVH_DEG = 180.0 / M_PI;
constexpr int64_t BVH_FIELD_MAX = 9999999999999ll;                                          // 9999999.999999 in millionths

constexpr bool bvh_has_rest(int n) { return BVH_REST[n][0] != 0 || BVH_REST[n][1] != 0 || BVH_REST[n][2] != 0; }
constexpr int bvh_bone_index(int n) {          // the how-manieth node with a rest direction
    int k = 0;
    for (int i = 0; i < n; ++i) k += bvh_has_rest(i) ? 1 : 0;
    return k;
}
constexpr int bvh_channel(int n) { return n == 0 ? 3 : 3 + 3 * n; }          // a node's first rotation channel
static_assert(bvh_bone_index(BVH_NODES) == BVH_BONES && BVH_BONES <= 16, "bvh_rest_kernel gives a frame 16 lanes, one per bone");

// joint j of a frame as it lies in memory, moved by the similarity (c * (p . R) + t, the row-vector convention of gem_sequence_align)
__device__ inline void bvh_moved_joint(const double* frame, const double* crt, int j, double* q) {
#pragma clang fp contract(off)
    const double p0 = frame[3 * j], p1 = frame[3 * j + 1], p2 = frame[3 * j + 2];
    q[0] = p0; q[1] = p1; q[2] = p2;
    if (crt) {
        const double c = crt[0];
        const double* R = crt + 1;
        const double* t = crt + 10;
#pragma unroll
        for (int d = 0; d < 3; ++d) q[d] = c * (p0 * R[d] + p1 * R[3 + d] + p2 * R[6 + d]) + t[d];
    }
}

constexpr int BVH_FT = 64;          // frames (threads) per workgroup of bvh_channels_kernel

// A frame's joints for the tree walk: a thread's column of the workgroup's moved joints in LDS, [number][thread] (gem_bvh_channels)
struct BvhLdsFrame {
    const double* X;
    __device__ void joint(int j, double* q) const {
#pragma unroll
        for (int d = 0; d < 3; ++d) q[d] = X[(3 * j + d) * BVH_FT];
    }
};

// where node N sits: on its joint; Hips on the midpoint of the hip joints; a helper on its parent
template <int N>
__device__ inline void bvh_pos(const BvhLdsFrame& fr, double* p) {
#pragma clang fp contract(off)
    if constexpr (BVH_JOINT[N] >= 0) {
        fr.joint(BVH_JOINT[N], p);
    } else if constexpr (N == 0) {
        double a[3], b[3];
        fr.joint(BVH_HIP_R, a);
        fr.joint(BVH_HIP_L, b);
#pragma unroll
        for (int d = 0; d < 3; ++d) p[d] = (a[d] + b[d]) / 2;
    } else {
        bvh_pos<BVH_PARENT[N]>(fr, p);
    }
}

template <int N>
__device__ inline double bvh_bone(const BvhLdsFrame& fr, double* d) {          // d = pos(N) - pos(parent), -> its length
#pragma clang fp contract(off)
    double a[3], b[3];
    bvh_pos<N>(fr, a);
    bvh_pos<BVH_PARENT[N]>(fr, b);
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = a[i] - b[i];
    return sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

// the two joints whose midpoint node n sits on (twice the same joint for all but Hips and Spine)
constexpr int bvh_node_joint(int n, int which) {
    return BVH_JOINT[n] >= 0 ? BVH_JOINT[n] : n == 0 ? (which ? BVH_HIP_L : BVH_HIP_R) : bvh_node_joint(BVH_PARENT[n], which);
}

struct BvhRestArgs {
    const double* seq;
    const double* crt;
    double* rest;
    int64_t n_frames;
    int bone_of_node[BVH_NODES];          // -1: a node without a rest direction
    int ends[16][4];                      // per bone: the joints under the node (two), the joints under its parent (two)
};

constexpr int BVH_REST_SLOTS = ERR_ST / 16;          // 64

// One workgroup, 16 lanes per frame (lane = bone): thread (slot, bone) adds its bone's length over frames slot, slot + 64, ... in that
// order, then one thread per node adds the 64 partial sums in slot order: the same bits on every call, no atomics, no scratch buffer.
__global__ __launch_bounds__(ERR_ST) void bvh_rest_kernel(BvhRestArgs a) {
    __shared__ double part[BVH_REST_SLOTS][16];
    const int tid = threadIdx.x, k = tid & 15, slot = tid >> 4;
    double sum = 0.0;
    if (k < BVH_BONES) {
        const int j0 = a.ends[k][0], j1 = a.ends[k][1], p0 = a.ends[k][2], p1 = a.ends[k][3];
#pragma unroll 4
        for (int64_t f = slot; f < a.n_frames; f += BVH_REST_SLOTS) {
#pragma clang fp contract(off)
            const double* frame = a.seq + f * (BVH_J * 3);
            double x[3], y[3], u[3], v[3];
            bvh_moved_joint(frame, a.crt, j0, x);
            bvh_moved_joint(frame, a.crt, p0, u);
            if (j1 != j0) {
                bvh_moved_joint(frame, a.crt, j1, y);
                for (int d = 0; d < 3; ++d) x[d] = (x[d] + y[d]) / 2;
            }
            if (p1 != p0) {
                bvh_moved_joint(frame, a.crt, p1, v);
                for (int d = 0; d < 3; ++d) u[d] = (u[d] + v[d]) / 2;
            }
            const double d0 = x[0] - u[0], d1 = x[1] - u[1], d2 = x[2] - u[2];
            sum += sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        }
    }
    part[slot][k] = sum;
    __syncthreads();
    if (tid < BVH_NODES) {
        const int bone = a.bone_of_node[tid];
        double t = 0.0;
        if (bone >= 0) {
            for (int s = 0; s < BVH_REST_SLOTS; ++s) t += part[s][bone];
            t = t / (double)a.n_frames;
        }
        a.rest[tid] = t;
    }
}

// ---------------------------------------------------------------------------------------------------  the kinematics of one frame
// 3 x 3 matrices are row-major double[9]; a node's frame G holds its axes in world coordinates as COLUMNS.

__device__ inline void bvh_identity(double* R) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
}

// G = columns (x, y, z) with x = unit(xd), z = unit(x cross hint), y = z cross x; false (G untouched) where xd or x cross hint has no direction
__device__ inline bool bvh_frame_from(const double* xd, const double* hint, double* G) {
#pragma clang fp contract(off)
    const double nx = sqrt(xd[0] * xd[0] + xd[1] * xd[1] + xd[2] * xd[2]);
    if (nx < BVH_TINY) return false;
    const double x[3] = {xd[0] / nx, xd[1] / nx, xd[2] / nx};
    const double zc[3] = {x[1] * hint[2] - x[2] * hint[1], x[2] * hint[0] - x[0] * hint[2], x[0] * hint[1] - x[1] * hint[0]};
    const double nz = sqrt(zc[0] * zc[0] + zc[1] * zc[1] + zc[2] * zc[2]);
    if (nz < BVH_TINY) return false;
    const double z[3] = {zc[0] / nz, zc[1] / nz, zc[2] / nz};
    const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
#pragma unroll
    for (int r = 0; r < 3; ++r) { G[3 * r] = x[r]; G[3 * r + 1] = y[r]; G[3 * r + 2] = z[r]; }
    return true;
}

// the shortest-arc rotation S that takes the unit vector r to the unit vector l
__device__ inline void bvh_shortest_arc(const double* r, const double* l, double* S) {
#pragma clang fp contract(off)
    const double v[3] = {r[1] * l[2] - r[2] * l[1], r[2] * l[0] - r[0] * l[2], r[0] * l[1] - r[1] * l[0]};
    const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double c = r[0] * l[0] + r[1] * l[1] + r[2] * l[2];
    if (s < BVH_TINY) {
        bvh_identity(S);
        if (c < 0.0) {          // antiparallel: a half turn about unit(r cross X), or about unit(r cross Y) where r is near X: S = 2 k k^T - I
            const bool near_x = fabs(r[0]) >= 0.9;
            const double e[3] = {near_x ? 0.0 : 1.0, near_x ? 1.0 : 0.0, 0.0};
            double k[3] = {r[1] * e[2] - r[2] * e[1], r[2] * e[0] - r[0] * e[2], r[0] * e[1] - r[1] * e[0]};
            const double nk = sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
#pragma unroll
            for (int i = 0; i < 3; ++i) k[i] = k[i] / nk;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) S[3 * i + j] = 2.0 * (k[i] * k[j]) - (i == j ? 1.0 : 0.0);
        }
        return;
    }
    const double k[3] = {v[0] / s, v[1] / s, v[2] / s};
    const double th = atan2(s, c), sn = sin(th), cs = cos(th), vs = 1.0 - cs;
    // Rodrigues: S = cos I + sin [k]x + (1 - cos) k k^T
    S[0] = cs + vs * (k[0] * k[0]);          S[1] = vs * (k[0] * k[1]) - sn * k[2];   S[2] = vs * (k[0] * k[2]) + sn * k[1];
    S[3] = vs * (k[1] * k[0]) + sn * k[2];   S[4] = cs + vs * (k[1] * k[1]);          S[5] = vs * (k[1] * k[2]) - sn * k[0];
    S[6] = vs * (k[2] * k[0]) - sn * k[1];   S[7] = vs * (k[2] * k[1]) + sn * k[0];   S[8] = cs + vs * (k[2] * k[2]);
}

// R = Rz(a) Rx(b) Ry(c) -> (a, b, c) in degrees, the order of the file's channels, into a thread's column of the channels in LDS
__device__ inline void bvh_euler(const double* R, double* out) {
#pragma clang fp contract(off)
    double a, b, c;
    if (fabs(R[7]) > BVH_GIMBAL) {
        b = R[7] > 0.0 ? 90.0 : -90.0;
        a = atan2(R[3], R[0]) * BVH_DEG;
        c = 0.0;
    } else {
        b = asin(R[7]) * BVH_DEG;
        a = atan2(-R[1], R[4]) * BVH_DEG;
        c = atan2(-R[6], R[8]) * BVH_DEG;
    }
    out[0] = a; out[BVH_FT] = b; out[2 * BVH_FT] = c;
}

__device__ inline void bvh_matmul(const double* A, const double* B, double* C) {          // C = A B
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

__device__ inline void bvh_matmul_tn(const double* A, const double* B, double* C) {          // C = A^T B
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}

// What a frame's walk hands its results to: `position` the root's position, `rotation<N>` node N's local rotation matrix, `leaf<N>` a
// node that has no rotation of its own.  BvhEulerOut makes the BVH file's channels of them (a thread's column in LDS): the position
// times the unit scale, (Z, X, Y) Euler angles, three zeros for a leaf.  (gltf.h has the one that makes quaternions.)
struct BvhEulerOut {
    double* ch;
    double unit_scale;
    __device__ void position(const double* P) const {
#pragma clang fp contract(off)
#pragma unroll
        for (int d = 0; d < 3; ++d) ch[d * BVH_FT] = P[d] * unit_scale;
    }
    template <int N>
    __device__ void rotation(const double* R) const { bvh_euler(R, ch + bvh_channel(N) * BVH_FT); }
    template <int N>
    __device__ void leaf() const {
#pragma unroll
        for (int k = 0; k < 3; ++k) ch[(bvh_channel(N) + k) * BVH_FT] = 0.0;
    }
};

// Node N with its one child CHILD: G (on entry its parent's frame) becomes G S, S the shortest arc from CHILD's rest direction to
// the bone as the parent's frame sees it; S, N's local rotation, goes to out.
template <int N, int CHILD, class Out>
__device__ inline void bvh_arc_node(const BvhLdsFrame& X, double* G, Out& out) {
#pragma clang fp contract(off)
    static_assert(BVH_PARENT[CHILD] == N && bvh_has_rest(CHILD), "CHILD hangs on N by a bone");
    const double r[3] = {BVH_REST[CHILD][0], BVH_REST[CHILD][1], BVH_REST[CHILD][2]};
    double d[3], S[9];
    const double len = bvh_bone<CHILD>(X, d);
    if (len == 0.0) {
        bvh_identity(S);
    } else {
        const double u[3] = {d[0] / len, d[1] / len, d[2] / len};
        double l[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) l[i] = G[i] * u[0] + G[3 + i] * u[1] + G[6 + i] * u[2];
        bvh_shortest_arc(r, l, S);
        double T[9];
        bvh_matmul(G, S, T);
#pragma unroll
        for (int i = 0; i < 9; ++i) G[i] = T[i];
    }
    out.template rotation<N>(S);
}

// a limb: the three arc nodes A, A + 1, A + 2 under the frame G and the leaf A + 3 (no rotation of its own)
template <int A, class Out>
__device__ inline void bvh_limb(const BvhLdsFrame& X, const double* G_parent, Out& out) {
    double G[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) G[i] = G_parent[i];
    bvh_arc_node<A, A + 1>(X, G, out);
    bvh_arc_node<A + 1, A + 2>(X, G, out);
    bvh_arc_node<A + 2, A + 3>(X, G, out);
    out.template leaf<A + 3>();
}

// One frame: X its moved joints (a thread's columns in LDS), out what takes its position and local rotations
template <class Out>
__device__ inline void bvh_walk_frame(const BvhLdsFrame& X, Out& out) {
#pragma clang fp contract(off)
    double P[3], a[3], b[3], G0[9], G1[9], G2[9], L[9];
    // Hips: its position, and the frame of the hip line (x, towards the left hip) and the direction to the neck
    bvh_pos<0>(X, P);
    out.position(P);
    bvh_pos<15>(X, a);
    bvh_pos<11>(X, b);
    double xd[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
    bvh_pos<2>(X, a);
    double up[3] = {a[0] - P[0], a[1] - P[1], a[2] - P[2]};
    bvh_identity(G0);
    bvh_frame_from(xd, up, G0);          // (degenerate: the identity stays)
    out.template rotation<0>(G0);
    // Spine: turns +Y onto the direction to the neck
#pragma unroll
    for (int i = 0; i < 9; ++i) G1[i] = G0[i];
    bvh_arc_node<1, 2>(X, G1, out);
    // Neck: the frame of the shoulder line (x, towards the left shoulder) and the spine's y axis
    bvh_pos<8>(X, a);
    bvh_pos<4>(X, b);
#pragma unroll
    for (int d = 0; d < 3; ++d) xd[d] = a[d] - b[d];
    up[0] = G1[1]; up[1] = G1[4]; up[2] = G1[7];
    if (bvh_frame_from(xd, up, G2)) {
        bvh_matmul_tn(G1, G2, L);
    } else {          // (degenerate: the spine's frame)
#pragma unroll
        for (int i = 0; i < 9; ++i) G2[i] = G1[i];
        bvh_identity(L);
    }
    out.template rotation<2>(L);
    bvh_limb<3>(X, G2, out);           // right arm: collar, shoulder, elbow | wrist
    bvh_limb<7>(X, G2, out);           // left arm
    bvh_limb<11>(X, G0, out);          // right leg: hip, knee, ankle | foot
    bvh_limb<15>(X, G0, out);          // left leg
}

constexpr int BVH_XS = BVH_J * 3, BVH_CS = BVH_CHANNELS;    // numbers per frame in LDS, [number][thread]: conflict-free columns

__global__ __launch_bounds__(BVH_FT) void bvh_channels_kernel(const double* seq, int64_t n_frames, const double* crt, double unit_scale,
                                                              double* channels) {
    __shared__ double xs[BVH_XS * BVH_FT];
    __shared__ double cs[BVH_CS * BVH_FT];
    const int tx = threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * BVH_FT;
    const int nf = (int)(n_frames - f0 < BVH_FT ? n_frames - f0 : BVH_FT);
    // the workgroup's joints, read as they lie (contiguous) and moved by the similarity: joint by joint
    for (int i = tx; i < nf * BVH_J; i += BVH_FT) {
        const int fl = i / BVH_J, j = i - fl * BVH_J;
        double q[3];
        bvh_moved_joint(seq + (f0 + fl) * (BVH_J * 3), crt, j, q);
#pragma unroll
        for (int d = 0; d < 3; ++d) xs[(3 * j + d) * BVH_FT + fl] = q[d];
    }
    __syncthreads();
    if (tx < nf) {
        BvhEulerOut out{cs + tx, unit_scale};
        bvh_walk_frame(BvhLdsFrame{xs + tx}, out);
    }
    __syncthreads();
    double* out = channels + f0 * BVH_CHANNELS;
    for (int i = tx; i < nf * BVH_CHANNELS; i += BVH_FT) {
        const int fl = i / BVH_CHANNELS, k = i - fl * BVH_CHANNELS;
        out[i] = cs[k * BVH_FT + fl];
    }
}

// ---------------------------------------------------------------------------------------------------  the text
typedef uint32_t bvh_u4 __attribute__((ext_vector_type(4)));

// Field i of the text: "%15.6f" of values[i] and one separator (a space; a newline after the last value of a line).  The decimal
// digits of a finite v = m 2^e: N = m 15625 2^(e + 6) millionths, rounded to the nearest integer, ties to even, on the exact
// binary value.  m 15625 < 2^67 lives in 128 bits; e + 6 >= 0 with m != 0 is a value above 2^46, which does not fit the field.
__global__ __launch_bounds__(256) void format_fields_kernel(const double* values, int64_t n, int64_t per_line, unsigned char* text,
                                                           unsigned long long* bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(values[i]);
    const bool neg = bits >> 63;
    const int ex = (int)((bits >> 52) & 0x7FF);
    const unsigned long long frac = bits & 0xFFFFFFFFFFFFFull;
    unsigned char c[BVH_FIELD];
#pragma unroll
    for (int k = 0; k < 15; ++k) c[k] = ' ';
    c[15] = (i % per_line == per_line - 1) ? '\n' : ' ';
    bool is_bad = false;
    if (ex == 0x7FF) {          // Python: "nan" whatever the sign bit, "inf" / "-inf"
        is_bad = true;
        if (frac) { c[12] = 'n'; c[13] = 'a'; c[14] = 'n'; }
        else { c[12] = 'i'; c[13] = 'n'; c[14] = 'f'; if (neg) c[11] = '-'; }
    } else {
        const unsigned long long m = ex ? (frac | (1ull << 52)) : frac;
        const int sh = -((ex ? ex - 1075 : -1074) + 6);          // N = m 15625 / 2^sh
        unsigned long long q = 0;
        if (m != 0 && sh <= 0) {
            is_bad = true;
        } else if (m != 0 && sh < 68) {          // (from 2^68 on the quotient is 0 and the remainder below one half)
            const unsigned __int128 p = (unsigned __int128)m * 15625u;
            const unsigned __int128 quo = p >> sh, rem = p & ((((unsigned __int128)1) << sh) - 1), half = ((unsigned __int128)1) << (sh - 1);
            const unsigned __int128 r = quo + ((rem > half || (rem == half && ((unsigned long long)quo & 1ull))) ? 1 : 0);
            if (r > (unsigned __int128)BVH_FIELD_MAX) is_bad = true;
            else q = (unsigned long long)r;
        }
        if (is_bad) {          // does not fit: the field is filled with asterisks
#pragma unroll
            for (int k = 0; k < 15; ++k) c[k] = '*';
        } else {
            unsigned long long ip = q / 1000000ull, fp = q - ip * 1000000ull;
#pragma unroll
            for (int k = 14; k >= 9; --k) { c[k] = (unsigned char)('0' + fp % 10ull); fp /= 10ull; }
            c[8] = '.';
            bool sign = neg;
#pragma unroll
            for (int k = 7; k >= 0; --k) {
                if (k == 7 || ip != 0) { c[k] = (unsigned char)('0' + ip % 10ull); ip /= 10ull; }
                else if (sign) { c[k] = '-'; sign = false; }
            }
        }
    }
    bvh_u4 w;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        w[k] = (uint32_t)c[4 * k] | ((uint32_t)c[4 * k + 1] << 8) | ((uint32_t)c[4 * k + 2] << 16) | ((uint32_t)c[4 * k + 3] << 24);
    __builtin_nontemporal_store(w, reinterpret_cast<bvh_u4*>(text) + i);
    if (is_bad) {
        atomicAdd(bad, 1ull);
        atomicMin(bad + 1, (unsigned long long)(i / per_line));          // (-1 as the caller set it is the largest unsigned value)
    }
}

}  // namespace gem

extern "C" {

int gem_bvh_layout(int64_t* out) {
    using namespace gem;
    if (!out) { set_error("gem_bvh_layout: null argument"); return 1; }
    out[0] = BVH_NODES; out[1] = BVH_CHANNELS; out[2] = BVH_FIELD; out[3] = BVH_FRAME_BYTES;
    return 0;
}

int gem_bvh_tables(int32_t* parents, int32_t* joint_of_node, double* rest_dirs) {
    using namespace gem;
    if (!parents || !joint_of_node || !rest_dirs) { set_error("gem_bvh_tables: null argument"); return 1; }
    for (int n = 0; n < BVH_NODES; ++n) {
        parents[n] = BVH_PARENT[n];
        joint_of_node[n] = BVH_JOINT[n];
        for (int d = 0; d < 3; ++d) rest_dirs[3 * n + d] = BVH_REST[n][d];
    }
    return 0;
}

int gem_bvh_rest(const double* d_seq, int64_t n_frames, const double* d_crt, double* d_rest, void* stream) {
    using namespace gem;
    if (n_frames < 1) { set_error("gem_bvh_rest: need at least one frame"); return 1; }
    if (!d_seq || !d_rest) { set_error("gem_bvh_rest: null argument"); return 1; }
    BvhRestArgs a;
    a.seq = d_seq; a.crt = d_crt; a.rest = d_rest; a.n_frames = n_frames;
    for (int k = 0; k < 16; ++k)
        for (int i = 0; i < 4; ++i) a.ends[k][i] = 0;
    for (int n = 0; n < BVH_NODES; ++n) {
        a.bone_of_node[n] = bvh_has_rest(n) ? bvh_bone_index(n) : -1;
        if (!bvh_has_rest(n)) continue;
        int* e = a.ends[bvh_bone_index(n)];
        e[0] = bvh_node_joint(n, 0); e[1] = bvh_node_joint(n, 1);
        e[2] = bvh_node_joint(BVH_PARENT[n], 0); e[3] = bvh_node_joint(BVH_PARENT[n], 1);
    }
    hipLaunchKernelGGL(bvh_rest_kernel, dim3(1), dim3(ERR_ST), 0, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_bvh_channels(const double* d_seq, int64_t n_frames, const double* d_crt, const double* d_rest, double unit_scale,
                     double* d_channels, void* stream) {
    using namespace gem;
    if (n_frames < 0) { set_error("gem_bvh_channels: n_frames < 0"); return 1; }
    if (n_frames == 0) return 0;
    if (!d_seq || !d_rest || !d_channels) { set_error("gem_bvh_channels: null argument"); return 1; }
    if (n_frames > 0x7fffffffll * BVH_FT) { set_error("gem_bvh_channels: too many frames for one launch"); return 1; }
    hipLaunchKernelGGL(bvh_channels_kernel, dim3((unsigned)((n_frames + BVH_FT - 1) / BVH_FT)), dim3(BVH_FT), 0,
                       static_cast<hipStream_t>(stream), d_seq, n_frames, d_crt, unit_scale, d_channels);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_format_fields(const double* d_values, int64_t n_values, int64_t values_per_line, void* d_text, int64_t* d_bad, void* stream) {
    using namespace gem;
    if (n_values < 0 || values_per_line < 1) { set_error("gem_format_fields: need n_values >= 0 and values_per_line >= 1"); return 1; }
    if (reinterpret_cast<uintptr_t>(d_text) % 16) { set_error("gem_format_fields: the text must be 16-byte aligned"); return 1; }
    if (n_values == 0) return 0;
    if (!d_values || !d_text || !d_bad) { set_error("gem_format_fields: null argument"); return 1; }
    if (n_values > 0x7fffffffll * 256) { set_error("gem_format_fields: too many values for one launch"); return 1; }
    hipLaunchKernelGGL(format_fields_kernel, dim3((unsigned)((n_values + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       d_values, n_values, values_per_line, static_cast<unsigned char*>(d_text), reinterpret_cast<unsigned long long*>(d_bad));
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
