// Bridging the frames on which SLAM lost tracking.  Included from gem_api.hip.
//
//   gem_slam_bridge_work    the bytes of the work buffer a span of n frames needs (no GPU)
//   gem_slam_bridge         tracked poses, the mask, the system table and the chunk starts -> every frame's matrix, the per-chunk
//                           cameras and origins, the mask of invented frames and one 16-double record; TWO launches
//
// Kernel 1, one workgroup of 256 per system: the system's frames (its tracked neighbours and theirs included, 131 at most) are read
// into LDS, every unknown's thread builds its own row of the normal equations in the twin's order (no two threads write one entry),
// the workgroup factorises the matrix by columns (Cholesky, right-looking, the three right-hand sides carried along; every entry has
// ONE writer per column, so the order is fixed), substitutes back, and the unknowns' threads write their frames' matrices: translation
// = straight line between the system's neighbours + the solved offset, rotation by slerp between the gap's neighbours.  Thread 0
// leaves the system's share of the record in the work buffer.  Then all workgroups stride over the tracked frames and write theirs.
// Kernel 2 needs every G: a second launch, a thread per frame, cams[f] = inv(G[a]) G[f]; its first workgroup folds the systems'
// shares into the record (maxima and integer sums: exact in any order).  tests/bridge_twin.py is the specification.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>

#include "gem_internal.h"

namespace gem {

constexpr int BR_T = 256;
constexpr int BR_M = GEM_BRIDGE_MAX_GAP;             // unknowns of one system
constexpr int BR_SPAN = GEM_BRIDGE_MAX_SPAN;         // frames of one system
constexpr int BR_LOCAL = BR_SPAN + 4;                // ... with e - 1, e, s and s + 1
constexpr int BR_PART = 8;                           // doubles a system leaves in the work buffer
constexpr int BR_REC = GEM_BRIDGE_RECORD_DOUBLES;
constexpr int64_t BR_MAX_FRAMES = 1 << 20;
constexpr int BR_MAX_GRID = 256;                     // workgroups that stride over the tracked frames when the systems are fewer
constexpr double BR_SMALL_ANGLE = 1e-8;
static_assert(2 * BR_M - 1 == BR_SPAN, "64 lost frames with single tracked frames between them");
static_assert((BR_M * BR_M + 3 * BR_M + 6 * BR_LOCAL + 4 * BR_M) * 8 + (BR_LOCAL + 2 * BR_M + 4) * 4 <= 64 * 1024, "a system fits a workgroup's static LDS");

struct BridgeArgs {
    const double* poses;               // [n,7]
    const unsigned char* tracked;      // [n]
    const int32_t* systems;            // [n_systems,2]
    const int32_t* chunk_starts;       // [n_chunks]
    int n_systems, n_chunks, n;
    double *G, *cams, *origins;
    unsigned char* bridged;
    double* work;                      // [n_systems, BR_PART]
    double* rec;
};

__device__ __forceinline__ void br_unit(const double* q, double* out) {
#pragma clang fp contract(off)
    const double len = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; ++k) out[k] = q[k] / len;
}

// the 4x4 matrix of the unit quaternion q (x, y, z, w) and the translation c
__device__ __forceinline__ void br_matrix(const double* q, const double* c, double* G) {
#pragma clang fp contract(off)
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    G[0] = 1.0 - 2.0 * (y * y + z * z); G[1] = 2.0 * (x * y - z * w); G[2] = 2.0 * (x * z + y * w); G[3] = c[0];
    G[4] = 2.0 * (x * y + z * w); G[5] = 1.0 - 2.0 * (x * x + z * z); G[6] = 2.0 * (y * z - x * w); G[7] = c[1];
    G[8] = 2.0 * (x * z - y * w); G[9] = 2.0 * (y * z + x * w); G[10] = 1.0 - 2.0 * (x * x + y * y); G[11] = c[2];
    G[12] = 0.0; G[13] = 0.0; G[14] = 0.0; G[15] = 1.0;
}

// slerp between the quaternions a and b at u -> out (unit); returns the angle between the two quaternions
__device__ inline double br_slerp(const double* a, const double* b, double u, double* out) {
#pragma clang fp contract(off)
    double q0[4], q1[4], q[4];
    br_unit(a, q0);
    br_unit(b, q1);
    double d = q0[0] * q1[0] + q0[1] * q1[1] + q0[2] * q1[2] + q0[3] * q1[3];
    if (d < 0.0) {
        d = -d;
        for (int k = 0; k < 4; ++k) q1[k] = -q1[k];
    }
    const double theta = acos(d < 1.0 ? d : 1.0);
    if (theta < BR_SMALL_ANGLE) {
        for (int k = 0; k < 4; ++k) q[k] = (1.0 - u) * q0[k] + u * q1[k];
    } else {
        const double s0 = sin((1.0 - u) * theta), s1 = sin(u * theta), st = sin(theta);
        for (int k = 0; k < 4; ++k) q[k] = (s0 * q0[k] + s1 * q1[k]) / st;
    }
    br_unit(q, out);
    return theta;
}

// the point at local frame l of the straight line through the points at local frames le and ls
__device__ __forceinline__ void br_line(const double* cl, int le, int ls, int l, double* out) {
#pragma clang fp contract(off)
    const double u = (double)(l - le) / (double)(ls - le);
    for (int k = 0; k < 3; ++k) out[k] = cl[3 * le + k] + u * (cl[3 * ls + k] - cl[3 * le + k]);
}

__device__ __forceinline__ double br_norm3(const double* v) {
#pragma clang fp contract(off)
    return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}

__global__ __launch_bounds__(BR_T) void slam_bridge_solve_kernel(BridgeArgs a) {
    __shared__ double A[BR_M * BR_M];          // the normal equations, then their Cholesky factor (lower triangle)
    __shared__ double rhs[BR_M * 3];           // right-hand sides, then the offsets from the system's line
    __shared__ double cl[BR_LOCAL * 3];        // translations of the local frames
    __shared__ double kn[BR_LOCAL * 3];        // a tracked local frame's offset from the system's line
    __shared__ double share[BR_M * 4];         // per unknown: offset from its gap's line; where it begins a gap: lost frames, angle, distance
    __shared__ int kind[BR_LOCAL];             // unknown index; -1 tracked; -2 outside the span
    __shared__ int local_of[BR_M];
    __shared__ int m_shared, bad_shared;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < a.n_systems) {
        const int first = a.systems[2 * blockIdx.x], L = a.systems[2 * blockIdx.x + 1];
        double* part = a.work + (size_t)blockIdx.x * BR_PART;
        // (the host has checked the table; a row that would leave LDS or the arrays is not touched all the same)
        const bool usable = L >= 1 && L <= BR_SPAN && first >= 1 && (int64_t)first + L <= (int64_t)a.n - 1;
        const int base = first - 2, count = L + 4;          // local frame l is frame base + l: e at 1, s at L + 2
        if (usable) {
            if (tid < count) {
                const int t = base + tid;
                int k = -2;
                if (t >= 0 && t < a.n) {
                    k = a.tracked[t] ? -1 : -3;
                    for (int c = 0; c < 3; ++c) cl[3 * tid + c] = k == -1 ? a.poses[(size_t)t * 7 + c] : 0.0;
                }
                kind[tid] = k;
            }
            __syncthreads();
            if (tid == 0) {
                int m = 0, bad = 0;
                for (int l = 0; l < count; ++l)
                    if (kind[l] == -3) {
                        if (m < BR_M) { kind[l] = m; local_of[m] = l; ++m; } else { kind[l] = -1; bad = 1; }
                    }
                if (kind[1] != -1 || kind[L + 2] != -1) bad = 1;
                m_shared = m; bad_shared = bad;
            }
            __syncthreads();
        }
        const int m = usable ? m_shared : 0;
        if (!usable || bad_shared) {          // (uniform: nothing of this system is written but its share of the record)
            if (tid == 0) {
                for (int k = 0; k < BR_PART; ++k) part[k] = 0.0;
                part[6] = 1.0;
            }
        } else {
            const int le_sys = 1, ls_sys = L + 2;
            if (tid < count && kind[tid] == -1) {
#pragma clang fp contract(off)
                double on[3];
                br_line(cl, le_sys, ls_sys, tid, on);
                for (int c = 0; c < 3; ++c) kn[3 * tid + c] = cl[3 * tid + c] - on[c];
            }
            for (int i = tid; i < m * BR_M; i += BR_T) A[i] = 0.0;
            if (tid < 3 * m) rhs[tid] = 0.0;
            __syncthreads();
            // every unknown's row, in the twin's order: centre frames ascending, the triple's frames ascending
            if (tid < m) {
#pragma clang fp contract(off)
                const int p = local_of[tid];
                const double w[3] = {1.0, -2.0, 1.0};
                for (int tc = p - 1; tc <= p + 1; ++tc) {
                    if (tc < 1 || tc > L + 2 || kind[tc - 1] == -2 || kind[tc + 1] == -2) continue;
                    const double wp = w[p - (tc - 1)];
                    for (int r = 0; r < 3; ++r) {
                        const int lr = tc - 1 + r;
                        if (kind[lr] >= 0) {
                            A[tid * BR_M + kind[lr]] += wp * w[r];
                        } else {
                            for (int c = 0; c < 3; ++c) rhs[3 * tid + c] = rhs[3 * tid + c] - (wp * w[r]) * kn[3 * lr + c];
                        }
                    }
                }
            }
            __syncthreads();
            // Cholesky by columns; the right-hand sides are carried along (L y = b)
            int bad = 0;
            for (int j = 0; j < m; ++j) {
#pragma clang fp contract(off)
                const double d = A[j * BR_M + j];
                if (!(d > 0.0)) { bad = 1; break; }          // (every thread reads the same value)
                const double ljj = sqrt(d);
                const int r = m - j - 1;
                if (tid < r) A[(j + 1 + tid) * BR_M + j] = A[(j + 1 + tid) * BR_M + j] / ljj;
                if (tid >= BR_M && tid < BR_M + 3) rhs[3 * j + tid - BR_M] = rhs[3 * j + tid - BR_M] / ljj;
                __syncthreads();
                for (int idx = tid; idx < r * r; idx += BR_T) {
                    const int i = j + 1 + idx / r, k = j + 1 + idx % r;
                    if (k <= i) A[i * BR_M + k] = A[i * BR_M + k] - A[i * BR_M + j] * A[k * BR_M + j];
                }
                for (int idx = tid; idx < 3 * r; idx += BR_T) {
                    const int i = j + 1 + idx / 3, c = idx % 3;
                    rhs[3 * i + c] = rhs[3 * i + c] - A[i * BR_M + j] * rhs[3 * j + c];
                }
                __syncthreads();
            }
            // L^T x = y, by columns from the last
            for (int j = m - 1; j >= 0 && !bad; --j) {
#pragma clang fp contract(off)
                const double ljj = sqrt(A[j * BR_M + j]);
                if (tid < 3) rhs[3 * j + tid] = rhs[3 * j + tid] / ljj;
                __syncthreads();
                for (int idx = tid; idx < 3 * j; idx += BR_T) {
                    const int i = idx / 3, c = idx % 3;
                    rhs[3 * i + c] = rhs[3 * i + c] - A[j * BR_M + i] * rhs[3 * j + c];
                }
                __syncthreads();
            }
            if (bad) {          // not solved: the straight line, and the record says so
                __syncthreads();
                if (tid < 3 * m) rhs[tid] = 0.0;
                __syncthreads();
            }
            // the lost frames' matrices and their shares of the record
            if (tid < m) {
#pragma clang fp contract(off)
                const int l = local_of[tid], t = base + l;
                int le = l - 1, ls = l + 1;
                while (kind[le] >= 0) --le;
                while (kind[ls] >= 0) ++ls;
                double c[3], on[3], q[4], off[3];
                br_line(cl, le_sys, ls_sys, l, on);
                for (int k = 0; k < 3; ++k) c[k] = on[k] + rhs[3 * tid + k];
                br_line(cl, le, ls, l, on);
                for (int k = 0; k < 3; ++k) off[k] = c[k] - on[k];
                const double u = (double)(l - le) / (double)(ls - le);
                const double theta = br_slerp(a.poses + (size_t)(base + le) * 7 + 3, a.poses + (size_t)(base + ls) * 7 + 3, u, q);
                br_matrix(q, c, a.G + (size_t)t * 16);
                share[4 * tid] = br_norm3(off);
                const bool begins = le == l - 1;
                const double across[3] = {cl[3 * ls] - cl[3 * le], cl[3 * ls + 1] - cl[3 * le + 1], cl[3 * ls + 2] - cl[3 * le + 2]};
                share[4 * tid + 1] = begins ? (double)(ls - le - 1) : 0.0;
                share[4 * tid + 2] = begins ? 2.0 * theta : 0.0;
                share[4 * tid + 3] = begins ? br_norm3(across) : 0.0;
            }
            __syncthreads();
            if (tid == 0) {
                double gaps = 0.0, longest = 0.0, off = 0.0, angle = 0.0, far = 0.0;
                for (int i = 0; i < m; ++i) {
                    off = share[4 * i] > off ? share[4 * i] : off;
                    if (share[4 * i + 1] > 0.0) {
                        gaps += 1.0;
                        longest = share[4 * i + 1] > longest ? share[4 * i + 1] : longest;
                        angle = share[4 * i + 2] > angle ? share[4 * i + 2] : angle;
                        far = share[4 * i + 3] > far ? share[4 * i + 3] : far;
                    }
                }
                part[0] = (double)m; part[1] = gaps; part[2] = longest; part[3] = off; part[4] = angle; part[5] = far; part[6] = bad ? 1.0 : 0.0; part[7] = 0.0;
            }
        }
    }
    // the tracked frames, strided over by all workgroups
    for (int64_t f = (int64_t)blockIdx.x * BR_T + tid; f < a.n; f += (int64_t)gridDim.x * BR_T) {
        if (!a.tracked[f]) continue;
        double q[4];
        const double* p = a.poses + (size_t)f * 7;
        br_unit(p + 3, q);
        br_matrix(q, p, a.G + (size_t)f * 16);
    }
}

__global__ __launch_bounds__(BR_T) void slam_bridge_rebase_kernel(BridgeArgs a) {
    __shared__ double red[BR_T * 7];
    const int tid = threadIdx.x;
    const int64_t f = (int64_t)blockIdx.x * BR_T + tid;
    if (f < a.n) {
#pragma clang fp contract(off)
        int lo = 0, hi = a.n_chunks - 1;          // the last chunk that starts at or before f
        while (lo < hi) {
            const int mid = (lo + hi + 1) / 2;
            if ((int64_t)a.chunk_starts[mid] <= f) lo = mid; else hi = mid - 1;
        }
        const int64_t first = a.chunk_starts[lo];
        const double* Ga = a.G + (size_t)first * 16;
        const double* Gf = a.G + (size_t)f * 16;
        double* o = a.cams + (size_t)f * 16;
        const double d[3] = {Gf[3] - Ga[3], Gf[7] - Ga[7], Gf[11] - Ga[11]};
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) o[4 * i + j] = (Ga[i] * Gf[j] + Ga[4 + i] * Gf[4 + j]) + Ga[8 + i] * Gf[8 + j];
            o[4 * i + 3] = (Ga[i] * d[0] + Ga[4 + i] * d[1]) + Ga[8 + i] * d[2];
        }
        o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
        if (f == first) {
            double* org = a.origins + (size_t)lo * 16;
            for (int k = 0; k < 16; ++k) org[k] = Ga[k];
        }
        a.bridged[f] = a.tracked[f] ? 0 : 1;
    }
    if (blockIdx.x != 0) return;
    // the record: integer sums and maxima of the systems' shares
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < a.n_systems; i += BR_T) {
        const double* part = a.work + (size_t)i * BR_PART;
        v[0] += part[0]; v[1] += part[1]; v[6] += part[6];
        for (int k = 2; k < 6; ++k) v[k] = part[k] > v[k] ? part[k] : v[k];
    }
    for (int k = 0; k < 7; ++k) red[tid * 7 + k] = v[k];
    __syncthreads();
    if (tid != 0) return;
    for (int i = 1; i < BR_T; ++i) {
        v[0] += red[i * 7]; v[1] += red[i * 7 + 1]; v[6] += red[i * 7 + 6];
        for (int k = 2; k < 6; ++k) v[k] = red[i * 7 + k] > v[k] ? red[i * 7 + k] : v[k];
    }
    a.rec[0] = v[6] > 0.0 ? (double)GEM_BRIDGE_NOT_SOLVED : 0.0;
    a.rec[1] = (double)a.n; a.rec[2] = v[0]; a.rec[3] = v[1]; a.rec[4] = (double)a.n_systems; a.rec[5] = v[2]; a.rec[6] = v[3]; a.rec[7] = v[4];
    a.rec[8] = v[5];
    for (int k = 9; k < BR_REC; ++k) a.rec[k] = 0.0;
}

inline int64_t bridge_work_doubles(int64_t n) { return ((n + 1) / 2) * BR_PART + BR_PART; }

}  // namespace gem

extern "C" {

int64_t gem_slam_bridge_work(int64_t n) {
    using namespace gem;
    if (n < 1 || n > BR_MAX_FRAMES) { set_error("gem_slam_bridge_work: n must lie in 1 .. 2^20"); return -1; }
    return bridge_work_doubles(n) * (int64_t)sizeof(double);
}

int gem_slam_bridge(const double* d_poses, const unsigned char* h_tracked, const unsigned char* d_tracked, const int32_t* h_systems,
                    const int32_t* d_systems, int n_systems, const int32_t* h_chunk_starts, const int32_t* d_chunk_starts, int n_chunks,
                    int64_t n, double* d_G, double* d_cams, double* d_origins, unsigned char* d_bridged, double* d_work, int64_t work_bytes,
                    double* d_record, void* stream) {
    using namespace gem;
    if (n < 1 || n > BR_MAX_FRAMES) { set_error("gem_slam_bridge: n must lie in 1 .. 2^20"); return 1; }
    if (n_systems < 0 || n_systems > n / 2) { set_error("gem_slam_bridge: n_systems must lie in 0 .. n / 2"); return 1; }
    if (n_chunks < 1 || n_chunks > n) { set_error("gem_slam_bridge: n_chunks must lie in 1 .. n"); return 1; }
    const struct { const void* p; const char* name; } needed[] = {
        {d_poses, "d_poses"}, {h_tracked, "h_tracked"}, {d_tracked, "d_tracked"}, {h_chunk_starts, "h_chunk_starts"}, {d_chunk_starts, "d_chunk_starts"},
        {d_G, "d_G"}, {d_cams, "d_cams"}, {d_origins, "d_origins"}, {d_bridged, "d_bridged"}, {d_work, "d_work"}, {d_record, "d_record"}};
    for (const auto& x : needed)
        if (!x.p) { set_error(std::string("gem_slam_bridge: ") + x.name + " is null"); return 1; }
    if (n_systems > 0 && !h_systems) { set_error("gem_slam_bridge: h_systems is null"); return 1; }
    if (n_systems > 0 && !d_systems) { set_error("gem_slam_bridge: d_systems is null"); return 1; }
    const struct { const void* p; const char* name; } doubles[] = {{d_poses, "d_poses"}, {d_G, "d_G"}, {d_cams, "d_cams"}, {d_origins, "d_origins"},
                                                                    {d_work, "d_work"}, {d_record, "d_record"}};
    for (const auto& x : doubles)
        if (reinterpret_cast<uintptr_t>(x.p) & 7) { set_error(std::string("gem_slam_bridge: ") + x.name + " must be 8-byte aligned"); return 1; }
    const struct { const void* p; const char* name; } ints[] = {{h_systems, "h_systems"}, {d_systems, "d_systems"}, {h_chunk_starts, "h_chunk_starts"},
                                                                 {d_chunk_starts, "d_chunk_starts"}};
    for (const auto& x : ints)
        if (reinterpret_cast<uintptr_t>(x.p) & 3) { set_error(std::string("gem_slam_bridge: ") + x.name + " must be 4-byte aligned"); return 1; }
    const int64_t need = bridge_work_doubles(n) * (int64_t)sizeof(double);
    if (work_bytes < need) { set_error("gem_slam_bridge: d_work holds " + std::to_string(work_bytes) + " bytes, " + std::to_string(need) + " are needed"); return 1; }
    if (!h_tracked[0] || !h_tracked[n - 1]) { set_error("gem_slam_bridge: h_tracked: the first and the last frame must be tracked"); return 1; }
    if (h_chunk_starts[0] != 0) { set_error("gem_slam_bridge: h_chunk_starts must begin with 0"); return 1; }
    for (int k = 1; k < n_chunks; ++k)
        if (h_chunk_starts[k] <= h_chunk_starts[k - 1] || h_chunk_starts[k] >= n) {
            set_error("gem_slam_bridge: h_chunk_starts: chunk " + std::to_string(k) + " does not start behind its predecessor and inside the span"); return 1;
        }
    // the system table must be the one of the mask
    int64_t lost = 0, covered = 0, behind = 0;
    for (int64_t t = 0; t < n; ++t) lost += h_tracked[t] ? 0 : 1;
    for (int i = 0; i < n_systems; ++i) {
        const int64_t first = h_systems[2 * i], L = h_systems[2 * i + 1];
        const std::string who = "gem_slam_bridge: h_systems: system " + std::to_string(i);
        if (L < 1 || first < 1 || first + L > n - 1) { set_error(who + " does not lie inside the span with a tracked frame on either side"); return 1; }
        if (L > BR_SPAN) { set_error(who + " is longer than " + std::to_string(BR_SPAN) + " frames"); return 1; }
        if (first < behind + 2 && i > 0) { set_error(who + " must lie at least two tracked frames behind its predecessor"); return 1; }
        if (h_tracked[first] || h_tracked[first + L - 1] || !h_tracked[first - 1] || !h_tracked[first + L]) {
            set_error(who + " must begin and end with a lost frame and have tracked neighbours"); return 1;
        }
        int64_t unknowns = 0;
        for (int64_t t = first; t < first + L; ++t) {
            unknowns += h_tracked[t] ? 0 : 1;
            if (h_tracked[t] && h_tracked[t + 1]) { set_error(who + " holds two tracked frames in a row: these are two systems"); return 1; }
        }
        if (unknowns > BR_M) { set_error(who + " is longer than " + std::to_string(BR_M) + " lost frames"); return 1; }
        covered += unknowns;
        behind = first + L;
    }
    if (covered != lost) { set_error("gem_slam_bridge: h_systems: " + std::to_string(lost - covered) + " lost frames of h_tracked lie in no system"); return 1; }
    BridgeArgs a;
    a.poses = d_poses; a.tracked = d_tracked; a.systems = d_systems; a.chunk_starts = d_chunk_starts;
    a.n_systems = n_systems; a.n_chunks = n_chunks; a.n = (int)n;
    a.G = d_G; a.cams = d_cams; a.origins = d_origins; a.bridged = d_bridged; a.work = d_work; a.rec = d_record;
    const int64_t frame_groups = (n + BR_T - 1) / BR_T;
    const int64_t grid = std::max<int64_t>(n_systems, std::min<int64_t>(frame_groups, BR_MAX_GRID));
    hipLaunchKernelGGL(slam_bridge_solve_kernel, dim3((unsigned)grid), dim3(BR_T), 0, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(slam_bridge_rebase_kernel, dim3((unsigned)frame_groups), dim3(BR_T), 0, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
