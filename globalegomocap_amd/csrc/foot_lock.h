// Foot-skate clean-up of a pose sequence: every stance of a foot is held at one place on the floor, the legs re-solved by two-bone
// inverse kinematics.  Included from errors.hip, behind ground.h.
//
//   gem_foot_lock_work    the work-buffer offsets of the sequences and the bytes they need (no GPU)
//   gem_foot_lock         a table of sequences and their gem_ground_plane records -> the cleaned sequences and one 24-double
//                         record each, ONE launch, a workgroup of 1024 per sequence
//
// The contact rule is ground.h's (gr_contact: a candidate within tau_h of the plane), the plane is read from the sequence's ground
// record on the device.  A RUN is a maximal stretch of at least min_run contact frames of one foot; its ANCHOR the mean of the foot
// point over it, put onto the plane; inside a run the foot point is moved onto the anchor, around it the correction is eased out
// over `blend` frames; the leg follows by two-bone inverse kinematics from the unmoved hip.  tests/foot_lock_twin.py is the
// specification, step for step.
//
// Everything is float64.  The foot points lie in LDS up to GEM_GROUND_LDS_FRAMES frames (48 KB) and in the work buffer beyond, as in
// ground.h; the corrections are not stored: the pass that moves a leg computes its frame's correction from the run table (two
// anchors and two foot points at most), so the static 64 KB of LDS are enough at every length.  The contact flags, the prefix counts
// and the run table (starts, ends, anchors) lie in the work buffer at every length.  Runs are found without a search: the number of
// run starts at or before a frame is an integer prefix count (exact in any order), which is the frame's own or preceding run's
// index + 1; the threads that stand on a run's first and last frame write its bounds.  An anchor is summed by one wavefront (lanes
// stride over the run's frames, DPP) or, for a run longer than FL_LONG_RUN frames, by the workgroup (block_sums): a standing wearer
// is one run as long as the sequence.  Every sum has a fixed order and there are no floating-point atomics: two calls give the same
// bytes.  The whole output block is written here: copied from the input, then the legs that move.
#pragma once
#include "ground.h"

namespace gem {

constexpr int FL_REC = GEM_FOOT_LOCK_RECORD_DOUBLES;
constexpr int FL_LONG_RUN = 1024;          // a longer run's anchor is summed by the workgroup, not by one wavefront
constexpr double FL_DEGENERATE = 1e-9;     // a direction shorter than this is none
constexpr double FL_ON_PLANE = 1e-12;      // an anchor this near the plane is on it
static_assert(GR_LDS_FRAMES * 48 + 2 * 16 * ERR_NW * 8 + 1024 <= 64 * 1024, "the foot points and the sums' partials fit a workgroup's static LDS");

struct FootLockArgs {
    const int64_t* table;      // device: [n] input addresses, [n] frames, [n] output addresses, [n] work offsets (doubles)
    int n, lag, min_run, blend, snap;
    double tau_v, tau_h, stretch;
    const double* ground;      // [n, GR_REC]
    double* work;
    double* rec;               // [n, FL_REC]
};

// where a sequence of F frames keeps what in its part of the work buffer (offsets in doubles) and how long that part is
struct FootLockWork {
    int64_t runs, anchors, bounds, prefix, flags, total;
};
__host__ __device__ inline FootLockWork fl_work(int64_t F) {
    FootLockWork w;
    w.runs = (F + 1) / 2;                                          // the most runs one foot can have
    w.anchors = F > GR_LDS_FRAMES ? 6 * F : 0;                     // [2, runs, 3] doubles (the foot points of a long sequence come first)
    w.bounds = w.anchors + 6 * w.runs;                             // [2, runs, 2] int32: first and last frame
    w.prefix = w.bounds + 2 * w.runs;                              // [2, F] int32: run starts at or before the frame
    w.flags = w.prefix + F;                                        // [F, 2] bytes: in contact
    w.total = w.flags + (2 * F + 7) / 8;
    return w;
}

__device__ __forceinline__ double fl_norm(const double* v) { return sqrt(gr_dot(v, v)); }

// k(u) = 1 - u^2 (3 - 2 u) on [0, 1], 0 beyond
__device__ __forceinline__ double fl_ease(double u) {
#pragma clang fp contract(off)
    return u < 1.0 ? 1.0 - (u * u) * (3.0 - 2.0 * u) : 0.0;
}

// a frame's view of its foot's runs
struct FootLockRuns {
    const double* anchors;     // [runs, 3]
    const int* bounds;         // [runs, 2]
    const int* prefix;         // [F]: run starts at or before the frame
    int count;
};

// the correction of foot point (f, side) -> whether the frame lies inside a run (`run`: which)
__device__ inline bool fl_delta(const double* q, int f, int side, const FootLockRuns& t, int blend, double* delta, int& run) {
#pragma clang fp contract(off)
    const int r = t.prefix[f] - 1;
    run = r;
    const double* p = q + ((size_t)f * 2 + side) * 3;
    if (r >= 0 && f <= t.bounds[2 * r + 1]) {
        for (int k = 0; k < 3; ++k) delta[k] = t.anchors[3 * r + k] - p[k];
        return true;
    }
    const bool before = r >= 0, after = r + 1 < t.count;
    double B = (double)blend;
    if (before && after) {
        const double half = 0.5 * (double)(t.bounds[2 * (r + 1)] - t.bounds[2 * r + 1]);
        B = half < B ? half : B;
    }
    delta[0] = 0.0; delta[1] = 0.0; delta[2] = 0.0;
    if (before) {
        const int e = t.bounds[2 * r + 1];
        const double* pe = q + ((size_t)e * 2 + side) * 3;
        const double w = fl_ease((double)(f - e) / B);
        for (int k = 0; k < 3; ++k) delta[k] = delta[k] + (t.anchors[3 * r + k] - pe[k]) * w;
    }
    if (after) {
        const int s = t.bounds[2 * (r + 1)];
        const double* ps = q + ((size_t)s * 2 + side) * 3;
        const double w = fl_ease((double)(s - f) / B);
        for (int k = 0; k < 3; ++k) delta[k] = delta[k] + (t.anchors[3 * (r + 1) + k] - ps[k]) * w;
    }
    return false;
}

// v without its part along the unit vector u
__device__ __forceinline__ void fl_across(const double* v, const double* u, double* w) {
#pragma clang fp contract(off)
    const double along = gr_dot(v, u);
    for (int k = 0; k < 3; ++k) w[k] = v[k] - along * u[k];
}

// the leg (hip h, knee, ankle, foot) with its ankle moved by delta -> knee2, ankle2, foot2, the lengthening g and the kind:
// 0 reachable, 1 too far and held, 2 too far and missed, 3 too near
__device__ inline int fl_solve_leg(const double* h, const double* knee, const double* ankle, const double* foot, const double* delta, double stretch,
                                   double* knee2, double* ankle2, double* foot2, double& g) {
#pragma clang fp contract(off)
    double a[3], b[3], t[3], u[3];
    for (int k = 0; k < 3; ++k) { a[k] = knee[k] - h[k]; b[k] = ankle[k] - knee[k]; }
    const double l1 = fl_norm(a), l2 = fl_norm(b);
    for (int k = 0; k < 3; ++k) { t[k] = ankle[k] + delta[k]; u[k] = t[k] - h[k]; }
    const double D = fl_norm(u);
    int kind = 0;
    g = 1.0;
    if (D >= l1 + l2) {
        for (int k = 0; k < 3; ++k) u[k] = u[k] / D;
        const double ratio = D / (l1 + l2), most = 1.0 + stretch;
        g = ratio < most ? ratio : most;
        kind = ratio > most ? 2 : 1;
        const double gk = g * l1, ga = g * (l1 + l2);
        for (int k = 0; k < 3; ++k) { knee2[k] = h[k] + gk * u[k]; ankle2[k] = h[k] + ga * u[k]; }
    } else if (D <= fabs(l1 - l2)) {
        kind = 3;
        if (D < FL_DEGENERATE) {          // the target is the hip itself: fold along the leg as it is
            double v[3];
            for (int k = 0; k < 3; ++k) v[k] = ankle[k] - h[k];
            const double len = fl_norm(v);
            if (len < FL_DEGENERATE) {
                for (int k = 0; k < 3; ++k) { knee2[k] = knee[k]; ankle2[k] = ankle[k]; foot2[k] = foot[k]; }
                return kind;
            }
            for (int k = 0; k < 3; ++k) u[k] = v[k] / len;
        } else {
            for (int k = 0; k < 3; ++k) u[k] = u[k] / D;
        }
        const double lk = l1 >= l2 ? l1 : -l1, la = fabs(l1 - l2);
        for (int k = 0; k < 3; ++k) { knee2[k] = h[k] + lk * u[k]; ankle2[k] = h[k] + la * u[k]; }
    } else {
        for (int k = 0; k < 3; ++k) u[k] = u[k] / D;
        const double c = (l1 * l1 - l2 * l2 + D * D) / (2.0 * D);
        const double ss = l1 * l1 - c * c;
        const double s = sqrt(ss > 0.0 ? ss : 0.0);
        double w[3];
        fl_across(a, u, w);
        if (fl_norm(w) < FL_DEGENERATE) {
            double v[3];
            for (int k = 0; k < 3; ++k) v[k] = foot[k] - ankle[k];
            fl_across(v, u, w);
            if (fl_norm(w) < FL_DEGENERATE) {          // the axis rule of the upright transform (ground.h, step 8)
                int e = 0;
                for (int k = 1; k < 3; ++k)
                    if (fabs(u[k]) < fabs(u[e])) e = k;
                for (int k = 0; k < 3; ++k) w[k] = (k == e ? 1.0 : 0.0) - u[e] * u[k];
            }
        }
        const double wl = fl_norm(w);
        for (int k = 0; k < 3; ++k) { knee2[k] = (h[k] + c * u[k]) + s * (w[k] / wl); ankle2[k] = t[k]; }
    }
    for (int k = 0; k < 3; ++k) foot2[k] = foot[k] + (ankle2[k] - ankle[k]);
    return kind;
}

// a run's anchor from the sum of its foot points about the first: the mean, put onto the plane
__device__ inline void fl_anchor(const double* first, const double* acc, int len, bool snap, const double* n, double d, double* out) {
#pragma clang fp contract(off)
    double a[3];
    for (int k = 0; k < 3; ++k) a[k] = first[k] + acc[k] / (double)len;
    if (snap) {
        const double off = gr_dot(n, a) - d;
        if (!(fabs(off) < FL_ON_PLANE))
            for (int k = 0; k < 3; ++k) a[k] = a[k] - off * n[k];
    }
    for (int k = 0; k < 3; ++k) out[k] = a[k];
}

// the in-plane length of q1 - q0
__device__ __forceinline__ double fl_slide(const double* q0, const double* q1, const double* n) {
#pragma clang fp contract(off)
    double v[3] = {q1[0] - q0[0], q1[1] - q0[1], q1[2] - q0[2]};
    const double along = gr_dot(v, n);
    for (int k = 0; k < 3; ++k) v[k] = v[k] - along * n[k];
    return sqrt(gr_dot(v, v));
}

__global__ __launch_bounds__(ERR_ST) void foot_lock_kernel(FootLockArgs a) {
    __shared__ double qs[GR_LDS_FRAMES * 6];
    __shared__ double red[2 * 16 * ERR_NW];
    __shared__ double mx[ERR_NW];
    __shared__ int wave_total[2][ERR_NW];
    const int tid = threadIdx.x, seq = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    int parity = 0;
    double* rec = a.rec + (size_t)seq * FL_REC;
    const int64_t addr = a.table[seq], frames = a.table[a.n + seq], out_addr = a.table[2 * a.n + seq], work_at = a.table[3 * a.n + seq];
    for (int k = tid; k < FL_REC; k += ERR_ST) rec[k] = 0.0;
    __syncthreads();
    if (addr == 0 || (addr & 7) || out_addr == 0 || (out_addr & 7) || out_addr == addr || frames < 1 || frames > GR_MAX_FRAMES || work_at < 0) {
        if (tid == 0) rec[0] = (double)GEM_FOOT_LOCK_BAD_SEQUENCE;
        return;
    }
    const int F = (int)frames;
    const double* x = reinterpret_cast<const double*>(addr);
    double* y = reinterpret_cast<double*>(out_addr);
    // 0. the whole block, copied; the legs that move are written over it in step 5
    for (size_t k = tid; k < (size_t)F * GR_J * 3; k += ERR_ST) y[k] = x[k];
    const double* g = a.ground + (size_t)seq * GR_REC;
    if (!(g[0] == 0.0)) {
        if (tid == 0) { rec[0] = (double)GEM_FOOT_LOCK_BAD_GROUND; rec[15] = (double)F; }
        return;
    }
    const double n[3] = {g[2], g[3], g[4]}, d = g[5];
    const FootLockWork w = fl_work(F);
    double* part = a.work + work_at;
    double* q = F <= GR_LDS_FRAMES ? qs : part;
    double* anchors = part + w.anchors;
    int* bounds = reinterpret_cast<int*>(part + w.bounds);
    int* prefix = reinterpret_cast<int*>(part + w.prefix);
    unsigned char* flags = reinterpret_cast<unsigned char*>(part + w.flags);
    // 1. foot points (ground.h, step 1)
    for (int f = tid; f < F; f += ERR_ST) {
#pragma clang fp contract(off)
        const double* p = x + (size_t)f * GR_J * 3;
        double* o = q + (size_t)f * 6;
        for (int dd = 0; dd < 3; ++dd) {
            o[dd] = 0.5 * (p[9 * 3 + dd] + p[10 * 3 + dd]);
            o[3 + dd] = 0.5 * (p[13 * 3 + dd] + p[14 * 3 + dd]);
        }
    }
    __threadfence();
    __syncthreads();
    //    contact flags
    for (int i = tid; i < 2 * F; i += ERR_ST) flags[i] = gr_contact(q, i, F, a.lag, a.tau_v, a.tau_h, n, d) ? 1 : 0;
    __threadfence();
    __syncthreads();
    // 2. runs: every thread counts the run starts of its stretch of frames, an integer scan over the threads, and the second walk
    //    writes the prefix counts and the runs' bounds
    const int per = (F + ERR_ST - 1) / ERR_ST;
    const int f_lo = tid * per < F ? tid * per : F, f_hi = f_lo + per < F ? f_lo + per : F;
    auto starts = [&](int f, int side) {          // a run of at least min_run frames begins at f
        if (!flags[2 * f + side] || (f > 0 && flags[2 * (f - 1) + side])) return false;
        if (a.min_run > F - f) return false;
        for (int k = 1; k < a.min_run; ++k)
            if (!flags[2 * (f + k) + side]) return false;
        return true;
    };
    auto ends = [&](int f, int side) {            // such a run ends at f
        if (!flags[2 * f + side] || (f + 1 < F && flags[2 * (f + 1) + side])) return false;
        if (f + 1 < a.min_run) return false;
        for (int k = 1; k < a.min_run; ++k)
            if (!flags[2 * (f - k) + side]) return false;
        return true;
    };
    int base[2], count[2];
    for (int side = 0; side < 2; ++side) {
        int c = 0;
        for (int f = f_lo; f < f_hi; ++f) c += starts(f, side) ? 1 : 0;
        int v = c;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(v, o);
            if (lane >= o) v += t;
        }
        if (lane == 63) wave_total[side][wave] = v;
        base[side] = v - c;
    }
    __syncthreads();
    for (int side = 0; side < 2; ++side) {
        int total = 0;
        for (int i = 0; i < ERR_NW; ++i) {
            if (i == wave) base[side] += total;
            total += wave_total[side][i];
        }
        count[side] = total;
    }
    for (int side = 0; side < 2; ++side) {
        int c = base[side];
        int* pre = prefix + (size_t)side * F;
        int* bnd = bounds + (size_t)side * w.runs * 2;
        for (int f = f_lo; f < f_hi; ++f) {
            if (starts(f, side)) { bnd[2 * c] = f; ++c; }
            pre[f] = c;
            if (c > 0 && ends(f, side)) bnd[2 * (c - 1) + 1] = f;
        }
    }
    __threadfence();
    __syncthreads();
    if (count[0] + count[1] == 0) {
        if (tid == 0) { rec[0] = (double)GEM_FOOT_LOCK_NO_CONTACT; rec[11] = 1.0; rec[15] = (double)F; }
        return;
    }
    // 3. anchors: a wavefront per run, the workgroup for a long one
    for (int j = wave; j < count[0] + count[1]; j += ERR_NW) {
        const int side = j >= count[0] ? 1 : 0, r = j - side * count[0];
        const int* bnd = bounds + ((size_t)side * w.runs + r) * 2;
        const int s = bnd[0], e = bnd[1];
        if (e - s + 1 > FL_LONG_RUN) continue;
        const double* first = q + ((size_t)s * 2 + side) * 3;
        double acc[3] = {0.0, 0.0, 0.0};
        for (int f = s + lane; f <= e; f += 64) {
#pragma clang fp contract(off)
            const double* p = q + ((size_t)f * 2 + side) * 3;
            for (int k = 0; k < 3; ++k) acc[k] += p[k] - first[k];
        }
        for (int k = 0; k < 3; ++k) acc[k] = wave_sum_dpp(acc[k]);
        if (lane == 0) fl_anchor(first, acc, e - s + 1, a.snap != 0, n, d, anchors + ((size_t)side * w.runs + r) * 3);
    }
    for (int m = 0; m < F; m += FL_LONG_RUN)          // (a long run holds a multiple of FL_LONG_RUN: the first one it holds stands for it)
        for (int side = 0; side < 2; ++side) {
            const int r = prefix[(size_t)side * F + m] - 1;
            if (r < 0) continue;
            const int* bnd = bounds + ((size_t)side * w.runs + r) * 2;
            const int s = bnd[0], e = bnd[1];
            if (m > e || e - s + 1 <= FL_LONG_RUN || m - s >= FL_LONG_RUN) continue;
            const double* first = q + ((size_t)s * 2 + side) * 3;
            double acc[3] = {0.0, 0.0, 0.0};
            for (int f = s + tid; f <= e; f += ERR_ST) {
#pragma clang fp contract(off)
                const double* p = q + ((size_t)f * 2 + side) * 3;
                for (int k = 0; k < 3; ++k) acc[k] += p[k] - first[k];
            }
            block_sums<3>(acc, red, parity);
            if (tid == 0) fl_anchor(first, acc, e - s + 1, a.snap != 0, n, d, anchors + ((size_t)side * w.runs + r) * 3);
        }
    __threadfence();
    __syncthreads();
    // 4. + 5. every frame's corrections from the run table, and the legs that move
    double sums[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};          // pinned right, left; changed; lengthened; unreachable; |delta| over pinned; slide before, its pairs; slide after
    double delta_max = 0.0, knee_max = 0.0, g_max = 1.0;
    for (int f = tid; f < F; f += ERR_ST) {
        bool touched = false;
        for (int side = 0; side < 2; ++side) {
            const FootLockRuns t = {anchors + (size_t)side * w.runs * 3, bounds + (size_t)side * w.runs * 2, prefix + (size_t)side * F, count[side]};
            double delta[3];
            int run;
            const bool pinned = fl_delta(q, f, side, t, a.blend, delta, run);
            if (pinned) {
                const double size = fl_norm(delta);
                sums[side] += 1.0; sums[5] += size;
                delta_max = size > delta_max ? size : delta_max;
                if (f + 1 <= t.bounds[2 * run + 1]) {
                    sums[6] += fl_slide(q + ((size_t)f * 2 + side) * 3, q + ((size_t)(f + 1) * 2 + side) * 3, n);
                    sums[7] += 1.0;
                }
            }
            if (!(delta[0] != 0.0 || delta[1] != 0.0 || delta[2] != 0.0)) continue;
            touched = true;
            const int hip = side ? GR_LHIP : GR_RHIP;
            const double* p = x + ((size_t)f * GR_J + hip) * 3;
            double* o = y + ((size_t)f * GR_J + hip) * 3;
            double knee2[3], ankle2[3], foot2[3], gg;
            const int kind = fl_solve_leg(p, p + 3, p + 6, p + 9, delta, a.stretch, knee2, ankle2, foot2, gg);
            sums[3] += (kind == 1 || kind == 2) ? 1.0 : 0.0;
            sums[4] += (kind == 2 || kind == 3) ? 1.0 : 0.0;
            g_max = gg > g_max ? gg : g_max;
            double moved[3];
            for (int k = 0; k < 3; ++k) {
                moved[k] = knee2[k] - p[3 + k];
                o[3 + k] = knee2[k]; o[6 + k] = ankle2[k]; o[9 + k] = foot2[k];
            }
            const double far = fl_norm(moved);
            knee_max = far > knee_max ? far : knee_max;
        }
        sums[2] += touched ? 1.0 : 0.0;
    }
    __threadfence();
    __syncthreads();
    // 6. the slide that is left, from the sequence as it was written
    for (int f = tid; f < F; f += ERR_ST)
        for (int side = 0; side < 2; ++side) {
#pragma clang fp contract(off)
            const int r = prefix[(size_t)side * F + f] - 1;
            if (r < 0 || f + 1 > bounds[((size_t)side * w.runs + r) * 2 + 1]) continue;
            const int ankle = side ? 13 : 9;
            const double* p0 = y + ((size_t)f * GR_J + ankle) * 3;
            const double* p1 = p0 + GR_J * 3;
            double q0[3], q1[3];
            for (int k = 0; k < 3; ++k) { q0[k] = 0.5 * (p0[k] + p0[3 + k]); q1[k] = 0.5 * (p1[k] + p1[3 + k]); }
            sums[8] += fl_slide(q0, q1, n);
        }
    block_sums<9>(sums, red, parity);
    delta_max = gr_block_max(delta_max, mx);
    knee_max = gr_block_max(knee_max, mx);
    g_max = gr_block_max(g_max, mx);
    if (tid != 0) return;
    rec[0] = 0.0; rec[1] = (double)count[0]; rec[2] = (double)count[1]; rec[3] = sums[0]; rec[4] = sums[1]; rec[5] = sums[2]; rec[6] = sums[3];
    rec[7] = sums[4]; rec[8] = delta_max; rec[9] = sums[5] / (sums[0] + sums[1]); rec[10] = knee_max; rec[11] = g_max;
    rec[12] = sums[7] > 0.0 ? sums[6] / sums[7] : 0.0; rec[13] = sums[7] > 0.0 ? sums[8] / sums[7] : 0.0; rec[14] = sums[7]; rec[15] = (double)F;
}

// the work offsets (doubles) of the sequences, -1 for one whose frame count cannot be used; -> doubles in all
inline int64_t foot_lock_work_doubles(const int64_t* frames, int n, int64_t* offsets) {
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        const bool fine = frames[i] >= 1 && frames[i] <= GR_MAX_FRAMES;
        if (offsets) offsets[i] = fine ? at : -1;
        if (fine) at += fl_work(frames[i]).total;
    }
    return at;
}

}  // namespace gem

extern "C" {

int64_t gem_foot_lock_work(const int64_t* h_frames, int n_sequences, int64_t* h_offsets) {
    using namespace gem;
    if (!h_frames || n_sequences < 1 || n_sequences > (1 << 20)) { set_error("gem_foot_lock_work: need the frame counts of 1 .. 2^20 sequences"); return -1; }
    return foot_lock_work_doubles(h_frames, n_sequences, h_offsets) * (int64_t)sizeof(double);
}

int gem_foot_lock(const int64_t* h_table, const int64_t* d_table, int n_sequences, const double* d_ground_records, int lag, double tau_v, double tau_h,
                  int min_run, int blend, int snap, double stretch, double* d_work, int64_t work_bytes, double* d_records, void* stream) {
    using namespace gem;
    if (n_sequences < 1 || n_sequences > (1 << 20)) { set_error("gem_foot_lock: n_sequences must lie in 1 .. 2^20"); return 1; }          // (no grid of zero workgroups)
    if (lag < 1) { set_error("gem_foot_lock: lag must be at least 1"); return 1; }
    if (!(tau_v > 0.0) || !std::isfinite(tau_v)) { set_error("gem_foot_lock: tau_v must be positive and finite"); return 1; }
    if (!(tau_h > 0.0) || !std::isfinite(tau_h)) { set_error("gem_foot_lock: tau_h must be positive and finite"); return 1; }
    if (min_run < 1) { set_error("gem_foot_lock: min_run must be at least 1"); return 1; }
    if (blend < 1) { set_error("gem_foot_lock: blend must be at least 1"); return 1; }
    if (!(stretch >= 0.0) || !std::isfinite(stretch)) { set_error("gem_foot_lock: stretch must be finite and not negative"); return 1; }
    if (!h_table) { set_error("gem_foot_lock: h_table is null"); return 1; }
    if (!d_table) { set_error("gem_foot_lock: d_table is null"); return 1; }
    if (!d_ground_records) { set_error("gem_foot_lock: d_ground_records is null"); return 1; }
    if (!d_records) { set_error("gem_foot_lock: d_records is null"); return 1; }
    if ((reinterpret_cast<uintptr_t>(d_table) | reinterpret_cast<uintptr_t>(d_ground_records) | reinterpret_cast<uintptr_t>(d_records) |
         reinterpret_cast<uintptr_t>(d_work)) & 7) {
        set_error("gem_foot_lock: d_table, d_ground_records, d_work and d_records must be 8-byte aligned"); return 1;
    }
    // the work offsets must be the ones gem_foot_lock_work gives (parts that do not overlap, inside d_work), and no sequence is locked in place
    int64_t at = 0;
    for (int i = 0; i < n_sequences; ++i) {
        const int64_t in = h_table[i], frames = h_table[n_sequences + i], out = h_table[2 * (int64_t)n_sequences + i], given = h_table[3 * (int64_t)n_sequences + i];
        const bool fine = frames >= 1 && frames <= GR_MAX_FRAMES;
        if (given != (fine ? at : -1)) { set_error("gem_foot_lock: sequence " + std::to_string(i) + ": its work offset is not the one gem_foot_lock_work gives"); return 1; }
        if (fine) at += fl_work(frames).total;
        if ((in | out) & 7) { set_error("gem_foot_lock: sequence " + std::to_string(i) + ": its addresses must be 8-byte aligned"); return 1; }
        const int64_t bytes = fine ? frames * GR_J * 3 * (int64_t)sizeof(double) : 0;
        if (in != 0 && out != 0 && (in == out || (in < out + bytes && out < in + bytes))) {
            set_error("gem_foot_lock: sequence " + std::to_string(i) + ": the output overlaps the input (in place is not supported)"); return 1;
        }
    }
    const int64_t need = at * (int64_t)sizeof(double);
    if (need > 0 && (!d_work || work_bytes < need)) {
        set_error("gem_foot_lock: d_work holds " + std::to_string(d_work ? work_bytes : 0) + " bytes, " + std::to_string(need) + " are needed"); return 1;
    }
    FootLockArgs a;
    a.table = d_table; a.n = n_sequences; a.lag = lag; a.min_run = min_run; a.blend = blend; a.snap = snap ? 1 : 0;
    a.tau_v = tau_v; a.tau_h = tau_h; a.stretch = stretch;
    a.ground = d_ground_records; a.work = d_work; a.rec = d_records;
    hipLaunchKernelGGL(foot_lock_kernel, dim3((unsigned)n_sequences), dim3(ERR_ST), 0, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
