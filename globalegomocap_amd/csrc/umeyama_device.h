// The similarity alignment of a whole sequence (Umeyama with the reflection fix) as device code that more than one kernel
// uses: the 3x3 SVD, rigid_transform_3D from moments, the fixed-order workgroup sums and the two passes over the points that
// produce the moments.  Included by errors.hip (the error report's sequence-level part) and through it by skeleton_mesh.h
// (gem_sequence_align, the alignment of the --save meshes).  Reference: utils/rigid_transform_with_scale.py:18-43,
// calculate_errors.py:8-21.
#pragma once
#include "gem_internal.h"

namespace gem {

// ---------------------------------------------------------------------------------------------------
// 3x3 SVD by one-sided Jacobi (Hestenes): A = U diag(S) V^T, columns of U/V orthonormal, S >= 0 unsorted.
// Accurate to eps * cond(A) (no A^T A squaring).  Row-major 3x3 arrays.
// U is orthonormal for every finite A and no element of it is read before it is written.  A column k of U is a[:,k] / S[k] where
// S[k] > 1e-14 * max(S) and S[k] > 0; the others are completed by a fixed rule:
//   rank 3  nothing to complete
//   rank 2  the missing column is the cross product of the other two in cyclic order (det U = +1)
//   rank 1  with u the one column there is, at k: column k+1 = u x e / |u x e|, e the coordinate axis with the smallest |u . e| (the
//           first of equals), column k+2 = u x column k+1, indices mod 3 (det U = +1)
//   rank 0  U = I
// V is a product of plane rotations: orthonormal, det V = +1.  (tests/umeyama_twin.py is the float64 twin, step for step.)
__device__ inline void svd3(const double* A, double* U, double* S, double* V) {
    double a[9];
    for (int i = 0; i < 9; ++i) { a[i] = A[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double alpha = a[p] * a[p] + a[3 + p] * a[3 + p] + a[6 + p] * a[6 + p];
                const double beta = a[q] * a[q] + a[3 + q] * a[3 + q] + a[6 + q] * a[6 + q];
                const double gamma = a[p] * a[q] + a[3 + p] * a[3 + q] + a[6 + p] * a[6 + q];
                if (gamma == 0.0 || fabs(gamma) <= 1e-300) continue;
                const double rel = fabs(gamma) / sqrt(alpha * beta);
                off = rel > off ? rel : off;
                if (!(rel > 1e-17)) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < 3; ++r) {
                    const double ap = a[3 * r + p], aq = a[3 * r + q];
                    a[3 * r + p] = c * ap - s * aq;
                    a[3 * r + q] = s * ap + c * aq;
                    const double vp = V[3 * r + p], vq = V[3 * r + q];
                    V[3 * r + p] = c * vp - s * vq;
                    V[3 * r + q] = s * vp + c * vq;
                }
            }
        if (off < 1e-16) break;
    }
    double smax = 0.0;
    for (int k = 0; k < 3; ++k) {
        S[k] = sqrt(a[k] * a[k] + a[3 + k] * a[3 + k] + a[6 + k] * a[6 + k]);
        smax = S[k] > smax ? S[k] : smax;
    }
    int bad = -1, good = -1, n_good = 0;
    for (int k = 0; k < 3; ++k) {
        if (S[k] > 1e-14 * smax && S[k] > 0.0) {
            for (int r = 0; r < 3; ++r) U[3 * r + k] = a[3 * r + k] / S[k];
            good = k;
            ++n_good;
        } else {
            bad = k;
        }
    }
    if (bad >= 0) S[bad] = 0.0;          // (the last one below the threshold; an earlier one keeps its value, at most 1e-14 * smax)
    if (n_good == 2) {       // rank 2 (coplanar points): complete U with the cross product of the other two
        const int i = (bad + 1) % 3, j = (bad + 2) % 3;
        U[bad] = U[3 + i] * U[6 + j] - U[6 + i] * U[3 + j];
        U[3 + bad] = U[6 + i] * U[j] - U[i] * U[6 + j];
        U[6 + bad] = U[i] * U[3 + j] - U[3 + i] * U[j];
    } else if (n_good == 1) {          // rank 1 (collinear points): u, then u x e normalised (e: the first axis least aligned with u), then their cross product
        const int i = (good + 1) % 3, j = (good + 2) % 3;
        const double u[3] = {U[good], U[3 + good], U[6 + good]};
        int e = 0;
        for (int r = 1; r < 3; ++r)
            if (fabs(u[r]) < fabs(u[e])) e = r;
        const int e1 = (e + 1) % 3, e2 = (e + 2) % 3;
        double v[3];                   // u x e: zero along e, and at least sqrt(2/3) long
        v[e] = 0.0;
        v[e1] = u[e2];
        v[e2] = -u[e1];
        const double n = sqrt(v[e1] * v[e1] + v[e2] * v[e2]);
        for (int r = 0; r < 3; ++r) v[r] /= n;
        U[i] = v[0]; U[3 + i] = v[1]; U[6 + i] = v[2];
        U[j] = u[1] * v[2] - u[2] * v[1];
        U[3 + j] = u[2] * v[0] - u[0] * v[2];
        U[6 + j] = u[0] * v[1] - u[1] * v[0];
    } else if (n_good == 0) {          // rank 0 (the zero matrix): U = I
        for (int r = 0; r < 9; ++r) U[r] = (r % 4 == 0) ? 1.0 : 0.0;
    }
}

__device__ inline double det3(const double* m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

struct Sim3 {
    double cR[9];      // c * R, row-major: aligned = p @ cR + t  (row vector convention of the reference)
    double t[3];
};

// rigid_transform_3D from moments: cov = (P-mp)^T (Q-mq) / n, var = sum_d var(P_d).  PARTS: also the scale and the rotation on
// their own (c_out, R_out row-major; gem_sequence_align); the error report's instantiation is the function it has always been.
template <bool PARTS>
__device__ inline void umeyama_moments_t(const double* mp, const double* mq, const double* cov, double var, Sim3* out, double* c_out,
                                         double* R_out) {
    double U[9], S[3], V[9];
    svd3(cov, U, S, V);
    // numpy: cov = Vn diag(S) Wn, R = Vn @ Wn with (S[-1], Vn[:, -1]) negated when det(Vn) det(Wn) < 0; here
    // Vn = U, Wn = V^T, and "last" = the smallest singular value.
    int kmin = 0;
    for (int k = 1; k < 3; ++k)
        if (S[k] < S[kmin]) kmin = k;
    double d[3] = {1.0, 1.0, 1.0};
    if (det3(U) * det3(V) < 0.0) d[kmin] = -1.0;
    const double c = (d[0] * S[0] + d[1] * S[1] + d[2] * S[2]) / var;
    if constexpr (PARTS) *c_out = c;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double r = 0.0;
            for (int k = 0; k < 3; ++k) r += U[3 * i + k] * d[k] * V[3 * j + k];
            out->cR[3 * i + j] = c * r;
            if constexpr (PARTS) R_out[3 * i + j] = r;
        }
    for (int j = 0; j < 3; ++j) out->t[j] = mq[j] - (mp[0] * out->cR[j] + mp[1] * out->cR[3 + j] + mp[2] * out->cR[6 + j]);
}

__device__ inline void umeyama_moments(const double* mp, const double* mq, const double* cov, double var, Sim3* out) {
    umeyama_moments_t<false>(mp, mq, cov, var, out, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------------
// Sums over a 1024-thread workgroup in a fixed order.
constexpr int ERR_ST = 1024;
constexpr int ERR_NW = ERR_ST / 64;

// K sums at once: wavefront DPP reductions, [K][16] partials in LDS, every thread adds the 16 partials of each value
// in the same order.  Alternating LDS halves: one barrier per call is enough (see lbfgs.hip's BlockRed).
template <int K>
__device__ inline void block_sums(double (&v)[K], double* lds, int& parity) {
    double* r = lds + parity * (16 * ERR_NW);
    parity ^= 1;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double w = wave_sum_dpp(v[k]);
        if ((threadIdx.x & 63) == 0) r[k * ERR_NW + (threadIdx.x >> 6)] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = 0.0;
        for (int i = 0; i < ERR_NW; ++i) t += r[k * ERR_NW + i];
        v[k] = t;
    }
}

// The sequence's moments: means of P and Q (m[0..2], m[3..5]) and, centred, cov = (P-mp)^T (Q-mq) / N in c[0..8] and
// sum_d var(P_d) in c[9], over all N points; every thread of the ERR_ST-thread workgroup ends up with the same values.
// Two barriers (one per group of sums).
__device__ inline void sequence_moments(const double* P, const double* Q, size_t N, int tid, double* red, int& parity, double (&m)[6],
                                        double (&c)[10]) {
    for (int k = 0; k < 6; ++k) m[k] = 0.0;
    for (size_t i = tid; i < N; i += ERR_ST)
        for (int d = 0; d < 3; ++d) { m[d] += P[i * 3 + d]; m[3 + d] += Q[i * 3 + d]; }
    block_sums<6>(m, red, parity);
    for (int k = 0; k < 6; ++k) m[k] /= (double)N;
    for (int k = 0; k < 10; ++k) c[k] = 0.0;
    for (size_t i = tid; i < N; i += ERR_ST) {
        double p[3], q[3];
        for (int d = 0; d < 3; ++d) { p[d] = P[i * 3 + d] - m[d]; q[d] = Q[i * 3 + d] - m[3 + d]; }
        for (int x = 0; x < 3; ++x) {
            c[9] += p[x] * p[x];
            for (int y = 0; y < 3; ++y) c[3 * x + y] += p[x] * q[y];
        }
    }
    block_sums<10>(c, red, parity);
    for (int k = 0; k < 10; ++k) c[k] /= (double)N;
}

}  // namespace gem
