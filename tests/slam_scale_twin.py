"""numpy float64 twin of the SLAM-scale estimator, written from that text: the reference for
`gem_slam_scale`.  Every sum is written out (no BLAS, no einsum), products are added left to right, so that a power-of-two change
of the trajectory's unit changes nothing but exponents."""
import numpy as np

N_CAND = 513                      # s_ref * 2^(g / 32), g = -256 .. 256
ROUNDS = 4
FEET = (9, 10, 13, 14)            # right ankle, right foot, left ankle, left foot (skeleton.JOINT_NAMES)
NO_PAIRS, TOO_FEW, BAD_SCALE = 2, 3, 4


class Refusal(ValueError):
    def __init__(self, code, message, report):
        ValueError.__init__(self, message)
        self.code, self.report = code, report


def sq(v):
    return v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]


def dot(u, v):
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]


def foot_points(x, R, feet=FEET):
    """step 1: q[t,side] = R_t (x[t,ankle] + x[t,foot]) / 2 -> [N,2,3]"""
    x, R = np.asarray(x, dtype=np.float64), np.asarray(R, dtype=np.float64)
    q = np.empty((len(x), 2, 3))
    for side in range(2):
        m = 0.5 * (x[:, feet[2 * side]] + x[:, feet[2 * side + 1]])
        for r in range(3):
            q[:, side, r] = R[:, r, 0] * m[:, 0] + R[:, r, 1] * m[:, 1] + R[:, r, 2] * m[:, 2]
    return q


def pairs(q, c, ids, lag):
    """step 2 -> (a [P,2,3], b [P,3], t [P]: the first frame's row of every pair)"""
    c, ids = np.asarray(c, dtype=np.float64), np.asarray(ids, dtype=np.int64)
    n = len(ids)
    if n <= lag:
        return np.empty((0, 2, 3)), np.empty((0, 3)), np.empty(0, dtype=np.int64)
    t = np.nonzero(ids[lag:] - ids[:n - lag] == lag)[0]
    return q[t + lag] - q[t], c[t + lag] - c[t], t


def residuals(a, b, s):
    """|a[p,side] + s b[p]|^2 -> [P,2]"""
    return sq(a + (s * b)[:, None, :])


def estimate(x, R, c, ids, lag, tau=0.10, min_pairs=50, chunk_starts=None, feet=FEET):
    """-> dict: scale, s0, s_ref, g0, costs [513], pairs, inliers, informative, residual_rms, path_length, stance_share (right, left),
    per_chunk [n_chunks,3] (numerator, denominator, scale), margins (see `margins`).  Raises Refusal (a ValueError) with `code`.
    chunk_starts [n_chunks + 1]: rows at which the chunks begin (default: one chunk); a pair belongs to its first frame's chunk."""
    n = len(np.asarray(ids))
    chunk_starts = np.array([0, n], dtype=np.int64) if chunk_starts is None else np.asarray(chunk_starts, dtype=np.int64)
    tau2 = tau * tau
    a, b, t = pairs(foot_points(x, R, feet), c, ids, lag)
    P = len(t)
    rep = {"pairs": P, "inliers": 0, "informative": 0}
    saa = float(np.sum(sq(a))) if P else 0.0
    sbb = float(np.sum(sq(b))) if P else 0.0
    if P == 0 or sbb == 0.0:
        raise Refusal(NO_PAIRS, "no pairs of frames %d apart with a camera translation between them (%d pairs)" % (lag, P), rep)
    s_ref = np.sqrt(saa / (2.0 * sbb))
    g = np.arange(N_CAND) - (N_CAND // 2)
    cand = s_ref * np.exp2(g / 32.0)
    costs = np.array([np.sum(np.minimum(np.min(residuals(a, b, s), axis=1), tau2)) for s in cand])
    g0 = int(np.argmin(costs))                          # (the first of equal minima: the smallest g)
    s = s0 = float(cand[g0])
    seen = []                                           # every residual that was compared with tau^2, and the two sides' difference
    for _ in range(ROUNDS):
        r = residuals(a, b, s)
        side = (r[:, 1] < r[:, 0]).astype(np.int64)     # (a tie takes the right foot, side 0)
        rs = r[np.arange(P), side]
        inl = rs < tau2
        seen.append((r, rs))
        num = np.sum(dot(a[np.arange(P), side], b)[inl])
        den = np.sum(sq(b)[inl])
        with np.errstate(invalid="ignore", divide="ignore"):
            s = float(-np.float64(num) / np.float64(den))
    r = residuals(a, b, s)
    side = (r[:, 1] < r[:, 0]).astype(np.int64)
    rs = r[np.arange(P), side]
    with np.errstate(invalid="ignore"):
        inl = rs < tau2
    seen.append((r, rs))
    nb = np.sqrt(sq(b))
    sel = a[np.arange(P), side]
    n_inl = int(inl.sum())
    with np.errstate(invalid="ignore"):
        informative = int((inl & (s * nb > tau)).sum())
    per_chunk = np.zeros((len(chunk_starts) - 1, 3))
    ab, bb = dot(sel, b), sq(b)
    for k in range(len(chunk_starts) - 1):
        m = inl & (t >= chunk_starts[k]) & (t < chunk_starts[k + 1])
        per_chunk[k, 0], per_chunk[k, 1] = np.sum(ab[m]), np.sum(bb[m])
    with np.errstate(invalid="ignore", divide="ignore"):
        per_chunk[:, 2] = -per_chunk[:, 0] / per_chunk[:, 1]
        rms = float(np.sqrt(np.float64(np.sum(rs[inl])) / np.float64(n_inl)))
        shares = (float(np.float64((inl & (side == 0)).sum()) / np.float64(n_inl)), float(np.float64((inl & (side == 1)).sum()) / np.float64(n_inl)))
    rep = {"scale": s, "s0": s0, "s_ref": float(s_ref), "g0": g0, "costs": costs, "pairs": P, "inliers": n_inl, "informative": informative,
           "residual_rms": rms, "path_length": float(s * np.sum(nb) / lag), "stance_share": shares, "per_chunk": per_chunk,
           "margins": margins(costs, seen, s * nb, tau)}
    if not (np.isfinite(s) and s > 0):
        raise Refusal(BAD_SCALE, "the fitted scale %r is not a positive number (%d pairs, %d inliers)" % (s, P, n_inl), rep)
    if informative < min_pairs:
        raise Refusal(TOO_FEW, "the wearer did not walk enough to fix the scale: %d informative pairs of %d (%d inliers), %d are needed"
                      % (informative, P, n_inl, min_pairs), rep)
    return rep


def margins(costs, seen, s_nb, tau):
    """How far the discrete decisions are from flipping, relative: (gap between the two lowest costs, smallest |r - tau^2| / tau^2 over
    every residual that was compared with tau^2, smallest |r_right - r_left| / tau^2 where the smaller one is an inlier, smallest
    |s|b| - tau| / tau).  A device that agrees with the twin to 1e-12 takes the same decisions when all are above 1e-9."""
    tau2 = tau * tau
    two = np.sort(costs)[:2]
    with np.errstate(invalid="ignore"):
        near = min(float(np.min(np.abs(rs - tau2))) for _, rs in seen) / tau2
        sides = min(float(np.min(np.where(rs < tau2, np.abs(r[:, 0] - r[:, 1]), np.inf))) for r, rs in seen) / tau2
        info = float(np.min(np.abs(s_nb - tau))) / tau
    return {"cost_gap": float((two[1] - two[0]) / two[0]) if two[0] > 0 else np.inf, "tau": near, "sides": sides, "informative": info}
