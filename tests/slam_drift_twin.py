"""numpy twin of the drifting-scale estimator, written from that text: the reference for `gem_slam_drift`.
The global estimate is `slam_scale_twin.estimate` as it is; the curve's knots, rounds, banded solve and the metric track follow
here, every sum written out, products added left to right, so that a power-of-two change of the trajectory's unit changes nothing
but exponents.  `dtype` np.longdouble runs the same arithmetic in extended precision (the global estimate stays float64): the
distance between the two runs is what float64 itself costs."""
import numpy as np

import slam_scale_twin as T

ROUNDS = 4
MAX_KNOTS = 2048
NOT_SOLVED = 5


def knot_count(ids, knot):
    """K = max(2, ceil((B - A) / knot) + 1) knots at A + k knot"""
    span = int(ids[-1]) - int(ids[0])
    return max(2, -(-span // int(knot)) + 1)


def place(m2, knot, K, dtype=np.float64):
    """A time tau given as the integer m2 = 2 (tau - A) -> (interval k = min(floor((tau - A) / knot), K - 2), fraction u inside it)"""
    m2 = np.asarray(m2, dtype=np.int64)
    k = np.clip(m2 // (2 * int(knot)), 0, K - 2)
    u = (m2 - 2 * int(knot) * k).astype(dtype) / dtype(2 * int(knot))
    return k, u


def curve_at(s, k, u):
    return (1 - u) * s[k] + u * s[k + 1]


def penalty_bands(K):
    """D^T D of the K - 2 second differences, as integer bands (diagonal, first, second off-diagonal)"""
    d0, d1, d2 = np.zeros(K), np.zeros(K), np.zeros(K)
    for j in range(1, K - 1):
        d0[j - 1] += 1.0; d0[j] += 4.0; d0[j + 1] += 1.0
        d1[j - 1] += -2.0; d1[j] += -2.0
        d2[j - 1] += 1.0
    return d0, d1, d2


def solve_bands(M0, M1, M2, rhs):
    """L D L^T of the symmetric pentadiagonal matrix in a fixed order -> (solution, index of the first pivot that is not positive and
    finite, or -1)"""
    K = len(M0)
    dt = M0.dtype
    d, l1, l2, e1s, y, s = (np.zeros(K, dtype=dt) for _ in range(6))
    for i in range(K):
        e2 = M2[i - 2] if i >= 2 else dt.type(0)
        l2[i] = e2 / d[i - 2] if i >= 2 else dt.type(0)
        if i >= 2:
            e1 = M1[i - 1] - l2[i] * (l1[i - 1] * d[i - 2])
        elif i == 1:
            e1 = M1[0]
        else:
            e1 = dt.type(0)
        l1[i] = e1 / d[i - 1] if i >= 1 else dt.type(0)
        d[i] = M0[i] - l1[i] * e1 - l2[i] * e2
        if not (np.isfinite(d[i]) and d[i] > 0):
            return None, i
    for i in range(K):
        v = rhs[i]
        if i >= 1:
            v = v - l1[i] * y[i - 1]
        if i >= 2:
            v = v - l2[i] * y[i - 2]
        y[i] = v
    for i in range(K - 1, -1, -1):
        v = y[i] / d[i]
        if i + 1 < K:
            v = v - l1[i + 1] * s[i + 1]
        if i + 2 < K:
            v = v - l2[i + 2] * s[i + 2]
        s[i] = v
    return s, -1


def _assess(a, b, sp, tau2):
    r = T.sq(a + (sp[:, None] * b)[:, None, :])
    side = (r[:, 1] < r[:, 0]).astype(np.int64)          # (a tie takes the right foot)
    rs = r[np.arange(len(sp)), side]
    with np.errstate(invalid="ignore"):
        inl = rs < tau2
    return r, side, rs, inl


def _interval_sums(vals, inl, kp, K):
    """[K-1, len(vals)]: per interval the inliers' sums, the pairs added one after the other in their order"""
    out = np.zeros((K - 1, len(vals)), dtype=vals[0].dtype)
    for c, v in enumerate(vals):
        np.add.at(out[:, c], kp[inl], v[inl])
    return out


def metric_track(s, c, ids, knot, dtype=np.float64):
    """Step 5: C_0 = 0, C_i = C_i-1 + s((ids[i-1] + ids[i]) / 2) (c_i - c_i-1), summed left to right
    -> (C [N,3], summed length of the scaled steps, summed length of the steps)"""
    ids = np.asarray(ids, dtype=np.int64)
    s, c = np.asarray(s, dtype=dtype), np.asarray(c, dtype=np.float64).astype(dtype)
    km, um = place(ids[:-1] + ids[1:] - 2 * int(ids[0]), knot, len(s), dtype)
    sm = curve_at(s, km, um)
    dc = c[1:] - c[:-1]
    ln = np.sqrt(T.sq(dc))
    return np.concatenate([np.zeros((1, 3), dtype=dtype), np.cumsum(sm[:, None] * dc, axis=0)]), np.sum(sm * ln), np.sum(ln)


def estimate(x, R, c, ids, lag, knot, stiffness=1.0, tau=0.10, min_pairs=50, feet=T.FEET, dtype=np.float64):
    """-> dict: `global` (slam_scale_twin.estimate's), knot_ids [K], knot_scale [K], interval_count [K-1], interval_bb [K-1], inliers,
    informative, residual_rms, scale_min, scale_max, scale_mean, metric_length, slam_length, lam, metric [N,3], margins.
    Raises slam_scale_twin.Refusal with the global estimate's codes, or NOT_SOLVED naming the knots without inliers."""
    ids = np.asarray(ids, dtype=np.int64)
    knot = int(knot)
    g = T.estimate(x, R, c, ids, lag, tau, min_pairs, None, feet)
    K = knot_count(ids, knot)
    if K > MAX_KNOTS:
        raise ValueError("%d knots, at most %d are possible" % (K, MAX_KNOTS))
    A = int(ids[0])
    a, b, t = T.pairs(T.foot_points(x, R, feet), c, ids, lag)
    a, b = a.astype(dtype), b.astype(dtype)
    P = len(t)
    tau2 = dtype(tau) * dtype(tau)
    kp, up = place(2 * (ids[t] - A) + lag, knot, K, dtype)
    w0, w1 = 1 - up, up
    bb = T.sq(b)
    d0, d1, d2 = (v.astype(dtype) for v in penalty_bands(K))
    s = np.full(K, g["scale"], dtype=dtype)
    seen, lam = [], dtype(0)
    for _ in range(ROUNDS):
        sp = curve_at(s, kp, up)
        r, side, rs, inl = _assess(a, b, sp, tau2)
        seen.append((r, rs))
        ab = T.dot(a[np.arange(P), side], b)
        S = _interval_sums([w0 * w0 * bb, w0 * w1 * bb, w1 * w1 * bb, w0 * ab, w1 * ab, bb], inl, kp, K)
        counts = np.bincount(kp[inl], minlength=K - 1)
        tot = dtype(0)
        for j in range(K - 1):
            tot = tot + S[j, 5]
        lam = dtype(stiffness) * tot / dtype(K - 1)
        M0, M1, M2, rhs = (np.zeros(K, dtype=dtype) for _ in range(4))
        for k in range(K):
            m0 = g0 = dtype(0)
            if k > 0:
                m0, g0 = m0 + S[k - 1, 2], g0 + S[k - 1, 4]
            if k < K - 1:
                m0, g0 = m0 + S[k, 0], g0 + S[k, 3]
            M0[k], rhs[k] = m0 + lam * d0[k], -g0
            if k < K - 1:
                M1[k] = S[k, 1] + lam * d1[k]
            if k < K - 2:
                M2[k] = lam * d2[k]
        informed = int((S[:, 5] > 0).sum())
        new, bad = solve_bands(M0, M1, M2, rhs) if (K == 2 or informed >= 2) else (None, -1)
        if new is None:
            empty = [j for j in range(K - 1) if counts[j] == 0]
            raise T.Refusal(NOT_SOLVED, "the recording does not fix the scale curve: no inlier pairs between knots %s (%d knots, %d intervals with "
                            "a moving camera)" % (", ".join("%d-%d" % (j, j + 1) for j in empty) or "none", K, informed),
                            {"interval_count": counts, "bad_pivot": bad})
        s = new
    sp = curve_at(s, kp, up)
    r, side, rs, inl = _assess(a, b, sp, tau2)
    seen.append((r, rs))
    nb = np.sqrt(bb)
    S = _interval_sums([bb, rs], inl, kp, K)
    counts = np.bincount(kp[inl], minlength=K - 1)
    n_inl = int(inl.sum())
    informative = int((inl & (sp * nb > dtype(tau))).sum())
    rss = dtype(0)
    for j in range(K - 1):
        rss = rss + S[j, 1]
    metric, metric_length, slam_length = metric_track(s, c, ids, knot, dtype)
    m = dict(g["margins"])
    tau2f = float(tau2)
    with np.errstate(invalid="ignore"):
        m["drift_tau"] = min(float(np.min(np.abs(q - tau2))) for _, q in seen) / tau2f
        m["drift_sides"] = min(float(np.min(np.where(q < tau2, np.abs(p[:, 0] - p[:, 1]), np.inf))) for p, q in seen) / tau2f
        m["drift_informative"] = float(np.min(np.abs(sp * nb - dtype(tau)))) / float(tau)
    return {"global": g, "knot_ids": A + knot * np.arange(K, dtype=np.int64), "knot_scale": s, "interval_count": counts, "interval_bb": S[:, 0],
            "inliers": n_inl, "informative": informative, "residual_rms": np.sqrt(rss / dtype(n_inl)), "scale_min": s.min(), "scale_max": s.max(),
            "scale_mean": metric_length / slam_length, "metric_length": metric_length, "slam_length": slam_length, "lam": lam, "metric": metric,
            "margins": m, "pair_rows": t, "pair_interval": kp}


def margins_ok(m, bound=1e-9):
    return all(v > bound for v in m.values())
