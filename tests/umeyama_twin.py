"""numpy twin of the similarity alignment in globalegomocap_amd/csrc/umeyama_device.h (`svd3`, `umeyama_moments_t`; DESIGN.md
section 6), float64, written step by step as the device writes it: the same sweep order, the same three thresholds, the same
completion of U by rank, `kmin` the first smallest singular value, the reflection on it.  Only the order of the sums over the
points differs (the device adds them in a fixed tree).  And the table of point sets and 15-joint sequences on which
tests/test_alignment_cpu.py holds the twin to LAPACK (`errors.umeyama`) and tests/test_alignment_gpu.py the device to both.  No GPU."""
import math

import numpy as np

SWEEPS = 30
TINY_GAMMA, REL_SKIP, REL_DONE = 1e-300, 1e-17, 1e-16          # the three thresholds of the sweeps
RANK_TOL = 1e-14                                               # a column of U exists where S[k] > RANK_TOL * max(S)
THICKNESS = (1.0, 1e-2, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 0.0)


# ------------------------------------------------------------------------------------------------ the device's steps
def svd3(A, info=None):
    """A [3,3] -> U, S, V with A = U diag(S) V^T; S unsorted.  One-sided Jacobi on the columns of a copy of A.  info: a dict that
    receives "rank", the number of columns of U that came from A."""
    # alpha * beta may underflow to zero beside a gamma above TINY_GAMMA (a column of norm 1e-160 that an exactly collinear set
    # leaves behind): rel = inf and zeta * zeta = inf then make t = 0, the identity rotation, here as on the device
    with np.errstate(divide="ignore", over="ignore"):
        return _svd3(A, info)


def _svd3(A, info):
    a = np.array(A, dtype=np.float64)
    V = np.eye(3)
    for _ in range(SWEEPS):
        off = 0.0
        for p in range(2):
            for q in range(p + 1, 3):
                alpha = a[0, p] * a[0, p] + a[1, p] * a[1, p] + a[2, p] * a[2, p]
                beta = a[0, q] * a[0, q] + a[1, q] * a[1, q] + a[2, q] * a[2, q]
                gamma = a[0, p] * a[0, q] + a[1, p] * a[1, q] + a[2, p] * a[2, q]
                if gamma == 0.0 or abs(gamma) <= TINY_GAMMA:
                    continue
                rel = abs(gamma) / math.sqrt(alpha * beta)
                off = rel if rel > off else off
                if not rel > REL_SKIP:
                    continue
                zeta = (beta - alpha) / (2.0 * gamma)
                t = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                c = 1.0 / math.sqrt(1.0 + t * t)
                s = c * t
                for M in (a, V):
                    mp, mq = M[:, p].copy(), M[:, q].copy()
                    M[:, p] = c * mp - s * mq
                    M[:, q] = s * mp + c * mq
        if off < REL_DONE:
            break
    S = np.array([math.sqrt(a[0, k] * a[0, k] + a[1, k] * a[1, k] + a[2, k] * a[2, k]) for k in range(3)])
    smax = max(0.0, S[0], S[1], S[2])
    U = np.full((3, 3), np.nan)          # (a column that nobody writes would show)
    bad, good, n_good = -1, -1, 0
    for k in range(3):
        if S[k] > RANK_TOL * smax and S[k] > 0.0:
            U[:, k] = a[:, k] / S[k]
            good = k
            n_good += 1
        else:
            bad = k
    if bad >= 0:
        S[bad] = 0.0
    if n_good == 2:
        U[:, bad] = np.cross(U[:, (bad + 1) % 3], U[:, (bad + 2) % 3])
    elif n_good == 1:
        complete_rank1(U, good)
    elif n_good == 0:
        U = np.eye(3)
    if info is not None:
        info["rank"] = n_good
    return U, S, V


def complete_rank1(U, good):
    """With u the one column there is: column good + 1 = u x e normalised, e the coordinate axis with the smallest |u . e| (the
    first of equals), column good + 2 = u x that one: a right-handed basis."""
    u = U[:, good].copy()
    e = 0
    for r in (1, 2):
        if abs(u[r]) < abs(u[e]):
            e = r
    e1, e2 = (e + 1) % 3, (e + 2) % 3
    v = np.zeros(3)          # u x e
    v[e1], v[e2] = u[e2], -u[e1]
    v = v / math.sqrt(v[e1] * v[e1] + v[e2] * v[e2])
    U[:, (good + 1) % 3] = v
    U[:, (good + 2) % 3] = np.cross(u, v)


def first_smallest(S):
    k = 0
    for i in (1, 2):
        if S[i] < S[k]:
            k = i
    return k


def reflect(U, V):
    return np.linalg.det(U) * np.linalg.det(V) < 0.0


def umeyama_moments(mp, mq, cov, var):
    """The means, cov = (P - mp)^T (Q - mq) / n and var = sum_d var(P_d) -> c, R, t with Q ~ c * P @ R + t."""
    U, S, V = svd3(cov)
    d = np.ones(3)
    if reflect(U, V):
        d[first_smallest(S)] = -1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.float64(d[0] * S[0] + d[1] * S[1] + d[2] * S[2]) / np.float64(var)
    R = (U * d) @ V.T
    return float(c), R, mq - mp @ (c * R)


def umeyama(P, Q):
    P, Q = np.asarray(P, dtype=np.float64).reshape(-1, 3), np.asarray(Q, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    mp, mq = P.sum(axis=0) / n, Q.sum(axis=0) / n
    p, q = P - mp, Q - mq
    return umeyama_moments(mp, mq, p.T @ q / n, float((p * p).sum() / n))


def crt13(c, R, t):
    return np.concatenate([[c], np.asarray(R).reshape(-1), t])


def apply(crt, P):
    """c * (p . R) + t, as every reader of the 13 numbers applies them (the device applies p . (cR) + t)."""
    crt = np.asarray(crt, dtype=np.float64)
    return np.asarray(P, dtype=np.float64) @ (crt[0] * crt[1:10].reshape(3, 3)) + crt[10:13]


# ------------------------------------------------------------------------------------------------ the point sets
def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


RA, RB = rotation((1.0, 2.0, -1.0), 0.7), rotation((0.3, -1.0, 0.5), 1.1)
LINE = np.array([1.0, 0.5, -0.25])          # dyadic: multiples of it by dyadic numbers are exactly collinear in float64
QUARTER = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])          # an exact rotation
OCTAHEDRON = np.concatenate([np.eye(3), -np.eye(3)])
MIRROR = np.array([1.0, 1.0, -1.0])


def dyadic(x, bits=20):
    return np.round(np.asarray(x, dtype=np.float64) * 2.0 ** bits) / 2.0 ** bits


def _cloud(rng, n):
    return rng.normal(size=(n, 3)) * np.array([1.0, 0.7, 0.5]) * 0.3


def _image(P, rng, noise=0.01):
    return 0.8 * (P @ RB) + np.array([0.4, 0.1, -0.7]) + rng.normal(0.0, noise, P.shape)


def _build_cases():
    out = {}
    # thickness: one set of draws for every member; the cloud and the noise are squashed along z before they are turned
    rng = np.random.default_rng(101)
    X, E = _cloud(rng, 15), rng.normal(0.0, 0.01, (15, 3))
    for th in THICKNESS:
        sq = np.array([1.0, 1.0, th])
        P = (X * sq) @ RA + np.array([0.3, 1.2, -0.4])
        for tag, m in (("", np.ones(3)), (" mirrored", MIRROR)):
            Q = 0.8 * (((X + E) * sq * m) @ RB) + np.array([0.4, 0.1, -0.7])
            out["thickness %g%s" % (th, tag)] = (P, Q, "full")
    # equal singular values: no noise, the values are equal to rounding
    for name, axes in (("three equal", (1.0, 1.0, 1.0)), ("two equal", (1.0, 1.0, 0.3))):
        P = (OCTAHEDRON * np.array(axes)) @ RA + np.array([0.3, 1.2, -0.4])
        out[name] = (P, 1.7 * (P @ RB) + np.array([0.4, 0.1, -0.7]), "full")
    P = OCTAHEDRON @ RA
    out["isotropic mirrored"] = (P, 1.7 * ((OCTAHEDRON * MIRROR) @ RA @ RB) + np.array([0.4, 0.1, -0.7]), "residual")
    # offsets: every number dyadic, so that the same centred cloud stands at every distance
    rng = np.random.default_rng(102)
    X, E = dyadic(_cloud(rng, 15)), dyadic(rng.normal(0.0, 0.01, (15, 3)))
    for off in (0.0, 100.0, 1000.0, 10000.0):
        P = X + np.array([off, -off, 0.5 * off])
        Q = 0.5 * ((X + E) @ QUARTER) + np.array([0.25 - off, 2.0 * off, off])
        out["offset %g m" % off] = (P, Q, "full")
    rng = np.random.default_rng(103)
    X = _cloud(rng, 15) @ RA + np.array([0.3, 1.2, -0.4])
    Q = _image(X, rng)
    for s in (1e3, 1e-3, 1e6, 1e-6):
        out["scale %g" % s] = (s * X, Q, "full")
    out["identity"] = (X, X.copy(), "full")
    out["180 degrees"] = (X, 1.25 * (X * np.array([-1.0, -1.0, 1.0])) + np.array([0.4, 0.1, -0.7]), "full")
    # rank 1: exactly collinear in float64 (dyadic multiples of LINE from a dyadic point)
    rng = np.random.default_rng(104)
    a = dyadic(rng.normal(0.0, 0.3, 15))
    line = a[:, None] * LINE + np.array([0.5, -1.25, 2.0])
    G = _cloud(rng, 15) @ RA + np.array([0.3, 1.2, -0.4])
    out["rank 1, source collinear"] = (line, _image(G, rng), "full")
    out["rank 1, target collinear"] = (G, line, "residual")
    rng = np.random.default_rng(105)
    for n in (15, 68 * 15, 69 * 15, 3):
        P = _cloud(rng, n) @ RA + np.array([0.3, 1.2, -0.4])
        out["N = %d" % n] = (P, _image(P, rng), "full")
    for P, Q, _ in out.values():
        P.setflags(write=False)
        Q.setflags(write=False)
    return out


_CASES = None


def cases():
    """name -> (P [N,3], Q [N,3], kind): kind "full" compares (c, R, t) and the aligned points, "residual" c and sum |aligned - Q|^2
    (the rotation is not unique there).  Built once from fixed seeds; the arrays are read-only."""
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
    return _CASES


def family(name):
    for f in ("thickness", "offset", "scale", "rank 1", "N ="):
        if name.startswith(f):
            return f + (" mirrored" if name.endswith("mirrored") else "")
    return name if name in ("identity", "180 degrees", "isotropic mirrored") else "equal singular values"


RESIDUAL = ("isotropic mirrored", "rank 1, target collinear")
# the one "full" case whose R and t are not unique: every point of P lies on one line, so only the image of that line's direction
# is determined (u . R), and with it c and the aligned points; the completion of U turns the rest of space freely
LINE_SOURCE = "rank 1, source collinear"


def covariance_singular_values(P, Q):
    """numpy's view of a case: singular values (descending) of the covariance and det(V) det(W)."""
    p, q = P - P.mean(axis=0), Q - Q.mean(axis=0)
    V, S, W = np.linalg.svd(p.T @ q / len(P))
    return S, float(np.linalg.det(V) * np.linalg.det(W))


# ------------------------------------------------------------------------------------------------ 15-joint sequences for the report
MIN_BONE = 1e-4          # metres: a hundred steps of the dyadic grid the line frames are rounded to


def _walk(F, seed):
    """gt as tests/test_hip_post.py builds it: the walking mean skeleton with per-frame articulation and drift."""
    from globalegomocap_amd.skeleton import MEAN3D_MM
    rng = np.random.default_rng(seed)
    base = MEAN3D_MM.T / 1000.0
    t = np.arange(F)[:, None, None]
    return base[None] + 0.05 * np.sin(0.1 * t + rng.uniform(0, 6, (1, 15, 3))) + np.array([0.01, 0.0, 0.002]) * t, rng


def frame_squashes(F, descending=True):
    """Three frames per thickness in turn (descending from 1, or ascending from 0): the first squashed along one axis ("z"), the
    other two along two ("yz"), which at thickness 0 puts every joint on a line."""
    order = THICKNESS if descending else THICKNESS[::-1]
    return [("z" if f % 3 == 0 else "yz", order[(f // 3) % len(order)]) for f in range(F)]


def is_line(how):
    return how == ("yz", 0.0)


def squash_frame(x, how):
    """One frame [15,3] about a dyadic point near its centroid.  A line frame has every joint on the line through that point along
    LINE, at its dyadic coordinate along it: exactly collinear in float64."""
    axes, th = how
    m = dyadic(x.mean(axis=0))
    if is_line(how):
        return m + dyadic((x - m) @ LINE / (LINE @ LINE))[:, None] * LINE
    return m + (x - m) * np.array([1.0, th if axes == "yz" else 1.0, th])


def sequences(F, seed, descending=True):
    """(est, mid, opt, gt) [F,15,3] and the squash of every frame: gt generic; est / mid / opt rotated, scaled, noisy copies of it
    whose frame f is squashed by frame_squashes(F)[f] and then turned about its centre by a rotation of its own (line frames are
    not turned: they stay exact).  Every bone of every line frame keeps a length above MIN_BONE, every other one is not zero."""
    from globalegomocap_amd.skeleton import KINEMATIC_PARENTS
    gt, rng = _walk(F, seed)
    squash = frame_squashes(F, descending)
    out = []
    for k, s in enumerate((0.03, 0.02, 0.01)):
        a = 0.2 * (k + 1)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
        x = (1.0 + 0.05 * k) * gt @ Rz + rng.normal(0, s, gt.shape) + rng.normal(0, 0.1, (1, 1, 3))
        for f in range(F):
            x[f] = squash_frame(x[f], squash[f])
            if not is_line(squash[f]):
                m = x[f].mean(axis=0)
                x[f] = (x[f] - m) @ rotation((1.0, -0.5, 0.25 + 0.1 * f), 0.3 + 0.37 * f) + m
        bones = np.linalg.norm(x - x[:, list(KINEMATIC_PARENTS)], axis=-1)[:, 1:]
        assert bones.min() > 0.0 and bones[[is_line(h) for h in squash]].min() > MIN_BONE, bones.min(axis=1)
        out.append(x)
    out.append(gt)
    for x in out:
        x.setflags(write=False)
    return tuple(out), tuple(squash)


def line_sequences(F, seed):
    """A sequence whose est / mid / opt lie on ONE line, all frames: the per-frame and the sequence alignments are both rank 1."""
    from globalegomocap_amd.skeleton import KINEMATIC_PARENTS
    gt, rng = _walk(F, seed)
    out = []
    for k in range(3):
        x = (1.0 + 0.05 * k) * gt + rng.normal(0, 0.01 * (3 - k), gt.shape)
        m = dyadic(np.array([0.5, -1.25, 2.0]) * (k + 1))
        x = m + dyadic((x - m) @ LINE / (LINE @ LINE))[..., None] * LINE
        bones = np.linalg.norm(x - x[:, list(KINEMATIC_PARENTS)], axis=-1)[:, 1:]
        assert bones.min() > MIN_BONE, bones.min()
        out.append(x)
    out.append(gt)
    for x in out:
        x.setflags(write=False)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ comparing two (c, R, t)
# The project's float64 allowances (no new ones): (c, R, t) to 1e-12 relative as in test_sequence_align_against_umeyama, read
# norm-wise -- an entry of R against |R| = 1, an entry of t against the larger of the two terms it is the difference of, |mq| and
# c |mp| (an exact zero, as in the identity fit, has no relative error); aligned points to test_meshes_gpu.py's 1e-12 m, times the
# magnitude of Q where that is above 1; properness and the squared residual at the same float64 level.
RTOL = 1e-12


def reference(name):
    """LAPACK's answer (errors.umeyama) as 13 numbers: computed once per case."""
    from globalegomocap_amd.errors import umeyama as lapack
    if name not in _REFERENCE:
        P, Q, _ = cases()[name]
        _REFERENCE[name] = crt13(*lapack(P, Q))
        _REFERENCE[name].setflags(write=False)
    return _REFERENCE[name]


_REFERENCE = {}


def deviations(name, got, want):
    """The figures of one case: got / want 13 numbers each -> dict of deviations, every one to be at most RTOL."""
    P, Q, kind = cases()[name]
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == (13,) and np.isfinite(got).all(), (name, got)
    R, Rw = got[1:10].reshape(3, 3), want[1:10].reshape(3, 3)
    out = {"c": abs(got[0] / want[0] - 1.0), "orthonormal": float(np.abs(R @ R.T - np.eye(3)).max()),
           "det": abs(float(np.linalg.det(R)) - 1.0)}
    A, Aw = apply(got, P), apply(want, P)
    if kind == "residual":
        out["residual"] = abs(((A - Q) ** 2).sum() / ((Aw - Q) ** 2).sum() - 1.0)
        return out
    out["aligned"] = float(np.abs(A - Aw).max()) / max(1.0, float(np.abs(Q).max()))
    if name == LINE_SOURCE:
        u = LINE / math.sqrt(LINE @ LINE)
        out["R on the line"] = float(np.abs(u @ R - u @ Rw).max())
    else:
        out["R"] = float(np.abs(R - Rw).max())
        scale = max(float(np.abs(Q.mean(axis=0)).max()), abs(want[0]) * float(np.abs(P.mean(axis=0)).max()))
        out["t"] = float(np.abs(got[10:] - want[10:]).max()) / scale
    return out


def check(name, got, want, what):
    d = deviations(name, got, want)
    bad = {k: v for k, v in d.items() if not v <= RTOL}
    assert not bad, "%s, %s: beyond %g: %s" % (what, name, RTOL, bad)
    return d


class Worst:
    """The largest deviation per family and figure, for the report a test module prints."""

    def __init__(self):
        self.rows = {}

    def see(self, name, d):
        row = self.rows.setdefault(family(name), {})
        for k, v in d.items():
            row[k] = max(row.get(k, 0.0), v)

    def lines(self, what):
        return ["%s, %-26s %s" % (what, f + ":", "  ".join("%s %.2g" % kv for kv in sorted(row.items()))) for f, row in self.rows.items()]
