"""numpy twin of gem_ground_plane and gem_similarity_compose (globalegomocap_amd/csrc/ground.h): the ground
plane of a pose sequence from its foot contacts, the foot figures and the upright transform, float64, written step by step as the
device writes it.  The twin is the specification; eigenvectors come from numpy.linalg.eigh.  No GPU."""
import numpy as np

NECK, RIGHT_HIP, LEFT_HIP = 0, 7, 11
FEET = ((9, 10), (13, 14))          # (ankle, foot) right, left
SOURCES = ("plane", "body_normal", "body")
STATUS_OK, NO_BODY = 0, 2
ROUNDS = 4
DEFAULTS = dict(tau_v=0.10, tau_h=0.05, min_spread=0.05, min_points=8, foot_height=0.0)


def default_lag(fps):
    return max(1, int(round(0.2 * fps)))


def apply(crt, p):
    """c * (p . R) + t for row vectors: how every writer applies a 13-double (c, R, t)."""
    crt = np.asarray(crt, dtype=np.float64)
    return crt[0] * (np.asarray(p, dtype=np.float64) @ crt[1:10].reshape(3, 3)) + crt[10:13]


def compose(a, b):
    """a, then b: c = c_a c_b, R = R_a R_b, t = c_b (t_a . R_b) + t_b."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    Ra, Rb = a[1:10].reshape(3, 3), b[1:10].reshape(3, 3)
    return np.concatenate([[a[0] * b[0]], (Ra @ Rb).reshape(-1), b[0] * (a[10:13] @ Rb) + b[10:13]])


def _unit(v):
    return v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def _fit(p, u0):
    """centroid, eigenvalues (ascending) and the normal of the points p [N,3]."""
    m = p.sum(axis=0) / len(p)
    c = p - m
    w, V = np.linalg.eigh(c.T @ c / len(p))
    n = V[:, 0]
    if n @ u0 < 0:
        n = -n
    return m, w, n, float(n @ m)


class _Margin:
    """The smallest distance of any compared quantity from its threshold."""

    def __init__(self):
        self.value = np.inf

    def see(self, values, threshold):
        v = np.abs(np.asarray(values, dtype=np.float64) - threshold)
        if v.size:
            self.value = min(self.value, float(v.min()))


def estimate(x, lag=5, tau_v=0.10, tau_h=0.05, min_spread=0.05, min_points=8, foot_height=0.0, crt_in=None, check=True):
    """x [F,15,3] -> dict: status, source (index into SOURCES), n, d, u0, tilt_cos, points, inliers, rms, spread, extent,
    contact_frames [2], skate (metres per frame), skate_pairs, penetration, lift_max, crt [13], margin, and `contact` [F,2].
    crt_in [13]: applied to the joints first.  check: ValueError for a sequence without a body direction (status NO_BODY)."""
    x = np.asarray(x, dtype=np.float64)
    if crt_in is not None:
        x = apply(crt_in, x)
    F, k = len(x), int(lag)
    margin = _Margin()
    q = np.stack([0.5 * (x[:, a] + x[:, b]) for a, b in FEET], axis=1)          # [F,2,3]
    body = np.zeros(3)
    for f in range(F):
        body = body + (x[f, NECK] - 0.5 * (q[f, 0] + q[f, 1]))
    norm = np.sqrt(body @ body)
    hips = x[0, RIGHT_HIP] + x[0, LEFT_HIP]
    if not (np.isfinite(norm) and norm >= 1e-6 * F and np.isfinite(hips).all()):
        if check:
            raise ValueError("the sequence has no body direction (status NO_BODY): %d frames, |sum of neck - feet| = %r" % (F, norm))
        return {"status": NO_BODY}
    u0 = body / norm
    # candidates: the earlier frame of a still pair
    cand = np.zeros((F, 2), dtype=bool)
    if F > k:
        dq = np.sqrt(((q[k:] - q[:-k]) ** 2).sum(-1))
        margin.see(dq, tau_v)
        cand[:F - k] = dq < tau_v
    P = q[cand]                                                                  # (frame, side) order
    n_pts = len(P)
    source, spread, extent, inliers, rms = 2, 0.0, 0.0, 0, 0.0
    if n_pts >= min_points:
        m, w, n, d = _fit(P, u0)
        ok = True
        for _ in range(ROUNDS):
            r = P @ n - d
            margin.see(r, tau_h)
            margin.see(r, -tau_h)
            inl = np.abs(r) < tau_h
            if inl.sum() < min_points:
                ok = False
                break
            m, w, n, d = _fit(P[inl], u0)
        spread, extent = float(np.sqrt(max(w[1], 0.0))), float(np.sqrt(max(w[2], 0.0)))
        margin.see(spread, min_spread)
        if ok and spread >= min_spread:
            source = 0
        else:          # the candidates do not span a plane: the body's direction, the height from the candidates
            source, n = 1, u0
            h = P @ u0
            d = float(np.sort(h)[(n_pts - 1) // 2])                              # the lower median
            for _ in range(ROUNDS):
                margin.see(h - d, tau_h)
                margin.see(h - d, -tau_h)
                inl = np.abs(h - d) < tau_h
                if inl.any():
                    d = float(h[inl].sum() / inl.sum())
        r = P @ n - d
        margin.see(r, tau_h)
        margin.see(r, -tau_h)
        inl = np.abs(r) < tau_h
        inliers = int(inl.sum())
        rms = float(np.sqrt((r[inl] ** 2).sum() / max(inliers, 1)))
    else:
        n, d = u0, float((q.reshape(-1, 3) @ u0).min())
    # the foot figures
    h = q @ n - d                                                                # [F,2]
    margin.see(h[cand], tau_h)
    margin.see(h[cand], -tau_h)
    contact = cand & (np.abs(h) < tau_h)
    total, pairs = 0.0, 0
    for side in range(2):
        for f in range(F - 1):
            if contact[f, side] and contact[f + 1, side]:
                v = q[f + 1, side] - q[f, side]
                v = v - (v @ n) * n
                total += float(np.sqrt(v @ v))
                pairs += 1
    # the upright transform
    l = x[0, LEFT_HIP] - x[0, RIGHT_HIP]
    X = l - (l @ n) * n
    if np.sqrt(X @ X) < 1e-6:
        e = np.eye(3)[int(np.argmin(np.abs(n)))]
        X = e - (e @ n) * n
    X = _unit(X)
    Z = np.cross(X, n)
    o = 0.5 * (x[0, RIGHT_HIP] + x[0, LEFT_HIP])
    o = o - ((o @ n) - (d - foot_height)) * n
    R = np.stack([X, n, Z], axis=1)
    assert abs(np.linalg.det(R) - 1.0) < 1e-12, "the upright transform must be right-handed"
    crt = np.concatenate([[1.0], R.reshape(-1), -(o @ R)])
    return {"status": STATUS_OK, "source": source, "n": n, "d": float(d), "u0": u0, "tilt_cos": float(n @ u0), "points": n_pts,
            "inliers": inliers, "rms": rms, "spread": spread, "extent": extent, "contact_frames": contact.sum(axis=0).astype(np.int64),
            "skate": total / pairs if pairs else 0.0, "skate_pairs": pairs, "penetration": max(0.0, -float(h.min())),
            "lift_max": float(h.max()), "crt": crt, "margin": margin.value, "contact": contact, "frames": F, "lag": k}


def upright(x, crt):
    return apply(crt, x)


def angle_deg(a, b):
    """The angle between two directions, accurate near 0 (atan2 of the cross product's length and the dot product)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    c = np.cross(a, b)
    return float(np.degrees(np.arctan2(np.sqrt(c @ c), a @ b)))


def walker_world(n_frames, **kw):
    """A `synth_walk.walk` recording in its chunk world, the frame of its first camera -> (x [F,15,3], the true upward normal there,
    the floor's offset: the floor is normal . p = offset, and a standing foot point lies FOOT_HEIGHT above it), the walker.
    Without noise the joints are the walker's world joints themselves, so that a standing foot holds the same doubles in every frame
    of its stance; with noise they are the noisy camera-frame poses carried into the world by the true cameras."""
    from globalegomocap_amd import synth_walk
    w = synth_walk.walk(n_frames, **kw)
    R, head = w["cams"][:, :3, :3], w["cams"][:, :3, 3]
    world = np.einsum("fij,fkj->fki", R, w["local"]) + head[:, None, :] if kw.get("noise", 0.0) > 0 else w["world"]
    x = (world - head[0]) @ R[0]                                                 # inv(cams[0]): R0^T (p - head0), row vectors
    normal = R[0].T @ np.array([0.0, 0.0, 1.0])
    return x, normal, -float(head[0, 2]), w
