"""numpy twin of gem_slam_bridge: the specification of the kinematic bridge over frames on which SLAM lost
tracking.  Everything is float64; the normal equations are built with explicit loops, in the order the device builds them.

`poses` [n,7] are the metric poses relative to the span's first frame (t xyz, q xyzw; rows of lost frames ignored), `tracked` [n]
says which rows count.  A GAP is a maximal run of lost frames with tracked neighbours e and s; a SYSTEM a maximal run of gaps
separated by fewer than two tracked frames, given as (first lost frame, frames up to and including its last lost frame).

  rotation     slerp between the unit quaternions of e and s (the second negated where their dot product is negative) at
               u = (t - e) / (s - e); the normalised linear blend where the angle between them is below 1e-8; the result is
               normalised and the matrix made from it
  translation  the unknown c_t minimise the sum of |c_{t-1} - 2 c_t + c_{t+1}|^2 over every t in [e, s] of the system whose three
               frames lie in the span and hold a lost frame.  Solved for the OFFSET from the straight line between the system's
               tracked neighbours (second differences of a line vanish), so the solve's rounding scales with centimetres of offset,
               not with metres of position
  chunks       origins[k] = G[a_k], cams[f] = inv(G[a_k]) G[f] with the rigid inverse (R^T, -R^T c)
"""
import numpy as np

SMALL_ANGLE = 1e-8
MAX_GAP = 64                  # GEM_BRIDGE_MAX_GAP: lost frames of one gap, and unknowns of one system
RECORD = ("status", "frames", "lost", "gaps", "systems", "longest_gap", "offset_max", "angle_max", "translation_max")
COUNTS = RECORD[:6]
FLOATS = RECORD[6:]


def quat_matrix(q):
    x, y, z, w = q
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                     [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                     [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]])


def unit(q):
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def slerp(q0, q1, u):
    """-> (the unit quaternion at u, the angle between the two QUATERNIONS: half the rotation's angle)."""
    q0, q1 = unit(np.asarray(q0, dtype=np.float64)), unit(np.asarray(q1, dtype=np.float64))
    d = q0[0] * q1[0] + q0[1] * q1[1] + q0[2] * q1[2] + q0[3] * q1[3]
    if d < 0.0:
        q1, d = -q1, -d
    theta = np.arccos(min(d, 1.0))
    if theta < SMALL_ANGLE:
        q = (1.0 - u) * q0 + u * q1
    else:
        q = (np.sin((1.0 - u) * theta) * q0 + np.sin(u * theta) * q1) / np.sin(theta)
    return unit(q), theta


def gaps_of(tracked):
    """[(first lost frame, lost frames)] of the maximal runs of lost frames."""
    out, t, n = [], 0, len(tracked)
    while t < n:
        if tracked[t]:
            t += 1
            continue
        s = t
        while s < n and not tracked[s]:
            s += 1
        out.append((t, s - t))
        t = s
    return out


def systems_of(tracked):
    """[(first lost frame, frames up to and including the last lost one)]: gaps with fewer than two tracked frames between them are one."""
    out = []
    for f, m in gaps_of(tracked):
        if out and f - (out[-1][0] + out[-1][1]) < 2:
            out[-1] = (out[-1][0], f + m - out[-1][0])
        else:
            out.append((f, m))
    return out


def line(c, e, s, t):
    u = (t - e) / (s - e)
    return c[e] + u * (c[s] - c[e])


def solve_system(c, tracked, first, length):
    """The translations of the system's lost frames, written into c."""
    n = len(c)
    e, s = first - 1, first + length
    lost = [t for t in range(first, s) if not tracked[t]]
    index = {t: i for i, t in enumerate(lost)}
    m = len(lost)
    known = {t: c[t] - line(c, e, s, t) for t in range(max(e - 1, 0), min(s + 1, n - 1) + 1) if tracked[t]}
    A, b = np.zeros((m, m)), np.zeros((m, 3))
    w = (1.0, -2.0, 1.0)
    for t in range(e, s + 1):
        if t - 1 < 0 or t + 1 > n - 1:
            continue
        tri = (t - 1, t, t + 1)
        if all(tracked[r] for r in tri):
            continue
        for p in range(3):
            if tracked[tri[p]]:
                continue
            i = index[tri[p]]
            for r in range(3):
                if tracked[tri[r]]:
                    b[i] = b[i] - (w[p] * w[r]) * known[tri[r]]
                else:
                    A[i, index[tri[r]]] += w[p] * w[r]
    x = np.linalg.solve(A, b)
    for t, i in index.items():
        c[t] = line(c, e, s, t) + x[i]
    return m


def rigid_inverse_times(Ga, Gf):
    R = Ga[:3, :3].T
    out = np.zeros((4, 4))
    out[:3, :3] = R @ Gf[:3, :3]
    out[:3, 3] = R @ (Gf[:3, 3] - Ga[:3, 3])
    out[3, 3] = 1.0
    return out


def bridge(poses, tracked, chunk_starts=(0,)):
    """-> dict: G [n,4,4], cams [n,4,4] (each chunk relative to its first frame), origins [n_chunks,4,4], bridged [n] uint8, and the
    record's fields."""
    poses, tracked = np.asarray(poses, dtype=np.float64), np.asarray(tracked).astype(bool)
    n = len(poses)
    if not (tracked[0] and tracked[-1]):
        raise ValueError("the first and the last frame must be tracked")
    c = np.where(tracked[:, None], poses[:, :3], 0.0)
    offset_max = angle_max = translation_max = 0.0
    systems = systems_of(tracked)
    for first, length in systems:
        if solve_system(c, tracked, first, length) > MAX_GAP:
            raise ValueError("a system of more than %d unknowns" % MAX_GAP)
    G = np.zeros((n, 4, 4))
    G[:, 3, 3] = 1.0
    for t in range(n):
        if tracked[t]:
            G[t, :3, :3] = quat_matrix(unit(poses[t, 3:7]))
    gaps = gaps_of(tracked)
    for first, m in gaps:
        e, s = first - 1, first + m
        for t in range(first, s):
            q, theta = slerp(poses[e, 3:7], poses[s, 3:7], (t - e) / (s - e))
            G[t, :3, :3] = quat_matrix(q)
            d = c[t] - line(c, e, s, t)
            offset_max = max(offset_max, float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])))
        d = c[s] - c[e]
        angle_max = max(angle_max, 2.0 * float(theta))
        translation_max = max(translation_max, float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])))
    G[:, :3, 3] = c
    starts = [int(a) for a in chunk_starts]
    cams = np.zeros((n, 4, 4))
    for k, a in enumerate(starts):
        b = starts[k + 1] if k + 1 < len(starts) else n
        for f in range(a, b):
            cams[f] = rigid_inverse_times(G[a], G[f])
    return {"G": G, "cams": cams, "origins": G[starts].copy(), "bridged": (~tracked).astype(np.uint8), "status": 0, "frames": n,
            "lost": int((~tracked).sum()), "gaps": len(gaps), "systems": len(systems), "longest_gap": max([m for _, m in gaps], default=0),
            "offset_max": offset_max, "angle_max": angle_max, "translation_max": translation_max}


# ------------------------------------------------------------------------------------------------------------------ test inputs
def walker_rows(n, seed=3, lost=()):
    """(the walker, its trajectory rows without the lines of the frame ranges `lost` [(a, b)])."""
    from globalegomocap_amd import synth_walk
    w = synth_walk.walk(n, seed=seed)
    keep = np.ones(n, dtype=bool)
    for a, b in lost:
        keep[a:b] = False
    return w, w["rows"][keep]


def relative_truth(w):
    """The walker's true cameras relative to its first one [n,4,4]."""
    return np.einsum("ij,njk->nik", np.linalg.inv(w["cams"][0]), w["cams"])


def errors(G, truth, frames):
    """(position errors in metres, rotation errors in degrees) of G against truth on `frames`."""
    pos = np.sqrt(((G[frames, :3, 3] - truth[frames, :3, 3]) ** 2).sum(-1))
    tr = np.einsum("nij,nij->n", G[frames, :3, :3], truth[frames, :3, :3])
    return pos, np.degrees(np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0)))


# the device tests' cases: name -> (frames, lost ranges, chunk starts)
CASES = {
    "12 frames, one lost": (12, ((5, 6),), (0,)),
    "40 frames, two gaps around one tracked frame": (40, ((5, 8), (9, 12)), (0,)),
    "220 frames, [80,100)": (220, ((80, 100),), (0, 100)),
    "220 frames, [60,68) and [130,160)": (220, ((60, 68), (130, 160)), (0, 100)),
    "200 frames, a gap of 64": (200, ((70, 134),), (0, 100)),
    "130 frames, the second chunk starts lost": (130, ((60, 70),), (0, 65)),
}
