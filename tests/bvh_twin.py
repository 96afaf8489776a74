"""The numpy twin of the BVH route, written from its formulas: the tree, rest lengths, the position-only inverse
kinematics, Euler angles, `regrow` (positions only: no rotation anywhere), the text via Python's `%`, a file writer, and a parser with
forward kinematics of its own."""
import numpy as np

NAMES = ("Hips", "Spine", "Neck", "Right_collar", "Right_shoulder", "Right_elbow", "Right_wrist", "Left_collar", "Left_shoulder",
         "Left_elbow", "Left_wrist", "Right_hip", "Right_knee", "Right_ankle", "Right_foot", "Left_hip", "Left_knee", "Left_ankle", "Left_foot")
PARENTS = (-1, 0, 1, 2, 3, 4, 5, 2, 7, 8, 9, 0, 11, 12, 13, 0, 15, 16, 17)
JOINT = (-1, -1, 0, -1, 1, 2, 3, -1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14)
_X, _Y, _Z, _0 = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
_neg = lambda v: tuple(-x for x in v)          # noqa: E731
REST = np.array([_0, _0, _Y, _0, _neg(_X), _neg(_X), _neg(_X), _0, _X, _X, _X, _neg(_X), _neg(_Y), _neg(_Y), _Z, _X, _neg(_Y), _neg(_Y), _Z]) + 0.0          # (+ 0.0: no negative zeros)
N, CHANNELS, FIELD, FRAME_BYTES = 19, 60, 16, 960
HAS_REST = tuple(bool(np.any(r != 0)) for r in REST)
KIDS = tuple(tuple(c for c in range(N) if PARENTS[c] == n) for n in range(N))
ROOT_CHANNELS = ("Xposition", "Yposition", "Zposition", "Zrotation", "Xrotation", "Yrotation")
TINY, GIMBAL, DEG = 1e-12, 1.0 - 1e-10, 180.0 / np.pi


def move(X, crt=None):
    """c * (p . R) + t for every joint, crt = (c, R, t) or the 13 numbers of gem_sequence_align."""
    X = np.asarray(X, dtype=np.float64)
    if crt is None:
        return X
    if not isinstance(crt, tuple):
        crt = (crt[0], np.asarray(crt[1:10]).reshape(3, 3), np.asarray(crt[10:13]))
    return crt[0] * (X @ crt[1]) + crt[2]


def node_positions(X):
    """[..., 15, 3] joints -> [..., 19, 3]: a node on its joint, Hips on the midpoint of joints 7 and 11, a helper on its parent."""
    X = np.asarray(X, dtype=np.float64)
    out = np.empty(X.shape[:-2] + (N, 3))
    for n in range(N):
        out[..., n, :] = X[..., JOINT[n], :] if JOINT[n] >= 0 else (X[..., 7, :] + X[..., 11, :]) / 2 if n == 0 else out[..., PARENTS[n], :]
    return out


def rest_lengths(X, crt=None):
    pos = node_positions(move(X, crt)).reshape(-1, N, 3)
    return np.array([np.linalg.norm(pos[:, n] - pos[:, PARENTS[n]], axis=-1).mean() if HAS_REST[n] else 0.0 for n in range(N)])


def _unit(v):
    return v / np.sqrt(v @ v)


def _frame_from(xd, hint):
    """Columns x = unit(xd), z = unit(x cross hint), y = z cross x; None where a direction is missing."""
    nx = np.sqrt(xd @ xd)
    if nx < TINY:
        return None
    x = xd / nx
    zc = np.cross(x, hint)
    nz = np.sqrt(zc @ zc)
    if nz < TINY:
        return None
    z = zc / nz
    return np.stack([x, np.cross(z, x), z], axis=1)


def shortest_arc(r, l):
    v = np.cross(r, l)
    s, c = np.sqrt(v @ v), r @ l
    if s < TINY:
        if not c < 0:
            return np.eye(3)
        k = _unit(np.cross(r, _Y if abs(r[0]) >= 0.9 else _X))
        return 2.0 * np.outer(k, k) - np.eye(3)
    k = v / s
    th = np.arctan2(s, c)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(th) * np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * np.outer(k, k)


def euler(R):
    """R = Rz(a) Rx(b) Ry(c) -> (a, b, c) in degrees."""
    if abs(R[2, 1]) > GIMBAL:
        return np.array([np.arctan2(R[1, 0], R[0, 0]) * DEG, 90.0 if R[2, 1] > 0 else -90.0, 0.0])
    return np.array([np.arctan2(-R[0, 1], R[1, 1]) * DEG, np.arcsin(R[2, 1]) * DEG, np.arctan2(-R[2, 0], R[2, 2]) * DEG])


def euler_matrix(a, b, c):
    a, b, c = np.radians(a), np.radians(b), np.radians(c)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    Ry = np.array([[np.cos(c), 0, np.sin(c)], [0, 1, 0], [-np.sin(c), 0, np.cos(c)]])
    return Rz @ Rx @ Ry


def frame_locals(X):
    """One frame [15,3] -> (P, the 19 local rotations [19,3,3])."""
    pos = node_positions(X)
    G, L = [None] * N, np.tile(np.eye(3), (N, 1, 1))
    G0 = _frame_from(X[11] - X[7], X[0] - pos[0])
    G[0] = np.eye(3) if G0 is None else G0
    L[0] = G[0]
    for n in range(1, N):
        Gp = G[PARENTS[n]]
        arcs = [c for c in KIDS[n] if HAS_REST[c]]
        if n == 2:
            Gn = _frame_from(X[4] - X[1], Gp[:, 1])
            G[n], L[n] = (Gp, np.eye(3)) if Gn is None else (Gn, Gp.T @ Gn)
        elif len(arcs) == 1 and len(KIDS[n]) == 1:
            d = pos[arcs[0]] - pos[n]
            ln = np.sqrt(d @ d)
            S = np.eye(3) if ln == 0.0 else shortest_arc(REST[arcs[0]], Gp.T @ (d / ln))
            G[n], L[n] = Gp @ S, S
        else:
            assert not KIDS[n], n          # a leaf: its parent's frame
            G[n] = Gp
    return pos[0], L


def channels(X, crt=None, unit_scale=1.0):
    """[n,15,3] -> [n,60]: the root's position times unit_scale, then (a, b, c) per node; leaves three zeros."""
    X = move(X, crt)
    out = np.zeros((len(X), CHANNELS))
    for f, x in enumerate(X):
        P, L = frame_locals(x)
        out[f, :3] = P * unit_scale
        for n in range(N):
            if n == 0 or KIDS[n]:
                out[f, 3 + 3 * n:6 + 3 * n] = euler(L[n])
    return out


def local_matrices(chan):
    """[n,60] -> [n,19,3,3] rebuilt from the angles."""
    return np.array([[euler_matrix(*row[3 + 3 * n:6 + 3 * n]) for n in range(N)] for row in np.asarray(chan)])


def fk(chan, offsets):
    """Forward kinematics of channels [n,60] over the offsets [19,3] -> node positions [n,19,3]."""
    chan = np.asarray(chan)
    out = np.empty((len(chan), N, 3))
    for f, row in enumerate(chan):
        G = [None] * N
        for n in range(N):
            R = euler_matrix(*row[3 + 3 * n:6 + 3 * n])
            if n == 0:
                out[f, 0], G[0] = offsets[0] + row[:3], R
            else:
                p = PARENTS[n]
                out[f, n], G[n] = out[f, p] + G[p] @ offsets[n], G[p] @ R
    return out


def offsets_of(rest, unit_scale=1.0):
    return REST * np.asarray(rest)[:, None] * unit_scale + 0.0


def regrow(X, rest, crt=None, unit_scale=1.0):
    """Positions only: a node = its parent's position plus its rest length times the observed direction of its bone; a helper on its
    parent; Hips on the observed midpoint.  [n,15,3] -> [n,19,3]."""
    pos = node_positions(move(X, crt))
    out = np.empty_like(pos)
    for n in range(N):
        if n == 0:
            out[:, 0] = pos[:, 0]
        elif not HAS_REST[n]:
            out[:, n] = out[:, PARENTS[n]]
        else:
            d = pos[:, n] - pos[:, PARENTS[n]]
            ln = np.linalg.norm(d, axis=-1, keepdims=True)
            assert (ln > 0).all(), "regrow needs bones with a direction"
            out[:, n] = out[:, PARENTS[n]] + rest[n] * d / ln
    return out * unit_scale


def joints_of(nodes):
    out = np.empty(nodes.shape[:-2] + (15, 3))
    for n, j in enumerate(JOINT):
        if j >= 0:
            out[..., j, :] = nodes[..., n, :]
    return out


# ------------------------------------------------------------------------------------------------------------------ text and files
def format_fields(values, per_line):
    """The bytes of the fields: Python's "%15.6f" and a space, a newline after every per_line-th value."""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    return "".join("%15.6f" % v + ("\n" if i % per_line == per_line - 1 else " ") for i, v in enumerate(values.tolist())).encode("ascii")


def hierarchy(rest, unit_scale=1.0):
    off, lines = offsets_of(rest, unit_scale), ["HIERARCHY"]

    def node(n, depth):
        pad = "  " * depth
        names = ROOT_CHANNELS if n == 0 else ROOT_CHANNELS[3:]
        lines.extend(["%s%s %s" % (pad, "JOINT" if n else "ROOT", NAMES[n]), pad + "{", "%s  OFFSET %.6f %.6f %.6f" % ((pad,) + tuple(off[n])),
                      "%s  CHANNELS %d %s" % (pad, len(names), " ".join(names))])
        for c in KIDS[n]:
            node(c, depth + 1)
        if not KIDS[n]:
            lines.extend([pad + "  End Site", pad + "  {", pad + "    OFFSET 0.000000 0.000000 0.000000", pad + "  }"])
        lines.append(pad + "}")
    node(0, 0)
    return "\n".join(lines) + "\n"


def write(path, X, fps=25, unit_scale=1.0, crt=None):
    rest, chan = rest_lengths(X, crt), channels(X, crt, unit_scale)
    with open(path, "wb") as f:
        f.write((hierarchy(rest, unit_scale) + "MOTION\nFrames: %d\nFrame Time: %.6f\n" % (len(chan), 1.0 / fps)).encode("ascii"))
        f.write(format_fields(chan, CHANNELS))
    return rest, chan


def parse(path):
    """A BVH file -> dict(names, parents, offsets [N,3], channels (names per node), frame_time, motion [n,C]), line by line."""
    with open(path) as f:
        lines = [l.split() for l in f.read().splitlines() if l.strip()]
    names, parents, offsets, chans, stack, end_site, i = [], [], [], [], [], False, 1
    assert lines[0] == ["HIERARCHY"]
    while lines[i] != ["MOTION"]:
        w = lines[i]
        if w[0] in ("ROOT", "JOINT"):
            names.append(w[1])
            parents.append(stack[-1] if stack else -1)
            offsets.append(None)
            chans.append(None)
            stack.append(len(names) - 1)
        elif w[0] == "End":
            end_site = True
        elif w[0] == "OFFSET" and not end_site:
            offsets[stack[-1]] = [float(x) for x in w[1:4]]
        elif w[0] == "CHANNELS":
            assert int(w[1]) == len(w) - 2
            chans[stack[-1]] = tuple(w[2:])
        elif w[0] == "}":
            if end_site:
                end_site = False
            else:
                stack.pop()
        else:
            assert w[0] in ("{", "OFFSET"), w
        i += 1
    assert not stack
    assert lines[i + 1][0] == "Frames:" and lines[i + 2][:2] == ["Frame", "Time:"]
    n = int(lines[i + 1][1])
    motion = np.array([[float(x) for x in l] for l in lines[i + 3:]]).reshape(n, -1)
    assert len(lines) - (i + 3) == n
    return dict(names=names, parents=parents, offsets=np.array(offsets), channels=chans, frame_time=float(lines[i + 2][2]), motion=motion)


def parsed_positions(p):
    """Forward kinematics of `parse`'s result for files of this module's tree and channel order -> [n,19,3]."""
    assert tuple(p["names"]) == NAMES and tuple(p["parents"]) == PARENTS
    assert p["channels"][0] == ROOT_CHANNELS and all(c == ROOT_CHANNELS[3:] for c in p["channels"][1:])
    return fk(p["motion"], p["offsets"])


def random_frames(n, seed, noise=0.05):
    """n frames: the mean skeleton plus `noise` metres of noise under a random rotation and translation, [n,15,3]."""
    from globalegomocap_amd import synth
    rng = np.random.default_rng(seed)
    out = np.empty((n, 15, 3))
    for f in range(n):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        Q *= np.sign(np.linalg.det(Q))
        out[f] = (synth.rest_skeleton() + rng.normal(0.0, noise, (15, 3))) @ Q.T + rng.normal(0.0, 1.0, 3)
    return out


def axis_aligned_pose():
    """The rest pose itself, bones of exactly representable lengths along their rest directions, away from the origin: [15,3]."""
    rest = np.array([0, 0, 0.5, 0, 0.25, 0.25, 0.125, 0, 0.25, 0.25, 0.125, 0.125, 0.5, 0.25, 0.125, 0.125, 0.5, 0.25, 0.125])
    nodes = np.zeros((N, 3))
    for n in range(1, N):
        nodes[n] = nodes[PARENTS[n]] + REST[n] * rest[n]
    return joints_of(nodes[None])[0] + np.array([0.25, 1.0, -0.5])


def corner_frames():
    """Axis-aligned skeletons that meet the defined corners, name -> [15,3]: every bone along an axis, so that every matrix entry is 0
    or +-1 (up to sin and cos of a right angle) and two implementations take the same branch."""
    P = axis_aligned_pose()

    def moved(joints, by):          # the joints of a limb from its first moved one on, rigidly
        a = P.copy()
        a[joints] = a[joints] + np.asarray(by, dtype=np.float64)
        return a
    out = {"every bone along its rest direction": P.copy()}
    out["right elbow bone antiparallel (r = -X)"] = moved([2, 3], [0.5, 0, 0])              # joint 2 = joint 1 + (0.25, 0, 0)
    out["left knee bone antiparallel (r = -Y)"] = moved([12, 13, 14], [0, 1.0, 0])         # joint 12 = joint 11 + (0, 0.5, 0)
    out["right foot bone antiparallel (r = +Z)"] = moved([10], [0, 0, -0.25])
    a = P.copy()
    a[3] = a[2]
    out["zero-length right wrist bone"] = a
    a = P.copy()
    a[11] = a[7]
    out["coinciding hips"] = a
    a = P.copy()          # the right knee straight ahead / behind of the hip: Rx(-+90) of the hip node, |R21| = 1
    a[8] = a[7] + np.array([0, 0, 0.5])
    a[9] = a[8] + np.array([0, 0, 0.25])
    a[10] = a[9] + np.array([0, 0.125, 0])
    out["gimbal, b = -90"] = a
    a = P.copy()
    a[8] = a[7] + np.array([0, 0, -0.5])
    a[9] = a[8] + np.array([0, 0, -0.25])
    a[10] = a[9] + np.array([0, -0.125, 0])
    out["gimbal, b = +90"] = a
    a = P.copy()
    a[0] = (P[7] + P[11]) / 2 + np.array([0.5, 0, 0])
    out["the neck on the hip line"] = a
    a = P.copy()
    a[4] = a[1]
    out["coinciding shoulders"] = a
    return out
