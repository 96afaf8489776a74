"""numpy twin of gem_foot_lock (globalegomocap_amd/csrc/foot_lock.h): every stance of a foot is held at one
place on the floor, the correction is eased in and out around it, and each leg is re-solved by two-bone inverse kinematics from the
unmoved hip.  float64, written step by step as the device writes it; the twin is the specification.  The contact rule is
ground_twin's (a candidate within tau_h of the plane), and the plane (n, d) is an argument.  No GPU."""
import numpy as np

from ground_twin import FEET, _Margin

LEGS = ((7, 8, 9, 10), (11, 12, 13, 14))          # (hip, knee, ankle, foot) right, left
MOVED = (8, 9, 10, 12, 13, 14)
STATUS_OK, NO_CONTACT, BAD_GROUND = 0, 2, 3
DEGENERATE = 1e-9          # a direction shorter than this is none
ON_PLANE = 1e-12           # an anchor this near the plane is on it: d is a rounded sum, and moving an anchor by that rounding would change doubles that are right
DEFAULTS = dict(lag=5, tau_v=0.10, tau_h=0.05, min_run=3, blend=3, snap=True, stretch=0.05)
COUNTS = ("runs_right", "runs_left", "pinned_right", "pinned_left", "changed", "lengthened", "unreachable", "slide_pairs", "frames")
FLOATS = ("delta_max", "delta_mean", "knee_max", "stretch_max", "slide_before", "slide_after")


def default_blend(fps):
    """0.12 s in frames, at least one."""
    return max(1, int(round(0.12 * fps)))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _norm(a):
    return float(np.sqrt(_dot(a, a)))


def ease(u):
    """k(u) = 1 - u^2 (3 - 2 u) on [0, 1], 0 beyond."""
    return 1.0 - (u * u) * (3.0 - 2.0 * u) if u < 1.0 else 0.0


def foot_points(x):
    return np.stack([0.5 * (x[:, a] + x[:, b]) for a, b in FEET], axis=1)          # [F,2,3]


def contacts(q, n, d, lag, tau_v, tau_h, margin):
    """Step 1: [F,2] bool, a candidate (the earlier frame of a still pair) within tau_h of the plane."""
    F = len(q)
    cand = np.zeros((F, 2), dtype=bool)
    if F > lag:
        diff = q[lag:] - q[:-lag]
        dq = np.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2])
        margin.see(dq, tau_v)
        cand[:F - lag] = dq < tau_v
    h = (q[..., 0] * n[0] + q[..., 1] * n[1] + q[..., 2] * n[2]) - d
    margin.see(h[cand], tau_h)
    margin.see(h[cand], -tau_h)
    return cand & (np.abs(h) < tau_h)


def runs_of(c, min_run):
    """Step 2: the (start, end) pairs, end inclusive, of the maximal stretches of at least min_run set flags."""
    out, f, F = [], 0, len(c)
    while f < F:
        if not c[f]:
            f += 1
            continue
        s = f
        while f + 1 < F and c[f + 1]:
            f += 1
        if f - s + 1 >= min_run:
            out.append((s, f))
        f += 1
    return out


def anchor(q, s, e, n, d, snap, margin_s):
    """Step 3: the mean of q[s..e], taken about q[s] (feet that hold the same doubles give exactly those), put onto the plane unless
    it lies within ON_PLANE of it already."""
    acc = np.zeros(3)
    for f in range(s, e + 1):
        acc = acc + (q[f] - q[s])
    a = q[s] + acc / float(e - s + 1)
    if snap:
        off = _dot(n, a) - d
        margin_s.see(abs(off), ON_PLANE)
        if not abs(off) < ON_PLANE:
            a = a - off * n
    return a


def corrections(q, runs, anchors, blend):
    """Step 4 for one side: delta [F,3] and `pinned` [F] (the frames inside a run)."""
    F = len(q)
    delta, pinned = np.zeros((F, 3)), np.zeros(F, dtype=bool)
    r = -1          # the last run that starts at or before f
    for f in range(F):
        while r + 1 < len(runs) and runs[r + 1][0] <= f:
            r += 1
        if r >= 0 and f <= runs[r][1]:
            delta[f] = anchors[r] - q[f]
            pinned[f] = True
            continue
        before, after = r >= 0, r + 1 < len(runs)
        B = float(blend)
        if before and after:
            B = min(B, 0.5 * float(runs[r + 1][0] - runs[r][1]))
        t = np.zeros(3)
        if before:
            e = runs[r][1]
            t = t + (anchors[r] - q[e]) * ease(float(f - e) / B)
        if after:
            s = runs[r + 1][0]
            t = t + (anchors[r + 1] - q[s]) * ease(float(s - f) / B)
        delta[f] = t
    return delta, pinned


def _across(v, u):
    """The component of v perpendicular to the unit vector u."""
    return v - _dot(v, u) * u


def solve_leg(h, knee, ankle, foot, delta, stretch, margin, margin_b, axis_rule=None):
    """Step 5 -> (knee', ankle', foot', g, kind): kind 0 reachable, 1 too far and held, 2 too far and missed, 3 too near."""
    l1, l2 = _norm(knee - h), _norm(ankle - knee)
    target = ankle + delta
    D = _norm(target - h)
    margin.see(D, l1 + l2)
    margin.see(D, abs(l1 - l2))
    g, kind = 1.0, 0
    if D >= l1 + l2:
        u = (target - h) / D
        ratio = D / (l1 + l2)
        margin.see(ratio, 1.0 + stretch)
        g = min(ratio, 1.0 + stretch)
        kind = 2 if ratio > 1.0 + stretch else 1
        knee2, ankle2 = h + (g * l1) * u, h + (g * (l1 + l2)) * u
    elif D <= abs(l1 - l2):
        kind = 3
        margin_b.see(D, DEGENERATE)
        if D < DEGENERATE:          # the target is the hip itself: fold along the leg as it is
            v = ankle - h
            margin_b.see(_norm(v), DEGENERATE)
            if _norm(v) < DEGENERATE:
                return knee, ankle, foot, 1.0, kind
            u = v / _norm(v)
        else:
            u = (target - h) / D
        knee2 = h + (l1 if l1 >= l2 else -l1) * u
        ankle2 = h + abs(l1 - l2) * u
    else:
        u = (target - h) / D
        c = (l1 * l1 - l2 * l2 + D * D) / (2.0 * D)
        s = float(np.sqrt(max(l1 * l1 - c * c, 0.0)))
        w = _across(knee - h, u)
        margin_b.see(_norm(w), DEGENERATE)
        if _norm(w) < DEGENERATE:
            w = _across(foot - ankle, u)
            margin_b.see(_norm(w), DEGENERATE)
            if _norm(w) < DEGENERATE:          # the axis rule of the upright transform: the most nearly perpendicular world axis
                e = np.eye(3)[int(np.argmin(np.abs(u)))]
                w = _across(e, u)
                if axis_rule is not None:
                    axis_rule.append(1)
        b = w / _norm(w)
        knee2, ankle2 = h + c * u + s * b, target
    return knee2, ankle2, foot + (ankle2 - ankle), g, kind


def slide(q, runs, n):
    """The sum of the in-plane movement of a foot point between consecutive frames of one run, and the number of such pairs."""
    total, pairs = 0.0, 0
    for s, e in runs:
        for f in range(s, e):
            v = q[f + 1] - q[f]
            v = v - _dot(v, n) * n
            total += _norm(v)
            pairs += 1
    return total, pairs


def lock(x, n, d, lag=5, tau_v=0.10, tau_h=0.05, min_run=3, blend=3, snap=True, stretch=0.05):
    """x [F,15,3], the plane n . p = d -> dict: `sequence` [F,15,3], status, the counts of COUNTS, the figures of FLOATS (slide_* in
    metres per frame), `margin` (the smallest distance of a compared quantity from tau_v, +-tau_h, l1 +- l2 or 1 + stretch),
    `margin_degenerate` (likewise from the 1e-9 of the degeneracy tests), `margin_snap` (of an anchor's height from ON_PLANE), and for the tests `runs` (per side the (start, end) pairs),
    `anchors`, `delta` [F,2,3], `pinned` [F,2], `kind` [F,2] (-1: the leg was not touched) and `axis_rule` (legs bent towards a world axis)."""
    x = np.asarray(x, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    d = float(d)
    F = len(x)
    margin, margin_b, margin_s = _Margin(), _Margin(), _Margin()
    q = foot_points(x)
    c = contacts(q, n, d, int(lag), tau_v, tau_h, margin)
    runs = [runs_of(c[:, side], int(min_run)) for side in range(2)]
    out = x.copy()
    res = dict(status=STATUS_OK, sequence=out, runs=runs, frames=F, runs_right=len(runs[0]), runs_left=len(runs[1]))
    zero = dict(pinned_right=0, pinned_left=0, changed=0, lengthened=0, unreachable=0, slide_pairs=0, delta_max=0.0, delta_mean=0.0,
                knee_max=0.0, stretch_max=1.0, slide_before=0.0, slide_after=0.0)
    kind = np.full((F, 2), -1, dtype=np.int64)
    if not (runs[0] or runs[1]):
        res.update(zero, status=NO_CONTACT, axis_rule=0, margin=margin.value, margin_degenerate=margin_b.value, margin_snap=np.inf, anchors=[[], []],
                   delta=np.zeros((F, 2, 3)), pinned=np.zeros((F, 2), dtype=bool), kind=kind)
        return res
    anchors = [[anchor(q[:, side], s, e, n, d, snap, margin_s) for s, e in runs[side]] for side in range(2)]
    delta, pinned = np.zeros((F, 2, 3)), np.zeros((F, 2), dtype=bool)
    for side in range(2):
        delta[:, side], pinned[:, side] = corrections(q[:, side], runs[side], anchors[side], blend)
    fig = dict(zero)
    size_sum, axis_rule = 0.0, []
    for f in range(F):
        touched = False
        for side, (hip, kn, an, ft) in enumerate(LEGS):
            dl = delta[f, side]
            if pinned[f, side]:
                size = _norm(dl)
                size_sum += size
                fig["delta_max"] = max(fig["delta_max"], size)
            if not (dl[0] != 0.0 or dl[1] != 0.0 or dl[2] != 0.0):
                continue
            touched = True
            knee2, ankle2, foot2, g, k = solve_leg(x[f, hip], x[f, kn], x[f, an], x[f, ft], dl, stretch, margin, margin_b, axis_rule)
            kind[f, side] = k
            fig["lengthened"] += k in (1, 2)
            fig["unreachable"] += k in (2, 3)
            fig["stretch_max"] = max(fig["stretch_max"], g)
            fig["knee_max"] = max(fig["knee_max"], _norm(knee2 - x[f, kn]))
            out[f, kn], out[f, an], out[f, ft] = knee2, ankle2, foot2
        fig["changed"] += touched
    fig["pinned_right"], fig["pinned_left"] = int(pinned[:, 0].sum()), int(pinned[:, 1].sum())
    fig["delta_mean"] = size_sum / float(fig["pinned_right"] + fig["pinned_left"])
    q2 = foot_points(out)
    before = [slide(q[:, side], runs[side], n) for side in range(2)]
    after = [slide(q2[:, side], runs[side], n) for side in range(2)]
    fig["slide_pairs"] = before[0][1] + before[1][1]
    if fig["slide_pairs"]:
        fig["slide_before"] = (before[0][0] + before[1][0]) / fig["slide_pairs"]
        fig["slide_after"] = (after[0][0] + after[1][0]) / fig["slide_pairs"]
    res.update(fig, axis_rule=len(axis_rule), margin=margin.value, margin_degenerate=margin_b.value, margin_snap=margin_s.value, anchors=anchors, delta=delta, pinned=pinned, kind=kind)
    return res


# ------------------------------------------------------------------------------------------------------------------ the tests' inputs
WALKER_CASES = {          # name: (frames, the walker's parameters): the lengths tests/test_ground_gpu.py uses
    "3 frames": (3, {}),
    "6 frames": (6, {}),
    "40 frames": (40, dict(noise=0.03, seed=1)),
    "98 frames": (98, dict(noise=0.03, seed=0)),
    "98 frames without noise": (98, {}),
    "513 frames": (513, dict(noise=0.03, seed=4)),
    "the last length in LDS": (1024, dict(noise=0.03, seed=5)),
    "the first length in the work buffer": (1025, dict(noise=0.03, seed=6)),
    "standing": (98, dict(stand=[(0, 98)], noise=0.01, seed=7)),
}
# beyond the issue's list: a wearer who walks, then stands for 1 692 frames -- one run per foot that is longer than the 1 024 frames up
# to which a wavefront sums a run's anchor, and that does not begin at frame 0
LONG_STANCE = {"a stance of 1692 frames": (2000, dict(stand=[(300, 2000)], noise=0.01, seed=8))}
NOISY = ("40 frames", "98 frames", "513 frames", "the last length in LDS", "the first length in the work buffer", "standing")
HAND_FRAMES, HAND_FRAME = 12, 3          # the hand-made sequences' length, and the frame that is special in two of them


def _figure():
    """A figure that stands still with straight vertical legs, the floor at z = 0 and the neck above the middle of the foot points, so
    that the body's direction -- the plane's normal for feet that span no plane -- is (0, 0, 1) exactly."""
    p = np.zeros((15, 3))
    p[0] = (0.0, 0.06, 1.5)
    p[1:7] = [(-0.2, 0.03, 1.45), (-0.3, 0.03, 1.2), (-0.3, 0.1, 0.95), (0.2, 0.03, 1.45), (0.3, 0.03, 1.2), (0.3, 0.1, 0.95)]
    p[7:11] = [(-0.1, 0.0, 0.85), (-0.1, 0.0, 0.45), (-0.1, 0.0, 0.05), (-0.1, 0.12, 0.05)]          # the right foot points forward
    p[11:15] = [(0.1, 0.06, 0.85), (0.1, 0.06, 0.5), (0.1, 0.06, 0.1), (0.1, 0.06, 0.0)]             # the left one straight down
    return p


def hand_made(which):
    """Three sequences the walker never produces, HAND_FRAMES frames each:
    "knee on the line": both legs straight and the feet moved along them, so that every corrected knee lies exactly on the line from
        hip to target: the right leg takes its bending direction from the foot, the left one (its foot on the line too) from the axis rule;
    "hip raised": in frame HAND_FRAME the right leg and its hip stand 4.8 cm higher: the pin needs a leg more than 1.05 times as long;
    "target too near": a right leg folded almost shut whose foot stands 3 cm lower in frame HAND_FRAME: the pin lies nearer to the
        hip than |l1 - l2|."""
    x = np.repeat(_figure()[None], HAND_FRAMES, axis=0)
    up = np.array([0.0, 0.0, 1.0])
    if which == "knee on the line":
        for f in range(HAND_FRAMES):
            x[f, 9:11] += (0.004 * ((f * 7) % 5 - 2) + 0.001) * up
            x[f, 13:15] += (0.003 * ((f * 3) % 5 - 2) - 0.0005) * up
    elif which == "hip raised":
        x[HAND_FRAME, 7:11] += 0.048 * up
    elif which == "target too near":
        for f in range(HAND_FRAMES):
            low = f == HAND_FRAME
            hip, ankle = np.array([-0.1, 0.0, 0.30]), np.array([-0.1, 0.0, 0.02 if low else 0.05])
            l1, l2 = 0.45, 0.18 if low else 0.21
            D = _norm(ankle - hip)
            u = (ankle - hip) / D
            c = (l1 * l1 - l2 * l2 + D * D) / (2.0 * D)
            x[f, 7], x[f, 8], x[f, 9] = hip, hip + c * u + np.sqrt(l1 * l1 - c * c) * np.array([0.0, 1.0, 0.0]), ankle
            x[f, 10] = ankle + np.array([0.0, 0.12, 0.0])
    else:
        raise KeyError(which)
    return x


HAND_MADE = ("knee on the line", "hip raised", "target too near")


def case_input(name):
    """The sequence of a case, by its name in WALKER_CASES, LONG_STANCE or HAND_MADE."""
    if name in HAND_MADE:
        return hand_made(name)
    from ground_twin import walker_world
    F, kw = WALKER_CASES[name] if name in WALKER_CASES else LONG_STANCE[name]
    return walker_world(F, **kw)[0]
