"""numpy twin of gem_heatmap_peaks: the kernel operation for operation, vectorised over frames and joints (every
operation is elementwise over them, so a joint's numbers are those of a scalar loop), in float64 or -- the same code -- np.longdouble;
the other peak estimators the design compares it with; and the inputs of the device tests."""
import numpy as np

import bone_depth_twin as BT
import keypoints_twin as KT

R, N, ITERS, LANES = 4, 9, 8, 16          # the window's reach, its side, the iterations, the lanes of a joint's group
TAU = 1.5


def integer_stage(heat):
    """heat [n,H,W,J] f32 -> (arg [n,J] int32: the flat row-major index of the maximum, peak [n,J] f32).  The rule of `lift_better`,
    restated without np.argmax on the values: the first NaN if there is one, else the first texel equal to the largest value."""
    heat = np.asarray(heat, dtype=np.float32)
    n, H, W, J = heat.shape
    flat = heat.reshape(n, H * W, J)
    nan = np.isnan(flat)
    with np.errstate(invalid="ignore"):
        top = np.where(nan, -np.inf, flat).max(axis=1, keepdims=True)
        first_top = (flat == top).argmax(axis=1)          # (argmax of booleans: the first True)
    arg = np.where(nan.any(axis=1), nan.argmax(axis=1), first_top).astype(np.int32)
    peak = np.take_along_axis(flat, arg[:, None, :].astype(np.int64), axis=1)[:, 0, :]
    return arg, peak


def window(heat, arg):
    """The registers of pass 2: [n,J,16,9] float32 -- lane r < 9 holds row sy - 4 + r, columns sx - 4 .. sx + 4, zero outside the map and in
    lanes 9 .. 15."""
    heat = np.asarray(heat, dtype=np.float32)
    n, H, W, J = heat.shape
    sx, sy = arg % W, arg // W
    rows = sy[..., None] - R + np.arange(LANES)                     # [n,J,16]
    cols = sx[..., None] - R + np.arange(N)                         # [n,J,9]
    inside = ((rows >= 0) & (rows < H) & (np.arange(LANES) < N))[..., :, None] & ((cols >= 0) & (cols < W))[..., None, :]
    f = np.arange(n)[:, None, None, None]
    j = np.arange(J)[None, :, None, None]
    t = heat[f, np.clip(rows, 0, H - 1)[..., :, None], np.clip(cols, 0, W - 1)[..., None, :], j]
    return np.where(inside, t, np.float32(0.0))


def _sum16(v):
    """The xor butterfly over the 16 lanes (last axis): levels 8, 4, 2, 1; every lane ends with the same sum."""
    lane = np.arange(LANES)
    for o in (8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v


def mean_shift(heat, arg, dtype=np.float64, iters=ITERS):
    """-> (m_x, m_y) [n,J] in texels, `dtype`: eight iterations from the integer maximum, the kernel's expressions in the kernel's order."""
    heat = np.asarray(heat, dtype=np.float32)
    W = heat.shape[2]
    sx, sy = arg % W, arg // W
    w = np.fmax(window(heat, arg).astype(dtype), dtype(0.0))        # [n,J,16,9]; (a NaN texel weighs nothing)
    lane = np.arange(LANES)
    xc = (sx[..., None] - R + lane).astype(dtype)                   # [n,J,16]: lane r makes the table entry of column sx - 4 + r ...
    yc = (sy[..., None] - R + lane).astype(dtype)                   # ... and of row sy - 4 + r
    xs = (sx[..., None] - R + np.arange(N)).astype(dtype)           # [n,J,9]
    inv2t2 = dtype(1.0) / (dtype(2.0) * dtype(TAU) * dtype(TAU))
    mx, my = sx.astype(dtype), sy.astype(dtype)
    with np.errstate(all="ignore"):
        for _ in range(iters):
            dx, dy = xc - mx[..., None], yc - my[..., None]
            kx, ky = np.exp(-(dx * dx) * inv2t2), np.exp(-(dy * dy) * inv2t2)
            s0, s1 = np.zeros_like(kx), np.zeros_like(kx)
            for c in range(N):
                t = w[..., c] * kx[..., c:c + 1]                      # (the broadcast of lane c's column weight)
                s0 = s0 + t
                s1 = s1 + t * xs[..., c:c + 1]
            r0, r1 = ky * s0, ky * s1
            r2 = r0 * yc
            t0, t1, t2 = _sum16(r0)[..., 0], _sum16(r1)[..., 0], _sum16(r2)[..., 0]
            mx, my = t1 / t0, t2 / t0
    return mx, my


def usable_peak(peak, min_peak=0.0):
    """Not NaN, positive, not below min_peak."""
    with np.errstate(invalid="ignore"):
        return (peak > 0) & ~(peak.astype(np.float64) < min_peak)


def peaks(heat, upscale=16, pad_x=128, pad_y=0, min_peak=0.0, dtype=np.float64):
    """heat [n,H,W,J] f32 -> (kp [n,J,3] `dtype`: (u, v, confidence), (0, 0, 0) for an unusable joint; arg [n,J] int32)."""
    heat = np.asarray(heat, dtype=np.float32)
    _, H, W, _ = heat.shape
    arg, peak = integer_stage(heat)
    mx, my = mean_shift(heat, arg, dtype)
    su = dtype(upscale) * dtype(W) / dtype(W - 1)
    sv = dtype(upscale) * dtype(H) / dtype(H - 1)
    ok = usable_peak(peak, min_peak)
    with np.errstate(invalid="ignore"):
        u, v = dtype(pad_x) + mx * su, dtype(pad_y) + my * sv
        conf = np.fmin(peak, np.float32(1.0)).astype(dtype)
    kp = np.stack([np.where(ok, u, 0), np.where(ok, v, 0), np.where(ok, conf, 0)], axis=-1).astype(dtype)
    return kp, arg


# ------------------------------------------------------------------------------------------------------------------ the other estimators
def _texel_to_image(ix, iy, conf, H, W, upscale=16, pad_x=128, pad_y=0):
    return np.stack([pad_x + ix * (upscale * W / (W - 1)), pad_y + iy * (upscale * H / (H - 1)), conf], axis=-1)


def reference_argmax(heat):
    """gem_lift_skeleton's image point: (128 + 16 sx, 16 sy), the top-left pixel of the maximum's 16 x 16 block."""
    arg, peak = integer_stage(heat)
    W = heat.shape[2]
    return np.stack([128.0 + 16.0 * (arg % W), 16.0 * (arg // W), np.fmin(peak, 1.0)], axis=-1).astype(np.float64)


def sampled_argmax(heat):
    """The integer maximum through the map at which the reprojection term samples."""
    arg, peak = integer_stage(heat)
    _, H, W, _ = heat.shape
    return _texel_to_image((arg % W).astype(np.float64), (arg // W).astype(np.float64), np.fmin(peak, 1.0).astype(np.float64), H, W)


def centroid(heat, reach=3):
    """The centre of mass of the (2 reach + 1)^2 texels round the maximum."""
    heat = np.asarray(heat, dtype=np.float32)
    n, H, W, J = heat.shape
    arg, peak = integer_stage(heat)
    sx, sy = arg % W, arg // W
    off = np.arange(-reach, reach + 1)
    rows, cols = sy[..., None] + off, sx[..., None] + off
    inside = ((rows >= 0) & (rows < H))[..., :, None] & ((cols >= 0) & (cols < W))[..., None, :]
    t = heat[np.arange(n)[:, None, None, None], np.clip(rows, 0, H - 1)[..., :, None], np.clip(cols, 0, W - 1)[..., None, :],
             np.arange(J)[None, :, None, None]]
    w = np.where(inside, np.fmax(t.astype(np.float64), 0.0), 0.0)
    with np.errstate(all="ignore"):
        ix = (w * cols[..., None, :]).sum(axis=(-1, -2)) / w.sum(axis=(-1, -2))
        iy = (w * rows[..., :, None]).sum(axis=(-1, -2)) / w.sum(axis=(-1, -2))
    return _texel_to_image(ix, iy, np.fmin(peak, 1.0).astype(np.float64), H, W)


def log_parabola(heat):
    """The vertex of the parabola through the logarithms of the maximum and its two neighbours, per axis."""
    heat = np.asarray(heat, dtype=np.float32)
    n, H, W, J = heat.shape
    arg, peak = integer_stage(heat)
    sx, sy = arg % W, arg // W
    f, j = np.arange(n)[:, None], np.arange(J)[None, :]
    g = lambda yy, xx: np.log(np.fmax(heat[f, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1), j].astype(np.float64), 1e-12))          # noqa: E731
    c = g(sy, sx)
    with np.errstate(all="ignore"):
        lx, rx, uy, dy = g(sy, sx - 1), g(sy, sx + 1), g(sy - 1, sx), g(sy + 1, sx)
        ox = np.where((sx > 0) & (sx < W - 1), 0.5 * (lx - rx) / (lx - 2 * c + rx), 0.0)
        oy = np.where((sy > 0) & (sy < H - 1), 0.5 * (uy - dy) / (uy - 2 * c + dy), 0.0)
    ox, oy = np.clip(np.nan_to_num(ox), -1, 1), np.clip(np.nan_to_num(oy), -1, 1)
    return _texel_to_image(sx + ox, sy + oy, np.fmin(peak, 1.0).astype(np.float64), H, W)


# ------------------------------------------------------------------------------------------------------------------ the accuracy case
ACC_FRAMES, ACC_SEED, ACC_SIGMA_POSE = 200, 2024, 0.3


def accuracy_case(camera):
    """The 200 generator poses of the design's table and their exact detections: (truth [200,15,3], kp [200,15,3])."""
    truth = BT.poses(ACC_FRAMES, ACC_SIGMA_POSE, np.random.default_rng(ACC_SEED))
    return truth, BT.detect(truth, camera, noise=0)


def noisy_maps(kp, sigma, noise=0.0, seed=1, H=64, W=64):
    """`KT.splat(kp, H, W, sigma)`, plus Gaussian noise of `noise` on every texel."""
    heat = KT.splat(kp, H, W, sigma)
    if noise:
        heat = (heat + np.random.default_rng(seed).normal(0, noise, heat.shape)).astype(np.float32)
    return heat


def pixel_error(kp, truth_kp):
    """Distance in pixels of the fisheye image between the detections' (u, v): [n,J]."""
    return np.linalg.norm(np.asarray(kp, dtype=np.float64)[..., :2] - np.asarray(truth_kp, dtype=np.float64)[..., :2], axis=-1)


def solve_mpjpe(kp, truth, camera, opts):
    """Mean over frames of the MPJPE, in metres, of the bone solve's positions from these detections against the generated poses."""
    depth, _, _ = BT.solve(kp, camera, opts)
    return float(BT.mpjpe(BT.positions(kp, depth, camera), truth).mean())


# ------------------------------------------------------------------------------------------------------------------ the device test's cases
CASE_SIZES, CASE_SEED = (1, 3, 67), 11
H, W, J = 64, 64, 15
GATE_FLOOR = 1e-12          # pixels


def special_maps(rng):
    """The maps that try the integer stage and the clipping of the window, [k,64,64] float32 each with what it tries: ties, a plateau,
    NaNs, non-positive values only, all zeros, -inf only, and the maximum in each corner and on each edge."""
    out = []
    blob = lambda cx, cy, s=1.5, a=0.8: (a * np.exp(-((np.arange(W)[None, :] - cx) ** 2 + (np.arange(H)[:, None] - cy) ** 2) / (2 * s * s))).astype(np.float32)          # noqa: E731
    tie = blob(20.3, 30.6) + blob(44.3, 12.6)                       # two blobs of the same shape ...
    tie[13, 44] = tie[31, 20] = max(tie[13, 44], tie[31, 20])       # ... and the same maximum bit for bit: the first in row-major order wins
    out.append(tie)
    plateau = blob(33.0, 40.0)
    plateau[39:42, 32:35] = plateau.max()                           # a 3 x 3 plateau
    out.append(plateau)
    nan1 = blob(10.2, 50.7)
    nan1[7, 9] = nan1[20, 3] = np.nan                               # NaN is maximal, the first one wins
    out.append(nan1)
    nan2 = blob(25.5, 25.5)
    nan2[24, 27] = np.nan                                           # a NaN beside the maximum: it weighs nothing
    nan2[0, 0] = -1.0
    out.append(np.where(np.isnan(nan2), np.float32(np.nan), nan2))
    neg = -np.abs(rng.normal(0.3, 0.2, (H, W))).astype(np.float32) - np.float32(1e-3)
    out.append(neg)                                                 # only negative values
    out.append(np.minimum(rng.normal(-0.2, 0.2, (H, W)), 0.0).astype(np.float32))          # non-positive with zeros
    out.append(np.zeros((H, W), dtype=np.float32))
    out.append(np.full((H, W), -np.inf, dtype=np.float32))
    for cx, cy in ((0.0, 0.0), (63.0, 0.0), (0.0, 63.0), (63.0, 63.0), (0.4, 31.7), (62.8, 17.2), (40.1, 0.3), (22.6, 62.9), (2.5, 61.2)):
        out.append(blob(cx, cy))
    out[4][63, 63] = np.float32(-1e-3)                               # (the largest of the negative map: its last texel)
    return out


def cases(n, camera, seed=CASE_SEED):
    """n frames [n,64,64,15] float32 for the device test: splats of generator detections (sigma 1.5, confidence 0.8) with, from the second
    frame on, the special maps put in joint after joint; for n = 67 texel noise of 0.02 on every frame from the tenth on."""
    rng = np.random.default_rng(seed + n)
    kp = BT.detect(BT.poses(n, 0.3, rng), camera, conf=0.8)
    heat = KT.splat(kp, H, W, 1.5)
    if n > 9:
        heat[9:] = (heat[9:] + rng.normal(0, 0.02, heat[9:].shape)).astype(np.float32)
    special = special_maps(rng)
    slots = [(f, j) for f in range(min(1, n - 1), n) for j in range(J)]
    if n == 1:
        slots = slots[:6]          # (a single frame: some usual joints stay)
    for (f, j), m in zip(slots, special):
        heat[f, :, :, j] = m
    return np.ascontiguousarray(heat)


_gate = {}


def device_cases(camera):
    """Per size of CASE_SIZES: the maps, the float64 twin's (kp, arg), and per joint the spread in pixels between the float64 and the
    longdouble twin; under "gate" THE GATE of the device test on (u, v): 16 times the largest spread over all these cases (the margin
    covers another valid rounding of the same expressions: the device's exp is not numpy's), floor GATE_FLOOR.  No joint is left out: the
    iteration is a contraction without accept / reject decisions, so the twins cannot part ways.  Computed once per process."""
    if not _gate:
        worst = 0.0
        for n in CASE_SIZES:
            heat = cases(n, camera)
            kp, arg = peaks(heat)
            kl, _ = peaks(heat, dtype=np.longdouble)
            spread = np.abs(kp[..., :2] - kl[..., :2]).max(axis=-1).astype(np.float64)
            assert np.isfinite(spread).all() and np.array_equal(kp[..., 2], kl[..., 2].astype(np.float64))
            worst = max(worst, float(spread.max()))
            _gate[n] = dict(heat=heat, kp=kp, arg=arg, spread=spread)
        _gate["gate"] = max(16.0 * worst, GATE_FLOOR)
    return _gate


def bone_gate(camera, opts):
    """Section 6q's gate on the bone solve's depths, in metres, as tests/test_bone_depth_gpu.py computes it: 16 times the largest spread
    between the float64 and the longdouble twin of the solve over that test's cases, the ill-conditioned frames left out."""
    worst = 0.0
    for n in BT.CASE_SIZES:
        kp = BT.cases(n, camera)
        d, _, rms = BT.solve(kp, camera, opts)
        dl, _, rl = BT.solve(kp, camera, opts, np.longdouble)
        spread = np.maximum(np.abs(d - dl).max(axis=1), np.abs(rms - rl)).astype(np.float64)
        worst = max(worst, float(spread[spread <= BT.ILL_CONDITIONED].max()))
    return 16.0 * worst
