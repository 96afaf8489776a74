"""numpy float64 twins of the 2-D detection kernels: the splat, camera2world, hold and interpolate."""
import numpy as np

from globalegomocap_amd import synth


def usable(kp):
    """confidence > 0 (NaN is not) and u, v finite."""
    kp = np.asarray(kp, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (kp[..., 2] > 0) & np.isfinite(kp[..., 0]) & np.isfinite(kp[..., 1])


def heat_coords(kp, H=64, W=64):
    """Where the reprojection term samples image point (u, v): `synth.heatmap_coords` for an H x W map."""
    kp = np.asarray(kp, dtype=np.float64)
    return (kp[..., 0] - 128.0) * (W - 1) / 1024.0, kp[..., 1] * (H - 1) / 1024.0


def splat(kp, H=64, W=64, sigma=1.5):
    """kp [F,J,3] -> [F,H,W,J] float32: `synth.gaussian_heatmaps(ix, iy, sigma) * a`, a = clip(confidence, 0, 1), computed in float64
    and rounded once; an unusable joint's map is zero."""
    kp = np.asarray(kp, dtype=np.float64)
    ok = usable(kp)
    ix, iy = heat_coords(np.where(ok[..., None], kp, 0.0), H, W)
    a = np.where(ok, np.clip(np.where(ok, kp[..., 2], 0.0), 0.0, 1.0), 0.0)
    if H == W:
        g = synth.gaussian_heatmaps(ix, iy, sigma, size=H, dtype=np.float64)
    else:          # (gaussian_heatmaps' expression on an H x W grid)
        ys = np.arange(H, dtype=np.float64)[:, None, None]
        xs = np.arange(W, dtype=np.float64)[None, :, None]
        g = np.exp(-((xs - ix[..., None, None, :]) ** 2 + (ys - iy[..., None, None, :]) ** 2) / (2.0 * sigma * sigma))
    out = (g * a[:, None, None, :]).astype(np.float32)
    out[np.broadcast_to(~ok[:, None, None, :], out.shape)] = 0.0
    return out


def camera2world(points, depth, poly_c2w, cx, cy):
    """FishEyeCameraCalibrated.camera2world (utils/fisheye/FishEyeCalibrated.py:18-33): points [n,2], depth [n] -> [n,3]."""
    centred = np.asarray(points, dtype=np.float64) - np.array([cx, cy])
    x, y = centred[:, 0], centred[:, 1]
    r = np.sqrt(np.square(x) + np.square(y))
    z = np.polyval(np.asarray(poly_c2w, dtype=np.float64)[::-1], r)
    p = np.array([x, y, -z])
    return (p / np.linalg.norm(p, axis=0) * np.asarray(depth, dtype=np.float64)).transpose()


def lift(kp, depth, camera, prev=None):
    """kp [F,J,3], depth [F,J] -> (out [F,J,3], valid [F,J] uint8, prev afterwards).  prev None: unusable joints are zeros; prev [J,3]:
    frames in order, an unusable joint takes prev's value, a usable one updates it."""
    kp, depth = np.asarray(kp, dtype=np.float64), np.asarray(depth, dtype=np.float64)
    F, J = kp.shape[:2]
    ok = usable(kp)
    out = np.zeros((F, J, 3))
    held = None if prev is None else np.array(prev, dtype=np.float64)
    for f in range(F):
        for j in range(J):
            if ok[f, j]:
                out[f, j] = camera2world(kp[f, j:j + 1, :2], depth[f, j:j + 1], camera.poly_c2w, camera.cx, camera.cy)[0]
                if held is not None:
                    held[j] = out[f, j]
            elif held is not None:
                out[f, j] = held[j]
    return out, ok.astype(np.uint8), held


def fill_missing(seq, valid, n_chunks):
    """Per chunk and joint: invalid frames between valid frames lo < f < hi become seq[lo] + (seq[hi] - seq[lo]) (f - lo) / (hi - lo);
    in front of the first valid frame its value, behind the last valid frame that one's.  Explicit loops; -> a new array."""
    seq, valid = np.array(seq, dtype=np.float64), np.asarray(valid).astype(bool)
    n, J = valid.shape
    fpc = n // n_chunks
    for c in range(n_chunks):
        for j in range(J):
            good = [f for f in range(fpc) if valid[c * fpc + f, j]]
            if not good:
                continue
            for f in range(fpc):
                if valid[c * fpc + f, j]:
                    continue
                before = [g for g in good if g < f]
                after = [g for g in good if g > f]
                if not before:
                    seq[c * fpc + f, j] = seq[c * fpc + after[0], j]
                elif not after:
                    seq[c * fpc + f, j] = seq[c * fpc + before[-1], j]
                else:
                    lo, hi = before[-1], after[0]
                    p, q = seq[c * fpc + lo, j], seq[c * fpc + hi, j]
                    seq[c * fpc + f, j] = p + (q - p) * ((f - lo) / (hi - lo))
    return seq


# the validity pattern of the tests: 7 frames, joints 0 .. 4 -- leading gap, inner gap, trailing gap, a single valid frame, all valid
PATTERN = np.array([[0, 0, 1, 1, 1, 1, 1],
                    [1, 1, 0, 0, 0, 1, 1],
                    [1, 1, 1, 1, 0, 0, 0],
                    [0, 0, 0, 1, 0, 0, 0],
                    [1, 1, 1, 1, 1, 1, 1]], dtype=np.uint8).T          # [frame, joint]


def pattern_valid(n_chunks=1, n_joints=15):
    """PATTERN's five columns over `n_joints` joints (joint j: column j % 5, chunk k shifts the columns by k), [n_chunks * 7, n_joints]."""
    return np.concatenate([np.stack([PATTERN[:, (j + k) % 5] for j in range(n_joints)], axis=1) for k in range(n_chunks)])
