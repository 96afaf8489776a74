"""Synthetic recordings in the pose network's file format, from parameters (tests, tools/prepare_bench.py, the golden recipe).

The pixels are a function of IEEE basic operations only -- the paraboloid max(0, 1 - ((x - cx)^2 + (y - cy)^2) / r^2) in float64,
then one cast -- so the same parameters give the same bits on every machine (no exp: libm's last bit differs between machines)."""
import hashlib
import os

import numpy as np


def paraboloid_heatmaps(centres, radii, size=64):
    """centres [n,J,2] (x = column, y = row), radii [n,J] -> [n,size,size,J] float64."""
    centres, radii = np.asarray(centres, dtype=np.float64), np.asarray(radii, dtype=np.float64)
    x = np.arange(size, dtype=np.float64)[None, None, :, None]
    y = np.arange(size, dtype=np.float64)[None, :, None, None]
    cx, cy = centres[:, None, None, :, 0], centres[:, None, None, :, 1]
    d2 = (x - cx) * (x - cx) + (y - cy) * (y - cy)
    return np.maximum(0.0, 1.0 - d2 / (radii * radii)[:, None, None, :])


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def write_recording(root, heat64, depth, names, as_float64=None, compressed=None, trajectory_rows=None, gt=None):
    """Writes `<root>/heatmaps/<name>` ({'heatmap': [H,W,J]}) and `<root>/depths/<name>` ({'depth': [1,J]}) per frame with
    scipy.io.savemat -- frame k's heat-map as float64 where as_float64[k], else cast to float32; both files compressed where
    compressed[k] -- plus `<root>/traj.txt` (rows `time tx ty tz qx qy qz qw`) and `<root>/gt.pkl` (a list of [J,3] arrays).
    Returns the paths (heatmap_dir, depth_dir, trajectory, gt)."""
    import pickle
    from scipy.io import savemat
    n = len(names)
    as_float64 = np.zeros(n, bool) if as_float64 is None else np.asarray(as_float64, bool)
    compressed = np.zeros(n, bool) if compressed is None else np.asarray(compressed, bool)
    hd, dd = os.path.join(root, "heatmaps"), os.path.join(root, "depths")
    os.makedirs(hd, exist_ok=True)
    os.makedirs(dd, exist_ok=True)
    for k, name in enumerate(names):
        h = heat64[k] if as_float64[k] else heat64[k].astype(np.float32)
        savemat(os.path.join(hd, name), {"heatmap": h}, do_compression=bool(compressed[k]))
        savemat(os.path.join(dd, name), {"depth": np.asarray(depth[k], dtype=np.float64).reshape(1, -1)}, do_compression=bool(compressed[k]))
    traj, gtp = os.path.join(root, "traj.txt"), os.path.join(root, "gt.pkl")
    if trajectory_rows is not None:
        with open(traj, "w") as f:
            for r in np.asarray(trajectory_rows):
                f.write(" ".join("%.9f" % v for v in r) + "\n")
    if gt is not None:
        with open(gtp, "wb") as f:
            pickle.dump([np.array(g) for g in gt], f)
    return hd, dd, traj, gtp


def random_parameters(n, seed, J=15, fps=25, first_id=0):
    """Parameters of an n-frame recording: heat-map centres / radii, depths, a smooth trajectory (frame ids first_id ..) and a
    ground truth whose head track is the SLAM head track under a similarity of scale 1.7, plus noise."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    centres = rng.uniform(6.2, 57.8, (n, J, 2))
    centres = np.floor(centres) + rng.uniform(0.1, 0.4, (n, J, 2))          # (no ties: the peak pixel is unique)
    radii = rng.uniform(3.0, 8.0, (n, J))
    depth = rng.uniform(0.3, 2.0, (n, J))
    i = np.arange(n, dtype=np.float64)
    t = (i + first_id) / fps + rng.uniform(-0.004, 0.004, n)
    quat = Rotation.from_euler("xyz", np.stack([0.3 + 0.01 * i, -0.2 + 0.02 * i, 0.1 - 0.015 * i], 1)).as_quat()
    pos = np.stack([1.0 + 0.1 * i, 0.002 * i * i, 0.3 - 0.05 * i], 1) + rng.normal(0, 0.01, (n, 3))
    rows = np.concatenate([t[:, None], pos, quat], 1)
    Rg = Rotation.from_euler("zyx", [0.4, -0.3, 0.2]).as_matrix()
    gt = (1.7 * pos @ Rg.T + np.array([0.5, -1.0, 2.0]))[:, None, :] + rng.normal(0, 0.05, (1, J, 3)) + rng.normal(0, 0.01, (n, J, 3))
    return {"centres": centres, "radii": radii, "depth": depth, "rows": rows, "gt": gt}
