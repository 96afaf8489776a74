"""Shared by the motion-window tests: the sequences of tests/golden/motion_windows.npz (tools/make_golden_motion.py) as the dicts the
reference's pickles hold, written to a directory, and the per-element ulp distance of the parity contract."""
import os
import pickle

import numpy as np


def sequences(g):
    """[(name, dict as a motion pickle holds it)] in the fixture's order; float32 / float64 poses as recorded, the frame rate as a
    numpy scalar for every second sequence (the restricted reader must take both)."""
    out = []
    for k in range(int(g["n_seq"])):
        p = "seq%d/" % k
        rate = float(g[p + "frame_rate"])
        d = {"local_pose_list": [a for a in g[p + "poses"]],
             "cam_list": [{"loc": l, "rot": r} for l, r in zip(g[p + "loc"], g[p + "quat"])],
             "frame_rate": np.float64(rate) if k % 2 else rate, "other_key": "ignored"}
        out.append((str(g[p + "name"]) + ".pkl", d))
    return out


def write_pickles(g, path, protocol=pickle.HIGHEST_PROTOCOL):
    names = []
    for name, d in sequences(g):
        with open(os.path.join(str(path), name), "wb") as f:
            pickle.dump(d, f, protocol=protocol)
        names.append(name)
    return names


def cases(g):
    c = 0
    while "case%d/config" % c in g.files:
        fn, ws, fps, slide = (int(v) for v in g["case%d/config" % c])
        yield c, str(g["case%d/poses" % c]), fn, ws, fps, bool(slide)
        c += 1


def ulps(a, ref):
    """|a - ref| in units of float32 spacing at ref (np.spacing), per element."""
    ref = np.asarray(ref, np.float32)
    return np.abs(np.asarray(a, np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
