#!/usr/bin/env python3
"""Generate tests/golden/motion_windows.npz by running the UNMODIFIED reference's dataset code.

TEST INFRASTRUCTURE, like oracle/make_golden.py (whose import recipe this follows): runs only where the reference tree exists, never on
the GPU box, never from tests.  The reference's `networks/dataset/global_dataset.py` and `local_dataset.py` are imported with inert
stand-ins for open3d / cv2 / natsort; their `get_relative_global_pose_list` / `get_local_pose_list` run on an instance made with
`object.__new__` over synthetic sequences built by this repo's `synth`, and `load_pkls` over a recorded directory listing.  Stored:
the sequences' arrays (the tests write the pickles from them), every case's window counts and a deterministic subset of its windows
(the first and last of every sequence plus a few at random) as the reference's `__getitem__` returns them, and the file selections.

    python tools/make_golden_motion.py            # writes tests/golden/motion_windows.npz   (a few seconds)
"""
import os
import pickle
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("GEM_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "motion_windows.npz")
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from globalegomocap_amd import synth          # noqa: E402

# (name, frame_rate, frames, pose dtype, quaternion style): the frame rates give timers 1, 2, 2, 3 / 2 (75 at 30: half to even),
# 5 / 4; F and G are exactly total * timer and total * timer + 1 frames for frame_num 10, windows_size 2 at 25 fps
SEQUENCES = [("A", 25.0, 40, np.float32, "unit"), ("B", 50.0, 45, np.float64, "scaled"), ("C", 59.94, 50, np.float32, "negw"),
             ("D", 75.0, 60, np.float64, "near180"), ("E", 120.0, 60, np.float32, "scaled"), ("F", 25.0, 20, np.float64, "negw"),
             ("G", 25.0, 21, np.float64, "near180")]
# (poses, frame_num, windows_size, fps, slide_window)
CASES = [("global", 10, 1, 25, True), ("global", 10, 1, 30, True), ("global", 5, 2, 25, False), ("global", 10, 2, 25, True),
         ("local", 10, 1, 25, True), ("local", 5, 2, 30, True), ("local", 10, 1, 30, False)]
LISTING = ["CMU_01_walk_a.pkl", "KIT_3_run.pkl", "BMLmovi_Walking_2.pkl", "CMU_02_jump.pkl", "ACCAD_dance_1.pkl", "CMU_01_kick.pkl",
           "KIT_12_walk.pkl", "EKUT_sit_3.pkl", "CMU_walk_07.pkl", "HumanEva_box.pkl", "TotalCapture_walking2.pkl", "SFU_spin.pkl",
           "KIT_12_throw.pkl", "MPI_HDM05_bd_walk.pkl", "Transitions_mazurka.pkl", "CMU_09_wave.pkl", "BMLrub_sit.pkl",
           "DFaust_punch.pkl", "SSM_synced_walk.pkl", "CMU_01_crouch.pkl", "Eyes_Japan_walk_3.pkl", "KIT_5_stand.pkl",
           "ACCAD_walk_female.pkl", "BioMotionLab_run.pkl", "CMU_13_climb.pkl", "HumanEva_walking.pkl", "MPI_Limits_pose.pkl",
           "CMU_01_sit.pkl", "KIT_12_wipe.pkl", "SFU_walkturn.pkl"]
SEQ_NAMES = ["CMU_01", "KIT_12", "CMU", "walk", "nothing_matches"]


def import_reference(workdir):
    for name in ("open3d", "cv2", "natsort"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path[:0] = [REF, os.path.join(REF, "networks")]
    os.symlink(os.path.join(REF, "utils"), os.path.join(workdir, "utils"))
    os.chdir(workdir)
    from dataset import global_dataset, local_dataset
    return global_dataset, local_dataset


def make_sequences(rng):
    from scipy.spatial.transform import Rotation
    out = []
    for name, rate, n, dtype, style in SEQUENCES:
        poses = synth.make_motion(n, rng, t0=rng.uniform(0, 10)).astype(dtype)
        cams = synth.jitter_cameras(synth.make_cameras(n, step=0.03), rng, rot_deg=15.0, trans_m=0.2)
        base = Rotation.from_rotvec(rng.normal(size=3) * 1.5)
        R = base * Rotation.from_matrix(cams[:, :3, :3])
        loc = cams[:, :3, 3] + rng.normal(size=3) * 3.0
        if style == "near180":                # rotations within ~1 degree of a half turn: w close to 0, both signs
            axis = rng.normal(size=(n, 3))
            axis /= np.linalg.norm(axis, axis=1, keepdims=True)
            R = Rotation.from_rotvec(axis * (np.pi - rng.uniform(-0.02, 0.02, size=(n, 1))))
        q = R.as_quat()
        if style in ("scaled", "near180"):
            q = q * rng.uniform(0.3, 3.0, size=(n, 1))
        if style == "negw":
            q = q * np.where(q[:, 3:] > 0, -1.0, 1.0) * rng.uniform(0.5, 2.0, size=(n, 1))
        out.append(dict(name=name, frame_rate=rate, poses=poses, loc=loc, quat=q))
    return out


def as_pickle_dict(s):
    """The dict a motion pickle holds: a list of [15,3] arrays, a list of {'loc', 'rot'} dicts, the frame rate."""
    return {"local_pose_list": [p for p in s["poses"]], "cam_list": [{"loc": l, "rot": r} for l, r in zip(s["loc"], s["quat"])],
            "frame_rate": s["frame_rate"]}


def record_windows(gd, ld, seqs, rng, out):
    data_list = [as_pickle_dict(s) for s in seqs]
    for c, (poses, frame_num, ws, fps, slide) in enumerate(CASES):
        mod = gd if poses == "global" else ld
        inst = object.__new__(mod.AMASSDataset)
        inst.slide_window = slide

        def run(dl):
            if poses == "global":
                return inst.get_relative_global_pose_list(dl, frame_num=frame_num, windows_size=ws, fps=fps)
            return inst.get_local_pose_list(dl, frame_num=frame_num, windows_size=ws, fps=fps)
        counts = np.array([len(run([d])) for d in data_list], np.int64)
        allw = run(data_list)
        assert len(allw) == counts.sum()
        if poses == "global":
            inst.relative_pose_seq_list = allw
        else:
            inst.local_pose_seq_list = allw
        starts = np.concatenate([[0], np.cumsum(counts)])
        ids = set()
        for s in range(len(seqs)):
            if counts[s]:
                ids.update((int(starts[s]), int(starts[s + 1] - 1)))
        ids.update(int(i) for i in rng.choice(int(counts.sum()), size=6, replace=False))
        ids = np.array(sorted(ids), np.int64)
        win = np.stack([inst[int(i)].numpy() for i in ids])          # __getitem__: reshape to [T, 45], .float()
        assert win.dtype == np.float32
        key = "case%d/" % c
        out[key + "config"] = np.array([frame_num, ws, fps, int(slide)], np.int64)
        out[key + "poses"] = np.array(poses)
        out[key + "counts"] = counts
        out[key + "ids"] = ids
        out[key + "windows"] = win
        print("case %d %s frame_num %d windows_size %d fps %d slide %s: %d windows, %d recorded" %
              (c, poses, frame_num, ws, fps, slide, counts.sum(), len(ids)))


def record_selection(gd, workdir, out):
    d = os.path.join(workdir, "listing")
    os.makedirs(d)
    for name in LISTING:
        with open(os.path.join(d, name), "wb") as f:
            pickle.dump(name, f)

    class NumpyShim(types.ModuleType):
        def __getattr__(self, k):
            return getattr(np, k)

    shim_np = NumpyShim("numpy")
    shim_np.load = lambda path: np.array(SEQ_NAMES)          # the reference's hard-coded seq_names.npy
    shim_os = types.SimpleNamespace(listdir=lambda path: list(LISTING), path=os.path)
    gd.np, gd.os = shim_np, shim_os
    inst = object.__new__(gd.AMASSDataset)
    for train in (True, False):
        for mo2cap2 in (False, True):
            key = "select/%s_%s" % ("train" if train else "test", "seqnames" if mo2cap2 else "all")
            out[key] = np.array(inst.load_pkls(d, train, mo2cap2, False))
            out[key + "_balanced_count"] = np.array(len(inst.load_pkls(d, train, mo2cap2, True)), np.int64)
    gd.np, gd.os = np, os
    out["select/listing"] = np.array(LISTING)
    out["select/seq_names"] = np.array(SEQ_NAMES)


def main():
    import scipy
    rng = np.random.default_rng(20261016)
    seqs = make_sequences(rng)
    out = {"scipy_version": np.array(scipy.__version__), "numpy_version": np.array(np.__version__)}
    for k, s in enumerate(seqs):
        p = "seq%d/" % k
        out[p + "name"] = np.array(s["name"])
        out[p + "frame_rate"] = np.array(s["frame_rate"], np.float64)
        out[p + "poses"], out[p + "loc"], out[p + "quat"] = s["poses"], s["loc"], s["quat"]
    out["n_seq"] = np.array(len(seqs), np.int64)
    with tempfile.TemporaryDirectory() as work:
        gd, ld = import_reference(work)
        record_windows(gd, ld, seqs, rng, out)
        record_selection(gd, work, out)
        os.chdir(REPO)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%.0f KB)" % (OUT, os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
