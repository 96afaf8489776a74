#!/usr/bin/env python3
"""Measurements of the motion-window data path, one JSON line per leg.

    python tools/motion_windows_bench.py [--windows 1048576] [--fit-steps 300]      # on the GPU (under rocprofv3 for kernel times)
    python tools/motion_windows_bench.py --reference-rate [--windows 20000]          # on the CPU box: the reference's host build rate

Legs: `launch` (gem_motion_windows at B = 64 / 128: event time per launch over 2000 launches), `materialize` (every window of a
synthetic set of >= 1 M windows in one launch: bytes written per second), `fit` (full-size VAETrainer.fit steps/s at batch 64 from
the MotionWindows and from the same windows materialised), `load` (building the MotionWindows: host packing + upload + camera
conversion) and, with --reference-rate, the reference's get_relative_global_pose_list over the same synthetic sequences.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from globalegomocap_amd import synth  # noqa: E402


def synthetic_sequences(n_windows, frames=2000, seed=0):
    """Sequences of `frames` frames at 25 fps (frames - 10 global windows each at T = 10) with jittered cameras: (poses, loc, quat)."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    n_seq = -(-n_windows // (frames - 10))
    out = []
    for _ in range(n_seq):
        cams = synth.jitter_cameras(synth.make_cameras(frames, step=0.02), rng, rot_deg=10.0, trans_m=0.1)
        out.append((synth.make_motion(frames, rng, t0=rng.uniform(0, 10)).astype(np.float32), cams[:, :3, 3].copy(),
                    Rotation.from_matrix(cams[:, :3, :3]).as_quat()))
    return out


def emit(**kw):
    print(json.dumps(kw), flush=True)


def reference_rate(seqs, ref):
    import types
    import tempfile
    for name in ("open3d", "cv2", "natsort"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path[:0] = [ref, os.path.join(ref, "networks")]
    work = tempfile.mkdtemp()
    os.symlink(os.path.join(ref, "utils"), os.path.join(work, "utils"))
    os.chdir(work)
    from dataset import global_dataset
    inst = object.__new__(global_dataset.AMASSDataset)
    inst.slide_window = True
    data = [{"local_pose_list": list(p), "cam_list": [{"loc": l, "rot": r} for l, r in zip(lo, q)], "frame_rate": 25.0}
            for p, lo, q in seqs]
    t = time.perf_counter()
    w = inst.get_relative_global_pose_list(data, frame_num=10, windows_size=1, fps=25)
    dt = time.perf_counter() - t
    emit(leg="reference_host_build", windows=len(w), seconds=dt, windows_per_s=len(w) / dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1 << 20)
    ap.add_argument("--fit-steps", type=int, default=300)
    ap.add_argument("--reference-rate", action="store_true")
    ap.add_argument("--reference", default=os.environ.get("GEM_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    t = time.perf_counter()
    seqs = synthetic_sequences(a.windows)
    emit(leg="synthesis", seconds=time.perf_counter() - t, sequences=len(seqs))
    if a.reference_rate:
        return reference_rate(seqs, a.reference)

    import torch
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd.motion_data import MotionWindows
    from globalegomocap_amd.vae import VAEShape
    from globalegomocap_amd.vae_train import VAETrainer
    torch.cuda.set_device(0)
    torch.cuda.synchronize()
    t = time.perf_counter()
    ds = MotionWindows([(p, lo, q, 25.0) for p, lo, q in seqs], "global", 10)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    emit(leg="load", windows=len(ds), frames=ds.n_frames, seconds=dt, windows_per_s=len(ds) / dt,
         resident_bytes=int(ds.d_pose.numel() * 8 + ds.d_cam.numel() * 8))

    gen = torch.Generator(device="cpu").manual_seed(0)
    for B in (64, 128):
        ids = torch.randint(0, len(ds), (2000, B), generator=gen).to(ds.device)
        out = torch.empty((B, 10, 45), device=ds.device)
        for i in range(50):
            ds.batch(ids[i], out=out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(2000):
            ds.batch(ids[i], out=out)
        e1.record()
        torch.cuda.synchronize()
        emit(leg="launch", B=B, us_per_launch_including_enqueue=e0.elapsed_time(e1) * 1e3 / 2000)

    out = torch.empty((len(ds), 10, 45), device=ds.device)
    all_ids = torch.arange(len(ds), device=ds.device)
    perm = all_ids[torch.randperm(len(ds), generator=gen).to(ds.device)]
    for name, ids in (("in_order", all_ids), ("permuted", perm)):
        ds.batch(ids, out=out)
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ds.batch(ids, out=out)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        nbytes = out.numel() * 4
        emit(leg="materialize", ids=name, windows=len(ds), bytes_written=nbytes, median_s=float(np.median(times)),
             write_TB_per_s=nbytes / float(np.median(times)) / 1e12)
    del out, perm, all_ids

    shape = VAEShape()
    n_fit = 64 * a.fit_steps
    sub = MotionWindows([(p, lo, q, 25.0) for p, lo, q in synthetic_sequences(n_fit, seed=1)], "global", 10)
    mat = sub.materialize().cpu().numpy()
    for src_name, src in (("motion_windows", sub), ("materialized", mat), ("motion_windows", sub), ("materialized", mat)):
        tr = VAETrainer(shape, batch_size=64, seed=0)
        try:
            tr.fit(src, epochs=1, kl_weight=0.5, test_windows=False, log_step=10 ** 9, seed=0, log=lambda *x: None)   # warm-up
            torch.cuda.synchronize()
            t = time.perf_counter()
            tr.fit(src, epochs=1, kl_weight=0.5, test_windows=False, log_step=10 ** 9, seed=1, log=lambda *x: None)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
        finally:
            tr.close()
        steps = len(sub) // 64
        emit(leg="fit", source=src_name, batch=64, steps=steps, seconds=dt, steps_per_s=steps / dt)


if __name__ == "__main__":
    main()
