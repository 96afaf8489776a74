#!/usr/bin/env python3
"""What the 2-D detection route costs, for a synthetic recording of 2000 frames:

    python tools/keypoints_bench.py [--frames 2000] [--repeats 7] [--launches 20] [--work DIR] [--out profiles/keypoints_bench.json]

  splat            the device time of gem_keypoint_heatmaps for all frames: between two device events, after a warm-up, the median of
                   --launches launches into a resident buffer; the write rate it implies (frames x 64 x 64 x 15 x 4 bytes) next to the
                   write-only floor at the HBM rates MI355X_MICROARCH.md gives (6.29 TB/s measured with a float4 copy, 8.0 TB/s specified)
  lift, fill       the same for gem_lift_keypoints and gem_fill_missing
  detections       host-inclusive, synchronised: detections.recording_from_detections (scale route) alone, and followed by
                   whole_sequence.optimize_recording
  mat              the same recording -- its heat-maps are the splatted ones, written as float32 .mat files, page cache warm --
                   through prepare.prepare_sequence, alone and followed by optimize_recording: the route that existed before, whose
                   code this feature does not touch
  ratio            mat / detections, for both pairs

Prints one JSON object and, with --out, writes it to FILE."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402

HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "repeats": len(ms)}


def event_ms(fn, launches):
    import torch
    fn()
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(launches):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        z.record()
        z.synchronize()
        out.append(a.elapsed_time(z))
    return spread(out)


def wall_ms(fn, repeats):
    import torch
    fn()                                                          # first call: pools, pinned blocks, engines
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return spread(out)


def synthetic(n, seed=3):
    """n + 1 frames: detections at the projections of a moving skeleton, some lost; depths; trajectory rows."""
    from globalegomocap_amd import synth
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    rng = np.random.default_rng(seed)
    clean = synth.make_motion(n + 1, rng)
    est = clean + rng.normal(0.0, 0.02, clean.shape)
    uv = cam.project_numpy(clean.reshape(-1, 3)).reshape(n + 1, 15, 2)
    kp = np.concatenate([uv, rng.uniform(0.5, 1.0, (n + 1, 15, 1))], axis=2)
    lost = rng.random((n + 1, 15)) < 0.01
    lost[::100] = False                                           # (every chunk keeps every joint)
    kp[..., 2] = np.where(lost, 0.0, kp[..., 2])
    i = np.arange(n + 1, dtype=np.float64)
    rows = np.concatenate([(i / 25.0)[:, None], (0.004 * i)[:, None], np.zeros((n + 1, 5)), np.ones((n + 1, 1))], axis=1)
    return kp, np.linalg.norm(est, axis=-1), rows


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=2000)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--work", default=None, help="directory for the synthetic recording (default: a temporary one, removed afterwards)")
    p.add_argument("--out", default=None, metavar="FILE")
    a = p.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import detections as D, prepare as P, synth_recording as S, vae as V, whole_sequence as ws
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    from globalegomocap_amd.optimizer import SequenceOptimizer
    n = a.frames
    kp, depth, rows = synthetic(n)
    eng = P._lift_engine(DEFAULT_CALIBRATION, torch.cuda.current_device())
    res = {"frames": n, "device": torch.cuda.get_device_name(0), "detection_bytes": int(kp[:n].nbytes + depth[:n].nbytes),
           "heat_bytes": n * 64 * 64 * 15 * 4}
    # ---- the kernels
    kp_d, depth_d = torch.from_numpy(kp[:n]).to(eng.device), torch.from_numpy(depth[:n]).to(eng.device)
    heat = torch.empty(n, 64, 64, 15, dtype=torch.float32, device=eng.device)
    res["splat"] = event_ms(lambda: eng.keypoint_heatmaps(kp_d, out=heat), a.launches)
    res["splat"]["write_tb_s"] = round(res["heat_bytes"] / res["splat"]["median_ms"] / 1e9, 3)
    res["splat"]["floor_ms_at_%.2f_tb_s_measured_copy_rate" % HBM_MEASURED_TBS] = round(res["heat_bytes"] / HBM_MEASURED_TBS / 1e9, 4)
    res["splat"]["floor_ms_at_%.1f_tb_s_specified" % HBM_SPEC_TBS] = round(res["heat_bytes"] / HBM_SPEC_TBS / 1e9, 4)
    res["lift"] = event_ms(lambda: eng.lift_keypoints(kp_d, depth_d), a.launches)
    o64, _, valid = eng.lift_keypoints(kp_d, depth_d)
    res["fill"] = event_ms(lambda: eng.fill_missing(o64, valid, n // 100), a.launches)
    del heat, o64
    print("kernels: %s" % json.dumps({k: res[k] for k in ("splat", "lift", "fill")}), file=sys.stderr, flush=True)
    # ---- host-inclusive: detections against .mat files
    work = a.work or tempfile.mkdtemp(prefix="gem_keypoints_bench_")
    shape = V.VAEShape()
    kw = dict(global_vae_path=V.synthetic_state_dict(shape, seed=1, gain=2.0), local_vae_path=V.synthetic_state_dict(shape, seed=2, gain=2.0),
              verbose=False)
    kw["optimizer"] = SequenceOptimizer(DEFAULT_CALIBRATION, kw["global_vae_path"], kw["local_vae_path"], max_windows=12 * (n // 100))
    try:
        os.makedirs(work, exist_ok=True)
        det = os.path.join(work, "det.npz")
        np.savez(det, keypoints=kp, depth=depth)
        maps = eng.keypoint_heatmaps(kp).cpu().numpy()
        hd, dd, traj, _ = S.write_recording(os.path.join(work, "mat"), maps, depth, ["frame_%05d.mat" % k for k in range(n + 1)], None, None, rows, None)
        del maps
        print("recording written", file=sys.stderr, flush=True)
        res["mat_bytes"] = sum(os.path.getsize(os.path.join(d, f)) for d in (hd, dd) for f in os.listdir(d))
        for d in (hd, dd):                                        # page cache warm
            for f in os.listdir(d):
                with open(os.path.join(d, f), "rb") as fh:
                    fh.read()
        spans = P.chunk_spans(0, n + 1, 100)
        from_det = lambda: D.recording_from_detections(traj, det, scale=1.0, spans=spans, fps=25)                      # noqa: E731
        from_mat = lambda: P.prepare_sequence(traj, hd, dd, None, 0, n + 1, fps=25, test_size=100, verbose=False, scale=1.0)      # noqa: E731
        assert len(from_det()) == len(from_mat()) == n // 100
        res["detections_to_recording"] = wall_ms(from_det, a.repeats)
        res["mat_to_recording"] = wall_ms(from_mat, a.repeats)
        print("to_recording: detections %s, mat %s" % (res["detections_to_recording"], res["mat_to_recording"]), file=sys.stderr, flush=True)
        res["detections_to_result"] = wall_ms(lambda: ws.optimize_recording(from_det(), DEFAULT_CALIBRATION, ground_truth=False, **kw), a.repeats)
        res["mat_to_result"] = wall_ms(lambda: ws.optimize_recording(from_mat(), DEFAULT_CALIBRATION, ground_truth=False, **kw), a.repeats)
        res["ratio_to_recording"] = round(res["mat_to_recording"]["median_ms"] / res["detections_to_recording"]["median_ms"], 2)
        res["ratio_to_result"] = round(res["mat_to_result"]["median_ms"] / res["detections_to_result"]["median_ms"], 3)
    finally:
        if a.work is None:
            shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
