#!/usr/bin/env python3
"""What the depths from bone lengths cost, for a recording-sized batch:

    python tools/bone_depth_bench.py [--frames 2000] [--launches 20] [--out profiles/bone_depth_bench.json]

  bone_depths      the device time of gem_bone_depths for all frames in one call: between two device events, after a warm-up, the
                   median of --launches launches into resident buffers
  one_frame        the same for a single frame: a live push
  lift             gem_lift_keypoints for the same frames, for scale: the call the depths are made for
  accuracy         the mean distance (MPJPE) of depth x ray from the generated poses, and the solve's own residual

The frames are the generator's of the tests (forward kinematics with exact bone lengths, sigma 0.3 rad per bone, ray noise 0.003).
A record, not a gate.  Prints one JSON object and, with --out, writes it to FILE."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np          # noqa: E402


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


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=2000)
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--out", default=None, metavar="FILE")
    a = p.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    import bone_depth_twin as BT
    from globalegomocap_amd import bone_depth as B, prepare as P
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION, FisheyeCamera
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    n, rng = a.frames, np.random.default_rng(3)
    truth = BT.poses(n, 0.3, rng)
    kp = BT.detect(truth, cam, 0.003, rng)
    eng = P._lift_engine(DEFAULT_CALIBRATION, torch.cuda.current_device())
    opts = B.options()
    kp_d = torch.from_numpy(kp).to(eng.device)
    out = (torch.empty(n, 15, dtype=torch.float64, device=eng.device), torch.empty(n, 15, dtype=torch.uint8, device=eng.device),
           torch.empty(n, dtype=torch.float64, device=eng.device))
    res = {"frames": n, "device": torch.cuda.get_device_name(0), "iters": opts["iters"]}
    res["bone_depths"] = event_ms(lambda: eng.bone_depths(kp_d, opts=opts, out=out), a.launches)
    res["bone_depths"]["us_per_frame"] = round(1e3 * res["bone_depths"]["median_ms"] / n, 4)
    one = tuple(t[:1] for t in out)
    res["one_frame"] = event_ms(lambda: eng.bone_depths(kp_d[:1], opts=opts, out=one), a.launches)
    depth, solved, rms = eng.bone_depths(kp_d, opts=opts)
    res["lift"] = event_ms(lambda: eng.lift_keypoints(kp_d, depth), a.launches)
    lifted = eng.lift_keypoints(kp_d, depth)[0].cpu().numpy()
    err = BT.mpjpe(lifted, truth)
    res["accuracy"] = {"mpjpe_mean_mm": round(float(err.mean()) * 1e3, 3), "mpjpe_max_mm": round(float(err.max()) * 1e3, 3),
                       "frames_above_50_mm": int((err > 0.05).sum())}
    res["report"] = B.summarize(solved, rms).as_dict()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
