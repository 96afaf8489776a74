#!/usr/bin/env python3
"""What the sub-pixel peaks of the heat-maps cost, against the kernel that has streamed the same bytes so far:

    python tools/heat_peaks_bench.py [--frames 2000] [--launches 20] [--out profiles/heat_peaks_bench.json]

  heatmap_peaks    the device time of gem_heatmap_peaks for all frames in one call: between two device events, after a warm-up, the
                   median of --launches launches into resident buffers
  lift_skeleton    gem_lift_skeleton on the same tensor in the same run: the yardstick -- one pass over the same bytes, the integer
                   maximum alone
  ratio            heatmap_peaks / lift_skeleton.  Pass 2 re-reads about 5 KB of a 245 KB frame and adds a short dependent chain: a
                   ratio above 1.5 means that pass 2 is exposed
  one_frame        gem_heatmap_peaks for a single frame: a live push
  generic          gem_heatmap_peaks on the same frames behind a pointer that is not 16-byte aligned (the scalar scan)
  accuracy         the peaks against the detections the maps were splatted from, in pixels of the fisheye image

The maps are splats (sigma 1.5) of the tests' generator detections.  A record, not a gate.  Prints one JSON object and, with --out,
writes it to FILE."""
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
    import heat_peaks_twin as HT
    from globalegomocap_amd import prepare as P
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION, FisheyeCamera
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    n, rng = a.frames, np.random.default_rng(3)
    kp = BT.detect(BT.poses(n, 0.3, rng), cam, conf=0.8)
    eng = P._lift_engine(DEFAULT_CALIBRATION, torch.cuda.current_device())
    kp_d = torch.from_numpy(kp).to(eng.device)
    heat = eng.keypoint_heatmaps(kp_d, 1.5)
    depth = torch.full((n, 15), 0.5, dtype=torch.float64, device=eng.device)
    out = (torch.empty(n, 15, 3, dtype=torch.float64, device=eng.device), torch.empty(n, 15, dtype=torch.int32, device=eng.device))
    res = {"frames": n, "device": torch.cuda.get_device_name(0), "frame_bytes": int(heat[0].numel() * 4)}
    res["heatmap_peaks"] = event_ms(lambda: eng.heatmap_peaks(heat, out=out), a.launches)
    res["lift_skeleton"] = event_ms(lambda: eng.lift_skeleton(heat, depth), a.launches)
    res["ratio"] = round(res["heatmap_peaks"]["median_ms"] / res["lift_skeleton"]["median_ms"], 3)
    for k in ("heatmap_peaks", "lift_skeleton"):
        res[k]["GB_per_s"] = round(heat.numel() * 4 / (res[k]["median_ms"] * 1e-3) / 1e9, 1)
    one = tuple(t[:1] for t in out)
    res["one_frame"] = event_ms(lambda: eng.heatmap_peaks(heat[:1], out=one), a.launches)
    shifted = torch.empty(heat.numel() + 4, dtype=torch.float32, device=eng.device)[1:1 + heat.numel()].view(heat.shape)
    shifted.copy_(heat)
    res["generic"] = event_ms(lambda: eng.heatmap_peaks(shifted, out=out), a.launches)
    err = HT.pixel_error(eng.heatmap_peaks(heat)[0].cpu().numpy(), kp)
    res["accuracy"] = {"pixel_error_mean": round(float(err.mean()), 4), "pixel_error_max": round(float(err.max()), 4)}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
