#!/usr/bin/env python3
"""What following a drifting SLAM scale costs, on synthetic walkers (`synth_walk`, 3 cm noise) of 2 000 and
100 000 frames whose trajectory's scale runs from 0.8 to 1.1, knots 10 s apart:

    python tools/slam_drift_bench.py [--frames 2000 100000] [--repeats 7] [--launches 20] [--out profiles/slam_drift_bench.json]

  call             device events around one call that is only enqueued (the one upload of table, ids and poses + the kernels), for
                   gem_slam_drift and, beside it, for gem_slam_scale, whose six kernels are its first six
  estimate         the host clock around `estimate_drift` and `estimate_scale` (upload, kernels, the records back, synchronised)
  twin             the numpy twin (tests/slam_drift_twin.py) on the same input
  accuracy         the worst error in distance from the start, metres, of the metric track and of the trajectory at the one scale

Prints one JSON object and, with --out, writes it to FILE."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np          # noqa: E402

FPS, CHUNK = 25, 100


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, nargs="+", default=[2000, 100000])
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--out", default=None, metavar="FILE")
    a = p.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    import slam_drift_twin as D
    from globalegomocap_amd import slam_scale as S, synth_walk as W
    from slam_scale_bench import event_ms, wall_ms
    lag, knot = S.default_lag(FPS), S.default_knot(FPS)
    res = {"fps": FPS, "chunk_frames": CHUNK, "noise_m": 0.03, "scale": [0.8, 1.1], "knot_frames": knot, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in a.frames:
        w = W.walk(n, scale=0.8 + 0.3 * np.arange(n) / n, fps=FPS, noise=0.03, seed=11)
        R, c = W.slam_inputs(w)
        ids = w["frame_ids"]
        x = torch.from_numpy(np.ascontiguousarray(w["local"])).to("cuda")
        chunks = [x[lo:lo + CHUNK] for lo in range(0, n, CHUNK)]
        spans = [(lo, min(lo + CHUNK, n)) for lo in range(0, n, CHUNK)]
        r = res["sizes"][str(n)] = {}
        r["drift_call_enqueued_device_ms"] = event_ms(lambda: S.drift_call(chunks, R, c, ids, lag, knot, read_back=False), a.launches)
        r["scale_call_enqueued_device_ms"] = event_ms(lambda: S.scale_call(chunks, R, c, ids, lag, read_back=False), a.launches)
        r["estimate_drift_wall_ms"] = wall_ms(lambda: S.estimate_drift(chunks, w["rows"], spans, FPS), a.repeats)
        r["estimate_scale_wall_ms"] = wall_ms(lambda: S.estimate_scale(chunks, w["rows"], spans, FPS), a.repeats)
        est = S.estimate_drift(chunks, w["rows"], spans, FPS)
        t = time.perf_counter()
        twin = D.estimate(w["local"], R, c, ids, lag, knot)
        r["twin_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        true = np.linalg.norm(w["head"] - w["head"][0], axis=1)
        r["knots"] = est.n_knots
        r["curve"] = [est.scale_min, est.scale_max, est.scale_mean]
        r["one_scale"] = est.global_estimate.scale
        r["worst_error_m"] = {"curve": float(np.abs(np.linalg.norm(est.metric, axis=1) - true).max()),
                              "one_scale": float(np.abs(np.linalg.norm(est.global_estimate.scale * c, axis=1) - true).max())}
        r["knots_relative_difference_to_twin"] = float(np.max(np.abs(est.knot_scale / twin["knot_scale"] - 1)))
        r["path_m"] = est.metric_length
        print("%d: %s" % (n, json.dumps(r)), file=sys.stderr, flush=True)
        del chunks, x
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
