#!/usr/bin/env python3
"""What bridging lost SLAM tracking costs, on synthetic walkers (`synth_walk`) with trajectory lines removed:

    python tools/slam_bridge_bench.py [--long 100000] [--repeats 7] [--launches 20] [--out profiles/slam_bridge_bench.json]

  table    walk(220, seed=3) with the lost ranges of the table in DESIGN.md 6o: device events around the two launches of gem_slam_bridge
           alone (everything uploaded before), device events around the enqueued `bridge_call` (one upload, two launches), the host
           clock around `bridge_cameras` (gap search, relative poses, upload, launches, record and origins back, synchronised) and
           around the host's `prepare.scaled_cameras` on the trajectory WITH all its lines, which is what the option replaces; the
           numpy twin (tests/bridge_twin.py) on the same input and the largest difference from it
  worst    one gap of 64 frames in 200 (the largest system the kernel takes)
  long     --long frames in chunks of 100 with a gap of 8 to 30 frames every 250 frames (400 systems)

Prints one JSON object and, with --out, writes it to FILE."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np          # noqa: E402

from ground_bench import FPS, event_ms, wall_ms          # noqa: E402


def launch_only(engine, poses, mask, systems, starts):
    """-> a function that launches gem_slam_bridge on tables that are on the device already."""
    import torch
    from globalegomocap_amd import _capi
    lib, n = engine.lib, len(mask)
    mask8 = np.ascontiguousarray(mask.astype(np.uint8))
    sys32 = np.ascontiguousarray(np.asarray(systems, dtype=np.int32).reshape(-1, 2))
    starts32 = np.ascontiguousarray(starts, dtype=np.int32)
    dev = lambda x: torch.from_numpy(x).to(engine.device)          # noqa: E731
    d_poses, d_mask, d_sys, d_starts = dev(np.ascontiguousarray(poses)), dev(mask8), dev(sys32), dev(starts32)
    need = int(lib.gem_slam_bridge_work(n))
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=engine.device)          # noqa: E731
    G, cams, origins, work, record = f64(n, 4, 4), f64(n, 4, 4), f64(len(starts32), 4, 4), f64(need // 8), f64(_capi.BRIDGE_RECORD_DOUBLES)
    bridged = torch.empty(n, dtype=torch.uint8, device=engine.device)

    def launch():
        _capi.check(lib.gem_slam_bridge(C.c_void_p(d_poses.data_ptr()), C.c_void_p(mask8.ctypes.data), C.c_void_p(d_mask.data_ptr()),
                                        C.c_void_p(sys32.ctypes.data), C.c_void_p(d_sys.data_ptr()), len(sys32), C.c_void_p(starts32.ctypes.data),
                                        C.c_void_p(d_starts.data_ptr()), len(starts32), n, C.c_void_p(G.data_ptr()), C.c_void_p(cams.data_ptr()),
                                        C.c_void_p(origins.data_ptr()), C.c_void_p(bridged.data_ptr()), C.c_void_p(work.data_ptr()), need,
                                        C.c_void_p(record.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)
    launch.keep = (d_poses, d_mask, d_sys, d_starts, G, cams, origins, work, record, bridged)
    return launch


def measure(engine, n, lost, size, a, twin=True):
    import bridge_twin as T
    from globalegomocap_amd import prepare, slam_bridge as B
    w, rows = T.walker_rows(n, seed=3, lost=lost)
    spans = [(s, min(s + size, n)) for s in range(0, n, size)]
    starts = [s for s, _ in spans]
    poses, mask = B.relative_rows(rows, 0, n, FPS, 1.0)
    systems = B.find_gaps(w["frame_ids"][mask], 0, n, 64)
    r = {"frames": n, "chunks": len(spans), "lost": int((~mask).sum()), "gaps": len(lost), "systems": len(systems)}
    r["kernels_device_ms"] = event_ms(launch_only(engine, poses, mask, systems, starts), a.launches)
    r["call_enqueued_device_ms"] = event_ms(lambda: B.bridge_call(engine.device, poses, mask, systems, starts), a.launches)
    r["bridge_cameras_wall_ms"] = wall_ms(lambda: B.bridge_cameras(engine, rows, spans, FPS, 1.0, 64 / FPS), a.repeats)
    r["host_scaled_cameras_of_the_whole_trajectory_wall_ms"] = wall_ms(lambda: prepare.scaled_cameras(w["rows"], spans, FPS, 1.0), a.repeats)
    cams, origins, report = B.bridge_cameras(engine, rows, spans, FPS, 1.0, 64 / FPS)
    r["report"] = {k: v for k, v in report.as_dict().items() if k != "gap_ids"}
    pos, rot = T.errors(np.concatenate([np.einsum("ij,njk->nik", o, c.cpu().numpy()) for o, c in zip(origins, cams)]), T.relative_truth(w),
                        np.flatnonzero(~mask))
    r["error_against_the_true_cameras"] = {"position_mean_m": float(pos.mean()), "position_max_m": float(pos.max()),
                                           "rotation_mean_deg": float(rot.mean()), "rotation_max_deg": float(rot.max())}
    if twin:
        t = time.perf_counter()
        e = T.bridge(poses, mask, starts)
        r["twin_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        r["largest_difference_to_twin"] = float(np.abs(np.concatenate([c.cpu().numpy() for c in cams]) - e["cams"]).max())
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--long", type=int, default=100000)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--out", default=None, metavar="FILE")
    a = p.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import prepare
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    engine = prepare._lift_engine(DEFAULT_CALIBRATION, 0)
    res = {"device": torch.cuda.get_device_name(0), "fps": FPS}
    long_lost = tuple((s, s + 8 + (7 * k) % 23) for k, s in enumerate(range(100, a.long - 100, 250)))
    cases = (("table [80,100)", 220, ((80, 100),), 100, True), ("table [60,68) + [130,160)", 220, ((60, 68), (130, 160)), 100, True),
             ("worst: one gap of 64 in 200", 200, ((70, 134),), 100, True), ("long", a.long, long_lost, 100, a.long <= 20000))
    for name, n, lost, size, twin in cases:
        res[name] = measure(engine, n, lost, size, a, twin)
        print("%s: %s" % (name, json.dumps(res[name])), file=sys.stderr, flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
