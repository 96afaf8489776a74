#!/usr/bin/env python3
"""What estimating the SLAM scale costs, on synthetic walkers (`synth_walk`, 3 cm noise) of 2 000 and 100 000 frames
in chunks of 100:

    python tools/slam_scale_bench.py [--frames 2000 100000] [--repeats 7] [--launches 20] [--work DIR] [--out profiles/slam_scale_bench.json]

  kernels          the device time of each of gem_slam_scale's six kernels, from a `rocprofv3 --kernel-trace --stats` run of its own:
                   this script starts itself under rocprofv3 with --kernels-only (mean over --launches calls after a warm-up call)
  call             device events around one call that is only enqueued (the one upload of table, ids and poses + the six kernels), and
                   the host clock around `estimate_scale` (upload, kernels, the record back, synchronised)
  twin             the numpy twin (tests/slam_scale_twin.py) on the same input, one CPU thread's worth of numpy
  prepare          host-inclusive, synchronised, --prepare-frames frames of .mat files (page cache warm): `prepare.prepare_sequence` with
                   the number against scale="auto", alternating; and the same for `detections.recording_from_detections`

Prints one JSON object and, with --out, writes it to FILE."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np          # noqa: E402

KERNELS = ("scale_feet_kernel", "scale_pairs_kernel", "scale_ref_kernel", "scale_cost_kernel", "scale_argmin_kernel", "scale_fit_kernel")
SCALE, FPS, CHUNK = 1.7, 25, 100


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "repeats": len(ms)}


def walker(n):
    from globalegomocap_amd import synth_walk as W
    w = W.walk(n, scale=SCALE, fps=FPS, noise=0.03, seed=11)
    R, c = W.slam_inputs(w)
    return w, R, c


def device_chunks(w):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(w["local"])).to("cuda")
    return [x[lo:lo + CHUNK] for lo in range(0, len(x), CHUNK)]


def kernels_only(n, launches):
    """launches + 1 calls of gem_slam_scale and nothing else (run under rocprofv3)."""
    import torch
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import slam_scale as S
    w, R, c = walker(n)
    chunks = device_chunks(w)
    for _ in range(launches + 1):
        rc, _, _, msg = S.scale_call(chunks, R, c, w["frame_ids"], S.default_lag(FPS), read_back=False)
        assert rc == 0, msg
    torch.cuda.synchronize()


def kernel_times(n, launches, work):
    """Mean device time per call of every kernel, microseconds, from a rocprofv3 run of this script; or why there is none."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="scale_prof_", dir=work)
    try:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--kernels-only", str(n), "--launches", str(launches)], capture_output=True, text=True, timeout=900)
        if r.returncode:
            return "rocprofv3 run failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:])
        files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        if not files:
            return "no kernel_stats.csv under %s" % d
        out = {}
        for row in csv.DictReader(open(files[0])):
            for k in KERNELS:
                if k in row["Name"]:
                    assert int(row["Calls"]) == launches + 1, (k, row["Calls"])
                    out[k] = {"mean_us": round(float(row["TotalDurationNs"]) / int(row["Calls"]) * 1e-3, 2), "min_us": round(float(row["MinNs"]) * 1e-3, 2),
                              "max_us": round(float(row["MaxNs"]) * 1e-3, 2)}
        out["sum_of_means_us"] = round(sum(v["mean_us"] for v in out.values()), 2)
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


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


def wall_ms(fn, repeats, sync=True):
    import torch
    fn()
    out = []
    for _ in range(repeats):
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return spread(out)


def alternating_ms(fns, repeats):
    """{name: spread}: the functions in turn, `repeats` rounds after one warm-up round, synchronised."""
    import torch
    for f in fns.values():
        f()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t) * 1e3)
    return {k: spread(v) for k, v in out.items()}


def write_mat_recording(work, w, n):
    """The walker's first n frames in the pose network's file format: paraboloid heat-maps at the projected joints, its depths."""
    from globalegomocap_amd import synth, synth_recording as SR
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    ix, iy = synth.heatmap_coords(cam.project_numpy(w["local"][:n].reshape(-1, 3)).reshape(n, 15, 2))
    centres = np.floor(np.stack([ix, iy], -1)) + np.array([0.3, 0.2])
    paths = None
    for lo in range(0, n, 200):
        hi = min(n, lo + 200)
        heat = SR.paraboloid_heatmaps(centres[lo:hi], np.full((hi - lo, 15), 5.0))
        paths = SR.write_recording(work, heat, w["depth"][lo:hi], ["frame_%05d.mat" % k for k in range(lo, hi)], None, None,
                                   w["rows"][:n] if hi == n else None, None)
    for d in paths[:2]:                                       # page cache warm
        for f in os.listdir(d):
            with open(os.path.join(d, f), "rb") as fh:
                fh.read()
    return paths


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, nargs="+", default=[2000, 100000])
    p.add_argument("--prepare-frames", type=int, default=2000)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--work", default=None, help="directory for the synthetic recording and the profiler's files (default: a temporary one)")
    p.add_argument("--out", default=None, metavar="FILE")
    p.add_argument("--kernels-only", type=int, default=None, metavar="FRAMES", help="(the run under rocprofv3)")
    a = p.parse_args()
    if a.kernels_only is not None:
        kernels_only(a.kernels_only, a.launches)
        return
    work = a.work or tempfile.mkdtemp(prefix="gem_scale_bench_")
    os.makedirs(work, exist_ok=True)
    res = {"scale": SCALE, "fps": FPS, "chunk_frames": CHUNK, "noise_m": 0.03, "sizes": {}}
    try:
        # ---- the kernels, each size in a profiler run of its own (before this process opens the device)
        for n in a.frames:
            res["sizes"][str(n)] = {"kernels": kernel_times(n, a.launches, work)}
            print("kernels %d: %s" % (n, json.dumps(res["sizes"][str(n)]["kernels"])), file=sys.stderr, flush=True)
        import torch
        import __graft_entry__ as ge
        ge.build()
        import slam_scale_twin as T
        from globalegomocap_amd import detections as D, prepare as P, slam_scale as S
        res["device"] = torch.cuda.get_device_name(0)
        lag = S.default_lag(FPS)
        walkers = {}
        for n in a.frames:
            w, R, c = walkers[n] = walker(n)
            chunks = device_chunks(w)
            spans = [(lo, min(lo + CHUNK, n)) for lo in range(0, n, CHUNK)]
            r = res["sizes"][str(n)]
            r["call_enqueued_device_ms"] = event_ms(lambda: S.scale_call(chunks, R, c, w["frame_ids"], lag, read_back=False), a.launches)
            r["estimate_scale_wall_ms"] = wall_ms(lambda: S.estimate_scale(chunks, w["rows"], spans, FPS), a.repeats)
            r["of_it_selected_poses_host_ms"] = wall_ms(lambda: S.selected_poses(w["rows"], spans, FPS), a.repeats, sync=False)
            est = S.estimate_scale(chunks, w["rows"], spans, FPS)
            cuts = [0] + [b for _, b in spans]
            t = time.perf_counter()
            twin = T.estimate(w["local"], R, c, w["frame_ids"], lag, chunk_starts=cuts)
            r["twin_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            r["estimate"] = est.as_dict()
            del r["estimate"]["per_chunk"]
            r["per_chunk_min_max"] = [float(np.nanmin(est.per_chunk)), float(np.nanmax(est.per_chunk))]
            r["relative_error"] = abs(est.scale / SCALE - 1)
            r["relative_difference_to_twin"] = abs(est.scale / twin["scale"] - 1)
            r["candidate_pair_evaluations"] = est.pairs * 513
            print("%d: %s" % (n, json.dumps(r)), file=sys.stderr, flush=True)
            del chunks
        # ---- what scale="auto" adds to prepare and to the detection route, host-inclusive
        n = a.prepare_frames          # (n + 1 frames: `chunk_spans` drops the last chunk of a span that is a multiple of the chunk size)
        w, end = walker(n + 1)[0], n + 1
        hd, dd, traj, _ = write_mat_recording(os.path.join(work, "mat"), w, end)
        mat = alternating_ms({"number": lambda: P.prepare_sequence(traj, hd, dd, None, 0, end, fps=FPS, test_size=CHUNK, verbose=False, scale=SCALE),
                              "auto": lambda: P.prepare_sequence(traj, hd, dd, None, 0, end, fps=FPS, test_size=CHUNK, verbose=False, scale="auto")},
                             a.repeats)
        mat["added_ms"] = round(mat["auto"]["median_ms"] - mat["number"]["median_ms"], 3)
        from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
        cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
        m = len(P.chunk_spans(0, end, CHUNK)) * CHUNK
        kp = np.concatenate([cam.project_numpy(w["local"][:m].reshape(-1, 3)).reshape(m, 15, 2), np.ones((m, 15, 1))], axis=2)
        det = {"keypoints": kp, "depth": w["depth"][:m]}
        spans = P.chunk_spans(0, end, CHUNK)
        dets = alternating_ms({"number": lambda: D.recording_from_detections(traj, det, None, SCALE, spans, FPS),
                               "auto": lambda: D.recording_from_detections(traj, det, None, "auto", spans, FPS)}, a.repeats)
        dets["added_ms"] = round(dets["auto"]["median_ms"] - dets["number"]["median_ms"], 3)
        res["prepare"] = {"frames": m, "mat_files": mat, "detections": dets}
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
