#!/usr/bin/env python3
"""What the skeleton meshes of `--save` cost, for one 100-frame chunk (its three sequences: 300 frames) and
for 20 chunks (6000 frames):

    python tools/mesh_bench.py [--chunks 1 20] [--dir DIR] [--twin-frames 320]

  kernel   the device time of gem_skeleton_mesh's launches and the store bandwidth they reach (vertex-block bytes / time), from a
           `rocprofv3 --kernel-trace --stats` run of its own: this script starts itself under rocprofv3 with --kernels-only
  d2h      the vertex blocks' copies device -> pinned memory (HIP events), in `meshes.write_meshes`' batches
  files    the writer pool writing the files from pinned memory that is already filled (no device involved)
  total    `meshes.write_meshes`, all of it: kernel, copies and files pipelined
  twin     the numpy twin (tests/mesh_twin.py) building the same frames' vertices on 16 host processes, measured on --twin-frames
           frames and scaled to the frame count; the only comparison there is (open3d is not available)

Prints one JSON line per configuration.  The files go to a temporary directory under --dir (default: the system's) and are removed.
"""
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

FRAMES_PER_CHUNK, SEQUENCES = 100, 3


def poses(n):
    from globalegomocap_amd import synth
    rng = np.random.default_rng(7)
    return synth.make_motion(n, rng) + np.array([0.3, 1.2, -0.4])


def engine():
    import torch
    from globalegomocap_amd import prepare
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    return prepare._lift_engine(DEFAULT_CALIBRATION, torch.cuda.current_device())


def batches(n):
    from globalegomocap_amd import meshes
    per = max(1, meshes.PINNED_BYTES // meshes.layout().vertex_bytes)
    return [(lo, min(per, n - lo)) for lo in range(0, n, per)]


def kernels_only(n, repeats):
    """The launches `write_meshes` would make for n frames, `repeats` times, and nothing else (run under rocprofv3)."""
    import torch
    from globalegomocap_amd import meshes
    e = engine()
    seq = torch.from_numpy(poses(n)).to(e.device)
    out = torch.empty(max(b for _, b in batches(n)), meshes.layout().vertex_bytes, dtype=torch.uint8, device=e.device)
    for _ in range(repeats + 1):          # (the first round also uploads the template table)
        for lo, b in batches(n):
            e.skeleton_mesh(seq[lo:lo + b], None, out=out[:b])
    torch.cuda.synchronize()


def kernel_time(n, repeats, work):
    """Mean device time of one round of launches, from a rocprofv3 run of this script; None when rocprofv3 is not there."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="mesh_prof_", dir=work)
    try:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--kernels-only", str(n), "--repeats", str(repeats)], capture_output=True, text=True, timeout=600)
        if r.returncode:
            return None, "rocprofv3 run failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:])
        files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        if not files:
            return None, "no kernel_stats.csv under %s" % d
        for row in csv.DictReader(open(files[0])):
            if "skeleton_mesh_" in row["Name"]:          # (the vertex-block kernel)
                rounds = repeats + 1
                calls = int(row["Calls"])
                assert calls == rounds * len(batches(n)), (calls, rounds, len(batches(n)))
                return float(row["TotalDurationNs"]) / rounds * 1e-9, {"launches_per_round": calls // rounds, "min_ns": float(row["MinNs"]),
                                                                       "max_ns": float(row["MaxNs"])}
        return None, "no skeleton_mesh kernel in the stats"
    finally:
        shutil.rmtree(d, ignore_errors=True)


def twin_frames(chunk):
    import mesh_twin as T
    return sum(T.frame_mesh(p)[0].shape[0] for p in chunk)


def twin_time(seq, n_measured):
    from concurrent.futures import ProcessPoolExecutor
    n_measured = min(n_measured, len(seq))
    parts = [seq[i:n_measured:16] for i in range(16)]
    import multiprocessing
    with ProcessPoolExecutor(max_workers=16, mp_context=multiprocessing.get_context("spawn")) as pool:          # fresh processes
        list(pool.map(twin_frames, [p[:1] for p in parts if len(p)]))          # (the workers are up and have imported numpy)
        t = time.perf_counter()
        list(pool.map(twin_frames, [p for p in parts if len(p)]))
        dt = time.perf_counter() - t
    return dt, n_measured


def measure(n_chunks, work, n_twin, repeats):
    import torch
    from globalegomocap_amd import meshes
    from globalegomocap_amd.staging import cpus_near, reader_pool
    n = n_chunks * FRAMES_PER_CHUNK * SEQUENCES
    lay = meshes.layout()
    res = {"chunks": n_chunks, "frames": n, "vertex_block_mb": round(n * lay.vertex_bytes / 1e6, 1), "file_mb": round(n * lay.file_bytes / 1e6, 1)}
    seq_h = poses(n)
    tw, m = twin_time(seq_h, n_twin)          # (first: before this process opens the device)
    k, info = kernel_time(n, repeats, work)
    if k is None:
        res["kernel"] = info
    else:
        res.update(kernel_ms=round(k * 1e3, 4), kernel_store_gb_s=round(n * lay.vertex_bytes / k / 1e9, 1), kernel_info=info)
    e = engine()
    seq = torch.from_numpy(seq_h).to(e.device)
    # device -> pinned memory, batch by batch
    per = max(b for _, b in batches(n))
    dev = torch.empty(per, lay.vertex_bytes, dtype=torch.uint8, device=e.device)
    pin = torch.empty(per, lay.vertex_bytes, dtype=torch.uint8).pin_memory()
    best = None
    for _ in range(3):
        total = 0.0
        for lo, b in batches(n):
            e.skeleton_mesh(seq[lo:lo + b], None, out=dev[:b])
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            pin[:b].copy_(dev[:b], non_blocking=True)
            z.record()
            z.synchronize()
            total += a.elapsed_time(z) * 1e-3
        best = total if best is None else min(best, total)
    res.update(d2h_ms=round(best * 1e3, 3), d2h_gb_s=round(n * lay.vertex_bytes / best / 1e9, 1))
    # the files from pinned memory that is already filled (the last batch's blocks stand in for every batch's)
    header, faces = meshes.constant()
    pool = reader_pool("mesh", min(meshes.MAX_WRITERS, os.cpu_count() or 1), cpus_near(e.device))
    d = tempfile.mkdtemp(prefix="mesh_files_", dir=work)
    try:
        rows = pin.numpy()
        t = time.perf_counter()
        futures = [pool.submit(meshes._write_file, os.path.join(d, "out_%04d.ply" % f), (header, rows[f % per], faces)) for f in range(n)]
        for f in futures:
            f.result()
        dt = time.perf_counter() - t
        res.update(files_ms=round(dt * 1e3, 1), files_gb_s=round(n * lay.file_bytes / dt / 1e9, 2))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    # all of it, pipelined (twice: the first call also allocates the pinned buffers)
    totals = []
    for _ in range(2):
        d = tempfile.mkdtemp(prefix="mesh_total_", dir=work)
        try:
            torch.cuda.synchronize()
            t = time.perf_counter()
            meshes.write_meshes(e, seq, d)
            totals.append(time.perf_counter() - t)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    res.update(total_ms=[round(x * 1e3, 1) for x in totals], total_frames_per_s=round(n / min(totals), 1))
    res.update(twin_frames_measured=m, twin_ms_measured=round(tw * 1e3, 1), twin_ms_scaled_to_all_frames=round(tw * 1e3 * n / m, 1),
               twin_note="16 processes, vertices only (no file is written)")
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--chunks", type=int, nargs="+", default=[1, 20])
    p.add_argument("--dir", default=None, help="where the temporary files go")
    p.add_argument("--twin-frames", type=int, default=320)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernels-only", type=int, default=None, metavar="FRAMES", help="(the run under rocprofv3)")
    a = p.parse_args()
    import __graft_entry__ as ge
    ge.build()
    if a.kernels_only is not None:
        kernels_only(a.kernels_only, a.repeats)
        return
    for c in a.chunks:
        print(json.dumps(measure(c, a.dir, a.twin_frames, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
