#!/usr/bin/env python3
"""What the rendered frames of `--render` cost, for one 98-frame chunk with its three sequences overlaid at
640 x 480, beside the skeleton meshes of `--save` for the same chunk on the same card:

    python tools/render_bench.py [--frames 98] [--size 640x480] [--dir DIR] [--repeats 5]

  kernel_frames    gem_render_capsules for the chunk's per-frame images (90 capsules each): the kernel's device time from a
                   `rocprofv3 --kernel-trace --stats` run of its own (this script starts itself under rocprofv3 with --kernels-only),
                   and the call between two HIP events (that includes the call's read-back of `first` and its wait), best of
                   --repeats; the store bandwidth is scanline bytes / kernel time
  kernel_overview  the same for ONE overview image of one sequence (frames x 30 capsules: 2 940 for 98 frames): where the culling matters
  d2h              the scanlines' copies device -> pinned memory (HIP events)
  deflate          the writer pool deflating and writing the files from pinned memory that is already filled (no device involved),
                   and, apart, zlib alone on one thread per image
  total            `render.write_frames`, all of it: kernels, copies, deflate and files pipelined (frames + three overviews)
  meshes           `meshes.write_result_meshes` for the same three sequences (3 x frames PLY files)

Prints one JSON line.  The files go to a temporary directory under --dir (default: the system's) and are removed.
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
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402


def poses(n, seed):
    from globalegomocap_amd import synth
    rng = np.random.default_rng(seed)
    return synth.make_motion(n, rng) + np.array([0.3, 1.2, -0.4])


def engine():
    import torch
    from globalegomocap_amd import prepare
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    return prepare._lift_engine(DEFAULT_CALIBRATION, torch.cuda.current_device())


def timed(fn, repeats):
    """Best device time (s) of fn() between two events on the current stream."""
    import torch
    best = None
    for _ in range(repeats + 1):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        z.record()
        z.synchronize()
        t = a.elapsed_time(z) * 1e-3
        best = t if best is None else min(best, t)
    return best


def scenes(e, frames, size):
    """The chunk's per-frame scene and one sequence's overview scene, the view, and the sequences."""
    from globalegomocap_amd import render as R
    seqs = [poses(frames, 7), poses(frames, 8), poses(frames, 9)]
    colours = list(R.PALETTE.values())
    view = R.frames_view(e, seqs, size=size)
    d_seqs, crts = R._prepare(e, seqs, None)
    return seqs, view, R._scene(e, d_seqs, crts, colours, False), R._scene(e, d_seqs[:1], crts[:1], colours[:1], True)


def kernels_only(frames, size, repeats):
    """`repeats` + 1 launches for the frames, then as many for the overview, and nothing else (run under rocprofv3)."""
    import torch
    from globalegomocap_amd import render as R
    e = engine()
    lay = R.layout(*size)
    _, view, per_frame, overview = scenes(e, frames, size)
    out = torch.empty(frames, lay.stride, dtype=torch.uint8, device=e.device)
    for scene in (per_frame, overview):
        for _ in range(repeats + 1):
            e.render_capsules(*scene, view, out=out[:scene[2].numel() - 1])
    torch.cuda.synchronize()


def kernel_times(frames, size, repeats, work, script=None, kernels=("render_capsules_kernel",), groups=2):
    """(frames launch, overview launch) best device times in seconds from a rocprofv3 run of this script, or (None, reason).
    `script`: a sibling tool (tools/camera_view_bench.py) that under --kernels-only launches each of `kernels` groups * (repeats + 1)
    times; the best time of every group of every kernel, in that order."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="render_prof_", dir=work)
    try:
        r = subprocess.run([exe, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, script or os.path.abspath(__file__),
                            "--kernels-only", "--frames", str(frames), "--size", "%dx%d" % size, "--repeats", str(repeats)],
                           capture_output=True, text=True, timeout=600)
        if r.returncode:
            return None, "rocprofv3 run failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:])
        files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
        if not files:
            return None, "no kernel_trace.csv under %s" % d
        trace, best = list(csv.DictReader(open(files[0]))), []
        for kernel in kernels:
            rows = [row for row in trace if kernel in row["Kernel_Name"]]
            rows.sort(key=lambda row: int(row["Start_Timestamp"]))
            if len(rows) != groups * (repeats + 1):
                return None, "%d %s launches in the trace, expected %d" % (len(rows), kernel, groups * (repeats + 1))
            ns = [int(row["End_Timestamp"]) - int(row["Start_Timestamp"]) for row in rows]
            best += [min(ns[g * (repeats + 1):(g + 1) * (repeats + 1)]) * 1e-9 for g in range(groups)]
        return tuple(best), None
    finally:
        shutil.rmtree(d, ignore_errors=True)


def measure(frames, size, work, repeats):
    import torch
    from globalegomocap_amd import meshes, render as R
    from globalegomocap_amd.staging import cpus_near, reader_pool
    e = engine()
    W, H = size
    lay = R.layout(W, H)
    res = {"frames": frames, "size": "%dx%d" % size, "sequences": 3, "image_kb": round(lay.image_bytes / 1e3, 1),
           "scanline_mb": round(frames * lay.image_bytes / 1e6, 1)}
    kt, why = kernel_times(frames, size, repeats, work)          # (first: before this process opens the device)
    seqs, view, (geom, rgb, first), (og, orgb, ofirst) = scenes(e, frames, size)
    if kt is None:
        res["kernel"] = why
    else:
        res.update(kernel_frames_ms=round(kt[0] * 1e3, 4), kernel_frames_store_gb_s=round(frames * lay.image_bytes / kt[0] / 1e9, 1),
                   kernel_frames_mpixel_s=round(frames * W * H / kt[0] / 1e6, 1), kernel_overview_ms=round(kt[1] * 1e3, 4))
    out = torch.empty(frames, lay.stride, dtype=torch.uint8, device=e.device)
    k = timed(lambda: e.render_capsules(geom, rgb, first, view, out=out), repeats)
    res.update(call_frames_ms=round(k * 1e3, 4), capsules_per_frame_image=90)
    one = torch.empty(1, lay.stride, dtype=torch.uint8, device=e.device)
    k = timed(lambda: e.render_capsules(og, orgb, ofirst, view, out=one), repeats)
    res.update(call_overview_ms=round(k * 1e3, 4), capsules_in_overview=int(og.shape[0]))
    res["bytes_not_white"] = round(float((out[:, :lay.image_bytes] != 255).float().mean()), 4)          # (something was drawn)
    # device -> pinned memory
    pin = torch.empty(frames, lay.stride, dtype=torch.uint8).pin_memory()
    k = timed(lambda: pin.copy_(out, non_blocking=True), repeats)
    res.update(d2h_ms=round(k * 1e3, 3), d2h_gb_s=round(frames * lay.stride / k / 1e9, 1))
    # deflate alone, one thread
    rows = pin.numpy()
    t = time.perf_counter()
    packed = [len(zlib.compress(rows[f, :lay.image_bytes], 1)) for f in range(frames)]
    dt = time.perf_counter() - t
    res.update(zlib_one_thread_ms_per_image=round(dt * 1e3 / frames, 3), png_kb_mean=round(float(np.mean(packed)) / 1e3, 1))
    # the writer pool from filled pinned memory
    pool = reader_pool("mesh", min(R.MAX_WRITERS, os.cpu_count() or 1), cpus_near(e.device))
    d = tempfile.mkdtemp(prefix="render_files_", dir=work)
    try:
        t = time.perf_counter()
        futures = [pool.submit(R.write_png, os.path.join(d, "frame_%04d.png" % f), rows[f, :lay.image_bytes], W, H) for f in range(frames)]
        for f in futures:
            f.result()
        dt = time.perf_counter() - t
        res.update(deflate_and_files_ms=round(dt * 1e3, 1), deflate_and_files_images_s=round(frames / dt, 1))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    # all of it, pipelined (twice: the first call also allocates the pinned buffers); then the meshes of the same chunk
    totals, mesh_totals = [], []
    for _ in range(2):
        d = tempfile.mkdtemp(prefix="render_total_", dir=work)
        try:
            torch.cuda.synchronize()
            t = time.perf_counter()
            n = R.write_frames(e, seqs, d, size=size)
            totals.append(time.perf_counter() - t)
            assert n == frames + 3
        finally:
            shutil.rmtree(d, ignore_errors=True)
    for _ in range(2):
        d = tempfile.mkdtemp(prefix="render_meshes_", dir=work)
        try:
            torch.cuda.synchronize()
            t = time.perf_counter()
            n = meshes.write_result_meshes(e, d, seqs[0], seqs[1], seqs[2], align=False)
            mesh_totals.append(time.perf_counter() - t)
            assert n == 3 * frames
        finally:
            shutil.rmtree(d, ignore_errors=True)
    res.update(write_frames_ms=[round(x * 1e3, 1) for x in totals], write_frames_images_s=round((frames + 3) / min(totals), 1),
               write_meshes_ms=[round(x * 1e3, 1) for x in mesh_totals], mesh_file_mb=round(3 * frames * meshes.layout().file_bytes / 1e6, 1))
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=98)
    p.add_argument("--size", default="640x480")
    p.add_argument("--dir", default=None, help="where the temporary files go")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernels-only", action="store_true", help="(the run under rocprofv3)")
    a = p.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import render as R
    if a.kernels_only:
        kernels_only(a.frames, R._size(a.size), a.repeats)
        return
    print(json.dumps(measure(a.frames, R._size(a.size), a.dir, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
