#!/usr/bin/env python3
"""What a Motion-JPEG clip costs, for the 98-frame chunk of tools/render_bench.py with its three sequences
overlaid at 640 x 480, beside the PNG route for the same frames on the same card:

    python tools/video_bench.py [--frames 98] [--size 640x480] [--quality 90] [--dir DIR] [--repeats 5]

  kernels       gem_jpeg_encode alone on the chunk's rendered frames: per kernel the device time of one call from a `rocprofv3
                --kernel-trace` run of its own (this script starts itself under rocprofv3 with --kernels-only; no counters in that
                run), best of --repeats, with the VGPRs, scratch and LDS the trace reports; and the call between two HIP events
  write_video   `video.write_video` end to end (twice: the first call allocates the buffers), its laps -- render, encode (with the
                offsets' read-back), copy, file: time the main thread waited in each -- and the bytes per frame
  write_frames  the parent's route for the same frames: `render.write_frames(overview=False)`, PNG files

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from render_bench import engine, scenes, timed          # noqa: E402

KERNELS = ("jpeg_blocks_kernel", "jpeg_segments_kernel", "jpeg_offsets_kernel")


def rendered(e, frames, size):
    """The chunk's frames as scanlines on the device, and what drew them."""
    import torch
    from globalegomocap_amd import render as R
    lay = R.layout(*size)
    seqs, view, (geom, rgb, first), _ = scenes(e, frames, size)
    scan = torch.empty(frames, lay.stride, dtype=torch.uint8, device=e.device)
    e.render_capsules(geom, rgb, first, view, out=scan)
    return seqs, view, (geom, rgb, first), scan


def kernels_only(frames, size, quality, repeats):
    """`repeats` + 1 calls of gem_jpeg_encode and nothing else after the frames are drawn (run under rocprofv3)."""
    import torch
    e = engine()
    _, _, _, scan = rendered(e, frames, size)
    out = torch.empty(frames * e.jpeg_bound(*size) // 16, dtype=torch.uint8, device=e.device)
    offsets = torch.empty(frames + 1, dtype=torch.int64, device=e.device)
    for _ in range(repeats + 1):
        e.jpeg_encode_into(scan, size[0], size[1], quality, True, out, offsets)
    torch.cuda.synchronize()


def kernel_rows(frames, size, quality, repeats, work):
    """{kernel: {ms, launches_per_call, vgpr, scratch, lds}} from a rocprofv3 run of this script, or (None, reason)."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="video_prof_", dir=work)
    try:
        r = subprocess.run([exe, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--kernels-only", "--frames", str(frames), "--size", "%dx%d" % size, "--quality", str(quality),
                            "--repeats", str(repeats)], capture_output=True, text=True, timeout=600)
        if r.returncode:
            return None, "rocprofv3 run failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:])
        files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
        if not files:
            return None, "no kernel_trace.csv under %s" % d
        trace, out = list(csv.DictReader(open(files[0]))), {}
        for kernel in KERNELS:
            rows = sorted((row for row in trace if kernel in row["Kernel_Name"]), key=lambda row: int(row["Start_Timestamp"]))
            per = len(rows) // (repeats + 1)
            if per < 1 or len(rows) != per * (repeats + 1):
                return None, "%d %s launches in the trace for %d calls" % (len(rows), kernel, repeats + 1)
            ns = [int(row["End_Timestamp"]) - int(row["Start_Timestamp"]) for row in rows]
            calls = [sum(ns[c * per:(c + 1) * per]) for c in range(repeats + 1)]
            out[kernel] = {"ms": round(min(calls) * 1e-6, 4), "launches_per_call": per, "vgpr": int(rows[0].get("VGPR_Count", -1)),
                           "scratch": int(rows[0].get("Scratch_Size", -1)), "lds": int(rows[0].get("LDS_Block_Size", -1))}
        return out, None
    finally:
        shutil.rmtree(d, ignore_errors=True)


def measure(frames, size, quality, work, repeats):
    import torch
    from globalegomocap_amd import render as R, video as V
    W, H = size
    res = {"frames": frames, "size": "%dx%d" % size, "quality": quality, "sequences": 3}
    kt, why = kernel_rows(frames, size, quality, repeats, work)          # (first: before this process opens the device)
    res["kernels"] = why if kt is None else kt
    e = engine()
    lay = R.layout(W, H)
    seqs, view, (geom, rgb, first), scan = rendered(e, frames, size)
    res["scanline_mb"] = round(frames * lay.image_bytes / 1e6, 1)
    out = torch.empty(frames * e.jpeg_bound(W, H) // 16, dtype=torch.uint8, device=e.device)
    offsets = torch.empty(frames + 1, dtype=torch.int64, device=e.device)
    k = timed(lambda: e.jpeg_encode_into(scan, W, H, quality, True, out, offsets), repeats)
    total = int(offsets[-1])
    res.update(encode_call_ms=round(k * 1e3, 4), encode_mpixel_s=round(frames * W * H / k / 1e6, 1), clip_mb=round(total / 1e6, 3),
               bytes_per_frame=round(total / frames, 1), scanline_bytes_per_frame=lay.image_bytes,
               pcie_ratio=round(frames * lay.image_bytes / total, 1))
    if kt is not None:
        res["kernels_ms"] = round(sum(v["ms"] for v in kt.values()), 4)
    draw = lambda lo, n, o: e.render_capsules(geom, rgb, first[lo:lo + n + 1], view, out=o)          # noqa: E731
    runs = []
    for timings in (None, None, {}):          # (the first call allocates; the last is taken apart, which costs a wait per batch)
        d = tempfile.mkdtemp(prefix="video_total_", dir=work)
        try:
            torch.cuda.synchronize()
            t = time.perf_counter()
            assert V.write_video(e, draw, W, H, frames, os.path.join(d, "frames.avi"), 25, quality, timings=timings) == frames
            runs.append(time.perf_counter() - t)
            res["file_mb"] = round(os.path.getsize(os.path.join(d, "frames.avi")) / 1e6, 3)
            if timings is not None:
                res["laps_ms"] = {k: round(v * 1e3, 2) for k, v in timings.items()}
            assert len(V.read_avi(os.path.join(d, "frames.avi"))[3]) == frames
        finally:
            shutil.rmtree(d, ignore_errors=True)
    res.update(write_video_ms=[round(x * 1e3, 1) for x in runs], write_video_frames_s=round(frames / min(runs[:2]), 1))
    png = []
    for _ in range(2):
        d = tempfile.mkdtemp(prefix="video_png_", dir=work)
        try:
            torch.cuda.synchronize()
            t = time.perf_counter()
            assert R.write_frames(e, seqs, d, size=size, overview=False) == frames
            png.append(time.perf_counter() - t)
            res["png_mb"] = round(sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) / 1e6, 3)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    res.update(write_frames_ms=[round(x * 1e3, 1) for x in png], png_over_clip=round(min(png) / min(runs[:2]), 2))
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=98)
    p.add_argument("--size", default="640x480")
    p.add_argument("--quality", type=int, default=90)
    p.add_argument("--dir", default=None, help="where the temporary files go")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernels-only", action="store_true", help="(the run under rocprofv3)")
    a = p.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import render as R
    if a.kernels_only:
        kernels_only(a.frames, R._size(a.size), a.quality, a.repeats)
        return
    print(json.dumps(measure(a.frames, R._size(a.size), a.quality, a.dir, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
