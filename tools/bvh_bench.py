#!/usr/bin/env python3
"""What BVH export costs, for a resident sequence of 2 000 and of 100 000 frames:

    python tools/bvh_bench.py [--frames 2000 100000] [--dir DIR] [--twin-frames 640] [--repeats 7] [--out FILE]

  rest / channels / text   the device time of the three launches (gem_bvh_rest, gem_bvh_channels, gem_format_fields over the whole
                           motion block), each between two device events, after a warm-up: median, minimum and maximum of --repeats
  d2h                      the motion block's text device -> pinned memory in `write_bvh`'s slices (events)
  file                     the text written to a file from pinned memory that is already filled (no device involved)
  write_bvh                all of it, to a file under --dir: upload-free (the sequence is resident), rest lengths read back, header,
                           slices formatted, copied and appended
  twin                     the host route: the numpy twin's channels (tests/bvh_twin.py) and Python's "%15.6f" for the same frames on
                           16 processes, measured on --twin-frames frames and scaled to the frame count

Prints one JSON line per frame count and, with --out, writes them to FILE as a JSON list."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np          # noqa: E402


def poses(n):
    """n frames of smooth synthetic motion under a slowly turning, moving body: [n,15,3]."""
    from globalegomocap_amd import synth
    rng = np.random.default_rng(7)
    base = synth.make_motion(min(n, 2000), rng)
    seq = np.concatenate([base] * (-(-n // len(base))))[:n]
    a = np.linspace(0.0, 6.0, n)
    R = np.stack([np.stack([np.cos(a), np.zeros(n), np.sin(a)], -1), np.stack([np.zeros(n), np.ones(n), np.zeros(n)], -1),
                  np.stack([-np.sin(a), np.zeros(n), np.cos(a)], -1)], -2)
    return np.einsum("nij,nkj->nki", R, seq) + np.stack([np.sin(a), 1.0 + 0.0 * a, np.cos(a)], -1)[:, None]


def twin_text(chunk):
    import bvh_twin as T
    return len(T.format_fields(T.channels(chunk, unit_scale=100.0), T.CHANNELS))


def twin_time(seq, n_measured):
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    n_measured = min(n_measured, len(seq))
    parts = [p for p in (seq[i:n_measured:16] for i in range(16)) if len(p)]
    with ProcessPoolExecutor(max_workers=16, mp_context=multiprocessing.get_context("spawn")) as pool:          # fresh processes
        list(pool.map(twin_text, [p[:1] for p in parts]))          # (the workers are up and have imported numpy)
        t = time.perf_counter()
        list(pool.map(twin_text, parts))
        return time.perf_counter() - t, n_measured


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def timed(fn, repeats):
    import torch
    fn()
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        z.record()
        z.synchronize()
        out.append(a.elapsed_time(z))
    return stats(out)


def measure(n, work, n_twin, repeats):
    import torch
    from globalegomocap_amd import bvh, prepare
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    lay = bvh.layout()
    res = {"frames": n, "numbers": n * lay.channels, "text_mb": round(n * lay.frame_bytes / 1e6, 2)}
    seq_h = poses(n)
    tw, m = twin_time(seq_h, n_twin)          # (first: before this process opens the device)
    e = prepare._lift_engine(DEFAULT_CALIBRATION, torch.cuda.current_device())
    seq = torch.from_numpy(seq_h).to(e.device)
    rest = bvh.rest_lengths(e, seq)
    chan = bvh.channels(e, seq, None, rest)
    text = torch.empty(n * lay.frame_bytes, dtype=torch.uint8, device=e.device)
    bad = bvh.new_counter(e.device)
    res["rest"] = timed(lambda: bvh.rest_lengths(e, seq), repeats)
    res["channels"] = timed(lambda: bvh.channels(e, seq, None, rest), repeats)
    res["text"] = timed(lambda: bvh.format_fields(e, chan, lay.channels, bad, out=text), repeats)
    res["text"]["store_gb_s"] = round(n * lay.frame_bytes / res["text"]["median_ms"] / 1e6, 1)
    assert bad.cpu().tolist() == [0, -1]
    per = max(1, bvh.PINNED_BYTES // lay.frame_bytes)
    pin = torch.empty(min(per, n) * lay.frame_bytes, dtype=torch.uint8).pin_memory()

    def copies():
        for lo in range(0, n, per):
            b = min(per, n - lo) * lay.frame_bytes
            pin[:b].copy_(text[lo * lay.frame_bytes:lo * lay.frame_bytes + b], non_blocking=True)
    res["d2h"] = timed(copies, repeats)
    res["d2h"]["gb_s"] = round(n * lay.frame_bytes / res["d2h"]["median_ms"] / 1e6, 1)
    d = tempfile.mkdtemp(prefix="bvh_bench_", dir=work)
    try:
        rows, files, totals = pin.numpy(), [], []
        for _ in range(repeats):
            t = time.perf_counter()
            with open(os.path.join(d, "text.bin"), "wb") as f:
                for lo in range(0, n, per):
                    f.write(rows[:min(per, n - lo) * lay.frame_bytes])
            files.append((time.perf_counter() - t) * 1e3)
        res["file"] = stats(files)
        res["file"]["gb_s"] = round(n * lay.frame_bytes / res["file"]["median_ms"] / 1e6, 2)
        bvh.write_bvh(e, seq, os.path.join(d, "seq.bvh"))          # (allocates the pinned buffers)
        for _ in range(repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            bvh.write_bvh(e, seq, os.path.join(d, "seq.bvh"))
            totals.append((time.perf_counter() - t) * 1e3)
        res["write_bvh"] = stats(totals)
        res["write_bvh"]["frames_per_s"] = round(n / res["write_bvh"]["median_ms"] * 1e3)
        res["file_bytes"] = os.path.getsize(os.path.join(d, "seq.bvh"))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res["twin"] = {"frames_measured": m, "ms_measured": round(tw * 1e3, 1), "ms_scaled_to_all_frames": round(tw * 1e3 * n / m, 1),
                   "note": "16 processes: numpy channels and Python's %15.6f, no file is written"}
    bvh.release()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, nargs="+", default=[2000, 100000])
    p.add_argument("--dir", default=None, help="where the temporary files go")
    p.add_argument("--twin-frames", type=int, default=640)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--out", default=None, metavar="FILE")
    a = p.parse_args()
    import __graft_entry__ as ge
    ge.build()
    out = []
    for n in a.frames:
        out.append(measure(n, a.dir, a.twin_frames, a.repeats))
        print(json.dumps(out[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
