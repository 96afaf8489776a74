#!/usr/bin/env python3
"""What glTF export costs, for resident sequences of 98 (one chunk), 2 000 and 100 000 frames:

    python tools/gltf_bench.py [--frames 98 2000 100000] [--dir DIR] [--repeats 7] [--out FILE]

  rest / rest_mesh / animation   the device time of the launches per skeleton (gem_bvh_rest; gem_gltf_rest_mesh; gem_gltf_animation's
                                 three), each between two device events, after a warm-up: median, minimum and maximum of --repeats
  write_result                   host-inclusive: `gltf.write_result` of three resident sequences, the first two aligned to the third, to
                                 a file under --dir -- alignment, the launches, the read-back, the JSON, the BIN chunk streamed out
  write_result_bvh               the same three sequences through `bvh.write_result_bvh` (three files), for comparison

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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bvh_bench import poses, stats, timed          # noqa: E402


def wall(fn, repeats):
    import torch
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return stats(out)


def measure(n, work, repeats):
    import torch
    from globalegomocap_amd import bvh, gltf, prepare
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    lay = gltf.layout(n)
    res = {"frames": n, "animation_block_bytes": lay.block_bytes, "vertex_block_bytes": lay.vertex_bytes}
    e = prepare._lift_engine(DEFAULT_CALIBRATION, torch.cuda.current_device())
    gt_h = poses(n)
    gt = torch.from_numpy(gt_h).to(e.device)
    est = torch.from_numpy(0.9 * gt_h[:, :, [2, 0, 1]] + 0.3).to(e.device)
    opt = torch.from_numpy(1.1 * gt_h[:, :, [1, 2, 0]] - 0.2).to(e.device)
    rest = bvh.rest_lengths(e, gt)
    block = torch.zeros(lay.block_bytes, dtype=torch.uint8, device=e.device)
    verts = torch.empty(lay.vertex_bytes, dtype=torch.uint8, device=e.device)
    bad = bvh.new_counter(e.device)
    res["rest"] = timed(lambda: bvh.rest_lengths(e, gt), repeats)
    res["rest_mesh"] = timed(lambda: gltf.rest_mesh(e, rest, out=verts), repeats)
    res["animation"] = timed(lambda: gltf.animation(e, gt, None, 25.0, bad, out=block), repeats)
    res["animation"]["store_gb_s"] = round(lay.block_bytes / res["animation"]["median_ms"] / 1e6, 2)
    assert bad.cpu().tolist() == [0, -1]
    d = tempfile.mkdtemp(prefix="gltf_bench_", dir=work)
    try:
        path = os.path.join(d, "result.glb")
        res["write_result"] = wall(lambda: gltf.write_result(e, path, est, opt, gt, fps=25.0), repeats)
        res["write_result"]["frames_per_s"] = round(n / res["write_result"]["median_ms"] * 1e3)
        res["file_bytes"] = os.path.getsize(path)
        res["write_result_bvh"] = wall(lambda: bvh.write_result_bvh(e, os.path.join(d, "bvh"), est, opt, gt, fps=25.0), repeats)
        res["bvh_files_bytes"] = sum(os.path.getsize(os.path.join(d, "bvh", f)) for f in os.listdir(os.path.join(d, "bvh")))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    gltf.release()
    bvh.release()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, nargs="+", default=[98, 2000, 100000])
    p.add_argument("--dir", default=None, help="where the temporary files go")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--out", default=None, metavar="FILE")
    a = p.parse_args()
    import __graft_entry__ as ge
    ge.build()
    out = []
    for n in a.frames:
        out.append(measure(n, a.dir, a.repeats))
        print(json.dumps(out[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
