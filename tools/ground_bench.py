#!/usr/bin/env python3
"""What estimating the ground plane costs, on synthetic walkers (`synth_walk`, 3 cm noise) in their chunk world:

    python tools/ground_bench.py [--chunks 20] [--chunk-frames 100] [--long 100000] [--repeats 7] [--launches 20] [--pipeline-chunks 4]
                                 [--out profiles/ground_bench.json]

  batch      ONE call for --chunks sequences of --chunk-frames frames, each its own allocation: device events around the launch alone
             (the table already uploaded), device events around `ground_call` (the table's upload and the launch, enqueued only), and
             the host clock around `estimate_ground` (upload, kernel, the records back, synchronised); the numpy twin
             (tests/ground_twin.py) on the same sequences, one after the other
  long       the same for one sequence of --long frames (its foot points in the work buffer)
  pipeline   `whole_sequence.optimize_directory` with bvh=DIR on --pipeline-chunks synthetic chunks of 26 frames, without and with
             upright=True, alternating, host-inclusive and synchronised

Prints one JSON object and, with --out, writes it to FILE."""
import argparse
import ctypes as C
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

FPS = 25


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


def wall_ms(fn, repeats):
    import torch
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return spread(out)


def launch_only(engine, seqs, lag):
    """-> a function that launches gem_ground_plane on tables that are on the device already."""
    import torch
    from globalegomocap_amd import _capi, ground as G
    lib, n = engine.lib, len(seqs)
    frames = np.array([len(x) for x in seqs], dtype=np.int64)
    offsets = np.full(n, -1, dtype=np.int64)
    need = int(lib.gem_ground_plane_work(C.c_void_p(frames.ctypes.data), n, C.c_void_p(offsets.ctypes.data)))
    table = np.concatenate([np.array([x.data_ptr() for x in seqs], dtype=np.int64), frames, np.zeros(n, dtype=np.int64), offsets])
    d_table = torch.from_numpy(table).to(engine.device)
    work = torch.empty(max(need // 8, 1), dtype=torch.float64, device=engine.device)
    records = torch.empty(n, _capi.GROUND_RECORD_DOUBLES, dtype=torch.float64, device=engine.device)

    def launch():
        _capi.check(lib.gem_ground_plane(C.c_void_p(table.ctypes.data), C.c_void_p(d_table.data_ptr()), n, lag, G.TAU_V, G.TAU_H, G.MIN_SPREAD,
                                         G.MIN_POINTS, 0.0, C.c_void_p(work.data_ptr()), need, C.c_void_p(records.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)
    launch.keep = (d_table, work, records)
    return launch


def measure(engine, arrays, a):
    import torch
    import ground_twin as T
    from globalegomocap_amd import ground as G
    lag = G.default_lag(FPS)
    seqs = [torch.from_numpy(np.ascontiguousarray(x)).to(engine.device) for x in arrays]
    r = {"sequences": len(seqs), "frames_each": len(arrays[0])}
    r["kernel_device_ms"] = event_ms(launch_only(engine, seqs, lag), a.launches)
    r["call_enqueued_device_ms"] = event_ms(lambda: G.ground_call(engine, seqs, lag), a.launches)
    r["estimate_ground_wall_ms"] = wall_ms(lambda: G.estimate_ground(engine, seqs, fps=FPS), a.repeats)
    found = G.estimate_ground(engine, seqs, fps=FPS)
    t = time.perf_counter()
    twins = [T.estimate(x, lag=lag) for x in arrays]
    r["twin_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    r["largest_normal_difference_to_twin"] = float(max(np.abs(g.normal - e["n"]).max() for g, e in zip(found, twins)))
    r["first_estimate"] = {k: v for k, v in found[0].as_dict().items() if k != "crt"}
    return r


def pipeline(a, work):
    """optimize_directory(bvh=DIR) on synthetic chunks without and with upright=True, alternating."""
    import torch
    from globalegomocap_amd import prepare as P, synth_recording as S, vae as vae_schema, whole_sequence as ws
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    size, n = 26, 26 * a.pipeline_chunks + 1
    par = S.random_parameters(n, seed=23)
    heat = S.paraboloid_heatmaps(par["centres"], par["radii"])
    hd, dd, traj, gtp = S.write_recording(os.path.join(work, "rec"), heat, par["depth"], ["f_%d.mat" % k for k in range(n)], None, None,
                                          par["rows"], par["gt"])
    rec = P.prepare_sequence(traj, hd, dd, gtp, 0, n, fps=FPS, test_size=size, verbose=False)
    root = os.path.join(work, "chunks", "studio")
    rec.write_chunks(root)
    shape = vae_schema.VAEShape()
    kw = dict(global_vae_path=vae_schema.structured_state_dict(shape, 8, feature_offset=3.0),          # (bench.py's full-size VAEs)
              local_vae_path=vae_schema.structured_state_dict(shape, 7, feature_offset=0.0), verbose=False)
    runs = {"bvh": lambda: ws.optimize_directory(root, DEFAULT_CALIBRATION, bvh=os.path.join(work, "b0"), **kw),
            "bvh_upright": lambda: ws.optimize_directory(root, DEFAULT_CALIBRATION, bvh=os.path.join(work, "b1"), upright=True, **kw)}
    for f in runs.values():
        f()
    out = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, f in runs.items():
            torch.manual_seed(3)
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t) * 1e3)
    res = {k: spread(v) for k, v in out.items()}
    res["chunks"], res["frames_per_chunk"] = a.pipeline_chunks, size
    res["added_ms"] = round(res["bvh_upright"]["median_ms"] - res["bvh"]["median_ms"], 3)
    ws.release_pools()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--chunks", type=int, default=20)
    p.add_argument("--chunk-frames", type=int, default=100)
    p.add_argument("--long", type=int, default=100000)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--pipeline-chunks", type=int, default=4, help="0: leave the pipeline out")
    p.add_argument("--out", default=None, metavar="FILE")
    a = p.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    import ground_twin as T
    from globalegomocap_amd import prepare
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    engine = prepare._lift_engine(DEFAULT_CALIBRATION, 0)
    res = {"device": torch.cuda.get_device_name(0), "fps": FPS, "noise_m": 0.03}
    res["batch"] = measure(engine, [T.walker_world(a.chunk_frames, noise=0.03, seed=k)[0] for k in range(a.chunks)], a)
    print("batch: %s" % json.dumps(res["batch"]), file=sys.stderr, flush=True)
    res["long"] = measure(engine, [T.walker_world(a.long, noise=0.03, seed=11)[0]], a)
    print("long: %s" % json.dumps(res["long"]), file=sys.stderr, flush=True)
    if a.pipeline_chunks:
        work = tempfile.mkdtemp(prefix="gem_ground_bench_")
        try:
            res["pipeline"] = pipeline(a, work)
        finally:
            shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
