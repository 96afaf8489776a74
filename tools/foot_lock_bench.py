#!/usr/bin/env python3
"""What locking the feet costs, on synthetic walkers (`synth_walk`) in their chunk world:

    python tools/foot_lock_bench.py [--chunks 20] [--chunk-frames 100] [--long 100000] [--repeats 7] [--launches 20] [--pipeline-chunks 4]
                                    [--out profiles/foot_lock_bench.json]

  batch      ONE call for --chunks sequences of --chunk-frames frames (3 cm noise), each its own allocation: device events around
             the gem_foot_lock launch alone (the table uploaded and the ground records made before), device events around the
             enqueued pair `ground_call` + `lock_call` (two uploads, two launches), and the host clock around `lock_feet` (uploads,
             both kernels, the records back, synchronised); the numpy twin (tests/foot_lock_twin.py) on the same sequences at the
             device's planes, one after the other
  long       the same for one walking sequence of --long frames (its foot points in the work buffer, thousands of short runs)
  standing   the same for a wearer who stands for --long frames (1 cm noise): one run per foot as long as the sequence, whose
             anchor the whole workgroup sums
  pipeline   `whole_sequence.optimize_directory` with bvh=DIR on --pipeline-chunks synthetic chunks of 26 frames, without and with
             foot_lock=True, alternating, host-inclusive and synchronised

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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np          # noqa: E402

from ground_bench import FPS, event_ms, spread, wall_ms          # noqa: E402


def launch_only(engine, seqs, g_records, lag, blend):
    """-> a function that launches gem_foot_lock on a table and ground records that are on the device already."""
    import torch
    from globalegomocap_amd import _capi, foot_lock as L, ground as G
    lib, n = engine.lib, len(seqs)
    frames = np.array([len(x) for x in seqs], dtype=np.int64)
    offsets = np.full(n, -1, dtype=np.int64)
    need = int(lib.gem_foot_lock_work(C.c_void_p(frames.ctypes.data), n, C.c_void_p(offsets.ctypes.data)))
    outs = [torch.empty_like(x) for x in seqs]
    table = np.concatenate([np.array([x.data_ptr() for x in seqs], dtype=np.int64), frames, np.array([y.data_ptr() for y in outs], dtype=np.int64),
                            offsets])
    d_table = torch.from_numpy(table).to(engine.device)
    work = torch.empty(max(need // 8, 1), dtype=torch.float64, device=engine.device)
    records = torch.empty(n, _capi.FOOT_LOCK_RECORD_DOUBLES, dtype=torch.float64, device=engine.device)

    def launch():
        _capi.check(lib.gem_foot_lock(C.c_void_p(table.ctypes.data), C.c_void_p(d_table.data_ptr()), n, C.c_void_p(g_records.data_ptr()), lag, G.TAU_V,
                                      G.TAU_H, L.MIN_RUN, blend, 1, L.STRETCH, C.c_void_p(work.data_ptr()), need, C.c_void_p(records.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)
    launch.keep = (d_table, work, records, outs)
    return launch


def measure(engine, arrays, a):
    import torch
    import foot_lock_twin as T
    from globalegomocap_amd import foot_lock as L, ground as G
    lag, blend = G.default_lag(FPS), L.default_blend(FPS)
    seqs = [torch.from_numpy(np.ascontiguousarray(x)).to(engine.device) for x in arrays]
    g_records = G.ground_call(engine, seqs, lag)
    r = {"sequences": len(seqs), "frames_each": len(arrays[0])}
    r["kernel_device_ms"] = event_ms(launch_only(engine, seqs, g_records, lag, blend), a.launches)
    r["ground_and_lock_enqueued_device_ms"] = event_ms(lambda: L.lock_call(engine, seqs, G.ground_call(engine, seqs, lag), lag, blend=blend), a.launches)
    r["lock_feet_wall_ms"] = wall_ms(lambda: L.lock_feet(engine, seqs, fps=FPS), a.repeats)
    found = L.lock_feet(engine, seqs, fps=FPS)
    planes = g_records.cpu().numpy()
    t = time.perf_counter()
    twins = [T.lock(x, g[2:5], g[5], lag=lag, blend=blend) for x, g in zip(arrays, planes)]
    r["twin_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    r["largest_joint_difference_to_twin"] = float(max(np.abs(f.sequence.cpu().numpy() - e["sequence"]).max() for f, e in zip(found, twins)))
    r["runs"] = int(sum(sum(f.runs) for f in found))
    r["first_lock"] = found[0].as_dict()
    return r


def pipeline(a, work):
    """optimize_directory(bvh=DIR) on synthetic chunks without and with foot_lock=True, alternating."""
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
            "bvh_foot_lock": lambda: ws.optimize_directory(root, DEFAULT_CALIBRATION, bvh=os.path.join(work, "b1"), foot_lock=True, **kw)}
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
    res["added_ms"] = round(res["bvh_foot_lock"]["median_ms"] - res["bvh"]["median_ms"], 3)
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
    import ground_twin as GT
    from globalegomocap_amd import prepare
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    engine = prepare._lift_engine(DEFAULT_CALIBRATION, 0)
    res = {"device": torch.cuda.get_device_name(0), "fps": FPS}
    cases = (("batch", lambda: [GT.walker_world(a.chunk_frames, noise=0.03, seed=k)[0] for k in range(a.chunks)]),
             ("long", lambda: [GT.walker_world(a.long, noise=0.03, seed=11)[0]]),
             ("standing", lambda: [GT.walker_world(a.long, stand=[(0, a.long)], noise=0.01, seed=12)[0]]))
    for name, make in cases:
        res[name] = measure(engine, make(), a)
        print("%s: %s" % (name, json.dumps(res[name])), file=sys.stderr, flush=True)
    if a.pipeline_chunks:
        work = tempfile.mkdtemp(prefix="gem_foot_lock_bench_")
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
