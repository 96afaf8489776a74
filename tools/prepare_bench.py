#!/usr/bin/env python3
"""Measurements of the data preparation, one JSON line per leg (appended to --out when given).

    python tools/prepare_bench.py [--frames 2000] [--repeats 5] [--out profiles/prepare_bench.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/prepare_bench.py --kernels-only          # device times, a run of its own

Legs (page cache WARM: every file is read once before the clock starts; median, min and max over --repeats):
  mat_to_recording        .mat directories (float32, uncompressed) -> device-resident Recording, host-inclusive, synchronised
  mat_to_result           the same + whole_sequence.optimize_recording
  chunks_to_result        whole_sequence.optimize_directory on the chunk pickles the Recording writes (the route that existed before)
  chunks_read_stage       its read + copy pipeline alone (files -> frame buffer on the device: parse, gem_file_stage, gem_heat_gather)
  mat_compressed_*        as the first two, every file written with do_compression=True
  stages                  where the .mat route's time goes: sizes (stat), read + scan, inflate, copy + gem_mat_frames, lift, scale, global
--kernels-only launches gem_mat_frames and gem_heat_gather 20 times each on the same 2000 float32 frames (heat_gather on the .mat
layout and on a pickle-like layout: payloads 245 760 + 163 bytes apart, unaligned) and prints event times; under rocprofv3 the
stats file holds the kernels' own times.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

OUT = [None]


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT[0]:
        with open(OUT[0], "a") as f:
            f.write(line + "\n")


def spread(ts):
    ts = sorted(ts)
    return {"median_ms": 1e3 * ts[len(ts) // 2], "min_ms": 1e3 * ts[0], "max_ms": 1e3 * ts[-1], "repeats": len(ts)}


def timed(fn, repeats, sync):
    out, ts = None, []
    for _ in range(repeats):
        sync()
        t = time.perf_counter()
        out = fn()
        sync()
        ts.append(time.perf_counter() - t)
    return out, ts


def write_recording(root, n, compressed, seed=0):
    """n frames of float32 heat-maps: one peak per joint on a noise floor (so that the compressed files are not trivially small)."""
    from globalegomocap_amd import synth_recording as S
    par = S.random_parameters(n, seed)
    rng = np.random.default_rng(seed)
    base = S.paraboloid_heatmaps(par["centres"][:50], par["radii"][:50])
    heat = base.astype(np.float32)[np.arange(n) % 50] * rng.uniform(0.5, 1.0, (n, 1, 1, 1)).astype(np.float32)
    heat += rng.random(heat.shape, dtype=np.float32) * np.float32(0.05)
    names = ["frame_%05d.mat" % k for k in range(n)]
    return S.write_recording(root, heat, par["depth"], names, None, np.full(n, bool(compressed)), par["rows"], par["gt"])


def warm(*dirs):
    total = 0
    for d in dirs:
        for dirpath, _, files in os.walk(d):
            for f in files:
                with open(os.path.join(dirpath, f), "rb") as fh:
                    total += len(fh.read())
    return total


def kernels_only(frames):
    import ctypes as C
    import torch
    from globalegomocap_amd import _capi, prepare as P
    lib = _capi.load_library()
    dev = torch.device("cuda", 0)
    per, file_len = 64 * 64 * 15 * 4, 245976                      # payload bytes; a float32 heat-map file's place (245 960 + slack, 16-aligned)
    arena = torch.randint(0, 255, (frames * file_len + 4096,), dtype=torch.uint8, device=dev)
    depth_at = torch.arange(frames, dtype=torch.int64, device=dev) * file_len + 64
    layouts = {"mat": torch.arange(frames, dtype=torch.int64, device=dev) * file_len + 200,
               "pickle": torch.arange(frames, dtype=torch.int64, device=dev) * (per + 163) + 161}
    kinds = torch.zeros(frames, dtype=torch.int32, device=dev)
    heat = torch.empty((frames, 64, 64, 15), dtype=torch.float32, device=dev)
    ref = torch.empty_like(heat)
    depth = torch.empty((frames, 15), dtype=torch.float64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def gather(offs):
        _capi.check(lib.gem_heat_gather(C.c_void_p(arena.data_ptr()), arena.numel() - 16, C.c_void_p(offs.data_ptr()), frames, 64, 64, 15,
                                        _capi.DT_F32, 1, C.c_void_p(ref.data_ptr()), st), lib)

    def event_ms(fn, n=20):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(n):
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        return spread(ts)
    for name, offs in layouts.items():
        emit(leg="kernel_event_time", kernel="gem_heat_gather", layout=name, frames=frames, **event_ms(lambda: gather(offs)))
        emit(leg="kernel_event_time", kernel="gem_mat_frames", layout=name, frames=frames,
             **event_ms(lambda: P.mat_frames(arena, arena.numel() - 16, offs, depth_at, kinds, heat, depth)))
        gather(offs)
        torch.cuda.synchronize()
        assert torch.equal(heat.view(torch.int32), ref.view(torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--work", default=None, help="directory for the synthetic recording (default: a temporary one, removed afterwards)")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--skip-compressed", action="store_true")
    a = ap.parse_args()
    OUT[0] = a.out
    import torch
    import __graft_entry__ as ge
    ge.build()
    if a.kernels_only:
        return kernels_only(a.frames)
    from globalegomocap_amd import prepare as P, staging, vae as V, whole_sequence as ws
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    sync = torch.cuda.synchronize
    work = a.work or tempfile.mkdtemp(prefix="gem_prepare_bench_")
    n = a.frames + 1                                              # (the chunk loop drops the last chunk of an exact multiple)
    shape = V.VAEShape()
    kw = dict(global_vae_path=V.synthetic_state_dict(shape, seed=1, gain=2.0), local_vae_path=V.synthetic_state_dict(shape, seed=2, gain=2.0),
              verbose=False)
    from globalegomocap_amd.optimizer import SequenceOptimizer
    kw["optimizer"] = SequenceOptimizer(DEFAULT_CALIBRATION, kw["global_vae_path"], kw["local_vae_path"], max_windows=12 * (a.frames // 100))
    emit(leg="setup", frames=a.frames, device=torch.cuda.get_device_name(0), page_cache="warm (every file read once before timing)")
    try:
        for tag, compressed in (("mat", False),) + (() if a.skip_compressed else (("mat_compressed", True),)):
            root = os.path.join(work, tag)
            t = time.perf_counter()
            hd, dd, traj, gtp = write_recording(root, n, compressed)
            emit(leg=tag + "_written", seconds=time.perf_counter() - t, bytes=warm(hd, dd))
            prep = lambda: P.prepare_sequence(traj, hd, dd, gtp, 0, n, fps=25, test_size=100, verbose=False)      # noqa: E731
            rec = prep()                                          # first call: pools, pinned blocks, the lifting engine
            assert len(rec) == a.frames // 100
            rec, ts = timed(prep, a.repeats, sync)
            emit(leg=tag + "_to_recording", chunks=len(rec), **spread(ts))
            torch.manual_seed(0)
            ws.optimize_recording(rec, DEFAULT_CALIBRATION, **kw)
            _, ts = timed(lambda: ws.optimize_recording(prep(), DEFAULT_CALIBRATION, **kw), a.repeats, sync)
            emit(leg=tag + "_to_result", **spread(ts))
            if not compressed:
                chunks = os.path.join(work, "chunks")
                rec.write_chunks(chunks)
                emit(leg="chunks_written", bytes=warm(chunks))
                ws.optimize_directory(chunks, DEFAULT_CALIBRATION, **kw)
                _, ts = timed(lambda: ws.optimize_directory(chunks, DEFAULT_CALIBRATION, **kw), a.repeats, sync)
                emit(leg="chunks_to_result", **spread(ts))
                dev = torch.device("cuda", torch.cuda.current_device())
                paths = ws.list_chunks(chunks)

                def read_stage():
                    pool = staging.reader_pool("read", 8, staging.cpus_near(dev))
                    for c in [f.result() for f in [pool.submit(ws.load_chunk, q, dev) for q in paths]]:
                        c["heat_ready"].synchronize()
                read_stage()
                _, ts = timed(read_stage, a.repeats, sync)
                emit(leg="chunks_read_stage", note="load_chunk per chunk on 8 reader threads: parse + gem_file_stage + gem_heat_gather", **spread(ts))
                # where the .mat route's time goes (wall time of the calling thread's phases, summed over the repeats)
                tm = {}
                for _ in range(a.repeats):
                    P.prepare_spans(traj, hd, dd, gtp, P.chunk_spans(0, n, 100), 25, 0, timings=tm)
                emit(leg="stages", phases_ms={k: 1e3 * v / a.repeats for k, v in tm.items()})
                heat_paths, depth_paths = P.list_frames(hd, 0, a.frames), P.list_frames(dd, 0, a.frames)
                (heat, depth, _), ts = timed(lambda: P.frames_to_device(heat_paths, depth_paths, dev), a.repeats, sync)
                emit(leg="stage_files_to_frames", note="sizes + read + scan + copy + gem_mat_frames", **spread(ts))
                eng = P._lift_engine(DEFAULT_CALIBRATION, dev.index)
                _, ts = timed(lambda: eng.lift_skeleton(heat, depth), a.repeats, sync)
                emit(leg="stage_lift", **spread(ts))
            del rec
    finally:
        if a.work is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
