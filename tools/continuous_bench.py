#!/usr/bin/env python3
"""What optimising a recording as one motion costs and gives, on a synthetic recording with known truth:

    python tools/continuous_bench.py [--frames 2000] [--launches 20] [--repeats 5] [--fit-steps 2000] [--weights-cache FILE]
                                     [--no-recording] [--out profiles/continuous_bench.json]

  merge      gem_merge_cover (merged + smoothed + count + spread, and merged alone) on the windows of --frames frames at stride 8 and at
             stride 1, device events around the launches alone (tables and outputs on the device already); beside it
             gem_merge_windows (merge + smoothing, and merge alone) on the regular windows of the same frames at stride 8 and
             gem_merge_dense at stride 1; the bytes each has to read and write, from the shapes
  recording  `synth.make_sequence(--frames)` (bench.py's camera noise) as a recording without ground truth whose truth is known, in 20
             chunks with their origins: `whole_sequence.optimize_recording` (the chunked route) against
             `continuous.optimize_continuous` on `Recording.continuous()`, the same VAEs (bench.py's fitted synthetic ones), the same
             seed, alternating, host-inclusive and synchronised.  Frames returned, MPJPE against the truth in the recording's frame,
             how much the error vector (result - truth) changes from one returned frame to the next, per joint, across the former
             chunk boundaries and elsewhere, and the ground's figures with one floor against one per chunk
  walker     the floor alone: `synth_walk.walk(--frames)` in its world with 3 cm noise, `ground.estimate_ground` once over all frames
             and once per 100-frame chunk

Prints one JSON object and, with --out, writes it to FILE."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402

FPS, CHUNK = 25, 100


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


def merge_timings(engine, frames, launches):
    import torch
    from globalegomocap_amd import _capi
    from globalegomocap_amd.sequence import cover_starts, window_starts
    lib, dev = engine.lib, engine.device
    P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    res = {}
    for stride in (8, 1):
        starts = cover_starts(frames, stride=stride)
        B, JC = len(starts), 45
        w = torch.randn(B, 10, 15, 3, dtype=torch.float64, device=dev)
        s_d = torch.from_numpy(starts).to(dev)
        merged, smoothed = (torch.empty(frames, 15, 3, dtype=torch.float64, device=dev) for _ in range(2))
        count, far = torch.empty(frames, dtype=torch.int32, device=dev), torch.empty(frames, dtype=torch.float64, device=dev)

        def cover(full):
            _capi.check(lib.gem_merge_cover(P(w), P(s_d), B, 10, 15, frames, P(merged), P(smoothed if full else None), P(count if full else None),
                                            P(far if full else None), stream()), lib)
        r = {"windows": B, "frames": frames,
             "bytes_read_windows": B * 10 * JC * 8, "bytes_read_table": B * 4, "bytes_written_merged": frames * JC * 8,
             "gem_merge_cover_all_outputs": event_ms(lambda: cover(True), launches), "gem_merge_cover_merged_alone": event_ms(lambda: cover(False), launches)}
        if stride == 8:
            regular = len(window_starts(frames))
            out = torch.empty(regular * 8 + 2, 15, 3, dtype=torch.float64, device=dev)

            def windows(smooth):
                _capi.check(lib.gem_merge_windows(engine._h, P(w), 1, regular, 2, smooth, P(out), stream()), lib)
            r.update(regular_windows=regular, gem_merge_windows_smoothed=event_ms(lambda: windows(1), launches),
                     gem_merge_windows_merged_alone=event_ms(lambda: windows(0), launches))
            r["ratio_all_outputs_to_merge_windows_smoothed"] = round(r["gem_merge_cover_all_outputs"]["median_ms"] / r["gem_merge_windows_smoothed"]["median_ms"], 3)
            r["ratio_merged_alone"] = round(r["gem_merge_cover_merged_alone"]["median_ms"] / r["gem_merge_windows_merged_alone"]["median_ms"], 3)
        else:
            out = torch.empty(1, (B - 1) * stride + 10, 15, 3, dtype=torch.float64, device=dev)
            r["gem_merge_dense"] = event_ms(lambda: _capi.check(lib.gem_merge_dense(P(w), 1, B, 10, JC, stride, P(out), stream()), lib), launches)
            r["ratio_merged_alone"] = round(r["gem_merge_cover_merged_alone"]["median_ms"] / r["gem_merge_dense"]["median_ms"], 3)
        res["stride_%d" % stride] = r
    return res


def weights(a, device):
    import torch
    from globalegomocap_amd import vae as vae_schema
    if a.weights_cache and os.path.exists(a.weights_cache):
        sd_local, err_l, sd_global, err_g = torch.load(a.weights_cache, weights_only=False)
    else:
        import bench
        shape = vae_schema.VAEShape()
        sd_local, err_l = bench.fit_weights(shape, 101, device, a.fit_steps, relative=False)
        sd_global, err_g = bench.fit_weights(shape, 102, device, a.fit_steps, relative=True)
        if a.weights_cache:
            torch.save((sd_local, err_l, sd_global, err_g), a.weights_cache)
    return sd_local, sd_global, "synthetic, fitted as bench.py fits them (recon %.1f / %.1f mm)" % (err_l * 1e3, err_g * 1e3)


def to_world(local, cams):
    return np.einsum("nij,nkj->nki", cams[:, :3, :3], local) + cams[:, None, :3, 3]


def error_jumps(err, frame_of, boundary):
    """Mean over joints of |e[i+1] - e[i]| between consecutive RETURNED frames i, i+1 (frames frame_of[i], frame_of[i+1] of the
    recording), split by whether a former chunk boundary lies between the two (the chunked route returns no frames 98 and 99 of a chunk:
    its pairs across a boundary are three frames apart)."""
    step = np.linalg.norm(err[1:] - err[:-1], axis=-1).mean(axis=1)
    across = (frame_of[1:] // boundary) != (frame_of[:-1] // boundary)
    return {"across_boundaries_m": float(step[across].mean()), "elsewhere_m": float(step[~across].mean()), "pairs_across": int(across.sum())}


def ground_figures(found):
    found = found if isinstance(found, list) else [found]
    return {"floors": len(found), "skate_m_per_s": float(np.mean([g.skate for g in found])), "inlier_share": float(sum(g.inliers for g in found) / max(1, sum(g.points for g in found))),
            "points": int(sum(g.points for g in found)), "rms_m": float(np.mean([g.rms for g in found]))}


def recording(a, device):
    import torch
    from globalegomocap_amd import continuous, ground, prepare as P, synth, whole_sequence as ws
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    from globalegomocap_amd.optimizer import SequenceOptimizer
    from globalegomocap_amd.sequence import cover_starts
    n, n_chunks = a.frames, a.frames // CHUNK
    sd_local, sd_global, note = weights(a, device)
    s = synth.make_sequence_device(n, seed=1000, device=device, cam_jitter=(0.3, 0.002))
    Cw, est = s["cams_np"], s["est_local_np"]
    first = np.linalg.inv(Cw[0])
    world = first[None] @ Cw
    truth = s["gt_global"] @ first[:3, :3].T + first[:3, 3]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)      # noqa: E731
    chunks = []
    for k in range(n_chunks):
        lo, hi = k * CHUNK, (k + 1) * CHUNK
        cams = np.linalg.inv(Cw[lo])[None] @ Cw[lo:hi]
        chunks.append(P.RecordingChunk(lo, hi, s["heat"][lo:hi], t(est[lo:hi]), t(to_world(est[lo:hi], cams)), t(cams), None))
    rec = P.Recording(chunks, world[::CHUNK].copy())
    one = rec.continuous()
    opt = SequenceOptimizer(DEFAULT_CALIBRATION, sd_global, sd_local, max_windows=len(cover_starts(n)))
    kw = dict(ground_truth=False, optimizer=opt, verbose=False)
    runs = {"chunked": lambda: ws.optimize_recording(rec, DEFAULT_CALIBRATION, **kw),
            "continuous": lambda: continuous.optimize_continuous(one, DEFAULT_CALIBRATION, **kw),
            "continuous_with_join": lambda: continuous.optimize_continuous(rec, DEFAULT_CALIBRATION, **kw)}
    results, wall = {}, {k: [] for k in runs}
    for k, f in runs.items():          # (warm-up, and the results that are compared)
        torch.manual_seed(5)
        results[k] = f()
    for _ in range(a.repeats):
        for k, f in runs.items():
            torch.manual_seed(5)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    res = {"frames": n, "chunks": n_chunks, "vae": note, "wall": {k: spread(v) for k, v in wall.items()}}
    res["wall"]["continuous_over_chunked"] = round(res["wall"]["continuous"]["median_ms"] / res["wall"]["chunked"]["median_ms"], 3)
    # the chunked route's frames, moved into the recording's frame
    per = CHUNK - 2
    parts = P.to_recording_frame(rec, [results["chunked"][3][k * per:(k + 1) * per] for k in range(n_chunks)])
    frame_of = np.concatenate([k * CHUNK + np.arange(per) for k in range(n_chunks)])
    chunked, cont = np.concatenate(parts), results["continuous"][3]
    mpjpe = lambda x, f: float(np.linalg.norm(x - truth[f], axis=-1).mean())      # noqa: E731
    res["chunked"] = {"frames_returned": int(len(chunked)), "mpjpe_m": mpjpe(chunked, frame_of), "error_jump": error_jumps(chunked - truth[frame_of], frame_of, CHUNK),
                      "report": {k: v for k, v in results["chunked"][0].items()}}
    all_frames = np.arange(n)
    res["continuous"] = {"frames_returned": int(len(cont)), "mpjpe_m": mpjpe(cont, all_frames), "mpjpe_on_the_chunked_routes_frames_m": mpjpe(cont[frame_of], frame_of),
                         "error_jump": error_jumps(cont - truth, all_frames, CHUNK), "report": results["continuous"][0]}
    res["estimated_mpjpe_m"] = mpjpe(results["continuous"][2], all_frames)
    e = opt.engine
    res["continuous"]["ground"] = ground_figures(ground.estimate_ground(e, cont, fps=FPS))
    res["chunked"]["ground"] = ground_figures(ground.estimate_ground(e, [results["chunked"][3][k * per:(k + 1) * per] for k in range(n_chunks)], fps=FPS))
    ws.release_pools()
    return res


def walker(engine, frames):
    from globalegomocap_amd import ground, synth_walk
    rng = np.random.default_rng(11)
    x = synth_walk.walk(frames, seed=11)["world"]
    x = x + rng.normal(0.0, 0.03, x.shape)
    return {"frames": frames, "noise_m": 0.03, "one_floor": ground_figures(ground.estimate_ground(engine, x, fps=FPS)),
            "floor_per_chunk": ground_figures(ground.estimate_ground(engine, [x[k:k + CHUNK] for k in range(0, frames - CHUNK + 1, CHUNK)], fps=FPS))}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=2000)
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--fit-steps", type=int, default=2000)
    p.add_argument("--weights-cache", default=None, metavar="FILE", help="bench.py's --weights-cache file: loaded when it exists, else written")
    p.add_argument("--no-recording", action="store_true", help="the merge kernels and the walker's floor alone")
    p.add_argument("--out", default=None, metavar="FILE")
    a = p.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import prepare
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    engine = prepare._lift_engine(DEFAULT_CALIBRATION, 0)
    res = {"device": torch.cuda.get_device_name(0), "merge": merge_timings(engine, a.frames, a.launches)}
    print("merge: %s" % json.dumps(res["merge"]), file=sys.stderr, flush=True)
    res["walker"] = walker(engine, a.frames)
    print("walker: %s" % json.dumps(res["walker"]), file=sys.stderr, flush=True)
    if not a.no_recording:
        res["recording"] = recording(a, device)
    print(json.dumps(res, default=str), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, default=str)
            f.write("\n")


if __name__ == "__main__":
    main()
