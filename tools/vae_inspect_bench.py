#!/usr/bin/env python3
"""What a reconstruction pass of `vae_inspect` costs, one JSON line per leg.  Runs ON THE GPU BOX.

    python tools/vae_inspect_bench.py [--windows 65536] [--batch 256] [--repeats 3]

The full-size VAE (2048-D, synthetic weights) over `--windows` windows of `synth.make_training_windows`, given as a host array:
  `reconstruct`   Inspector.reconstruct(posterior="sample"): encode -> decode -> gem_latent_report per batch, the table and the
                  per-dimension sums on the device until the one read-back at the end; HIP events around the whole call
  `reconstruct_mean`, `eps_draw`   the pass with posterior="mean", and the host's share of "sample" on its own: the noise of
                  every batch drawn from the CPU generator and copied to the device
  `evaluate`      the same windows through VAETrainer.evaluate, which synchronises once per batch and yields one number; it makes
                  its own engine on every call, so `evaluate_setup` (the call on one batch) is reported beside it
  `report`        gem_latent_report alone, as many calls as the pass has batches, on resident buffers of one batch: its share
Each leg is warmed up once and repeated `--repeats` times; `spread` is (max - min) / median of the repeats.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, repeats):
    """(event seconds, wall seconds) of `repeats` calls after one warm-up; the events bracket everything the call enqueues."""
    import torch
    fn()
    ev, wall = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t)
        ev.append(e0.elapsed_time(e1) * 1e-3)
    return ev, wall


def stats(ev, wall, n):
    med = float(np.median(ev))
    return dict(event_s=ev, wall_s=wall, median_s=med, spread=(max(ev) - min(ev)) / med, us_per_window=med / n * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import synth, vae, vae_inspect
    from globalegomocap_amd.vae_train import VAETrainer
    torch.cuda.set_device(0)
    shape = vae.VAEShape()
    sd = vae.synthetic_state_dict(shape, seed=3)
    t = time.perf_counter()
    windows = synth.make_training_windows(a.windows, shape.seq_len, 1)
    emit(leg="synthesis", windows=a.windows, seconds=time.perf_counter() - t, device=torch.cuda.get_device_name(0))
    n, bs = a.windows, a.batch

    ins = vae_inspect.Inspector(sd, shape=shape, max_windows=bs)
    try:
        rep = [None]

        def run():
            rep[0] = ins.reconstruct(windows, batch_size=bs, posterior="sample", seed=0)
        ev, wall = timed(run, a.repeats)
        emit(leg="reconstruct", windows=n, batch=bs, mpjpe=rep[0].means["mpjpe"], active_units=rep[0].active_units(), **stats(ev, wall, n))
        pass_s = float(np.median(ev))

        def run_mean():
            rep[0] = ins.reconstruct(windows, batch_size=bs, posterior="mean")
        ev, wall = timed(run_mean, a.repeats)
        emit(leg="reconstruct_mean", windows=n, batch=bs, mpjpe=rep[0].means["mpjpe"], **stats(ev, wall, n))

        # what posterior="sample" adds on the host: the noise of every batch from the CPU generator, and its copy to the device
        g = torch.Generator(device="cpu").manual_seed(0)

        def draw():
            for lo in range(0, n, bs):
                torch.randn(min(bs, n - lo), shape.latent_dim, generator=g).to("cuda")
        ev, wall = timed(draw, a.repeats)
        emit(leg="eps_draw", batches=-(-n // bs), **stats(ev, wall, n))

        # the report kernel alone: one batch's buffers, as many calls as the pass has batches
        eng = ins.engine
        x = torch.from_numpy(windows[:bs]).cuda()
        mu, lv, z = eng.encode(0, x, torch.randn(bs, shape.latent_dim))
        rec = eng.decode(0, z)
        table = torch.empty(bs, 5, device="cuda", dtype=torch.float64)
        cols = torch.zeros(3, shape.latent_dim, device="cuda", dtype=torch.float64)
        count = torch.zeros(1, device="cuda", dtype=torch.int64)
        calls = -(-n // bs)

        def report():
            for _ in range(calls):
                eng.latent_report(mu, lv, x, rec, cols=cols, count=count, out=table)
        ev, wall = timed(report, a.repeats)
        emit(leg="report", calls=calls, batch=bs, us_per_call=float(np.median(ev)) / calls * 1e6, share_of_pass=float(np.median(ev)) / pass_s,
             **stats(ev, wall, n))
    finally:
        ins.close()

    tr = VAETrainer(shape, batch_size=bs, state_dict=sd, seed=0)
    try:
        out = [None]

        def evaluate(w=windows):
            out[0] = tr.evaluate(w, batch_size=bs)
        ev, wall = timed(evaluate, a.repeats)
        emit(leg="evaluate", windows=n, batch=bs, mpjpe=out[0], **stats(ev, wall, n))
        ev, wall = timed(lambda: evaluate(windows[:bs]), a.repeats)
        emit(leg="evaluate_setup", windows=bs, batch=bs, **stats(ev, wall, bs))
    finally:
        tr.close()


if __name__ == "__main__":
    main()
