#!/usr/bin/env python3
"""Golden vectors of the One-Euro filter from the unmodified reference (test infrastructure; needs the reference tree).

    python tools/make_golden_one_euro.py        # GEM_REFERENCE=/path/to/reference; writes tests/golden/one_euro.npz

`utils/one_euro_filter.py` is loaded as it is, at generation time only, and its `OneEuroFilter` class is run -- one instance per
coordinate, started at the first frame, called for every later frame -- over a signal of 40 frames x 45 coordinates (a random walk
plus noise) with irregular timestamps i / 25 +- 4 ms, once per parameter set.  Stored: the signal, the timestamps, the parameter
sets and the class's outputs.  Only data goes into the fixture; no program text of the reference is stored.
"""
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("GEM_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "one_euro.npz")

N_FRAMES, N_COORDS, FPS = 40, 45, 25
PARAMS = [(1.0, 0.0, 1.0), (1.7, 0.3, 1.0), (0.5, 5.0, 2.0)]          # (min_cutoff, beta, d_cutoff); the first is the class's defaults


def main():
    spec = importlib.util.spec_from_file_location("one_euro_filter", os.path.join(REF, "utils", "one_euro_filter.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(2025)
    signal = np.cumsum(rng.normal(0.0, 0.02, (N_FRAMES, N_COORDS)), axis=0) + rng.normal(0.0, 0.01, (N_FRAMES, N_COORDS))
    times = np.arange(N_FRAMES) / FPS + rng.uniform(-0.004, 0.004, N_FRAMES)
    assert (np.diff(times) > 0).all()
    out = {"signal": signal, "times": times, "params": np.array(PARAMS)}
    for k, (mc, beta, dc) in enumerate(PARAMS):
        y = np.empty_like(signal)
        y[0] = signal[0]
        for c in range(N_COORDS):
            f = ref.OneEuroFilter(float(times[0]), float(signal[0, c]), min_cutoff=mc, beta=beta, d_cutoff=dc)
            for i in range(1, N_FRAMES):
                y[i, c] = f(float(times[i]), float(signal[i, c]))
        out["filtered_%d" % k] = y
        d2 = lambda a: np.abs(np.diff(a, 2, axis=0)).mean()          # noqa: E731
        print(PARAMS[k], "changes the signal by up to %.4f, second difference %.1f %% of the signal's" % (np.abs(y - signal).max(), 100 * d2(y) / d2(signal)))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
