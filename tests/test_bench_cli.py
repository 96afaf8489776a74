"""bench.py's own contract: --steps sets the timed steps, a plain run prints the lean line (the side records need --full),
--dump-outputs writes what the timed call returned as float32 / float64 .npy files within 64 MB, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_types_names_and_seeded_sample(tmp_path, monkeypatch):
    import bench
    arrays = {"poses": np.arange(40 * 6, dtype=np.float64).reshape(40, 6), "mid": np.ones((40, 3), np.float32),
              "evals": np.arange(80, dtype=np.int32), "none": None}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["evals", "mid", "poses"]
    assert got["poses"].dtype == np.float64 and np.array_equal(got["poses"], arrays["poses"])
    assert got["mid"].dtype == np.float32 and got["evals"].dtype == np.float64 and np.array_equal(got["evals"], np.arange(80))
    # above the budget: every array keeps the same fraction of its rows, the same rows on every call
    monkeypatch.setattr(bench, "DUMP_BYTES", 1000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    b = {f: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    c = {f: np.load(tmp_path / "c" / f) for f in os.listdir(tmp_path / "c")}
    assert sum(v.nbytes for v in b.values()) <= 1000
    assert all(np.array_equal(b[f], c[f]) for f in b)
    rows = b["poses.npy"][:, 0] / 6
    assert 0 < len(rows) < 40 and np.array_equal(rows, np.sort(rows)) and np.array_equal(b["mid.npy"], np.ones((len(rows), 3), np.float32))


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path):
    """One chunk (12 windows), structured VAEs: the plain line holds the headline fields and none of the side records, its
    `steps` / `ms_per_step` are those of the run, and two runs with the same arguments dump identical arrays."""
    lines = []
    for d in ("one", "two"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "1",
                            "--vae", "structured", "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "windows/s" and line["higher_is_better"] is True
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 12) < 0.05 * 12
    for k in ("roofline", "cpu_baseline", "other_precisions", "configs2", "partition8", "host_inclusive", "train", "summary"):
        assert k not in line, k
    files = sorted(os.listdir(tmp_path / "one"))
    assert files == sorted(os.listdir(tmp_path / "two"))
    assert {"mid_local.npy", "glob.npy", "stats_func_evals.npy", "stats_final_loss.npy"} <= set(files)
    g = np.load(tmp_path / "one" / "glob.npy")
    assert g.shape == (12, 10, 15, 3) and g.dtype == np.float64 and np.isfinite(g).all()
    for f in files:
        a, b = np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b, equal_nan=True), f
