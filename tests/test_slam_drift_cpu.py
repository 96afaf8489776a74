"""A SLAM scale that drifts within a recording, without a GPU: the numpy twin (tests/slam_drift_twin.py) on
the synthetic walker whose trajectory's scale creeps or wanders, its exact cases, standing stretches, lost rows, the refusal, the
margins of the cases the device is held to (tests/test_slam_drift_gpu.py imports them from here), and the host's logic.

Float64 against extended precision, measured on the CPU with `spread` below (the largest relative distance between the knot
values of the twin run in float64 and in np.longdouble) on the device's cases: walker 4.1e-16, two knots 2.9e-15, lost rows
5.7e-16, standing 2.1e-15, 2048 knots 2.4e-15.  All lie below 1e-13, so the device's knot values are held to 1e-12 relative."""
import functools
import os
import re

import numpy as np
import pytest

import slam_drift_twin as D
import slam_scale_twin as T
from globalegomocap_amd import synth_walk as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAG = 5
MARGIN = 1e-9
SEEDS = (1, 2, 3, 4, 5, 6)


def creeping(n):
    return 0.8 + 0.3 * np.arange(n) / n


def wandering(n):
    x = np.arange(n) / n
    return 1.0 + 0.15 * np.sin(5.0 * x) + 0.2 * x


def _twin(w, knot, keep=None, lag=LAG, c_factor=1.0, **kw):
    R, c = W.slam_inputs(w)
    keep = np.arange(len(c)) if keep is None else keep
    return D.estimate(w["local"][keep], R[keep], c[keep] * c_factor, w["frame_ids"][keep], lag, knot, **kw)


def worst_errors(w, r):
    """The worst error in distance from the start, metres: (of the metric track, of the trajectory at the one global scale)"""
    _, c = W.slam_inputs(w)
    true = np.sqrt(T.sq(w["head"] - w["head"][0]))
    return float(np.abs(np.sqrt(T.sq(r["metric"])) - true).max()), float(np.abs(np.sqrt(T.sq(r["global"]["scale"] * c)) - true).max())


# ------------------------------------------------------------------------------------------------- the cases the device is held to
@functools.lru_cache(maxsize=None)
def device_case(name):
    """-> dict(x, R, c, ids, lag, knot, min_pairs): the twin's and `drift_call`'s inputs"""
    n, lag, knot, min_pairs, keep, stand, seed = 600, LAG, 100, 50, None, (), 1
    if name == "two knots":
        n, min_pairs, seed = 37, 10, 2
    elif name == "lost rows":
        keep, seed = np.r_[0:200, 207:400, 402:600], 3
    elif name == "standing":
        stand, seed = ((190, 410),), 4
    elif name == "2048 knots":          # the solve's whole LDS: 4095 frames, a knot every second one
        n, lag, knot, min_pairs, seed = 4095, 1, 2, 0, 5
    else:
        assert name == "walker"
    w = W.walk(n, scale=creeping(n), noise=0.03, seed=seed, stand=stand)
    R, c = W.slam_inputs(w)
    keep = np.arange(n) if keep is None else keep
    return {"x": np.ascontiguousarray(w["local"][keep]), "R": R[keep], "c": c[keep], "ids": w["frame_ids"][keep], "lag": lag, "knot": knot,
            "min_pairs": min_pairs, "walk": w}


DEVICE_CASES = ("walker", "two knots", "lost rows", "standing", "2048 knots")


@functools.lru_cache(maxsize=None)
def device_twin(name, extended=False):
    k = device_case(name)
    return D.estimate(k["x"], k["R"], k["c"], k["ids"], k["lag"], k["knot"], min_pairs=k["min_pairs"], dtype=np.longdouble if extended else np.float64)


def spread(name):
    """How far float64 lies from extended precision on this case: the largest relative difference of the knot values"""
    a, b = device_twin(name)["knot_scale"], device_twin(name, True)["knot_scale"]
    return float(np.max(np.abs((a - b) / b)))


def knot_gate(name):
    """1e-12 relative where the spread is below 1e-13, ten times the spread otherwise"""
    s = spread(name)
    return 1e-12 if s < 1e-13 else 10.0 * s


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_margins_and_spread_of_the_device_cases(name):
    r = device_twin(name)
    k = device_case(name)
    print("%s: %d knots, curve %.6g .. %.6g, %d inliers, %d informative, margins %s, spread %.3g, gate %.3g" %
          (name, len(r["knot_scale"]), r["scale_min"], r["scale_max"], r["inliers"], r["informative"], r["margins"], spread(name), knot_gate(name)))
    assert all(v > MARGIN for v in r["margins"].values()), r["margins"]
    assert len(r["knot_scale"]) == {"walker": 7, "two knots": 2, "lost rows": 7, "standing": 7, "2048 knots": 2048}[name]
    assert np.finfo(np.longdouble).eps < 1e-18          # (extended precision is extended here)
    ext = device_twin(name, True)
    assert (ext["inliers"], ext["informative"]) == (r["inliers"], r["informative"]) and np.array_equal(ext["interval_count"], r["interval_count"])
    if name == "standing":          # intervals 2 and 3 lie inside the stand: their pairs are inliers that say nothing
        assert (r["interval_bb"][2:4] < 1e-20).all() and (r["interval_count"][2:4] > 0).all() and (r["interval_bb"][[0, 1, 4, 5]] > 0.1).all()
    if name == "lost rows":
        assert len(k["ids"]) == 591 and r["global"]["pairs"] == 591 - 3 * LAG


# ------------------------------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("seed", SEEDS)
def test_accuracy_against_the_one_scale(seed):
    n = 3000
    for name, scale, bound in (("creeping", creeping(n), 0.2), ("wandering", wandering(n), 0.2), ("constant", 1.7, 2.0)):
        w = W.walk(n, scale=scale, noise=0.03, seed=seed)
        drift, const = worst_errors(w, _twin(w, 250))
        print("seed %d, %s scale: worst error %.3f m with the curve, %.3f m with one scale (ratio %.3f, bound %.1f)" % (seed, name, drift, const, drift / const, bound))
        assert drift <= bound * const, name
    n = 600
    w = W.walk(n, scale=creeping(n), noise=0.03, seed=seed)
    drift, const = worst_errors(w, _twin(w, 100))
    print("seed %d, 600 frames: worst error %.3f m with the curve, %.3f m with one scale (ratio %.3f, bound 0.5)" % (seed, drift, const, drift / const))
    assert drift <= 0.5 * const


# --------------------------------------------------------------------------------------------------------------------- exact cases
def test_noise_free_constant_scale_comes_back():
    w = W.walk(600, scale=1.7)
    r = _twin(w, 100)
    err = float(np.abs(r["knot_scale"] / 1.7 - 1).max())
    print("noise-free, scale 1.7: knots %s, largest relative error %.3g" % (r["knot_scale"].tolist(), err))
    assert len(r["knot_scale"]) == 7 and err < 1e-12
    assert abs(r["scale_mean"] / 1.7 - 1) < 1e-12 and r["inliers"] == r["global"]["pairs"] == 595
    _, c = W.slam_inputs(w)
    assert np.abs(r["metric"] - 1.7 * c).max() < 1e-9


@pytest.mark.parametrize("factor", [4.0, 0.125])
def test_a_power_of_two_unit_changes_only_exponents(factor):
    n = 600
    w = W.walk(n, scale=creeping(n), noise=0.03, seed=5)
    one, other = _twin(w, 100), _twin(w, 100, c_factor=factor)
    assert np.array_equal(other["knot_scale"], one["knot_scale"] / factor) and other["lam"] == one["lam"] * factor * factor
    assert np.array_equal(other["metric"], one["metric"]) and other["metric_length"] == one["metric_length"]
    assert np.array_equal(other["interval_count"], one["interval_count"]) and np.array_equal(other["interval_bb"], one["interval_bb"] * factor * factor)
    for k in ("inliers", "informative", "residual_rms"):
        assert other[k] == one[k], k


# ---------------------------------------------------------------------------------------------------------------- standing and gaps
def test_a_stand_in_the_middle_is_interpolated():
    """600 of 3000 frames standing: intervals 5 and 6 (frames 1250 .. 1750) lie inside the stand, knot 6 has no informed neighbour.
    The accuracy asked of the walk above holds, and the knots in the stand lie on the line between their neighbours and at the true
    scale to the 5 % that tests/test_slam_scale_cpu.py asks of one scale on a walker that stands for most of the time."""
    n = 3000
    truth = creeping(n)
    w = W.walk(n, scale=truth, noise=0.03, seed=2, stand=[(1200, 1800)])
    r = _twin(w, 250)
    s, bb = r["knot_scale"], r["interval_bb"]
    assert (bb[5:7] < 1e-20).all() and (np.delete(bb, [5, 6]) > 0.1).all()
    drift, const = worst_errors(w, r)
    line = s[4] + (s[8] - s[4]) * np.array([0.25, 0.5, 0.75])
    print("stand 1200 .. 1800: knots %s, the line between knots 4 and 8 at knots 5 .. 7: %s, worst error %.3f m against %.3f m" %
          (s.tolist(), line.tolist(), drift, const))
    assert drift <= 0.2 * const
    assert np.abs(s[5:8] / line - 1).max() < 0.05 and np.abs(s[5:8] / truth[[1250, 1500, 1750]] - 1).max() < 0.05


def test_lost_rows_no_pair_and_the_midpoint_scale_across_a_gap():
    n = 600
    w = W.walk(n, scale=creeping(n), noise=0.03, seed=3)
    keep = np.r_[0:200, 207:400, 402:600]
    r = _twin(w, 100, keep)
    ids = w["frame_ids"][keep]
    t = r["pair_rows"]
    assert len(t) == len(keep) - 3 * LAG and (ids[t + LAG] - ids[t] == LAG).all()
    assert not set(range(195, 200)) & set(t.tolist()) and not set(range(388, 393)) & set(t.tolist())
    _, c = W.slam_inputs(w)
    c = c[keep]
    for i in (200, 393):          # the rows behind the two gaps
        assert ids[i] - ids[i - 1] > 1
        mid = 0.5 * (ids[i - 1] + ids[i])
        s = np.interp(mid, r["knot_ids"], r["knot_scale"])
        assert np.abs((r["metric"][i] - r["metric"][i - 1]) - s * (c[i] - c[i - 1])).max() <= 1e-12 * np.abs(r["metric"][i]).max()
    assert 0.5 * (ids[199] + ids[200]) == 203.0          # (inside interval 2, whose own pairs begin at frame 207)


# ------------------------------------------------------------------------------------------------------------------------- refusal
def one_interval_case():
    """100 frames that walk, then a line every seventh frame: no two of those are LAG apart, so every pair lies before knot 1"""
    n = 600
    w = W.walk(n, scale=creeping(n), noise=0.03, seed=6)
    return w, np.r_[0:100, 100:600:7]


def test_inliers_in_one_interval_only_are_refused_with_the_knots_named():
    w, keep = one_interval_case()
    with pytest.raises(T.Refusal, match=r"no inlier pairs between knots 1-2, 2-3, 3-4, 4-5, 5-6 \(7 knots, 1 intervals") as e:
        _twin(w, 100, keep, min_pairs=20)
    assert e.value.code == D.NOT_SOLVED and e.value.report["interval_count"][0] > 50 and not e.value.report["interval_count"][1:].any()
    # the same pairs under two knots are one interval that holds them all: no refusal
    r = _twin(w, 600, keep, min_pairs=20)
    assert len(r["knot_scale"]) == 2 and r["interval_count"][0] > 50
    # the global estimate's refusals come first, as they are
    with pytest.raises(T.Refusal, match="did not walk enough") as e:
        _twin(w, 100, min_pairs=10000)
    assert e.value.code == T.TOO_FEW


# ---------------------------------------------------------------------------------------------------------------------- host logic
def test_scale_arg_and_the_options():
    import argparse
    from globalegomocap_amd import continuous, detections, prepare, slam_scale
    assert slam_scale.scale_arg("drift") == "drift" and slam_scale.scale_arg("auto") == "auto" and slam_scale.scale_arg("2") == 2.0
    with pytest.raises(argparse.ArgumentTypeError):
        slam_scale.scale_arg("Drift")
    assert prepare.gt_or_scale(None, "drift") == "drift"
    with pytest.raises(ValueError):
        prepare.gt_or_scale("gt.pkl", "drift")          # the ground-truth route refuses it the way it refuses `auto`
    assert slam_scale.default_knot(25) == 250 and slam_scale.default_knot(30) == 300
    base = ["--slam", "t.txt", "--start", "0", "--end", "100"]
    for module, more in ((prepare, ["--heatmaps", "h", "--depths", "d", "--out", "o"]), (detections, ["--keypoints", "k.npz", "--out", "o"])):
        p = module._parser()
        a = prepare.parse_recording_options(p, base + more + ["--scale", "drift", "--knot", "4", "--stiffness", "0.5"])
        assert a.scale == "drift" and slam_scale.drift_options(p, a) == {"knot": 100, "stiffness": 0.5}
        a = prepare.parse_recording_options(p, base + more + ["--scale", "drift"])
        assert slam_scale.drift_options(p, a) == {"knot": None, "stiffness": 1.0}
        for bad in (["--scale", "auto", "--knot", "4"], ["--scale", "1.5", "--stiffness", "2"], ["--scale", "drift", "--knot", "0"],
                    ["--scale", "drift", "--stiffness", "-1"], ["--gt", "g", "--scale", "drift"]):
            with pytest.raises(SystemExit):
                slam_scale.drift_options(p, prepare.parse_recording_options(p, base + more + bad))
    a = continuous.parse_args(base + ["--keypoints", "k.npz", "--scale", "drift", "--knot", "2"])
    assert a.scale == "drift" and a.drift == {"knot": 50, "stiffness": 1.0}
    assert continuous.parse_args(base + ["--keypoints", "k.npz", "--scale", "auto"]).drift == {"knot": None, "stiffness": 1.0}
    with pytest.raises(SystemExit):
        continuous.parse_args(base + ["--keypoints", "k.npz", "--scale", "2", "--knot", "2"])
    a = slam_scale._parser().parse_args(base + ["--keypoints", "k.npz", "--scale", "drift", "--knot", "4"])
    assert a.scale == "drift" and slam_scale._parser().parse_args(base + ["--keypoints", "k.npz"]).scale == "auto"
    from globalegomocap_amd import live
    with pytest.raises(SystemExit):          # a live session needs its scale before the first window
        live._parser().parse_args(["--scale", "drift"])


def test_metric_rows_round_trip_through_relative_poses():
    from globalegomocap_amd import _capi, slam, slam_scale
    n, fps = 50, 25
    rng = np.random.default_rng(0)
    w = W.walk(n, scale=1.3)
    ids = w["frame_ids"] + 40
    metric = np.concatenate([np.zeros((1, 3)), np.cumsum(rng.normal(0.0, 0.05, (n - 1, 3)), axis=0)])
    _, rq = slam.relative_poses(w["rows"][:, 1:4], w["rows"][:, 4:8])
    report = np.zeros(_capi.DRIFT_REPORT_DOUBLES)
    report[[1, 2, 9, 13]] = 2, 100, 1.25, 40
    est = slam_scale.DriftEstimate(report, [[1.2, 45, 3.0, 0], [1.3, 0, 0, 0]], metric, slam_scale.ScaleEstimate(np.zeros(19)), ids, fps, rq)
    rows = est.metric_rows()
    assert rows.shape == (n, 8) and np.array_equal(slam.frame_ids(rows, fps), ids)
    rt, rq2 = slam.relative_poses(rows[:, 1:4], rows[:, 4:8])
    assert np.array_equal(rt, metric)          # the metric track itself, bit for bit
    assert np.abs(np.abs(np.sum(rq2 * rq, axis=1)) - 1).max() < 1e-14
    assert est.scale == est.scale_mean == 1.25 and est.knot_ids.tolist() == [40, 140] and est.interval_count.tolist() == [45]
    d = est.as_dict()
    assert d["knot_scale"] == [1.2, 1.3] and d["knot_ids"] == [40, 140] and d["scale"] == 1.25
    lines = est.knot_lines()
    assert len(lines) == 2 and lines[0].startswith("knot 0 at frame 40: scale 1.2") and "45 inlier pairs" in lines[0]
    assert "1.2 .. 1.3" not in est.line() and est.line().startswith("SLAM scale drift: 0 .. 0 over 2 knots 100 frames apart")


def test_walk_with_one_scale_per_frame():
    n = 300
    one = W.walk(n, scale=1.7, noise=0.03, seed=1)
    many = W.walk(n, scale=np.full(n, 1.7), noise=0.03, seed=1)
    assert np.array_equal(one["rows"][:, [0, 4, 5, 6, 7]], many["rows"][:, [0, 4, 5, 6, 7]]) and np.array_equal(one["local"], many["local"])
    # the running sum of n steps against the positions themselves: the standard bound of a sum of n terms
    bound = 2 * n * np.finfo(np.float64).eps * np.abs(one["rows"][:, 1:4]).max()
    assert np.abs(one["rows"][:, 1:4] - many["rows"][:, 1:4]).max() <= bound
    assert isinstance(one["scale"], float) and many["scale"].shape == (n,)
    # a drifting scale: the SLAM steps are the head's steps divided by the two frames' mean scale
    s = creeping(n)
    w = W.walk(n, scale=s)
    _, c = W.slam_inputs(w)
    steps = np.sqrt(T.sq(np.diff(w["head"], axis=0))) / np.sqrt(T.sq(np.diff(c, axis=0)))
    assert np.abs(steps / (0.5 * (s[1:] + s[:-1])) - 1).max() < 1e-9
    with pytest.raises(ValueError):
        W.walk(n, scale=np.ones(n - 1))


def test_report_record_layout_and_declarations():
    import ctypes as C
    from globalegomocap_amd import _capi
    header = open(os.path.join(ROOT, "include", "gem_hip.h")).read()
    body = re.search(r"typedef struct gem_drift_report \{(.*?)\} gem_drift_report;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"double ([^;]*);", body) for n in decl.split(",")]
    assert names == [f[0] for f in _capi.GemDriftReport._fields_]
    assert C.sizeof(_capi.GemDriftReport) == 8 * len(names) == 8 * _capi.DRIFT_REPORT_DOUBLES
    for macro, value in (("GEM_DRIFT_MAX_KNOTS", _capi.DRIFT_MAX_KNOTS), ("GEM_DRIFT_REPORT_DOUBLES", _capi.DRIFT_REPORT_DOUBLES),
                         ("GEM_DRIFT_NOT_SOLVED", _capi.DRIFT_NOT_SOLVED)):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value, macro
    assert (_capi.DRIFT_MAX_KNOTS, _capi.DRIFT_NOT_SOLVED) == (D.MAX_KNOTS, D.NOT_SOLVED)
    assert _capi.DRIFT_NOT_SOLVED not in (_capi.SCALE_NO_PAIRS, _capi.SCALE_TOO_FEW, _capi.SCALE_BAD_SCALE, 0, 1)
    for name in ("gem_slam_drift_work", "gem_slam_drift"):
        n_args = len(re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header).group(1).split(","))
        assert len(_capi.SIGNATURES[name][1]) == n_args, name
    src = open(os.path.join(ROOT, "globalegomocap_amd", "csrc", "errors.hip")).read()
    assert src.count('#include "slam_drift.h"') == 1 and src.index('#include "slam_scale.h"') < src.index('#include "slam_drift.h"')


def test_work_size_needs_no_gpu():
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import _capi
    lib = _capi.load_library()
    small, large = lib.gem_slam_drift_work(600, 5, 7), lib.gem_slam_drift_work(100000, 5, 401)
    assert lib.gem_slam_scale_work(600, 5, 1) < small < large < 64 << 20 and lib.gem_slam_drift_work(5, 5, 2) == 8
    assert lib.gem_slam_drift_work(600, 5, 2049) == -1 and b"n_knots" in lib.gem_last_error()
    assert lib.gem_slam_drift_work(600, 5, 1) == -1 and lib.gem_slam_drift_work(0, 5, 2) == -1
