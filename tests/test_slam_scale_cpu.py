"""The SLAM-scale estimator without a GPU: the numpy twin (tests/slam_scale_twin.py) on the synthetic walker
(`synth_walk`), the `--scale` parsers of `prepare` and `detections`, and the report record's layout."""
import os
import re

import numpy as np
import pytest

import slam_scale_twin as T
from globalegomocap_amd import synth_walk as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAG = 5          # max(1, round(0.2 * 25)); the walker's feet both stand for stance - step + 1 = 5 frames at every change-over

# The twin's relative error on the noisy walker below (3 cm on every coordinate, 2000 frames, scale 1.7, seeds 1, 2, 3), measured on
# the CPU: 7.554e-4, 6.893e-4, 5.882e-4.  The bound is the largest one plus half of it, because the seeds are few.
NOISY_SEEDS = (1, 2, 3)
NOISY_BOUND = 1.5 * 7.554e-4


def _twin(w, lag=LAG, c_factor=1.0, **kw):
    R, c = W.slam_inputs(w)
    return T.estimate(w["local"], R, c * c_factor, w["frame_ids"], lag, **kw)


@pytest.mark.parametrize("scale", [0.37, 2.5])
def test_noise_free_walker_gives_its_scale(scale):
    w = W.walk(40, scale=scale)
    assert w["stance"] - w["step"] + 1 >= LAG          # of two frames LAG apart, one foot stands in both
    r = _twin(w, min_pairs=20)
    print("scale %r: estimate %r, relative error %.3g, residual RMS %.3g" % (scale, r["scale"], abs(r["scale"] / scale - 1), r["residual_rms"]))
    assert abs(r["scale"] / scale - 1) < 1e-12
    assert r["pairs"] == r["inliers"] == r["informative"] == 35 and r["residual_rms"] < 1e-12
    chords = np.linalg.norm(w["head"][LAG:] - w["head"][:-LAG], axis=1)          # the path in metres: the pairs' chords, each counted 1 / LAG
    assert abs(r["path_length"] / (np.sum(chords) / LAG) - 1) < 1e-9


def test_stance_feet_are_exactly_stationary():
    w = W.walk(120, scale=1.3, noise=0.0)
    for side in range(2):
        st = w["standing"][:, side]
        both = st[1:] & st[:-1] & (np.abs(w["feet"][1:, side] - w["feet"][:-1, side]).max(axis=1) < 0.2)      # (same stance, not the next one)
        assert both.sum() > 40 and np.array_equal(w["feet"][1:, side][both], w["feet"][:-1, side][both])
    assert (w["standing"].any(axis=1)).all()
    # a function of the parameters alone
    again = W.walk(120, scale=1.3, noise=0.0)
    assert all(np.array_equal(w[k], again[k]) for k in ("feet", "head", "local", "rows", "cams"))
    # the local poses are the world's joints seen from the camera: the foot points come back through the true cameras
    mid = 0.5 * (w["local"][:, [9, 13]] + w["local"][:, [10, 14]])
    back = np.einsum("nij,nsj->nsi", w["cams"][:, :3, :3], mid) + w["cams"][:, None, :3, 3]
    assert np.abs(back - w["feet"]).max() < 1e-12


@pytest.mark.parametrize("factor", [4.0, 0.125])
def test_a_power_of_two_unit_divides_the_estimate_exactly(factor):
    w = W.walk(400, scale=1.7, noise=0.03, seed=5)
    one, other = _twin(w), _twin(w, c_factor=factor)
    assert other["scale"] == one["scale"] / factor and other["s0"] == one["s0"] / factor and other["s_ref"] == one["s_ref"] / factor
    assert other["g0"] == one["g0"] and np.array_equal(other["costs"], one["costs"])
    for k in ("pairs", "inliers", "informative", "residual_rms", "path_length", "stance_share"):
        assert other[k] == one[k], k


def test_another_slam_world_changes_nothing():
    a = W.walk(300, scale=1.7, noise=0.03, seed=6)
    b = W.walk(300, scale=1.7, noise=0.03, seed=6, world_rotation=(-1.1, 0.4, 2.0), world_offset=(-7.0, 3.0, 11.0))
    assert np.array_equal(a["local"], b["local"]) and not np.allclose(a["rows"][:, 1:], b["rows"][:, 1:])
    ra, rb = _twin(a), _twin(b)
    print("two SLAM worlds: %r %r" % (ra["scale"], rb["scale"]))
    assert abs(ra["scale"] / rb["scale"] - 1) < 1e-12
    assert (ra["pairs"], ra["inliers"], ra["informative"], ra["g0"]) == (rb["pairs"], rb["inliers"], rb["informative"], rb["g0"])


def test_noisy_walker_within_the_measured_bound():
    errs = []
    for seed in NOISY_SEEDS:
        r = _twin(W.walk(2000, scale=1.7, noise=0.03, seed=seed))
        errs.append(abs(r["scale"] / 1.7 - 1))
        print("seed %d: estimate %r, relative error %.4g, %d pairs, %d inliers, %d informative, residual RMS %.4f" %
              (seed, r["scale"], errs[-1], r["pairs"], r["inliers"], r["informative"], r["residual_rms"]))
        assert r["inliers"] >= 0.5 * r["pairs"]
    assert max(errs) <= NOISY_BOUND


def test_a_wearer_who_stands_still_is_refused():
    w = W.walk(300, scale=1.7, noise=0.0, stand=[(0, 300)])
    assert np.ptp(w["head"], axis=0).max() == 0.0 and np.ptp(w["cams"][:, :3, :3], axis=0).max() > 0.1          # (the head still turns)
    with pytest.raises(T.Refusal) as e:
        _twin(w)
    assert e.value.report["informative"] == 0 and e.value.code in (T.NO_PAIRS, T.TOO_FEW)
    noisy = W.walk(300, scale=1.7, noise=0.03, seed=2, stand=[(0, 300)])
    with pytest.raises(T.Refusal) as e:
        _twin(noisy)
    assert e.value.report["informative"] == 0
    # standing for 60 % of the time still fixes the scale
    part = W.walk(600, scale=1.7, noise=0.03, seed=2, stand=[(100, 460)])
    r = _twin(part)
    print("standing for 360 of 600 frames: estimate %r, %d informative of %d pairs" % (r["scale"], r["informative"], r["pairs"]))
    assert r["informative"] >= 50 and abs(r["scale"] / 1.7 - 1) < 0.05
    with pytest.raises(T.Refusal, match="did not walk enough") as e:
        _twin(part, min_pairs=r["informative"] + 1)
    assert e.value.code == T.TOO_FEW


def test_no_pair_spans_a_hole_in_the_frame_ids():
    w = W.walk(100, scale=1.7, noise=0.03, seed=3)
    keep = np.r_[0:30, 37:60, 62:100]                       # runs of 30, 23 and 38 frames
    R, c = W.slam_inputs(w)
    q = T.foot_points(w["local"][keep], R[keep])
    a, b, t = T.pairs(q, c[keep], w["frame_ids"][keep], LAG)
    assert len(t) == (30 - LAG) + (23 - LAG) + (38 - LAG)
    ids = w["frame_ids"][keep]
    assert (ids[t + LAG] - ids[t] == LAG).all()
    assert not set(range(25, 30)) & set(t.tolist()) and not set(range(48, 53)) & set(t.tolist())          # the last LAG rows of a run start no pair
    r = T.estimate(w["local"][keep], R[keep], c[keep], ids, LAG, min_pairs=20)
    assert r["pairs"] == len(t)
    with pytest.raises(T.Refusal) as e:
        T.estimate(w["local"][:LAG], R[:LAG], c[:LAG], w["frame_ids"][:LAG], LAG)
    assert e.value.code == T.NO_PAIRS


@pytest.mark.parametrize("module", ["prepare", "detections"])
def test_scale_option_of_the_parsers(module, capsys):
    import importlib
    m = importlib.import_module("globalegomocap_amd." + module)
    base = ["--slam", "t.txt", "--start", "0", "--end", "10"] + (["--heatmaps", "h", "--depths", "d"] if module == "prepare" else ["--keypoints", "k.npz"])
    a = m._parser().parse_args(base + ["--scale", "1.5"])
    assert a.scale == 1.5 and isinstance(a.scale, float) and a.gt is None
    assert m._parser().parse_args(base + ["--scale", "auto"]).scale == "auto"
    assert m._parser().parse_args(base + ["--gt", "g"]).scale is None
    for bad in (["--gt", "g", "--scale", "auto"], ["--scale", "-1"], ["--scale", "nan"], ["--scale", "foo"], ["--scale", "0"], ["--scale", "inf"]):
        with pytest.raises(SystemExit):
            m._parser().parse_args(base + bad)
    capsys.readouterr()


def test_gt_or_scale_passes_auto_through():
    from globalegomocap_amd import prepare
    assert prepare.gt_or_scale(None, "auto") == "auto"
    assert prepare.gt_or_scale(None, 2) == 2.0 and isinstance(prepare.gt_or_scale(None, 2), float)
    assert prepare.gt_or_scale("g", None) is None
    for gt, scale in (("g", "auto"), (None, None), (None, "Auto"), (None, -1.0), (None, float("nan"))):
        with pytest.raises(ValueError):
            prepare.gt_or_scale(gt, scale)
    stage = prepare.RecordingStage(prepare.CameraRoute(scale=1.25), [], 25)
    stage.fix_scale(None, None)
    assert (stage.scale, stage.scale_report) == (1.25, None)
    rec = prepare.Recording([])
    assert rec.scale is None and rec.scale_report is None


def test_report_record_layout_and_declarations():
    import ctypes as C
    from globalegomocap_amd import _capi, slam_scale
    header = open(os.path.join(ROOT, "include", "gem_hip.h")).read()
    body = re.search(r"typedef struct gem_scale_report \{(.*?)\} gem_scale_report;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"double ([^;]*);", body) for n in decl.split(",")]
    assert names == [f[0] for f in _capi.GemScaleReport._fields_]
    assert C.sizeof(_capi.GemScaleReport) == 8 * len(names) == 8 * _capi.SCALE_REPORT_DOUBLES
    for macro, value in (("GEM_SCALE_CANDIDATES", _capi.SCALE_CANDIDATES), ("GEM_SCALE_TILE", _capi.SCALE_TILE),
                         ("GEM_SCALE_REPORT_DOUBLES", _capi.SCALE_REPORT_DOUBLES), ("GEM_SCALE_NO_PAIRS", _capi.SCALE_NO_PAIRS),
                         ("GEM_SCALE_TOO_FEW", _capi.SCALE_TOO_FEW), ("GEM_SCALE_BAD_SCALE", _capi.SCALE_BAD_SCALE)):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value, macro
    assert (_capi.SCALE_NO_PAIRS, _capi.SCALE_TOO_FEW, _capi.SCALE_BAD_SCALE, _capi.SCALE_CANDIDATES) == (T.NO_PAIRS, T.TOO_FEW, T.BAD_SCALE, T.N_CAND)
    for name in ("gem_slam_scale_work", "gem_slam_scale"):
        n_args = len(re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header).group(1).split(","))
        assert len(_capi.SIGNATURES[name][1]) == n_args, name
    src = open(os.path.join(ROOT, "globalegomocap_amd", "csrc", "errors.hip")).read()
    assert src.count('#include "slam_scale.h"') == 1
    assert slam_scale.FEET == T.FEET == (9, 10, 13, 14) and slam_scale.default_lag(25) == LAG and slam_scale.default_lag(2) == 1
    # the record as Python reads it
    rep = np.arange(16 + 6, dtype=np.float64)
    est = slam_scale.ScaleEstimate(rep)
    assert (est.scale, est.s0, est.s_ref, est.g0, est.pairs, est.inliers, est.informative) == (0.0, 1.0, 2.0, 3, 4, 5, 6)
    assert est.stance_share == (9.0, 10.0) and est.per_chunk.tolist() == [18.0, 21.0] and est.as_dict()["per_chunk"] == [18.0, 21.0]


def test_work_size_needs_no_gpu():
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import _capi
    lib = _capi.load_library()
    small, large = lib.gem_slam_scale_work(100, 5, 1), lib.gem_slam_scale_work(100000, 5, 1000)
    assert 0 < small < large < 64 << 20 and lib.gem_slam_scale_work(5, 5, 1) == 8
    assert lib.gem_slam_scale_work(0, 5, 1) == -1 and b"n_frames" in lib.gem_last_error()
