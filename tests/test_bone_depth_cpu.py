"""Depths from bone lengths on the host: the numpy twin of gem_bone_depths against the truth of generated poses,
its handling of missing joints, the option handling, the report's arithmetic, the command lines, the ABI."""
import os
import re

import numpy as np
import pytest

import bone_depth_twin as BT
from globalegomocap_amd.camera import DEFAULT_CALIBRATION, FisheyeCamera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2024


@pytest.fixture(scope="module")
def cam():
    return FisheyeCamera.from_json(DEFAULT_CALIBRATION)


@pytest.fixture(scope="module")
def opts():
    from globalegomocap_amd import bone_depth as B
    return B.options()


# ------------------------------------------------------------------------------------------------------------------ accuracy
# (sigma, ray noise, mean MPJPE allowed in mm, share of frames allowed above 50 mm); the thresholds are the issue's, from its CPU
# prototype's 0.4 / 2.3 / 6.7 / 16.8 mm with margin.  Measured with the final settings (30 iterations, w_n = 100, w_m = 1e-3,
# lambda 1e-3 x 0.1 / x 10, seed 2024, 200 frames): 0.39 mm; 2.36 mm; 6.48 mm, none above 50 mm (worst 19.2 mm); 16.39 mm, none
# above 50 mm (worst 29.7 mm).
ACCURACY = [(0.15, 0.0, 1.0, None), (0.3, 0.0, 5.0, None), (0.3, 0.003, 10.0, 0.0), (0.3, 0.010, 25.0, 0.05)]


@pytest.mark.parametrize("sigma,noise,mean_mm,share", ACCURACY, ids=["sigma 0.15", "sigma 0.3", "sigma 0.3 noise 0.003", "sigma 0.3 noise 0.010"])
def test_twin_against_truth(cam, opts, sigma, noise, mean_mm, share, capsys):
    rng = np.random.default_rng(SEED)
    truth = BT.poses(200, sigma, rng)
    kp = BT.detect(truth, cam, noise, rng)
    if not noise:          # the generator's detections are the poses' rays
        np.testing.assert_allclose(BT.rays(kp, cam), truth / np.linalg.norm(truth, axis=-1, keepdims=True), rtol=0, atol=1e-12)
    depth, solved, rms = BT.solve(kp, cam, opts)
    err = BT.mpjpe(BT.positions(kp, depth, cam), truth)
    with capsys.disabled():
        print("sigma %.2f, ray noise %.3f: mean MPJPE %.2f mm, worst frame %.1f mm, %d of 200 frames above 50 mm, median rms %.2f mm"
              % (sigma, noise, err.mean() * 1e3, err.max() * 1e3, (err > 0.05).sum(), np.median(rms) * 1e3))
    assert solved.all() and (depth >= BT.FLOOR).all() and np.isfinite(depth).all()
    assert err.mean() * 1e3 <= mean_mm
    if share is not None:
        assert (err > 0.05).sum() <= share * 200


def test_twin_scales_with_the_skeleton(cam):
    """bones= 5 % longer: dbar and the anchor scale by sum(L) / sum(L_rest), and so does the pose (the rays are the same)."""
    from globalegomocap_amd import bone_depth as B
    base, big = B.options(), B.options(bones=B.options()["L"] * 1.05)
    np.testing.assert_allclose(big["dbar"], base["dbar"] * 1.05, rtol=1e-14)
    assert big["neck_depth"] == pytest.approx(base["neck_depth"] * 1.05, rel=1e-14)
    rng = np.random.default_rng(SEED)
    kp = BT.detect(BT.poses(20, 0.3, rng), cam)
    a, b = BT.solve(kp, cam, base)[0], BT.solve(kp, cam, big)[0]
    np.testing.assert_allclose(b, a * 1.05, rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ missing joints
def test_missing_joints(cam, opts):
    rng = np.random.default_rng(SEED + 1)
    kp = BT.detect(BT.poses(4, 0.3, rng), cam, 0.003, rng, conf=0.7)
    full = BT.solve(kp, cam, opts)
    assert full[1].all() and (full[2] > 0).all()
    # elbow (2) unusable: the wrist (3) is cut off; both keep their prior depth and are unsolved
    lost = kp.copy()
    lost[:, 2, 2] = 0.0
    depth, solved, rms = BT.solve(lost, cam, opts)
    want = np.ones(15, dtype=np.uint8)
    want[[2, 3]] = 0
    assert (solved == want).all()
    assert np.array_equal(depth[:, [2, 3]], np.broadcast_to(opts["dbar"][[2, 3]], (4, 2)))
    # ... and every other joint has the bytes of the reduced problem: here, the problem with the wrist lost as well (the wrist's own
    # detection plays no part), and with the lost detections replaced by rubbish
    also = lost.copy()
    also[:, 3] = (np.nan, 1e9, 0.5)
    also[:, 2, :2] = (-5.0, 7e5)
    d2, s2, r2 = BT.solve(also, cam, opts)
    assert np.array_equal(d2, depth) and np.array_equal(s2, solved) and np.array_equal(r2, rms)
    assert not np.array_equal(depth[:, 1], full[0][:, 1])          # (the shoulder lost a bone equation: another problem)
    # neck unusable: the whole frame is unsolved, at its prior depths, rms 0; the other frames are untouched by it
    noneck = kp.copy()
    noneck[1, 0, 0] = np.inf
    depth, solved, rms = BT.solve(noneck, cam, opts)
    assert not solved[1].any() and np.array_equal(depth[1], opts["dbar"]) and rms[1] == 0.0
    for f in (0, 2, 3):
        assert np.array_equal(depth[f], full[0][f]) and solved[f].all() and rms[f] == full[2][f]
    # the usable rule, one way of being unusable per frame: NaN confidence, negative confidence, NaN u, infinite v
    odd = kp.copy()
    odd[0, 14, 2], odd[1, 14, 2], odd[2, 14, 0], odd[3, 14, 1] = np.nan, -0.1, np.nan, -np.inf
    from globalegomocap_amd import bone_depth as B
    depth, solved, _ = BT.solve(odd, cam, opts)
    assert not solved[:, 14].any() and solved[:, :14].all() and np.array_equal(depth[:, 14], np.full(4, opts["dbar"][14]))
    assert np.array_equal(B.solved_mask(odd), solved.astype(bool)) and np.array_equal(B.solved_mask(lost), BT.solved_mask(lost))
    # a frame is solved on its own
    alone = BT.solve(kp[2:3], cam, opts)
    assert np.array_equal(alone[0][0], full[0][2]) and alone[2][0] == full[2][2]


def test_the_device_tests_cases_are_well_conditioned(cam, opts, capsys):
    """The cases of tests/test_bone_depth_gpu.py, on the twin alone: no more than 2 % of the frames are left out of the device
    comparison as ill-conditioned (the float64 and the longdouble twin more than 1e-9 m apart), and the gate that follows."""
    total = out = 0
    worst = 0.0
    for n in BT.CASE_SIZES:
        kp = BT.cases(n, cam)
        d, s, rms = BT.solve(kp, cam, opts)
        dl, sl, rl = BT.solve(kp, cam, opts, np.longdouble)
        assert np.array_equal(s, sl)
        spread = np.maximum(np.abs(d - dl).max(axis=1), np.abs(rms - rl)).astype(np.float64)
        keep = spread <= BT.ILL_CONDITIONED
        total, out, worst = total + n, out + int((~keep).sum()), max(worst, float(spread[keep].max()))
    with capsys.disabled():
        print("device cases: %d of %d frames ill-conditioned, largest spread of the others %.3g m: gate %.3g m" % (out, total, worst, 16 * worst))
    assert out <= 0.02 * total and 0 < worst <= BT.ILL_CONDITIONED


# ------------------------------------------------------------------------------------------------------------------ host-side behaviour
def test_options():
    from globalegomocap_amd import bone_depth as B
    from globalegomocap_amd.skeleton import mean_bone_length_mm
    o = B.options()
    assert o["neck_depth"] == pytest.approx(0.2929, abs=1e-4) and (o["w_n"], o["w_m"], o["iters"]) == (100.0, 1e-3, 30)
    np.testing.assert_allclose(o["L"], mean_bone_length_mm() / 1000.0, rtol=1e-14)
    assert o["L"][0] == 0 and o["dbar"][0] == o["neck_depth"] and o["dbar"].shape == (15,)
    L = o["L"].copy()
    L[3] *= 2.0
    s = L.sum() / o["L"].sum()
    scaled = B.options(bones=L)
    assert np.array_equal(scaled["L"], L)
    np.testing.assert_allclose(scaled["dbar"], o["dbar"] * s, rtol=1e-15)
    assert scaled["neck_depth"] == pytest.approx(o["neck_depth"] * s, rel=1e-15)
    fixed = B.options(bones=L, neck_depth=0.31, iters=12)
    assert fixed["neck_depth"] == 0.31 and fixed["iters"] == 12 and np.array_equal(fixed["dbar"], scaled["dbar"])
    rest = B.rest_skeleton() * 1.1
    np.testing.assert_allclose(B.options(rest=rest)["L"], o["L"] * 1.1, rtol=1e-14)
    bad_bones = {"shape": L[:14], "rank": L[None], "nan": np.where(np.arange(15) == 4, np.nan, L), "inf": np.where(np.arange(15) == 4, np.inf, L),
                 "negative": np.where(np.arange(15) == 4, -0.1, L), "entry 0": np.where(np.arange(15) == 0, 0.1, L), "all zero": np.zeros(15)}
    for name, b in bad_bones.items():
        with pytest.raises(ValueError, match="bones"):
            B.options(bones=b)
    for nd in (0.0, -0.3, np.nan, np.inf):
        with pytest.raises(ValueError, match="neck_depth"):
            B.options(neck_depth=nd)
    for r in (rest[:14], np.where(np.arange(15)[:, None] == 2, np.nan, rest), np.zeros((15, 3))):
        with pytest.raises(ValueError, match="rest"):
            B.options(rest=r)
    for it in (0, 1001):
        with pytest.raises(ValueError, match="iters"):
            B.options(iters=it)


def test_the_reports_arithmetic():
    from globalegomocap_amd import bone_depth as B
    # 6 frames: 70 joints solved, 5 frames with a neck
    r = B.BoneDepthReport.from_record(6, (70.0, 5.0, 0.004, 0.031))
    assert r.as_dict() == {"frames": 6, "solved": 70, "unsolved": 20, "frames_without_neck": 1, "rms_median": 0.004, "rms_max": 0.031}
    assert list(r.as_dict()) == list(B.BoneDepthReport.FIELDS)
    assert r.line() == ("depths from bone lengths: 6 frames, 70 of 90 joints solved, 1 frames without a neck, bone residual rms median 4.0 mm, "
                        "max 31.0 mm")
    import json
    assert json.loads(json.dumps(r.as_dict())) == r.as_dict()
    # `summarize` on a made-up result (torch on the host does what it does on the device)
    import torch
    solved = torch.ones(5, 15, dtype=torch.uint8)
    solved[1] = 0                      # no neck
    solved[2, 1:] = 0                  # a neck and nothing else: no bone, its rms does not count
    solved[3, [2, 3]] = 0
    rms = torch.tensor([0.003, 0.0, 0.5, 0.009, 0.001], dtype=torch.float64)
    got = B.summarize(solved, rms).as_dict()
    assert got == {"frames": 5, "solved": 15 + 0 + 1 + 13 + 15, "unsolved": 75 - 44, "frames_without_neck": 1, "rms_median": 0.003, "rms_max": 0.009}
    assert B.summarize(solved[:0], rms[:0]).as_dict()["frames"] == 0
    assert B.summarize(solved[1:2], rms[1:2]).as_dict() == {"frames": 1, "solved": 0, "unsolved": 15, "frames_without_neck": 1, "rms_median": 0.0,
                                                            "rms_max": 0.0}


def test_command_lines(tmp_path):
    from globalegomocap_amd import bone_depth as B, detections as D, live as L
    base = ["--slam", "t", "--keypoints", "k.npz", "--scale", "1.0", "--start", "0", "--end", "101"]
    a = D._parser().parse_args(base + ["--depth_from", "bones", "--bones", "b.npy", "--neck_depth", "0.3"])
    assert (a.depth_from, a.bones, a.neck_depth, a.depth, a.depths) == ("bones", "b.npy", 0.3, None, None)
    a = D._parser().parse_args(base)
    assert (a.depth_from, a.bones, a.neck_depth) == (None, None, None)
    for other in (["--depth", "d.npy"], ["--depths", "DIR"]):
        with pytest.raises(SystemExit):
            D._parser().parse_args(base + ["--depth_from", "bones"] + other)
    with pytest.raises(SystemExit):
        D._parser().parse_args(base + ["--depth_from", "network"])
    with pytest.raises(SystemExit):
        D._cli(base + ["--bones", "b.npy"])                          # --bones without --depth_from bones
    live = ["--slam", "t", "--keypoints", "k.npz", "--start", "0", "--end", "10"]
    a = L._parser().parse_args(live + ["--depth_from", "bones", "--neck_depth", "0.28"])
    assert (a.depth_from, a.bones, a.neck_depth) == ("bones", None, 0.28)
    with pytest.raises(SystemExit):
        L._cli(live + ["--depth_from", "bones", "--depths", "DIR"])
    with pytest.raises(SystemExit):
        L._cli(["--slam", "t", "--heatmaps", "H", "--depths", "DIR", "--start", "0", "--end", "10", "--depth_from", "bones"])
    with pytest.raises(SystemExit):
        L._cli(live + ["--neck_depth", "0.28"])
    a = B._parser().parse_args(["--keypoints", "k.npz", "--out", "depth.npy", "--json", "r.json", "--bones", "b.npy"])
    assert (a.keypoints, a.out, a.json, a.bones, a.neck_depth, a.camera) == ("k.npz", "depth.npy", "r.json", "b.npy", None, DEFAULT_CALIBRATION)
    np.save(tmp_path / "b.npy", np.arange(15.0) / 10)
    assert np.array_equal(B.bones_from_args(B._parser().parse_args(["--keypoints", "k", "--bones", str(tmp_path / "b.npy")])), np.arange(15.0) / 10)


def test_the_route_is_opt_in():
    """Without depths and without depth="bones": today's ValueError, word for word; the new arguments are checked before any device work."""
    from globalegomocap_amd import detections as D, live as L
    kp = np.concatenate([np.random.default_rng(0).uniform(200, 1000, (4, 15, 2)), np.ones((4, 15, 1))], axis=2)
    with pytest.raises(ValueError, match=r"^recording_from_detections: the joints' depths are needed \(depth=, or `depth` in the \.npz\)$"):
        D.recording_from_detections("traj.txt", kp, scale=1.0, spans=[(0, 4)])
    with pytest.raises(ValueError, match='"bones"'):
        D.recording_from_detections("traj.txt", kp, scale=1.0, spans=[(0, 4)], depth="network")
    with pytest.raises(ValueError, match="neck_depth"):
        D.recording_from_detections("traj.txt", kp, scale=1.0, spans=[(0, 4)], depth="bones", neck_depth=-1.0)
    with pytest.raises(ValueError, match='belong to depth="bones"'):
        D.recording_from_detections("traj.txt", kp, scale=1.0, spans=[(0, 4)], depth=np.ones((4, 15)), bones=np.zeros(15))
    with pytest.raises(ValueError, match="bones"):
        L.LiveOptimizer(DEFAULT_CALIBRATION, bones_for_depth=np.ones(14))
    from globalegomocap_amd import prepare as P
    assert P.Recording([]).depth_report is None


def test_the_header_declares_what_is_bound():
    import ctypes as C
    from globalegomocap_amd import _capi
    header = open(os.path.join(ROOT, "include", "gem_hip.h")).read()
    n_args = len(re.search(r"\b%s\s*\(([^;]*)\)\s*;" % "gem_bone_depths", header).group(1).split(","))
    assert len(_capi.SIGNATURES["gem_bone_depths"][1]) == n_args == 10
    src = open(os.path.join(ROOT, "globalegomocap_amd", "csrc", "errors.hip")).read()
    assert src.count('#include "bone_depth.h"') == 1 and src.index('#include "keypoints.h"') < src.index('#include "bone_depth.h"')
    # the options struct: two arrays of GEM_MAX_JOINTS doubles, three doubles, two int32
    assert C.sizeof(_capi.GemBoneDepthOpts) == 8 * (2 * _capi.GEM_MAX_JOINTS + 3) + 8
    fields = re.search(r"typedef struct gem_bone_depth_opts \{(.*?)\} gem_bone_depth_opts;", header, flags=re.S).group(1)
    names = re.findall(r"(\w+)(?:\[GEM_MAX_JOINTS\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", fields))
    assert names == [f[0] for f in _capi.GemBoneDepthOpts._fields_]
    import __graft_entry__ as ge
    ge.build()
    assert hasattr(_capi.load_library(), "gem_bone_depths")
