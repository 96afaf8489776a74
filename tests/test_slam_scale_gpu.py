"""The SLAM-scale estimator on the device: `gem_slam_scale` against its numpy twin (tests/slam_scale_twin.py)
on noisy synthetic walkers, its refusals, and `scale="auto"` through the detection route and through `prepare`."""
import os

import numpy as np
import pytest

import slam_scale_twin as T
from globalegomocap_amd import synth_walk as W
from test_slam_scale_cpu import LAG, NOISY_BOUND

pytestmark = pytest.mark.gpu

TILE = 256          # GEM_SCALE_TILE: pairs per workgroup of the cost kernel
RTOL = 1e-12
MARGIN = 1e-9       # the twin's discrete decisions must be this far from flipping, or the comparison below would hide nothing but prove nothing


@pytest.fixture(scope="module")
def S():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import _capi, slam_scale
    assert _capi.SCALE_TILE == TILE
    return slam_scale


def _inputs(n, seed, keep=None):
    w = W.walk(n, scale=1.7, noise=0.03, seed=seed)
    R, c = W.slam_inputs(w)
    keep = np.arange(n) if keep is None else keep
    return np.ascontiguousarray(w["local"][keep]), R[keep], c[keep], w["frame_ids"][keep]


def _on_device(x, cuts):
    """every chunk its own allocation"""
    import torch
    return [torch.from_numpy(x[lo:hi].copy()).to("cuda") for lo, hi in zip(cuts[:-1], cuts[1:])]


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(got == want, 0.0, np.abs(got - want) / np.abs(want)))) if got.size else 0.0


# name, frames, seed, rows kept (None: all), chunk cuts (None: one chunk), min_pairs
CASES = [
    ("one pair", LAG + 1, 1, None, None, 0),
    ("T - 1 pairs", TILE - 1 + LAG, 2, None, None, 50),
    ("T pairs", TILE + LAG, 3, None, None, 50),
    ("T + 1 pairs", TILE + 1 + LAG, 4, None, None, 50),
    ("2 T + 3 pairs", 2 * TILE + 3 + LAG, 5, None, None, 50),
    ("a hole in the frame ids", 300, 6, np.r_[0:100, 104:180, 181:300], None, 50),
    ("three chunks, one of a single frame", 120, 7, None, [0, 60, 61, 120], 50),
]


@pytest.mark.parametrize("name,n,seed,keep,cuts,min_pairs", CASES, ids=[c[0] for c in CASES])
def test_kernels_against_the_twin(S, name, n, seed, keep, cuts, min_pairs, capsys):
    x, R, c, ids = _inputs(n, seed, keep)
    cuts = [0, len(x)] if cuts is None else cuts
    want = T.estimate(x, R, c, ids, LAG, min_pairs=min_pairs, chunk_starts=cuts)
    m = want["margins"]
    with capsys.disabled():
        print("\n%s: twin scale %r, %d pairs, %d inliers, %d informative, margins %s" % (name, want["scale"], want["pairs"], want["inliers"],
                                                                                          want["informative"], m))
    # an unlucky seed fails here, loudly, instead of hiding a mismatch
    assert m["cost_gap"] > MARGIN and m["tau"] > MARGIN and m["sides"] > MARGIN and m["informative"] > MARGIN
    chunks = _on_device(x, cuts)
    rc, rep, costs, msg = S.scale_call(chunks, R, c, ids, LAG, 0.10, min_pairs)
    assert rc == 0, msg
    got = S.ScaleEstimate(rep, costs)
    dcosts = costs.cpu().numpy()
    with capsys.disabled():
        print("%s: device scale %r; relative differences: costs %.3g, scale %.3g, rms %.3g, s_ref %.3g, path %.3g" %
              (name, got.scale, _rel(dcosts, want["costs"]), _rel(got.scale, want["scale"]), _rel(got.residual_rms, want["residual_rms"]),
               _rel(got.s_ref, want["s_ref"]), _rel(got.path_length, want["path_length"])))
    np.testing.assert_allclose(dcosts, want["costs"], rtol=RTOL, atol=0)
    assert got.g0 == want["g0"]
    np.testing.assert_allclose([got.scale, got.residual_rms, got.s0, got.s_ref, got.path_length], [want[k] for k in ("scale", "residual_rms", "s0", "s_ref", "path_length")],
                               rtol=RTOL, atol=0)
    assert (got.pairs, got.inliers, got.informative) == (want["pairs"], want["inliers"], want["informative"])
    np.testing.assert_allclose(got.stance_share, want["stance_share"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(got.per_chunk_sums, want["per_chunk"][:, :2], rtol=RTOL, atol=0)
    np.testing.assert_allclose(got.per_chunk, want["per_chunk"][:, 2], rtol=RTOL, atol=0, equal_nan=True)
    assert got.status == 0 and (got.lag, got.tau, got.min_pairs) == (LAG, 0.10, min_pairs)
    # no floating-point atomics: a second call gives the same bytes
    rc2, rep2, costs2, _ = S.scale_call(chunks, R, c, ids, LAG, 0.10, min_pairs)
    assert rc2 == 0 and rep2.tobytes() == rep.tobytes() and costs2.cpu().numpy().tobytes() == dcosts.tobytes()


def test_refusals(S):
    from globalegomocap_amd import _capi
    x, R, c, ids = _inputs(200, 8)
    # N = lag: no pair -- decided on the host, nothing is launched (report and costs keep their zeros)
    rc, rep, costs, msg = S.scale_call(_on_device(x[:LAG], [0, LAG]), R[:LAG], c[:LAG], ids[:LAG], LAG)
    assert rc == _capi.SCALE_NO_PAIRS and "no pairs" in msg and not rep.any() and not costs.cpu().numpy().any()
    # a trajectory that never moves
    chunks = _on_device(x, [0, 200])
    rc, rep, _, msg = S.scale_call(chunks, R, np.zeros_like(c), ids, LAG)
    assert rc == _capi.SCALE_NO_PAIRS and "camera translation" in msg and "195 pairs" in msg and S.ScaleEstimate(rep).status == _capi.SCALE_NO_PAIRS
    # frame ids that leave no two frames LAG apart
    rc, rep, _, msg = S.scale_call(chunks, R, c, ids * 2, LAG)
    assert rc == _capi.SCALE_NO_PAIRS and "(0 pairs" in msg
    # more informative pairs asked for than there are
    rc, rep, _, _ = S.scale_call(chunks, R, c, ids, LAG)
    ok = S.ScaleEstimate(rep)
    assert rc == 0 and 50 <= ok.informative <= ok.inliers <= ok.pairs == 195
    rc, rep, _, msg = S.scale_call(chunks, R, c, ids, LAG, min_pairs=ok.informative + 1)
    assert rc == _capi.SCALE_TOO_FEW and "did not walk enough" in msg and "%d informative" % ok.informative in msg
    assert S.ScaleEstimate(rep).scale == ok.scale          # (the record is complete all the same)
    # without a host record the call only enqueues: the verdict is the record's status
    rc, dev_rep, _, _ = S.scale_call(chunks, R, c, ids, LAG, min_pairs=ok.informative + 1, read_back=False)
    assert rc == 0 and S.ScaleEstimate(dev_rep.cpu().numpy()).status == _capi.SCALE_TOO_FEW
    # arguments are checked before any launch
    for bad in (dict(lag=0), dict(tau=0.0), dict(tau=float("nan")), dict(feet=(9, 10, 13, 15))):
        kw = dict(lag=LAG, tau=0.10)
        kw.update(bad)
        rc, rep, _, msg = S.scale_call(chunks, R, c, ids, kw.pop("lag"), kw.pop("tau"), **kw)
        assert rc == 1 and msg and not rep.any(), bad
    with pytest.raises(ValueError):
        S.scale_call(chunks, R[:-1], c, ids, LAG)
    # the public function raises ValueError naming the counts
    w = W.walk(200, scale=1.7, noise=0.03, seed=8, stand=[(0, 200)])
    with pytest.raises(ValueError, match=r"cannot be estimated.*0 informative"):
        S.estimate_scale(_on_device(w["local"], [0, 200]), w["rows"], [(0, 200)], 25)
    est = S.estimate_scale(chunks[0], W.walk(200, scale=1.7, noise=0.03, seed=8)["rows"], [(0, 120), (120, 200)], 25)
    assert est.scale == ok.scale and len(est.per_chunk) == 2 and est.as_dict()["informative"] == ok.informative


def _twin_on_recording(S, rec, rows, spans, fps, min_pairs):
    x = np.concatenate([ch.est_local.cpu().numpy() for ch in rec.chunks])
    R, c, ids = S.selected_poses(rows, spans, fps)
    cuts = np.concatenate([[0], np.cumsum([b - a for a, b in spans])])
    want = T.estimate(x, R, c, ids, S.default_lag(fps), min_pairs=min_pairs, chunk_starts=cuts)
    m = want["margins"]
    assert m["cost_gap"] > MARGIN and m["tau"] > MARGIN and m["sides"] > MARGIN and m["informative"] > MARGIN, m
    return want


def test_detection_route_end_to_end(S, tmp_path, capsys):
    """A 60-frame walker projected through the fisheye model into (u, v, 1) detections, its depths beside them."""
    from globalegomocap_amd import detections, slam
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    n, fps, scale = 60, 25, 1.7
    w = W.walk(n, scale=scale)
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    uv = cam.project_numpy(w["local"].reshape(-1, 3)).reshape(n, 15, 2)
    kp = np.concatenate([uv, np.ones((n, 15, 1))], axis=2)
    traj = str(tmp_path / "traj.txt")
    with open(traj, "w") as f:
        f.write("\n".join(" ".join(repr(float(v)) for v in r) for r in w["rows"]) + "\n")
    rec = detections.recording_from_detections(traj, {"keypoints": kp, "depth": w["depth"]}, None, "auto", [(0, n)], fps, min_pairs=30)
    assert len(rec) == 1 and tuple(rec.chunks[0].heat.shape) == (n, 64, 64, 15) and rec.origins.shape == (1, 4, 4)
    est = rec.scale_report
    assert rec.scale == est.scale and est.pairs == n - LAG and est.informative >= 30
    with open(traj) as f:
        rows = slam.trajectory_rows(f.read())
    want = _twin_on_recording(S, rec, rows, [(0, n)], fps, 30)
    with capsys.disabled():
        print("\ndetection route: scale %r, twin %r (relative difference %.3g), true %r (relative error %.3g); %s" %
              (rec.scale, want["scale"], _rel(rec.scale, want["scale"]), scale, abs(rec.scale / scale - 1), est.line()))
    assert abs(rec.scale / want["scale"] - 1) <= RTOL
    assert (est.pairs, est.inliers, est.informative) == (want["pairs"], want["inliers"], want["informative"])
    assert abs(rec.scale / scale - 1) <= NOISY_BOUND
    # the recording is the one the number itself gives
    same = detections.recording_from_detections(traj, {"keypoints": kp, "depth": w["depth"]}, None, rec.scale, [(0, n)], fps)
    import torch
    assert same.scale is None and same.scale_report is None
    assert all(torch.equal(getattr(same.chunks[0], k), getattr(rec.chunks[0], k)) for k in ("heat", "est_local", "est_global", "cams"))
    with pytest.raises(ValueError, match="cannot be estimated"):
        detections.recording_from_detections(traj, {"keypoints": kp, "depth": w["depth"]}, None, "auto", [(0, n)], fps, min_pairs=n)


def test_prepare_with_auto_is_prepare_with_the_number(S, tmp_path, capsys):
    """Three 26-frame chunks in the pose network's file format whose heat-map centres and depths carry a walker: the argmax lift
    quantises, so no accuracy is asserted -- the estimate is the twin's on the lifted poses, and the recording is bit for bit the one
    the number gives."""
    import torch
    from globalegomocap_amd import prepare, slam, synth, synth_recording as R
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    n, fps, size, min_pairs = 78, 25, 26, 10
    w = W.walk(n, scale=0.6)
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    ix, iy = synth.heatmap_coords(cam.project_numpy(w["local"].reshape(-1, 3)).reshape(n, 15, 2))
    centres = np.floor(np.stack([ix, iy], -1)) + np.array([0.3, 0.2])          # (no ties: the peak pixel is unique)
    heat64 = R.paraboloid_heatmaps(centres, np.full((n, 15), 5.0))
    hd, dd, traj, _ = R.write_recording(str(tmp_path / "rec"), heat64, w["depth"], ["f_%d.mat" % k for k in range(n)], None, None, w["rows"], None)
    capsys.readouterr()
    rec = prepare.prepare_sequence(traj, hd, dd, None, 0, n + 1, fps=fps, test_size=size, scale="auto", min_pairs=min_pairs)
    printed = capsys.readouterr().out
    assert "SLAM scale estimate: " in printed and "informative" in printed
    spans = prepare.chunk_spans(0, n + 1, size)
    assert len(rec) == 3 and spans == [(0, 26), (26, 52), (52, 78)]
    with open(traj) as f:
        rows = slam.trajectory_rows(f.read())
    want = _twin_on_recording(S, rec, rows, spans, fps, min_pairs)
    est = rec.scale_report
    with capsys.disabled():
        print("\nprepare route: %s; twin %r (relative difference %.3g); per chunk %s" % (est.line(), want["scale"], _rel(est.scale, want["scale"]), est.per_chunk.tolist()))
    assert rec.scale == est.scale and abs(est.scale / want["scale"] - 1) <= RTOL
    assert (est.pairs, est.inliers, est.informative) == (want["pairs"], want["inliers"], want["informative"]) and est.pairs == n - LAG
    np.testing.assert_allclose(est.per_chunk, want["per_chunk"][:, 2], rtol=RTOL, atol=0, equal_nan=True)
    num = prepare.prepare_sequence(traj, hd, dd, None, 0, n + 1, fps=fps, test_size=size, scale=rec.scale, verbose=False)
    assert num.scale is None and num.scale_report is None and np.array_equal(num.origins, rec.origins)
    for a, b in zip(num.chunks, rec.chunks):
        for k in ("heat", "est_local", "est_global", "cams"):
            x, y = getattr(a, k), getattr(b, k)
            assert x.dtype == y.dtype and torch.equal(x, y), k
    # the refusal comes before any chunk is written
    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="cannot be estimated"):
        prepare.prepare_sequence(traj, hd, dd, None, 0, n + 1, fps=fps, test_size=size, scale="auto", min_pairs=n, out_root=out, verbose=False)
    assert not os.path.exists(out)


def test_command_line_prints_the_report_beside_the_ground_truths_scale(S, tmp_path, capsys):
    """`python -m globalegomocap_amd.slam_scale` on both routes: the estimate `prepare --scale auto` would use, per-chunk scales, and with
    --gt the Umeyama scale of every chunk's head track beside them."""
    import json
    from globalegomocap_amd import prepare, synth, synth_recording as R
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    n, size, scale = 78, 26, 0.6
    w = W.walk(n, scale=scale)
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    uv = cam.project_numpy(w["local"].reshape(-1, 3)).reshape(n, 15, 2)
    ix, iy = synth.heatmap_coords(uv)
    heat64 = R.paraboloid_heatmaps(np.floor(np.stack([ix, iy], -1)) + np.array([0.3, 0.2]), np.full((n, 15), 5.0))
    gt = np.einsum("nij,nkj->nki", w["cams"][:, :3, :3], w["local"]) + w["cams"][:, None, :3, 3]
    hd, dd, traj, gtp = R.write_recording(str(tmp_path / "rec"), heat64, w["depth"], ["f_%d.mat" % k for k in range(n)], None, None, w["rows"], gt)
    out = str(tmp_path / "report" / "scale.json")
    capsys.readouterr()
    est = S._cli(["--slam", traj, "--heatmaps", hd, "--depths", dd, "--start", "0", "--end", str(n), "--fps", "25", "--test_size", str(size),
                  "--min_pairs", "10", "--gt", gtp, "--json", out])
    printed = capsys.readouterr().out
    assert printed.startswith("SLAM scale estimate: ") and printed.count("Umeyama against the ground truth") == 3 and "chunk 2 [52, 78)" in printed
    with open(out) as f:
        d = json.load(f)
    assert d["scale"] == est.scale and d["pairs"] == n - LAG and len(d["per_chunk"]) == 3
    with capsys.disabled():
        print("\ncommand line: estimate %r, per chunk %s, Umeyama per chunk %s (true %r)" % (est.scale, d["per_chunk"], d["umeyama_per_chunk"], scale))
    # the neck is 0.3 m from the camera, where half a cell of the argmax lift's 16-pixel grid is some 6 mm, on a head track that spans
    # 1.2 m per chunk: the ground truth gives the true scale to a few per cent
    np.testing.assert_allclose(d["umeyama_per_chunk"], scale, rtol=0.05)
    rec = prepare.prepare_sequence(traj, hd, dd, None, 0, n + 1, fps=25, test_size=size, scale="auto", min_pairs=10, verbose=False)
    assert rec.scale == est.scale
    # detections
    np.savez(str(tmp_path / "det.npz"), keypoints=np.concatenate([uv, np.ones((n, 15, 1))], axis=2), depth=w["depth"])
    est = S._cli(["--slam", traj, "--keypoints", str(tmp_path / "det.npz"), "--start", "0", "--end", "60", "--test_size", "20", "--min_pairs", "30"])
    printed = capsys.readouterr().out
    assert "chunk 2 [40, 60)" in printed and "Umeyama" not in printed and abs(est.scale / scale - 1) < 1e-5          # (the file's rows have nine decimals)
    for bad in (["--slam", traj, "--start", "0", "--end", "60"], ["--slam", traj, "--heatmaps", hd, "--start", "0", "--end", "60"]):
        with pytest.raises(SystemExit):
            S._cli(bad)
    capsys.readouterr()
