"""A SLAM scale that drifts within a recording, on the device: `gem_slam_drift` against its numpy twin
(tests/slam_drift_twin.py) on the cases of tests/test_slam_drift_cpu.py, whose margins are asserted there; its refusals; and
`scale="drift"` through the detection route, `prepare_continuous`, `--bridge` and the command lines.

Knot values: float64 lies 4.1e-16 (walker), 2.9e-15 (two knots), 5.7e-16 (lost rows), 2.1e-15 (standing) and 2.4e-15 (2048 knots)
from the twin run in np.longdouble, measured on the CPU (`test_slam_drift_cpu.spread`); all are below 1e-13, so the gate is 1e-12
relative (`knot_gate` computes it again from the spread where the test runs)."""
import json
import os

import numpy as np
import pytest

import slam_drift_twin as D
from globalegomocap_amd import synth_walk as W
from test_slam_drift_cpu import DEVICE_CASES, LAG, MARGIN, creeping, device_case, device_twin, knot_gate, one_interval_case

pytestmark = pytest.mark.gpu

RTOL = 1e-12
EPS = np.finfo(np.float64).eps
BLOCK = 256          # rows per block of the metric track's scan (DR_THREADS)
FPS = 25


@pytest.fixture(scope="module")
def S():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import slam_scale
    return slam_scale


def _on_device(x):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).to("cuda")]


def _call(S, k, **kw):
    args = dict(stiffness=1.0, tau=0.10, min_pairs=k["min_pairs"])
    args.update(kw)
    return S.drift_call(_on_device(k["x"]), k["R"], k["c"], k["ids"], args.pop("lag", k["lag"]), args.pop("knot", k["knot"]), **args)


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(got == want, 0.0, np.abs(got - want) / np.abs(want)))) if got.size else 0.0


def scan_in_the_device_order(s, c, ids, knot):
    """The metric track as the device sums it: the scaled steps, an inclusive Hillis-Steele scan within blocks of BLOCK rows, the
    blocks' totals added up in order, every block behind the first shifted by what lies before it.  Rows behind a block never enter it."""
    n = len(ids)
    km, um = D.place(ids[:-1] + ids[1:] - 2 * int(ids[0]), knot, len(s))
    sm = (1.0 - um) * s[km] + um * s[km + 1]
    nb = -(-n // BLOCK)
    steps = np.zeros((nb * BLOCK, 3))
    steps[1:n] = sm[:, None] * (c[1:] - c[:-1])
    loc = steps.reshape(nb, BLOCK, 3)
    off = 1
    while off < BLOCK:
        new = loc.copy()
        new[:, off:] = loc[:, :-off] + loc[:, off:]
        loc, off = new, 2 * off
    before, t = np.zeros((nb, 3)), np.zeros(3)
    for b in range(nb):
        before[b] = t
        t = t + loc[b, -1]
    out = loc.copy()
    out[1:] = before[1:, None, :] + loc[1:]
    return out.reshape(-1, 3)[:n]


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_kernels_against_the_twin(S, name, capsys):
    from globalegomocap_amd import _capi
    k, want = device_case(name), device_twin(name)
    assert all(v > MARGIN for v in want["margins"].values())          # (asserted on the CPU too: an unlucky seed fails loudly)
    gate = knot_gate(name)
    rc, out, msg = _call(S, k)
    assert rc == 0, msg
    g = S.ScaleEstimate(out["scale_report"])
    rep = _capi.GemDriftReport.from_buffer_copy(out["report"].tobytes())
    knots, metric = out["knots"], out["metric"]
    K, n = len(want["knot_scale"]), len(k["ids"])
    with capsys.disabled():
        print("\n%s: %d knots, device curve %.9g .. %.9g; relative differences: knots %.3g (gate %.3g), interval sums %.3g, rms %.3g, mean %.3g, "
              "lambda %.3g" % (name, K, rep.scale_min, rep.scale_max, _rel(knots[:, 0], want["knot_scale"]), gate, _rel(knots[:-1, 2], want["interval_bb"]),
                               _rel(rep.residual_rms, want["residual_rms"]), _rel(rep.scale_mean, want["scale_mean"]), _rel(rep.lam, want["lam"])))
    # the global estimate is gem_slam_scale's
    gw = want["global"]
    np.testing.assert_allclose([g.scale, g.s0, g.s_ref, g.residual_rms], [gw[q] for q in ("scale", "s0", "s_ref", "residual_rms")], rtol=RTOL, atol=0)
    assert (g.pairs, g.inliers, g.informative, g.g0, g.status) == (gw["pairs"], gw["inliers"], gw["informative"], gw["g0"], 0)
    np.testing.assert_allclose(out["costs"].cpu().numpy(), gw["costs"], rtol=RTOL, atol=0)
    # counts are exact, sums to the project's tolerance
    assert (int(rep.status), int(rep.n_knots), int(rep.knot), rep.stiffness, int(rep.first_id)) == (0, K, k["knot"], 1.0, int(k["ids"][0]))
    assert np.array_equal(knots[:-1, 1], want["interval_count"]) and (int(rep.inliers), int(rep.informative)) == (want["inliers"], want["informative"])
    assert not knots[-1, 1:].any() and not knots[:, 3].any() and int(rep.bad_pivot) == -1
    np.testing.assert_allclose(knots[:-1, 2], want["interval_bb"], rtol=RTOL, atol=0)
    np.testing.assert_allclose([rep.residual_rms, rep.lam, rep.metric_length, rep.slam_length, rep.scale_mean],
                               [want[q] for q in ("residual_rms", "lam", "metric_length", "slam_length", "scale_mean")], rtol=RTOL, atol=0)
    # the knot values, to the gate the spread between float64 and extended precision sets
    assert _rel(knots[:, 0], want["knot_scale"]) <= gate
    assert rep.scale_min == knots[:, 0].min() and rep.scale_max == knots[:, 0].max()
    # the metric track: any summation order, and one rounding per product, of the device's own curve
    track, length, _ = D.metric_track(knots[:, 0], k["c"], k["ids"], k["knot"])
    err = float(np.abs(metric - track).max())
    with capsys.disabled():
        print("%s: metric track differs from the left-to-right sum by %.3g m, bound 2 N eps L = %.3g m (N = %d, L = %.2f m)" %
              (name, err, 2 * n * EPS * length, n, length))
    assert err <= 2 * n * EPS * length and not metric[0].any()
    assert np.abs(metric - want["metric"]).max() <= (2 * n * EPS + 2 * gate) * length          # (and the twin's own, whose curve lies within the gate)
    # ... and exactly what the scan's fixed order gives: the bytes up to the end of a block need no row behind it
    assert metric.tobytes() == scan_in_the_device_order(knots[:, 0], k["c"], k["ids"], k["knot"]).tobytes()
    if n > 2 * BLOCK:
        assert metric[:2 * BLOCK].tobytes() == scan_in_the_device_order(knots[:, 0], k["c"][:2 * BLOCK], k["ids"][:2 * BLOCK], k["knot"]).tobytes()
    # two calls give the same bytes
    rc2, out2, _ = _call(S, k)
    assert rc2 == 0 and all(out2[q].tobytes() == out[q].tobytes() for q in ("scale_report", "knots", "metric", "report"))
    # without a host record the call only enqueues
    rc3, dev, _ = _call(S, k, read_back=False)
    assert rc3 == 0 and dev["metric"].cpu().numpy().tobytes() == metric.tobytes() and dev["knots"].cpu().numpy().tobytes() == knots.tobytes()


def _poisoned(n_rep, K, n):
    import torch
    return tuple(torch.full(shape, 7.0, dtype=torch.float64, device="cuda") for shape in ((n_rep,), (K, 4), (n, 3), (16,)))


def _untouched(outputs, which=(0, 1, 2, 3)):
    return all(bool((outputs[i] == 7.0).all()) for i in which if outputs[i] is not None)


def test_refusals_leave_the_outputs_untouched(S):
    from globalegomocap_amd import _capi
    k = device_case("walker")
    n, K = len(k["ids"]), 7
    need = _capi.load_library().gem_slam_drift_work(n, LAG, K)
    seen = set()
    bad_calls = [("null", dict(drop=2), "null output"), ("null", dict(drop=1), "null output"), ("null", dict(drop=3), "null output"),
                 ("null", dict(drop=0), "null output"), ("knot", dict(knot=LAG), "at least lag + 1"), ("stiffness", dict(stiffness=-1.0), "stiffness"),
                 ("stiffness", dict(stiffness=float("nan")), "stiffness"), ("stiffness", dict(stiffness=float("inf")), "stiffness"),
                 ("knots", dict(knot=LAG + 1, ids=k["ids"] * 30), "too many knots: 2996"), ("work", dict(work_bytes=need - 8), "d_work holds")]
    for what, bad, text in bad_calls:
        bad = dict(bad)
        outputs = list(_poisoned(19, min(2048, 2996 if what == "knots" else K), n))
        drop = bad.pop("drop", None)
        if drop is not None:
            outputs[drop] = None
        case = dict(k, ids=bad.pop("ids", k["ids"]))
        rc, _, msg = _call(S, case, outputs=tuple(outputs), **bad)
        assert rc == 1 and text in msg and msg.startswith("gem_slam_drift: "), (what, msg)
        assert _untouched(outputs), what
        seen.add((what, msg))
    assert len({m for _, m in seen}) >= 5          # each kind of mistake has its own message
    # the inherited refusal: the two records tell it, the curve and the track stay as they were
    outputs = _poisoned(19, K, n)
    rc, out, msg = _call(S, k, min_pairs=10000, outputs=outputs)
    assert rc == _capi.SCALE_TOO_FEW and msg.startswith("gem_slam_scale: the wearer did not walk enough") and "10000 informative pairs are needed" in msg
    assert _untouched(outputs, (1, 2)) and int(out["report"][0]) == _capi.SCALE_TOO_FEW and S.ScaleEstimate(out["scale_report"]).status == _capi.SCALE_TOO_FEW
    # ... with gem_slam_scale's own text and counts
    rc1, _, _, msg1 = S.scale_call(_on_device(k["x"]), k["R"], k["c"], k["ids"], LAG, min_pairs=10000)
    assert rc1 == rc and msg1 == msg
    # no pair at all is decided before any launch
    outputs = _poisoned(19, 2, LAG)
    short = dict(k, x=k["x"][:LAG], R=k["R"][:LAG], c=k["c"][:LAG], ids=k["ids"][:LAG])
    rc, _, msg = _call(S, short, outputs=outputs)
    assert rc == _capi.SCALE_NO_PAIRS and "no pairs" in msg and _untouched(outputs)
    # a recording whose inliers all lie in one interval does not fix the curve: the knots are named, the track is not written
    w, keep = one_interval_case()
    R, c = W.slam_inputs(w)
    one = dict(x=w["local"][keep], R=R[keep], c=c[keep], ids=w["frame_ids"][keep], lag=LAG, knot=100, min_pairs=20)
    outputs = _poisoned(19, 7, len(keep))
    rc, out, msg = _call(S, one, outputs=outputs)
    assert rc == _capi.DRIFT_NOT_SOLVED and "1 of 6 knot intervals" in msg and _untouched(outputs, (2,))
    assert out["knots"][0, 1] > 50 and not out["knots"][1:, 1].any() and int(out["report"][0]) == _capi.DRIFT_NOT_SOLVED
    rows = w["rows"][keep]
    with pytest.raises(ValueError, match=r"drift cannot be estimated.*no inlier pairs between knots 1-2, 2-3, 3-4, 4-5, 5-6"):
        S.estimate_drift(_on_device(w["local"])[0], rows, [(0, 600)], FPS, knot=100, min_pairs=20, tracked=True)
    with pytest.raises(ValueError, match=r"cannot be estimated.*did not walk enough"):
        S.estimate_drift(_on_device(w["local"])[0], w["rows"], [(0, 600)], FPS, knot=100, min_pairs=10000)
    with pytest.raises(ValueError, match="a pair alone is 5 frames long"):
        S.estimate_drift(_on_device(w["local"])[0], w["rows"], [(0, 600)], FPS, knot=5)


# ---------------------------------------------------------------------------------------------------------------------- end to end
N = 600


def _write_rows(path, rows):
    with open(str(path), "w") as f:
        f.write("\n".join(" ".join(repr(float(v)) for v in r) for r in rows) + "\n")
    return str(path)


@pytest.fixture(scope="module")
def walker(S, tmp_path_factory):
    """The 600-frame walker whose trajectory's scale runs from 0.8 to 1.1, as (u, v, 1) detections with their depths, on files."""
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    root = tmp_path_factory.mktemp("walker")
    w = W.walk(N, scale=creeping(N), noise=0.03, seed=1)
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    uv = cam.project_numpy(w["local"].reshape(-1, 3)).reshape(N, 15, 2)
    det = {"keypoints": np.concatenate([uv, np.ones((N, 15, 1))], axis=2), "depth": w["depth"]}
    np.savez(str(root / "det.npz"), **det)
    return {"w": w, "det": det, "traj": _write_rows(root / "traj.txt", w["rows"]), "npz": str(root / "det.npz"), "root": root}


def _same_recording(a, b, keys=("heat", "est_local", "est_global", "cams")):
    import torch
    assert len(a) == len(b) and np.array_equal(a.origins, b.origins)
    for x, y in zip(a.chunks, b.chunks):
        for q in keys:
            assert torch.equal(getattr(x, q), getattr(y, q)), q


def test_detection_route_end_to_end(S, walker, capsys):
    from globalegomocap_amd import detections, slam
    spans = [(a, a + 100) for a in range(0, N, 100)]
    rec = detections.recording_from_detections(walker["traj"], walker["det"], None, "drift", spans, FPS, knot=100)
    est = rec.scale_report
    assert isinstance(est, S.DriftEstimate) and rec.scale == est.scale_mean and len(rec) == 6 and rec.origins.shape == (6, 4, 4)
    assert est.n_knots == 7 and est.knot_ids.tolist() == list(range(0, 601, 100)) and est.global_estimate.pairs == N - LAG
    # the twin on the poses the route lifted
    x = np.concatenate([ch.est_local.cpu().numpy() for ch in rec.chunks])
    with open(walker["traj"]) as f:
        rows = slam.trajectory_rows(f.read())
    R, c, ids = S.selected_poses(rows, spans, FPS)
    want = D.estimate(x, R, c, ids, LAG, 100)
    assert all(v > MARGIN for v in want["margins"].values()), want["margins"]
    true = np.linalg.norm(walker["w"]["head"] - walker["w"]["head"][0], axis=1)
    with capsys.disabled():
        print("\ndetection route: %s\n  knots differ from the twin's by %.3g; worst error in distance from the start %.3f m, with one scale %.3f m" %
              (est.line(), _rel(est.knot_scale, want["knot_scale"]), np.abs(np.linalg.norm(est.metric, axis=1) - true).max(),
               np.abs(np.linalg.norm(est.global_estimate.scale * c, axis=1) - true).max()))
    assert _rel(est.knot_scale, want["knot_scale"]) <= RTOL and np.array_equal(est.interval_count, want["interval_count"])
    assert np.abs(np.linalg.norm(est.metric, axis=1) - true).max() <= 0.5 * np.abs(np.linalg.norm(est.global_estimate.scale * c, axis=1) - true).max()
    # the recording is the one a metric SLAM with this track gives at scale 1
    rt, _ = slam.relative_poses(est.metric_rows()[:, 1:4], est.metric_rows()[:, 4:8])
    assert np.array_equal(rt, est.metric)
    metric_traj = _write_rows(walker["root"] / "metric.txt", est.metric_rows())
    same = detections.recording_from_detections(metric_traj, walker["det"], None, 1.0, spans, FPS)
    assert same.scale is None and same.scale_report is None
    _same_recording(rec, same)
    # the one-scale route is what it was: the recording the number it prints gives
    auto = detections.recording_from_detections(walker["traj"], walker["det"], None, "auto", spans, FPS)
    assert isinstance(auto.scale_report, S.ScaleEstimate) and auto.scale == auto.scale_report.scale == est.global_estimate.scale
    _same_recording(auto, detections.recording_from_detections(walker["traj"], walker["det"], None, auto.scale, spans, FPS))
    assert not np.array_equal(auto.origins, rec.origins)
    with pytest.raises(ValueError, match="cannot be estimated"):
        detections.recording_from_detections(walker["traj"], walker["det"], None, "drift", spans, FPS, knot=100, min_pairs=N)
    with pytest.raises(ValueError, match="exactly one of gt_path"):
        detections.recording_from_detections(walker["traj"], walker["det"], "gt.pkl", "drift", spans, FPS)


def test_prepare_continuous_is_the_metric_track_at_scale_one(S, walker, tmp_path, capsys):
    """The walker in the pose network's file format (the argmax lift quantises, so no accuracy is asserted)."""
    from globalegomocap_amd import prepare, synth, synth_recording as R
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    w = walker["w"]
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    ix, iy = synth.heatmap_coords(cam.project_numpy(w["local"].reshape(-1, 3)).reshape(N, 15, 2))
    heat64 = R.paraboloid_heatmaps(np.floor(np.stack([ix, iy], -1)) + np.array([0.3, 0.2]), np.full((N, 15), 5.0))
    hd, dd, traj, _ = R.write_recording(str(tmp_path / "rec"), heat64, w["depth"], ["f_%d.mat" % k for k in range(N)], None, None, w["rows"], None)
    capsys.readouterr()
    rec = prepare.prepare_continuous(traj, hd, dd, None, 0, N, fps=FPS, scale="drift", knot=100)
    printed = capsys.readouterr().out
    est = rec.scale_report
    assert "SLAM scale drift: " in printed and isinstance(est, S.DriftEstimate) and rec.scale == est.scale_mean and len(rec) == 1
    assert est.n_knots == 7 and 0 < est.scale_min <= est.scale_mean <= est.scale_max
    metric_traj = _write_rows(tmp_path / "metric.txt", est.metric_rows())
    same = prepare.prepare_continuous(metric_traj, hd, dd, None, 0, N, fps=FPS, scale=1.0, verbose=False)
    assert same.scale is None
    _same_recording(rec, same)
    with pytest.raises(ValueError, match="exactly one of gt_path"):
        prepare.prepare_continuous(traj, hd, dd, "gt.pkl", 0, N, fps=FPS, scale="drift")


def _small_vaes(golden):
    from helpers import sd_from_npz
    lt = golden("lbfgs_tiny")
    return dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False)


def test_bridge_with_five_lines_removed_prepares_and_optimises(S, walker, golden, capsys):
    import torch
    from globalegomocap_amd import detections, whole_sequence as ws
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    rows = walker["w"]["rows"]
    holed = _write_rows(walker["root"] / "holed.txt", np.delete(rows, np.arange(310, 315), axis=0))
    spans = [(a, a + 100) for a in range(0, N, 100)]
    with pytest.raises(ValueError, match=r"no line for frame ids \[310, 311, 312, 313, 314\]"):
        detections.recording_from_detections(holed, walker["det"], None, "drift", spans, FPS, knot=100)
    rec = detections.recording_from_detections(holed, walker["det"], None, "drift", spans, FPS, knot=100, bridge=1.0)
    est, br = rec.scale_report, rec.bridge_report
    assert isinstance(est, S.DriftEstimate) and len(est.frame_ids) == N - 5 and est.global_estimate.pairs == N - 5 - 2 * LAG
    assert (br.lost, br.gaps, br.gap_ids) == (5, 1, [(310, 5)]) and np.flatnonzero(np.concatenate(rec.bridged)).tolist() == list(range(310, 315))
    with capsys.disabled():
        print("\nbridged: %s\n  %s" % (est.line(), br.line()))
    # the tracked frames' cameras are those of the metric track at scale 1
    same = detections.recording_from_detections(_write_rows(walker["root"] / "holed_metric.txt", est.metric_rows()), walker["det"], None, 1.0, spans, FPS,
                                                bridge=1.0)
    _same_recording(rec, same)
    torch.manual_seed(31)
    out = ws.optimize_recording(rec, DEFAULT_CALIBRATION, ground_truth=False, **_small_vaes(golden))
    for i in (2, 3):          # (the chunked route's windows cover 98 frames of a chunk of 100)
        assert out[i].shape == (6 * 98, 15, 3) and np.isfinite(out[i]).all()
    ws.release_pools()


def test_command_lines(S, walker, golden, tmp_path, monkeypatch, capsys):
    from globalegomocap_amd import bvh, continuous
    out = str(tmp_path / "report" / "drift.json")
    capsys.readouterr()
    est = S._cli(["--slam", walker["traj"], "--keypoints", walker["npz"], "--start", "0", "--end", str(N), "--scale", "drift", "--knot", "4", "--json", out])
    printed = capsys.readouterr().out
    lines = printed.splitlines()
    assert lines[0].startswith("SLAM scale drift: ") and sum(x.startswith("knot ") for x in lines) == 7 and sum(x.startswith("chunk ") for x in lines) == 6
    with open(out) as f:
        d = json.load(f)
    assert d["knot_scale"] == [float(v) for v in est.knot_scale] and d["knot_ids"] == list(range(0, 601, 100)) and len(d["interval_count"]) == 6
    assert d["scale"] == est.scale_mean and d["global_scale"] == est.global_estimate.scale and len(d["per_chunk"]) == 6
    with pytest.raises(SystemExit):
        S._cli(["--slam", walker["traj"], "--keypoints", walker["npz"], "--start", "0", "--end", str(N), "--knot", "4"])
    capsys.readouterr()
    # `continuous --scale drift`: one motion, one optimized.bvh (the optimiser is given the test's small VAEs)
    real, calls = continuous.optimize_continuous, []

    def with_small_vaes(rec, camera, *args, **kwargs):
        calls.append(rec)
        return real(rec, camera, *args, **dict(kwargs, **_small_vaes(golden)))
    monkeypatch.setattr(continuous, "optimize_continuous", with_small_vaes)
    continuous._cli(["--slam", walker["traj"], "--keypoints", walker["npz"], "--start", "0", "--end", str(N), "--scale", "drift", "--knot", "4",
                     "--bvh", str(tmp_path / "b")])
    rec = calls[-1]
    assert len(rec) == 1 and isinstance(rec.scale_report, S.DriftEstimate) and rec.scale_report.knot_scale.tobytes() == est.knot_scale.tobytes()
    found = sorted(os.path.join(d, f) for d, _, files in os.walk(str(tmp_path / "b")) for f in files if f == "optimized.bvh")
    assert len(found) == 1 and bvh.read_bvh(found[0]).motion.shape[0] == N
    assert "SLAM scale drift: " in capsys.readouterr().out
