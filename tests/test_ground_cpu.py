"""The ground plane from foot contacts without a GPU: the numpy twin (tests/ground_twin.py) on the synthetic
walker -- accuracy without and with noise, the degenerate and the refused inputs, invariance under rigid motions, the upright frame,
the composition of two similarities -- and the wiring of `upright` through the writers, the outputs record and the command lines."""
import inspect
import os

import numpy as np
import pytest

import ground_twin as T
from globalegomocap_amd.synth_walk import FOOT_HEIGHT, _rotvec_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISY_SEEDS = (0, 2, 3)
# the tilt errors the twin gives on the walker of 98 frames with 3 cm of noise, seeds 0, 2, 3 (degrees).  The
# bound below is 1.5 x the largest: the margin covers a change of numpy's eigen-solver and nothing else.
NOISY_TILT = (0.5333, 0.1758, 2.6174)


@pytest.mark.parametrize("F", [40, 98])
def test_noise_free_walker(F):
    x, normal, floor, _ = T.walker_world(F)
    e = T.estimate(x)
    assert T.SOURCES[e["source"]] == "plane"
    assert T.angle_deg(e["n"], normal) < 1e-6
    assert abs(e["d"] - (floor + FOOT_HEIGHT)) < 1e-12
    assert e["skate"] == 0.0 and e["skate_pairs"] > 0
    assert e["penetration"] <= 1e-12
    assert 6.0 < T.angle_deg(e["u0"], normal) < 7.5          # (the body leans: what the renderer's "up" heuristic is off by)


def test_noisy_walker_beats_the_body_hint(capsys):
    got = []
    for seed in NOISY_SEEDS:
        x, normal, floor, _ = T.walker_world(98, noise=0.03, seed=seed)
        e = T.estimate(x)
        tilt, hint = T.angle_deg(e["n"], normal), T.angle_deg(e["u0"], normal)
        got.append(tilt)
        with capsys.disabled():
            print("seed %d: tilt error %.4f deg, body-up hint %.4f deg, offset error %.4f m, skate %.4f m/frame" %
                  (seed, tilt, hint, e["d"] - (floor + FOOT_HEIGHT), e["skate"]))
        assert T.SOURCES[e["source"]] == "plane"
        assert tilt < 0.5 * hint, seed
        assert tilt < 1.5 * max(NOISY_TILT), seed
    np.testing.assert_allclose(got, NOISY_TILT, rtol=0, atol=1.5 * max(NOISY_TILT))


def test_degenerate_and_refused_inputs():
    x, normal, floor, _ = T.walker_world(98, stand=[(0, 98)])
    e = T.estimate(x)
    assert T.SOURCES[e["source"]] == "body_normal" and e["spread"] < 0.05 and e["points"] >= 8
    assert np.array_equal(e["n"], e["u0"]) and e["inliers"] == e["points"]
    x3 = T.walker_world(3)[0]
    e = T.estimate(x3, lag=5)
    assert T.SOURCES[e["source"]] == "body" and e["points"] == 0 and e["penetration"] == 0.0
    assert abs(e["d"] - (x3[:, [9, 10, 13, 14]].reshape(-1, 2, 3).mean(1) @ e["u0"]).min()) < 1e-12
    bad = T.walker_world(40)[0].copy()
    bad[17, 13, 1] = np.nan
    with pytest.raises(ValueError, match="NO_BODY"):
        T.estimate(bad)
    assert T.estimate(bad, check=False)["status"] == T.NO_BODY
    with pytest.raises(ValueError):
        T.estimate(np.zeros((40, 15, 3)))


def test_invariance_and_the_upright_frame():
    x, normal, floor, w = T.walker_world(98)
    e = T.estimate(x, foot_height=0.02)
    Q, t = _rotvec_matrix((0.7, -1.1, 0.4)), np.array([3.0, -2.0, 0.5])
    y = x @ Q + t
    f = T.estimate(y, foot_height=0.02)
    np.testing.assert_allclose(f["n"], e["n"] @ Q, rtol=0, atol=1e-12)
    np.testing.assert_allclose(f["d"], e["d"] + (e["n"] @ Q) @ t, rtol=0, atol=1e-12)
    up_x, up_y = T.upright(x, e["crt"]), T.upright(y, f["crt"])
    np.testing.assert_allclose(up_y, up_x, rtol=0, atol=1e-10)
    mid = 0.5 * (up_x[0, 7] + up_x[0, 11])
    assert abs(mid[0]) < 1e-12 and abs(mid[2]) < 1e-12 and mid[1] > 0.5
    R = e["crt"][1:10].reshape(3, 3)
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and e["crt"][0] == 1.0
    np.testing.assert_allclose(R.T @ R, np.eye(3), rtol=0, atol=1e-12)
    feet = np.stack([0.5 * (up_x[:, 9] + up_x[:, 10]), 0.5 * (up_x[:, 13] + up_x[:, 14])], axis=1)
    # y = 0 is the plane n . p = d - foot_height, the floor; the standing foot points lie on n . p = d, foot_height above it
    np.testing.assert_allclose(feet[w["standing"]][:, 1], 0.02, rtol=0, atol=1e-12)
    for given in (0.0, FOOT_HEIGHT):          # told the truth, the walker's own floor (z = 0 in its world) is y = 0
        up = T.upright(x, T.estimate(x, foot_height=given)["crt"])
        feet_y = np.stack([0.5 * (up[:, 9] + up[:, 10]), 0.5 * (up[:, 13] + up[:, 14])], axis=1)[w["standing"]][:, 1]
        np.testing.assert_allclose(feet_y, given, rtol=0, atol=1e-12)
        np.testing.assert_allclose(up[..., 1], w["world"][..., 2] - (FOOT_HEIGHT - given), rtol=0, atol=1e-12)
    # the wearer faces +Z: the left hip is on +X, and the walk goes forward
    assert up_x[0, 11, 0] > up_x[0, 7, 0] and up_x[-1, 0, 2] > up_x[0, 0, 2] + 1.0
    # a transform applied first is the same as the moved input
    crt_in = np.concatenate([[1.0], Q.reshape(-1), t])
    g = T.estimate(x, foot_height=0.02, crt_in=crt_in)
    np.testing.assert_allclose(g["crt"], f["crt"], rtol=0, atol=1e-12)


def test_composition_against_explicit_application():
    rng = np.random.default_rng(5)
    a = np.concatenate([[1.3], _rotvec_matrix((0.2, 0.9, -0.4)).reshape(-1), rng.normal(size=3)])
    b = np.concatenate([[0.7], _rotvec_matrix((-1.2, 0.1, 0.5)).reshape(-1), rng.normal(size=3)])
    p = rng.normal(size=(50, 3))
    np.testing.assert_allclose(T.apply(T.compose(a, b), p), T.apply(b, T.apply(a, p)), rtol=0, atol=1e-13)
    identity = np.concatenate([[1.0], np.eye(3).reshape(-1), np.zeros(3)])
    assert np.array_equal(T.compose(a, identity), a) and np.array_equal(T.compose(identity, a), a)


def test_the_new_keywords_are_keyword_only_with_their_defaults():
    from globalegomocap_amd import bvh, ground, meshes, optimizer, render, report, whole_sequence as ws
    for fn in (ws._settings, optimizer.main):
        par = inspect.signature(fn).parameters
        assert par["upright"].kind is inspect.Parameter.KEYWORD_ONLY and par["upright"].default is False, fn
        assert par["foot_height"].kind is inspect.Parameter.KEYWORD_ONLY and par["foot_height"].default is None, fn
    for fn in (bvh.write_bvh, meshes.write_meshes, meshes.vertex_blocks, render.write_frames):
        assert inspect.signature(fn).parameters["move"].default is None, fn
    for fn in (bvh.write_result_bvh, meshes.write_result_meshes, render.write_result_frames):
        par = list(inspect.signature(fn).parameters.values())
        assert par[-1].name == "upright" and par[-1].default is None, fn
    par = inspect.signature(ground.estimate_ground).parameters
    want = dict(fps=25.0, lag=None, tau_v=0.10, tau_h=0.05, min_spread=0.05, min_points=8, foot_height=0.0, moved_by=None, stream=None)
    assert list(par)[:2] == ["engine", "sequences"] and {k: par[k].default for k in want} == want
    fields = [f.name for f in report.Outputs.__dataclass_fields__.values()]
    assert fields[-3:] == ["upright", "upright_foot_height", "upright_lag"] and fields[8] == "video_quality"
    o = report.Outputs()
    assert o.upright is None and o.upright_foot_height is None and o.upright_lag is None and not o
    assert not report.Outputs(upright=True)          # (upright alone asks for no file)
    cfg = ws._settings("cam.json")
    assert cfg.upright is False and cfg.outputs == report.Outputs()
    cfg = ws._settings("cam.json", bvh="b", upright=True, foot_height=0.03)
    assert cfg.outputs == report.Outputs(bvh="b", upright=True, upright_foot_height=0.03)
    assert ws._settings("cam.json", bvh="b", foot_height=0.03).outputs == report.Outputs(bvh="b")
    with pytest.raises(ValueError, match="foot_height"):
        ws._settings("cam.json", upright=True, foot_height=float("nan"))
    assert ground.default_lag(25) == 5 and ground.default_lag(2) == 1 and ground.default_lag(30) == 6


def test_outputs_without_upright_pass_no_new_keyword_and_with_it_one_estimate(monkeypatch, tmp_path):
    from globalegomocap_amd import bvh, ground, meshes, render, report
    calls = []
    for mod, name in ((meshes, "write_result_meshes"), (render, "write_result_frames"), (bvh, "write_result_bvh")):
        monkeypatch.setattr(mod, name, lambda *a, _n=name, **k: calls.append((_n, a, k)))
    monkeypatch.setattr(ground, "estimate_ground", lambda *a, **k: pytest.fail("no estimate without upright"))
    seqs = (np.zeros((3, 15, 3)), np.ones((3, 15, 3)), None)
    everything = dict(mesh_root="m", render="r", bvh="b", video="v")
    assert report.Outputs(**everything).write("engine", "d/studio/chunk_0", seqs) is None
    assert [c[0] for c in calls] == ["write_result_meshes", "write_result_frames", "write_result_bvh", "write_result_frames"]
    assert all("upright" not in c[2] for c in calls)
    assert calls[0][2] == {} and calls[1][2] == {} and calls[2][2] == {"fps": 25}
    assert calls[3][2] == {"video": os.path.join("v", "studio", "chunk_0", "frames.avi"), "video_fps": 25, "video_quality": 90, "frames": False}
    before = list(calls)
    assert report.Outputs(upright=False, **everything).write("engine", "d/studio/chunk_0", seqs) is None
    assert [(c[0], c[2]) for c in calls[4:]] == [(c[0], c[2]) for c in before]
    # with upright: ONE estimate, of the optimised sequence (no ground truth), handed to every writer
    del calls[:]
    made = []

    def estimate(engine, reference, **k):
        made.append((reference, k))
        return "the estimate"
    monkeypatch.setattr(ground, "estimate_ground", estimate)
    found = report.Outputs(upright=True, upright_foot_height=0.04, bvh_fps=50, **everything).write("engine", "d/studio/chunk_0", seqs)
    assert found == "the estimate" and len(made) == 1 and made[0][0] is seqs[1]
    assert made[0][1] == dict(fps=50, lag=None, foot_height=0.04)
    assert len(calls) == 4 and all(c[2]["upright"] == "the estimate" for c in calls)
    gt = np.full((3, 15, 3), 2.0)
    report.Outputs(upright=True, bvh="b").write("engine", "d/studio/chunk_0", (seqs[0], seqs[1], gt))
    assert len(made) == 2 and made[1][0] is gt and made[1][1] == dict(fps=25, lag=None, foot_height=0.0)
    # the camera's views take no part, and upright alone estimates nothing
    monkeypatch.setattr(render, "write_result_camera_frames", lambda *a, **k: calls.append(("camera", a, k)))
    cams, heat = np.zeros((3, 4, 4)), np.zeros((3, 4, 4, 15))
    assert report.Outputs(upright=True, render_camera="c", video_camera="vc").write("engine", "d/studio/chunk_0", seqs, cams, heat) is None
    assert len(made) == 2 and all("upright" not in c[2] for c in calls[-2:])


def test_the_result_writers_hand_one_move_to_every_file(monkeypatch, tmp_path):
    from globalegomocap_amd import bvh, ground, meshes, render

    class Estimate(ground.GroundEstimate):
        def __init__(self, crt):
            self.crt = crt
    calls = []
    monkeypatch.setattr(bvh, "write_bvh", lambda *a, **k: calls.append(k))
    monkeypatch.setattr(meshes, "write_meshes", lambda *a, **k: calls.append(k) or 0)
    monkeypatch.setattr(render, "write_frames", lambda *a, **k: calls.append(k) or 0)
    est, opt, gt = np.zeros((3, 15, 3)), np.ones((3, 15, 3)), np.full((3, 15, 3), 2.0)
    bvh.write_result_bvh("engine", str(tmp_path / "a"), est, opt, gt)
    meshes.write_result_meshes("engine", str(tmp_path / "a"), est, opt, gt)
    render.write_result_frames("engine", str(tmp_path / "a"), est, opt, gt)
    assert len(calls) == 7 and all("move" not in k for k in calls)
    del calls[:]
    e = Estimate("crt")
    bvh.write_result_bvh("engine", str(tmp_path / "a"), est, opt, gt, upright=e)
    meshes.write_result_meshes("engine", str(tmp_path / "a"), est, opt, gt, upright=e)
    render.write_result_frames("engine", str(tmp_path / "a"), est, opt, gt, upright=e)
    assert [k["move"] for k in calls] == ["crt"] * 6 + [["crt"] * 3]
    # True: the ground truth where the others are aligned to it, else the optimised sequence
    seen = []
    monkeypatch.setattr(ground, "estimate_ground", lambda engine, ref, **k: seen.append(ref) or Estimate("made"))
    bvh.write_result_bvh("engine", str(tmp_path / "a"), est, opt, gt, upright=True)
    bvh.write_result_bvh("engine", str(tmp_path / "a"), est, opt, None, upright=True)
    assert len(seen) == 2 and seen[0] is gt and seen[1] is opt
    with pytest.raises(TypeError, match="upright"):
        bvh.write_result_bvh("engine", str(tmp_path / "a"), est, opt, None, upright="yes")


def test_the_parser_flags_are_present():
    from globalegomocap_amd import ground, whole_sequence as ws
    a = ws._parser().parse_args(["--data_path", "d"])
    assert a.upright is False and a.foot_height is None
    a = ws._parser().parse_args(["--data_path", "d", "--upright", "true", "--foot_height", "0.04"])
    assert a.upright is True and a.foot_height == 0.04
    a = ground._parser().parse_args(["r.pkl"])
    assert (a.fps, a.lag, a.tau_v, a.tau_h, a.foot_height, a.json) == (25.0, None, 0.10, 0.05, 0.0, None)
    a = ground._parser().parse_args(["r.pkl", "--fps", "50", "--lag", "7", "--tau_v", "0.2", "--tau_h", "0.03", "--foot_height", "0.05", "--json", "o.json"])
    assert (a.fps, a.lag, a.tau_v, a.tau_h, a.foot_height, a.json) == (50.0, 7, 0.2, 0.03, 0.05, "o.json")
    for mod in ("bvh", "meshes", "render"):
        src = open(os.path.join(ROOT, "globalegomocap_amd", mod + ".py")).read()
        assert 'p.add_argument("--upright", action="store_true"' in src, mod


def test_record_layout_and_declarations():
    import ctypes
    import re
    from globalegomocap_amd import _capi
    assert ctypes.sizeof(_capi.GemGroundRecord) == 8 * _capi.GROUND_RECORD_DOUBLES == 384
    assert _capi.GemGroundRecord.crt.offset == 23 * 8 and _capi.GemGroundRecord.points.offset == 80
    header = open(os.path.join(ROOT, "include", "gem_hip.h")).read()
    for name, value in (("GEM_GROUND_RECORD_DOUBLES", _capi.GROUND_RECORD_DOUBLES), ("GEM_GROUND_LDS_FRAMES", _capi.GROUND_LDS_FRAMES),
                        ("GEM_GROUND_NO_BODY", _capi.GROUND_NO_BODY), ("GEM_GROUND_BAD_SEQUENCE", _capi.GROUND_BAD_SEQUENCE)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    for k, source in enumerate(_capi.GROUND_SOURCES):
        assert re.search(r"#define GEM_GROUND_SOURCE_%s %d\b" % (source.upper(), k), header) and T.SOURCES[k] == source
    for name, n_args in (("gem_ground_plane_work", 3), ("gem_ground_plane", 13), ("gem_similarity_compose", 5)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == n_args == len(_capi.SIGNATURES[name][1]), name


def test_the_report_row_of_an_estimate():
    from globalegomocap_amd import ground
    x, normal, floor, _ = T.walker_world(40)
    e = T.estimate(x)
    rec = np.zeros(48)
    rec[1] = e["source"]
    rec[2:5], rec[5], rec[6:9], rec[9] = e["n"], e["d"], e["u0"], e["tilt_cos"]
    rec[10:15] = e["points"], e["inliers"], e["rms"], e["spread"], e["extent"]
    rec[15:17], rec[17], rec[18], rec[19], rec[20] = e["contact_frames"], 0.01, e["penetration"], e["lift_max"], e["skate_pairs"]
    rec[21], rec[22], rec[23:36] = 40, 5, e["crt"]
    g = ground.GroundEstimate(rec, fps=30.0)
    assert g.source == "plane" and g.points == e["points"] and g.frames == 40 and g.lag == 5
    assert abs(g.skate - 0.3) < 1e-15 and abs(g.tilt_deg - T.angle_deg(e["n"], e["u0"])) < 1e-9
    assert g.contact_share == tuple(c / 40 for c in e["contact_frames"])
    d = g.as_dict()
    assert d["source"] == "plane" and len(d["crt"]) == 13 and d["normal"] == e["n"].tolist()
    assert "plane" in g.line() and "skate" in g.line()
    text = ground.report_text({"estimated": g, "optimized": g})
    assert "skate (m/s)" in text and text.count("plane") == 2


def test_a_chunks_ground_record_stays_out_of_the_summary():
    from collections import OrderedDict
    from globalegomocap_amd import report as R
    seq = np.zeros((3, 15, 3))
    for raw in (np.arange(7.0), None):          # (a row of the device report, or the chunk-by-chunk route)
        reports = []
        for k in range(2):
            res = OrderedDict(zip(R.QUALITY_KEYS, (np.arange(7.0) + k).tolist()))
            res["ground"] = {"source": "plane", "skate": 0.1 * k}
            reports.append(R.ChunkReport(result=res, est=seq, opt=seq, gt=None, mid=None, raw=None if raw is None else raw + k, views=None))
        summary, results, est, opt, gt = R.sequence_result(reports, None, False)
        assert list(summary) == list(R.QUALITY_KEYS) and summary[R.QUALITY_KEYS[2]] == 2.5
        assert [r["ground"]["skate"] for r in results] == [0.0, 0.1] and gt is None
