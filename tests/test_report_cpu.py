"""The report module on the host (`globalegomocap_amd/report.py`): a sequence's summary, printed lines and return value from
hand-made ChunkReports, where a chunk's files go, what `result_pose.pkl` holds, and which writer gets which directory and which
sequences."""
from collections import OrderedDict

import numpy as np
import pytest

from globalegomocap_amd import report as R
from globalegomocap_amd.engine import WindowEngine

KEYS = list(WindowEngine.ERROR_KEYS) + ["joints_error"]
SEPARATOR, END = "-----------------------------------------", "-------------------------------------------------------------"


def _poses(n, seed):
    return np.random.default_rng(seed).normal(size=(n, 15, 3))


def _with_gt(seed, n, raw=True):
    row = np.random.default_rng(seed).uniform(0.01, 0.2, 17 + 15)
    res = OrderedDict(zip(KEYS[:17], row[:17].tolist()))
    res["joints_error"] = row[17:].copy()
    return R.ChunkReport(res, _poses(n, seed), _poses(n, seed + 1), _poses(n, seed + 2), _poses(n, seed + 3), row if raw else None, None)


def _without_gt(seed, n):
    row = np.random.default_rng(seed).uniform(0.01, 0.2, 7)
    return R.ChunkReport(OrderedDict(zip(R.QUALITY_KEYS, row.tolist())), _poses(n, seed), _poses(n, seed + 1), None, None, row, None)


def _printed(lines, summary, title, tail):
    out = ["sequence: %s" % title] if title is not None else []
    out += [SEPARATOR if line is None else "{}: {}".format(line[0], summary[line[1]]) for line in lines]
    return "\n".join(out + tail + [END]) + "\n"          # (`joints_error` prints over several lines)


@pytest.mark.parametrize("case", ["every raw row", "one raw row missing"])
def test_sequence_result_with_ground_truth(case, capsys):
    reports = [_with_gt(1, 4), _with_gt(11, 3, raw=case == "every raw row"), _with_gt(21, 5)]
    summary, results, est, opt, gt = R.sequence_result(reports, "walk", True)
    assert list(summary) == KEYS and results == [r.result for r in reports]
    if case == "every raw row":          # one mean over the rows of the device report
        mean = np.mean(np.stack([r.raw for r in reports]), axis=0)
        want = {k: float(mean[i]) for i, k in enumerate(KEYS[:17])}
        want["joints_error"] = mean[17:]
    else:                                # key by key over the chunks' dicts
        want = {k: float(np.average([r.result[k] for r in reports])) for k in KEYS[:17]}
        want["joints_error"] = np.mean([r.result["joints_error"] for r in reports], axis=0)
    for k in KEYS[:17]:
        assert isinstance(summary[k], float) and summary[k] == want[k], k
    assert summary["joints_error"].shape == (15,) and np.array_equal(summary["joints_error"], want["joints_error"])
    assert capsys.readouterr().out == _printed(R.SUMMARY_LINES, summary, "walk", ["joints error is: {}".format(summary["joints_error"])])
    for got, name in ((est, "est"), (opt, "opt"), (gt, "gt")):
        assert got.shape == (12, 15, 3) and np.array_equal(got, np.concatenate([getattr(r, name) for r in reports])), name
    R.sequence_result(reports, None, False)
    assert capsys.readouterr().out == ""


def test_sequence_result_without_ground_truth(capsys):
    reports = [_without_gt(3, 4), _without_gt(13, 6)]
    out = R.sequence_result(reports, None, True)
    assert len(out) == 5
    summary, results, est, opt, gt = out
    assert list(summary) == list(R.QUALITY_KEYS) and results == [r.result for r in reports]
    mean = np.mean(np.stack([r.raw for r in reports]), axis=0)
    for i, k in enumerate(R.QUALITY_KEYS):
        assert isinstance(summary[k], float) and summary[k] == float(mean[i]), k
    assert capsys.readouterr().out == _printed(R.QUALITY_LINES, summary, None, [])
    assert gt is None
    assert np.array_equal(est, np.concatenate([r.est for r in reports])) and np.array_equal(opt, np.concatenate([r.opt for r in reports]))


def test_sequence_result_of_no_chunk(capsys):
    summary, results, est, opt, gt = R.sequence_result([], "empty", True)
    assert summary == OrderedDict() and results == [] and capsys.readouterr().out == ""
    assert est.shape == opt.shape == gt.shape == (0, 15, 3)


def test_chunk_report_sequences_and_views():
    r = _with_gt(5, 3)
    assert r.sequences() == (r.est, r.opt, r.gt)
    r.views = ("e", "o", "g")
    assert r.sequences() == ("e", "o", "g")
    r.drop_views()
    assert r.views is None and r.sequences() == (r.est, r.opt, r.gt)
    with pytest.raises(AttributeError):
        r.anything_else = 1


def test_result_dir():
    assert R.result_dir("out", "a/b/c") == "out/b/c"
    assert R.result_dir("out", "a/b/c/") == "out/c/"          # as it stands ...
    import os
    assert R.result_dir("out", os.path.normpath("a/b/c/")) == "out/b/c"          # ... and after the caller's normalisation
    assert R.result_dir("out", "./c") == "out/./c"
    assert R.result_dir("/x/y", "c") == "/x/y/c"


@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("ground_truth", [True, False])
def test_result_pose_dict(ground_truth, smooth):
    est, opt, mid, gt = (_poses(4, s) for s in range(4))
    d = R.result_pose_dict(list(est), opt if smooth else list(opt), mid, gt if ground_truth else None, smooth)
    assert list(d) == ["estimated_pose", "optimized_pose", "mid_optimized_pose"] + (["gt_pose"] if ground_truth else [])
    for k, want in (("estimated_pose", est), ("mid_optimized_pose", mid)) + ((("gt_pose", gt),) if ground_truth else ()):
        assert isinstance(d[k], list) and len(d[k]) == 4 and d[k][0].shape == (15, 3) and np.array_equal(np.asarray(d[k]), want), k
    assert isinstance(d["optimized_pose"], np.ndarray if smooth else list) and np.array_equal(np.asarray(d["optimized_pose"]), opt)
    if not smooth:
        assert d["optimized_pose"][0].shape == (15, 3) and d["optimized_pose"][0].dtype == np.float64


def test_write_result_outputs_calls_the_writers_asked_for(monkeypatch):
    from globalegomocap_amd import meshes, render
    calls = []
    monkeypatch.setattr(meshes, "write_result_meshes", lambda *a: calls.append(("meshes",) + a))
    monkeypatch.setattr(render, "write_result_frames", lambda *a: calls.append(("frames",) + a))
    monkeypatch.setattr(render, "write_result_camera_frames", lambda *a: calls.append(("camera",) + a))
    r = _with_gt(7, 3)
    cams, heat = np.arange(10), np.arange(10) * 2
    R.Outputs().write("engine", "d/studio/chunk_2", r.sequences())
    assert calls == []
    R.Outputs(mesh_root="m").write("engine", "d/studio/chunk_2", r.sequences())
    assert [c[:3] for c in calls] == [("meshes", "engine", "m/studio/chunk_2")] and all(x is y for x, y in zip(calls[0][3:], (r.est, r.opt, r.gt)))
    del calls[:]
    # the device views where the report left them, every writer, the camera's frames from the chunk's first frame on
    r.views = ("est_d", "opt_d", "gt_d")
    R.Outputs("m", "f", "c").write("engine", "d/studio/chunk_2", r.sequences(), cams, heat, 4)
    assert [c[:6] for c in calls[:2]] == [("meshes", "engine", "m/studio/chunk_2", "est_d", "opt_d", "gt_d"),
                                          ("frames", "engine", "f/studio/chunk_2", "est_d", "opt_d", "gt_d")] and len(calls) == 3
    name, engine, folder, est, opt, c, h, gt = calls[2]
    assert (name, engine, folder, est, opt, gt) == ("camera", "engine", "c/studio/chunk_2", "est_d", "opt_d", "gt_d")
    assert c.tolist() == [4, 5, 6, 7, 8] and h.tolist() == [8, 10, 12, 14, 16]          # len("est_d") frames from frame 4
    del calls[:]
    # without ground truth and without views: the host arrays, None for the third
    q = _without_gt(9, 3)
    R.Outputs(render="f", render_camera="c").write("engine", "chunk_0", q.sequences(), cams=cams, heat=heat)
    assert [c[0] for c in calls] == ["frames", "camera"] and calls[0][2] == "f/chunk_0" and calls[1][2] == "c/chunk_0"
    assert calls[0][3] is q.est and calls[0][4] is q.opt and calls[0][5] is None and calls[1][7] is None
    assert calls[1][5].tolist() == [0, 1, 2] and calls[1][6].tolist() == [0, 2, 4]
