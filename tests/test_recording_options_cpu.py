"""How the options of a recording's camera route and depth route travel: from the command lines and the wrapper functions to the two
functions that spell them out, `prepare.prepare_spans` (the .mat route) and `detections.recording_from_detections` (the detection
route).  Those two are replaced by recorders that bind what they are called with to the real function's signature, defaults applied,
so that every test compares the arguments that would take effect -- however the caller spelled them -- with a literal.  No file of a
recording is opened and no device is touched."""
import inspect
import os

import numpy as np
import pytest

from globalegomocap_amd import continuous, detections, prepare, slam_scale
from globalegomocap_amd.camera import DEFAULT_CALIBRATION

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BONES = np.array([0.0, 0.2, 0.3, 0.25, 0.1, 0.2, 0.3, 0.25, 0.1, 0.5, 0.45, 0.15, 0.5, 0.45, 0.15])


class _Report:
    per_chunk = ()

    def line(self):
        return "a scale report"

    def as_dict(self):
        return {}

    def knot_lines(self):
        return ["a knot"]


class _Recording:
    """What a preparation returns, as far as its callers look at it."""
    depth_report = bridge_report = None
    chunks = ()

    def __init__(self):
        self.scale_report = _Report()
        self.written = []

    def write_chunk(self, i, out_dir):
        self.written.append(("chunk", i, out_dir))

    def write_chunks(self, out_root):
        self.written.append(("chunks", out_root))


class _Recorder:
    """Stands in for `real`: binds every call to its signature (an unknown keyword is Python's TypeError, as in the real function),
    keeps the arguments with the defaults filled in, and returns a `_Recording`."""

    def __init__(self, real):
        self.signature, self.calls, self.returned = inspect.signature(real), [], []

    def __call__(self, *args, **kwargs):
        bound = self.signature.bind(*args, **kwargs)
        bound.apply_defaults()
        self.calls.append(dict(bound.arguments))
        self.returned.append(_Recording())
        return self.returned[-1]

    @property
    def only(self):
        assert len(self.calls) == 1, self.calls
        return self.calls[0]


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            assert isinstance(g, np.ndarray) and g.dtype == w.dtype and np.array_equal(g, w), k
        else:
            assert type(g) is type(w) and g == w, (k, g, w)


@pytest.fixture
def routes(monkeypatch):
    """Both route functions replaced by recorders -> (the .mat route's, the detection route's)."""
    mat, det = _Recorder(prepare.prepare_spans), _Recorder(detections.recording_from_detections)
    monkeypatch.setattr(prepare, "prepare_spans", mat)
    monkeypatch.setattr(detections, "recording_from_detections", det)
    return mat, det


# ------------------------------------------------------------------------------------------------------------------ the wrappers
# a distinct value that is not the default for every option of the camera route and of the depth route
CAMERA_ROUTE = dict(scale="drift", bridge=0.4, lag=4, tau=0.2, min_pairs=7, knot=60, stiffness=2.5)
MAT_OPTIONS = dict(CAMERA_ROUTE, depth="bones", bones=BONES, neck_depth=0.31, min_peak=0.2, peaks="subpixel")
DET_OPTIONS = dict(bridge=0.4, lag=4, tau=0.2, min_pairs=7, knot=60, stiffness=2.5, depth="bones", bones=BONES, neck_depth=0.31, sigma=2.5, first_id=5,
                   camera_model_path="c.json", device="cuda:1", gt_start_frame=2)


def _mat_call(spans, mat_start_frame, **more):
    return dict(dict(slam_result_path="t", heatmap_dir="h", depth_dir=None, gt_path=None, spans=spans, fps=30, mat_start_frame=mat_start_frame,
                     camera_model_path="c.json", device=None, timings=None, **MAT_OPTIONS), **more)


def test_main_hands_every_option_to_the_mat_route(routes, tmp_path, capsys):
    mat, _ = routes
    rec = prepare.main("t", "h", None, None, 3, 90, str(tmp_path), 30, camera_model_path="c.json", **MAT_OPTIONS)
    _same(mat.only, _mat_call([(3, 90)], 3))
    assert rec is mat.returned[0] and rec.written == [("chunk", 0, str(tmp_path))]
    prepare.main("t", "h", None, None, 3, 90, str(tmp_path), 30, 2, "c.json", **MAT_OPTIONS)
    _same(mat.calls[1], _mat_call([(3, 90)], 2))
    with pytest.raises(TypeError):
        prepare.main("t", "h", None, None, 3, 90, str(tmp_path), 30, min_pears=3, **MAT_OPTIONS)
    assert len(mat.calls) == 2


def test_prepare_sequence_hands_every_option_to_the_mat_route(routes, tmp_path):
    mat, _ = routes
    rec = prepare.prepare_sequence("t", "h", None, None, 3, 90, 30, test_size=20, out_root=str(tmp_path), camera_model_path="c.json", verbose=False,
                                   **MAT_OPTIONS)
    _same(mat.only, _mat_call([(3, 23), (23, 43), (43, 63), (63, 83)], 3))
    assert rec is mat.returned[0] and rec.written == [("chunks", str(tmp_path))]
    rec = prepare.prepare_sequence("t", "h", None, None, 3, 90, 30, 2, 20, None, "c.json", False, **MAT_OPTIONS)
    _same(mat.calls[1], _mat_call([(3, 23), (23, 43), (43, 63), (63, 83)], 2))
    assert rec.written == []
    with pytest.raises(TypeError):
        prepare.prepare_sequence("t", "h", None, None, 3, 90, 30, verbose=False, min_pears=3, **MAT_OPTIONS)
    assert len(mat.calls) == 2


def test_prepare_continuous_hands_every_option_to_the_mat_route(routes):
    mat, _ = routes
    rec = prepare.prepare_continuous("t", "h", None, None, 3, 90, 30, camera_model_path="c.json", verbose=False, **MAT_OPTIONS)
    _same(mat.only, _mat_call([(3, 90)], 3))
    assert rec is mat.returned[0] and rec.written == []
    prepare.prepare_continuous("t", "h", None, None, 3, 90, 30, 2, "c.json", False, **MAT_OPTIONS)
    _same(mat.calls[1], _mat_call([(3, 90)], 2))
    with pytest.raises(TypeError):
        prepare.prepare_continuous("t", "h", None, None, 3, 90, 30, verbose=False, min_pears=3, **MAT_OPTIONS)
    assert len(mat.calls) == 2


def test_the_wrappers_print_the_report_they_printed(routes, tmp_path, capsys):
    """(`_Recording` has a scale report and no chunks: one line each, where the wrapper is verbose.)"""
    prepare.main("t", "h", "d", None, 3, 90, str(tmp_path), 30, scale=1.0)
    prepare.prepare_sequence("t", "h", "d", None, 3, 90, scale=1.0)
    prepare.prepare_continuous("t", "h", "d", None, 3, 90, scale=1.0)
    prepare.prepare_continuous("t", "h", "d", None, 3, 90, scale=1.0, verbose=False)
    assert capsys.readouterr().out == "a scale report\n" * 3


def test_continuous_from_detections_hands_every_option_to_the_detection_route(routes):
    _, det = routes
    rec = detections.continuous_from_detections("t", "k", None, "drift", 3, 90, 30, **DET_OPTIONS)
    _same(det.only, dict(slam_result_path="t", detections="k", gt_path=None, scale="drift", spans=[(3, 90)], fps=30, **DET_OPTIONS))
    assert rec is det.returned[0]
    detections.continuous_from_detections("t", "k", scale=2.0, start_frame=np.int64(3), end_frame=90.0)
    _same(det.calls[1], dict(slam_result_path="t", detections="k", gt_path=None, scale=2.0, spans=[(3, 90)], fps=25, depth=None, sigma=1.5, first_id=0,
                             camera_model_path=None, device=None, gt_start_frame=None, lag=None, tau=0.10, min_pairs=50, bridge=None, bones=None,
                             neck_depth=None, knot=None, stiffness=1.0))
    assert all(type(v) is int for v in det.calls[1]["spans"][0])
    with pytest.raises(TypeError):
        detections.continuous_from_detections("t", "k", None, "drift", 3, 90, 30, min_pears=3)
    assert len(det.calls) == 2


# ------------------------------------------------------------------------------------------------------------------ the command lines
@pytest.fixture
def files(tmp_path):
    """A bone-length file and a one-line trajectory for the command lines that read them themselves."""
    np.save(str(tmp_path / "bones.npy"), BONES)
    (tmp_path / "traj.txt").write_text("0.0 0 0 0 0 0 0 1\n")
    return {"bones": str(tmp_path / "bones.npy"), "slam": str(tmp_path / "traj.txt"), "json": str(tmp_path / "out" / "scale.json")}


@pytest.fixture
def optimisers(monkeypatch):
    """`optimize_recording`, `optimize_continuous` and `detections_from_args` replaced -> the calls they got, by name."""
    from globalegomocap_amd import whole_sequence
    calls = {"optimize_recording": [], "optimize_continuous": [], "detections_from_args": []}
    monkeypatch.setattr(whole_sequence, "optimize_recording", lambda *a, **k: calls["optimize_recording"].append((a, k)))
    monkeypatch.setattr(continuous, "optimize_continuous", lambda *a, **k: calls["optimize_continuous"].append((a, k)))

    def detections_from_args(a):
        calls["detections_from_args"].append(a)
        return "DETECTIONS"
    monkeypatch.setattr(detections, "detections_from_args", detections_from_args)
    return calls


DRIFT = ["--scale", "drift", "--knot", "4", "--stiffness", "2", "--fps", "30"]          # 4 s at 30 fps: knots 120 frames apart
TRACK = DRIFT + ["--slam", "t", "--bridge", "0.4", "--start", "3", "--end", "90", "--mat_start", "2", "--camera", "c.json"]
CHUNKS = ["--test_size", "20", "--out", "o", "--optimize"]
MINIMAL = ["--slam", "t", "--gt", "g", "--start", "0", "--end", "50"]
MAT_DEFAULTS = dict(slam_result_path="t", heatmap_dir="h", depth_dir="d", gt_path="g", fps=25, mat_start_frame=0, camera_model_path=DEFAULT_CALIBRATION,
                    device=None, timings=None, scale=None, lag=None, tau=0.10, min_pairs=50, bridge=None, depth=None, bones=None, neck_depth=None,
                    min_peak=None, peaks=None, knot=None, stiffness=1.0)
DET_DEFAULTS = dict(slam_result_path="t", detections="DETECTIONS", gt_path="g", scale=None, fps=25, depth=None, sigma=1.5, first_id=0,
                    camera_model_path=DEFAULT_CALIBRATION, device=None, gt_start_frame=None, lag=None, tau=0.10, min_pairs=50, bridge=None, bones=None,
                    neck_depth=None, knot=None, stiffness=1.0)


def _bones(files):
    return ["--depth_from", "bones", "--bones", files["bones"], "--neck_depth", "0.31"]


def test_prepare_command_line_to_the_mat_route(routes, optimisers, files, capsys):
    mat, _ = routes
    prepare._cli(["--heatmaps", "h", "--min_peak", "0.2", "--peaks", "subpixel"] + _bones(files) + TRACK + CHUNKS)
    _same(mat.only, dict(slam_result_path="t", heatmap_dir="h", depth_dir=None, gt_path=None, spans=[(3, 23), (23, 43), (43, 63), (63, 83)], fps=30.0,
                         mat_start_frame=2, camera_model_path="c.json", device=None, timings=None, scale="drift", lag=None, tau=0.10, min_pairs=50,
                         bridge=0.4, depth="bones", bones=BONES, neck_depth=0.31, min_peak=0.2, peaks="subpixel", knot=120, stiffness=2.0))
    assert mat.returned[0].written == [("chunks", "o")]
    assert optimisers["optimize_recording"] == [((mat.returned[0], "c.json"), {"ground_truth": False})]
    prepare._cli(["--heatmaps", "h", "--depths", "d", "--out", "o"] + MINIMAL)
    _same(mat.calls[1], dict(MAT_DEFAULTS, spans=[]))
    assert len(optimisers["optimize_recording"]) == 1
    assert capsys.readouterr().out == "a scale report\n" * 2


def test_detections_command_line_to_the_detection_route(routes, optimisers, files, capsys):
    _, det = routes
    detections._cli(["--keypoints", "k", "--sigma", "2.5", "--first_id", "5"] + _bones(files) + TRACK + CHUNKS)
    _same(det.only, dict(slam_result_path="t", detections="DETECTIONS", gt_path=None, scale="drift", spans=[(3, 23), (23, 43), (43, 63), (63, 83)],
                         fps=30.0, depth="bones", sigma=2.5, first_id=0, camera_model_path="c.json", device=None, gt_start_frame=2, lag=None, tau=0.10,
                         min_pairs=50, bridge=0.4, bones=BONES, neck_depth=0.31, knot=120, stiffness=2.0))
    a, = optimisers["detections_from_args"]
    assert (a.keypoints, a.first_id, a.depth, a.depths) == ("k", 5, None, None)
    assert det.returned[0].written == [("chunks", "o")]
    assert optimisers["optimize_recording"] == [((det.returned[0], "c.json"), {"ground_truth": False})]
    detections._cli(["--keypoints", "k", "--optimize"] + MINIMAL)
    _same(det.calls[1], dict(DET_DEFAULTS, spans=[]))
    assert det.returned[1].written == []
    assert optimisers["optimize_recording"][1] == ((det.returned[1], DEFAULT_CALIBRATION), {"ground_truth": True})
    assert capsys.readouterr().out == "a scale report\n" * 2


def test_continuous_command_line_to_both_routes(routes, optimisers, files, capsys):
    mat, det = routes
    more = ["--stride", "4", "--final_smooth", "false", "--save_pose", "p"]
    continuous._cli(["--heatmaps", "h", "--min_peak", "0.2", "--peaks", "subpixel"] + _bones(files) + TRACK + more)
    _same(mat.only, dict(slam_result_path="t", heatmap_dir="h", depth_dir=None, gt_path=None, spans=[(3, 90)], fps=30.0, mat_start_frame=2,
                         camera_model_path="c.json", device=None, timings=None, scale="drift", lag=None, tau=0.10, min_pairs=50, bridge=0.4,
                         depth="bones", bones=BONES, neck_depth=0.31, min_peak=0.2, peaks="subpixel", knot=120, stiffness=2.0))
    continuous._cli(["--keypoints", "k", "--sigma", "2.5", "--first_id", "5"] + _bones(files) + TRACK + more)
    _same(det.only, dict(slam_result_path="t", detections="DETECTIONS", gt_path=None, scale="drift", spans=[(3, 90)], fps=30.0, depth="bones", sigma=2.5,
                         first_id=0, camera_model_path="c.json", device=None, gt_start_frame=2, lag=None, tau=0.10, min_pairs=50, bridge=0.4,
                         bones=BONES, neck_depth=0.31, knot=120, stiffness=2.0))
    a, = optimisers["detections_from_args"]
    assert (a.keypoints, a.first_id, a.depth, a.depths) == ("k", 5, None, None)
    for (args, kwargs), rec in zip(optimisers["optimize_continuous"], (mat.returned[0], det.returned[0])):
        assert args[:2] == (rec, "c.json") and (kwargs["ground_truth"], kwargs["stride"], kwargs["final_smooth"], kwargs["save_pose"]) == (False, 4, False, "p")
    continuous._cli(["--heatmaps", "h", "--depths", "d"] + MINIMAL)
    _same(mat.calls[1], dict(MAT_DEFAULTS, spans=[(0, 50)]))
    continuous._cli(["--keypoints", "k"] + MINIMAL)
    _same(det.calls[1], dict(DET_DEFAULTS, spans=[(0, 50)]))
    a = optimisers["detections_from_args"][1]
    assert (a.first_id, a.depth, a.depths) == (0, None, None)
    assert [(args[1], kwargs["ground_truth"], kwargs["stride"]) for args, kwargs in optimisers["optimize_continuous"][2:]] == [(DEFAULT_CALIBRATION, True, 8)] * 2
    assert capsys.readouterr().out == "a scale report\n" * 4          # (the .mat route's wrapper and the detection route's command line print it)


def test_slam_scale_command_line_to_both_routes(routes, optimisers, files, monkeypatch, capsys):
    mat, det = routes
    compared = []
    monkeypatch.setattr(slam_scale, "umeyama_scales", lambda *a: compared.append(a) or [])
    spans = [(3, 23), (23, 43), (43, 63), (63, 83), (83, 90)]
    common = ["--slam", files["slam"], "--start", "3", "--end", "90", "--lag", "4", "--tau", "0.2", "--min_pairs", "7", "--test_size", "20", "--json", files["json"],
              "--gt", "g", "--mat_start", "2", "--camera", "c.json"] + DRIFT + _bones(files)
    est = slam_scale._cli(["--heatmaps", "h", "--min_peak", "0.2"] + common)
    _same(mat.only, dict(slam_result_path=files["slam"], heatmap_dir="h", depth_dir=None, gt_path=None, spans=spans, fps=30.0, mat_start_frame=3,
                         camera_model_path="c.json", device=None, timings=None, scale="drift", lag=4, tau=0.2, min_pairs=7, bridge=None, depth="bones",
                         bones=BONES, neck_depth=0.31, min_peak=0.2, peaks=None, knot=120, stiffness=2.0))
    assert est is mat.returned[0].scale_report and os.path.exists(files["json"])
    slam_scale._cli(["--keypoints", "k", "--first_id", "5"] + common)
    _same(det.only, dict(slam_result_path=files["slam"], detections="DETECTIONS", gt_path=None, scale="drift", spans=spans, fps=30.0, depth="bones", sigma=1.5,
                         first_id=0, camera_model_path="c.json", device=None, gt_start_frame=None, lag=4, tau=0.2, min_pairs=7, bridge=None, bones=BONES,
                         neck_depth=0.31, knot=120, stiffness=2.0))
    assert optimisers["detections_from_args"][0].first_id == 5
    assert [(c[1], c[2], c[3], c[4]) for c in compared] == [(mat.returned[0], "g", 30.0, 2), (det.returned[0], "g", 30.0, 2)]
    assert capsys.readouterr().out == "a scale report\na knot\n" * 2
    slam_scale._cli(["--slam", "t", "--heatmaps", "h", "--depths", "d", "--start", "0", "--end", "50"])
    _same(mat.calls[1], dict(MAT_DEFAULTS, gt_path=None, scale="auto", spans=[(0, 50)]))
    slam_scale._cli(["--slam", "t", "--keypoints", "k", "--start", "0", "--end", "50"])
    _same(det.calls[1], dict(DET_DEFAULTS, gt_path=None, scale="auto", spans=[(0, 50)]))
    assert len(compared) == 2


# ------------------------------------------------------------------------------------------------------------------ the help texts
@pytest.mark.parametrize("module", ["prepare", "detections", "continuous", "slam_scale"])
def test_help_texts_are_what_they_were(module, monkeypatch):
    """`--help` of the four command lines at 100 columns against the texts kept under tests/golden/ (taken before the options'
    declarations were shared)."""
    import importlib
    monkeypatch.setenv("COLUMNS", "100")
    p = importlib.import_module("globalegomocap_amd." + module)._parser()
    p.prog = "python -m globalegomocap_amd." + module
    with open(os.path.join(GOLDEN, "help_%s.txt" % module)) as f:
        assert p.format_help() == f.read()
