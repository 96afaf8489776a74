"""Foot-skate clean-up without a GPU: the numpy twin (tests/foot_lock_twin.py) on the synthetic walker and on
three hand-made sequences -- what is copied bit for bit, that a pinned foot stands still on the floor, the bone lengths, invariance
under rigid motions, how many pins are missed and how much slide is left --, and the wiring of `foot_lock` through the outputs record,
the entry points, the command lines and the C interface (its refusals need no device)."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest

import foot_lock_twin as T
import ground_twin as GT
from globalegomocap_amd.synth_walk import _rotvec_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN, MARGIN_DEGENERATE, MARGIN_SNAP = 1e-9, 0.5e-9, 0.5e-12          # as in tests/test_foot_lock_gpu.py
BLENDS = (3, 8)
CASES = list(T.WALKER_CASES) + list(T.LONG_STANCE) + list(T.HAND_MADE)
OTHERS = [j for j in range(15) if j not in T.MOVED]


@functools.lru_cache(maxsize=None)
def _case(name, blend=3):
    """(the sequence, ground_twin's estimate of it, the twin's result at that plane): computed once, never changed."""
    x = T.case_input(name)
    x.setflags(write=False)
    g = GT.estimate(x)
    return x, g, T.lock(x, g["n"], g["d"], blend=blend)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _lengths(x, side):
    hip, kn, an, ft = T.LEGS[side]
    norm = lambda v: np.sqrt((v * v).sum(-1))          # noqa: E731
    return norm(x[:, kn] - x[:, hip]), norm(x[:, an] - x[:, kn]), norm(x[:, ft] - x[:, an])


@pytest.mark.parametrize("blend", BLENDS)
@pytest.mark.parametrize("name", CASES)
def test_what_is_copied_what_is_pinned_and_the_bones(name, blend):
    x, g, r = _case(name, blend)
    y = r["sequence"]
    assert r["margin"] > MARGIN and r["margin_degenerate"] > MARGIN_DEGENERATE and r["margin_snap"] > MARGIN_SNAP
    assert np.array_equal(_bits(y[:, OTHERS]), _bits(x[:, OTHERS]))
    q2 = T.foot_points(y)
    for side, (hip, kn, an, ft) in enumerate(T.LEGS):
        still = ~(r["delta"][:, side] != 0.0).any(axis=1)
        assert np.array_equal(_bits(y[still, kn:ft + 1]), _bits(x[still, kn:ft + 1]))
        assert (r["kind"][still, side] == -1).all() and (r["kind"][~still, side] >= 0).all()
        kind = r["kind"][:, side]
        for (s, e), a in zip(r["runs"][side], r["anchors"][side]):
            if np.isin(kind[s:e + 1], (-1, 0, 1)).all():          # every pin of the run is held
                assert np.abs(q2[s:e + 1, side] - a).max() <= 1e-12, (name, side, s)
                assert np.abs(q2[s:e + 1, side] @ g["n"] - g["d"]).max() <= 1e-12, (name, side, s)
        (t0, s0, f0), (t1, s1, f1) = _lengths(x, side), _lengths(y, side)
        fixed = np.isin(kind, (-1, 0, 3))          # (folded on the axis, a leg keeps its lengths too)
        assert np.abs(t1 - t0)[fixed].max(initial=0.0) <= 1e-12 and np.abs(s1 - s0)[fixed].max(initial=0.0) <= 1e-12
        for a, b in ((t0, t1), (s0, s1)):
            ratio = (b / a)[~fixed]
            assert (ratio >= 1.0 - 1e-12).all() and (ratio <= 1.05 + 1e-12).all()
        assert np.abs(f1 - f0).max() <= 1e-12
    assert r["frames"] == len(x) and r["changed"] == int(((r["delta"] != 0.0).any(axis=(1, 2))).sum())
    assert r["pinned_right"] == sum(e - s + 1 for s, e in r["runs"][0]) and r["pinned_left"] == sum(e - s + 1 for s, e in r["runs"][1])


def test_sequences_without_a_stance_and_the_noise_free_walker_come_back_bit_for_bit():
    for name in ("3 frames", "6 frames"):
        x, g, r = _case(name)
        assert GT.SOURCES[g["source"]] == "body" and r["status"] == T.NO_CONTACT and r["runs"] == [[], []]
        assert np.array_equal(_bits(r["sequence"]), _bits(x))
    for blend in BLENDS:
        x, g, r = _case("98 frames without noise", blend)
        assert r["status"] == T.STATUS_OK and r["runs_right"] == 5 and r["runs_left"] == 5
        assert np.array_equal(_bits(r["sequence"]), _bits(x))
        assert r["delta_max"] == 0.0 and r["lengthened"] == 0 and r["unreachable"] == 0 and r["changed"] == 0


def test_the_hand_made_frames_take_the_branches_the_walker_never_takes():
    x, g, r = _case("knee on the line")
    assert np.array_equal(g["n"], [0.0, 0.0, 1.0]) and r["margin_degenerate"] == 1e-9          # (a direction of length exactly 0)
    kinds = r["kind"][:7]
    assert (kinds[:, 0] == 0).any() and (kinds[:, 1] == 0).any() and (kinds == 1).any()
    y = r["sequence"]
    for f in np.nonzero(kinds[:, 0] == 0)[0]:          # the right knee bends where the foot points: +y
        assert y[f, 8, 1] > 1e-3 and abs(y[f, 8, 0] - x[f, 8, 0]) < 1e-15
    for f in np.nonzero(kinds[:, 1] == 0)[0]:          # the left foot lies on the line too: the axis rule, x before y on equal size
        assert abs(y[f, 12, 0] - x[f, 12, 0]) > 1e-3 and abs(y[f, 12, 1] - x[f, 12, 1]) < 1e-15
    x, g, r = _case("hip raised")
    assert r["kind"][T.HAND_FRAME, 0] == 2 and r["unreachable"] == 1 and r["stretch_max"] == 1.05
    t, s, _ = _lengths(r["sequence"], 0)
    t0, s0, _ = _lengths(x, 0)
    assert abs(t[T.HAND_FRAME] / t0[T.HAND_FRAME] - 1.05) < 1e-12 and abs(s[T.HAND_FRAME] / s0[T.HAND_FRAME] - 1.05) < 1e-12
    assert T.lock(x, g["n"], g["d"], stretch=0.06)["unreachable"] == 0
    x, g, r = _case("target too near")
    assert r["kind"][T.HAND_FRAME, 0] == 3 and r["unreachable"] == 1
    y = r["sequence"][T.HAND_FRAME]
    fold = np.cross(y[8] - y[7], y[9] - y[7])
    assert np.sqrt(fold @ fold) < 1e-15          # hip, knee and ankle on one line


@pytest.mark.parametrize("blend", BLENDS)
@pytest.mark.parametrize("name", T.NOISY)
def test_unreachable_frames_and_the_slide_that_is_left(name, blend, capsys):
    x, g, r = _case(name, blend)
    after = GT.estimate(r["sequence"])
    pinned = r["pinned_right"] + r["pinned_left"]
    with capsys.disabled():
        print("%s, blend %d: %d of %d pinned frames unreachable, slide %.3e -> %.3e m/frame (a factor of %.0f), skate %.5f -> %.5f (a factor of %.1f)"
              % (name, blend, r["unreachable"], pinned, r["slide_before"], r["slide_after"], r["slide_before"] / max(r["slide_after"], 1e-300),
                 g["skate"], after["skate"], g["skate"] / max(after["skate"], 1e-300)))
    assert r["unreachable"] <= 0.05 * pinned
    assert r["slide_after"] <= r["slide_before"] / 10.0
    assert after["skate"] <= g["skate"] / 10.0


def test_both_branches_of_the_blend_length_and_continuity():
    gaps = set()
    for name in ("98 frames", "the first length in the work buffer"):
        for runs in _case(name, 8)[2]["runs"]:
            gaps |= {b[0] - a[1] for a, b in zip(runs, runs[1:])}
    assert min(gaps) < 16 <= max(gaps), sorted(gaps)
    # the easing reaches exactly 0 in the middle of a short gap (B = (s - e) / 2) and `blend` frames from a run in a long one, and
    # next to a run the correction is the run's own at its end frame, eased by k(1 / B)
    x, g, r = _case("the first length in the work buffer", 8)
    q, seen = T.foot_points(x), set()
    for side in range(2):
        d, runs, anchors = r["delta"][:, side], r["runs"][side], r["anchors"][side]
        for k, ((s0, e0), (s1, e1)) in enumerate(zip(runs, runs[1:])):
            gap = s1 - e0
            seen.add(gap <= 16)
            if gap <= 16 and gap % 2 == 0:
                assert not d[e0 + gap // 2].any()
            if gap > 16:
                assert not d[e0 + 8:s1 - 7].any() and d[e0 + 7].any() and d[s1 - 7].any()
            if gap >= 4:
                B = min(8.0, 0.5 * gap)
                np.testing.assert_allclose(d[e0 + 1], (anchors[k] - q[e0, side]) * T.ease(1.0 / B), rtol=0, atol=1e-15)
    assert seen == {True, False}
    assert T.ease(0.0) == 1.0 and T.ease(1.0) == 0.0 and T.ease(0.5) == 0.5 and T.ease(7.0) == 0.0


def test_a_rigid_motion_moves_the_result_along():
    """On every case but the two whose straight legs, with the foot on the line too, are bent towards a WORLD axis: that rule, the
    upright transform's, is the one step that looks at the world's axes."""
    Q, t = _rotvec_matrix((0.7, -1.1, 0.4)), np.array([3.0, -2.0, 0.5])
    exempt = []
    for name in CASES:
        x, g, r = _case(name)
        if r["axis_rule"]:
            exempt.append(name)
            continue
        n2 = g["n"] @ Q
        moved = T.lock(x @ Q + t, n2, g["d"] + n2 @ t)
        assert moved["margin"] > MARGIN and moved["axis_rule"] == 0, name
        for k in T.COUNTS:
            assert moved[k] == r[k], (name, k)
        np.testing.assert_allclose(moved["sequence"], r["sequence"] @ Q + t, rtol=0, atol=1e-10, err_msg=name)
    assert exempt == ["knee on the line", "hip raised"]


def test_options():
    x, g, r = _case("98 frames")
    loose = T.lock(x, g["n"], g["d"], snap=False)
    q2 = T.foot_points(loose["sequence"])
    for side in range(2):
        for (s, e) in loose["runs"][side]:
            if np.isin(loose["kind"][s:e + 1, side], (-1, 0, 1)).all():
                assert np.abs(q2[s:e + 1, side] - T.foot_points(x)[s:e + 1, side].mean(axis=0)).max() <= 1e-12
    assert T.lock(x, g["n"], g["d"], stretch=0.0)["unreachable"] == r["lengthened"] and T.lock(x, g["n"], g["d"], stretch=0.0)["stretch_max"] == 1.0
    assert T.lock(x, g["n"], g["d"], min_run=6)["runs_left"] < r["runs_left"] <= T.lock(x, g["n"], g["d"], min_run=1)["runs_left"]
    assert T.default_blend(25) == 3 and T.default_blend(2) == 1 and T.default_blend(50) == 6


# ------------------------------------------------------------------------------------------------------------------ the host's wiring
def test_the_new_keywords_are_keyword_only_with_their_defaults():
    from globalegomocap_amd import foot_lock, ground, optimizer, report, whole_sequence as ws
    for fn in (ws._settings, optimizer.main):
        par = inspect.signature(fn).parameters
        for name, default in (("foot_lock", False), ("foot_lock_stretch", None), ("foot_lock_blend", None)):
            assert par[name].kind is inspect.Parameter.KEYWORD_ONLY and par[name].default is default, (fn, name)
    par = inspect.signature(foot_lock.lock_feet).parameters
    want = dict(fps=25.0, lag=None, tau_v=ground.TAU_V, tau_h=ground.TAU_H, min_run=3, blend=None, snap=True, stretch=0.05, ground=None, stream=None)
    assert list(par) == ["engine", "sequences"] + list(want) and {k: par[k].default for k in want} == want
    assert foot_lock.default_blend(25) == T.default_blend(25) == 3 and foot_lock.default_blend(1) == 1 and foot_lock.default_blend(60) == 7
    fields = [f.name for f in report.Outputs.__dataclass_fields__.values()]
    assert fields[8:12] == ["video_quality", "foot_lock", "foot_lock_stretch", "foot_lock_blend"] and fields[12] == "upright" and len(fields) == 15
    o = report.Outputs()
    assert o.foot_lock is None and o.foot_lock_stretch is None and o.foot_lock_blend is None
    assert not report.Outputs(foot_lock=True)          # (the lock alone asks for no file)
    cfg = ws._settings("cam.json")
    assert cfg.foot_lock is False and cfg.outputs == report.Outputs()
    cfg = ws._settings("cam.json", bvh="b", foot_lock=True, foot_lock_stretch=0.1, foot_lock_blend=5)
    assert cfg.outputs == report.Outputs(bvh="b", foot_lock=True, foot_lock_stretch=0.1, foot_lock_blend=5)
    assert ws._settings("cam.json", bvh="b", foot_lock_stretch=0.1).outputs == report.Outputs(bvh="b")
    assert ws._settings("cam.json", bvh="b", upright=True, foot_lock=True).outputs == report.Outputs(bvh="b", upright=True, foot_lock=True)
    for bad in (dict(foot_lock_stretch=-0.1), dict(foot_lock_stretch=float("nan")), dict(foot_lock_blend=0)):
        with pytest.raises(ValueError, match="foot_lock"):
            ws._settings("cam.json", foot_lock=True, **bad)


class _Lock:
    def __init__(self, sequence):
        self.sequence = sequence


def test_outputs_without_the_switch_call_nothing_new_and_with_it_lock_once(monkeypatch):
    from globalegomocap_amd import bvh, foot_lock, ground, meshes, render, report
    calls = []
    for mod, name in ((meshes, "write_result_meshes"), (render, "write_result_frames"), (bvh, "write_result_bvh"),
                      (render, "write_result_camera_frames")):
        monkeypatch.setattr(mod, name, lambda *a, _n=name, **k: calls.append((_n, a, k)))
    monkeypatch.setattr(foot_lock, "lock_feet", lambda *a, **k: pytest.fail("no lock without foot_lock"))
    monkeypatch.setattr(ground, "estimate_ground", lambda *a, **k: pytest.fail("no estimate without upright"))
    est, opt = np.zeros((3, 15, 3)), np.ones((3, 15, 3))
    cams, heat = np.zeros((3, 4, 4)), np.zeros((3, 4, 4, 15))
    everything = dict(mesh_root="m", render="r", bvh="b", video="v", render_camera="c", video_camera="vc")
    for switch in ({}, dict(foot_lock=False), dict(foot_lock=None, foot_lock_stretch=0.2, foot_lock_blend=4)):
        del calls[:]
        o = report.Outputs(**everything, **switch)
        assert o.lock("engine", opt) is None
        assert o.write("engine", "d/studio/chunk_0", (est, opt, None), cams, heat) is None
        assert len(calls) == 6 and all(c[1][2] is est and c[1][3] is opt for c in calls)
        assert [c[2] for c in calls if "camera" not in c[0]] == [{}, {}, {"fps": 25},
                                                                  {"video": os.path.join("v", "studio", "chunk_0", "frames.avi"), "video_fps": 25,
                                                                   "video_quality": 90, "frames": False}]
    # with the switch: ONE lock per chunk, of the optimised sequence; its sequence reaches every writer but the camera's
    del calls[:]
    made = []

    def lock(engine, sequence, **k):
        made.append((sequence, k))
        return _Lock("the locked sequence")
    monkeypatch.setattr(foot_lock, "lock_feet", lock)
    o = report.Outputs(foot_lock=True, foot_lock_stretch=0.1, foot_lock_blend=4, bvh_fps=50, upright_lag=7, **everything)
    assert o.write("engine", "d/studio/chunk_0", (est, opt, None), cams, heat) is None
    assert len(made) == 1 and made[0][0] is opt and made[0][1] == dict(fps=50, lag=7, blend=4, stretch=0.1)
    assert len(calls) == 6 and all(c[1][2] is est for c in calls)
    assert [c[1][3] for c in calls if "camera" not in c[0]] == ["the locked sequence"] * 4
    assert all(c[1][3] is opt for c in calls if "camera" in c[0])
    assert all("foot_lock" not in c[2] and "locked" not in c[2] for c in calls)
    # a lock the caller made is used as it is; the defaults; the lock alone writes and locks nothing
    del calls[:]
    assert report.Outputs(foot_lock=True, bvh="b").write("engine", "d/studio/chunk_0", (est, opt, None), locked=_Lock("made before")) is None
    assert len(made) == 1 and calls[0][1][3] == "made before"
    report.Outputs(foot_lock=True, bvh="b").write("engine", "d/studio/chunk_0", (est, opt, None))
    assert len(made) == 2 and made[1][1] == dict(fps=25, lag=None, blend=None, stretch=0.05)
    report.Outputs(foot_lock=True, render_camera="c").write("engine", "d/studio/chunk_0", (est, opt, None), cams, heat)
    assert len(made) == 2
    # upright is estimated from the locked sequence where there is no ground truth
    seen = []
    monkeypatch.setattr(ground, "estimate_ground", lambda engine, ref, **k: seen.append(ref) or "the estimate")
    del calls[:]
    found = report.Outputs(foot_lock=True, upright=True, bvh="b").write("engine", "d/studio/chunk_0", (est, opt, None))
    assert found == "the estimate" and seen == ["the locked sequence"] and calls[0][2]["upright"] == "the estimate"


def test_the_pose_pickle_and_the_summary():
    from collections import OrderedDict
    from globalegomocap_amd import report as R
    est, opt, mid, locked = np.zeros((3, 15, 3)), np.ones((3, 15, 3)), np.full((3, 15, 3), 2.0), np.full((3, 15, 3), 3.0)
    assert list(R.result_pose_dict(est, opt, mid, None, True)) == ["estimated_pose", "optimized_pose", "mid_optimized_pose"]
    d = R.result_pose_dict(est, opt, mid, None, True, locked=locked)
    assert list(d)[-1] == "foot_locked_pose" and isinstance(d["foot_locked_pose"], np.ndarray) and np.array_equal(d["foot_locked_pose"], locked)
    d = R.result_pose_dict(est, opt, mid, est, False, locked=locked)
    assert isinstance(d["foot_locked_pose"], list) and len(d["foot_locked_pose"]) == 3 and np.array_equal(d["optimized_pose"], opt)
    reports = []
    for k in range(2):
        res = OrderedDict(zip(R.QUALITY_KEYS, (np.arange(7.0) + k).tolist()))
        res["foot_lock"] = {"status": "ok", "unreachable": k}
        res["ground"] = {"source": "plane"}
        reports.append(R.ChunkReport(result=res, est=est, opt=opt, gt=None, mid=None, raw=np.arange(7.0) + k, views=None))
    summary, results, *_ = R.sequence_result(reports, None, False)
    assert list(summary) == list(R.QUALITY_KEYS) and [r["foot_lock"]["unreachable"] for r in results] == [0, 1]


def test_the_parser_flags_are_present():
    from globalegomocap_amd import foot_lock, whole_sequence as ws
    a = ws._parser().parse_args(["--data_path", "d"])
    assert a.foot_lock is False and a.foot_lock_stretch is None and a.foot_lock_blend is None
    a = ws._parser().parse_args(["--data_path", "d", "--foot_lock", "true", "--foot_lock_stretch", "0.1", "--foot_lock_blend", "5"])
    assert a.foot_lock is True and a.foot_lock_stretch == 0.1 and a.foot_lock_blend == 5
    a = foot_lock._parser().parse_args(["r.pkl", "--out", "o.pkl"])
    assert (a.sequence, a.fps, a.lag, a.tau_v, a.tau_h, a.min_run, a.blend, a.stretch, a.no_snap, a.json) == \
        ("optimized", 25.0, None, 0.10, 0.05, 3, None, 0.05, False, None)
    a = foot_lock._parser().parse_args(["r.pkl", "--out", "o.pkl", "--sequence", "both", "--fps", "50", "--lag", "7", "--tau_v", "0.2", "--tau_h", "0.03",
                                        "--min_run", "4", "--blend", "6", "--stretch", "0.1", "--no_snap", "--json", "o.json"])
    assert (a.sequence, a.fps, a.lag, a.tau_v, a.tau_h, a.min_run, a.blend, a.stretch, a.no_snap, a.json) == \
        ("both", 50.0, 7, 0.2, 0.03, 4, 6, 0.1, True, "o.json")
    with pytest.raises(SystemExit):
        foot_lock._parser().parse_args(["r.pkl"])
    for mod in ("bvh", "meshes", "render"):
        src = open(os.path.join(ROOT, "globalegomocap_amd", mod + ".py")).read()
        assert 'p.add_argument("--foot_lock", action="store_true"' in src, mod


def test_record_layout_and_declarations():
    from globalegomocap_amd import _capi
    assert ctypes.sizeof(_capi.GemFootLockRecord) == 8 * _capi.FOOT_LOCK_RECORD_DOUBLES == 192
    names = [f[0] for f in _capi.GemFootLockRecord._fields_]
    assert names[:16] == ["status", "runs_right", "runs_left", "pinned_right", "pinned_left", "changed", "lengthened", "unreachable", "delta_max",
                          "delta_mean", "knee_max", "stretch_max", "slide_before", "slide_after", "slide_pairs", "frames"]
    assert _capi.GemFootLockRecord.frames.offset == 15 * 8 and _capi.GemFootLockRecord.slide_before.offset == 12 * 8
    assert set(T.COUNTS) | set(T.FLOATS) | {"status"} == set(names[:16])
    header = open(os.path.join(ROOT, "include", "gem_hip.h")).read()
    for name, value in (("GEM_FOOT_LOCK_RECORD_DOUBLES", _capi.FOOT_LOCK_RECORD_DOUBLES), ("GEM_FOOT_LOCK_NO_CONTACT", _capi.FOOT_LOCK_NO_CONTACT),
                        ("GEM_FOOT_LOCK_BAD_GROUND", _capi.FOOT_LOCK_BAD_GROUND), ("GEM_FOOT_LOCK_BAD_SEQUENCE", _capi.FOOT_LOCK_BAD_SEQUENCE)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert (T.NO_CONTACT, T.BAD_GROUND) == (_capi.FOOT_LOCK_NO_CONTACT, _capi.FOOT_LOCK_BAD_GROUND)
    struct = re.search(r"typedef struct gem_foot_lock_record \{(.*?)\} gem_foot_lock_record;", header, re.S).group(1)
    declared = re.findall(r"\b([a-z_]+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    assert declared == names
    for name, n_args in (("gem_foot_lock_work", 3), ("gem_foot_lock", 15)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == n_args == len(_capi.SIGNATURES[name][1]), name


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import _capi
    return _capi.load_library()


def test_the_work_helper_and_every_refusal_of_the_host_entry_point(lib):
    P = ctypes.c_void_p
    frames = np.array([98, 1024, 1025, 0, 3], dtype=np.int64)
    offsets = np.zeros(5, dtype=np.int64)
    need = lib.gem_foot_lock_work(P(frames.ctypes.data), 5, P(offsets.ctypes.data))

    def part(F):          # the run table (anchors and bounds of at most (F + 1) / 2 runs per foot), the prefix counts, the flags; the foot points beyond LDS
        runs = (F + 1) // 2
        return (6 * F if F > 1024 else 0) + 6 * runs + 2 * runs + F + (2 * F + 7) // 8
    assert offsets.tolist() == [0, part(98), part(98) + part(1024), -1, part(98) + part(1024) + part(1025)]
    assert need == 8 * (offsets[4] + part(3)) and part(1025) - part(1024) > 6 * 1024
    assert lib.gem_foot_lock_work(None, 5, None) == -1 and b"gem_foot_lock_work" in lib.gem_last_error()
    assert lib.gem_foot_lock_work(P(frames.ctypes.data), 0, None) == -1

    fake = 1 << 20          # device addresses are never read by the host checks: no launch happens behind a refusal
    base = dict(n=2, ground=fake, lag=5, tau_v=0.1, tau_h=0.05, min_run=3, blend=3, snap=1, stretch=0.05, work=fake, records=fake, d_table=fake)

    def call(table=None, work_bytes=None, **k):
        a = dict(base, **k)
        fr = np.array([98, 40], dtype=np.int64)
        off = np.zeros(2, dtype=np.int64)
        bytes_ = lib.gem_foot_lock_work(P(fr.ctypes.data), 2, P(off.ctypes.data))
        t = np.concatenate([[fake * 2, fake * 3], fr, [fake * 4, fake * 5], off]).astype(np.int64) if table is None else np.asarray(table, dtype=np.int64)
        a.setdefault("h_table", t.ctypes.data)
        rc = lib.gem_foot_lock(P(a["h_table"]), P(a["d_table"]), a["n"], P(a["ground"]), a["lag"], a["tau_v"], a["tau_h"], a["min_run"], a["blend"],
                               a["snap"], a["stretch"], P(a["work"]), bytes_ if work_bytes is None else work_bytes, P(a["records"]), None)
        return rc, lib.gem_last_error().decode()

    good = np.concatenate([[fake * 2, fake * 3], [98, 40], [fake * 4, fake * 5], [0, part(98)]])
    refusals = [(dict(n=0), "n_sequences"), (dict(n=(1 << 20) + 1), "n_sequences"), (dict(lag=0), "lag"), (dict(tau_v=0.0), "tau_v"),
                (dict(tau_v=float("inf")), "tau_v"), (dict(tau_h=-1.0), "tau_h"), (dict(tau_h=float("nan")), "tau_h"), (dict(min_run=0), "min_run"),
                (dict(blend=0), "blend"), (dict(stretch=-0.01), "stretch"), (dict(stretch=float("nan")), "stretch"), (dict(h_table=None), "h_table"),
                (dict(d_table=None), "d_table"), (dict(ground=None), "d_ground_records"), (dict(records=None), "d_records"),
                (dict(records=fake + 4), "8-byte aligned"), (dict(ground=fake + 2), "8-byte aligned"), (dict(work=fake + 1), "8-byte aligned"),
                (dict(d_table=fake + 4), "8-byte aligned"), (dict(work=None), "d_work holds 0 bytes"), (dict(work_bytes=8), "d_work holds 8 bytes")]
    for k, word in refusals:
        rc, msg = call(**k)
        assert rc == 1 and msg.startswith("gem_foot_lock: ") and word in msg, (k, msg)
    for change, word in (((7, 1), "sequence 1: its work offset"), ((6, -1), "sequence 0: its work offset"), ((4, fake * 2), "sequence 0: the output overlaps the input"),
                         ((5, fake * 3 + 8 * 45 * 39), "sequence 1: the output overlaps the input"), ((0, fake * 2 + 4), "sequence 0: its addresses"),
                         ((5, fake * 5 + 2), "sequence 1: its addresses")):
        t = good.copy()
        t[change[0]] = change[1]
        rc, msg = call(table=t)
        assert rc == 1 and word in msg, (change, msg)
