"""Live mode on the host: the numpy twins against the reference's One-Euro filter (tests/golden/one_euro.npz)
and against `sequence.merge_batches`, `push`'s argument checks, the CLI parser, the bindings."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import live_twin as LT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_twin_filter_is_the_reference_class(golden):
    g = golden("one_euro")
    assert g["signal"].shape == (40, 45) and (np.diff(g["times"]) > 0).all() and len(g["params"]) == 3
    outs = []
    for k, p in enumerate(g["params"]):
        got = LT.one_euro(g["signal"], g["times"], p)
        np.testing.assert_allclose(got, g["filtered_%d" % k], rtol=1e-13, atol=0)
        outs.append(got)
    # the fixture tells the three parameter sets apart, and the filter from no filter
    for a in range(3):
        assert np.abs(outs[a] - g["signal"]).max() > 1e-2
        for b in range(a):
            assert np.abs(outs[a] - outs[b]).max() > 1e-3
    # fresh state per chunk: the second half filtered on its own
    two = LT.one_euro(g["signal"], g["times"], g["params"][1], n_chunks=2)
    assert np.array_equal(two[:20], outs[1][:20]) and np.array_equal(two[20], g["signal"][20])
    assert np.array_equal(two[20:], LT.one_euro(g["signal"][20:], g["times"][20:], g["params"][1]))


@pytest.mark.parametrize("n_windows", [1, 2, 5])
def test_twin_schedule_is_merge_batches(n_windows):
    from globalegomocap_amd.sequence import merge_batches
    rng = np.random.default_rng(n_windows)
    G = rng.normal(size=(n_windows, 10, 15, 3))
    want = np.asarray(merge_batches(G, 2))
    s = LT.EmitSchedule()
    for w in range(n_windows):
        out = s.window(G[w])
        assert out.shape == (8, 15, 3) and np.array_equal(out, want[8 * w:8 * w + 8])
    assert np.array_equal(s.flush(), want[8 * n_windows:])
    assert np.array_equal(LT.stream(G), want) and len(want) == 8 * n_windows + 2


@pytest.mark.parametrize("n_pushed,windows,dropped", [(10, 1, 0), (17, 1, 7), (18, 2, 0), (37, 4, 3), (9, 0, 9)])
def test_dropped_frames(n_pushed, windows, dropped):
    from globalegomocap_amd import live
    from globalegomocap_amd.sequence import window_starts
    assert LT.n_windows(n_pushed) == windows == len(window_starts(n_pushed))
    assert LT.dropped(n_pushed) == dropped == live.dropped_frames(n_pushed)
    # however the frames arrive, every piece is at most 8 frames and ends where a window completes at the latest
    for k in (1, 5, 8, 13, n_pushed):
        at = 0
        while at < n_pushed:
            step = min(k, n_pushed - at)
            pieces = live._pieces(at, step)
            assert pieces[0][0] == 0 and pieces[-1][1] == step and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
            for a, b in pieces:
                assert 1 <= b - a <= 8
                inside = [f for f in range(at + a, at + b - 1) if f >= 9 and (f - 9) % 8 == 0]
                assert not inside, (at, k, pieces)
            at += step


def _session():
    """A LiveOptimizer without a device behind it: push's checks come before anything touches one."""
    from globalegomocap_amd.live import LiveOptimizer
    s = object.__new__(LiveOptimizer)
    s.engine, s._flushed, s._last_time = SimpleNamespace(heat_size=(64, 64)), False, None
    return s


def _frames(k, t0=0.0):
    rng = np.random.default_rng(k)
    cams = np.tile(np.eye(4), (k, 1, 1))
    rows = np.concatenate([t0 + np.arange(k)[:, None] / 25.0, rng.normal(size=(k, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (k, 1))], 1)
    return dict(heat=np.zeros((k, 64, 64, 15), np.float32), depth=np.ones((k, 15)), est_local=rng.normal(size=(k, 15, 3)).astype(np.float32),
                rows=rows, cams=cams, times=rows[:, 0].copy())


def test_push_rejects_bad_arguments_before_touching_the_device():
    from globalegomocap_amd import live
    f = _frames(3)
    good = dict(heat=f["heat"], est_local=f["est_local"], cams=f["cams"], times=f["times"])
    k, t, _ = live.check_push(None, good["heat"], None, good["est_local"], None, good["cams"], good["times"])
    assert k == 3 and np.array_equal(t, f["times"])
    s = _session()
    bad = [
        dict(good, times=f["times"][::-1].copy()),                              # decreasing
        dict(good, times=np.array([0.0, 0.04, 0.04])),                          # not strictly increasing
        dict(good, times=np.array([0.0, np.nan, 0.08])),
        dict(good, depth=f["depth"]),                                           # depth and est_local together
        dict(heat=f["heat"], cams=f["cams"], times=f["times"]),                 # neither
        dict(good, rows=f["rows"]),                                             # rows and cams together
        dict(heat=f["heat"], est_local=f["est_local"]),                         # neither
        dict(heat=f["heat"], est_local=f["est_local"], cams=f["cams"]),         # cams without times
        dict(good, heat=f["heat"][:, :32]),                                     # wrong shapes
        dict(good, heat=f["heat"][0]),
        dict(good, heat=f["heat"][:0], est_local=f["est_local"][:0], cams=f["cams"][:0], times=f["times"][:0]),
        dict(good, est_local=f["est_local"][:2]),
        dict(good, cams=f["cams"][:, :3]),
        dict(good, times=f["times"][:2]),
        dict(heat=f["heat"], depth=f["depth"][:, :14], rows=f["rows"]),
        dict(heat=f["heat"], depth=f["depth"], rows=f["rows"][:, :7]),
        dict(est_local=f["est_local"], cams=f["cams"], times=f["times"]),       # no heat-maps
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            s.push(**kw)
    # the last timestamp of the pushes before counts
    s._last_time = 0.08
    with pytest.raises(ValueError, match="increase strictly"):
        s.push(**dict(good, times=f["times"] + 0.08))
    live.check_push(0.08, good["heat"], None, good["est_local"], None, good["cams"], f["times"] + 0.12)


def test_cli_parser_round_trips_its_options(tmp_path):
    from globalegomocap_amd import live
    bone = tmp_path / "bone.npy"
    np.save(bone, np.linspace(0.1, 0.4, 15).astype(np.float32))
    a = live._parser().parse_args(["--slam", "traj.txt", "--heatmaps", "H", "--depths", "D", "--scale", "1.7", "--start", "3", "--end", "40",
                                   "--fps", "30", "--pace", "realtime", "--one_euro", "1.7,0.3", "--bone", str(bone), "--save_pose", "out",
                                   "--vae", "0.1", "--smooth", "0.2", "--bone_length", "0.3", "--weight_3d", "0.4", "--reproj_weight", "0.5",
                                   "--global_vae", "g.pth", "--local_vae", "l.pth", "--seed", "7"])
    assert (a.slam, a.heatmaps, a.depths, a.scale, a.start, a.end, a.fps, a.pace) == ("traj.txt", "H", "D", 1.7, 3, 40, 30.0, "realtime")
    assert a.one_euro == (1.7, 0.3, 1.0) and a.save_pose == "out" and np.array_equal(a.bone, np.load(bone))
    assert (a.vae, a.smooth, a.bone_length, a.weight_3d, a.reproj_weight, a.global_vae, a.local_vae, a.seed) == (0.1, 0.2, 0.3, 0.4, 0.5, "g.pth", "l.pth", 7)
    d = live._parser().parse_args(["--slam", "t", "--heatmaps", "H", "--depths", "D", "--start", "0", "--end", "10"])
    assert d.pace == "max" and d.one_euro is None and d.bone == "running" and d.scale == 1.0 and d.fps == 25 and d.save_pose is None
    assert (d.vae, d.smooth, d.bone_length, d.weight_3d, d.reproj_weight) == tuple(live.DEFAULT_WEIGHTS[k] for k in (
        "vae_weight", "smoothness_weight", "bone_length_weight", "weight_3d", "reproj_weight"))
    assert live._parser().parse_args(["--slam", "t", "--heatmaps", "H", "--depths", "D", "--start", "0", "--end", "10", "--one_euro", "0.5,5,2"]).one_euro == (0.5, 5.0, 2.0)
    with pytest.raises(SystemExit):
        live._parser().parse_args(["--slam", "t", "--heatmaps", "H", "--depths", "D", "--start", "0", "--end", "10", "--pace", "slow"])
    assert "rig" in live._parser().format_help()


def test_default_weights_are_whole_sequences():
    import inspect
    from globalegomocap_amd import live, whole_sequence
    sig = inspect.signature(whole_sequence._settings).parameters
    assert {k: sig[k].default for k in live.DEFAULT_WEIGHTS} == live.DEFAULT_WEIGHTS


def test_every_live_symbol_of_the_header_is_bound():
    from globalegomocap_amd import _capi
    header = open(os.path.join(ROOT, "include", "gem_hip.h")).read()
    declared = set(re.findall(r"\b(gem_live_[a-z0-9_]+|gem_one_euro)\s*\(", header))
    assert declared == {"gem_live_push", "gem_live_window", "gem_live_emit", "gem_one_euro"}
    for name in declared:
        assert name in _capi.SIGNATURES, name
        n_args = len(re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header).group(1).split(","))
        assert len(_capi.SIGNATURES[name][1]) == n_args, name
    consts = dict(re.findall(r"#define (GEM_LIVE_[A-Z_]+) (\d+)", header))
    assert (int(consts["GEM_LIVE_WINDOW"]), int(consts["GEM_LIVE_STRIDE"]), int(consts["GEM_LIVE_RING"]), int(consts["GEM_LIVE_PUSH_MAX"]),
            int(consts["GEM_LIVE_STATE_DOUBLES"])) == (_capi.LIVE_WINDOW, _capi.LIVE_STRIDE, _capi.LIVE_RING, _capi.LIVE_PUSH_MAX, _capi.LIVE_STATE_DOUBLES)
    fields = re.search(r"typedef struct gem_live_buffers \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [k for k, _ in _capi.GemLiveBuffers._fields_]


def test_rows_become_the_cameras_of_scaled_trajectory_however_they_arrive():
    """The session's frame is the first frame's camera: rows pushed in pieces give, bit for bit, `slam.scaled_trajectory` of all rows."""
    from globalegomocap_amd import slam, synth_recording as S
    from globalegomocap_amd.live import LiveOptimizer
    rows = S.random_parameters(37, seed=5)["rows"]
    whole = slam.scaled_trajectory(rows[:, 1:4], rows[:, 4:8], 1.7)
    for pieces in ((1, 5, 8, 13, 10), (1,) * 37):
        s = object.__new__(LiveOptimizer)
        s._row0, s.scale, at, parts = None, 1.7, 0, []
        for k in pieces:
            parts.append(s._cameras(rows[at:at + k]))
            at += k
        assert np.array_equal(np.concatenate(parts), whole)
