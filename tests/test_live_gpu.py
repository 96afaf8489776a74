"""Live mode on the device: a 37-frame stream -- four windows, a first, two inner and a last one, and three
left-over frames -- pushed in uneven pieces, against `optimize_windows` called directly on every window and `sequence.merge_batches`;
with graphs, with the running bone length, from raw inputs, with the One-Euro filter, and the failure paths."""
import numpy as np
import pytest

import live_twin as LT
from helpers import TINY
from globalegomocap_amd import synth, vae as vae_schema
from globalegomocap_amd.camera import DEFAULT_CALIBRATION
from globalegomocap_amd.skeleton import KINEMATIC_PARENTS

pytestmark = pytest.mark.gpu

N, PIECES = 37, (1, 5, 8, 13, 10)          # a piece shorter than a stride, one spanning two windows, an exact stride
N_WINDOWS, N_OUT, DROPPED = 4, 34, 3
EURO = (1.7, 0.3, 1.0)
WEIGHTS = dict(vae_weight=1e-3, smoothness_weight=1e-3, bone_length_weight=1e-2, weight_3d=1e-2, reproj_weight=1e-2)


@pytest.fixture(scope="module")
def S():
    """The stream, the weights, and the sessions' results shared by the tests (each computed once, never changed)."""
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from types import SimpleNamespace
    seq = synth.make_sequence(n_frames=N, seed=21, cam_jitter=(1.0, 0.005))
    rng = np.random.default_rng(5)
    s = SimpleNamespace(torch=torch, cache={})
    s.est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    s.cams = np.asarray(seq["camera_pose_list"], dtype=np.float64)
    s.heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    s.times = np.arange(N) / 25.0 + rng.uniform(-0.004, 0.004, N)          # irregular, like a trajectory's time column
    s.sd_l, s.sd_g = vae_schema.synthetic_state_dict(TINY, 11), vae_schema.synthetic_state_dict(TINY, 12)
    s.eps = rng.normal(size=(N_WINDOWS, 2, TINY.latent_dim)).astype(np.float32)
    s.bone = np.linalg.norm(s.est - s.est[:, list(KINEMATIC_PARENTS)], axis=-1).mean(0).astype(np.float32)          # a fixed, calibrated value
    return s


def _session(S, **kw):
    from globalegomocap_amd.live import LiveOptimizer
    kw.setdefault("eps", lambda w: S.eps[w])
    kw.setdefault("weights", WEIGHTS)
    return LiveOptimizer(DEFAULT_CALIBRATION, S.sd_g, S.sd_l, **kw)


def _run(S, live, pieces=PIECES, **inputs):
    """Pushes the stream in `pieces`; -> (result dict incl. "dropped", window_log, graph stats), checking the per-push returns."""
    inputs = inputs or dict(heat=S.heat, est_local=S.est, cams=S.cams, times=S.times)
    at, emitted = 0, 0
    for k in pieces:
        got = live.push(**{name: x[at:at + k] for name, x in inputs.items()})
        at += k
        done = LT.n_windows(at) - emitted // 8
        assert got["frames"] == emitted and got["optimized"].shape == (8 * done, 15, 3) == got["estimated"].shape
        assert got["optimized"].dtype == np.float64
        emitted += 8 * done
    tail = live.flush()
    assert tail["frames"] == emitted and tail["optimized"].shape == (2, 15, 3) and tail["dropped"] == LT.dropped(at)
    res = dict(live.result(), dropped=tail["dropped"])
    log, gs = list(live.window_log), live.graph_stats()
    again = live.flush()
    assert again["optimized"].shape == (0, 15, 3) and again["dropped"] == tail["dropped"]
    live.close()
    return res, log, gs


def _direct(S, bones):
    """`optimize_windows` called directly with B = 1 on every window (bones[w]: the mean bone lengths it is given), merged with
    `sequence.merge_batches` -> ([34,15,3] f64, the windows' stats)."""
    import torch
    from globalegomocap_amd.engine import WindowEngine, stats_to_numpy
    from globalegomocap_amd.camera import FisheyeCamera
    from globalegomocap_amd.optimizer import SequenceOptimizer
    from globalegomocap_amd.sequence import merge_batches
    eng = WindowEngine(TINY, FisheyeCamera.from_json(DEFAULT_CALIBRATION), max_windows=1)
    eng.load_vae(0, S.sd_l)
    eng.load_vae(1, S.sd_g)
    w_local, w_global = SequenceOptimizer.stage_weights(None, **WEIGHTS)
    dev, wins, stats = eng.device, [], []
    f0 = torch.zeros(1, dtype=torch.int32, device=dev)
    for w in range(N_WINDOWS):
        sl = slice(8 * w, 8 * w + 10)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt).contiguous()          # noqa: E731
        _, glob, st = eng.optimize_windows(t(S.est[sl], torch.float32), t(S.cams[sl], torch.float64), t(S.heat[sl], torch.float32), f0,
                                           t(np.asarray(bones[w]).reshape(1, 15), torch.float32), t(S.eps[w, 0:1], torch.float32),
                                           t(S.eps[w, 1:2], torch.float32), w_local, w_global)
        wins.append(glob.cpu().numpy()[0])
        stats.append(stats_to_numpy(st))
    eng.close()
    return np.asarray(merge_batches(np.stack(wins), 2)), stats


def _plain(S):
    """Test 1's session (filter off, fixed bone, graphs off) and the direct calls, shared."""
    if "plain" not in S.cache:
        S.cache["plain"] = _run(S, _session(S, bone=S.bone, graphs=False))
        S.cache["direct"] = _direct(S, [S.bone] * N_WINDOWS)
    return S.cache["plain"], S.cache["direct"]


def test_window_by_window_bitwise(S):
    (res, log, _), (want, stats) = _plain(S)
    assert res["optimized"].shape == (N_OUT, 15, 3) and res["dropped"] == DROPPED and len(log) == N_WINDOWS
    assert np.array_equal(res["optimized"], want)
    est = np.einsum("nij,nkj->nki", S.cams[:N_OUT, :3, :3], S.est[:N_OUT].astype(np.float64)) + S.cams[:N_OUT, None, :3, 3]
    np.testing.assert_allclose(res["estimated"], est, rtol=1e-12, atol=1e-12)
    for w, row in enumerate(log):
        assert row["window"] == w and np.array_equal(row["mean_bone"], S.bone) and row["step_ms"] > 0
        for k, stage in enumerate(("local", "global")):
            assert row[stage]["finished"] and all(row[stage][f] == stats[w][k][f] for f in ("n_iter", "func_evals", "status"))
    # (the windows did move their poses: the comparison above is not one of untouched inputs)
    assert np.abs(res["optimized"] - res["estimated"]).max() > 1e-3


def test_graphs_replay_every_window_after_the_capture(S):
    (res, _, _), _ = _plain(S)
    got, log, gs = _run(S, _session(S, bone=S.bone, graphs=True))
    assert np.array_equal(got["optimized"], res["optimized"]) and np.array_equal(got["estimated"], res["estimated"])
    # the first window runs eagerly, the second is captured and launched, every later one is a launch of that graph
    assert gs["captures"] == 1 and gs["replays"] == N_WINDOWS - 1, gs


def test_running_bone_length(S):
    import torch
    from globalegomocap_amd import prepare
    res, log, _ = _run(S, _session(S, bone="running", graphs=False))
    eng = prepare._lift_engine(DEFAULT_CALIBRATION, 0)
    for w, row in enumerate(log):
        want = eng.mean_bone_length(S.est[:8 * w + 10]).cpu().numpy()
        print("window", w, "running mean bone", row["mean_bone"], "mean_bone_length", want)
        np.testing.assert_allclose(row["mean_bone"], want, rtol=1e-6, atol=0)
    assert not np.array_equal(log[0]["mean_bone"], log[-1]["mean_bone"])
    want, _ = _direct(S, [row["mean_bone"] for row in log])
    assert np.array_equal(res["optimized"], want)
    torch.cuda.synchronize()


def test_from_raw_inputs(S):
    from globalegomocap_amd import prepare, slam, synth_recording as SR
    rows = SR.random_parameters(N, seed=5)["rows"]
    depth = np.linalg.norm(S.est.astype(np.float64), axis=-1)
    eng = prepare._lift_engine(DEFAULT_CALIBRATION, 0)
    lifted = eng.lift_skeleton(S.heat, depth)[1].cpu().numpy()
    assert lifted.dtype == np.float32 and np.isfinite(lifted).all() and np.abs(lifted).max() > 0.1
    cams = slam.scaled_trajectory(rows[:, 1:4], rows[:, 4:8], 1.7)
    raw, _, _ = _run(S, _session(S, bone="running", graphs=False, scale=1.7), heat=S.heat, depth=depth, rows=rows)
    ready, _, _ = _run(S, _session(S, bone="running", graphs=False), pieces=(N,), heat=S.heat, est_local=lifted, cams=cams, times=rows[:, 0].copy())
    assert raw["optimized"].shape == (N_OUT, 15, 3)
    assert np.array_equal(raw["optimized"], ready["optimized"]) and np.array_equal(raw["estimated"], ready["estimated"])


@pytest.mark.parametrize("n_chunks", [1, 2])
def test_one_euro_kernel_against_the_reference(S, golden, n_chunks):
    from globalegomocap_amd import prepare
    g = golden("one_euro")
    eng = prepare._lift_engine(DEFAULT_CALIBRATION, 0)
    seq = g["signal"].reshape(40, 15, 3)
    for k, p in enumerate(g["params"]):
        got = eng.one_euro_filter(seq, g["times"], n_chunks, p)
        assert got.is_cuda and tuple(got.shape) == (40, 15, 3)
        got = got.cpu().numpy().reshape(40, 45)
        if n_chunks == 1:
            want = g["filtered_%d" % k]
        else:          # fresh state per chunk: the reference's class started again at frame 20 is the twin on the second half
            want = np.concatenate([g["filtered_%d" % k][:20], LT.one_euro(g["signal"][20:], g["times"][20:], p)])
        print("one-euro", tuple(p), n_chunks, "chunk(s): largest relative difference", np.abs(got / want - 1).max())
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def test_live_filter_carries_its_state(S):
    (plain, _, _), _ = _plain(S)
    got, _, _ = _run(S, _session(S, bone=S.bone, graphs=False, one_euro=EURO))
    want = LT.one_euro(plain["optimized"], S.times[:N_OUT], EURO)
    print("live filter: largest relative difference", np.abs(got["optimized"] / want - 1).max(), "filter moved the poses by up to",
          np.abs(want - plain["optimized"]).max())
    assert np.abs(want - plain["optimized"]).max() > 1e-4
    np.testing.assert_allclose(got["optimized"], want, rtol=1e-12, atol=0)
    assert np.array_equal(got["estimated"], plain["estimated"])             # the filter applies to the optimised sequence only


def test_failure_paths(S):
    from globalegomocap_amd import _capi
    # the degenerate test's decoder: it outputs exactly its final bias, every joint at (0, 0, 1) on the optical axis
    sd = dict(vae_schema.synthetic_state_dict(TINY, 11))
    for k in list(sd):
        if k.startswith(("decoder", "final_layer")) and k.endswith(".weight") and np.asarray(sd[k]).ndim == 3:
            sd[k] = np.zeros_like(sd[k])
    sd["final_layer.3.bias"] = np.tile(np.array([0.0, 0.0, 1.0], np.float32), 15)
    pose = synth.rest_skeleton()[None].repeat(10, 0).astype(np.float32)
    from globalegomocap_amd.live import LiveOptimizer
    live = LiveOptimizer(DEFAULT_CALIBRATION, sd, sd, graphs=False, bone="running", eps=lambda w: S.eps[w],
                         weights=dict(vae_weight=0.0, smoothness_weight=1e-3, bone_length_weight=1e-2, weight_3d=1e-2, reproj_weight=1e-2))
    frames = dict(heat=np.zeros((10, 64, 64, 15), np.float32), est_local=pose, cams=np.tile(np.eye(4), (10, 1, 1)), times=np.arange(10) / 25.0)
    got = live.push(**{k: v[:9] for k, v in frames.items()})
    assert got["optimized"].shape == (0, 15, 3)
    with pytest.raises(Exception, match="norm is zero"):
        live.push(**{k: v[9:] for k, v in frames.items()})
    assert live.window_log[0]["local"]["degenerate"]
    live.close()
    with pytest.raises(_capi.GemError):
        live.push(**{k: v[:1] + (1.0 if k == "times" else 0) for k, v in frames.items()})
    with pytest.raises(_capi.GemError):
        live.flush()
    # the library's own checks: a push that would overwrite frames a window still needs, a window that is not complete
    live = _session(S, bone=S.bone, graphs=False)
    e, t = live.engine, S.torch
    dev = e.device
    k8 = (t.zeros(8, 64, 64, 15, device=dev), t.zeros(8, 15, 3, device=dev), t.zeros(8, 4, 4, device=dev, dtype=t.float64),
          t.zeros(8, device=dev, dtype=t.float64))
    with pytest.raises(_capi.GemError, match="ring overrun"):
        e.live_push(live._bufs, 25, 0, *k8)
    with pytest.raises(_capi.GemError, match="frames per call"):
        e.live_push(live._bufs, 0, 0, t.zeros(9, 64, 64, 15, device=dev), t.zeros(9, 15, 3, device=dev), t.zeros(9, 4, 4, device=dev, dtype=t.float64),
                    t.zeros(9, device=dev, dtype=t.float64))
    with pytest.raises(_capi.GemError, match="have been pushed"):
        e.live_window(live._bufs, 0, 9, live._win_pose, live._win_cams, live._win_heat, live._mean_bone)
    with pytest.raises(_capi.GemError, match="ring overrun"):
        e.live_window(live._bufs, 0, 33, live._win_pose, live._win_cams, live._win_heat, live._mean_bone)
    live.close()
