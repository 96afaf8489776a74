"""Dense live mode on the device ("Dense live mode"): the 37-frame stream of test_live_gpu.py at strides 1, 3 and
8, pushed in uneven pieces, against `optimize_windows` called directly on every window and the numpy twins of live_dense_twin.py --
the `now` stream, the settled stream, the estimated frames, with graphs, over more than two laps of the rings, the flush, the
filter, the refusals -- and gem_merge_dense against the twin."""
import numpy as np
import pytest

import live_twin as LT
import live_dense_twin as DT
from helpers import TINY
from globalegomocap_amd import synth, vae as vae_schema
from globalegomocap_amd.camera import DEFAULT_CALIBRATION
from globalegomocap_amd.skeleton import KINEMATIC_PARENTS

pytestmark = pytest.mark.gpu

N, PIECES = 37, (1, 5, 8, 13, 10)          # test_live_gpu.py's stream and pieces: shorter than a stride, across windows, an exact stride
N_LONG = 70                                # more than two laps of the 32 frame slots and four of the 16 sum slots
EURO = (1.7, 0.3, 1.0)
WEIGHTS = dict(vae_weight=1e-3, smoothness_weight=1e-3, bone_length_weight=1e-2, weight_3d=1e-2, reproj_weight=1e-2)


@pytest.fixture(scope="module")
def S():
    """The streams, the weights, and the sessions' and direct calls' results shared by the tests (each computed once, never changed)."""
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from types import SimpleNamespace
    s = SimpleNamespace(torch=torch, cache={})
    rng = np.random.default_rng(5)
    for name, n, seed in (("short", N, 21), ("long", N_LONG, 22)):
        seq = synth.make_sequence(n_frames=n, seed=seed, cam_jitter=(1.0, 0.005))
        setattr(s, name, SimpleNamespace(
            n=n, est=np.asarray(seq["estimated_local_skeleton"], dtype=np.float32), cams=np.asarray(seq["camera_pose_list"], dtype=np.float64),
            heat=np.asarray(seq["heatmap_list"], dtype=np.float32), times=np.arange(n) / 25.0 + rng.uniform(-0.004, 0.004, n)))
    s.sd_l, s.sd_g = vae_schema.synthetic_state_dict(TINY, 11), vae_schema.synthetic_state_dict(TINY, 12)
    s.eps = rng.normal(size=(DT.n_windows(N_LONG, 1), 2, TINY.latent_dim)).astype(np.float32)
    est = s.short.est
    s.bone = np.linalg.norm(est - est[:, list(KINEMATIC_PARENTS)], axis=-1).mean(0).astype(np.float32)          # a fixed, calibrated value
    return s


def _session(S, **kw):
    from globalegomocap_amd.live import LiveOptimizer
    kw.setdefault("eps", lambda w: S.eps[w])
    kw.setdefault("weights", WEIGHTS)
    return LiveOptimizer(DEFAULT_CALIBRATION, S.sd_g, S.sd_l, **kw)


def _pieces_of(n):
    at, i = 0, 0
    while at < n:
        step = min(PIECES[i % len(PIECES)], n - at)
        yield step
        at, i = at + step, i + 1


def _run(S, live, stream):
    """Pushes `stream` in pieces; -> (result dict incl. "dropped" and "tail", window_log, graph stats), checking every push's return."""
    k, dense = live.stride, live.dense
    at, windows, emitted, n_now = 0, 0, 0, 0
    frames = dict(heat=stream.heat, est_local=stream.est, cams=stream.cams, times=stream.times)
    for step in _pieces_of(stream.n):
        got = live.push(**{name: x[at:at + step] for name, x in frames.items()})
        at += step
        done = DT.n_windows(at, k) - windows
        assert got["frames"] == emitted and got["optimized"].shape == (k * done, 15, 3) == got["estimated"].shape
        assert got["optimized"].dtype == np.float64
        if dense:
            m = k * done + (10 - k if done and windows == 0 else 0)
            assert got["now_frames"] == n_now and got["now"].shape == (m, 15, 3) and got["now"].dtype == np.float64
            n_now += m
        else:
            assert "now" not in got
        windows, emitted = windows + done, emitted + k * done
    tail = live.flush()
    assert tail["frames"] == emitted and tail["optimized"].shape == (10 - k, 15, 3) == tail["estimated"].shape and tail["dropped"] == DT.dropped(at, k)
    if dense:
        assert tail["now"].shape == (0, 15, 3) and tail["now_frames"] == n_now == (windows - 1) * k + 10
    res = dict(live.result(), dropped=tail["dropped"], tail=tail["optimized"])
    log, gs = list(live.window_log), live.graph_stats()
    again = live.flush()
    assert again["optimized"].shape == (0, 15, 3) and again["dropped"] == tail["dropped"]
    from globalegomocap_amd import _capi
    with pytest.raises(_capi.GemError, match="flushed"):                  # a flushed session refuses push
        live.push(heat=stream.heat[:1], est_local=stream.est[:1], cams=stream.cams[:1], times=stream.times[-1:] + 1.0)
    live.close()
    return res, log, gs


def _direct(S, stream, k, bones):
    """`optimize_windows` called directly with B = 1 on every window [k w, k w + 10) of `stream` (bones[w]: the mean bone lengths it
    is given, S.eps[w] its noise) -> [n_windows,10,15,3] f64."""
    import torch
    from globalegomocap_amd.engine import WindowEngine
    from globalegomocap_amd.camera import FisheyeCamera
    from globalegomocap_amd.optimizer import SequenceOptimizer
    eng = WindowEngine(TINY, FisheyeCamera.from_json(DEFAULT_CALIBRATION), max_windows=1)
    eng.load_vae(0, S.sd_l)
    eng.load_vae(1, S.sd_g)
    w_local, w_global = SequenceOptimizer.stage_weights(None, **WEIGHTS)
    dev, wins = eng.device, []
    f0 = torch.zeros(1, dtype=torch.int32, device=dev)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt).contiguous()          # noqa: E731
    for w in range(DT.n_windows(stream.n, k)):
        sl = slice(k * w, k * w + 10)
        _, glob, _ = eng.optimize_windows(t(stream.est[sl], torch.float32), t(stream.cams[sl], torch.float64), t(stream.heat[sl], torch.float32), f0,
                                          t(np.asarray(bones[w]).reshape(1, 15), torch.float32), t(S.eps[w, 0:1], torch.float32),
                                          t(S.eps[w, 1:2], torch.float32), w_local, w_global)
        wins.append(glob.cpu().numpy()[0])
    eng.close()
    return np.stack(wins)


def _plain(S, k):
    """The dense session at stride k with the running bone length, filter and graphs off, and the direct calls given its logged bone
    lengths: shared."""
    if ("plain", k) not in S.cache:
        S.cache["plain", k] = run = _run(S, _session(S, bone="running", graphs=False, stride=k, now=True), S.short)
        S.cache["direct", k] = _direct(S, S.short, k, [row["mean_bone"] for row in run[1]])
    return S.cache["plain", k], S.cache["direct", k]


@pytest.mark.parametrize("stride", [1, 2, 3, 4, 5, 8, 10])
def test_merge_dense_kernel_is_the_twin(S, stride):
    from globalegomocap_amd import prepare
    from globalegomocap_amd.sequence import merge_dense
    eng = prepare._lift_engine(DEFAULT_CALIBRATION, 0)
    assert eng.T == 10
    G = np.random.default_rng(stride).normal(size=(24, 10, 15, 3))
    G[0, 0, 0, 0] = -0.0
    for wpc in (1, 2, 12):
        one = eng.merge_dense(G[:wpc], 1, stride)
        two = eng.merge_dense(G[:2 * wpc], 2, stride)
        assert one.is_cuda and one.dtype == S.torch.float64 and tuple(one.shape) == (1, (wpc - 1) * stride + 10, 15, 3)
        assert tuple(two.shape) == (2,) + tuple(one.shape[1:])
        want = DT.merge_dense(G[:2 * wpc].reshape(-1, 10, 45), stride, 2).reshape(two.shape)
        one, two, again = one.cpu().numpy(), two.cpu().numpy(), eng.merge_dense(G[:2 * wpc], 2, stride).cpu().numpy()
        assert two.tobytes() == want.tobytes() == again.tobytes()          # the twin's bits, on every call
        assert one.tobytes() == want[:1].tobytes()                         # a chunk's rows do not depend on its neighbour
        assert eng.merge_dense(G[wpc:2 * wpc], 1, stride).cpu().numpy().tobytes() == want[1:].tobytes()
        assert two.tobytes() == merge_dense(G[:2 * wpc], stride, 2).tobytes()
    for bad in (0, 11):
        with pytest.raises(ValueError, match="stride"):
            eng.merge_dense(G, 2, bad)
    assert eng.lib.gem_merge_dense(G.ctypes.data, 1, 2, 10, 45, 11, G.ctypes.data, None) == 1          # refused on the host: nothing is launched
    assert b"stride" in eng.lib.gem_last_error()


@pytest.mark.parametrize("k", [1, 3, 8])
def test_dense_session_is_the_direct_calls(S, k):
    from globalegomocap_amd import prepare
    (res, log, _), direct = _plain(S, k)
    n_w = DT.n_windows(N, k)
    n_out = (n_w - 1) * k + 10
    assert len(log) == n_w == len(direct) and res["dropped"] == (N - 10) % k
    assert res["optimized"].shape == res["estimated"].shape == res["now"].shape == (n_out, 15, 3) and res["now_frames"] == 0
    settled, now = DT.stream(direct, k)
    # `now`: all 10 frames of window 0, then the last k frames of every window's direct call; every frame once
    assert res["now"].tobytes() == now.tobytes() == np.concatenate([direct[0]] + [g[10 - k:] for g in direct[1:]]).tobytes()
    # `optimized`: every frame the mean of the direct results of all windows that cover it, oldest first
    assert res["optimized"].tobytes() == settled.tobytes() == DT.merge_dense(direct, k)[0].tobytes()
    assert res["tail"].tobytes() == settled[n_w * k:].tobytes() and len(res["tail"]) == 10 - k
    assert res["estimated"].tobytes() == DT.estimated(S.short.cams[:n_out], S.short.est[:n_out]).tobytes()
    # the running bone length of window w covers the frames [0, k w + 10)
    eng = prepare._lift_engine(DEFAULT_CALIBRATION, 0)
    for w, row in enumerate(log):
        assert row["window"] == w and row["stride"] == k and row["step_ms"] > 0 and row["local"]["finished"] and row["global"]["finished"]
        np.testing.assert_allclose(row["mean_bone"], eng.mean_bone_length(S.short.est[:k * w + 10]).cpu().numpy(), rtol=1e-6, atol=0)
    assert not np.array_equal(log[0]["mean_bone"], log[-1]["mean_bone"])
    # (the windows did move their poses, and averaging moved them again: neither comparison is one of untouched inputs)
    assert np.abs(res["optimized"] - res["estimated"]).max() > 1e-3
    if k < 8:
        assert np.abs(res["optimized"] - res["now"]).max() > 1e-6


@pytest.mark.parametrize("k", [1, 3, 8])
def test_graphs_replay_every_dense_window_after_the_capture(S, k):
    # (a fixed bone length: the direct calls of the first test do not apply, the eager dense session is the yardstick)
    if ("fixed", k) not in S.cache:
        S.cache["fixed", k] = _run(S, _session(S, bone=S.bone, graphs=False, stride=k, now=True), S.short)
    res = S.cache["fixed", k][0]
    got, log, gs = _run(S, _session(S, bone=S.bone, graphs=True, stride=k, now=True), S.short)
    for key in ("optimized", "estimated", "now"):
        assert got[key].tobytes() == res[key].tobytes(), key
    assert gs["captures"] == 1 and gs["replays"] == len(log) - 1 == DT.n_windows(N, k) - 1, gs


def test_stride_8_with_now_is_the_default_session(S):
    if ("fixed", 8) not in S.cache:
        S.cache["fixed", 8] = _run(S, _session(S, bone=S.bone, graphs=False, stride=8, now=True), S.short)
    dense = S.cache["fixed", 8][0]
    live = _session(S, bone=S.bone, graphs=False)
    assert not live.dense and live.stride == 8
    default, log, _ = _run(S, live, S.short)
    assert default["optimized"].shape == (34, 15, 3) and "now" not in default and log[0]["stride"] == 8
    assert dense["optimized"].tobytes() == default["optimized"].tobytes() and dense["estimated"].tobytes() == default["estimated"].tobytes()
    assert dense["tail"].tobytes() == default["tail"].tobytes() and dense["dropped"] == default["dropped"] == 3


def test_more_than_two_laps_of_the_rings(S):
    got, log, gs = _run(S, _session(S, bone=S.bone, graphs=True, stride=1, now=True), S.long)
    n_w = N_LONG - 9
    direct = _direct(S, S.long, 1, [S.bone] * n_w)
    assert len(log) == n_w and gs["captures"] == 1 and gs["replays"] == n_w - 1
    settled, now = DT.stream(direct, 1)
    assert got["now"].shape == (N_LONG, 15, 3) and got["now"].tobytes() == now.tobytes()
    assert got["optimized"].tobytes() == settled.tobytes() and got["dropped"] == 0
    assert got["estimated"].tobytes() == DT.estimated(S.long.cams, S.long.est).tobytes()


@pytest.mark.parametrize("k,dropped", [(1, 0), (3, 0), (8, 3)])
def test_flush_emits_the_held_frames(S, k, dropped):
    (res, _, _), direct = _plain(S, k)
    n_w = DT.n_windows(N, k)
    s = DT.DenseSchedule(k)
    for G in direct:
        s.window(G)
    tail = s.flush()
    assert tail.shape == (10 - k, 15, 3) and res["tail"].tobytes() == tail.tobytes() == res["optimized"][n_w * k:].tobytes()
    assert res["dropped"] == dropped == DT.dropped(N, k) and len(res["optimized"]) + dropped == N


@pytest.mark.parametrize("k", [1, 3])
def test_filter_runs_over_now_and_leaves_optimized_alone(S, k):
    (plain, plain_log, _), _ = _plain(S, k)
    got, log, _ = _run(S, _session(S, bone="running", graphs=False, stride=k, now=True, one_euro=EURO), S.short)
    assert all(np.array_equal(a["mean_bone"], b["mean_bone"]) for a, b in zip(log, plain_log))
    want = LT.one_euro(plain["now"], S.short.times[:len(plain["now"])], EURO)
    print("dense filter, stride", k, ": largest relative difference", np.abs(got["now"] / want - 1).max(), "filter moved the poses by up to",
          np.abs(want - plain["now"]).max())
    assert np.abs(want - plain["now"]).max() > 1e-4
    np.testing.assert_allclose(got["now"], want, rtol=1e-12, atol=0)
    # the settled stream, its flushed tail included, and the estimated one are never filtered
    for key in ("optimized", "estimated", "tail"):
        assert got[key].tobytes() == plain[key].tobytes(), key


def test_refusals_are_host_side(S):
    from globalegomocap_amd import _capi
    live = _session(S, bone=S.bone, graphs=False, stride=1, now=True)
    e, t = live.engine, S.torch
    win = (live._win_pose, live._win_cams, live._win_heat, live._mean_bone)
    with pytest.raises(_capi.GemError, match="gem_live_window_at.*have been pushed"):
        e.live_window_at(live._bufs, 5, 14, *win)                          # frames 5 .. 14 with 14 pushed: incomplete
    with pytest.raises(_capi.GemError, match="gem_live_window_at.*ring overrun"):
        e.live_window_at(live._bufs, 5, 38, *win)                          # frame 5 went when frame 37 came
    with pytest.raises(_capi.GemError, match="first frame"):
        e.live_window_at(live._bufs, -1, 38, *win)
    glob = t.zeros(1, 10, 15, 3, device=e.device, dtype=t.float64)
    for bad in (0, 9):
        with pytest.raises(_capi.GemError, match="gem_live_emit_dense: the stride"):
            e.live_emit_dense(live._bufs, live._dense_state, bad, 0, live._out_dense, glob, live._win_pose, live._win_cams)
    with pytest.raises(_capi.GemError, match="null argument"):
        e.live_emit_dense(live._bufs, live._dense_state, 1, 0, live._out_dense)          # no window result and not final
    with pytest.raises(TypeError):
        e.live_emit_dense(live._bufs, None, 1, 0, live._out_dense, glob, live._win_pose, live._win_cams)
    t.cuda.synchronize()
    # nothing was launched: the state block is as it was zeroed, the window buffers and the output block untouched
    assert not live._dense_state.any() and not live._out_dense.any() and not live._win_pose.any() and not live._mean_bone.any()
    live.close()
    with pytest.raises(ValueError, match="stride"):
        _session(S, stride=0)
