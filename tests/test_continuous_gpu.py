"""A recording optimised as one motion on the device: gem_merge_cover against `sequence.merge_cover` and
against the merges it generalises, and `continuous.optimize_continuous` end to end -- without and with ground truth, from chunks and
from one span, with its output files."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from globalegomocap_amd import sequence as S
from globalegomocap_amd.camera import DEFAULT_CALIBRATION

pytestmark = pytest.mark.gpu

N = 27          # four windows at stride 8: [0, 8, 16] and the one anchored to the end, 17


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def engine():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import prepare
    return prepare._lift_engine(DEFAULT_CALIBRATION, 0)


def _windows(starts, J, seed):
    """Windows that agree about a frame to a few centimetres around a track at 1e3 m, with a -0.0 in a frame only one window covers
    and one in a frame several do."""
    rng = np.random.default_rng(seed)
    starts = np.asarray(starts)
    track = 1e3 + rng.normal(0.0, 1.0, (int(starts[-1]) + 10, J, 3))
    w = np.stack([track[a:a + 10] for a in starts]) + rng.normal(0.0, 0.02, (len(starts), 10, J, 3))
    w[0, 0, 0, 0] = -0.0
    w[-1, 9, J - 1, 2] = -0.0
    w[0, 9, 0, 1] = -0.0
    return w


def _raw_merge(engine, w, starts, n, smooth=True, count=True, spread=True):
    """gem_merge_cover as it is -> (status, merged, smoothed, count, spread); an output not asked for is passed as NULL."""
    import torch
    dev = engine.device
    w_d = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    s_d = torch.from_numpy(np.asarray(starts, dtype=np.int32)).to(dev)
    B, T, J = w.shape[:3]
    out = [torch.full((n, J, 3), 7.0, dtype=torch.float64, device=dev), torch.full((n, J, 3), 7.0, dtype=torch.float64, device=dev) if smooth else None,
           torch.full((n,), -7, dtype=torch.int32, device=dev) if count else None, torch.full((n,), 7.0, dtype=torch.float64, device=dev) if spread else None]
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)      # noqa: E731
    rc = engine.lib.gem_merge_cover(ptr(w_d), ptr(s_d), B, T, J, n, *[ptr(t) for t in out], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (rc,) + tuple(None if t is None else t.cpu().numpy() for t in out)


CASES = {"one window": [0], "[0, 1]": [0, 1], "[0, 8, 9]": [0, 8, 9], "stride 1, 12 windows": list(range(12)), "N = 300": S.cover_starts(300).tolist()}


@pytest.mark.parametrize("J", [15, 1, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_against_the_definition(engine, case, J, capsys):
    starts = CASES[case]
    if case == "N = 300":
        assert starts[-2:] == [288, 290] and len(starts) == 38
    w = _windows(starts, J, seed=len(starts) + J)
    want, want_count, want_spread = S.merge_cover(w, starts, want_spread=True)
    n = len(want)
    rc, merged, _, count, spread = _raw_merge(engine, w, starts, n)
    assert rc == 0
    assert np.array_equal(_bits(merged), _bits(want)) and count.dtype == np.int32 and np.array_equal(count, want_count)
    assert np.signbit(merged[0, 0, 0]) and merged[0, 0, 0] == 0 and np.signbit(merged[-1, J - 1, 2])
    if case == "stride 1, 12 windows":
        assert count.max() == 10
    with capsys.disabled():
        print("gem_merge_cover %s, J = %d: spread differs from numpy's by at most %.3g m (%s)" %
              (case, J, np.abs(spread - want_spread).max(), "the same bits" if np.array_equal(_bits(spread), _bits(want_spread)) else "not the same bits"))
    # (float64 subtractions, products and sums in the definition's order and a correctly rounded square root: the same bits, measured)
    assert np.array_equal(_bits(spread), _bits(want_spread)) and (spread[want_count == 1] == 0).all()
    assert (spread[want_count > 1] > 0).all()
    if J == 15:          # the engine's binding: the same bytes, tensors on the device
        import torch
        m, s, c, d = engine.merge_cover(torch.from_numpy(w).to(engine.device), np.asarray(starts), smooth=False, want_spread=True)
        assert s is None and m.is_cuda and c.dtype == torch.int32 and tuple(m.shape) == (n, 15, 3)
        assert np.array_equal(_bits(m.cpu().numpy()), _bits(merged)) and np.array_equal(_bits(d.cpu().numpy()), _bits(spread))
        assert engine.merge_cover(w, starts)[3] is None


def test_bits_of_the_merges_it_generalises(engine):
    import torch
    starts = S.window_starts(100)
    w = _windows(starts, 15, seed=3)
    w_d = torch.from_numpy(w).to(engine.device)
    for smooth in (False, True):
        m, s, _, _ = engine.merge_cover(w_d, starts, smooth=smooth)
        got = (s if smooth else m).cpu().numpy()
        want = engine.merge_windows(w_d, 1, overlap=2, smooth=smooth).cpu().numpy()
        assert got.shape == want.shape == (98, 15, 3) and np.array_equal(_bits(got), _bits(want)), smooth
    for stride in range(1, 9):
        starts = np.arange(12) * stride
        w = _windows(starts, 15, seed=20 + stride)
        w_d = torch.from_numpy(w).to(engine.device)
        got = engine.merge_cover(w_d, starts)[0].cpu().numpy()
        want = engine.merge_dense(w_d, 1, stride).cpu().numpy()[0]
        assert np.array_equal(_bits(got), _bits(want)), stride
    # a table that is on the device already (the caller vouches for it): the same bytes
    on_device = engine.merge_cover(w_d, torch.from_numpy(starts.astype(np.int32)).to(engine.device), want_spread=True)
    on_host = engine.merge_cover(w_d, starts, want_spread=True)
    assert all(torch.equal(a, b) for a, b in zip(on_device, on_host) if a is not None) and on_device[1] is None


def test_smoothing_at_irregular_starts(engine):
    starts = S.cover_starts(N)
    w = _windows(starts, 15, seed=9)
    rc, merged, smoothed, _, _ = _raw_merge(engine, w, starts, N)
    assert rc == 0
    taps = np.exp(-0.5 * np.arange(-4, 5) ** 2.0)
    taps /= taps.sum()
    padded = np.pad(merged, ((4, 4), (0, 0), (0, 0)), mode="symmetric")          # scipy's 'reflect': d c b a | a b c d | d c b a
    want = sum(taps[k] * padded[k:k + N] for k in range(9))
    assert np.abs(smoothed - want).max() <= 1e-9
    np.testing.assert_allclose(smoothed, S.final_smooth(merged), rtol=0, atol=1e-9)


def test_null_outputs_change_nothing(engine):
    starts = S.cover_starts(N, stride=3)
    w = _windows(starts, 15, seed=11)
    rc, merged, smoothed, count, spread = _raw_merge(engine, w, starts, N)
    assert rc == 0
    for kw in (dict(smooth=False), dict(count=False), dict(spread=False), dict(smooth=False, count=False, spread=False)):
        rc, m, s, c, d = _raw_merge(engine, w, starts, N, **kw)
        assert rc == 0 and np.array_equal(_bits(m), _bits(merged)), kw
        for got, want in ((s, smoothed), (d, spread)):
            assert got is None or np.array_equal(_bits(got), _bits(want)), kw
        assert c is None or np.array_equal(c, count), kw


def test_bad_arguments_launch_nothing(engine):
    import torch
    lib, dev = engine.lib, engine.device
    w = torch.zeros(2, 10, 15, 3, dtype=torch.float64, device=dev)
    s = torch.tensor([0, 8], dtype=torch.int32, device=dev)
    out = torch.full((18, 15, 3), 7.0, dtype=torch.float64, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(w=w, s=s, B=2, T=10, J=15, n=18, out=out)
    for change, word in ((dict(w=None), "null"), (dict(s=None), "null"), (dict(out=None), "null"), (dict(T=0), "T"), (dict(J=0), "n_joints"),
                         (dict(J=17), "n_joints"), (dict(B=-1), "negative"), (dict(n=-1), "negative"), (dict(n=1 << 34), "too many frames"),
                         (dict(B=1 << 40), "too many windows")):
        a = dict(good, **change)
        rc = lib.gem_merge_cover(P(a["w"]), P(a["s"]), a["B"], a["T"], a["J"], a["n"], P(a["out"]), None, None, None, stream)
        assert rc != 0 and word in lib.gem_last_error().decode(), change
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert lib.gem_merge_cover(P(w), P(s), 2, 10, 15, (1 << 30), P(out), P(out), None, None, stream) != 0 and "smooth" in lib.gem_last_error().decode()
    assert lib.gem_merge_cover(P(w), P(s), 2, 10, 15, 0, P(out), None, None, None, stream) == 0          # (no frames: nothing to do)
    with pytest.raises(ValueError):
        engine.merge_cover(w, [0, 11])
    with pytest.raises(ValueError):
        engine.merge_cover(w, [0, 8, 9])
    with pytest.raises(TypeError):
        engine.merge_cover(w, s.to(torch.int64))


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def world(engine, golden):
    """The 27 synthetic frames every end-to-end test uses, made once: poses, heat-maps, cameras relative to the first frame (the
    recording's frame), the ground truth in it; the `lbfgs_tiny` VAEs."""
    import torch
    from globalegomocap_amd import synth
    from helpers import sd_from_npz
    s = synth.make_sequence(n_frames=N, seed=60, cam_jitter=(1.0, 0.005))
    Cw = np.asarray(s["camera_pose_list"], dtype=np.float64)
    est = np.asarray(s["estimated_local_skeleton"], dtype=np.float64)
    first = np.linalg.inv(Cw[0])
    cams = first[None] @ Cw
    heat = torch.from_numpy(np.asarray(s["heatmap_list"], dtype=np.float32)).to("cuda:0")
    gt = np.asarray(s["gt_global_skeleton"], dtype=np.float64) @ first[:3, :3].T + first[:3, 3]
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False)
    return dict(est=est, cams=cams, heat=heat, gt=gt, absolute=Cw, kw=kw)


RESPONSE_TOL = dict(rtol=5e-5, atol=1e-7)          # the report without ground truth against its twin: the bounds of tests/test_no_gt_gpu.py
F64_RTOL = 1e-12
SEVEN = ["estimated_heatmap_response", "optimized_heatmap_response", "estimated_bone_length_rms", "optimized_bone_length_rms",
         "estimated_acceleration", "optimized_acceleration", "optimized_displacement"]


def _check_against_twin(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    for c, name in enumerate(("heatmap_response", "bone_length_rms", "acceleration", "displacement")):
        print("%s %s: device %s twin %s" % (what, name, got[..., c].tolist(), want[..., c].tolist()))
    np.testing.assert_allclose(got[..., 0], want[..., 0], **RESPONSE_TOL)
    np.testing.assert_allclose(got[..., 1:], want[..., 1:], rtol=F64_RTOL, atol=0, equal_nan=True)


def _to_global(local, cams):
    return np.einsum("nij,nkj->nki", cams[:, :3, :3], local) + cams[:, None, :3, 3]


def _one_span(world, gt=False):
    import torch
    from globalegomocap_amd import prepare as P
    dev = world["heat"].device
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    chunk = P.RecordingChunk(0, N, world["heat"], t(world["est"]), t(_to_global(world["est"], world["cams"])), t(world["cams"]),
                             t(world["gt"]) if gt else None)
    return P.Recording([chunk], None if gt else np.eye(4)[None])


def _optimizer(world, max_windows):
    from globalegomocap_amd.optimizer import SequenceOptimizer
    return SequenceOptimizer(DEFAULT_CALIBRATION, world["kw"]["global_vae_path"], world["kw"]["local_vae_path"], max_windows=max_windows)


@pytest.fixture(scope="module")
def no_gt_run(world):
    import torch
    from globalegomocap_amd import continuous
    torch.manual_seed(41)
    return continuous.optimize_continuous(_one_span(world), DEFAULT_CALIBRATION, ground_truth=False, final_smooth=False,
                                          optimizer=_optimizer(world, 8), **world["kw"])


def test_end_to_end_without_ground_truth(engine, world, no_gt_run, capsys):
    import torch
    from globalegomocap_amd import whole_sequence as ws
    from helpers import oracle_camera
    from quality_twin import sequence_quality
    summary, reports, est, opt, gt = no_gt_run
    assert gt is None and len(reports) == 1 and est.shape == opt.shape == (N, 15, 3) and np.isfinite(opt).all()
    assert np.array_equal(est, _to_global(world["est"], world["cams"]))
    # the chunked route leaves the last frame out: 27 = 8 * 3 + 2 + 1
    torch.manual_seed(41)
    chunked = ws.optimize_recording(_one_span(world), DEFAULT_CALIBRATION, ground_truth=False, final_smooth=False, optimizer=_optimizer(world, 8), **world["kw"])
    assert chunked[3].shape == (N - 1, 15, 3)
    # the optimiser's own call on the same windows after the same seed, merged by the definition
    starts = S.cover_starts(N)
    so = _optimizer(world, 8)
    torch.manual_seed(41)
    _, glob, _ = so.run(world["est"], world["cams"], world["heat"], starts, np.zeros(len(starts), dtype=np.int64), [(0, N)],
                        *so.stage_weights(0.0, 0.001, 0.01, 0.01, 0.01))
    want, count, spread = S.merge_cover(glob, starts, want_spread=True)
    assert np.array_equal(_bits(opt), _bits(want))
    r = reports[0]
    assert list(r)[:7] == SEVEN and list(r)[7:] == ["windows_per_frame", "window_disagreement"] and list(summary) == list(r)
    assert r["windows_per_frame"] == (int(count.min()), int(count.max())) == (1, 3)
    d = r["window_disagreement"]
    assert list(d) == ["mean", "max", "frame"] and d["max"] == spread.max() and d["frame"] == int(np.argmax(spread))
    assert abs(d["mean"] - spread.mean()) <= 1e-15 and d["max"] > 0
    # the seven entries are the twin's on the returned sequences
    mb = engine.mean_bone_length(world["est"].astype(np.float32)).cpu().numpy()[None]
    heat, cam, frame0 = world["heat"].cpu().numpy(), oracle_camera(), np.zeros(1, dtype=np.int64)
    q_est = sequence_quality(est, world["cams"], heat, frame0, mb, 1, cam)
    q_opt = sequence_quality(opt, world["cams"], heat, frame0, mb, 1, cam, ref=est)
    got_est = np.array([[r["estimated_heatmap_response"], r["estimated_bone_length_rms"], r["estimated_acceleration"], np.nan]])
    got_opt = np.array([[r["optimized_heatmap_response"], r["optimized_bone_length_rms"], r["optimized_acceleration"], r["optimized_displacement"]]])
    with capsys.disabled():
        _check_against_twin(got_est, q_est, "optimize_continuous, estimated")
        _check_against_twin(got_opt, q_opt, "optimize_continuous, optimised")


def test_the_split_into_calls_does_not_matter(world, no_gt_run):
    import torch
    from globalegomocap_amd import continuous, whole_sequence as ws
    torch.manual_seed(41)
    two = continuous.optimize_continuous(_one_span(world), DEFAULT_CALIBRATION, ground_truth=False, final_smooth=False,
                                         optimizer=_optimizer(world, 2), **world["kw"])
    assert np.array_equal(_bits(two[3]), _bits(no_gt_run[3])) and two[1][0] == no_gt_run[1][0]
    torch.manual_seed(41)
    via = ws.optimize_recording(_one_span(world), DEFAULT_CALIBRATION, ground_truth=False, final_smooth=False, optimizer=_optimizer(world, 8),
                                continuous=True, **world["kw"])
    assert np.array_equal(_bits(via[3]), _bits(no_gt_run[3]))
    for bad in (dict(chunks_per_batch=1), dict(per_sequence=True), dict(overlap=4), dict(device_metrics=False), dict(stride=9), dict(stride=0)):
        with pytest.raises(ValueError):
            continuous.optimize_continuous(_one_span(world), DEFAULT_CALIBRATION, ground_truth=False, **dict(world["kw"], **bad))
    with pytest.raises(KeyError, match="gt_global_skeleton"):
        continuous.optimize_continuous(_one_span(world), DEFAULT_CALIBRATION, **world["kw"])


def test_chunks_join_into_the_one_span_recording(world):
    """The same 27 frames as chunks of 10, 9 and 8 frames, each relative to its own first frame, with the origins that join them."""
    import torch
    from globalegomocap_amd import continuous, prepare as P
    dev, Cw, chunks, origins, a = world["heat"].device, world["absolute"], [], [], 0
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    for m in (10, 9, 8):
        cams = np.linalg.inv(Cw[a])[None] @ Cw[a:a + m]
        chunks.append(P.RecordingChunk(a, a + m, world["heat"][a:a + m], t(world["est"][a:a + m]), t(_to_global(world["est"][a:a + m], cams)), t(cams), None))
        origins.append(world["cams"][a])
        a += m
    rec = P.Recording(chunks, np.stack(origins))
    assert np.abs(np.stack(origins)[1:] - np.eye(4)).max() > 1e-3
    one = rec.continuous()
    c = one.chunks[0]
    assert len(one) == 1 and c.n == N and c.cams.is_cuda and c.cams.dtype == torch.float64 and c.name == "data_start_0_end_27"
    err = np.abs(c.cams.cpu().numpy() - world["cams"]).max()
    err_g = np.abs(c.est_global.cpu().numpy() - _to_global(world["est"], world["cams"])).max()
    print("continuous(): cameras differ from the one-span recording's by %.3g, global poses by %.3g" % (err, err_g))
    assert err <= 1e-12 and err_g <= 1e-12
    assert torch.equal(c.heat, world["heat"]) and torch.equal(c.est_local, t(world["est"]))
    torch.manual_seed(41)
    out = continuous.optimize_continuous(rec, DEFAULT_CALIBRATION, ground_truth=False, **world["kw"])
    assert out[3].shape == (N, 15, 3) and np.isfinite(out[2]).all() and np.isfinite(out[3]).all()
    assert all(np.isfinite(v) for k, v in out[1][0].items() if isinstance(v, float))


def test_end_to_end_with_ground_truth(world, tmp_path):
    import torch
    from globalegomocap_amd import continuous
    from globalegomocap_amd.errors import calculate_errors
    torch.manual_seed(43)
    summary, reports, est, opt, gt = continuous.optimize_continuous(_one_span(world, gt=True), DEFAULT_CALIBRATION, save_pose=str(tmp_path), **world["kw"])
    assert est.shape == opt.shape == gt.shape == (N, 15, 3) and np.array_equal(gt, world["gt"])
    with open(str(tmp_path / "data_start_0_end_27" / "result_pose.pkl"), "rb") as f:
        poses = pickle.load(f)
    assert list(poses) == ["estimated_pose", "optimized_pose", "mid_optimized_pose", "gt_pose", "window_disagreement"]
    assert np.array_equal(poses["optimized_pose"], opt) and isinstance(poses["optimized_pose"], np.ndarray)          # (smoothed: an array)
    mid = np.asarray(poses["mid_optimized_pose"])
    assert mid.shape == (N, 15, 3) and np.isfinite(mid).all()
    want = calculate_errors(est, mid, opt, gt)
    r = reports[0]
    assert set(r) == set(want) | {"windows_per_frame", "window_disagreement"} and len(want) == 18
    for k in want:
        np.testing.assert_allclose(r[k], want[k], rtol=1e-9, atol=1e-12, err_msg=k)
        np.testing.assert_allclose(summary[k], want[k], rtol=1e-9, atol=1e-12, err_msg=k)


def test_one_set_of_files(world, tmp_path):
    import torch
    from globalegomocap_amd import bvh, continuous, gltf
    torch.manual_seed(47)
    out = continuous.optimize_continuous(_one_span(world), DEFAULT_CALIBRATION, ground_truth=False, bvh=str(tmp_path / "b"), gltf=str(tmp_path / "g"),
                                         save_pose=str(tmp_path / "p"), upright=True, foot_lock=True, **world["kw"])
    found = sorted(os.path.relpath(os.path.join(d, f), str(tmp_path)) for d, _, files in os.walk(str(tmp_path)) for f in files)
    name = "data_start_0_end_27"
    assert found == sorted([os.path.join("b", "recording_0", name, "estimated.bvh"), os.path.join("b", "recording_0", name, "optimized.bvh"),
                            os.path.join("g", "recording_0", name, "result.glb"), os.path.join("p", name, "result_pose.pkl")])
    assert bvh.read_bvh(str(tmp_path / "b" / "recording_0" / name / "optimized.bvh")).motion.shape[0] == N
    glb = gltf.read_glb(str(tmp_path / "g" / "recording_0" / name / "result.glb"))
    assert glb.accessors[glb.json["animations"][0]["samplers"][0]["input"]].shape[0] == N
    with open(str(tmp_path / "p" / name / "result_pose.pkl"), "rb") as f:
        poses = pickle.load(f)
    assert list(poses) == ["estimated_pose", "optimized_pose", "mid_optimized_pose", "foot_locked_pose", "window_disagreement"]
    assert poses["window_disagreement"].shape == (N,) and len(poses["estimated_pose"]) == N and np.asarray(poses["foot_locked_pose"]).shape == (N, 15, 3)
    assert np.array_equal(poses["optimized_pose"], out[3])
    r = out[1][0]
    assert isinstance(r["ground"], dict) and isinstance(r["foot_lock"], dict) and poses["window_disagreement"].max() == r["window_disagreement"]["max"]


def test_command_line_prepares_one_span_and_optimises_it(world, tmp_path, monkeypatch, capsys):
    """The command line on files: `prepare`'s route with a scale and with a ground truth, `detections`' route; the optimiser's call is
    given the test's small VAEs (the command line's own are the reference's checkpoint files)."""
    from globalegomocap_amd import continuous, synth_recording as R
    n = 29
    par = R.random_parameters(n, seed=23)
    heat64 = R.paraboloid_heatmaps(par["centres"], par["radii"])
    hd, dd, traj, gtp = R.write_recording(str(tmp_path / "rec"), heat64, par["depth"], ["f_%d.mat" % k for k in range(n)], np.arange(n) % 7 == 3,
                                          np.arange(n) % 5 == 1, par["rows"], par["gt"])
    real, calls = continuous.optimize_continuous, []

    def with_small_vaes(rec, camera, *args, **kwargs):
        calls.append((rec, args, kwargs))
        return real(rec, camera, *args, **dict(kwargs, **world["kw"]))
    monkeypatch.setattr(continuous, "optimize_continuous", with_small_vaes)
    base = ["--slam", traj, "--start", "0", "--end", str(n), "--fps", "25"]
    continuous._cli(base + ["--heatmaps", hd, "--depths", dd, "--scale", "1.7", "--stride", "4", "--bvh", str(tmp_path / "b"), "--final_smooth", "false"])
    rec, args, kw = calls[-1]
    assert len(rec) == 1 and rec.chunks[0].n == n and rec.chunks[0].gt is None and rec.origins.shape == (1, 4, 4)
    assert kw["stride"] == 4 and kw["ground_truth"] is False and kw["final_smooth"] is False and args == (0.0, 0.0, 0.001, 0.01, 0.01, 0.01)
    from globalegomocap_amd import bvh
    assert bvh.read_bvh(str(tmp_path / "b" / "recording_0" / ("data_start_0_end_%d" % n) / "optimized.bvh")).motion.shape[0] == n
    continuous._cli(base + ["--heatmaps", hd, "--depths", dd, "--gt", gtp, "--save_pose", str(tmp_path / "p")])
    rec, args, kw = calls[-1]
    assert len(rec) == 1 and rec.chunks[0].gt is not None and tuple(rec.chunks[0].gt.shape) == (n, 15, 3) and kw["ground_truth"] is True
    assert "The initial mpjpe is" in capsys.readouterr().out
    with open(str(tmp_path / "p" / ("data_start_0_end_%d" % n) / "result_pose.pkl"), "rb") as f:
        assert len(pickle.load(f)["gt_pose"]) == n
    rng = np.random.default_rng(2)
    kp = np.concatenate([rng.uniform(350.0, 900.0, (n, 15, 2)), np.ones((n, 15, 1))], axis=2)
    np.save(str(tmp_path / "kp.npy"), kp)
    np.save(str(tmp_path / "depth.npy"), rng.uniform(0.5, 1.5, (n, 15)))
    continuous._cli(base + ["--keypoints", str(tmp_path / "kp.npy"), "--depth", str(tmp_path / "depth.npy"), "--scale", "1.7"])
    rec, args, kw = calls[-1]
    assert len(rec) == 1 and rec.chunks[0].n == n and tuple(rec.chunks[0].heat.shape) == (n, 64, 64, 15) and kw["stride"] == 8
