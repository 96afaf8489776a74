"""Depths from bone lengths on the device: gem_bone_depths against its numpy twin (tests/bone_depth_twin.py),
its determinism and batch independence, its guards, and both routes end to end -- `recording_from_detections(depth="bones")` through
`optimize_recording`, and the live session's `bone_depths`.

THE GATE on `depth` and `rms`: 16 times the largest spread between the float64 twin and the same twin in np.longdouble over these very
cases (the margin covers a different but valid order of operations: the device fuses the multiply-adds of the ray, numpy does not).
Thirty Levenberg-Marquardt iterations with a prior of weight 1e-3 leave the weakly determined directions short of convergence, and
the accept / reject decision of a step can fall either way on a rounding error: the spread's median is 1e-14 m, its tail reaches
1e-9 m.  Frames whose twins differ by more than 1e-9 m are ill-conditioned and left out: 1 of the 331 here (the cap is 2 %;
tests/test_bone_depth_cpu.py checks it on the twin alone).  Measured: largest spread of the others 6.79e-10 m, so the gate is
1.09e-8 m.  It is computed below, not typed in."""
import ctypes as C

import numpy as np
import pytest

import bone_depth_twin as BT
from globalegomocap_amd.camera import DEFAULT_CALIBRATION, FisheyeCamera

pytestmark = pytest.mark.gpu

F64_RTOL = 1e-12          # tests/test_keypoints_gpu.py's, for the un-projection


@pytest.fixture(scope="module")
def E():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import prepare
    return prepare._lift_engine(DEFAULT_CALIBRATION, 0)


@pytest.fixture(scope="module")
def cam():
    return FisheyeCamera.from_json(DEFAULT_CALIBRATION)


@pytest.fixture(scope="module")
def opts():
    from globalegomocap_amd import bone_depth as B
    return B.options()


def _spread(kp, cam, opts):
    d, s, rms = BT.solve(kp, cam, opts)
    dl, _, rl = BT.solve(kp, cam, opts, np.longdouble)
    return d, s, rms, np.maximum(np.abs(d - dl).max(axis=1), np.abs(rms - rl)).astype(np.float64)


@pytest.fixture(scope="module")
def twin(cam, opts):
    """Per size: the cases, the float64 twin's result, and which frames are kept; the gate over all of them.  Computed once."""
    out, worst, left = {}, 0.0, 0
    for n in BT.CASE_SIZES:
        kp = BT.cases(n, cam)
        d, s, rms, spread = _spread(kp, cam, opts)
        keep = spread <= BT.ILL_CONDITIONED
        worst, left = max(worst, float(spread[keep].max())), left + int((~keep).sum())
        out[n] = dict(kp=kp, depth=d, solved=s, rms=rms, keep=keep)
    assert left <= 0.02 * sum(BT.CASE_SIZES)
    out["gate"] = 16.0 * worst
    return out


@pytest.mark.parametrize("n", BT.CASE_SIZES)
def test_device_against_the_twin(E, twin, opts, n, capsys):
    import torch
    t, gate = twin[n], twin["gate"]
    depth, solved, rms = E.bone_depths(t["kp"])
    assert depth.dtype == torch.float64 and solved.dtype == torch.uint8 and rms.dtype == torch.float64 and depth.is_cuda
    assert tuple(depth.shape) == (n, 15) and tuple(solved.shape) == (n, 15) and tuple(rms.shape) == (n,)
    depth, solved, rms = depth.cpu().numpy(), solved.cpu().numpy(), rms.cpu().numpy()
    keep = t["keep"]
    dd, dr = np.abs(depth - t["depth"]).max(axis=1), np.abs(rms - t["rms"])
    with capsys.disabled():
        print("%d frames (%d left out): depth differs from the twin by at most %.3g m, rms by %.3g m (gate %.3g m); %d of %d depths are the twin's bits"
              % (n, (~keep).sum(), dd[keep].max(), dr[keep].max(), gate, (depth == t["depth"]).sum(), depth.size))
    assert np.array_equal(solved, t["solved"])
    assert np.isfinite(depth).all() and (depth >= BT.FLOOR).all() and np.isfinite(rms).all() and (rms >= 0).all()
    assert dd[keep].max() <= gate and dr[keep].max() <= gate
    # unsolved joints: the prior depth's bits
    off = solved == 0
    assert np.array_equal(depth[off], np.broadcast_to(opts["dbar"], depth.shape)[off])
    if n > 7:
        assert not solved[2].any() and rms[2] == 0.0 and solved[1].sum() == 13 and solved[3].sum() == 9 and solved[7].sum() == 8
        assert rms[4] > 0.01 and rms[6] > 0.01 and np.median(rms) < 0.002          # the contradictions show, the rest does not


def test_same_bytes_twice_and_alone(E, twin):
    import torch
    kp = twin[67]["kp"]
    a, b = E.bone_depths(kp), E.bone_depths(kp)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    part = E.bone_depths(kp[10:20])
    assert all(torch.equal(x[10:20], y) for x, y in zip(a, part))
    one = E.bone_depths(kp[66:67])
    assert all(torch.equal(x[66:67], y) for x, y in zip(a, one))
    # two-column detections: confidence 1, and a usable confidence does not matter
    two = E.bone_depths(np.where(BT.usable(kp)[..., None], kp, 700.0)[..., :2])
    ok = BT.usable(kp).all(axis=1)
    assert torch.equal(two[0][torch.from_numpy(ok).to(E.device)], a[0][torch.from_numpy(ok).to(E.device)])


def test_positions_are_lift_keypoints(E, twin, cam):
    """depth x ray: `lift_keypoints` with the device's depths against the twin's rays times those depths."""
    t = twin[260]
    depth = E.bone_depths(t["kp"])[0]
    o64, _, valid = E.lift_keypoints(t["kp"], depth)
    want = BT.positions(t["kp"], depth.cpu().numpy(), cam)
    assert np.array_equal(valid.cpu().numpy().astype(bool), BT.usable(t["kp"]))
    np.testing.assert_allclose(o64.cpu().numpy(), want, rtol=F64_RTOL, atol=0)
    # ... and, where the frame is well-conditioned, the twin's own positions to the gate
    own = BT.positions(t["kp"], t["depth"], cam)
    assert np.abs(o64.cpu().numpy() - own)[t["keep"]].max() <= twin["gate"]


def _opts_struct(o):
    from globalegomocap_amd import _capi
    s = _capi.GemBoneDepthOpts(neck_depth=o["neck_depth"], w_n=o["w_n"], w_m=o["w_m"], iters=o["iters"], reserved=0)
    for j in range(15):
        s.bone[j], s.dbar[j] = o["L"][j], o["dbar"][j]
    return s


def _call(E, kp_d, n, o, depth, solved, rms, handle=True, n_poly=None):
    import torch
    poly = np.ascontiguousarray(E.camera.poly_c2w, dtype=np.float64)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)          # noqa: E731
    rc = E.lib.gem_bone_depths(E._h if handle else C.c_void_p(0), p(kp_d), n, poly.ctypes.data_as(C.POINTER(C.c_double)),
                               len(poly) if n_poly is None else n_poly, C.byref(_opts_struct(o)) if o is not None else None, p(depth), p(solved),
                               p(rms), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, E.lib.gem_last_error().decode()


def test_guards_null_outputs_and_bad_arguments(E, twin, opts):
    import torch
    n = 67
    kp = twin[n]["kp"]
    kp_d = torch.from_numpy(kp).to(E.device)
    full = E.bone_depths(kp_d)
    # canaries behind (and in front of) every output
    bufs = [torch.full((n * 15 + 128,), -7.0, dtype=torch.float64, device=E.device), torch.full((n * 15 + 128,), 7, dtype=torch.uint8, device=E.device),
            torch.full((n + 128,), -7.0, dtype=torch.float64, device=E.device)]
    views = (bufs[0][64:64 + n * 15].view(n, 15), bufs[1][64:64 + n * 15].view(n, 15), bufs[2][64:64 + n])
    got = E.bone_depths(kp_d, out=views)
    assert all(g is v for g, v in zip(got, views)) and all(torch.equal(g, f) for g, f in zip(got, full))
    for b, size, canary in zip(bufs, (n * 15, n * 15, n), (-7.0, 7, -7.0)):
        assert (b[:64] == canary).all() and (b[64 + size:] == canary).all()
    # each output may be NULL, not all three
    for skip in range(3):
        outs = [torch.zeros_like(f) for f in full]
        args = [None if i == skip else o for i, o in enumerate(outs)]
        rc, _ = _call(E, kp_d, n, opts, *args)
        assert rc == 0
        assert all(torch.equal(o, f) for i, (o, f) in enumerate(zip(outs, full)) if i != skip)
    # refusals: nothing is launched, so nothing is written
    outs = [torch.full_like(f, 3) for f in full]
    bad = dict(opts, L=np.where(np.arange(15) == 0, 0.1, opts["L"]))
    nan = dict(opts, L=np.where(np.arange(15) == 5, np.nan, opts["L"]))
    near = dict(opts, dbar=np.where(np.arange(15) == 5, 0.001, opts["dbar"]))
    refused = [_call(E, kp_d, n, opts, None, None, None), _call(E, kp_d, n, opts, *outs, handle=False), _call(E, kp_d, n, opts, *outs, n_poly=0),
               _call(E, kp_d, n, opts, *outs, n_poly=17), _call(E, kp_d, -1, opts, *outs), _call(E, kp_d, 1 << 27, opts, *outs),
               _call(E, kp_d, n, None, *outs), _call(E, None, n, opts, *outs), _call(E, kp_d, n, bad, *outs), _call(E, kp_d, n, nan, *outs),
               _call(E, kp_d, n, near, *outs), _call(E, kp_d, n, dict(opts, w_m=0.0), *outs), _call(E, kp_d, n, dict(opts, w_n=-1.0), *outs),
               _call(E, kp_d, n, dict(opts, neck_depth=0.0), *outs), _call(E, kp_d, n, dict(opts, iters=0), *outs),
               _call(E, kp_d, n, dict(opts, iters=1001), *outs)]
    torch.cuda.synchronize()
    assert all(rc == 1 and msg.startswith("gem_bone_depths: ") for rc, msg in refused), refused
    assert all((o == 3).all() for o in outs)
    assert _call(E, None, 0, opts, None, None, None)[0] == 0          # no frames: nothing to do
    with pytest.raises(ValueError):
        E.bone_depths(kp[:, :14])
    with pytest.raises(TypeError):
        E.bone_depths(kp, out=(full[0].float(), None, None))
    with pytest.raises(ValueError):
        E.bone_depths(kp, out=(full[0][:5], None, None))
    with pytest.raises(ValueError, match="neck_depth"):
        E.bone_depths(kp, neck_depth=0.0)
    # the options reach the kernel: another anchor, other depths; more iterations, a residual no larger
    far = E.bone_depths(kp, neck_depth=0.35)
    assert abs(float(far[0][0, 0]) - 0.35) < 0.01 and abs(float(full[0][0, 0]) - opts["neck_depth"]) < 0.01
    longer = E.bone_depths(kp, iters=60)
    d60, s60, _, spread60 = _spread(kp, FisheyeCamera.from_json(DEFAULT_CALIBRATION), dict(opts, iters=60))
    keep60 = spread60 <= BT.ILL_CONDITIONED
    assert keep60.sum() >= 0.98 * n and np.array_equal(longer[1].cpu().numpy(), s60)
    assert np.abs(longer[0].cpu().numpy() - d60)[keep60].max() <= 16 * BT.ILL_CONDITIONED          # (the gate's rule with the cap for the spread)
    assert np.abs(d60 - twin[n]["depth"]).max() > 1e-6                                              # (it is another result)


# ------------------------------------------------------------------------------------------------------------------ end to end, offline
N_FRAMES, TEST_SIZE = 40, 20          # the recording sizes of tests/test_keypoints_gpu.py's offline fixture: two chunks


def _trajectory(path, n):
    with open(path, "w") as f:
        for i in range(n + 1):
            f.write("%.9f %.9f 0 0 0 0 0 1\n" % (i / 25.0, 0.004 * i))


def test_offline_route_end_to_end(E, twin, cam, opts, golden, tmp_path, capsys):
    import torch
    from helpers import sd_from_npz
    from globalegomocap_amd import bone_depth as B, detections as D, prepare as P, whole_sequence as ws
    truth = BT.motion(N_FRAMES, 0.3, np.random.default_rng(34))
    kp = BT.detect(truth, cam, conf=0.9)
    kp[5:8, 6, 2] = 0.0                          # the detector lost the left wrist for three frames
    d, s, rms, spread = _spread(kp, cam, opts)
    assert (spread <= BT.ILL_CONDITIONED).all()          # (this sequence has no ill-conditioned frame: a filled frame reads its neighbours)
    traj = str(tmp_path / "traj.txt")
    _trajectory(traj, N_FRAMES)
    spans = P.chunk_spans(0, N_FRAMES + 1, TEST_SIZE)
    assert spans == [(0, 20), (20, 40)]
    rec = D.recording_from_detections(traj, kp, scale=1.0, spans=spans, depth="bones")
    ref = D.recording_from_detections(traj, kp, scale=1.0, spans=spans, depth=d)
    assert ref.depth_report is None and isinstance(rec.depth_report, B.BoneDepthReport)
    rep = rec.depth_report.as_dict()
    assert (rep["frames"], rep["solved"], rep["unsolved"], rep["frames_without_neck"]) == (40, 40 * 15 - 3, 3, 0)
    assert abs(rep["rms_max"] - rms.max()) <= twin["gate"] and abs(rep["rms_median"] - np.sort(rms)[19]) <= twin["gate"]
    worst = 0.0
    for a, b in zip(rec.chunks, ref.chunks):
        worst = max(worst, float((a.est_local - b.est_local).abs().max()))
        assert torch.equal(a.heat, b.heat) and torch.equal(a.cams, b.cams)
    assert np.array_equal(rec.origins, ref.origins)
    assert not rec.chunks[0].heat[5:8, :, :, 6].any() and rec.chunks[0].heat[4, :, :, 6].any()
    with capsys.disabled():
        print("offline route: est_local with device-made depths against the twin's depths: at most %.3g m (gate %.3g m)" % (worst, twin["gate"]))
    assert worst <= twin["gate"]
    # a joint the solve cannot reach in a whole chunk: refused, like a joint that was never detected
    cut = kp.copy()
    cut[20:, 2, 2] = 0.0
    with pytest.raises(ValueError, match=r"joints \[2, 3\] have no usable detection in the chunk \[20, 40\)"):
        D.recording_from_detections(traj, cut, scale=1.0, spans=spans, depth="bones")
    # the optimiser takes it; recorded, not gated: how far its result lies from that of the route fed the true depths
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False)
    true = D.recording_from_detections(traj, kp, scale=1.0, spans=spans, depth=np.linalg.norm(truth, axis=-1))
    torch.manual_seed(5)
    a = ws.optimize_recording(rec, DEFAULT_CALIBRATION, ground_truth=False, **kw)
    torch.manual_seed(5)
    b = ws.optimize_recording(true, DEFAULT_CALIBRATION, ground_truth=False, **kw)
    assert a[3].shape == b[3].shape and a[3].shape[1:] == (15, 3) and np.isfinite(a[3]).all()
    lifted = float(np.linalg.norm(np.concatenate([c.est_local.cpu().numpy() for c in rec.chunks]) - truth, axis=-1).mean())
    with capsys.disabled():
        print("offline route: the lift with bone-length depths lies %.2f mm (MPJPE) from the truth; optimised, %.2f mm from the optimised route fed "
              "the true depths" % (lifted * 1e3, float(np.linalg.norm(a[3] - b[3], axis=-1).mean()) * 1e3))
    # the command writes the array `--depth FILE.npy` reads, and the three agree
    det = str(tmp_path / "det.npz")
    np.savez(det, keypoints=kp)
    B._cli(["--keypoints", det, "--out", str(tmp_path / "depth.npy"), "--json", str(tmp_path / "report.json")])
    saved = np.load(str(tmp_path / "depth.npy"))
    assert saved.dtype == np.float64 and saved.shape == (40, 15)
    import json
    with open(str(tmp_path / "report.json")) as f:
        assert json.load(f) == rep
    again = D.recording_from_detections(traj, det, scale=1.0, spans=spans, depth=saved)
    masked = D.recording_from_detections(traj, det, scale=1.0, spans=spans, depth="bones")
    assert all(torch.equal(x.est_local, y.est_local) and torch.equal(x.est_local, z.est_local) for x, y, z in zip(again.chunks, rec.chunks, masked.chunks))


# ------------------------------------------------------------------------------------------------------------------ end to end, live
def test_live_route_end_to_end(E, cam, tmp_path):
    """A 26-frame stream whose depths the session solves push by push: the rings hold, bit for bit, what the offline route lifts for
    those frames -- a frame's depths do not depend on the frames that share its call -- and `replay(depth_from="bones")` is that
    session."""
    import torch
    from helpers import TINY
    from globalegomocap_amd import detections as D, live as L, slam, vae as vae_schema
    n, pieces = 26, (1, 5, 8, 12)
    kp = BT.detect(BT.motion(n, 0.3, np.random.default_rng(45)), cam, conf=0.7)
    kp[9:12, 3, 2] = 0.0                         # a wrist lost for three frames: held in the stream, interpolated offline
    det, traj = str(tmp_path / "det.npz"), str(tmp_path / "traj.txt")
    np.savez(det, keypoints=kp)
    _trajectory(traj, n)
    with open(traj) as f:
        rows = slam.trajectory_rows(f.read())[:n]
    sd_l, sd_g = vae_schema.synthetic_state_dict(TINY, 11), vae_schema.synthetic_state_dict(TINY, 12)
    eps = np.random.default_rng(6).normal(size=(3, 2, TINY.latent_dim)).astype(np.float32)
    session = dict(global_vae=sd_g, local_vae=sd_l, eps=lambda w: eps[w], scale=1.0)
    live = L.LiveOptimizer(DEFAULT_CALIBRATION, **session)
    at = 0
    for k in pieces:
        depth, solved, masked = live.bone_depths(kp[at:at + k])
        assert depth.is_cuda and tuple(depth.shape) == (k, 15) and solved.dtype == torch.uint8 and tuple(masked.shape) == (k, 15, 3)
        live.push(keypoints=masked, depth=depth, rows=rows[at:at + k])
        at += k
    ring = live._bufs["ring_pose"][:n].cpu().numpy()
    live.flush()
    own = live.result()
    live.close()
    rec = D.recording_from_detections(traj, det, scale=1.0, spans=[(0, n)], depth="bones")
    lifted = E.lift_keypoints(kp, E.bone_depths(kp)[0])[0].cpu().numpy().astype(np.float32)
    seen = BT.solved_mask(kp)
    assert (~seen).sum() == 3 and np.array_equal(ring[seen].view(np.uint32), lifted[seen].view(np.uint32))
    offline = rec.chunks[0].est_local.cpu().numpy().astype(np.float32)
    assert np.array_equal(ring[seen].view(np.uint32), offline[seen].view(np.uint32))
    assert np.array_equal(ring[9:12, 3], np.broadcast_to(ring[8, 3], (3, 3))) and not np.array_equal(offline[10, 3], offline[8, 3])
    assert own["optimized"].shape == (n, 15, 3) and np.isfinite(own["optimized"]).all()
    res, log = L.replay(traj, None, None, 0, n, DEFAULT_CALIBRATION, verbose=False, keypoints=det, depth_from="bones", **session)
    assert res["optimized"].shape == (n, 15, 3) and res["dropped"] == 0 and len(log) == 3          # every frame is emitted
    assert np.array_equal(res["estimated"].view(np.uint64), own["estimated"].view(np.uint64))
    assert np.array_equal(res["optimized"].view(np.uint64), own["optimized"].view(np.uint64))
    with pytest.raises(ValueError, match="depths are needed"):
        L.replay(traj, None, None, 0, n, DEFAULT_CALIBRATION, verbose=False, keypoints=det, **session)
    with pytest.raises(ValueError, match="depth_from"):
        L.replay(traj, None, "DIR", 0, n, DEFAULT_CALIBRATION, verbose=False, keypoints=det, depth_from="bones", **session)
    # the session's own skeleton: 5 % longer bones, depths 5 % larger
    big = L.LiveOptimizer(DEFAULT_CALIBRATION, bones_for_depth=1.05 * np.asarray(live._depth_opts["L"]), **session)
    d_big = big.bone_depths(kp[:4])[0].cpu().numpy()
    big.close()
    np.testing.assert_allclose(d_big, 1.05 * E.bone_depths(kp[:4])[0].cpu().numpy(), rtol=1e-6)
