"""2-D joint detections on the device: the three kernels against their numpy twins (tests/keypoints_twin.py), the
un-projection against the existing heat-map route bit for bit, and both routes end to end -- `recording_from_detections` through
`optimize_recording`, and `LiveOptimizer.push(keypoints=)`."""
import os
import pickle

import numpy as np
import pytest

import keypoints_twin as KT
from globalegomocap_amd import synth
from globalegomocap_amd.camera import DEFAULT_CALIBRATION, FisheyeCamera

pytestmark = pytest.mark.gpu

SPLAT_ATOL = 1e-6          # values <= 1; two exponentials and a product, and the argument's rounding x e^-x 2^-23 <= 5e-8: an indexing mistake shows as 0.1
F64_RTOL = 1e-12
GATE = 0.5e-3              # the merged-pose difference tests/test_hip_full_size.py holds the chained call to


@pytest.fixture(scope="module")
def E():
    """The 64 x 64 engine `prepare` lifts under, and the calibration."""
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import prepare
    return prepare._lift_engine(DEFAULT_CALIBRATION, 0)


def _engine_of(size):
    from helpers import TINY
    from globalegomocap_amd.engine import WindowEngine
    return WindowEngine(TINY, FisheyeCamera.from_json(DEFAULT_CALIBRATION), max_windows=1, heat_size=size)


def _splat_case(F, H, W, seed):
    """Sub-pixel centres all over the map (some within a pixel of its border), and the special detections."""
    rng = np.random.default_rng(seed)
    ix, iy = rng.uniform(-1.0, W, (F, 15)), rng.uniform(-1.0, H, (F, 15))
    kp = np.stack([128.0 + ix * 1024.0 / (W - 1), iy * 1024.0 / (H - 1), rng.uniform(0.05, 1.0, (F, 15))], axis=2)
    kp[0, 2, :2] = (5000.0, -3000.0)          # far outside the map
    kp[0, 5, 2] = 0.0                         # confidence 0
    kp[0, 7, 0] = np.nan                      # NaN u
    kp[0, 9] = (128.0 + (W // 2 + 0.3) * 1024.0 / (W - 1), (H // 2 - 0.4) * 1024.0 / (H - 1), 1.7)          # clamped to 1, peak exp(-0.25 / 4.5)
    kp[F - 1, 0, 2] = np.nan
    kp[F - 1, 14, 1] = np.inf
    kp[F - 1, 3, 2] = -0.3
    return kp


@pytest.mark.parametrize("F,H,W", [(3, 64, 64), (2, 47, 33)], ids=["3 x 64x64", "2 x 47x33 (odd run, unaligned frame)"])
def test_splat_against_the_twin(E, F, H, W, capsys):
    import torch
    eng = E if (H, W) == (64, 64) else _engine_of((H, W))
    kp = _splat_case(F, H, W, seed=H)
    want = KT.splat(kp, H, W, 1.5)
    got_d = eng.keypoint_heatmaps(kp)
    assert got_d.dtype == torch.float32 and tuple(got_d.shape) == (F, H, W, 15) and got_d.is_cuda
    got = got_d.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    with capsys.disabled():
        print("splat %d x %dx%d: largest difference to the twin %.3g, %d of %d values differ" % (F, H, W, err.max(), (got != want).sum(), got.size))
    assert err.max() <= SPLAT_ATOL
    blank = ~KT.usable(kp)
    assert blank.sum() == 5 and not got[np.broadcast_to(blank[:, None, None, :], got.shape)].any()          # exactly zero
    assert np.isfinite(got).all() and got.max() <= 1.0 and abs(got[0, :, :, 9].max() - np.exp(-0.25 / 4.5)) < 1e-6                       # 1.7 was clamped, not dropped
    assert not got[0, :, :, 2].any() or got[0, :, :, 2].max() < 1e-30                                       # far outside: nothing inside
    # H and W the right way round, peaks where the twin has them
    usable = ~blank & (got.reshape(F, -1, 15).max(axis=1) > 0)
    assert np.array_equal(got.reshape(F, -1, 15).argmax(axis=1)[usable], want.reshape(F, -1, 15).argmax(axis=1)[usable])
    # two-column detections: confidence 1
    two = eng.keypoint_heatmaps(kp[1:, :, :2]).cpu().numpy()
    assert np.abs(two - KT.splat(np.concatenate([kp[1:, :, :2], np.ones((F - 1, 15, 1))], 2), H, W)).max() <= SPLAT_ATOL
    # another sigma
    np.testing.assert_allclose(eng.keypoint_heatmaps(kp, sigma=2.25).cpu().numpy(), KT.splat(kp, H, W, 2.25), rtol=0, atol=SPLAT_ATOL)
    # into a buffer with 64 guard floats on either side: the same values, the guards untouched
    n = F * H * W * 15
    buf = torch.full((n + 128,), -7.0, dtype=torch.float32, device=eng.device)
    eng.keypoint_heatmaps(kp, out=buf[64:64 + n].view(F, H, W, 15))
    back = buf.cpu().numpy()
    assert (back[:64] == -7.0).all() and (back[64 + n:] == -7.0).all()
    assert np.array_equal(back[64:64 + n].reshape(F, H, W, 15), got)
    # ... and starting one float off a 16-byte boundary
    buf.fill_(-7.0)
    eng.keypoint_heatmaps(kp, out=buf[63:63 + n].view(F, H, W, 15))
    back = buf.cpu().numpy()
    assert (back[:63] == -7.0).all() and (back[63 + n:] == -7.0).all() and np.array_equal(back[63:63 + n].reshape(F, H, W, 15), got)
    with pytest.raises(ValueError):
        eng.keypoint_heatmaps(kp[:, :14])
    with pytest.raises(ValueError):
        eng.keypoint_heatmaps(kp, sigma=0.0)
    if eng is not E:
        eng.close()


def test_lift_against_the_twin(E, capsys):
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    rng = np.random.default_rng(11)
    kp = np.concatenate([rng.uniform(0, 1280, (9, 15, 1)), rng.uniform(0, 1024, (9, 15, 1)), rng.uniform(0.1, 1.0, (9, 15, 1))], axis=2)
    kp[2, 3, 2], kp[4, 0, 0], kp[8, 14, 1], kp[5, 5, 2] = 0.0, np.nan, -np.inf, np.nan
    depth = rng.uniform(0.2, 1.6, (9, 15))
    want, ok, _ = KT.lift(kp, depth, cam)
    o64, o32, valid = E.lift_keypoints(kp, depth)
    o64, o32, valid = o64.cpu().numpy(), o32.cpu().numpy(), valid.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.nanmax(np.abs(o64 - want) / np.abs(want))
    with capsys.disabled():
        print("lift: largest relative difference to the twin %.3g" % rel)
    assert valid.dtype == np.uint8 and np.array_equal(valid, ok) and ok.sum() == 9 * 15 - 4
    np.testing.assert_allclose(o64, want, rtol=F64_RTOL, atol=0)
    assert o32.dtype == np.float32 and np.array_equal(o32, o64.astype(np.float32))
    assert not o64[~ok.astype(bool)].any()
    none64, only32, _ = E.lift_keypoints(kp, depth, want_f64=False)
    assert none64 is None and np.array_equal(only32.cpu().numpy(), o32)
    with pytest.raises(ValueError):
        E.lift_keypoints(kp, depth[:, :14])
    with pytest.raises(ValueError):
        E.lift_keypoints(kp[..., :1], depth)


def test_lift_is_the_heat_map_route_on_its_grid_bitwise(E):
    """Detections whose splat peaks exactly on integer heat-map pixels p: `lift_skeleton` of the splatted maps un-projects the image
    pixel (16 px + 128, 16 py) (lift_skeleton_kernel: the top-left pixel of p's 16 x 16 block behind 128 padded columns);
    `lift_keypoints` at that pixel gives the same bits."""
    rng = np.random.default_rng(13)
    px, py = rng.integers(0, 64, (6, 15)), rng.integers(0, 64, (6, 15))
    kp = np.stack([128.0 + px * 1024.0 / 63.0, py * 1024.0 / 63.0, np.ones((6, 15))], axis=2)
    depth = rng.uniform(0.2, 1.6, (6, 15))
    heat = E.keypoint_heatmaps(kp)
    flat = heat.cpu().numpy().reshape(6, -1, 15).argmax(axis=1)
    assert np.array_equal(flat % 64, px) and np.array_equal(flat // 64, py)
    a64, a32 = E.lift_skeleton(heat, depth)
    kp_grid = np.stack([16.0 * px + 128.0, 16.0 * py, np.ones((6, 15))], axis=2)
    b64, b32, valid = E.lift_keypoints(kp_grid, depth)
    assert valid.cpu().numpy().all()
    assert np.array_equal(a64.cpu().numpy().view(np.uint64), b64.cpu().numpy().view(np.uint64))
    assert np.array_equal(a32.cpu().numpy().view(np.uint32), b32.cpu().numpy().view(np.uint32))
    # (the splat's own centre is another image point: the sampling map and the lifting map differ)
    assert np.abs(kp[..., :2] - kp_grid[..., :2]).max() > 1.0


def test_hold_and_fill(E, capsys):
    import torch
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    rng = np.random.default_rng(17)
    valid = KT.pattern_valid(2, 15)
    assert valid.shape == (14, 15) and valid[:7].any(axis=0).all() and valid[7:].any(axis=0).all()
    kp = np.concatenate([rng.uniform(100, 1200, (14, 15, 1)), rng.uniform(50, 1000, (14, 15, 1)), rng.uniform(0.1, 1.0, (14, 15, 1))], axis=2)
    kp[..., 2] = np.where(valid, kp[..., 2], 0.0)
    kp[1, 0, :] = (np.nan, 300.0, 0.9)          # (invalid in the pattern already: another way of being unusable)
    depth = rng.uniform(0.2, 1.6, (14, 15))
    # offline: lift, then interpolate inside each of the 2 chunks of 7 frames
    o64, _, v = E.lift_keypoints(kp, depth)
    assert np.array_equal(v.cpu().numpy(), valid)
    lifted = o64.cpu().numpy()
    filled = E.fill_missing(o64, v, 2)
    assert filled is o64
    want = KT.fill_missing(KT.lift(kp, depth, cam)[0], valid, 2)
    got = filled.cpu().numpy()
    with capsys.disabled():
        print("fill: largest difference to the twin %.3g m" % np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert np.array_equal(got[valid.astype(bool)], lifted[valid.astype(bool)])          # valid frames are not touched
    assert np.abs(got[~valid.astype(bool)]).min() > 0
    with pytest.raises(ValueError):
        E.fill_missing(o64, v, 3)
    with pytest.raises(TypeError):
        E.fill_missing(o64, v.to(torch.int32), 2)
    # live: hold the last usable value, `prev` carried across two consecutive calls
    prev0 = rng.normal(size=(15, 3))
    prev = torch.from_numpy(prev0.copy()).to(E.device)
    first = E.lift_keypoints(kp[:7], depth[:7], prev=prev)
    mid = prev.cpu().numpy()
    second = E.lift_keypoints(kp[7:], depth[7:], prev=prev)
    w_out, w_ok, w_held = KT.lift(kp, depth, cam, prev0)
    h64 = np.concatenate([first[0].cpu().numpy(), second[0].cpu().numpy()])
    np.testing.assert_allclose(h64, w_out, rtol=F64_RTOL, atol=0)
    assert np.array_equal(np.concatenate([first[2].cpu().numpy(), second[2].cpu().numpy()]), w_ok)
    np.testing.assert_allclose(prev.cpu().numpy(), w_held, rtol=F64_RTOL, atol=0)
    np.testing.assert_allclose(mid, KT.lift(kp[:7], depth[:7], cam, prev0)[2], rtol=F64_RTOL, atol=0)
    assert np.array_equal(h64[0, 0], prev0[0]) and np.array_equal(h64[7, 4], mid[4])          # held from before the call / from the call before
    assert np.array_equal(np.concatenate([first[1].cpu().numpy(), second[1].cpu().numpy()]), h64.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ end to end, offline
N_FRAMES, TEST_SIZE = 40, 20


@pytest.fixture(scope="module")
def offline(E, golden, tmp_path_factory):
    """A 40-frame synthetic recording as detections: the projections of the noise-free local skeleton, two joints knocked out, the
    depths of the noisy estimate; its trajectory file and ground-truth pickle."""
    from helpers import sd_from_npz
    tmp = tmp_path_factory.mktemp("keypoints")
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    seq = synth.make_sequence(n_frames=N_FRAMES, seed=33, camera=cam, with_heatmaps=False)
    cams = np.asarray(seq["camera_pose_list"])
    clean = np.asarray(seq["gt_global_skeleton"]) - cams[:, None, :3, 3]          # (make_cameras: identity rotations)
    uv = cam.project_numpy(clean.reshape(-1, 3)).reshape(N_FRAMES, 15, 2)
    kp = np.concatenate([uv, np.ones((N_FRAMES, 15, 1))], axis=2)
    kp[5:8, 6, 2] = 0.0                          # the detector lost joint 6 for three frames
    kp[31, 12, 0] = np.nan                       # ... and joint 12 for one, in the second chunk
    depth = np.linalg.norm(np.asarray(seq["estimated_local_skeleton"]), axis=-1)
    traj = str(tmp / "traj.txt")
    with open(traj, "w") as f:
        for i in range(N_FRAMES + 1):
            f.write("%.9f %.9f 0 0 0 0 0 1\n" % (i / 25.0, 0.004 * i))
    gt = str(tmp / "gt.pkl")
    with open(gt, "wb") as f:
        pickle.dump([np.asarray(p) for p in seq["gt_global_skeleton"]], f)
    np.savez(str(tmp / "det.npz"), keypoints=kp, depth=depth)
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False)
    return dict(tmp=tmp, kp=kp, depth=depth, traj=traj, gt=gt, det=str(tmp / "det.npz"), kw=kw, seq=seq, cams=cams)


def test_offline_route_end_to_end(E, offline, capsys):
    import torch
    from globalegomocap_amd import detections as D, prepare as P, whole_sequence as ws
    o, kw = offline, offline["kw"]
    spans = P.chunk_spans(0, N_FRAMES + 1, TEST_SIZE)
    assert spans == [(0, 20), (20, 40)]
    rec = D.recording_from_detections(o["traj"], o["det"], scale=1.0, spans=spans, fps=25)
    assert isinstance(rec, P.Recording) and len(rec) == 2 and rec.origins.shape == (2, 4, 4)
    valid = KT.usable(o["kp"])
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    want_local = KT.fill_missing(KT.lift(o["kp"], o["depth"], cam)[0], valid, 2)
    want_heat = KT.splat(o["kp"])
    for k, c in enumerate(rec.chunks):
        sl = slice(20 * k, 20 * k + 20)
        assert c.gt is None and c.heat.is_cuda and c.heat.dtype == torch.float32 and tuple(c.heat.shape) == (20, 64, 64, 15)
        np.testing.assert_allclose(c.est_local.cpu().numpy(), want_local[sl], rtol=0, atol=1e-12)
        assert np.abs(c.heat.cpu().numpy() - want_heat[sl]).max() <= SPLAT_ATOL
        rel = o["cams"][sl].copy()
        rel[:, 0, 3] -= o["cams"][20 * k, 0, 3]
        np.testing.assert_allclose(c.cams.cpu().numpy(), rel, rtol=0, atol=1e-9)          # (the file's nine decimals)
        g = np.einsum("nij,nkj->nki", c.cams.cpu().numpy()[:, :3, :3], c.est_local.cpu().numpy()) + c.cams.cpu().numpy()[:, None, :3, 3]
        np.testing.assert_allclose(c.est_global.cpu().numpy(), g, rtol=0, atol=1e-12)
    assert not rec.chunks[0].heat[5:8, :, :, 6].any() and not rec.chunks[1].heat[11, :, :, 12].any()          # blank where the joint was lost
    # the same detections given as arrays
    again = D.recording_from_detections(o["traj"], o["kp"], scale=1.0, spans=spans, depth=o["depth"])
    assert all(torch.equal(a.heat, b.heat) and torch.equal(a.est_local, b.est_local) for a, b in zip(again.chunks, rec.chunks))
    # a joint lost for a whole chunk: refused
    lost = o["kp"].copy()
    lost[20:, 3, 2] = 0.0
    with pytest.raises(ValueError, match=r"joints \[3\] have no usable detection in the chunk \[20, 40\)"):
        D.recording_from_detections(o["traj"], lost, scale=1.0, spans=spans, depth=o["depth"])
    with pytest.raises(ValueError, match="depths are needed"):
        D.recording_from_detections(o["traj"], o["kp"], scale=1.0, spans=spans)
    # optimised: against the same Recording with host-made heat-maps, within the project's own sequence gate
    host = P.Recording([P.RecordingChunk(c.start_frame, c.end_frame, torch.from_numpy(want_heat[20 * k:20 * k + 20]).to(c.heat.device), c.est_local,
                                         c.est_global, c.cams, None) for k, c in enumerate(rec.chunks)], rec.origins)
    torch.manual_seed(5)
    a = ws.optimize_recording(rec, DEFAULT_CALIBRATION, ground_truth=False, **kw)
    torch.manual_seed(5)
    b = ws.optimize_recording(host, DEFAULT_CALIBRATION, ground_truth=False, **kw)
    d_opt = float(np.linalg.norm(a[3] - b[3], axis=-1).mean())
    moved = float(np.linalg.norm(a[3] - a[2], axis=-1).mean())
    with capsys.disabled():
        print("offline route: merged optimised pose, device-made against host-made heat-maps: %.6f mm (the optimiser moved the poses by %.3f mm)"
              % (d_opt * 1e3, moved * 1e3))
    assert a[3].shape == b[3].shape and a[3].shape[1:] == (15, 3) and np.isfinite(a[3]).all() and moved > 1e-4
    assert d_opt < GATE
    # the pickles are ordinary chunks: read back, the same result
    root = str(o["tmp"] / "chunks")
    dirs = rec.write_chunks(root)
    assert [os.path.basename(d) for d in dirs] == ["data_start_0_end_20", "data_start_20_end_40"]
    with open(os.path.join(dirs[0], "test_data.pkl"), "rb") as f:
        assert list(pickle.load(f)) == list(P.PICKLE_KEYS[1:])
    torch.manual_seed(5)
    c = ws.optimize_directory(root, DEFAULT_CALIBRATION, ground_truth=False, **kw)
    assert np.array_equal(c[3], a[3]) and np.array_equal(c[2], a[2]) and list(c[0]) == list(a[0])
    # the ground-truth route, once: its initial mpjpe and the 18-entry report
    rec_gt = D.recording_from_detections(o["traj"], o["det"], gt_path=o["gt"], spans=spans, fps=25)
    assert rec_gt.origins is None and len(rec_gt) == 2
    for k, ch in enumerate(rec_gt.chunks):
        assert ch.gt is not None and len(ch.gt_list) == 20 and np.isfinite(ch.initial_mpjpe) and 0 < ch.initial_mpjpe < 0.1
        assert torch.equal(ch.heat, rec.chunks[k].heat) and torch.equal(ch.est_local, rec.chunks[k].est_local)
    torch.manual_seed(5)
    g = ws.optimize_recording(rec_gt, DEFAULT_CALIBRATION, **kw)
    assert len(g[0]) == 18 and len(g[1]) == 2 and g[4] is not None and np.isfinite(g[3]).all()
    assert all(np.isfinite(np.asarray(v)).all() for v in g[0].values())


# ------------------------------------------------------------------------------------------------------------------ end to end, live
def test_live_route_end_to_end(E):
    """A 26-frame stream pushed with keypoints= and depth= against a session pushed with the maps `keypoint_heatmaps` makes and the held
    lift of the same frames: the same bits."""
    import torch
    from helpers import TINY
    from globalegomocap_amd import vae as vae_schema
    from globalegomocap_amd.live import LiveOptimizer
    n, pieces = 26, (1, 5, 8, 12)
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    seq = synth.make_sequence(n_frames=n, seed=44, camera=cam, with_heatmaps=False, cam_jitter=(1.0, 0.005))
    clean = np.asarray(seq["estimated_local_skeleton"])          # (any plausible skeleton will do as the detector's target)
    kp = np.concatenate([cam.project_numpy(clean.reshape(-1, 3)).reshape(n, 15, 2), np.full((n, 15, 1), 0.9)], axis=2)
    kp[3:6, 8, 2], kp[6, 2, 0], kp[17, 11, 2] = 0.0, np.nan, -1.0          # lost across a push boundary, in one frame, late in the stream
    depth = np.linalg.norm(clean, axis=-1)
    cams, times = np.asarray(seq["camera_pose_list"]), np.arange(n) / 25.0
    sd_l, sd_g = vae_schema.synthetic_state_dict(TINY, 11), vae_schema.synthetic_state_dict(TINY, 12)
    eps = np.random.default_rng(6).normal(size=(3, 2, TINY.latent_dim)).astype(np.float32)
    weights = dict(vae_weight=1e-3, smoothness_weight=1e-3, bone_length_weight=1e-2, weight_3d=1e-2, reproj_weight=1e-2)

    def run(**inputs):
        live = LiveOptimizer(DEFAULT_CALIBRATION, sd_g, sd_l, eps=lambda w: eps[w], weights=weights)
        at = 0
        for k in pieces:
            live.push(**{name: x[at:at + k] for name, x in inputs.items()})
            at += k
        tail = live.flush()
        res = dict(live.result(), dropped=tail["dropped"])
        live.close()
        return res
    a = run(keypoints=kp, depth=depth, cams=cams, times=times)
    heat = E.keypoint_heatmaps(kp)
    held = E.lift_keypoints(kp, depth, prev=torch.zeros(15, 3, dtype=torch.float64, device=E.device), want_f64=False)[1]
    assert np.array_equal(held[4, 8].cpu().numpy(), held[2, 8].cpu().numpy()) and not np.array_equal(held[6, 8].cpu().numpy(), held[2, 8].cpu().numpy())
    b = run(heat=heat, est_local=held, cams=cams, times=times)
    assert a["optimized"].shape == (26, 15, 3) and a["dropped"] == 0
    assert np.array_equal(a["optimized"].view(np.uint64), b["optimized"].view(np.uint64))
    assert np.array_equal(a["estimated"].view(np.uint64), b["estimated"].view(np.uint64))
    assert np.abs(a["optimized"] - a["estimated"]).max() > 1e-4
    # est_local= with keypoints=: only the maps are made
    c = run(keypoints=kp, est_local=held, cams=cams, times=times)
    assert np.array_equal(c["optimized"].view(np.uint64), a["optimized"].view(np.uint64))
    # a first frame without one of its joints: refused before anything is pushed
    live = LiveOptimizer(DEFAULT_CALIBRATION, sd_g, sd_l, eps=lambda w: eps[w], weights=weights)
    bad = kp[:1].copy()
    bad[0, 5, 2] = 0.0
    with pytest.raises(ValueError, match=r"joints \[5\] of the session's first frame"):
        live.push(keypoints=bad, depth=depth[:1], cams=cams[:1], times=times[:1])
    assert live.n_pushed == 0
    live.close()


def test_replay_with_keypoints(E, tmp_path):
    """`live.replay(keypoints=FILE)`: the detections file pushed frame by frame, depths from the file -- the session a caller gets by
    pushing the same rows itself."""
    from helpers import TINY
    from globalegomocap_amd import live as L, slam, synth_recording as S, vae as vae_schema
    n = 26
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    seq = synth.make_sequence(n_frames=n, seed=45, camera=cam, with_heatmaps=False)
    pose = np.asarray(seq["estimated_local_skeleton"])
    kp = np.concatenate([cam.project_numpy(pose.reshape(-1, 3)).reshape(n, 15, 2), np.full((n, 15, 1), 0.7)], axis=2)
    kp[9:12, 4, 2] = 0.0
    depth = np.linalg.norm(pose, axis=-1)
    det, traj = str(tmp_path / "det.npz"), str(tmp_path / "traj.txt")
    np.savez(det, keypoints=kp, depth=depth, frame_ids=np.arange(100, 100 + n))
    with open(traj, "w") as f:
        for r in S.random_parameters(n, seed=5, first_id=100)["rows"]:
            f.write(" ".join("%.9f" % v for v in r) + "\n")
    with open(traj) as f:
        rows = slam.trajectory_rows(f.read())
    sd_l, sd_g = vae_schema.synthetic_state_dict(TINY, 11), vae_schema.synthetic_state_dict(TINY, 12)
    eps = np.random.default_rng(6).normal(size=(3, 2, TINY.latent_dim)).astype(np.float32)
    session = dict(global_vae=sd_g, local_vae=sd_l, eps=lambda w: eps[w], scale=1.3)
    res, log = L.replay(traj, None, None, 100, 100 + n, DEFAULT_CALIBRATION, verbose=False, keypoints=det, **session)
    assert res["optimized"].shape == (26, 15, 3) and res["dropped"] == 0 and len(log) == 3
    live = L.LiveOptimizer(DEFAULT_CALIBRATION, **session)
    for i in range(n):
        live.push(keypoints=kp[i:i + 1], depth=depth[i:i + 1], rows=rows[i:i + 1])
    live.flush()
    own = live.result()
    live.close()
    assert np.array_equal(res["optimized"].view(np.uint64), own["optimized"].view(np.uint64))
    assert np.array_equal(res["estimated"].view(np.uint64), own["estimated"].view(np.uint64))
    with pytest.raises(ValueError, match="exactly one"):
        L.replay(traj, None, None, 100, 100 + n, DEFAULT_CALIBRATION, verbose=False, **session)
    np.savez(str(tmp_path / "bare.npz"), keypoints=kp)
    with pytest.raises(ValueError, match="depths are needed"):
        L.replay(traj, None, None, 100, 100 + n, DEFAULT_CALIBRATION, verbose=False, keypoints=str(tmp_path / "bare.npz"), first_id=100, **session)
