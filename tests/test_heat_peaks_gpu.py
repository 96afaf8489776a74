"""Heat-maps without a depth network on the device: gem_heatmap_peaks against its numpy twin
(tests/heat_peaks_twin.py), its generic path, determinism, batch independence and guards, and the routes built on it end to end --
`prepare_spans(depth="bones")` from heat-map files alone, `peaks="subpixel"` with depth files, `LiveOptimizer.push(heat=,
depth="bones")`, and the optimiser on a recording that never had a depth.

THE GATE on (u, v): 16 times the largest spread between the float64 twin and the same twin in np.longdouble over these very cases,
floor 1e-12 px (`heat_peaks_twin.device_cases`; tests/test_heat_peaks_cpu.py holds it to what float64 allows).  Measured on the CPU:
largest spread 4.21e-13 px, so the gate is 6.74e-12 px -- u reaches 1152 px, whose unit in the last place is 2.3e-13 px.  No joint is
left out.  `arg`, the unusable mask and the confidence are exact."""
import ctypes as C
import os

import numpy as np
import pytest

import bone_depth_twin as BT
import heat_peaks_twin as HT
import keypoints_twin as KT
from globalegomocap_amd.camera import DEFAULT_CALIBRATION, FisheyeCamera

pytestmark = pytest.mark.gpu

H, W, J = HT.H, HT.W, HT.J


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


@pytest.fixture(scope="module")
def twin(cam):
    return HT.device_cases(cam)


@pytest.fixture(scope="module")
def bone_gate(cam, opts):
    return HT.bone_gate(cam, opts)


def _bits(t):
    return t.cpu().numpy().view(np.uint64 if t.element_size() == 8 else np.uint32)


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("n", HT.CASE_SIZES)
def test_device_against_the_twin(E, twin, n, capsys):
    import torch
    t, gate = twin[n], twin["gate"]
    kp, arg = E.heatmap_peaks(t["heat"])
    assert kp.dtype == torch.float64 and arg.dtype == torch.int32 and kp.is_cuda and tuple(kp.shape) == (n, J, 3) and tuple(arg.shape) == (n, J)
    kp, arg = kp.cpu().numpy(), arg.cpu().numpy()
    assert np.array_equal(arg, t["arg"]) and np.array_equal(arg, np.argmax(t["heat"].reshape(n, H * W, J), axis=1))
    usable = t["kp"][..., 2] > 0
    assert np.array_equal(kp[..., 2] > 0, usable) and not kp[~usable].any()
    assert np.array_equal(kp[..., 2].view(np.uint64), t["kp"][..., 2].view(np.uint64))          # the confidence: exact
    diff = np.abs(kp[..., :2] - t["kp"][..., :2]).max(axis=-1)
    with capsys.disabled():
        print("%d frames, %d of %d joints usable: (u, v) differ from the twin by at most %.3g px (gate %.3g px); %d of %d coordinates are the "
              "twin's bits" % (n, usable.sum(), usable.size, diff.max(), gate, (kp[..., :2] == t["kp"][..., :2]).sum(), 2 * usable.size))
    assert np.isfinite(kp).all() and diff.max() <= gate


def test_generic_path_same_bytes(E, twin):
    """A view whose data pointer is 4-byte but not 16-byte aligned takes the scalar scan: the same bytes."""
    import torch
    heat = torch.from_numpy(twin[67]["heat"]).to(E.device)
    flat = torch.empty(heat.numel() + 8, dtype=torch.float32, device=E.device)
    for shift in (1, 2, 3):
        view = flat[shift:shift + heat.numel()].view(heat.shape)
        view.copy_(heat)
        assert view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
        a, b = E.heatmap_peaks(heat), E.heatmap_peaks(view)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])


def test_round_trip_through_the_splat(E, cam, capsys):
    """gem_keypoint_heatmaps(kp, 1.5) then gem_heatmap_peaks returns kp within 0.1 px."""
    kp = BT.detect(BT.poses(67, 0.3, np.random.default_rng(5)), cam, conf=0.8)
    back, _ = E.heatmap_peaks(E.keypoint_heatmaps(kp, 1.5))
    back = back.cpu().numpy()
    err = HT.pixel_error(back, kp)
    with capsys.disabled():
        print("round trip through the splat (sigma 1.5): mean %.4f px, max %.4f px" % (err.mean(), err.max()))
    assert err.max() <= 0.1
    peak = KT.splat(kp, H, W, 1.5).reshape(67, H * W, J).max(axis=1)
    assert np.array_equal(back[..., 2], peak.astype(np.float64))


def _call(E, heat_d, n, kp, arg, upscale=16, pad_x=128, pad_y=0, min_peak=0.0, handle=True):
    import torch
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)          # noqa: E731
    rc = E.lib.gem_heatmap_peaks(E._h if handle else C.c_void_p(0), p(heat_d), n, upscale, pad_x, pad_y, min_peak, p(kp), p(arg),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, E.lib.gem_last_error().decode()


def test_same_bytes_twice_alone_bounds_and_guards(E, twin):
    import torch
    n = 67
    heat = torch.from_numpy(twin[n]["heat"]).to(E.device)
    full, again = E.heatmap_peaks(heat), E.heatmap_peaks(heat)
    assert np.array_equal(_bits(full[0]), _bits(again[0])) and torch.equal(full[1], again[1])
    for lo, hi in ((10, 20), (66, 67)):          # a frame's bytes do not depend on the frames that share its call
        part = E.heatmap_peaks(heat[lo:hi])
        assert np.array_equal(_bits(full[0][lo:hi]), _bits(part[0])) and torch.equal(full[1][lo:hi], part[1])
    # canaries round both outputs
    bufs = [torch.full((n * J * 3 + 128,), -7.0, dtype=torch.float64, device=E.device), torch.full((n * J + 128,), -7, dtype=torch.int32, device=E.device)]
    views = (bufs[0][64:64 + n * J * 3].view(n, J, 3), bufs[1][64:64 + n * J].view(n, J))
    got = E.heatmap_peaks(heat, out=views)
    assert all(g is v for g, v in zip(got, views)) and np.array_equal(_bits(got[0]), _bits(full[0])) and torch.equal(got[1], full[1])
    for b, size in zip(bufs, (n * J * 3, n * J)):
        assert (b[:64] == -7).all() and (b[64 + size:] == -7).all()
    # each output may be NULL, not both
    kp_only, arg_only = torch.zeros_like(full[0]), torch.zeros_like(full[1])
    assert _call(E, heat, n, kp_only, None)[0] == 0 and _call(E, heat, n, None, arg_only)[0] == 0
    assert np.array_equal(_bits(kp_only), _bits(full[0])) and torch.equal(arg_only, full[1])
    # refusals: nothing is launched, so nothing is written
    outs = [torch.full_like(full[0], 3), torch.full_like(full[1], 3)]
    refused = [_call(E, heat, n, None, None), _call(E, heat, n, *outs, handle=False), _call(E, heat, -1, *outs), _call(E, heat, 1 << 27, *outs),
               _call(E, heat, n, *outs, upscale=0), _call(E, heat, n, *outs, pad_x=-1), _call(E, heat, n, *outs, pad_y=-1),
               _call(E, heat, n, *outs, min_peak=-0.1), _call(E, heat, n, *outs, min_peak=float("nan")), _call(E, heat, n, *outs, min_peak=float("inf")),
               _call(E, None, n, *outs), _call(E, None, 0, None, None)]
    torch.cuda.synchronize()
    assert all(rc == 1 and msg.startswith("gem_heatmap_peaks: ") for rc, msg in refused), refused
    assert all((o == 3).all() for o in outs)
    assert _call(E, None, 0, *outs)[0] == 0 and all((o == 3).all() for o in outs)          # no frames: nothing to do
    with pytest.raises(ValueError):
        E.heatmap_peaks(heat[:, :32])
    with pytest.raises(ValueError, match="min_peak"):
        E.heatmap_peaks(heat, min_peak=-1.0)
    with pytest.raises(TypeError):
        E.heatmap_peaks(heat, out=(full[0].float(), None))
    with pytest.raises(ValueError):
        E.heatmap_peaks(heat, out=(full[0][:5], None))
    # min_peak and the other map reach the kernel
    peak = HT.integer_stage(twin[n]["heat"])[1]
    cut = E.heatmap_peaks(heat, min_peak=0.75)[0].cpu().numpy()          # (a splat of confidence 0.8 peaks between 0.716 and 0.8)
    assert np.abs(cut - HT.peaks(twin[n]["heat"], min_peak=0.75)[0]).max() <= twin["gate"]
    assert np.array_equal(cut[..., 2] > 0, HT.usable_peak(peak, 0.75)) and 0 < (cut[..., 2] > 0).sum() < int((full[0][..., 2] > 0).sum())
    other = E.heatmap_peaks(heat, upscale=8, pad_x=3, pad_y=40)[0].cpu().numpy()
    assert np.abs(other - HT.peaks(twin[n]["heat"], 8, 3, 40)[0]).max() <= twin["gate"]


# ------------------------------------------------------------------------------------------------------------------ end to end, offline
N_FRAMES, TEST_SIZE = 40, 20          # two chunks


def _trajectory(path, n):
    with open(path, "w") as f:
        for i in range(n + 1):
            f.write("%.9f %.9f 0 0 0 0 0 1\n" % (i / 25.0, 0.004 * i))


def _write_maps(directory, heat, depth=None):
    """One `heatmap` .mat per frame under <directory>/heat and, with `depth`, one `depth` .mat under <directory>/depth."""
    import scipy.io as sio
    hd, dd = os.path.join(str(directory), "heat"), os.path.join(str(directory), "depth")
    os.makedirs(hd)
    for f in range(len(heat)):
        sio.savemat(os.path.join(hd, "f_%d.mat" % f), {"heatmap": heat[f]})
    if depth is None:
        return hd, None
    os.makedirs(dd)
    for f in range(len(depth)):
        sio.savemat(os.path.join(dd, "f_%d.mat" % f), {"depth": depth[f][None]})
    return hd, dd


@pytest.fixture(scope="module")
def offline(cam, tmp_path_factory):
    """40 frames in two chunks as heat-map files (sigma 1.5 splats of a generated motion, the left wrist's map blank for three frames)."""
    truth = BT.motion(N_FRAMES, 0.3, np.random.default_rng(34))
    kp = BT.detect(truth, cam, conf=0.9)
    heat = KT.splat(kp, H, W, 1.5)
    heat[5:8, :, :, 6] = 0.0
    root = tmp_path_factory.mktemp("heat_only")
    hd, _ = _write_maps(root, heat)
    traj = str(root / "traj.txt")
    _trajectory(traj, N_FRAMES)
    return dict(truth=truth, kp=kp, heat=heat, heat_dir=hd, traj=traj, root=root, peaks=HT.peaks(heat)[0])


def test_offline_route_from_heat_maps_alone(E, offline, cam, opts, bone_gate, capsys):
    import torch
    from globalegomocap_amd import bone_depth as B, detections as D, prepare as P
    o = offline
    spans = P.chunk_spans(0, N_FRAMES + 1, TEST_SIZE)
    assert spans == [(0, 20), (20, 40)] and sorted(os.listdir(str(o["root"]))) == ["heat", "traj.txt"]          # no depth directory anywhere
    d, s, rms = BT.solve(o["peaks"], cam, opts)
    dl, _, rl = BT.solve(o["peaks"], cam, opts, np.longdouble)
    assert max(np.abs(d - dl).max(), np.abs(rms - rl).max()) <= BT.ILL_CONDITIONED          # (no ill-conditioned frame: a filled frame reads its neighbours)
    rec = P.prepare_spans(o["traj"], o["heat_dir"], None, None, spans, 25, 0, scale=1.0, depth="bones")
    ref = D.recording_from_detections(o["traj"], o["peaks"], scale=1.0, spans=spans, depth="bones")
    assert isinstance(rec.depth_report, B.BoneDepthReport)
    rep, want = rec.depth_report.as_dict(), ref.depth_report.as_dict()
    assert (rep["frames"], rep["solved"], rep["unsolved"], rep["frames_without_neck"]) == (40, 40 * 15 - 3, 3, 0)
    assert all(rep[k] == want[k] for k in ("frames", "solved", "unsolved", "frames_without_neck"))
    assert abs(rep["rms_max"] - want["rms_max"]) <= bone_gate and abs(rep["rms_median"] - want["rms_median"]) <= bone_gate
    worst = 0.0
    for k, (a, b) in enumerate(zip(rec.chunks, ref.chunks)):
        worst = max(worst, float((a.est_local - b.est_local).abs().max()))
        assert torch.equal(a.cams, b.cams)
        # the network's own maps, bit for bit -- not splats of the peaks
        assert np.array_equal(a.heat.cpu().numpy().view(np.uint32), o["heat"][20 * k:20 * k + 20].view(np.uint32)) and a.heat_files is None
        assert not torch.equal(a.heat, b.heat)
    assert np.array_equal(rec.origins, ref.origins)
    with capsys.disabled():
        print("heat-maps alone: est_local against the detection route fed the twin's peaks: at most %.3g m (section 6q's gate %.3g m)" % (worst, bone_gate))
    assert worst <= bone_gate
    # the pickles never held depths: they are written as ever
    dirs = rec.write_chunks(str(o["root"] / "out"))
    assert [os.path.basename(x) for x in dirs] == ["data_start_0_end_20", "data_start_20_end_40"]
    # a joint the solve cannot reach in a whole chunk: the detection route's refusal
    import scipy.io as sio
    cut = os.path.join(str(o["root"]), "cut")
    os.makedirs(cut)
    blank = o["heat"].copy()
    blank[20:, :, :, 2] = 0.0
    for f in range(N_FRAMES):
        sio.savemat(os.path.join(cut, "f_%d.mat" % f), {"heatmap": blank[f]})
    with pytest.raises(ValueError, match=r"joints \[2, 3\] have no usable detection in the chunk \[20, 40\)"):
        P.prepare_spans(o["traj"], cut, None, None, spans, 25, 0, scale=1.0, depth="bones")
    # min_peak reaches the kernel: above every peak nothing is left
    with pytest.raises(ValueError, match="have no usable detection"):
        P.prepare_spans(o["traj"], o["heat_dir"], None, None, spans, 25, 0, scale=1.0, depth="bones", min_peak=0.95)


def test_subpixel_lift_with_the_networks_depths(E, offline, tmp_path):
    """peaks="subpixel" with depth files: est_local is lift_keypoints(twin peaks, file depths), filled per chunk."""
    import torch
    from globalegomocap_amd import prepare as P
    o = offline
    depth = np.linalg.norm(o["truth"], axis=-1)
    hd, dd = _write_maps(tmp_path, o["heat"], depth)
    spans = P.chunk_spans(0, N_FRAMES + 1, TEST_SIZE)
    rec = P.prepare_spans(o["traj"], hd, dd, None, spans, 25, 0, scale=1.0, peaks="subpixel")
    old = P.prepare_spans(o["traj"], hd, dd, None, spans, 25, 0, scale=1.0)
    assert rec.depth_report is None and old.depth_report is None
    want, _, valid = E.lift_keypoints(o["peaks"], depth)
    E.fill_missing(want, valid, 2)
    got = torch.cat(rec.est_local).cpu().numpy()
    np.testing.assert_allclose(got, want.cpu().numpy(), rtol=1e-12, atol=1e-15)
    sub = np.linalg.norm(got - o["truth"], axis=-1).mean()
    arg = np.linalg.norm(torch.cat(old.est_local).cpu().numpy() - o["truth"], axis=-1).mean()
    assert sub < 0.25 * arg          # (the 16-pixel grid against the sub-pixel peak, both with the true depths)
    assert all(torch.equal(a.heat, b.heat) and torch.equal(a.cams, b.cams) for a, b in zip(rec.chunks, old.chunks))


# ------------------------------------------------------------------------------------------------------------------ end to end, live
def test_live_route_from_heat_maps_alone(E, cam, tmp_path):
    """26 frames pushed in pieces of 1, 5, 8 and 12 with depth="bones": the pose ring holds, bit for bit, what the offline steps lift
    for those frames; a joint whose map is blank holds its last lift; a first frame with a blank map is refused."""
    import torch
    from helpers import TINY
    from globalegomocap_amd import live as L, slam, vae as vae_schema
    n, pieces = 26, (1, 5, 8, 12)
    kp = BT.detect(BT.motion(n, 0.3, np.random.default_rng(45)), cam, conf=0.7)
    heat = KT.splat(kp, H, W, 1.5)
    heat[9:12, :, :, 3] = 0.0                          # a wrist's map blank for three frames
    traj = str(tmp_path / "traj.txt")
    _trajectory(traj, n)
    with open(traj) as f:
        rows = slam.trajectory_rows(f.read())[:n]
    sd_l, sd_g = vae_schema.synthetic_state_dict(TINY, 11), vae_schema.synthetic_state_dict(TINY, 12)
    eps = np.random.default_rng(6).normal(size=(3, 2, TINY.latent_dim)).astype(np.float32)
    session = dict(global_vae=sd_g, local_vae=sd_l, eps=lambda w: eps[w], scale=1.0)
    live = L.LiveOptimizer(DEFAULT_CALIBRATION, **session)
    blank_first = heat[:1].copy()
    blank_first[0, :, :, 5] = 0.0
    with pytest.raises(ValueError, match=r"joints \[5, 6\] of the session's first frame have no usable detection"):
        live.push(heat=blank_first, depth="bones", rows=rows[:1])
    assert live.n_pushed == 0
    at = 0
    for k in pieces:
        live.push(heat=heat[at:at + k], depth="bones", rows=rows[at:at + k])
        at += k
    ring = live._bufs["ring_pose"][:n].cpu().numpy()
    ring_heat = live._bufs["ring_heat"][:n].cpu().numpy()
    live.flush()
    own = live.result()
    live.close()
    assert own["optimized"].shape == (n, 15, 3) and np.isfinite(own["optimized"]).all()
    kp_d, _ = E.heatmap_peaks(heat)
    depth, solved, _ = E.bone_depths(kp_d)
    kp_d[..., 2] = torch.where(solved.bool(), kp_d[..., 2], torch.zeros_like(kp_d[..., 2]))
    lifted = E.lift_keypoints(kp_d, depth)[1].cpu().numpy()
    seen = solved.cpu().numpy().astype(bool)
    assert (~seen).sum() == 3 and np.array_equal(ring[seen].view(np.uint32), lifted[seen].view(np.uint32))
    assert np.array_equal(ring[9:12, 3], np.broadcast_to(ring[8, 3], (3, 3)))
    assert np.array_equal(ring_heat.view(np.uint32), heat.view(np.uint32))          # the caller's own maps
    # `replay` from a heat-map directory alone is that session
    hd, _ = _write_maps(tmp_path, heat)
    res, log = L.replay(traj, hd, None, 0, n, DEFAULT_CALIBRATION, verbose=False, depth_from="bones", **session)
    assert res["dropped"] == 0 and len(log) == 3
    assert np.array_equal(res["optimized"].view(np.uint64), own["optimized"].view(np.uint64))
    assert np.array_equal(res["estimated"].view(np.uint64), own["estimated"].view(np.uint64))
    with pytest.raises(ValueError, match="depths are needed"):
        L.replay(traj, hd, None, 0, n, DEFAULT_CALIBRATION, verbose=False, **session)


# ------------------------------------------------------------------------------------------------------------------ end to end, optimised
def test_optimised_from_heat_maps_alone(E, cam, golden, tmp_path, capsys):
    """18 frames (two windows) optimised from heat-maps alone, beside the same recording optimised with the true depths.  Recorded, not
    gated."""
    import torch
    from helpers import sd_from_npz
    from globalegomocap_amd import prepare as P, whole_sequence as ws
    n = 18
    truth = BT.motion(n, 0.3, np.random.default_rng(52))
    heat = KT.splat(BT.detect(truth, cam, conf=0.9), H, W, 1.5)
    hd, dd = _write_maps(tmp_path, heat, np.linalg.norm(truth, axis=-1))
    traj = str(tmp_path / "traj.txt")
    _trajectory(traj, n)
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False)
    out = {}
    for name, args in (("bones", dict(depth_dir=None, depth="bones")), ("true depths, sub-pixel", dict(depth_dir=dd, peaks="subpixel")),
                       ("true depths, argmax", dict(depth_dir=dd))):
        rec = P.prepare_spans(traj, hd, args.pop("depth_dir"), None, [(0, n)], 25, 0, scale=1.0, **args)
        torch.manual_seed(5)
        out[name] = (ws.optimize_recording(rec, DEFAULT_CALIBRATION, ground_truth=False, **kw)[3], rec.chunks[0].est_local.cpu().numpy())
    a = out["bones"][0]
    assert a.shape == (n, 15, 3) and np.isfinite(a).all()
    mm = lambda x, y: float(np.linalg.norm(x - y, axis=-1).mean()) * 1e3          # noqa: E731
    with capsys.disabled():
        print("heat-maps alone: the lift lies %.2f mm (MPJPE) from the truth (with the true depths: sub-pixel %.2f mm, argmax %.2f mm); "
              "optimised, %.2f mm from the recording optimised with the true depths at the sub-pixel peaks, %.2f mm from the one at the argmax"
              % (mm(out["bones"][1], truth), mm(out["true depths, sub-pixel"][1], truth), mm(out["true depths, argmax"][1], truth),
                 mm(a, out["true depths, sub-pixel"][0]), mm(a, out["true depths, argmax"][0])))


# ------------------------------------------------------------------------------------------------------------------ the command lines
def test_command_lines_from_heat_maps_alone(E, cam, tmp_path, capsys):
    """`slam_scale --heatmaps DIR --depth_from bones` and `prepare --heatmaps DIR --depth_from bones --scale auto --out DIR` on a walking
    wearer whose recording has no depth files: the scale the command prints is the one `prepare` then uses, and the chunks are written.
    How far it lies from the walker's true scale is recorded, not gated (the walker's leg bones are not of constant length)."""
    import pickle
    from globalegomocap_amd import prepare as P, slam_scale as S, synth_walk as SW
    n, size, scale = 78, 26, 0.6
    w = SW.walk(n, scale=scale)
    uv = cam.project_numpy(w["local"].reshape(-1, 3)).reshape(n, 15, 2)
    heat = KT.splat(np.concatenate([uv, np.full((n, 15, 1), 0.9)], axis=2), H, W, 1.5)
    hd, _ = _write_maps(tmp_path, heat)
    traj = str(tmp_path / "traj.txt")
    np.savetxt(traj, w["rows"], fmt="%.9f")
    capsys.readouterr()
    est = S._cli(["--slam", traj, "--heatmaps", hd, "--depth_from", "bones", "--start", "0", "--end", str(n), "--test_size", str(size), "--min_pairs", "10"])
    printed = capsys.readouterr().out
    assert "depths from bone lengths" not in printed and printed.startswith("SLAM scale estimate: ") and "chunk 2 [52, 78)" in printed
    rec = P.prepare_sequence(traj, hd, None, None, 0, n + 1, test_size=size, scale="auto", min_pairs=10, verbose=False, depth="bones",
                             out_root=str(tmp_path / "out"))
    assert rec.scale == est.scale and rec.depth_report.frames == n and rec.depth_report.unsolved == 0 and len(rec) == 3
    with open(os.path.join(str(tmp_path / "out"), "data_start_26_end_52", "test_data.pkl"), "rb") as f:
        d = pickle.load(f)
    assert list(d) == list(P.PICKLE_KEYS[1:]) and np.array_equal(np.stack(d["heatmap_list"]).view(np.uint32), heat[26:52].view(np.uint32))
    with capsys.disabled():
        print("walker without depth files: SLAM scale estimate %.4f (true %.4f); bone residual rms median %.1f mm"
              % (est.scale, scale, rec.depth_report.rms_median * 1e3))
    # the command line of `prepare` itself, to the pickles
    P._cli(["--slam", traj, "--heatmaps", hd, "--depth_from", "bones", "--scale", "%r" % est.scale, "--start", "0", "--end", str(n + 1),
            "--test_size", str(size), "--out", str(tmp_path / "cli")])
    printed = capsys.readouterr().out
    assert printed.startswith("depths from bone lengths: 78 frames, 1170 of 1170 joints solved")
    assert sorted(os.listdir(str(tmp_path / "cli"))) == ["data_start_0_end_26", "data_start_26_end_52", "data_start_52_end_78"]
