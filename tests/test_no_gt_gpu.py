"""Recordings without ground truth on the device: gem_sequence_quality against its numpy twin
(tests/quality_twin.py), `prepare` with a scale against `prepare` with the ground truth that gives that scale, and the
ground-truth-free route of the batch pipeline -- batched and per chunk, from a Recording and from its pickles, with `save_pose`."""
import os
import pickle

import numpy as np
import pytest

from globalegomocap_amd.camera import DEFAULT_CALIBRATION

pytestmark = pytest.mark.gpu

RESPONSE_TOL = dict(rtol=5e-5, atol=1e-7)          # column 0: what tests/test_hip_parity.py holds the fp32 energy parts to against the same oracle functions
F64_RTOL = 1e-12                                   # columns 1-3: float64 on both sides, like the device error report
SEVEN = ["estimated_heatmap_response", "optimized_heatmap_response", "estimated_bone_length_rms", "optimized_bone_length_rms",
         "estimated_acceleration", "optimized_acceleration", "optimized_displacement"]


@pytest.fixture(scope="module")
def P():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import prepare
    return prepare


def _engine(P):
    return P._lift_engine(DEFAULT_CALIBRATION, 0)


def _check_against_twin(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    for c, name in enumerate(("heatmap_response", "bone_length_rms", "acceleration", "displacement")):
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(got[..., c] - want[..., c]) / np.abs(want[..., c])
        print("%s %s: device %s twin %s relative difference %s" % (what, name, got[..., c].tolist(), want[..., c].tolist(), rel.tolist()))
    np.testing.assert_allclose(got[..., 0], want[..., 0], **RESPONSE_TOL)
    np.testing.assert_allclose(got[..., 1:], want[..., 1:], rtol=F64_RTOL, atol=0, equal_nan=True)


@pytest.mark.parametrize("n_chunks", [1, 3])
def test_kernel_against_the_twin(P, n_chunks, capsys):
    """Synthetic chunks (Gaussian heat-maps at the projected joints, jittered cameras with rotations), a merged sequence shorter than
    its chunk, frames shifted sideways until their joints leave the heat-maps (zero padding), a second sequence as `ref`."""
    import torch
    from globalegomocap_amd import synth
    from helpers import oracle_camera
    from oracle import np_oracle as O
    from quality_twin import sequence_quality, camera_points
    eng = _engine(P)
    dev = eng.device
    size, fpc = 26, 24
    rng = np.random.default_rng(17 + n_chunks)
    seqs = [synth.make_sequence(n_frames=size, seed=40 + k, cam_jitter=(2.0, 0.01)) for k in range(n_chunks)]
    cams = np.concatenate([np.asarray(s["camera_pose_list"]) for s in seqs])
    heat = np.concatenate([np.asarray(s["heatmap_list"], dtype=np.float32) for s in seqs])
    local = np.concatenate([np.asarray(s["estimated_local_skeleton"]) for s in seqs])
    frame0 = np.arange(n_chunks, dtype=np.int64) * size
    frames = (frame0[:, None] + np.arange(fpc)[None]).reshape(-1)
    in_cam = local[frames].copy()
    in_cam[3::7] += np.array([1.5, 0.0, -2.0])                              # sideways and behind the image plane, in the camera's frame: off the maps
    in_cam[5::7] += np.array([0.8, 0.0, -1.1])                              # ... and some joints off them, some across their right edge
    seq = np.einsum("nij,nkj->nki", cams[frames][:, :3, :3], in_cam) + cams[frames][:, None, :3, 3]
    ref = seq + rng.normal(0.0, 0.01, seq.shape)
    # what the kernel will see: every joint off the optical axis, some inside the maps and some outside
    pts = camera_points(seq, cams[frames])
    assert (np.linalg.norm(pts[..., :2], axis=-1) > 1e-3).all()
    cam = oracle_camera()
    ix, iy = O.heat_coords(O.fisheye_project(cam, pts.astype(np.float32).reshape(-1, 3)), 64, 64)
    outside = (ix < -1) | (ix > 64) | (iy < -1) | (iy > 64)
    edge = (ix > 63) & (ix < 64)                                            # (two of the four texels are padding)
    assert outside.sum() >= 3 * 15 and edge.sum() >= 1 and (~outside).sum() >= 10 * 15 * n_chunks
    mb = torch.stack([eng.mean_bone_length(local[k * size:(k + 1) * size].astype(np.float32)) for k in range(n_chunks)])
    seq_d, ref_d = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (seq, ref))
    cams_d, heat_d, frame0_d = torch.from_numpy(cams).to(dev), torch.from_numpy(heat).to(dev), torch.from_numpy(frame0).to(dev)
    got = eng.sequence_quality(seq_d, cams_d, heat_d, frame0_d, mb, n_chunks, ref=ref_d)
    again = eng.sequence_quality(seq_d, cams_d, heat_d, frame0_d, mb, n_chunks, ref=ref_d)
    bare = eng.sequence_quality(seq_d, cams_d, heat_d, frame0_d, mb, n_chunks)
    assert got.dtype == torch.float64 and tuple(got.shape) == (n_chunks, 4) and got.is_cuda
    got, again, bare = got.cpu().numpy(), again.cpu().numpy(), bare.cpu().numpy()
    assert eng.QUALITY_KEYS == ("heatmap_response", "bone_length_rms", "acceleration", "displacement")
    want = sequence_quality(seq, cams, heat, frame0, mb.cpu().numpy(), n_chunks, cam, ref=ref)
    with capsys.disabled():
        _check_against_twin(got, want, "kernel (%d chunks)" % n_chunks)
    assert np.isfinite(got).all() and (got[:, 0] > 0.05).all()              # (the joints that stayed inside do see their Gaussians)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))       # no floating-point atomics: the same bits
    assert np.isnan(bare[:, 3]).all() and np.array_equal(bare[:, :3].view(np.uint64), got[:, :3].view(np.uint64))
    # every chunk's row is the row it gets on its own
    for k in range(n_chunks):
        own = eng.sequence_quality(seq_d[k * fpc:(k + 1) * fpc].contiguous(), cams_d, heat_d, frame0_d[k:k + 1].contiguous(),
                                   mb[k:k + 1].contiguous(), 1, ref=ref_d[k * fpc:(k + 1) * fpc].contiguous()).cpu().numpy()
        assert np.array_equal(own[0].view(np.uint64), got[k].view(np.uint64)), k


def _write_recording(root, n, seed):
    from globalegomocap_amd import synth_recording as S
    par = S.random_parameters(n, seed=seed)
    heat64 = S.paraboloid_heatmaps(par["centres"], par["radii"])
    names = ["f_%d.mat" % k for k in range(n)]
    return S.write_recording(str(root), heat64, par["depth"], names, np.arange(n) % 7 == 3, np.arange(n) % 5 == 1, par["rows"], par["gt"])


def test_the_scale_route_is_the_ground_truth_route_at_its_scale(P, tmp_path, capsys):
    """One chunk prepared with its ground truth, its Umeyama scale recomputed here as `slam.camera_pose_list_from_heads` computes it,
    and the chunk prepared again with that scale: the same bits everywhere, no ground truth, no "initial mpjpe" line."""
    import torch
    from globalegomocap_amd import slam
    from globalegomocap_amd.errors import umeyama
    n, fps = 30, 25
    hd, dd, traj, gtp = _write_recording(tmp_path / "rec", n, seed=29)
    (a, b), = [(0, n)]
    rec_gt = P.prepare_spans(traj, hd, dd, gtp, [(a, b)], fps, 0)
    g = rec_gt.chunks[0]
    assert rec_gt.origins is None and g.gt is not None
    with open(traj) as f:
        rows = slam.trajectory_rows(f.read())
    rt, rq = slam.relative_poses(*slam.parse_trajectory(rows, a, b, fps))
    slam_head = np.einsum("nij,nj->ni", slam.pose_matrix(rt, rq)[:, :3, :3], g.est_local[:, 0].cpu().numpy()) + rt
    c, _, _ = umeyama(slam_head, g.gt[:, 0].cpu().numpy())
    capsys.readouterr()
    rec = P.prepare_sequence(traj, hd, dd, None, a, b + 1, fps=fps, test_size=n, scale=c)
    printed = capsys.readouterr().out
    assert "running test sequence from 0 to %d" % n in printed and "initial mpjpe" not in printed
    assert len(rec) == 1 and rec.origins.shape == (1, 4, 4)
    s = rec.chunks[0]
    assert s.gt is None and s.gt_list is None and s.initial_mpjpe is None
    for name in ("cams", "est_local", "est_global", "heat"):
        x, y = getattr(s, name), getattr(g, name)
        assert x.is_cuda and x.dtype == y.dtype and torch.equal(x, y), name
    d = rec.chunk_dict(0)
    full = rec_gt.chunk_dict(0)
    assert list(d) == list(P.PICKLE_KEYS[1:]) and all(np.array_equal(x, y) for k in d for x, y in zip(d[k], full[k]))
    out_dir = str(tmp_path / "one")
    P.main(traj, hd, dd, None, a, b, out_dir, fps, scale=c)
    assert "initial mpjpe" not in capsys.readouterr().out
    with open(os.path.join(out_dir, "test_data.pkl"), "rb") as f:
        assert list(pickle.load(f)) == list(P.PICKLE_KEYS[1:])


SIZE, N_CHUNKS = 26, 3


@pytest.fixture(scope="module")
def optimised(P, golden, tmp_path_factory):
    """Three chunks of 26 frames (three windows each) prepared with a scale; the same chunks with a ground truth attached; both
    optimised from the same seed with the `lbfgs_tiny` VAEs, `save_pose` on."""
    import torch
    from globalegomocap_amd import whole_sequence as ws
    from helpers import sd_from_npz
    tmp = tmp_path_factory.mktemp("no_gt")
    n = SIZE * N_CHUNKS + 1
    hd, dd, traj, gtp = _write_recording(tmp / "rec", n, seed=23)
    rec_scale = P.prepare_sequence(traj, hd, dd, None, 0, n, fps=25, test_size=SIZE, verbose=False, scale=1.7)
    with_gt = P.prepare_sequence(traj, hd, dd, gtp, 0, n, fps=25, test_size=SIZE, verbose=False)
    assert len(rec_scale) == len(with_gt) == N_CHUNKS
    # the ground-truth route on the very same inputs: the scale route's chunks with the ground truth attached (`prepare --gt` fits a
    # scale per chunk, so its cameras are not these)
    rec_gt = P.Recording([P.RecordingChunk(c.start_frame, c.end_frame, c.heat, c.est_local, c.est_global, c.cams, g.gt, gt_list=g.gt_list)
                          for c, g in zip(rec_scale.chunks, with_gt.chunks)])
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False)
    torch.manual_seed(31)
    a = ws.optimize_recording(rec_gt, DEFAULT_CALIBRATION, save_pose=str(tmp / "poses_gt"), **kw)
    torch.manual_seed(31)
    b = ws.optimize_recording(rec_scale, DEFAULT_CALIBRATION, ground_truth=False, save_pose=str(tmp / "poses"), **kw)
    return dict(tmp=tmp, rec_scale=rec_scale, rec_gt=rec_gt, kw=kw, a=a, b=b)


def _same_report(x, y):
    assert list(x[0]) == list(y[0]) == SEVEN and len(x[1]) == len(y[1])
    for rx, ry in zip([x[0]] + x[1], [y[0]] + y[1]):
        assert list(rx) == list(ry) == SEVEN
        for k in SEVEN:
            assert np.array_equal(np.float64(rx[k]).view(np.uint64), np.float64(ry[k]).view(np.uint64)), k
    assert x[4] is None and y[4] is None
    for i in (2, 3):
        assert x[i].shape == y[i].shape and np.array_equal(x[i], y[i]), i


def test_optimising_without_ground_truth(P, optimised, capsys):
    import torch
    from globalegomocap_amd import whole_sequence as ws
    from helpers import oracle_camera
    from quality_twin import sequence_quality
    a, b, rec, kw = optimised["a"], optimised["b"], optimised["rec_scale"], optimised["kw"]
    # the same poses as the ground-truth route, bit for bit; no ground-truth sequence; the seven keys, finite
    for i in (2, 3):
        assert a[i].shape == b[i].shape == (N_CHUNKS * SIZE, 15, 3) and np.array_equal(a[i], b[i]), i
    assert a[4] is not None and b[4] is None
    assert list(b[0]) == SEVEN and len(b[1]) == N_CHUNKS and all(list(r) == SEVEN for r in b[1])
    assert all(isinstance(v, float) and np.isfinite(v) for r in [b[0]] + b[1] for v in r.values())
    for k in SEVEN:
        assert b[0][k] == float(np.mean(np.stack([[r[q] for q in SEVEN] for r in b[1]]), axis=0)[SEVEN.index(k)])
    # the report is the twin's on the returned sequences
    eng = P._lift_engine(DEFAULT_CALIBRATION, 0)
    cams = np.concatenate([c.cams.cpu().numpy() for c in rec.chunks])
    heat = np.concatenate([c.heat.cpu().numpy() for c in rec.chunks])
    mb = np.stack([eng.mean_bone_length(c.est_local.cpu().numpy().astype(np.float32)).cpu().numpy() for c in rec.chunks])
    frame0, cam = np.arange(N_CHUNKS) * SIZE, oracle_camera()
    q_est = sequence_quality(b[2], cams, heat, frame0, mb, N_CHUNKS, cam)
    q_opt = sequence_quality(b[3], cams, heat, frame0, mb, N_CHUNKS, cam, ref=b[2])
    got_est = np.array([[r["estimated_heatmap_response"], r["estimated_bone_length_rms"], r["estimated_acceleration"], np.nan] for r in b[1]])
    got_opt = np.array([[r["optimized_heatmap_response"], r["optimized_bone_length_rms"], r["optimized_acceleration"], r["optimized_displacement"]]
                        for r in b[1]])
    with capsys.disabled():
        _check_against_twin(got_est, q_est, "optimize_recording, estimated")
        _check_against_twin(got_opt, q_opt, "optimize_recording, optimised")
    # the printed summary: one line per key
    torch.manual_seed(31)
    capsys.readouterr()
    again = ws.optimize_recording(rec, DEFAULT_CALIBRATION, ground_truth=False, **dict(kw, verbose=True))
    printed = capsys.readouterr().out
    _same_report(again, b)
    for (label, key) in [l for l in ws.QUALITY_LINES if l is not None]:
        assert "{}: {}".format(label, b[0][key]) in printed.splitlines()
    assert [l[1] for l in ws.QUALITY_LINES if l is not None] == SEVEN and "mpjpe" not in printed
    # the pickles written from it: the same poses and report; without ground_truth=False they are refused like any chunk without the key
    root = str(optimised["tmp"] / "chunks")
    rec.write_chunks(root)
    torch.manual_seed(31)
    _same_report(ws.optimize_directory(root, DEFAULT_CALIBRATION, ground_truth=False, **kw), b)
    with pytest.raises(KeyError, match="gt_global_skeleton"):
        ws.optimize_directory(root, DEFAULT_CALIBRATION, **kw)
    with pytest.raises(KeyError, match="gt_global_skeleton"):
        ws.optimize_recording(rec, DEFAULT_CALIBRATION, **kw)
    with pytest.raises(ValueError, match="device"):
        ws.optimize_recording(rec, DEFAULT_CALIBRATION, ground_truth=False, device_metrics=False, **kw)
    # a recording with ground truth may be asked for the report without it
    torch.manual_seed(31)
    _same_report(ws.optimize_recording(optimised["rec_gt"], DEFAULT_CALIBRATION, ground_truth=False, **kw), b)


def _synthetic_recording(P, lengths):
    import torch
    from globalegomocap_amd import synth
    chunks, at = [], 0
    for k, n in enumerate(lengths):
        s = synth.make_sequence(n_frames=n, seed=60 + k, cam_jitter=(1.0, 0.005))
        est, cams = np.asarray(s["estimated_local_skeleton"]), np.asarray(s["camera_pose_list"])
        heat = torch.from_numpy(np.asarray(s["heatmap_list"], dtype=np.float32)).to("cuda:0")
        chunks.append(P.RecordingChunk(at, at + n, heat, est, est, cams, None))
        at += n
    return P.Recording(chunks, np.tile(np.eye(4), (len(lengths), 1, 1)))


@pytest.mark.parametrize("lengths", [(26,) * 5, (26, 34, 26, 18, 42)], ids=["equal chunks", "unequal chunks"])
def test_pipelined_batches_give_the_results_of_one_batch(P, optimised, lengths):
    """Five chunks, one per device call: the frame-buffer slots are used again while the earlier batches' reports are read back.
    Equal chunks go through the batched report, unequal ones in one batch through the per-chunk one."""
    import torch
    from globalegomocap_amd import whole_sequence as ws
    from globalegomocap_amd.optimizer import SequenceOptimizer
    rec, kw = _synthetic_recording(P, lengths), dict(optimised["kw"])
    # (one optimiser for both runs, with room for all windows: the pipeline's own is sized by its first batch)
    kw["optimizer"] = SequenceOptimizer(DEFAULT_CALIBRATION, kw["global_vae_path"], kw["local_vae_path"], max_windows=32)
    torch.manual_seed(7)
    one = ws.optimize_recording(rec, DEFAULT_CALIBRATION, ground_truth=False, **kw)
    torch.manual_seed(7)
    piped = ws.optimize_recording(rec, DEFAULT_CALIBRATION, ground_truth=False, chunks_per_batch=1, **kw)
    assert len(one[1]) == 5 and one[3].shape == (sum(lengths), 15, 3)       # (every length here is 8 k + 2: all frames are merged frames)
    _same_report(piped, one)
    assert all(np.isfinite(v) for r in one[1] for v in r.values())


def test_save_pose(P, optimised):
    """`DIR/<chunk name>/result_pose.pkl` per chunk: the reference's keys and containers; no `gt_pose` without ground truth."""
    a, b, rec = optimised["a"], optimised["b"], optimised["rec_scale"]
    for sub, res, keys in (("poses", b, ["estimated_pose", "optimized_pose", "mid_optimized_pose"]),
                           ("poses_gt", a, ["estimated_pose", "optimized_pose", "mid_optimized_pose", "gt_pose"])):
        root = optimised["tmp"] / sub
        assert sorted(os.listdir(str(root))) == sorted(c.name for c in rec.chunks)
        for k, c in enumerate(rec.chunks):
            with open(str(root / c.name / "result_pose.pkl"), "rb") as f:
                d = pickle.load(f)
            assert list(d) == keys
            sl = slice(k * SIZE, (k + 1) * SIZE)
            assert isinstance(d["optimized_pose"], np.ndarray) and np.array_equal(d["optimized_pose"], res[3][sl])      # (smoothed: an array)
            for key in keys:
                if key != "optimized_pose":
                    assert isinstance(d[key], list) and len(d[key]) == SIZE and all(x.shape == (15, 3) and x.dtype == np.float64 for x in d[key])
            assert np.array_equal(np.asarray(d["estimated_pose"]), res[2][sl])
            if "gt_pose" in d:
                assert np.array_equal(np.asarray(d["gt_pose"]), res[4][sl])
    # both routes optimised the same poses through stage one as well
    for c in rec.chunks:
        with open(str(optimised["tmp"] / "poses" / c.name / "result_pose.pkl"), "rb") as f, \
                open(str(optimised["tmp"] / "poses_gt" / c.name / "result_pose.pkl"), "rb") as g:
            assert np.array_equal(np.asarray(pickle.load(f)["mid_optimized_pose"]), np.asarray(pickle.load(g)["mid_optimized_pose"]))
