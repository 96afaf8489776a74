"""2-D joint detections on the host: the file reader, the frame-id selection, the twins' interpolation against
np.interp, `check_push` with `keypoints=`, where the twin's splat peaks."""
import os
import re

import numpy as np
import pytest

import keypoints_twin as KT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kp(n, seed=0, cols=3):
    rng = np.random.default_rng(seed)
    kp = np.concatenate([rng.uniform(200, 1000, (n, 15, 2)), rng.uniform(0.2, 1.0, (n, 15, 1))], axis=2)
    return kp[..., :cols]


def test_read_detections_accepts_the_documented_files(tmp_path):
    from globalegomocap_amd import detections as D
    kp3, kp2 = _kp(6), _kp(6, cols=2)
    np.save(tmp_path / "a.npy", kp3)
    d = D.read_detections(str(tmp_path / "a.npy"))
    assert d["keypoints"].dtype == np.float64 and np.array_equal(d["keypoints"], kp3) and d["depth"] is None
    assert np.array_equal(d["frame_ids"], np.arange(6))
    np.save(tmp_path / "b.npy", kp2.astype(np.float32))
    d = D.read_detections(str(tmp_path / "b.npy"), first_id=40)
    assert d["keypoints"].shape == (6, 15, 3) and np.array_equal(d["keypoints"][..., :2], kp2.astype(np.float32)) and (d["keypoints"][..., 2] == 1).all()
    assert np.array_equal(d["frame_ids"], np.arange(40, 46))
    depth, ids = np.random.default_rng(1).uniform(0.2, 1.5, (6, 15)), np.array([9, 3, 4, 5, 6, 7])
    np.savez(tmp_path / "c.npz", keypoints=kp3, depth=depth, frame_ids=ids)
    d = D.read_detections(str(tmp_path / "c.npz"), first_id=40)
    assert np.array_equal(d["keypoints"], kp3) and np.array_equal(d["depth"], depth) and np.array_equal(d["frame_ids"], ids) and d["frame_ids"].dtype == np.int64
    np.savez(tmp_path / "d.npz", keypoints=kp2)
    d = D.read_detections(str(tmp_path / "d.npz"), first_id=2)
    assert d["depth"] is None and np.array_equal(d["frame_ids"], np.arange(2, 8)) and (d["keypoints"][..., 2] == 1).all()
    # rows are picked by frame id, in the span's order, wherever they stand in the file
    rows = D.span_rows(ids, [(3, 8), (9, 10)])
    assert [r.tolist() for r in rows] == [[1, 2, 3, 4, 5], [0]]


def test_read_detections_rejects_the_rest(tmp_path):
    from globalegomocap_amd import detections as D
    kp = _kp(6)
    bad = {"joints": kp[:, :14], "columns": np.concatenate([kp, kp[..., :1]], axis=2), "rank": kp[0], "text": np.array([["a"] * 15] * 6)}
    for name, arr in bad.items():
        np.save(tmp_path / (name + ".npy"), arr)
        with pytest.raises(ValueError):
            D.read_detections(str(tmp_path / (name + ".npy")))
    obj = np.empty((6, 15, 3), dtype=object)
    obj[:] = kp
    np.save(tmp_path / "object.npy", obj, allow_pickle=True)
    with pytest.raises(ValueError):                                   # (np.load(allow_pickle=False) refuses it)
        D.read_detections(str(tmp_path / "object.npy"))
    np.savez(tmp_path / "object.npz", keypoints=obj)
    with pytest.raises(ValueError):
        D.read_detections(str(tmp_path / "object.npz"))
    np.savez(tmp_path / "nokey.npz", points=kp)
    with pytest.raises(ValueError, match="keypoints"):
        D.read_detections(str(tmp_path / "nokey.npz"))
    np.savez(tmp_path / "depth.npz", keypoints=kp, depth=np.ones((6, 14)))
    with pytest.raises(ValueError, match="depth"):
        D.read_detections(str(tmp_path / "depth.npz"))
    np.savez(tmp_path / "dup.npz", keypoints=kp, frame_ids=np.array([0, 1, 2, 2, 4, 5]))
    with pytest.raises(ValueError, match=r"\[2\] appear more than once"):
        D.read_detections(str(tmp_path / "dup.npz"))
    np.savez(tmp_path / "float_ids.npz", keypoints=kp, frame_ids=np.arange(6.0))
    with pytest.raises(ValueError, match="frame_ids"):
        D.read_detections(str(tmp_path / "float_ids.npz"))
    np.savez(tmp_path / "short_ids.npz", keypoints=kp, frame_ids=np.arange(5))
    with pytest.raises(ValueError, match="frame_ids"):
        D.read_detections(str(tmp_path / "short_ids.npz"))
    # a gap inside a span: named; outside every span it does not matter
    np.savez(tmp_path / "gap.npz", keypoints=kp, frame_ids=np.array([0, 1, 2, 4, 5, 6]))
    ids = D.read_detections(str(tmp_path / "gap.npz"))["frame_ids"]
    with pytest.raises(ValueError, match=r"no row for frame ids \[3\] of \[0, 7\)"):
        D.span_rows(ids, [(0, 7)])
    assert [r.tolist() for r in D.span_rows(ids, [(0, 3), (4, 7)])] == [[0, 1, 2], [3, 4, 5]]


def test_recording_arguments_are_checked_before_any_device_work(tmp_path):
    from globalegomocap_amd import detections as D
    with pytest.raises(ValueError, match="exactly one"):
        D.recording_from_detections("traj.txt", _kp(4), spans=[(0, 4)])
    with pytest.raises(ValueError, match="exactly one"):
        D.recording_from_detections("traj.txt", _kp(4), gt_path="gt.pkl", scale=1.0, spans=[(0, 4)])
    # a joint with no usable detection in a chunk
    kp = _kp(14)
    kp[7:, 3, 2] = 0.0
    kp[:7, 5, 0] = np.nan
    D.check_chunks_have_every_joint(kp, [(0, 14)], [(0, 14)])
    with pytest.raises(ValueError, match=r"joints \[5\] have no usable detection in the chunk \[0, 7\)"):
        D.check_chunks_have_every_joint(kp, [(0, 7), (7, 14)], [(0, 7), (7, 14)])
    assert np.array_equal(D.usable(kp), KT.usable(kp))
    p = D._parser().parse_args(["--slam", "t", "--keypoints", "k.npz", "--scale", "1.0", "--start", "0", "--end", "101"])
    assert (p.sigma, p.first_id, p.test_size, p.fps, p.depth, p.depths, p.out, p.optimize) == (1.5, 0, 100, 25, None, None, None, False)
    with pytest.raises(SystemExit):
        D._parser().parse_args(["--slam", "t", "--keypoints", "k.npz", "--start", "0", "--end", "101"])          # neither --gt nor --scale
    with pytest.raises(SystemExit):
        D._parser().parse_args(["--slam", "t", "--keypoints", "k", "--scale", "1", "--start", "0", "--end", "9", "--depth", "a", "--depths", "b"])


def test_twin_interpolation_is_np_interp():
    """The hand-made validity pattern: leading gap, inner gap, trailing gap, a single valid frame, nothing missing."""
    rng = np.random.default_rng(3)
    valid = KT.pattern_valid(1, 5)
    assert valid.shape == (7, 5) and valid[:, 3].sum() == 1 and valid[:, 4].all()
    assert not valid[0, 0] and not valid[-1, 2] and valid[0, 1] and valid[-1, 1] and not valid[2:5, 1].any()
    seq = rng.normal(size=(7, 5, 3))
    got = KT.fill_missing(seq, valid, 1)
    t = np.arange(7.0)
    for j in range(5):
        v = valid[:, j].astype(bool)
        for c in range(3):
            np.testing.assert_allclose(got[:, j, c], np.interp(t, t[v], seq[v, j, c]), rtol=0, atol=1e-15)
        assert np.array_equal(got[v, j], seq[v, j])
    assert np.array_equal(got[:, 3], np.broadcast_to(seq[3, 3], (7, 3)))          # a single valid frame: held everywhere
    # chunks are filled on their own: the second chunk's leading gap does not look into the first
    valid2 = KT.pattern_valid(2, 5)
    seq2 = rng.normal(size=(14, 5, 3))
    got2 = KT.fill_missing(seq2, valid2, 2)
    for k in range(2):
        assert np.array_equal(got2[7 * k:7 * k + 7], KT.fill_missing(seq2[7 * k:7 * k + 7], valid2[7 * k:7 * k + 7], 1))
    # a joint with no valid frame at all is left alone
    none = valid.copy()
    none[:, 0] = 0
    assert np.array_equal(KT.fill_missing(seq, none, 1)[:, 0], seq[:, 0])
    # the causal twin holds instead
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    kp = _kp(7, seed=5)[:, :5]
    kp[..., 2] = np.where(valid, kp[..., 2], 0.0)
    depth = rng.uniform(0.3, 1.2, (7, 5))
    prev = rng.normal(size=(5, 3))
    out, ok, held = KT.lift(kp, depth, cam, prev)
    free, _, none_held = KT.lift(kp, depth, cam)
    assert np.array_equal(ok, valid) and none_held is None
    assert np.array_equal(out[0, 0], prev[0]) and np.array_equal(out[2, 1], free[1, 1]) and np.array_equal(out[6, 2], free[3, 2])
    assert np.array_equal(held[3], free[3, 3]) and np.array_equal(free[0, 0], np.zeros(3))


def _frames(k):
    rng = np.random.default_rng(k)
    return dict(heat=np.zeros((k, 64, 64, 15), np.float32), depth=np.ones((k, 15)), est_local=rng.normal(size=(k, 15, 3)).astype(np.float32),
                cams=np.tile(np.eye(4), (k, 1, 1)), times=np.arange(k) / 25.0, keypoints=_kp(k))


def test_check_push_with_keypoints():
    import inspect
    from types import SimpleNamespace
    from globalegomocap_amd import live
    from globalegomocap_amd.live import LiveOptimizer
    f = _frames(3)
    assert list(inspect.signature(live.check_push).parameters)[-1] == "keypoints"
    k, t, rest = live.check_push(None, None, f["depth"], None, None, f["cams"], f["times"], (64, 64), f["keypoints"])
    assert k == 3 and np.array_equal(t, f["times"]) and rest[0] is None
    live.check_push(None, None, None, f["est_local"], None, f["cams"], f["times"], keypoints=f["keypoints"][..., :2])
    with pytest.raises(ValueError, match="exactly one of heat= .* and keypoints="):
        live.check_push(None, f["heat"], f["depth"], None, None, f["cams"], f["times"], (64, 64), f["keypoints"])
    with pytest.raises(ValueError, match=r"^push: heat= is needed$"):
        live.check_push(None, None, f["depth"], None, None, f["cams"], f["times"])
    for bad in (f["keypoints"][:, :14], f["keypoints"][0], f["keypoints"][:0], np.zeros((3, 15, 4)), f["keypoints"][:2]):
        with pytest.raises(ValueError):
            live.check_push(None, None, f["depth"], None, None, f["cams"], f["times"], (64, 64), bad)
    # the positional call of before still means what it meant
    assert live.check_push(None, f["heat"], None, f["est_local"], None, f["cams"], f["times"])[0] == 3
    # push itself: the same refusals before a device is touched, and a first frame that lacks a joint
    s = object.__new__(LiveOptimizer)
    s.engine, s._flushed, s._last_time, s.n_pushed = SimpleNamespace(heat_size=(64, 64)), False, None, 0
    with pytest.raises(ValueError, match="exactly one of heat="):
        s.push(heat=f["heat"], keypoints=f["keypoints"], depth=f["depth"], cams=f["cams"], times=f["times"])
    with pytest.raises(ValueError, match="heat= is needed"):
        s.push(depth=f["depth"], cams=f["cams"], times=f["times"])
    lost = f["keypoints"].copy()
    lost[0, 4, 2] = 0.0
    lost[0, 9, 1] = np.inf
    with pytest.raises(ValueError, match=r"joints \[4, 9\] of the session's first frame"):
        s.push(keypoints=lost, depth=f["depth"], cams=f["cams"], times=f["times"])
    p = live._parser().parse_args(["--slam", "t", "--keypoints", "k.npz", "--start", "0", "--end", "10"])
    assert p.keypoints == "k.npz" and p.heatmaps is None and p.depths is None and p.sigma == 1.5 and p.first_id == 0
    with pytest.raises(SystemExit):
        live._parser().parse_args(["--slam", "t", "--keypoints", "k.npz", "--heatmaps", "H", "--start", "0", "--end", "10"])


def test_twin_splat_peaks_where_heatmap_coords_says():
    from globalegomocap_amd import synth
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    seq = synth.make_sequence(n_frames=4, seed=8, camera=cam, with_heatmaps=False)
    clean = np.einsum("nij,nkj->nki", np.linalg.inv(np.asarray(seq["camera_pose_list"]))[:, :3, :3],
                      np.asarray(seq["gt_global_skeleton"]) - np.asarray(seq["camera_pose_list"])[:, None, :3, 3])
    uv = cam.project_numpy(clean.reshape(-1, 3)).reshape(4, 15, 2)
    kp = np.concatenate([uv, np.full((4, 15, 1), 0.8)], axis=2)
    ix, iy = synth.heatmap_coords(uv)
    assert np.allclose(np.stack([ix, iy], -1), seq["heatmap_centres"], atol=1e-9)
    heat = KT.splat(kp)
    assert heat.shape == (4, 64, 64, 15) and heat.dtype == np.float32
    flat = heat.reshape(4, 64 * 64, 15).argmax(axis=1)
    assert np.array_equal(flat % 64, np.rint(ix).astype(int)) and np.array_equal(flat // 64, np.rint(iy).astype(int))
    # the peak's height is a Gaussian's value half a pixel away at the most, times the confidence
    peak = heat.reshape(4, 64 * 64, 15).max(axis=1)
    assert (peak <= 0.8 + 1e-7).all() and (peak >= 0.8 * np.exp(-0.5 / (2 * 1.5 ** 2)) - 1e-7).all()
    # with confidence 1 it is synth's own map
    one = KT.splat(np.concatenate([uv, np.ones((4, 15, 1))], axis=2))
    assert np.array_equal(one, synth.gaussian_heatmaps(ix, iy, 1.5))
    # blank rule, clamp, and a non-square map
    odd = kp[:1].copy()
    odd[0, 0, 2], odd[0, 1, 2], odd[0, 2, 0], odd[0, 3, 2] = 0.0, np.nan, np.inf, 1.7
    h = KT.splat(odd, 47, 33)
    assert h.shape == (1, 47, 33, 15) and not h[..., :3].any() and h[..., 4].any()
    jx, jy = KT.heat_coords(odd, 47, 33)
    assert np.array_equal(h[0, :, :, 3], np.exp(-((np.arange(33)[None] - jx[0, 3]) ** 2 + (np.arange(47)[:, None] - jy[0, 3]) ** 2) / 4.5).astype(np.float32))


def test_the_header_declares_what_is_bound():
    from globalegomocap_amd import _capi
    header = open(os.path.join(ROOT, "include", "gem_hip.h")).read()
    for name in ("gem_keypoint_heatmaps", "gem_lift_keypoints", "gem_fill_missing"):
        n_args = len(re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header).group(1).split(","))
        assert len(_capi.SIGNATURES[name][1]) == n_args, name
    src = open(os.path.join(ROOT, "globalegomocap_amd", "csrc", "errors.hip")).read()
    assert src.count('#include "keypoints.h"') == 1


def test_depths_from_the_pose_networks_mat_directory(tmp_path):
    """Frame id i is entry i of the naturally sorted listing, as in `prepare`; `loadmat(...)['depth'][0]` of each."""
    from scipy.io import savemat
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import detections as D
    rng = np.random.default_rng(2)
    depth = rng.uniform(0.2, 1.5, (11, 15))
    for k in range(11):
        savemat(str(tmp_path / ("f_%d.mat" % k)), {"depth": depth[k].reshape(1, 15)}, do_compression=k % 2 == 1)
    got = D.depths_from_mat_dir(str(tmp_path), np.array([10, 2, 9]))          # (f_10 sorts behind f_9: natural order)
    assert got.dtype == np.float64 and np.array_equal(got, depth[[10, 2, 9]])
    with pytest.raises(ValueError, match=r"no entry for frame ids \[11\]"):
        D.depths_from_mat_dir(str(tmp_path), np.array([3, 11]))
