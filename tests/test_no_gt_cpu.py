"""Recordings without ground truth, the host side: argument validation, the four-key pickles and their
readers, the recording's common frame (`Recording.origins`, `to_recording_frame`), and the numpy twin of the device report on
cases that can be worked out by hand."""
import os
import pickle

import numpy as np
import pytest

FOUR_KEYS = ["estimated_global_skeleton", "estimated_local_skeleton", "camera_pose_list", "heatmap_list"]


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import prepare
    return prepare


def test_exactly_one_of_ground_truth_and_scale(P, tmp_path):
    """Neither or both: ValueError before anything is opened (the paths do not exist) or any device is touched; the CLI refuses
    both and neither on its own."""
    missing = str(tmp_path / "nothing")
    for kw in (dict(gt_path=None, scale=None), dict(gt_path=missing, scale=1.0)):
        with pytest.raises(ValueError, match="exactly one"):
            P.prepare_sequence(missing, missing, missing, total_start_frame=0, total_end_frame=300, **kw)
        with pytest.raises(ValueError, match="exactly one"):
            P.prepare_spans(missing, missing, missing, kw["gt_path"], [(0, 100)], 25, 0, scale=kw["scale"])
        with pytest.raises(ValueError, match="exactly one"):
            P.main(missing, missing, missing, kw["gt_path"], 0, 100, missing, 25, 0, scale=kw["scale"])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="positive"):
            P.prepare_sequence(missing, missing, missing, None, 0, 300, scale=bad)
    common = ["--slam", "t", "--heatmaps", "h", "--depths", "d", "--start", "0", "--end", "300", "--out", "o"]
    with pytest.raises(SystemExit):
        P._parser().parse_args(common + ["--gt", "g.pkl", "--scale", "1.0"])
    with pytest.raises(SystemExit):
        P._parser().parse_args(common)
    a = P._parser().parse_args(common + ["--scale", "1.5"])
    assert a.gt is None and a.scale == 1.5
    a = P._parser().parse_args(common + ["--gt", "g.pkl"])
    assert a.gt == "g.pkl" and a.scale is None


def _chunk(P, rng, n=6, start=40, with_gt=False):
    heat = rng.random((n, 64, 64, 15)).astype(np.float32)
    gt = rng.normal(size=(n, 15, 3)) if with_gt else None
    return P.RecordingChunk(start, start + n, heat, rng.normal(size=(n, 15, 3)), rng.normal(size=(n, 15, 3)),
                            np.tile(np.eye(4), (n, 1, 1)) + rng.normal(size=(n, 4, 4)), gt)


def test_four_key_pickles_and_their_readers(P, tmp_path):
    from globalegomocap_amd.whole_sequence import parse_chunk
    rng = np.random.default_rng(5)
    c = _chunk(P, rng)
    assert c.gt is None and c.gt_list is None and c.initial_mpjpe is None
    rec = P.Recording([c], origins=np.eye(4)[None])
    d = rec.chunk_dict(0)
    assert list(d) == FOUR_KEYS
    flag = lambda x: (x.dtype.str, "F" if (x.flags.f_contiguous and not x.flags.c_contiguous) else "C")      # noqa: E731
    # the other four keys as a ground-truth chunk of the same arrays gives them: containers, dtypes, memory orders, values
    with_gt = P.RecordingChunk(c.start_frame, c.end_frame, c.heat, c.est_local, c.est_global, c.cams, np.zeros((c.n, 15, 3)))
    full = P.Recording([with_gt]).chunk_dict(0)
    assert list(full) == list(P.PICKLE_KEYS) == ["gt_global_skeleton"] + FOUR_KEYS
    for k in FOUR_KEYS:
        assert isinstance(d[k], list) and len(d[k]) == c.n
        assert [flag(x) for x in d[k]] == [flag(x) for x in full[k]], k
        assert all(np.array_equal(x, y) for x, y in zip(d[k], full[k])), k
    (path,) = rec.write_chunks(str(tmp_path))
    assert path == str(tmp_path / c.name)
    with open(os.path.join(path, "test_data.pkl"), "rb") as f:
        assert list(pickle.load(f)) == FOUR_KEYS
    for native in (True, False):
        q = parse_chunk(path, native=native, ground_truth=False)
        assert "gt" not in q and q["n"] == c.n
        assert np.array_equal(q["est_local"], c.est_local) and np.array_equal(q["cams"], c.cams)
        assert ("heat_offsets" in q) == native          # (the native reader takes such a file as it is)
        with pytest.raises(KeyError, match="gt_global_skeleton"):
            parse_chunk(path, native=native)
    q = parse_chunk(path, native=False, ground_truth=False)
    assert np.array_equal(np.asarray(q["heat_list"]), c.heat)
    # a file that has the key is fine without it being asked for
    (path5,) = P.Recording([with_gt]).write_chunks(str(tmp_path / "five"))
    for native in (True, False):
        q = parse_chunk(path5, native=native, ground_truth=False)
        assert "gt" not in q and np.array_equal(q["est_local"], c.est_local) and np.array_equal(q["cams"], c.cams)
        assert np.array_equal(parse_chunk(path5, native=native)["gt"], np.zeros((c.n, 15, 3)))


def _trajectory(n, fps, first_id):
    from globalegomocap_amd import synth_recording as S
    return S.random_parameters(n, seed=11, fps=fps, first_id=first_id)["rows"]


def test_origins_put_the_chunks_into_one_frame(P):
    from globalegomocap_amd import slam
    fps, first, size, scale = 25, 7, 20, 1.37
    rows = _trajectory(3 * size + 5, fps, first)
    spans = [(first + k * size, first + (k + 1) * size) for k in range(3)]
    cams, origins = P.scaled_cameras(rows, spans, fps, scale)
    assert origins.shape == (3, 4, 4) and origins.dtype == np.float64
    whole = slam.scaled_trajectory(*slam.parse_trajectory(rows, spans[0][0], spans[-1][1], fps), scale)
    assert whole.shape == (3 * size, 4, 4)
    rng = np.random.default_rng(2)
    poses = [rng.normal(size=(size, 15, 3)) for _ in spans]
    chunks = [P.RecordingChunk(a, b, np.zeros((size, 1, 1, 15), np.float32), poses[k], poses[k], cams[k], None) for k, (a, b) in enumerate(spans)]
    rec = P.Recording(chunks, origins)
    moved = P.to_recording_frame(rec, poses)
    for k, (a, b) in enumerate(spans):
        assert np.array_equal(cams[k], slam.scaled_trajectory(*slam.parse_trajectory(rows, a, b, fps), scale))      # the reference's read_trajectory, per chunk
        np.testing.assert_allclose(origins[k] @ cams[k], whole[k * size:(k + 1) * size], rtol=0, atol=1e-12)
        direct = np.einsum("ij,fnj->fni", origins[k][:3, :3], poses[k]) + origins[k][:3, 3]
        np.testing.assert_allclose(moved[k], direct, rtol=0, atol=1e-13)
    np.testing.assert_allclose(origins[0], np.eye(4), rtol=0, atol=1e-15)
    # a point that is at rest in the recording's frame, seen from every chunk, comes back to itself
    X = np.array([0.3, -1.2, 2.0])
    local = [np.einsum("fij,j->fi", np.linalg.inv(origins[k] @ cams[k])[:, :3, :], np.append(X, 1.0)) for k in range(3)]
    in_chunk = [np.einsum("fij,fj->fi", cams[k][:, :3, :3], local[k]) + cams[k][:, :3, 3] for k in range(3)]
    back = P.to_recording_frame(rec, [np.repeat(p[:, None], 15, axis=1) for p in in_chunk])
    for b_ in back:
        np.testing.assert_allclose(b_, np.broadcast_to(X, b_.shape), rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="ground truth"):
        P.to_recording_frame(P.Recording(chunks), poses)


def test_the_twin_on_cases_worked_out_by_hand():
    from globalegomocap_amd import synth
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    from globalegomocap_amd.skeleton import KINEMATIC_PARENTS
    from helpers import oracle_camera
    from quality_twin import sequence_quality, BONES
    cam = oracle_camera()
    assert len(BONES) == 14 and 0 not in BONES
    rest = synth.rest_skeleton()
    n, par = 7, list(KINEMATIC_PARENTS)
    cams = np.tile(np.eye(4), (n, 1, 1))
    mb = np.linalg.norm(rest - rest[par], axis=-1)
    # a static sequence under the identity camera, heat-maps equal to one everywhere: response 1 wherever the joints project inside
    # the maps, bones at their mean, no acceleration, no displacement against itself
    static = np.tile(rest, (n, 1, 1))
    ones = np.ones((n, 64, 64, 15), np.float32)
    q = sequence_quality(static, cams, ones, [0], mb.astype(np.float32), 1, cam, ref=static)
    uv = synth.heatmap_coords(FisheyeCamera.from_json(DEFAULT_CALIBRATION).project_numpy(rest))
    inside = (uv[0] >= 0) & (uv[0] <= 63) & (uv[1] >= 0) & (uv[1] <= 63)
    assert inside.all()
    np.testing.assert_allclose(q[0, 0], 1.0, rtol=0, atol=1e-6)
    assert q[0, 1] <= 1e-7          # (mean_bone is float32: its rounding is all that is left)
    assert q[0, 2] == 0.0 and q[0, 3] == 0.0
    assert np.isnan(sequence_quality(static, cams, ones, [0], mb.astype(np.float32), 1, cam)[0, 3])
    # blank heat-maps: response 0; a frame buffer that starts later: frame0 picks the frames
    heat = np.concatenate([np.zeros_like(ones[:3]), ones])
    cams10 = np.tile(np.eye(4), (10, 1, 1))
    assert sequence_quality(static[:3], cams10, heat, [0], mb.astype(np.float32), 1, cam)[0, 0] == 0.0
    np.testing.assert_allclose(sequence_quality(static, cams10, heat, [3], mb.astype(np.float32), 1, cam)[0, 0], 1.0, rtol=0, atol=1e-6)
    # every bone 1 cm too long: RMS 0.01; a uniform translation by d per frame: no acceleration, displacement f * |d|
    grown = rest.copy()
    for j in range(1, 15):          # parents come first in this skeleton
        v = rest[j] - rest[par[j]]
        grown[j] = grown[par[j]] + v * (1.0 + 0.01 / np.linalg.norm(v))
    step = np.array([0.003, -0.004, 0.0])
    moving = grown[None] + np.arange(n)[:, None, None] * step
    q = sequence_quality(moving, cams, ones, [0], mb.astype(np.float32), 1, cam, ref=np.tile(grown, (n, 1, 1)))
    np.testing.assert_allclose(q[0, 1], 0.01, rtol=1e-5)
    assert q[0, 2] <= 1e-15
    np.testing.assert_allclose(q[0, 3], 0.005 * np.mean(np.arange(n)), rtol=1e-12)
    # constant acceleration a per frame^2: |a| for every inner frame and joint
    acc = np.array([0.0, 0.002, -0.001])
    curved = rest[None] + 0.5 * (np.arange(n)[:, None, None] ** 2) * acc
    np.testing.assert_allclose(sequence_quality(curved, cams, ones, [0], mb.astype(np.float32), 1, cam)[0, 2], np.linalg.norm(acc), rtol=1e-10)
    # a camera that moves with the body leaves the response where it was; two chunks are reported one by one
    moved_cams = cams.copy()
    moved_cams[:, :3, 3] = np.arange(n)[:, None] * step
    both = sequence_quality(np.concatenate([static + np.arange(n)[:, None, None] * step, static]), np.concatenate([moved_cams, cams]),
                            np.concatenate([ones, 0.5 * ones]), [0, n], np.stack([mb, mb]).astype(np.float32), 2, cam)
    np.testing.assert_allclose(both[:, 0], [1.0, 0.5], rtol=0, atol=1e-6)
    assert both.shape == (2, 4) and np.isnan(both[:, 3]).all()
