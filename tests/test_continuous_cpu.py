"""A recording optimised as one motion, the host side: the window table that covers every frame, the float64
definition of the merge of windows that are not equally spaced, `Recording.continuous()` and the command line's parser."""
import numpy as np
import pytest

from globalegomocap_amd import sequence as S


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------ cover_starts / check_cover
@pytest.mark.parametrize("n, want", [(10, [0]), (11, [0, 1]), (18, [0, 8]), (19, [0, 8, 9]), (27, [0, 8, 16, 17])])
def test_cover_starts_small(n, want):
    got = S.cover_starts(n)
    assert got.dtype == np.int32 and got.tolist() == want


def test_cover_starts_against_window_starts():
    assert S.cover_starts(100).tolist() == S.window_starts(100).tolist() + [90]
    assert S.cover_starts(98).tolist() == S.window_starts(98).tolist()
    for k in range(1, 6):
        assert np.array_equal(S.cover_starts(8 * k + 2), S.window_starts(8 * k + 2))


def test_cover_starts_refuses():
    with pytest.raises(ValueError):
        S.cover_starts(9)
    for stride in (0, 9, -1):
        with pytest.raises(ValueError):
            S.cover_starts(27, stride=stride)


@pytest.mark.parametrize("stride", range(1, 9))
def test_cover_starts_cover_every_frame(stride):
    s = S.cover_starts(27, stride=stride)
    covered = np.zeros(27, dtype=int)
    for a in s:
        covered[a:a + 10] += 1
    assert (covered >= 1).all() and (np.diff(s) > 0).all() and s[0] == 0 and s[-1] + 10 == 27
    assert np.array_equal(S.check_cover(s, 10), s)


@pytest.mark.parametrize("starts", [[1, 9], [0, 8, 8], [0, 8, 7], [0, 11], []])
def test_check_cover_refuses(starts):
    with pytest.raises(ValueError):
        S.check_cover(starts, 10)


# ------------------------------------------------------------------------------------------------------------------ merge_cover
def _windows(n, seed, J=15):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, (n, 10, J, 3))


def test_merge_cover_is_merge_batches_at_window_starts():
    starts = S.window_starts(100)
    w = _windows(len(starts), 1)
    merged, count = S.merge_cover(w, starts)
    want = np.asarray(S.merge_batches(w, 2))
    assert merged.shape == want.shape == (98, 15, 3) and np.array_equal(_bits(merged), _bits(want))
    assert count.tolist() == S.dense_counts(12, 8).tolist()


@pytest.mark.parametrize("stride", range(1, 9))
def test_merge_cover_is_merge_dense_at_constant_strides(stride):
    w = _windows(12, 10 + stride)
    w[3, 2, 4, 1] = -0.0
    merged, count, spread = S.merge_cover(w, np.arange(12) * stride, want_spread=True)
    want = S.merge_dense(w, stride)
    assert np.array_equal(_bits(merged), _bits(want)) and count.tolist() == S.dense_counts(12, stride).tolist()
    assert spread.shape == count.shape and (spread[count == 1] == 0).all() and (spread[count > 1] > 0).all()


def test_merge_cover_keeps_a_negative_zero():
    w = _windows(3, 5)
    w[0, 0] = -0.0          # frame 0: window 0 alone
    w[2, 9] = -0.0          # frame 18: window 2 alone
    merged, count = S.merge_cover(w, [0, 8, 9])
    assert count[0] == 1 and count[18] == 1
    assert np.signbit(merged[0]).all() and (merged[0] == 0).all() and np.signbit(merged[18]).all()


def test_merge_cover_count_and_spread_against_a_loop():
    starts, T = [0, 8, 9], 10
    w = _windows(3, 7) * 0.01 + 1e3
    merged, count, spread = S.merge_cover(w, starts, want_spread=True)
    assert merged.shape == (19, 15, 3) and count.dtype == np.int32
    for f in range(19):
        cover = [(i, f - a) for i, a in enumerate(starts) if 0 <= f - a < T]
        assert count[f] == len(cover)
        total = w[cover[0][0], cover[0][1]].copy()
        for i, t in cover[1:]:
            total = total + w[i, t]
        mean = total / len(cover)
        assert np.array_equal(_bits(merged[f]), _bits(mean))
        far = 0.0
        for i, t in cover:
            for j in range(15):
                dx, dy, dz = (w[i, t, j, d] - mean[j, d] for d in range(3))
                far = max(far, np.sqrt((dx * dx + dy * dy) + dz * dz))
        assert spread[f] == (far if len(cover) > 1 else 0.0)
    assert count.tolist() == [1] * 8 + [2] + [3] + [2] * 8 + [1]
    with pytest.raises(ValueError):
        S.merge_cover(w, [0, 11, 12])
    with pytest.raises(ValueError):
        S.merge_cover(w, [0, 8])


# ------------------------------------------------------------------------------------------------------------------ Recording.continuous()
def _chunked(lengths, seed=3):
    from globalegomocap_amd import prepare as P, synth
    n = sum(lengths)
    s = synth.make_sequence(n_frames=n, seed=seed, cam_jitter=(2.0, 0.01))
    C = np.asarray(s["camera_pose_list"], dtype=np.float64)
    C[:, :3, 3] += np.array([300.0, -200.0, 50.0])          # (a world whose coordinates are not small)
    est = np.asarray(s["estimated_local_skeleton"], dtype=np.float64)
    heat = np.asarray(s["heatmap_list"], dtype=np.float32)
    world = np.linalg.inv(C[0])[None] @ C
    chunks, origins, a = [], [], 0
    for m in lengths:
        cams = np.linalg.inv(C[a])[None] @ C[a:a + m]
        glob = np.einsum("nij,nkj->nki", cams[:, :3, :3], est[a:a + m]) + cams[:, None, :3, 3]
        chunks.append(P.RecordingChunk(a, a + m, heat[a:a + m], est[a:a + m], glob, cams, None))
        origins.append(world[a])
        a += m
    return P, chunks, np.stack(origins), world, est, heat


def test_recording_continuous_on_the_host():
    P, chunks, origins, world, est, heat = _chunked((10, 12, 11))
    rec = P.Recording(chunks, origins, scale=1.5, scale_report="scale", bridge_report=None, depth_report="depth")
    one = rec.continuous()
    assert len(one) == 1 and np.array_equal(one.origins, np.eye(4)[None])
    assert (one.scale, one.scale_report, one.bridge_report, one.depth_report) == (1.5, "scale", None, "depth")
    c = one.chunks[0]
    assert (c.start_frame, c.end_frame, c.n, c.name) == (0, 33, 33, "data_start_0_end_33") and c.gt is None
    assert c.cams.dtype == np.float64 and c.cams.shape == (33, 4, 4)
    err = np.abs(c.cams - world).max()
    want = np.einsum("nij,nkj->nki", world[:, :3, :3], est) + world[:, None, :3, 3]
    err_g = np.abs(c.est_global - want).max()
    print("continuous(): cameras differ by %.3g, global poses by %.3g" % (err, err_g))
    assert err <= 1e-12 and err_g <= 1e-12
    assert np.array_equal(c.est_local, est) and c.heat.dtype == np.float32 and np.array_equal(c.heat, heat)
    assert one.continuous() is one and P.Recording(chunks[:1], origins[:1]).continuous().chunks[0] is chunks[0]


def test_recording_continuous_refuses():
    P, chunks, origins, *_ = _chunked((10, 12, 11))
    with pytest.raises(ValueError, match="follow"):
        P.Recording([chunks[0], chunks[2]], origins[[0, 2]]).continuous()
    with pytest.raises(ValueError, match="no common frame"):
        P.Recording(chunks[:2], None).continuous()
    assert len(P.Recording(chunks[:1], None).continuous()) == 1          # (one chunk is one span already, with a ground truth too)


# ------------------------------------------------------------------------------------------------------------------ the command line
BASE = ["--slam", "t.txt", "--start", "0", "--end", "100"]


def test_parser_accepts():
    from globalegomocap_amd import continuous
    a = continuous.parse_args(BASE + ["--heatmaps", "H", "--depth_from", "bones", "--scale", "auto", "--bridge", "--stride", "3", "--bvh", "out",
                                      "--upright", "true", "--foot_lock", "true", "--final_smooth", "false"])
    assert a.stride == 3 and a.scale == "auto" and a.bridge == 1.0 and a.bvh == "out" and a.upright and a.foot_lock and not a.final_smooth
    a = continuous.parse_args(BASE + ["--keypoints", "k.npz", "--depth", "d.npy", "--gt", "gt.pkl", "--gltf", "out", "--save_pose", "poses"])
    assert a.stride == 8 and a.gt == "gt.pkl" and a.keypoints == "k.npz" and a.gltf == "out" and a.final_smooth


@pytest.mark.parametrize("extra", [
    ["--heatmaps", "H", "--depths", "D", "--scale", "1", "--stride", "9"],
    ["--heatmaps", "H", "--depths", "D", "--scale", "1", "--stride", "0"],
    ["--heatmaps", "H", "--depths", "D", "--gt", "gt.pkl", "--bridge"],
    ["--heatmaps", "H", "--scale", "1"],                                         # no depths
    ["--heatmaps", "H", "--keypoints", "k.npz", "--depths", "D", "--scale", "1"],
    ["--heatmaps", "H", "--depths", "D", "--scale", "1", "--sigma", "2"],
    ["--keypoints", "k.npz", "--depths", "D", "--scale", "1", "--peaks", "subpixel"],
    ["--heatmaps", "H", "--depths", "D", "--scale", "1", "--chunks_per_batch", "2"],
    ["--heatmaps", "H", "--depths", "D", "--scale", "1", "--video", "v", "--video_quality", "0"],
])
def test_parser_refuses(extra, capsys):
    from globalegomocap_amd import continuous
    with pytest.raises(SystemExit):
        continuous.parse_args(BASE + extra)
    capsys.readouterr()


def test_the_chunked_command_lines_accept_what_they_accepted():
    """`whole_sequence`'s parser was split into helpers this module shares: its options and defaults are the ones it had."""
    from globalegomocap_amd import whole_sequence as ws
    a = ws._parser().parse_args(["--data_path", "d"])
    assert sorted(vars(a)) == sorted([
        "data_path", "camera", "vae", "gmm", "smooth", "bone_length", "weight_3d", "reproj_weight", "save", "mesh_root", "render", "render_camera",
        "bvh", "bvh_fps", "gltf", "gltf_fps", "video", "video_camera", "video_fps", "video_quality", "upright", "foot_height", "foot_lock",
        "foot_lock_stretch", "foot_lock_blend", "final_smooth", "merge", "chunks_per_batch", "ground_truth", "save_pose"])
    assert (a.vae, a.gmm, a.smooth, a.bone_length, a.weight_3d, a.reproj_weight) == (0.0, 0.0, 0.001, 0.01, 0.01, 0.01)
    assert a.final_smooth is True and a.merge is True and a.ground_truth is True and a.save is False and a.mesh_root == "out"
    assert all(getattr(a, k) is None for k in ("render", "render_camera", "bvh", "bvh_fps", "gltf", "gltf_fps", "video", "video_camera", "video_fps",
                                               "video_quality", "foot_height", "foot_lock_stretch", "foot_lock_blend", "chunks_per_batch", "save_pose"))
    with pytest.raises(ValueError, match="continuous"):
        ws.optimize_recording(None, "camera.json", stride=4)
