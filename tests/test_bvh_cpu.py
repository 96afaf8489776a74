"""BVH animation files, the part that needs no GPU: the numpy twin (tests/bvh_twin.py) against itself -- forward
kinematics of its inverse kinematics give back the re-grown skeleton --, the library's layout and tables against the tree,
`bvh.read_bvh` / `joint_positions` on a file the twin wrote, and the argument errors."""
import os
import pickle

import numpy as np
import pytest

import bvh_twin as T


@pytest.fixture(scope="module")
def B():
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import bvh
    return bvh


@pytest.fixture(scope="module")
def frames37():
    X = T.random_frames(37, seed=1)
    X.setflags(write=False)
    return X


def test_twin_forward_of_inverse_is_the_regrown_skeleton(frames37, capsys):
    """FK(IK(X)) = regrow(X) to 1e-12 m; with every channel rounded to six decimals (unit_scale 1) to 2e-6 m: 5e-7 from the root's
    position and below 1e-7 from at most 7 chained angles, each rounded by 5e-7 degrees over bones shorter than 1 m."""
    rest = T.rest_lengths(frames37)
    chan = T.channels(frames37)
    want = T.regrow(frames37, rest)
    exact = np.abs(T.fk(chan, T.offsets_of(rest)) - want).max()
    rounded = np.abs(T.fk(np.round(chan, 6), T.offsets_of(rest)) - want).max()
    with capsys.disabled():
        print("twin: FK(IK(X)) - regrow(X) %.3g m, with channels rounded to six decimals %.3g m" % (exact, rounded))
    assert exact <= 1e-12
    assert rounded <= 2e-6
    # the joints themselves come back up to the bones' lengths: a skeleton whose bones have the rest lengths comes back exactly
    fixed = T.joints_of(want)
    again = T.fk(T.channels(fixed), T.offsets_of(T.rest_lengths(fixed)))
    np.testing.assert_allclose(T.joints_of(again), fixed, rtol=0, atol=1e-12)
    # the local rotations are rotations, and the leaves' channels are zeros
    L = T.local_matrices(chan)
    np.testing.assert_allclose(L @ np.swapaxes(L, -1, -2), np.broadcast_to(np.eye(3), L.shape), rtol=0, atol=1e-12)
    for leaf in (6, 10, 14, 18):
        assert not T.KIDS[leaf] and (chan[:, 3 + 3 * leaf:6 + 3 * leaf] == 0).all()


def test_twin_behind_a_similarity(frames37):
    c, R, t = 1.3, T.euler_matrix(20.0, -35.0, 50.0), np.array([0.1, -0.2, 0.3])
    moved = c * (frames37 @ R) + t
    np.testing.assert_allclose(T.rest_lengths(frames37, (c, R, t)), T.rest_lengths(moved), rtol=1e-13)
    np.testing.assert_allclose(T.rest_lengths(moved), c * T.rest_lengths(frames37), rtol=1e-12)
    np.testing.assert_array_equal(T.channels(frames37, np.concatenate([[c], R.reshape(-1), t])), T.channels(moved))


def test_layout_and_tables_are_the_tree(B):
    import ctypes as C
    from globalegomocap_amd import _capi
    lib = _capi.load_library()
    out = (C.c_int64 * 4)()
    assert lib.gem_bvh_layout(out) == 0 and tuple(out) == (T.N, T.CHANNELS, T.FIELD, T.FRAME_BYTES) == (19, 60, 16, 960)
    assert tuple(B.layout()) == tuple(out)
    tab = B.tables()
    assert tuple(tab.parents.tolist()) == T.PARENTS and tuple(tab.joint_of_node.tolist()) == T.JOINT
    assert np.array_equal(tab.rest_dirs, T.REST) and B.NODE_NAMES == T.NAMES and B.ROOT_CHANNELS == T.ROOT_CHANNELS
    assert sorted(j for j in T.JOINT if j >= 0) == list(range(15))
    assert lib.gem_bvh_layout(None) != 0 and b"null" in lib.gem_last_error()
    assert lib.gem_bvh_tables(None, None, None) != 0 and b"null" in lib.gem_last_error()
    # the entry points that launch refuse their arguments before anything touches a device
    assert lib.gem_bvh_rest(None, 0, None, None, None) != 0 and b"at least one frame" in lib.gem_last_error()
    assert lib.gem_bvh_rest(None, 3, None, None, None) != 0 and b"null" in lib.gem_last_error()
    assert lib.gem_bvh_channels(None, -1, None, None, 1.0, None, None) != 0 and b"n_frames" in lib.gem_last_error()
    assert lib.gem_bvh_channels(None, 3, None, None, 1.0, None, None) != 0 and b"null" in lib.gem_last_error()
    assert lib.gem_bvh_channels(None, 0, None, None, 1.0, None, None) == 0
    assert lib.gem_format_fields(None, 4, 0, None, None, None) != 0 and b"values_per_line" in lib.gem_last_error()
    assert lib.gem_format_fields(None, 4, 2, C.c_void_p(8), None, None) != 0 and b"16-byte aligned" in lib.gem_last_error()
    assert lib.gem_format_fields(None, 4, 2, None, None, None) != 0 and b"null" in lib.gem_last_error()
    assert lib.gem_format_fields(None, 0, 2, None, None, None) == 0


def test_hierarchy_text_is_the_twins(B, frames37):
    rest = T.rest_lengths(frames37)
    assert B.hierarchy_text(rest, 1.0) == T.hierarchy(rest, 1.0)
    assert B.hierarchy_text(rest, 100.0) == T.hierarchy(rest, 100.0)
    assert "-0.000000" not in B.hierarchy_text(rest, 100.0)


def test_read_bvh_reads_what_the_twin_wrote(B, frames37, tmp_path, capsys):
    path = str(tmp_path / "twin.bvh")
    rest, chan = T.write(path, frames37, fps=30, unit_scale=1.0)
    assert os.path.getsize(path) == len(T.hierarchy(rest).encode()) + len("MOTION\nFrames: 37\nFrame Time: 0.033333\n") + 37 * T.FRAME_BYTES
    got, want = B.read_bvh(path), T.parse(path)
    assert got.names == T.NAMES == tuple(want["names"]) and tuple(got.parents.tolist()) == T.PARENTS
    assert got.channels == tuple(want["channels"]) and got.channels[0] == T.ROOT_CHANNELS
    assert got.frame_time == want["frame_time"] == 0.033333
    assert np.array_equal(got.offsets, want["offsets"]) and np.array_equal(got.motion, want["motion"])
    assert np.array_equal(got.motion, np.array([["%.6f" % v for v in row] for row in chan], dtype=np.float64))
    np.testing.assert_allclose(got.offsets, T.offsets_of(rest), rtol=0, atol=5.0000001e-7)
    pos = B.joint_positions(got)
    np.testing.assert_allclose(pos, T.parsed_positions(want), rtol=0, atol=1e-12)
    worst = np.abs(pos - T.regrow(frames37, rest)).max()
    with capsys.disabled():
        print("twin's file at unit_scale 1: positions read back - regrow(X) %.3g m" % worst)
    np.testing.assert_array_equal(B.skeleton_from_nodes(pos), T.joints_of(pos))
    # the channel names in another order: the rotations are multiplied in the order of the file's channels
    text = open(path).read().replace("CHANNELS 3 Zrotation Xrotation Yrotation", "CHANNELS 3 Yrotation Xrotation Zrotation")
    other = str(tmp_path / "other.bvh")
    with open(other, "w") as f:
        f.write(text)
    swapped = B.read_bvh(other)
    assert swapped.channels[1] == ("Yrotation", "Xrotation", "Zrotation") and swapped.channels[0] == T.ROOT_CHANNELS
    a, b, c = got.motion[0, 6:9]
    want_spine = T.euler_matrix(0, 0, a)[:, :] @ T.euler_matrix(0, b, 0) @ T.euler_matrix(c, 0, 0)          # Ry(a) Rx(b) Rz(c)
    G0 = T.euler_matrix(*got.motion[0, 3:6])
    neck = B.joint_positions(swapped)[0, 2]
    np.testing.assert_allclose(neck, got.motion[0, :3] + G0 @ want_spine @ got.offsets[2], rtol=0, atol=1e-12)


def test_read_bvh_refuses_what_it_does_not_understand(B, frames37, tmp_path):
    path = str(tmp_path / "good.bvh")
    T.write(path, frames37[:3])
    data = open(path).read()
    cases = {
        "no hierarchy": data.replace("HIERARCHY", "HIERARCHIE"),
        "a frame short": data[:-T.FRAME_BYTES],
        "a wrong count": data.replace("Frames: 3", "Frames: 4"),
        "an unknown channel": data.replace("Zrotation", "Wrotation", 1),
        "a channel twice": data.replace("CHANNELS 3 Zrotation Xrotation Yrotation", "CHANNELS 3 Zrotation Zrotation Yrotation", 1),
        "an open brace": data.replace("}\nMOTION", "MOTION"),
        "a word in the motion": data[:-16] + "       nan-ish \n",
        "two roots": data.replace("JOINT Spine", "ROOT Spine"),
    }
    for name, bad in cases.items():
        p = str(tmp_path / "bad.bvh")
        with open(p, "w") as f:
            f.write(bad)
        with pytest.raises(ValueError):
            B.read_bvh(p)
            pytest.fail("read_bvh accepted: " + name)


def test_cli_argument_errors(B, tmp_path, capsys):
    frames = [np.zeros((15, 3)) for _ in range(3)]
    no_gt = str(tmp_path / "no_gt.pkl")
    with open(no_gt, "wb") as f:
        pickle.dump({"estimated_pose": frames, "optimized_pose": np.asarray(frames), "mid_optimized_pose": frames}, f)
    no_opt = str(tmp_path / "no_opt.pkl")
    with open(no_opt, "wb") as f:
        pickle.dump({"estimated_pose": frames}, f)
    out = str(tmp_path / "o")
    for argv, word in (([no_gt, "--out", out, "--align", "true"], "gt_pose"),
                       ([no_gt], "--out"),
                       (["--out", out], "pose_pickle"),
                       ([no_opt, "--out", out], "optimized_pose"),
                       ([no_gt, "--out", out, "--fps", "0"], "--fps"),
                       ([no_gt, "--out", out, "--fps", "fast"], "--fps"),
                       ([no_gt, "--out", out, "--unit_scale", "-1"], "--unit_scale")):
        with pytest.raises(SystemExit) as e:
            B.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    assert not (tmp_path / "o").exists()
    with pytest.raises(ValueError, match="ground-truth"):
        B.write_result_bvh(None, out, frames, frames, None, align=True)
    assert not (tmp_path / "o").exists()


def test_the_argument_is_wired_and_none_writes_nothing(B, tmp_path, monkeypatch):
    import inspect
    from globalegomocap_amd import optimizer, report, whole_sequence as ws
    cfg = ws._settings("cam.json", bvh="somewhere", bvh_fps=30.0)
    assert cfg.bvh == "somewhere" and cfg.bvh_fps == 30.0
    assert ws._settings("cam.json").bvh is None and ws._settings("cam.json").bvh_fps is None
    for fn in (ws._settings, optimizer.main):
        par = [p for p in inspect.signature(fn).parameters.values() if p.kind is p.POSITIONAL_OR_KEYWORD]
        assert [p.name for p in par[-2:]] == ["bvh", "bvh_fps"] and par[-2].default is None and par[-1].default is None, fn
    # the positional order of `_settings` is closed: what comes later goes by keyword only
    assert [p.name for p in inspect.signature(ws._settings).parameters.values() if p.kind is p.POSITIONAL_OR_KEYWORD] == [
        "camera_model_path", "vae_weight", "gmm_weight", "smoothness_weight", "bone_length_weight", "weight_3d", "reproj_weight", "final_smooth",
        "merge", "global_vae_path", "local_vae_path", "chunks_per_batch", "optimizer", "device_metrics", "verbose", "seq_len", "overlap",
        "timings", "per_sequence", "ground_truth", "save_pose", "save", "mesh_root", "render", "render_camera", "bvh", "bvh_fps"]
    a = ws._parser().parse_args(["--data_path", "d", "--bvh", "B", "--bvh_fps", "50"])
    assert a.bvh == "B" and a.bvh_fps == 50.0
    a = ws._parser().parse_args(["--data_path", "d"])
    assert a.bvh is None and a.bvh_fps is None
    monkeypatch.chdir(tmp_path)
    seqs = (np.zeros((3, 15, 3)), np.zeros((3, 15, 3)), None)
    report.Outputs().write(None, "studio/chunk_0", seqs)
    report.Outputs(bvh=None, bvh_fps=30).write(None, "studio/chunk_0", seqs)
    assert os.listdir(str(tmp_path)) == []
    calls = []
    monkeypatch.setattr(B, "write_result_bvh", lambda *a, **k: calls.append((a, k)))
    report.Outputs(bvh="root").write("engine", "data/studio/chunk_0", seqs)
    report.Outputs(bvh="root", bvh_fps=50).write("engine", "data/studio/chunk_0", seqs)
    assert [c[0][:2] for c in calls] == [("engine", os.path.join("root", "studio", "chunk_0"))] * 2
    assert [c[1]["fps"] for c in calls] == [25, 50] and calls[0][0][2] is seqs[0] and calls[0][0][4] is None
