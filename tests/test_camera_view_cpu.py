"""The camera's view, the part that needs no GPU: the numpy twin (tests/camera_view_twin.py) on hand-made cases,
the view structure, and the arguments of the entry points."""
import ctypes as C
import pickle

import numpy as np
import pytest

import camera_view_twin as T

RED, BLUE, HEAT = (214, 39, 40), (31, 119, 180), (148, 103, 189)


@pytest.fixture(scope="module")
def R():
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import render
    return render


def far_away(S=1):
    """Image points far outside the crop for every joint, all in one place: nothing to draw."""
    return np.full((S, 15, 2), -5000.0, dtype=np.float32)


def lowest_covering(uv, N, joint_radius, line_radius, skip=()):
    """Per pixel the lowest index of the primitives of ONE sequence that cover it (-1: none), without those in `skip`: the rule
    spelt out, independent of the order in which the twin paints."""
    from globalegomocap_amd.skeleton import MESH_LINES
    _, (u, v) = T.places(N)
    ids = np.full((N, N), -1)
    for c in range(29, -1, -1):
        ja, jb = (c, c) if c < 15 else MESH_LINES[c - 15]
        if c not in skip:
            ids[T.distances(uv[ja].astype(float), uv[jb].astype(float), u, v)[0] <= (joint_radius if c < 15 else line_radius)] = c
    return ids


def test_the_places_of_the_pixels():
    for N in (32, 512, 1024):          # a power of two: both precisions hold the same numbers
        (u32, v32), (u64, v64) = T.places(N)
        assert u32.dtype == np.float32 and np.array_equal(u32.astype(np.float64), u64) and np.array_equal(v32.astype(np.float64), v64)
    (_, _), (u, v) = T.places(40)
    assert np.allclose(u[[0, -1]], [128 + 12.8, 1152 - 12.8]) and np.allclose(v[[0, -1]], [12.8, 1024 - 12.8])


def test_a_single_disc():
    """Joint 0 at the middle of the crop, radius 100 at N = 64 (16 image pixels per pixel): the pixels whose centres lie within 100,
    no heat-maps, so everything else is white."""
    uv = far_away()
    uv[0, 0] = (640.0, 512.0)
    im = T.render(None, uv, [RED], 64, joint_radius=100.0, line_radius=0.0)
    k = (np.arange(64) + 0.5) * 16.0
    want = (k[None, :] + 128.0 - 640.0) ** 2 + (k[:, None] - 512.0) ** 2 <= 100.0 ** 2
    assert np.array_equal(im.ids == 0, want) and set(np.unique(im.ids)) == {-1, 0} and want.sum() == 120
    assert (im.rgb[want] == RED).all() and (im.rgb[~want] == 255).all() and not im.response.any()
    assert not im.near_edge.any() and not im.near_round.any()
    # a rim through pixel centres is reported: at N = 128 the centres are 8 apart, so radius 8 about one of them goes through its four
    # neighbours (<=: they belong to the disc); the fifth is the centre itself, on the rim of the lines of radius 0 that start there
    uv[0, 0] = (128.0 + 8.0 * 10.5, 8.0 * 20.5)
    im = T.render(None, uv, [RED], 128, joint_radius=8.0, line_radius=0.0)
    assert im.near_edge.sum() == 5 and (im.ids == 0).sum() == 5 and im.near_edge[20, 10] and im.near_edge[19, 10] and not im.near_edge[19, 9]


def test_the_priority_order():
    """Two sequences with the same points: the higher one shows.  Within one: a joint over a line, the lower index within a class."""
    uv = far_away(2)
    for s in range(2):
        uv[s, 0], uv[s, 1], uv[s, 4] = (400.0, 500.0), (800.0, 500.0), (400.0, 800.0)          # lines 0 = (0, 1) and 1 = (0, 4) meet in joint 0
    im = T.render(None, uv, [RED, BLUE], 64, joint_radius=60.0, line_radius=30.0)
    assert im.ids.max() >= 30 and not ((im.ids >= 0) & (im.ids < 30)).any()          # nothing of sequence 0 is left
    assert (im.rgb[im.ids >= 0] == BLUE).all() and (im.rgb[im.ids < 0] == 255).all()
    one = T.render(None, uv[:1], [RED], 64, joint_radius=60.0, line_radius=30.0)
    assert np.array_equal(one.ids >= 0, im.ids >= 0) and np.array_equal(one.ids[one.ids >= 0] + 30, im.ids[im.ids >= 0])
    assert np.array_equal(one.ids, lowest_covering(uv[0], 64, 60.0, 30.0))
    at = lambda x, y: one.ids[int(y / 16), int((x - 128) / 16)]          # noqa: E731
    assert at(400, 500) == 0 and at(800, 500) == 1 and at(600, 500) == 15 and at(400, 650) == 16
    assert at(400 + 50, 500) == 0          # inside joint 0's disc AND line 0: the joint
    # where both lines cover a pixel outside the disc (a smaller one here) the lower index wins
    small = T.render(None, uv[:1], [RED], 64, joint_radius=20.0, line_radius=30.0)
    _, (u, v) = T.places(64)
    both = (T.distances(uv[0, 0].astype(float), uv[0, 1].astype(float), u, v)[0] <= 30.0) & \
           (T.distances(uv[0, 0].astype(float), uv[0, 4].astype(float), u, v)[0] <= 30.0) & (small.ids != 0)
    assert both.any() and (small.ids[both] == 15).all()


def test_a_point_that_is_not_finite():
    """Joint 1 NaN or infinite: its disc and the lines (0, 1), (1, 2), (1, 7) -- primitives 1, 15, 17 and 21 -- are not drawn, and
    what they hid shows."""
    uv = far_away()
    uv[0, 0], uv[0, 1], uv[0, 2], uv[0, 4], uv[0, 7] = (400.0, 500.0), (800.0, 500.0), (800.0, 300.0), (400.0, 800.0), (800.0, 700.0)
    whole = T.render(None, uv, [RED], 64, joint_radius=60.0, line_radius=30.0).ids
    assert {1, 15, 17, 21} <= set(np.unique(whole))
    want = lowest_covering(uv[0], 64, 60.0, 30.0, skip=(1, 15, 17, 21))
    assert {0, 2, 4, 7, 16} <= set(np.unique(want))
    for bad in (np.nan, np.inf, -np.inf):
        for axis in (0, 1):
            uv[0, 1, axis] = bad
            assert np.array_equal(T.render(None, uv, [RED], 64, joint_radius=60.0, line_radius=30.0).ids, want), (bad, axis)
            uv[0, 1] = (800.0, 500.0)


def test_the_background_and_a_mask_of_zero():
    heat = np.zeros((64, 64, 15), dtype=np.float32)
    heat[20, 30, 3], heat[20, 30, 5], heat[40, 10, 5] = 1.0, 0.5, 2.0
    im = T.render(heat, far_away(), [RED], 64)
    # pixel (px, py) of 64 stands at texel ((px + 0.5) * 63 / 64, (py + 0.5) * 63 / 64): texel (30, 20) is seen from pixels 29 and 30
    fx, fy = 30.5 * 63 / 64 - 30, 20.5 * 63 / 64 - 20
    assert np.isclose(im.response[20, 30], (1 - fx) * (1 - fy), atol=1e-6) and np.isclose(im.response[20, 29], (29.5 * 63 / 64 - 29) * (1 - fy), atol=1e-6)
    assert im.response.max() == 1.0 and im.response[40, 10] == 1.0          # clamped
    m = float(im.response[20, 30])
    assert (im.rgb[20, 30] == [int(np.floor(255 + (c - 255) * m + 0.5)) for c in HEAT]).all()
    assert (im.rgb[0, 0] == 255).all() and (im.ids == -1).all()
    only3 = T.render(heat, far_away(), [RED], 64, joint_mask=1 << 3)
    assert only3.response[40, 10] == 0.0 and only3.response[20, 30] == im.response[20, 30]
    only5 = T.render(heat, far_away(), [RED], 64, joint_mask=1 << 5)
    assert np.isclose(only5.response[20, 30], 0.5 * m, rtol=1e-6)
    none = T.render(heat, far_away(), [RED], 64, joint_mask=0)
    assert not none.response.any() and (none.rgb == 255).all()


def test_the_view_structure(R):
    from globalegomocap_amd import _capi
    assert C.sizeof(_capi.GemCameraView) == 32
    v = R.camera_view()
    assert (v.size, v.joint_mask, v.rgb_heat, v.joint_radius, v.line_radius) == (512, 0x7FFF, 148 | (103 << 8) | (189 << 16), 8.0, 3.0)
    v = R.camera_view(37, 2.5, 0.0, heat_joints=[0, 14, 14], heat_colour=(1, 2, 3))
    assert (v.size, v.joint_mask, v.rgb_heat, v.joint_radius, v.line_radius) == (37, 1 | (1 << 14), 1 | (2 << 8) | (3 << 16), 2.5, 0.0)
    assert R.camera_view(heat_joints=[]).joint_mask == 0
    for kw in (dict(size=0), dict(size=1025), dict(heat_joints=[15]), dict(joint_radius=-1.0), dict(line_radius=float("nan")),
               dict(joint_radius=float("inf"))):
        with pytest.raises(ValueError):
            R.camera_view(**kw)
    assert R.VIEWS == ("side", "front", "top") and _capi.load_library().gem_version() == 1


def test_cli_argument_errors(R, tmp_path, capsys):
    frames = [np.zeros((15, 3)) for _ in range(3)]
    poses = str(tmp_path / "poses.pkl")
    with open(poses, "wb") as f:
        pickle.dump({"estimated_pose": frames, "optimized_pose": np.asarray(frames)}, f)
    empty = tmp_path / "chunk_without_data"
    empty.mkdir()
    o = str(tmp_path / "o")
    for argv, word in (([poses, "--out", o, "--camera", str(empty)], "no test_data.pkl"),
                       ([poses, "--out", o, "--camera", str(tmp_path / "nowhere")], "no test_data.pkl"),
                       ([poses, "--out", o, "--camera", str(empty), "--size", "640x480"], "one number"),
                       ([poses, "--out", o, "--camera", str(empty), "--size", "2000"], "one number"),
                       ([poses, "--out", o, "--camera"], "--camera"),
                       ([poses, "--out", o, "--size", "512"], "WIDTHxHEIGHT")):
        with pytest.raises(SystemExit) as e:
            R.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    assert not (tmp_path / "o").exists()


def test_the_settings_and_the_command_line_take_render_camera():
    from globalegomocap_amd import whole_sequence as ws
    assert ws._settings("cam.json").render_camera is None
    s = ws._settings("cam.json", render_camera="somewhere")
    assert s.render_camera == "somewhere" and s.render is None
    a = ws._parser().parse_args(["--data_path", "d", "--render_camera", "seen"])
    assert a.render_camera == "seen" and a.render is None
    a = ws._parser().parse_args(["--data_path", "d", "--render", "seen", "--render_camera", "seen"])
    assert a.render_camera == a.render == "seen"
    assert ws._parser().parse_args(["--data_path", "d"]).render_camera is None
    import inspect
    from globalegomocap_amd import optimizer
    assert inspect.signature(optimizer.main).parameters["render_camera"].default is None
