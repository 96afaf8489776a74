"""The camera's view on the device: gem_project_sequence against the oracle's projection and against
gem_sequence_quality's column 0; gem_render_camera against the numpy twin (tests/camera_view_twin.py) -- ids, response, bytes -- the
defined corners, the refusals, determinism; `render.write_camera_frames` through small pinned buffers and the command line; and
`render_camera=DIR` end to end: the batch pipeline with and without ground truth, `optimizer.main`, and that `render=DIR` alone
writes what it wrote before."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

import camera_view_twin as T
from pipeline_checks import (CAMERA_N, IMG, SIZE, check_camera_tree as _check_camera_tree, check_folder, check_tree, same_bits as _same_bits,
                             write_recording as _write_recording)
from globalegomocap_amd.camera import DEFAULT_CALIBRATION

pytestmark = pytest.mark.gpu

RESPONSE_TOL = dict(rtol=5e-5, atol=1e-7)          # what the project holds fp32 projection-dependent values to (tests/test_no_gt_gpu.py)
COORD_ULPS = 3e-5          # texels: heat-map coordinates below 64 have an fp32 ulp of 2^-18 texels; 4 ulp each way
F = 3
SEED = 9
COLOURS = ((214, 39, 40), (31, 119, 180))
HEAT = (148, 103, 189)
CASES = ((32, 40.0, 16.0), (40, 40.0, 16.0), (37, 40.0, 16.0), (19, 60.0, 30.0))          # N, joint radius, line radius


def _rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


CRT = (1.3, _rotation((1.0, 2.0, -1.0), 0.7), np.array([0.1, -0.2, 0.3]))


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import prepare
    return prepare._lift_engine(DEFAULT_CALIBRATION, 0)


_data = {}


def data():
    """Three synthetic frames with rotated cameras: heat-maps, cameras, and two sequences in the cameras' world -- the estimated
    one and the same plus N(0, 3 cm).  Made once, never changed."""
    if not _data:
        from globalegomocap_amd import synth
        s = synth.make_sequence(n_frames=F, seed=SEED, cam_jitter=(2.0, 0.01))
        cams = np.asarray(s["camera_pose_list"], dtype=np.float64)
        local = np.asarray(s["estimated_local_skeleton"], dtype=np.float64)
        heat = np.asarray(s["heatmap_list"], dtype=np.float32)
        seq0 = np.einsum("nij,nkj->nki", cams[:, :3, :3], local) + cams[:, None, :3, 3]
        seq1 = seq0 + np.random.default_rng(SEED).normal(0.0, 0.03, seq0.shape)
        D = float(max(np.abs(np.diff(heat, axis=1)).max(), np.abs(np.diff(heat, axis=2)).max()))          # between neighbouring texels
        _data.update(cams=cams, local=local, heat=heat, seqs=[seq0, seq1], D=D)
    return _data


def _dev(env, a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(env.device)


def _word(c):
    return c[0] | (c[1] << 8) | (c[2] << 16)


def _view(N, jr, lr, mask=0x7FFF, colour=HEAT):
    from globalegomocap_amd import _capi
    return _capi.GemCameraView(size=N, joint_mask=mask, rgb_heat=_word(colour), reserved=0, joint_radius=jr, line_radius=lr)


# ------------------------------------------------------------------------------------------------------------------ 1. projection
def test_projection_against_the_oracle(env, capsys):
    import torch
    from helpers import oracle_camera
    from oracle import np_oracle as O
    from quality_twin import camera_points
    d, cam = data(), oracle_camera()
    seq, cams = d["seqs"][0], d["cams"]
    assert np.abs(cams[:, :3, :3] - np.eye(3)).max() > 1e-3          # the cameras are rotated
    seq_d, cams_d = _dev(env, seq), _dev(env, cams)
    crt_d = _dev(env, np.concatenate([[CRT[0]], CRT[1].reshape(-1), CRT[2]]))
    # a sequence that lands where `seq` is once the similarity has moved it, so that it stays in front of the camera
    pre = ((seq - CRT[2]) / CRT[0]) @ CRT[1].T
    cases = {"through the cameras": (seq_d, cams_d, None, camera_points(seq, cams)),
             "behind a similarity": (_dev(env, pre), cams_d, crt_d, camera_points(CRT[0] * (pre @ CRT[1]) + CRT[2], cams)),
             "in the camera's frame": (_dev(env, d["local"]), None, None, d["local"])}
    for what, (x, c, k, pts) in cases.items():
        got = env.project_sequence(x, c, k)
        assert got.dtype == torch.float32 and tuple(got.shape) == (F, 15, 2) and got.is_cuda
        want = O.fisheye_project(cam, pts.astype(np.float32).reshape(-1, 3)).reshape(F, 15, 2)
        got = got.cpu().numpy()
        with capsys.disabled():
            print("projection %s: largest relative difference to the oracle %.3g" % (what, float(np.abs(got / want - 1).max())))
        np.testing.assert_allclose(got, want, **RESPONSE_TOL)
        assert np.isfinite(got).all()
    assert tuple(env.project_sequence(seq_d[:0].contiguous(), cams_d[:0].contiguous()).shape) == (0, 15, 2)
    with pytest.raises(TypeError):
        env.project_sequence(seq_d.float(), cams_d)
    with pytest.raises(ValueError):
        env.project_sequence(seq_d, cams_d[:2].contiguous())
    with pytest.raises(ValueError):
        env.project_sequence(seq_d[:, :14].contiguous(), cams_d)
    with pytest.raises(TypeError):
        env.project_sequence(seq_d, cams_d, crt_d[:12].contiguous())


def test_a_joint_on_the_optical_axis(env):
    """Exactly on the axis -- in the camera's frame, and through a camera whose translation is exact -- gives a pair that is not
    finite and no error; its neighbours are not touched."""
    d = data()
    local = d["local"][:1].copy()
    local[0, 6] = (0.0, 0.0, -0.75)
    plain = env.project_sequence(_dev(env, d["local"][:1])).cpu().numpy()
    got = env.project_sequence(_dev(env, local)).cpu().numpy()
    assert not np.isfinite(got[0, 6]).any() and np.isfinite(np.delete(got, 6, axis=1)).all()
    assert np.array_equal(np.delete(got, 6, axis=1), np.delete(plain, 6, axis=1))
    cam = np.eye(4)[None].copy()
    cam[0, :3, 3] = (0.5, 0.25, 0.0)
    moved = local + cam[0, :3, 3]
    assert np.array_equal(moved[0, 6], (0.5, 0.25, -0.75))
    got = env.project_sequence(_dev(env, moved), _dev(env, cam)).cpu().numpy()
    assert not np.isfinite(got[0, 6]).any() and np.isfinite(np.delete(got, 6, axis=1)).all()


def test_projection_ties_to_the_quality_report(env, capsys):
    """The mean of the oracle's bilinear samples at the device's image points is gem_sequence_quality's column 0 for those frames."""
    import torch
    from oracle import np_oracle as O
    d = data()
    seq_d, cams_d, heat_d = _dev(env, d["seqs"][0]), _dev(env, d["cams"]), _dev(env, d["heat"])
    uv = env.project_sequence(seq_d, cams_d).cpu().numpy().reshape(-1, 2)
    ix, iy = O.heat_coords(uv, 64, 64)
    maps = d["heat"].transpose(0, 3, 1, 2).reshape(-1, 64, 64)
    want = np.sum(O.bilinear_sample(maps, ix, iy)[0], dtype=np.float64) / (F * 15)
    mb = env.mean_bone_length(d["local"].astype(np.float32)).reshape(1, 15).contiguous()
    got = float(env.sequence_quality(seq_d, cams_d, heat_d, torch.zeros(1, dtype=torch.int64, device=env.device), mb, 1)[0, 0])
    with capsys.disabled():
        print("heat-map response: at the device's image points %.9g, the quality report %.9g" % (want, got))
    assert want > 0.05
    np.testing.assert_allclose(got, want, **RESPONSE_TOL)


# ------------------------------------------------------------------------------------------------------------------ 2. drawing
def draw_with_canaries(env, heat_d, uv_d, colours, view, gap=64):
    """gem_render_camera into a buffer with canaries around and between the images -> (images' bytes [n, image_bytes], ids, response)."""
    import torch
    from globalegomocap_amd import render as R
    lay = R.layout(view.size, view.size)
    n, stride = uv_d.shape[1], lay.stride + gap
    buf = torch.full((64 + n * stride + 64,), 0xA5, dtype=torch.uint8, device=env.device)
    out = buf[64:64 + n * stride].view(n, stride)
    assert out.data_ptr() % 16 == 0
    rgb = torch.tensor([_word(c) for c in colours], dtype=torch.int32).to(env.device)
    got, ids, response = env.render_camera(heat_d, uv_d, rgb, view, out=out, want_ids=True)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:64] == 0xA5).all() and (host[-64:] == 0xA5).all()
    rows = host[64:-64].reshape(n, stride)
    assert (rows[:, lay.image_bytes:] == 0xA5).all()
    return rows[:, :lay.image_bytes], ids.cpu().numpy(), response.cpu().numpy()


def pixels_of(rows, i, N):
    lines = rows[i].reshape(N, 1 + 3 * N)
    assert not lines[:, 0].any()
    return lines[:, 1:].reshape(N, N, 3)


def compare(rows, ids, response, want, N, what, response_atol=0.0):
    off = 0
    for i, im in enumerate(want):
        assert np.array_equal(ids[i], im.ids), (what, i, int((ids[i] != im.ids).sum()))
        err = float(np.abs(response[i] - im.response).max())
        print("%s, image %d: largest response difference to the twin %.3g" % (what, i, err))
        np.testing.assert_allclose(response[i], im.response, rtol=RESPONSE_TOL["rtol"], atol=RESPONSE_TOL["atol"] + response_atol)
        diff = np.abs(pixels_of(rows, i, N).astype(np.int64) - im.rgb.astype(np.int64)).max(-1)
        assert (diff[~im.near_round] == 0).all() and diff.max(initial=0) <= 1, (what, i, int((diff != 0).sum()))
        off += int((diff != 0).sum())
    print("%s: %d pixels one level off" % (what, off))


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("N,jr,lr", CASES)
def test_kernel_against_the_twin(env, N, jr, lr, S, capsys):
    import torch
    d = data()
    cams_d, heat_d = _dev(env, d["cams"]), _dev(env, d["heat"])
    uv_d = torch.stack([env.project_sequence(_dev(env, s), cams_d) for s in d["seqs"][:S]])
    uv = uv_d.cpu().numpy()          # the twin draws the very image points the device holds: float64 on identical inputs
    want = [T.render(d["heat"][f], uv[:, f], COLOURS[:S], N, 0x7FFF, HEAT, jr, lr) for f in range(F)]
    # the conditions on the inputs under which ids and bytes must be equal
    total = F * N * N
    assert not any(im.near_edge.any() for im in want), "a pixel centre within 1e-6 of a rim"
    assert sum(int(im.near_round.sum()) for im in want) <= 0.01 * total
    assert sum(int((im.ids >= 0).sum()) for im in want) >= 0.05 * total
    assert sum(int((im.response > 0.05).sum()) for im in want) >= 0.05 * total
    if S == 2:
        assert any((im.ids >= 30).any() for im in want) and any(((im.ids >= 0) & (im.ids < 30)).any() for im in want)
    if N == 19:          # the last band is 3 rows of 58 bytes = 174 = 10 * 16 + 14: its last 14 bytes are stored singly
        from globalegomocap_amd import render as R
        assert R.layout(19, 19) == (58, 1102, 1104) and (3 * 58) % 16 == 14
    rows, ids, response = draw_with_canaries(env, heat_d, uv_d, COLOURS[:S], _view(N, jr, lr))
    with capsys.disabled():
        # N = 32: the pixels' places are exact in fp32, the coordinates' rounding term is not needed
        compare(rows, ids, response, want, N, "%d x %d, %d sequence(s)" % (N, N, S), 0.0 if N == 32 else COORD_ULPS * d["D"])


# ------------------------------------------------------------------------------------------------------------------ 3. corners
def test_defined_corners(env, capsys):
    """Each against the twin, 32 x 32 pixels (their places are exact): a point that is not finite, two joints in one place (a line
    of no length), a primitive wholly outside the crop, two coincident sequences, a mask with one joint, a mask of 0, no heat-maps,
    radius 0."""
    import torch
    d = data()
    N, jr, lr = 32, 40.0, 16.0
    cams_d = _dev(env, d["cams"][:1])
    base = env.project_sequence(_dev(env, d["seqs"][0][:1]), cams_d).cpu().numpy()          # [1,15,2]
    heat, heat_d = d["heat"][0], _dev(env, d["heat"][:1])

    def both(uv, colours, view, with_heat=True, what=""):
        uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 1, 15, 2)
        rows, ids, response = draw_with_canaries(env, heat_d if with_heat else None, _dev(env, uv), colours, view, gap=32)
        want = T.render(heat if with_heat else None, uv[:, 0], colours, view.size, view.joint_mask, HEAT, view.joint_radius, view.line_radius)
        with capsys.disabled():
            compare(rows, ids, response, [want], view.size, "corner: " + what)
        return want

    nan = base.copy()
    nan[0, 1] = (np.nan, 500.0)
    nan[0, 9] = (600.0, -np.inf)
    w = both(nan, COLOURS[:1], _view(N, jr, lr), what="points that are not finite")
    assert not np.isin(w.ids, [1, 15, 17, 21, 9, 23, 24]).any() and (w.ids == 0).any()
    same = base.copy()
    same[0, 1] = same[0, 0]
    w = both(same, COLOURS[:1], _view(N, 10.0, 70.0), what="a line of no length")
    assert (w.ids == 15).any()          # the line (0, 1) is a disc of the line's radius about the shared point, beyond the joints' discs
    out = np.full((1, 15, 2), 3000.0, dtype=np.float32)
    out[0, 0], out[0, 1], out[0, 4] = (640.0, 500.0), (5000.0, 500.0), (-300.0, 2000.0)
    w = both(out, COLOURS[:1], _view(N, jr, lr), what="primitives outside the crop")
    assert set(np.unique(w.ids)) == {-1, 0, 15, 16}          # joints 1 and 4 are outside; their lines from joint 0 run through the crop
    w = both(np.stack([base, base]), COLOURS, _view(N, jr, lr), what="two coincident sequences")
    assert (w.ids >= 30).any() and not ((w.ids >= 0) & (w.ids < 30)).any() and (w.rgb[w.ids >= 0] == COLOURS[1]).all()
    w = both(base, COLOURS[:1], _view(N, jr, lr, mask=1 << 10), what="a mask with one joint")
    assert 0.05 < w.response.max() and (w.response > 0.05).sum() < 0.03 * N * N
    w = both(base, COLOURS[:1], _view(N, jr, lr, mask=0), what="a mask of 0")
    assert not w.response.any() and (w.rgb[w.ids < 0] == 255).all()
    w = both(base, COLOURS[:1], _view(N, jr, lr), with_heat=False, what="no heat-maps")
    assert not w.response.any() and (w.rgb[w.ids < 0] == 255).all() and (w.ids >= 0).any()
    centred = base.copy()
    centred[0, 0] = (128.0 + 32.0 * 10.5, 32.0 * 7.5)          # exactly a pixel's centre: radius 0 covers that pixel alone
    w = both(centred, COLOURS[:1], _view(N, 0.0, 0.0), what="radius 0")
    assert w.ids[7, 10] == 0 and (w.ids == 0).sum() == 1
    # no sequence at all: the background alone
    rows, ids, response = draw_with_canaries(env, heat_d, torch.empty(0, 1, 15, 2, device=env.device), (), _view(N, jr, lr))
    want = T.render(heat, np.empty((0, 15, 2), dtype=np.float32), (), N, 0x7FFF, HEAT, jr, lr)
    with capsys.disabled():
        compare(rows, ids, response, [want], N, "corner: no sequence")
    assert (ids == -1).all() and (response > 0.05).any()


# ------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_without_a_launch(env):
    import torch
    from globalegomocap_amd import _capi, render as R
    from globalegomocap_amd.skeleton import KINEMATIC_PARENTS
    lib, d = env.lib, data()
    N = 32
    lay = R.layout(N, N)
    heat_d = _dev(env, d["heat"][:2])
    uv_d = torch.stack([env.project_sequence(_dev(env, d["seqs"][0][:2]), _dev(env, d["cams"][:2]))])
    rgb = torch.tensor([_word(COLOURS[0])], dtype=torch.int32).to(env.device)
    buf = torch.full((2 * lay.stride + 256,), 0x5A, dtype=torch.uint8, device=env.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = _view(N, 40.0, 16.0)
    # a handle whose skeleton has 14 joints
    cfg = _capi.GemConfig()
    cfg.seq_len, cfg.n_joints, cfg.latent_dim, cfg.n_hidden = 10, 14, 64, 5
    for i, v in enumerate((16, 16, 32, 32, 64)):
        cfg.hidden[i] = v
    cfg.heat_h, cfg.heat_w, cfg.n_poly = 64, 64, len(env.camera.poly_w2c)
    for i, v in enumerate(env.camera.poly_w2c):
        cfg.poly[i] = v
    cfg.cx, cfg.cy = env.camera.cx, env.camera.cy
    for i, v in enumerate(KINEMATIC_PARENTS[:14]):
        cfg.parents[i] = v
    cfg.max_windows, cfg.device = 1, env.device.index
    other = C.c_void_p()
    _capi.check(lib.gem_create(C.byref(cfg), C.byref(other)), lib)

    def call(h=env._h, heat=heat_d, uv=uv_d, colours=rgb, S=1, n=2, view=good, base=0, stride=lay.stride, no_out=False):
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
        return lib.gem_render_camera(h, ptr(heat), ptr(uv), ptr(colours), S, n, C.byref(view) if view is not None else None,
                                     None if no_out else C.c_void_p(buf.data_ptr() + base), stride, None, None, st)
    try:
        for kw, word in ((dict(h=other), b"15 joints"), (dict(h=None), b"null handle"), (dict(view=None), b"null view"),
                         (dict(view=_view(0, 40.0, 16.0)), b"1 .. 1024"), (dict(view=_view(1025, 40.0, 16.0), stride=16 * 3100), b"1 .. 1024"),
                         (dict(view=_view(N, 40.0, 16.0, mask=1 << 15)), b"joint_mask"), (dict(view=_view(N, -1.0, 16.0)), b"radius"),
                         (dict(view=_view(N, 40.0, float("nan"))), b"radius"), (dict(view=_view(N, float("inf"), 16.0)), b"radius"),
                         (dict(S=-1), b"sequences"), (dict(S=9), b"sequences"), (dict(n=-1), b"images"), (dict(n=65536), b"images"),
                         (dict(base=8), b"aligned"), (dict(stride=lay.stride + 8), b"multiple of 16"),
                         (dict(stride=lay.image_bytes - 16), b"at least"), (dict(no_out=True), b"null argument"),
                         (dict(uv=None), b"null argument"), (dict(colours=None), b"null argument")):
            assert call(**kw) != 0 and word in lib.gem_last_error(), (kw, lib.gem_last_error())
        assert call(n=0) == 0 and call(n=0, uv=None, colours=None, no_out=True) == 0          # nothing to draw
        torch.cuda.synchronize()
        assert bool((buf == 0x5A).all())
        assert call() == 0
        torch.cuda.synchronize()
        assert not bool((buf[:lay.image_bytes] == 0x5A).any()) and bool((buf[2 * lay.stride:] == 0x5A).all())
        assert call(heat=None) == 0 and call(S=0, uv=None, colours=None) == 0          # a white background; no sequence: neither is needed
    finally:
        lib.gem_destroy(other)
    # the wrapper's own checks
    with pytest.raises(ValueError):
        env.render_camera(heat_d, uv_d, rgb, good, out=buf[:2 * (lay.image_bytes - 16)].view(2, lay.image_bytes - 16))
    with pytest.raises(TypeError):
        env.render_camera(heat_d, uv_d.double(), rgb, good)
    with pytest.raises(TypeError):
        env.render_camera(heat_d, uv_d, rgb.long(), good)
    with pytest.raises(ValueError):
        env.render_camera(heat_d[:1].contiguous(), uv_d, rgb, good)
    with pytest.raises(_capi.GemError, match="radius"):
        env.render_camera(heat_d, uv_d, rgb, _view(N, -1.0, 16.0))


# ------------------------------------------------------------------------------------------------------------------ 5. determinism
def test_two_calls_give_the_same_bytes(env):
    import torch
    from globalegomocap_amd import render as R
    d = data()
    lay = R.layout(96, 96)
    a = R.camera_scanlines(env, d["seqs"], d["cams"], d["heat"], COLOURS, size=96, joint_radius=20.0)
    b = R.camera_scanlines(env, d["seqs"], d["cams"], d["heat"], COLOURS, size=96, joint_radius=20.0)
    assert a.dtype == torch.uint8 and tuple(a.shape) == (F, lay.stride) and a.is_cuda and a.data_ptr() != b.data_ptr()
    assert torch.equal(a[:, :lay.image_bytes], b[:, :lay.image_bytes])
    drawn = a[:, :lay.image_bytes].view(F, 96, lay.row_bytes)[:, :, 1:]
    assert bool((drawn != 255).any()) and bool((drawn == 255).any())


# ------------------------------------------------------------------------------------------------------------------ 6. files
def _image_of(rows, k, N):
    return rows[k, :N * (1 + 3 * N)].reshape(N, 1 + 3 * N)[:, 1:].reshape(N, N, 3)


def _five_frames():
    from globalegomocap_amd import synth
    s = synth.make_sequence(n_frames=5, seed=SEED + 1, cam_jitter=(2.0, 0.01))
    cams = np.asarray(s["camera_pose_list"], dtype=np.float64)
    local = np.asarray(s["estimated_local_skeleton"], dtype=np.float64)
    est = np.einsum("nij,nkj->nki", cams[:, :3, :3], local) + cams[:, None, :3, 3]
    return s, cams, np.asarray(s["heatmap_list"], dtype=np.float32), est


def test_write_camera_frames_through_small_buffers(env, tmp_path, monkeypatch):
    """Five frames through pinned buffers of two images each: three batches, both buffers used again; the files read back equal
    `camera_scanlines`; then the command line on a pose pickle plus a chunk directory."""
    from globalegomocap_amd import render as R, synth
    N = 40
    s, cams, heat, est = _five_frames()
    seqs = [est, est + 0.02]
    monkeypatch.setattr(R, "PINNED_BYTES", 2 * R.layout(N, N).stride)
    R.release()
    try:
        out = str(tmp_path / "five")
        assert R.write_camera_frames(env, seqs, cams, heat, out, colours=COLOURS, size=N, joint_radius=30.0, line_radius=12.0) == 5
        assert sorted(os.listdir(out)) == ["camera_%04d.png" % f for f in range(5)]
        want = R.camera_scanlines(env, seqs, cams, heat, COLOURS, size=N, joint_radius=30.0, line_radius=12.0).cpu().numpy()
        for f in range(5):
            got = R.read_png(os.path.join(out, "camera_%04d.png" % f))
            assert np.array_equal(got, _image_of(want, f, N)), f
            assert (got != 255).any() and (got == np.array(COLOURS[1], dtype=np.uint8)).all(-1).any()
    finally:
        R.release()
    gt = (est[:4] * 1.1) @ _rotation((0.2, 1.0, 0.1), 0.4) + 0.5          # a ground truth in a frame of its own
    pkl = str(tmp_path / "result_pose.pkl")
    with open(pkl, "wb") as f:
        pickle.dump({"estimated_pose": list(est[:4]), "optimized_pose": est[:4] + 0.01, "gt_pose": list(gt)}, f)
    chunk = tmp_path / "studio" / "chunk_3"
    chunk.mkdir(parents=True)
    with open(str(chunk / "test_data.pkl"), "wb") as f:
        pickle.dump(synth.reference_pickle_dict(s), f)
    R.main([pkl, "--out", str(tmp_path / "cli"), "--camera", str(chunk), "--size", "48"])
    assert sorted(os.listdir(str(tmp_path / "cli"))) == ["camera_%04d.png" % f for f in range(4)]
    trio = [est[:4], est[:4] + 0.01, gt]
    want = R.camera_scanlines(env, trio, cams[:4], heat[:4], list(R.PALETTE.values()), size=48, align_to=[None, None, est[:4] + 0.01]).cpu().numpy()
    got = R.read_png(str(tmp_path / "cli" / "camera_0002.png"))
    assert np.array_equal(got, _image_of(want, 2, 48)) and (got == np.array(R.PALETTE["gt"], dtype=np.uint8)).all(-1).any()
    with open(pkl, "wb") as f:
        pickle.dump({"estimated_pose": list(np.concatenate([est, est])), "optimized_pose": np.concatenate([est, est])}, f)
    with pytest.raises(SystemExit):          # more poses than the chunk has frames
        R.main([pkl, "--out", str(tmp_path / "cli2"), "--camera", str(chunk)])
    R.release()


# ------------------------------------------------------------------------------------------------------------------ 7. end to end
@pytest.fixture
def small_images(monkeypatch):
    """The pipeline's images are small where it asks for the default sizes."""
    from globalegomocap_amd import render as R
    monkeypatch.setattr(R, "DEFAULT_SIZE", IMG)
    monkeypatch.setattr(R, "CAMERA_SIZE", CAMERA_N)


@pytest.fixture(scope="module")
def chunk_dirs(env, golden, tmp_path_factory):
    """One chunk of 26 frames with ground truth and the same without, as pickles under <tmp>/with_gt/studio and <tmp>/no_gt/studio."""
    from globalegomocap_amd import prepare as P
    from helpers import sd_from_npz
    tmp = tmp_path_factory.mktemp("camera")
    n = SIZE + 1
    hd, dd, traj, gtp = _write_recording(tmp / "rec", n, seed=23)
    with_gt = P.prepare_sequence(traj, hd, dd, gtp, 0, n, fps=25, test_size=SIZE, verbose=False)
    no_gt = P.prepare_sequence(traj, hd, dd, None, 0, n, fps=25, test_size=SIZE, verbose=False, scale=1.7)
    assert len(with_gt) == len(no_gt) == 1
    with_gt.write_chunks(str(tmp / "with_gt" / "studio"))
    no_gt.write_chunks(str(tmp / "no_gt" / "studio"))
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False)
    return dict(tmp=tmp, kw=kw, name=with_gt.chunks[0].name)


def _chunk_frames(root, name):
    from globalegomocap_amd import whole_sequence as ws
    c = ws.parse_chunk(os.path.join(root, name), native=False, ground_truth=False)
    return c["cams"], np.asarray(c["heat_list"], dtype=np.float32)


@pytest.mark.parametrize("ground_truth", [True, False], ids=["with ground truth", "without ground truth"])
def test_camera_view_from_the_pipeline(env, chunk_dirs, small_images, ground_truth):
    import torch
    from globalegomocap_amd import whole_sequence as ws
    tmp, kw = chunk_dirs["tmp"], dict(chunk_dirs["kw"], ground_truth=ground_truth)
    root = str(tmp / ("with_gt" if ground_truth else "no_gt") / "studio")
    out = tmp / ("c_%d" % ground_truth)
    torch.manual_seed(31)
    off = ws.optimize_directory(root, DEFAULT_CALIBRATION, **kw)
    assert not out.exists()
    torch.manual_seed(31)
    on = ws.optimize_directory(root, DEFAULT_CALIBRATION, render_camera=str(out), **kw)
    _same_bits(on, off)
    assert os.listdir(str(out)) == ["studio"] and os.listdir(str(out / "studio")) == [chunk_dirs["name"]]
    assert on[2].shape == on[3].shape == (SIZE, 15, 3) and (on[4] is None) == (not ground_truth)
    cams, heat = _chunk_frames(root, chunk_dirs["name"])
    got = _check_camera_tree(env, str(out / "studio" / chunk_dirs["name"]), on[2], on[3], on[4], cams, heat)
    assert ((got == np.array((44, 160, 44), dtype=np.uint8)).all(-1).any()) == ground_truth          # the ground truth is drawn, in the cameras' frame


def test_render_alone_writes_what_it_wrote(env, chunk_dirs, small_images):
    """`render=DIR` with and without `render_camera=DIR` (the same DIR): the same frame files byte for byte, the camera's views
    beside them only when asked for."""
    import torch
    from globalegomocap_amd import whole_sequence as ws
    tmp, kw = chunk_dirs["tmp"], dict(chunk_dirs["kw"], ground_truth=False)
    root = str(tmp / "no_gt" / "studio")
    alone, both = tmp / "alone", tmp / "both"
    torch.manual_seed(31)
    a = ws.optimize_directory(root, DEFAULT_CALIBRATION, render=str(alone), **kw)
    torch.manual_seed(31)
    b = ws.optimize_directory(root, DEFAULT_CALIBRATION, render=str(both), render_camera=str(both), **kw)
    _same_bits(a, b)
    frames = sorted(["frame_%04d.png" % f for f in range(SIZE)] + ["overview_estimated.png", "overview_optimized.png"])
    d_alone, d_both = alone / "studio" / chunk_dirs["name"], both / "studio" / chunk_dirs["name"]
    assert sorted(os.listdir(str(d_alone))) == frames
    for name in frames:
        assert (d_alone / name).read_bytes() == (d_both / name).read_bytes(), name
    cams, heat = _chunk_frames(root, chunk_dirs["name"])
    _check_camera_tree(env, str(d_both), b[2], b[3], None, cams, heat, others=frames)


def test_main_writes_the_camera_view(env, chunk_dirs, small_images, tmp_path, monkeypatch):
    """optimizer.main(render_camera=DIR): DIR/<dataset>/<chunk>/camera_%04d.png from the pickle it loaded, every returned value what
    it is without it."""
    import torch
    from globalegomocap_amd import optimizer as gopt, synth
    data_ = synth.make_sequence(n_frames=SIZE, seed=9)
    d = tmp_path / "studio-x" / "chunk_7"
    d.mkdir(parents=True)
    with open(str(d / "test_data.pkl"), "wb") as f:
        pickle.dump(synth.reference_pickle_dict(data_), f)
    monkeypatch.chdir(tmp_path)
    kw = {k: chunk_dirs["kw"][k] for k in ("global_vae_path", "local_vae_path")}
    args = (str(d), DEFAULT_CALIBRATION, 0.0, 0.0, 0.001, 0.01, 0.01, 0.01)
    eps = torch.randn(6, 32, generator=torch.Generator().manual_seed(5))
    off = gopt.main(*args, final_smooth=True, eps=eps, **kw)
    on = gopt.main(*args, final_smooth=True, render_camera=str(tmp_path / "seen"), eps=eps, **kw)
    assert not (tmp_path / "out").exists()
    assert list(on[0]) == list(off[0])
    for k in on[0]:
        assert np.array_equal(np.asarray(on[0][k]), np.asarray(off[0][k])), k
    for i in (1, 2, 3, 4):
        assert np.array_equal(np.asarray(on[i]), np.asarray(off[i])), i
    assert os.listdir(str(tmp_path / "seen")) == ["studio-x"]
    got = _check_camera_tree(env, str(tmp_path / "seen" / "studio-x" / "chunk_7"), np.asarray(on[1]), np.asarray(on[3]), np.asarray(on[4]),
                             np.asarray(data_["camera_pose_list"]), np.asarray(data_["heatmap_list"], dtype=np.float32))
    tinted = (got[..., 0] >= 148) & (got[..., 0] < 255) & (got[..., 2] >= 189) & (got[..., 2] < 255)          # (no skeleton colour has that much blue)
    assert (got == np.array((31, 119, 180), dtype=np.uint8)).all(-1).any() and tinted.any()


SHORT = 18          # frames of the shorter second chunk: two windows


@pytest.fixture(scope="module")
def two_chunk_dirs(env, golden, tmp_path_factory):
    """Two chunks of one recording as pickles: <tmp>/equal/studio with 26 and 26 frames, <tmp>/unequal/studio with 26 and the first
    18 of the second."""
    from globalegomocap_amd import prepare as P
    from helpers import sd_from_npz
    tmp = tmp_path_factory.mktemp("outputs")
    n = 2 * SIZE + 1
    hd, dd, traj, gtp = _write_recording(tmp / "rec", n, seed=23)
    rec = P.prepare_sequence(traj, hd, dd, gtp, 0, n, fps=25, test_size=SIZE, verbose=False)
    assert len(rec) == 2
    names = [c.name for c in rec.chunks]
    rec.write_chunks(str(tmp / "equal" / "studio"))
    rec.write_chunk(0, str(tmp / "unequal" / "studio" / names[0]))
    os.makedirs(str(tmp / "unequal" / "studio" / names[1]))
    with open(str(tmp / "unequal" / "studio" / names[1] / "test_data.pkl"), "wb") as f:
        pickle.dump({k: v[:SHORT] for k, v in rec.chunk_dict(1).items()}, f)
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False)
    return dict(tmp=tmp, kw=kw, names=names)


@pytest.mark.parametrize("lengths", [(SIZE, SIZE), (SIZE, SHORT)], ids=["equal chunks: batched report", "unequal chunks: per-chunk report"])
def test_every_output_of_two_chunks(env, two_chunk_dirs, small_images, lengths):
    """One call with `save`, `render`, `render_camera` and `save_pose` on a directory of two chunks: the result is bit for bit that of
    the call without them, and every chunk's files -- the second's too, whose sequences and frames lie behind the first's in the
    batch's buffers -- hold that chunk's slices of the returned sequences, its camera views over its own cameras and heat-maps."""
    import torch
    from globalegomocap_amd import whole_sequence as ws
    from globalegomocap_amd.errors import align_sequence
    tmp, kw, names = two_chunk_dirs["tmp"], two_chunk_dirs["kw"], two_chunk_dirs["names"]
    case = "equal" if lengths[0] == lengths[1] else "unequal"
    root = str(tmp / case / "studio")
    out = {k: tmp / ("%s_%s" % (case, k)) for k in ("mesh", "frames", "camera", "pose")}
    torch.manual_seed(31)
    off = ws.optimize_directory(root, DEFAULT_CALIBRATION, **kw)
    assert not any(p.exists() for p in out.values())
    torch.manual_seed(31)
    on = ws.optimize_directory(root, DEFAULT_CALIBRATION, save=True, mesh_root=str(out["mesh"]), render=str(out["frames"]),
                               render_camera=str(out["camera"]), save_pose=str(out["pose"]), **kw)
    _same_bits(on, off)
    assert len(on[1]) == 2 and on[2].shape == on[3].shape == on[4].shape == (sum(lengths), 15, 3)
    for k in ("mesh", "frames", "camera"):
        assert os.listdir(str(out[k])) == ["studio"] and sorted(os.listdir(str(out[k] / "studio"))) == sorted(names), k
    assert sorted(os.listdir(str(out["pose"]))) == sorted(names)
    lo = 0
    for name, n in zip(names, lengths):
        est, opt, gt = (on[i][lo:lo + n] for i in (2, 3, 4))
        lo += n
        base = out["mesh"] / "studio" / name
        assert sorted(os.listdir(str(base))) == ["gt_global_aligned", "input_global_aligned", "optimized_global_aligned"]
        check_folder(str(base / "optimized_global_aligned"), align_sequence(opt, gt))
        check_folder(str(base / "input_global_aligned"), align_sequence(est, gt))
        check_folder(str(base / "gt_global_aligned"), gt)
        check_tree(env, str(out["frames"] / "studio" / name), est, opt, gt)
        c = ws.load_chunk(os.path.join(root, name))
        assert c["n"] == n
        _check_camera_tree(env, str(out["camera"] / "studio" / name), est, opt, gt, c["cams"], c["heat"])
        assert os.listdir(str(out["pose"] / name)) == ["result_pose.pkl"]
        with open(str(out["pose"] / name / "result_pose.pkl"), "rb") as f:
            saved = pickle.load(f)
        assert list(saved) == ["estimated_pose", "optimized_pose", "mid_optimized_pose", "gt_pose"]
        assert isinstance(saved["estimated_pose"], list) and isinstance(saved["optimized_pose"], np.ndarray) and isinstance(saved["gt_pose"], list)
        for key, want in (("estimated_pose", est), ("optimized_pose", opt), ("gt_pose", gt)):
            assert np.array_equal(np.asarray(saved[key]), want), (name, key)
        assert np.asarray(saved["mid_optimized_pose"]).shape == (n, 15, 3)
