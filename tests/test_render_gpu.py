"""Rendered frames on the device: gem_skeleton_capsules and gem_render_capsules against the numpy twin
(tests/render_twin.py) -- ids first, then depth, then the scanline bytes -- the defined corners, the refusals, determinism,
`render.write_frames` through small pinned buffers, and `render=DIR` end to end: the batch pipeline with and without ground truth,
`optimizer.main`, and that nothing else changes with it."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

import render_twin as T
from pipeline_checks import IMG, SIZE, check_tree as _check_tree, same_bits as _same_bits, write_recording as _write_recording
from globalegomocap_amd.camera import DEFAULT_CALIBRATION

pytestmark = pytest.mark.gpu

DEPTH_ATOL = 1e-9          # metres (the issue's bound; float64 rounding of metre-sized coordinates is 1e-16)
GEOM_ATOL = 1e-12          # metres: the project's float64 tolerance (test_meshes_gpu.ATOL)
F = 3
SEEDS = (9, 12)
COLOURS = ((214, 39, 40), (31, 119, 180))
HALF_WIDTH = 0.12          # metres: the zoom at which 2 cm spheres and 5 mm lines cover a tenth of a 37 x 24 image
SIZES = ((37, 24), (40, 32))


def _rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


CRT = (1.3, _rotation((1.0, 2.0, -1.0), 0.7), np.array([0.1, -0.2, 0.3]))


def synth_poses(n, seed):
    """`synth` poses in a world frame, as test_meshes_gpu draws them."""
    from globalegomocap_amd import synth
    s = synth.make_sequence(n_frames=n, seed=seed, with_heatmaps=False)
    return np.asarray(s["estimated_local_skeleton"], dtype=np.float64) @ _rotation((1.0, 0.3, 0.2), 1.0) + np.array([0.3, 1.2, -0.4])


def moved(seq, crt):
    return seq if crt is None else crt[0] * (seq @ crt[1]) + crt[2]


def make_scene(W, H, S, with_crt):
    """Sequences, similarities, the view (fit_view, zoomed in until the figure fills the image) and the twin's capsule lists: one
    per frame (all sequences overlaid), one per sequence (all its frames), and one with everything."""
    from globalegomocap_amd import render as R
    seqs = [synth_poses(F, seed) for seed in SEEDS[:S]]
    crts = [CRT if with_crt else None for i in range(S)]
    drawn = [moved(s, c) for s, c in zip(seqs, crts)]
    view = R.fit_view(drawn, W, H)
    view.half_width = HALF_WIDTH
    for i in range(3):          # ... about the neck and the shoulders of the first frame
        view.centre[i] = float(drawn[0][0, [0, 1, 4], i].mean())
    frames = [sum((T.frame_capsules(seqs[s][f], COLOURS[s], crts[s]) for s in range(S)), []) for f in range(F)]
    overviews = [sum((T.frame_capsules(seqs[s][f], COLOURS[s], crts[s]) for f in range(F)), []) for s in range(S)]
    return dict(seqs=seqs, crts=crts, view=view, frames=frames, overviews=overviews, everything=[sum(frames, [])])


def assert_generic_axes(caps, view):
    """No line nearer than 0.02 rad to `forward` (the cylinder's entry is well conditioned) and none shorter than 1 cm."""
    for a, b, r, _ in caps:
        d = np.asarray(b) - np.asarray(a)
        h = np.linalg.norm(d)
        if h == 0.0:
            continue
        assert h > 0.01 and np.sqrt(max(0.0, 1.0 - (d @ view.forward / h) ** 2)) >= 0.02, (a, b)


def twin_images(lists, view):
    tv = T.view_of(view)
    out = []
    for caps in lists:
        assert_generic_axes(caps, tv)
        out.append(T.render(caps, tv))
    return out


def assert_comparable(images):
    """The conditions on the inputs under which ids and bytes must be equal: no pixel on a silhouette or a tie, at most 1 % of the
    covered pixels on a rounding edge, at least 10 % of all pixels covered."""
    covered = sum(int(im.covered.sum()) for im in images)
    total = sum(im.covered.size for im in images)
    assert not any(im.near_silhouette.any() for im in images), "a pixel within 1e-7 m of a silhouette"
    assert not any(im.near_tie.any() for im in images), "two hits within 1e-7 m"
    assert sum(int(im.near_round.sum()) for im in images) <= 0.01 * covered
    assert covered >= 0.1 * total, (covered, total)


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import prepare
    return prepare._lift_engine(DEFAULT_CALIBRATION, 0)


def _crt_tensor(crt, dev):
    import torch
    return None if crt is None else torch.from_numpy(np.concatenate([[crt[0]], crt[1].reshape(-1), crt[2]])).to(dev)


def _word(c):
    return c[0] | (c[1] << 8) | (c[2] << 16)


def device_scene(env, scene):
    """geometry [S,F,30,7] and colours [S,F,30] of the scene's sequences from gem_skeleton_capsules."""
    import torch
    parts = [env.skeleton_capsules(torch.from_numpy(s.copy()).to(env.device), _crt_tensor(c, env.device), _word(col), _word(col))
             for s, c, col in zip(scene["seqs"], scene["crts"], COLOURS)]
    return torch.stack([p[0].view(F, 30, 7) for p in parts]), torch.stack([p[1].view(F, 30) for p in parts])


def device_capsules(caps, dev):
    import torch
    geom = np.array([np.concatenate([a, b, [r]]) for a, b, r, _ in caps], dtype=np.float64).reshape(-1, 7)
    rgb = np.array([_word(c) for _, _, _, c in caps], dtype=np.int32)
    return torch.from_numpy(geom).to(dev), torch.from_numpy(rgb).to(dev)


def check_images(env, geom, rgb, first, view, want, what, gap=0):
    """Render with canaries around and between the images and compare with the twin's images `want`."""
    import torch
    from globalegomocap_amd import render as R
    lay = R.layout(view.width, view.height)
    n, stride = len(want), lay.stride + gap
    buf = torch.full((64 + n * stride + 64,), 0xA5, dtype=torch.uint8, device=env.device)
    out = buf[64:64 + n * stride].view(n, stride)
    assert out.data_ptr() % 16 == 0
    got, ids, depth = env.render_capsules(geom, rgb, first, view, out=out, want_ids=True)
    assert got.data_ptr() == out.data_ptr()
    host, ids, depth = buf.cpu().numpy(), ids.cpu().numpy(), depth.cpu().numpy()
    assert (host[:64] == 0xA5).all() and (host[-64:] == 0xA5).all(), what
    rows = host[64:-64].reshape(n, stride)
    assert (rows[:, lay.image_bytes:] == 0xA5).all(), what
    worst, off = 0.0, 0
    for i, im in enumerate(want):
        assert np.array_equal(ids[i], im.ids), (what, i, int((ids[i] != im.ids).sum()))
        assert np.array_equal(np.isinf(depth[i]), ~im.covered), (what, i)
        if im.covered.any():
            worst = max(worst, float(np.abs(depth[i][im.covered] - im.depth[im.covered]).max()))
        lines = rows[i, :lay.image_bytes].reshape(view.height, lay.row_bytes)
        assert not lines[:, 0].any(), (what, i)
        px = lines[:, 1:].reshape(view.height, view.width, 3).astype(np.int64)
        diff = np.abs(px - im.rgb.astype(np.int64)).max(-1)
        assert (diff[~im.near_round] == 0).all() and diff.max(initial=0) <= 1, (what, i, int((diff != 0).sum()))
        off += int((diff != 0).sum())
    print("%s: largest depth difference to the twin %.3g m, %d pixels one level off" % (what, worst, off))
    assert worst <= DEPTH_ATOL, (what, worst)
    return rows[:, :lay.image_bytes]


_twins = {}


def twin_of(W, H, S, with_crt):
    """The scene and the twin's images of it: computed once per case, never changed."""
    key = (W, H, S, with_crt)
    if key not in _twins:
        scene = make_scene(W, H, S, with_crt)
        images = {k: twin_images(scene[k], scene["view"]) for k in ("frames", "overviews", "everything")}
        assert_comparable(images["frames"])
        assert_comparable(images["overviews"])
        assert_comparable(images["everything"])
        _twins[key] = (scene, images)
    return _twins[key]


@pytest.mark.parametrize("with_crt", [False, True], ids=["plain", "behind a similarity"])
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("W,H", SIZES)
def test_kernel_against_the_twin(env, W, H, S, with_crt, capsys):
    import torch
    from globalegomocap_amd import render as R
    scene, images = twin_of(W, H, S, with_crt)
    geom, rgb = device_scene(env, scene)
    want = np.array([np.concatenate([a, b, [r]]) for caps in scene["overviews"] for a, b, r, _ in caps]).reshape(S, F, 30, 7)
    np.testing.assert_allclose(geom.cpu().numpy(), want, rtol=0, atol=GEOM_ATOL)
    assert np.array_equal(rgb.cpu().numpy(), np.array([[[_word(c)] * 30] * F for c in COLOURS[:S]]))
    what = "%d x %d, %d sequence(s)%s" % (W, H, S, ", crt" if with_crt else "")
    by_frame = (geom.permute(1, 0, 2, 3).reshape(-1, 7).contiguous(), rgb.permute(1, 0, 2).reshape(-1).contiguous())
    with capsys.disabled():
        check_images(env, *by_frame, [30 * S * f for f in range(F + 1)], scene["view"], images["frames"], what + ", frames", gap=64)
        check_images(env, geom.reshape(-1, 7), rgb.reshape(-1), [30 * F * s for s in range(S + 1)], scene["view"], images["overviews"],
                     what + ", overviews")
        rows = check_images(env, *by_frame, [0, 30 * S * F], scene["view"], images["everything"], what + ", everything in one image")
    if not with_crt:          # the module's own route to the same bytes
        lay = R.layout(W, H)
        got = R.scanlines(env, scene["seqs"], scene["view"], COLOURS[:S], overview=True)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (S, lay.stride) and got.is_cuda
        again = env.render_capsules(geom.reshape(-1, 7), rgb.reshape(-1), [30 * F * s for s in range(S + 1)], scene["view"])
        assert torch.equal(got[:, :lay.image_bytes], again[:, :lay.image_bytes])
        assert rows.shape == (1, lay.image_bytes)


def test_a_last_band_that_ends_between_two_stores(env, capsys):
    """40 x 19: the last band is 3 rows of 121 bytes = 363 = 22 * 16 + 11, so its last 11 bytes are stored singly."""
    from globalegomocap_amd import render as R
    scene = make_scene(40, 19, 1, False)
    images = twin_images(scene["frames"], scene["view"])
    assert_comparable(images)
    assert R.layout(40, 19) == (121, 2299, 2304) and (3 * 121) % 16 == 11
    geom, rgb = device_scene(env, scene)
    with capsys.disabled():
        check_images(env, geom.permute(1, 0, 2, 3).reshape(-1, 7).contiguous(), rgb.permute(1, 0, 2).reshape(-1).contiguous(),
                     [30 * f for f in range(F + 1)], scene["view"], images, "40 x 19", gap=16)


def axis_view(W, H, half_width, centre=(0.0, 0.0, 0.0)):
    """A view along +z with x to the right and y down: projections are exact."""
    from globalegomocap_amd import _capi
    v = _capi.GemView()
    for name, vec in (("right", (1, 0, 0)), ("down", (0, 1, 0)), ("forward", (0, 0, 1)), ("centre", centre)):
        for i in range(3):
            getattr(v, name)[i] = float(vec[i])
    v.half_width, v.width, v.height = half_width, W, H
    return v


def test_defined_corners(env, capsys):
    """A bone along `forward` (both ways round), a bone of no length, two capsules that coincide, a capsule wholly outside the image,
    one with a NaN, and an image whose range is empty -- each against the twin."""
    red, blue, green = (214, 39, 40), (31, 119, 180), (44, 160, 44)
    p = lambda *x: np.array(x, dtype=np.float64)          # noqa: E731
    view = axis_view(40, 32, 0.1)
    along = [(p(-0.04, 0.0, 0.5), p(-0.04, 0.0, 0.25), 0.02, red), (p(0.04, 0.0, -0.3), p(0.04, 0.0, 0.1), 0.015, blue)]
    no_length = [(p(0.0, 0.03, 0.2), p(0.0, 0.03, 0.2), 0.005, green), (p(0.01, -0.02, 0.2), p(0.05, -0.03, 0.1), 0.005, red)]
    twice = [(p(-0.05, -0.03, 0.3), p(0.05, 0.02, 0.1), 0.01, red), (p(0.0, 0.0, 0.0), p(0.0, 0.0, 0.0), 0.02, green),
             (p(-0.05, -0.03, 0.3), p(0.05, 0.02, 0.1), 0.01, blue), (p(0.0, 0.0, 0.0), p(0.0, 0.0, 0.0), 0.02, blue)]
    outside = [(p(0.5, 0.5, 0.0), p(0.6, 0.5, 0.0), 0.02, red), (p(0.0, 0.0, 1.0), p(0.03, 0.01, 1.0), 0.02, green),
               (p(0.0, np.nan, 0.0), p(0.0, 0.0, 0.0), 0.05, blue)]
    lists = [along, no_length, twice, outside, []]
    want = [T.render(c, T.view_of(view)) for c in lists]
    assert set(np.unique(want[0].ids)) == {-1, 0, 1} and set(np.unique(want[1].ids)) == {-1, 0, 1}
    assert set(np.unique(want[2].ids)) == {-1, 0, 1} and np.array_equal(want[2].near_tie, want[2].covered)
    assert set(np.unique(want[3].ids)) == {-1, 1} and not want[4].covered.any() and (want[4].rgb == 255).all()
    # the nearer end of a bone along `forward` is the one with the smaller depth, whichever is listed first
    assert np.isclose(want[0].depth[want[0].ids == 0].min(), 0.25 - 0.02, atol=1e-3) and np.isclose(want[0].depth[want[0].ids == 1].min(), -0.3 - 0.015, atol=1e-3)
    geom, rgb = device_capsules(sum(lists, []), env.device)
    first = np.cumsum([0] + [len(c) for c in lists])
    with capsys.disabled():
        check_images(env, geom, rgb, first, view, want, "corners", gap=32)


def test_refusals_without_a_launch(env):
    import torch
    from globalegomocap_amd import _capi, render as R
    lib = env.lib
    view = axis_view(40, 32, 0.1)
    lay = R.layout(40, 32)
    geom, rgb = device_capsules([(np.zeros(3), np.zeros(3), 0.05, (1, 2, 3))] * 2, env.device)
    buf = torch.full((2 * lay.stride + 256,), 0x5A, dtype=torch.uint8, device=env.device)
    up = torch.tensor([0, 1, 2], dtype=torch.int32, device=env.device)
    down = torch.tensor([0, 2, 1], dtype=torch.int32, device=env.device)
    past = torch.tensor([0, 1, 3], dtype=torch.int32, device=env.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    skewed = axis_view(40, 32, 0.1)
    skewed.right[1] = 1e-6
    long = axis_view(40, 32, 0.1)
    long.forward[2] = 1.0 + 1e-6
    flat = axis_view(40, 0, 0.1)
    wide = axis_view(1025, 32, 0.1)

    def call(first, v, base, stride):
        return lib.gem_render_capsules(C.c_void_p(geom.data_ptr()), C.c_void_p(rgb.data_ptr()), 2, C.c_void_p(first.data_ptr()), 2, C.byref(v),
                                       C.c_void_p(buf.data_ptr() + base), stride, None, None, st)
    for first, v, base, stride, word in ((up, view, 8, lay.stride, b"aligned"), (up, view, 0, lay.stride + 8, b"multiple of 16"),
                                         (up, view, 0, lay.image_bytes - 16, b"at least"), (down, view, 0, lay.stride, b"ascending"),
                                         (past, view, 0, lay.stride, b"leaves"), (up, skewed, 0, lay.stride, b"orthonormal"),
                                         (up, long, 0, lay.stride, b"orthonormal"), (up, flat, 0, lay.stride, b"at least 1"),
                                         (up, wide, 0, 16 * 3100, b"1024")):
        assert call(first, v, base, stride) != 0 and word in lib.gem_last_error(), word
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())
    assert call(up, view, 0, lay.stride) == 0
    torch.cuda.synchronize()
    assert not bool((buf[:lay.image_bytes] == 0x5A).all()) and bool((buf[2 * lay.stride:] == 0x5A).all())
    with pytest.raises(_capi.GemError, match="ascending"):
        env.render_capsules(geom, rgb, [0, 2, 1], view)
    with pytest.raises(ValueError):
        env.render_capsules(geom, rgb, [0, 1, 2], view, out=buf[:2 * (lay.image_bytes - 16)].view(2, lay.image_bytes - 16))
    with pytest.raises(TypeError):
        env.render_capsules(geom.float(), rgb, [0, 1, 2], view)
    with pytest.raises(TypeError):
        env.skeleton_capsules(torch.zeros(2, 15, 3, device=env.device))
    with pytest.raises(ValueError):
        env.skeleton_capsules(torch.zeros(2, 14, 3, device=env.device, dtype=torch.float64))


def test_two_calls_give_the_same_bytes(env):
    import torch
    from globalegomocap_amd import render as R
    seqs = [synth_poses(5, seed) for seed in SEEDS]
    view = R.fit_view(seqs, 64, 48)
    for overview in (False, True):
        a = R.scanlines(env, seqs, view, COLOURS, overview=overview)
        b = R.scanlines(env, seqs, view, COLOURS, overview=overview)
        lay = R.layout(64, 48)
        assert tuple(a.shape) == ((2 if overview else 5), lay.stride) and torch.equal(a[:, :lay.image_bytes], b[:, :lay.image_bytes])
        drawn = a[:, :lay.image_bytes].view(a.shape[0], 48, lay.row_bytes)[:, :, 1:]
        assert bool((drawn != 255).any()) and bool((drawn == 255).any())


def _image_of(rows, k, W, H):
    return rows[k, :H * (1 + 3 * W)].reshape(H, 1 + 3 * W)[:, 1:].reshape(H, W, 3)


def test_write_frames_through_small_buffers(env, tmp_path, monkeypatch):
    """Five frames through pinned buffers of two images each: three batches, both buffers used again; files read back by the module's
    reader and by the twin's equal `scanlines`; the CLI on a pose pickle."""
    from globalegomocap_amd import render as R
    W, H = 40, 32
    seqs = [synth_poses(5, seed) for seed in SEEDS]
    monkeypatch.setattr(R, "PINNED_BYTES", 2 * R.layout(W, H).stride)
    R.release()
    try:
        out = str(tmp_path / "five")
        assert R.write_frames(env, seqs, out, colours=COLOURS, size=(W, H), names=("a", "b")) == 7
        assert sorted(os.listdir(out)) == ["frame_%04d.png" % f for f in range(5)] + ["overview_a.png", "overview_b.png"]
        view = R.frames_view(env, seqs, size=(W, H))
        frames = R.scanlines(env, seqs, view, COLOURS).cpu().numpy()
        overviews = R.scanlines(env, seqs, view, COLOURS, overview=True).cpu().numpy()
        for f in range(5):
            got = R.read_png(os.path.join(out, "frame_%04d.png" % f))
            assert np.array_equal(got, _image_of(frames, f, W, H)), f
            assert np.array_equal(T.read_png(os.path.join(out, "frame_%04d.png" % f)), got)
        for k, name in enumerate("ab"):
            assert np.array_equal(R.read_png(os.path.join(out, "overview_%s.png" % name)), _image_of(overviews, k, W, H)), name
        assert all((_image_of(frames, f, W, H) != 255).any() for f in range(5))
    finally:
        R.release()
    pkl = str(tmp_path / "result_pose.pkl")
    with open(pkl, "wb") as f:
        pickle.dump({"estimated_pose": list(seqs[0][:2]), "optimized_pose": seqs[0][:2] + 0.01, "gt_pose": list(seqs[0][:2] * 1.1)}, f)
    R.main([pkl, "--out", str(tmp_path / "cli"), "--align", "true", "--size", "32x24", "--view", "front"])
    names = ["frame_0000.png", "frame_0001.png", "overview_estimated.png", "overview_gt.png", "overview_optimized.png"]
    assert sorted(os.listdir(str(tmp_path / "cli"))) == names
    gt = seqs[0][:2] * 1.1
    trio = [seqs[0][:2], seqs[0][:2] + 0.01, gt]
    view = R.frames_view(env, trio, align_to=[gt, gt, None], size=(32, 24), view="front")
    want = R.scanlines(env, trio, view, list(R.PALETTE.values()), align_to=[gt, gt, None]).cpu().numpy()
    assert np.array_equal(R.read_png(str(tmp_path / "cli" / "frame_0001.png")), _image_of(want, 1, 32, 24))
    R.release()


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture
def small_images(monkeypatch):
    """`write_result_frames` draws 64 x 48 images where the pipeline asks for its default size."""
    from globalegomocap_amd import render as R
    monkeypatch.setattr(R, "DEFAULT_SIZE", IMG)


@pytest.fixture(scope="module")
def chunk_dirs(env, golden, tmp_path_factory):
    """One chunk of 26 frames with ground truth and the same without, as pickles under <tmp>/with_gt/studio and <tmp>/no_gt/studio."""
    from globalegomocap_amd import prepare as P
    from helpers import sd_from_npz
    tmp = tmp_path_factory.mktemp("frames")
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


@pytest.mark.parametrize("ground_truth", [True, False], ids=["with ground truth", "without ground truth"])
def test_render_from_the_pipeline(env, chunk_dirs, small_images, monkeypatch, ground_truth):
    import torch
    from globalegomocap_amd import whole_sequence as ws
    tmp, kw = chunk_dirs["tmp"], dict(chunk_dirs["kw"], ground_truth=ground_truth)
    root = str(tmp / ("with_gt" if ground_truth else "no_gt") / "studio")
    out = tmp / ("r_%d" % ground_truth)
    torch.manual_seed(31)
    off = ws.optimize_directory(root, DEFAULT_CALIBRATION, **kw)
    assert not out.exists()
    torch.manual_seed(31)
    on = ws.optimize_directory(root, DEFAULT_CALIBRATION, render=str(out), **kw)
    _same_bits(on, off)
    assert os.listdir(str(out)) == ["studio"] and os.listdir(str(out / "studio")) == [chunk_dirs["name"]]
    assert on[2].shape == on[3].shape == (SIZE, 15, 3) and (on[4] is None) == (not ground_truth)
    _check_tree(env, str(out / "studio" / chunk_dirs["name"]), on[2], on[3], on[4])


def test_main_renders_under_the_given_root(env, chunk_dirs, small_images, tmp_path, monkeypatch):
    """optimizer.main(render=DIR): DIR/<dataset>/<chunk>/..., every returned value what it is without it."""
    import torch
    from globalegomocap_amd import optimizer as gopt, synth
    data = synth.make_sequence(n_frames=SIZE, seed=9)
    d = tmp_path / "studio-x" / "chunk_7"
    d.mkdir(parents=True)
    with open(str(d / "test_data.pkl"), "wb") as f:
        pickle.dump(synth.reference_pickle_dict(data), f)
    monkeypatch.chdir(tmp_path)
    kw = {k: chunk_dirs["kw"][k] for k in ("global_vae_path", "local_vae_path")}
    args = (str(d), DEFAULT_CALIBRATION, 0.0, 0.0, 0.001, 0.01, 0.01, 0.01)
    eps = torch.randn(6, 32, generator=torch.Generator().manual_seed(5))
    off = gopt.main(*args, final_smooth=True, eps=eps, **kw)
    on = gopt.main(*args, final_smooth=True, render=str(tmp_path / "seen"), eps=eps, **kw)
    assert not (tmp_path / "out").exists()
    assert list(on[0]) == list(off[0])
    for k in on[0]:
        assert np.array_equal(np.asarray(on[0][k]), np.asarray(off[0][k])), k
    for i in (1, 2, 3, 4):
        assert np.array_equal(np.asarray(on[i]), np.asarray(off[i])), i
    _check_tree(env, str(tmp_path / "seen" / "studio-x" / "chunk_7"), np.asarray(on[1]), np.asarray(on[3]), np.asarray(on[4]))
