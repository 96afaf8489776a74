"""Motion-JPEG clips on the device: gem_jpeg_encode against the numpy twin (tests/jpeg_twin.py) -- the
quantised coefficients first, then the bytes -- on the cases of tests/video_cases.py, AVI chunks, the capacity rule, a wide stride,
determinism and the refusals; `render.write_frames(video=)` / `write_camera_frames(video=)` read back frame by frame; and
`video=DIR` / `video_camera=DIR` through the batch pipeline on two chunks, the result bit for bit that of the call without them."""
import ctypes as C
import os
import pickle
import struct

import numpy as np
import pytest

import jpeg_twin as T
import video_cases as K
from pipeline_checks import IMG, CAMERA_N, SIZE, same_bits, write_recording
from globalegomocap_amd.camera import DEFAULT_CALIBRATION

pytestmark = pytest.mark.gpu

GUARD = 0xA5
COLOURS = ((214, 39, 40), (31, 119, 180))
_twin = {}


def twin(name, quality):
    """(coefficients, file) of a case at a quality: computed once, never changed."""
    if (name, quality) not in _twin:
        img = K.cases()[name][0]
        coef = T.coefficients(img, quality)
        coef.setflags(write=False)
        _twin[(name, quality)] = (coef, T.encode(img, quality, coef))
    return _twin[(name, quality)]


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import prepare
    return prepare._lift_engine(DEFAULT_CALIBRATION, 0)


def scanlines_of(images, stride=None, filter_byte=0):
    """uint8 [n, stride]: every image as H rows of a filter byte and 3 W bytes; what lies behind an image's bytes is GUARD."""
    H, W = images[0].shape[:2]
    need = H * (1 + 3 * W)
    rows = np.full((len(images), need if stride is None else stride), GUARD, dtype=np.uint8)
    for i, img in enumerate(images):
        rows[i, :need] = np.concatenate([np.full((H, 1), filter_byte, dtype=np.uint8), img.reshape(H, 3 * W)], axis=1).reshape(-1)
    return rows


def on_device(env, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


CASES = [(name, q) for name, (_, named) in K.cases().items() for q in sorted({90, named})]


@pytest.mark.parametrize("name,quality", CASES, ids=["%s, quality %d" % c for c in CASES])
def test_encoder_against_the_twin(env, name, quality):
    img, named = K.cases()[name]
    K.assert_exercises(name, T.symbol_stats(twin(name, named)[1]))          # on the twin: the case does what it is for
    want_coef, want = twin(name, quality)
    H, W = img.shape[:2]
    data, at, coef = env.jpeg_encode(on_device(env, scanlines_of([img], filter_byte=3)), W, H, quality, coef=True)
    got_coef = coef.cpu().numpy()
    assert got_coef.shape == (1,) + want_coef.shape
    assert np.array_equal(got_coef[0], want_coef), "coefficients differ at %s" % (np.argwhere(got_coef[0] != want_coef)[:4].tolist(),)
    got = bytes(data.cpu().numpy())
    assert at == [0, len(want)] and len(got) == len(want)
    assert got[:T.HEADER_BYTES] == want[:T.HEADER_BYTES], "header"
    assert got == want, "entropy data differs from byte %d" % next(i for i in range(len(want)) if got[i] != want[i])


@pytest.fixture(scope="module")
def three_images():
    """Three different 20 x 12 images whose files show an odd and an even length (seeds chosen on the twin)."""
    images = [K.noise(20, 12, seed) for seed in (11, 14, 13)]
    files = [T.encode(img, 90) for img in images]
    assert {len(f) % 2 for f in files} == {0, 1}, [len(f) for f in files]
    return images, files


def test_avi_chunks_of_a_batch(env, three_images):
    import torch
    images, files = three_images
    want = b"".join(T.avi_chunk(f) for f in files)
    out = torch.full((len(want) + 64,), GUARD, dtype=torch.uint8, device=env.device)
    data, at = env.jpeg_encode(on_device(env, scanlines_of(images)), 20, 12, avi=True, out=out)
    assert data.data_ptr() == out.data_ptr() and at[0] == 0 and at[3] == len(want)
    got = out.cpu().numpy()
    assert (got[len(want):] == GUARD).all()          # nothing behind offsets[n] is written
    for i, f in enumerate(files):
        chunk = bytes(got[at[i]:at[i + 1]])
        assert at[i + 1] - at[i] == 8 + len(f) + len(f) % 2
        assert chunk[:4] == b"00dc" and struct.unpack("<I", chunk[4:8])[0] == len(f) and chunk[8:8 + len(f)] == f
        assert len(f) % 2 == 0 or chunk[-1] == 0
    assert bytes(got[:len(want)]) == want
    # the same images as plain files
    data, at = env.jpeg_encode(on_device(env, scanlines_of(images)), 20, 12)
    assert bytes(data.cpu().numpy()) == b"".join(files) and at == list(np.cumsum([0] + [len(f) for f in files]))


def test_a_capacity_one_byte_short(env, three_images):
    """`offsets` is complete, the last image is not written at all, the others are; the wrapper then calls once more."""
    import torch
    images, files = three_images
    total = sum(len(f) for f in files)
    scan = on_device(env, scanlines_of(images))
    room = torch.full((total + 32,), GUARD, dtype=torch.uint8, device=env.device)
    offsets = torch.full((4,), -1, dtype=torch.int64, device=env.device)
    env.jpeg_encode_into(scan, 20, 12, 90, False, room[:total - 1], offsets)
    at = offsets.tolist()
    assert at == list(np.cumsum([0] + [len(f) for f in files]))
    got = room.cpu().numpy()
    assert bytes(got[:at[2]]) == files[0] + files[1] and (got[at[2]:] == GUARD).all()
    data, at2 = env.jpeg_encode(scan, 20, 12, out=room[:total - 1])
    assert at2 == at and data.numel() == total and bytes(data.cpu().numpy()) == b"".join(files)
    assert (room.cpu().numpy()[total - 1:] == GUARD).all()
    # room for nothing (an empty tensor has no address, and a null d_out is refused): only the offsets
    offsets.fill_(-1)
    env.jpeg_encode_into(scan, 20, 12, 90, False, room[:1], offsets)
    assert offsets.tolist() == at and (room.cpu().numpy()[at[2]:] == GUARD).all()


def test_a_stride_wider_than_the_image(env, three_images):
    images, files = three_images
    need = 12 * (1 + 3 * 20)
    wide = on_device(env, scanlines_of(images, stride=need + 37, filter_byte=9))
    data, at = env.jpeg_encode(wide, 20, 12)
    assert bytes(data.cpu().numpy()) == b"".join(files)
    data, at = env.jpeg_encode(wide[1:], 20, 12)          # (a batch that does not start at the buffer's first byte)
    assert bytes(data.cpu().numpy()) == files[1] + files[2]


def test_two_calls_give_the_same_bytes(env):
    import torch
    img = K.noise(200, 40, 21)
    scan = on_device(env, scanlines_of([img, img[::-1].copy()]))
    a, at_a, ca = env.jpeg_encode(scan, 200, 40, 75, avi=True, coef=True)
    b, at_b, cb = env.jpeg_encode(scan, 200, 40, 75, avi=True, coef=True)
    assert a.data_ptr() != b.data_ptr() and at_a == at_b and torch.equal(a, b) and torch.equal(ca, cb)
    want = T.encode(img, 75)
    assert bytes(a.cpu().numpy()[8:8 + len(want)]) == want


def test_refusals_without_a_launch(env):
    import torch
    from globalegomocap_amd._capi import GemError
    scan = on_device(env, scanlines_of([K.noise(8, 8, 0)]))
    out = torch.full((4096,), GUARD, dtype=torch.uint8, device=env.device)
    offsets = torch.full((2,), -7, dtype=torch.int64, device=env.device)
    P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)          # noqa: E731

    def call(n=1, W=8, H=8, stride=200, quality=90, scan_=scan, out_=out, offsets_=offsets):
        return env.lib.gem_jpeg_encode(env._h, P(scan_), n, W, H, stride, quality, 0, P(out_), out.numel(), P(offsets_), None, None)
    for kw, word in ((dict(W=0), "width must be 1 .. 1024"), (dict(W=1025, stride=1 << 20), "width must be 1 .. 1024"),
                     (dict(H=0), "height must be 1 .. 16384"), (dict(H=16385, stride=1 << 30), "height must be 1 .. 16384"),
                     (dict(quality=0), "quality must be 1 .. 100"), (dict(quality=101), "quality must be 1 .. 100"),
                     (dict(n=-1), "images per call"), (dict(stride=199), "in_stride must be at least"),
                     (dict(scan_=None), "null argument"), (dict(out_=None), "null argument"), (dict(offsets_=None), "null argument")):
        assert call(**kw) == 1 and word in env.lib.gem_last_error().decode(), kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all() and offsets.tolist() == [-7, -7]
    assert call(n=0, scan_=None, out_=None) == 0          # no image: nothing to do, offsets[0] = 0
    assert offsets.tolist()[0] == 0
    with pytest.raises(ValueError, match="scanline bytes"):
        env.jpeg_encode(scan, 9, 8)
    with pytest.raises(GemError, match="quality"):
        env.jpeg_encode(scan, 8, 8, quality=0)


# ------------------------------------------------------------------------------------------------------------------ clips
def world_poses(n, seed):
    from globalegomocap_amd import synth
    s = synth.make_sequence(n_frames=n, seed=seed, cam_jitter=(2.0, 0.01))
    cams = np.asarray(s["camera_pose_list"], dtype=np.float64)
    local = np.asarray(s["estimated_local_skeleton"], dtype=np.float64)
    return s, cams, np.einsum("nij,nkj->nki", cams[:, :3, :3], local) + cams[:, None, :3, 3]


def check_clip(path, rows, W, H, fps, quality=90):
    """The clip holds one frame per row of `rows` (scanline streams), each the twin's file of that image."""
    from globalegomocap_amd import video as V
    got_fps, got_W, got_H, frames = V.read_avi(path)
    assert (got_fps, got_W, got_H, len(frames)) == (fps, W, H, len(rows))
    for k, frame in enumerate(frames):
        img = T.image_of(rows[k], W, H)
        assert frame == T.encode(img, quality), k
    return frames


def test_write_frames_as_a_clip(env, tmp_path, monkeypatch):
    """Three frames, two sequences overlaid, 64 x 48: `frames.avi` holds the twin's files of `render.scanlines`; with frames=False no
    PNG appears; with both, the PNG files are what they are without the clip.  Then batches of two frames: both pinned buffers."""
    from globalegomocap_amd import render as R, video as V
    seqs = [world_poses(3, 9)[2], world_poses(3, 12)[2]]
    clip = str(tmp_path / "clips" / "frames.avi")
    assert R.write_frames(env, seqs, str(tmp_path / "none"), colours=COLOURS, size=(64, 48), video=clip, frames=False) == 1
    assert not (tmp_path / "none").exists()
    view = R.frames_view(env, seqs, size=(64, 48))
    rows = R.scanlines(env, seqs, view, COLOURS).cpu().numpy()
    frames = check_clip(clip, rows, 64, 48, 25.0)
    back = T.decode(frames[1])
    assert (T.image_of(rows[1], 64, 48) != 255).any() and np.abs(back.astype(int) - T.image_of(rows[1], 64, 48)).mean() < 4.0
    both = str(tmp_path / "both")
    assert R.write_frames(env, seqs, both, colours=COLOURS, size=(64, 48), names=("a", "b"), video=clip, video_fps=50, video_quality=60) == 6
    assert sorted(os.listdir(both)) == ["frame_%04d.png" % f for f in range(3)] + ["overview_a.png", "overview_b.png"]
    assert np.array_equal(R.read_png(os.path.join(both, "frame_0002.png")), T.image_of(rows[2], 64, 48))
    check_clip(clip, rows, 64, 48, 50.0, 60)
    monkeypatch.setattr(V, "SCAN_BYTES", 2 * R.layout(64, 48).stride)
    V.release()
    try:
        five = [world_poses(5, 9)[2]]
        assert R.write_frames(env, five, None, colours=COLOURS[:1], size=(64, 48), video=clip, frames=False) == 1
        check_clip(clip, R.scanlines(env, five, R.frames_view(env, five, size=(64, 48)), COLOURS[:1]).cpu().numpy(), 64, 48, 25.0)
    finally:
        V.release()


def test_write_camera_frames_as_a_clip(env, tmp_path):
    from globalegomocap_amd import render as R
    s, cams, est = world_poses(3, 5)
    heat = np.asarray(s["heatmap_list"], dtype=np.float32)
    seqs = [est, est + 0.02]
    clip = str(tmp_path / "camera.avi")
    kw = dict(colours=COLOURS, size=64, joint_radius=30.0, line_radius=12.0)
    assert R.write_camera_frames(env, seqs, cams, heat, str(tmp_path / "none"), video=clip, video_fps=12.5, frames=False, **kw) == 1
    assert not (tmp_path / "none").exists()
    rows = R.camera_scanlines(env, seqs, cams, heat, COLOURS, size=64, joint_radius=30.0, line_radius=12.0).cpu().numpy()
    check_clip(clip, rows, 64, 64, 12.5)
    assert (T.image_of(rows[0], 64, 64) != 255).any()
    assert R.write_camera_frames(env, seqs, cams, heat, str(tmp_path / "png"), video=clip, **kw) == 4
    assert sorted(os.listdir(str(tmp_path / "png"))) == ["camera_%04d.png" % f for f in range(3)]
    check_clip(clip, rows, 64, 64, 25.0)


def test_the_command_line_writes_a_clip(env, tmp_path):
    from globalegomocap_amd import render as R
    est = world_poses(2, 9)[2]
    pkl = str(tmp_path / "result_pose.pkl")
    with open(pkl, "wb") as f:
        pickle.dump({"estimated_pose": list(est), "optimized_pose": est + 0.01}, f)
    R.main([pkl, "--out", str(tmp_path / "cli"), "--size", "32x24", "--video", "--video_fps", "10", "--video_quality", "80", "--no_frames"])
    assert os.listdir(str(tmp_path / "cli")) == ["frames.avi"]
    trio = [est, est + 0.01]
    rows = R.scanlines(env, trio, R.frames_view(env, trio, size=(32, 24)), list(R.PALETTE.values())[:2]).cpu().numpy()
    check_clip(str(tmp_path / "cli" / "frames.avi"), rows, 32, 24, 10.0, 80)


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture
def small_images(monkeypatch):
    """The pipeline's images are small where it asks for the default sizes."""
    from globalegomocap_amd import render as R
    monkeypatch.setattr(R, "DEFAULT_SIZE", IMG)
    monkeypatch.setattr(R, "CAMERA_SIZE", CAMERA_N)


@pytest.fixture(scope="module")
def two_chunk_dirs(env, golden, tmp_path_factory):
    """Two chunks of 26 frames of one recording as pickles under <tmp>/equal/studio (the fixture of test_camera_view_gpu.py)."""
    from globalegomocap_amd import prepare as P
    from helpers import sd_from_npz
    tmp = tmp_path_factory.mktemp("clips")
    n = 2 * SIZE + 1
    hd, dd, traj, gtp = write_recording(tmp / "rec", n, seed=23)
    rec = P.prepare_sequence(traj, hd, dd, gtp, 0, n, fps=25, test_size=SIZE, verbose=False)
    assert len(rec) == 2
    rec.write_chunks(str(tmp / "equal" / "studio"))
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False)
    return dict(tmp=tmp, kw=kw, names=[c.name for c in rec.chunks])


def test_clips_from_the_pipeline(env, two_chunk_dirs, small_images):
    """`video=` and `video_camera=` on a directory of two chunks: both files per chunk, no PNG, the result bit for bit that of the call
    without them; every chunk's clips hold the twin's files of what `render` and `render_camera` draw for that chunk."""
    import torch
    from globalegomocap_amd import render as R, whole_sequence as ws
    tmp, kw, names = two_chunk_dirs["tmp"], two_chunk_dirs["kw"], two_chunk_dirs["names"]
    root = str(tmp / "equal" / "studio")
    out = tmp / "seen"
    torch.manual_seed(31)
    off = ws.optimize_directory(root, DEFAULT_CALIBRATION, **kw)
    assert not out.exists()
    torch.manual_seed(31)
    on = ws.optimize_directory(root, DEFAULT_CALIBRATION, video=str(out), video_camera=str(out), video_fps=30, **kw)
    same_bits(on, off)
    assert os.listdir(str(out)) == ["studio"] and sorted(os.listdir(str(out / "studio"))) == sorted(names)
    lo = 0
    for name in names:
        est, opt, gt = (on[i][lo:lo + SIZE] for i in (2, 3, 4))
        lo += SIZE
        base = out / "studio" / name
        assert sorted(os.listdir(str(base))) == ["camera.avi", "frames.avi"]
        trio, to = [est, opt, gt], [gt, gt, None]
        colours = list(R.PALETTE.values())
        view = R.frames_view(env, trio, align_to=to, size=IMG)
        rows = R.scanlines(env, trio, view, colours, align_to=to).cpu().numpy()
        check_clip(str(base / "frames.avi"), rows, IMG[0], IMG[1], 30.0)
        c = ws.load_chunk(os.path.join(root, name))
        rows = R.camera_scanlines(env, trio, c["cams"][:SIZE], c["heat"][:SIZE], colours, align_to=[None, None, opt]).cpu().numpy()
        check_clip(str(base / "camera.avi"), rows, CAMERA_N, CAMERA_N, 30.0)
        assert (T.image_of(rows[3], CAMERA_N, CAMERA_N) != 255).any()
