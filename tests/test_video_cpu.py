"""Motion-JPEG clips, the part that needs no GPU: the library's header and bound against the numpy twin
(tests/jpeg_twin.py), the twin against itself and -- where PIL is installed -- against PIL's tables, decoder and encoder, the AVI
container written and read back, and the argument errors."""
import ctypes as C
import io
import os
import struct

import numpy as np
import pytest

import jpeg_twin as T


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import _capi
    return _capi.load_library()


@pytest.fixture(scope="module")
def V(lib):
    from globalegomocap_amd import video
    return video


def noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def flat_scene():
    """88 x 64, a few flat colours on white: what the renderers draw."""
    img = np.full((64, 88, 3), 255, dtype=np.uint8)
    img[10:30, 5:40] = (214, 39, 40)
    img[20:60, 30:80] = (31, 119, 180)
    img[40:50, :] = (44, 160, 44)
    return img


def library_header(lib, W, H, quality):
    buf = (C.c_ubyte * 700)()
    assert lib.gem_jpeg_header(W, H, quality, buf, 700) == T.HEADER_BYTES
    return bytes(buf[:T.HEADER_BYTES])


@pytest.mark.parametrize("W,H,quality", [(640, 480, 90), (20, 12, 50), (8, 8, 100)])
def test_header_is_the_twins(lib, W, H, quality):
    assert library_header(lib, W, H, quality) == T.header(W, H, quality)


def test_header_and_bound_refuse_bad_arguments(lib):
    buf = (C.c_ubyte * 700)()
    for args, word in (((0, 8, 90), "width"), ((1025, 8, 90), "width"), ((8, 0, 90), "height"), ((8, 16385, 90), "height"),
                       ((8, 8, 0), "quality"), ((8, 8, 101), "quality")):
        assert lib.gem_jpeg_header(*args, buf, 700) == -1 and word in lib.gem_last_error().decode(), args
    assert lib.gem_jpeg_header(8, 8, 90, buf, 628) == -1 and "629" in lib.gem_last_error().decode()
    assert lib.gem_jpeg_bound(0, 8) == -1 and lib.gem_jpeg_bound(8, 16385) == -1


def test_bound_covers_noise_at_quality_100(lib):
    """The derivation of 6j: 629 + ceil(H/8) (2 ceil(3 ceil(W/8) 1660 / 8) + 2)."""
    assert lib.gem_jpeg_bound(8, 8) == 629 + 2 * ((3 * 1660 + 7) // 8) + 2
    assert lib.gem_jpeg_bound(640, 480) == 629 + 60 * (2 * ((240 * 1660 + 7) // 8) + 2)
    for seed in range(4):
        assert lib.gem_jpeg_bound(8, 8) >= len(T.encode(noise(8, 8, seed), 100))


def test_the_twin_decodes_its_own_files():
    """Quality 100 divides by 1: a flat grey image's only coefficient is its DC, and it comes back exactly (a flat colour within
    the rounding of the colour transforms, 2 levels).  Noise comes back within the quantisation's bound: a coefficient moves by at
    most half its step q / 2 and every basis function is at most c(u) c(v) / 4 <= 1/4 in magnitude, so a sample moves by at most
    64 * (1/4) * max(q) / 2 = 8 max(q), and by 1/2 more for the rounding of the forward colour transform; a colour is at most
    1 + 1.772 times that (blue: Y + 1.772 Cb), plus 1/2 for its own rounding and 1/2 for the 16-bit colour matrix."""
    for colour in ((77, 77, 77), (255, 255, 255), (0, 0, 0), (214, 39, 40)):
        img = np.empty((16, 16, 3), dtype=np.uint8)
        img[:] = colour
        back = T.decode(T.encode(img, 100)).astype(int)
        assert np.abs(back - img).max() <= (0 if colour[0] == colour[1] == colour[2] else 2), colour
    for quality in (100, 90, 50):
        img = noise(20, 12, 3)
        data = T.encode(img, quality)
        back = T.decode(data)
        assert back.shape == img.shape
        step = max(max(q) for q in T.quant_tables(quality))
        assert np.abs(back.astype(int) - img).max() <= 2.772 * (8 * step + 0.5) + 1, quality
        assert np.array_equal(T._walk(data)[1], T.coefficients(img, quality))          # the entropy code is lossless


def test_zigzag_and_tables():
    assert T.ZIGZAG[:10] == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and sorted(T.ZIGZAG) == list(range(64))
    assert T.quant_tables(50)[0] == T.Q_LUMA and T.quant_tables(100) == [[1] * 64] * 2
    assert T.quant_tables(1)[0][0] == 255 and T.quant_tables(25)[0][0] == 32
    C8 = T.dct_matrix()
    exact = 2.0 ** 14 * np.where(np.arange(8)[:, None] == 0, np.sqrt(0.5), 1.0) / 2.0 * np.cos((2 * np.arange(8)[None, :] + 1) * np.arange(8)[:, None] * np.pi / 16)
    assert np.abs(np.abs(exact - np.floor(exact)) - 0.5).min() > 0.01          # no entry near a rounding tie
    assert C8[0, 0] == 5793 and np.abs(C8).max() == 8035
    for bits, vals in zip(T.DC_BITS + T.AC_BITS, T.DC_VALS + T.AC_VALS):
        assert sum(bits) == len(vals) == len(set(vals))


def test_symbol_stats_of_the_gpu_cases():
    """The inputs of tests/test_video_gpu.py do what they are for (the same assertions stand there, next to the device's bytes)."""
    import video_cases as K
    for name, (img, quality) in K.cases().items():
        K.assert_exercises(name, T.symbol_stats(T.encode(img, quality)))


# ------------------------------------------------------------------------------------------------------------------ against PIL
def _segments(data):
    """{marker: [bodies]} of a JPEG file's header."""
    out, at = {}, 2
    while data[at + 1] != 0xDA:
        n = struct.unpack(">H", data[at + 2:at + 4])[0]
        out.setdefault(data[at + 1], []).append(data[at + 4:at + 2 + n])
        at += 2 + n
    return out


def test_tables_are_pils(lib):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(noise(16, 16, 0)).save(buf, "JPEG", quality=50, subsampling=0)
    pil = _segments(buf.getvalue())
    split = lambda bodies, size: sorted(b[i:i + size] for b in bodies for i in range(0, len(b), size))          # noqa: E731  (PIL may pack tables into one segment)
    for mine in (_segments(T.header(16, 16, 50)), _segments(library_header(lib, 16, 16, 50))):
        assert split(mine[0xDB], 65) == split(pil[0xDB], 65)
        tables = lambda bodies: sorted(_dht_tables(b"".join(bodies)))          # noqa: E731
        assert tables(mine[0xC4]) == tables(pil[0xC4])


def _dht_tables(body):
    at = 0
    while at < len(body):
        n = sum(body[at + 1:at + 17])
        yield body[at:at + 17 + n]
        at += 17 + n


ROUND_TRIP = (("8 x 80 noise", lambda: noise(8, 80, 0), 90), ("88 x 64 flat-colour scene", flat_scene, 90), ("20 x 12 noise", lambda: noise(20, 12, 0), 100))


@pytest.mark.parametrize("name,make,quality", ROUND_TRIP, ids=[r[0] for r in ROUND_TRIP])
def test_round_trip_error_against_pils_encoder(name, make, quality, capsys):
    """PIL decodes the twin's file, and the mean absolute round-trip error is at most 1.02 times that of PIL's own encoder at the same
    quality with subsampling=0 (the margin covers nothing but a different rounding of the DCT).  Measured: 8 x 80 noise 1.0010,
    flat-colour scene 0.9963, 20 x 12 noise 0.9853."""
    Image = pytest.importorskip("PIL.Image")
    img = make()
    mine = np.asarray(Image.open(io.BytesIO(T.encode(img, quality))).convert("RGB"))
    assert mine.shape == img.shape
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=0)
    theirs = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    e_mine, e_theirs = np.abs(mine.astype(int) - img).mean(), np.abs(theirs.astype(int) - img).mean()
    with capsys.disabled():
        print("%s at quality %d: mean abs error %.4f, PIL's encoder %.4f, ratio %.4f" % (name, quality, e_mine, e_theirs, e_mine / e_theirs))
    assert e_mine <= 1.02 * e_theirs


# ------------------------------------------------------------------------------------------------------------------ the container
@pytest.fixture(scope="module")
def twin_frames():
    frames = [T.encode(noise(20, 12, seed), 90) for seed in range(6)]
    lengths = [len(f) % 2 for f in frames]
    assert 0 in lengths and 1 in lengths, lengths          # odd and even lengths: with and without a pad byte
    return frames


def test_avi_round_trip(V, twin_frames, tmp_path):
    path = str(tmp_path / "sub" / "clip.avi")
    assert V.write_avi(path, twin_frames, 20, 12, fps=29.97) == len(twin_frames)
    fps, W, H, back = V.read_avi(path)
    assert (fps, W, H) == (29.97, 20, 12) and back == twin_frames
    with open(path, "rb") as f:
        data = f.read()
    n, largest = len(twin_frames), max(len(f) for f in twin_frames)
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == len(data) - 8 and data[8:12] == b"AVI "
    assert data[12:16] == b"LIST" and data[20:28] == b"hdrlavih" and struct.unpack("<I", data[28:32])[0] == 56
    assert struct.unpack("<14I", data[32:88]) == (33367, 0, 0, 0x10, n, 0, 1, largest, 20, 12, 0, 0, 0, 0)
    assert data[88:92] == b"LIST" and data[96:104] == b"strlstrh" and struct.unpack("<I", data[104:108])[0] == 56
    assert struct.unpack("<4s4sIHHIIIIIIII4h", data[108:164]) == (b"vids", b"MJPG", 0, 0, 0, 0, 1000, 29970, 0, n, largest, 0xFFFFFFFF, 0, 0, 0, 20, 12)
    assert data[164:168] == b"strf" and struct.unpack("<I", data[168:172])[0] == 40
    assert struct.unpack("<IiiHH4sIiiII", data[172:212]) == (40, 20, 12, 1, 24, b"MJPG", 3 * 20 * 12, 0, 0, 0, 0)
    assert data[212:216] == b"LIST" and data[220:224] == b"movi"
    at, entries = 224, []
    for frame in twin_frames:
        assert data[at:at + 4] == b"00dc" and struct.unpack("<I", data[at + 4:at + 8])[0] == len(frame)
        assert data[at + 8:at + 8 + len(frame)] == frame
        entries.append((at - 220, len(frame)))
        at += 8 + len(frame)
        if len(frame) % 2:
            assert data[at] == 0
            at += 1
    assert entries[0][0] == 4 and at == 220 + struct.unpack("<I", data[216:220])[0]
    assert data[at:at + 4] == b"idx1" and struct.unpack("<I", data[at + 4:at + 8])[0] == 16 * n and len(data) == at + 8 + 16 * n
    for i, (where, size) in enumerate(entries):
        e = at + 8 + 16 * i
        assert data[e:e + 4] == b"00dc" and struct.unpack("<III", data[e + 4:e + 16]) == (0x10, where, size)
    # an empty clip is a valid file too
    empty = str(tmp_path / "empty.avi")
    V.write_avi(empty, [], 20, 12)
    assert V.read_avi(empty) == (25.0, 20, 12, []) and os.path.getsize(empty) == 224 + 8


def test_read_avi_refuses(V, twin_frames, tmp_path):
    good = str(tmp_path / "good.avi")
    V.write_avi(good, twin_frames, 20, 12)
    with open(good, "rb") as f:
        data = f.read()
    idx = data.rindex(b"idx1")
    bad = {"truncated inside the index": data[:-5], "truncated inside movi": data[:400], "no index": data[:idx],
           "an index offset that disagrees": data[:idx + 8 + 8] + struct.pack("<I", 6) + data[idx + 8 + 12:],
           "an index size that disagrees": data[:idx + 8 + 16 + 12] + struct.pack("<I", 1) + data[idx + 8 + 16 + 16:],
           "a wrong frame count": data[:48] + struct.pack("<I", len(twin_frames) + 1) + data[52:],
           "a wrong RIFF size": data[:4] + struct.pack("<I", len(data)) + data[8:],
           "bytes behind the index": data + b"\0\0",
           "a chunk that is no 00dc": data[:224] + b"01wb" + data[228:]}
    for name, blob in bad.items():
        p = str(tmp_path / "bad.avi")
        with open(p, "wb") as f:
            f.write(blob)
        with pytest.raises(ValueError):
            V.read_avi(p)
            pytest.fail("read_avi accepted: " + name)
    assert V.read_avi(good)[3] == twin_frames


def test_a_file_stops_below_2_gib(V, twin_frames, tmp_path, monkeypatch):
    """The next run would pass the limit: the file is closed, valid, with the frames before it, and the call names their count."""
    path = str(tmp_path / "full.avi")
    sizes = [8 + len(f) + len(f) % 2 for f in twin_frames]
    monkeypatch.setattr(V, "MAX_FILE", 224 + sum(sizes[:4]) + 8 + 16 * 4 + 10)
    w = V.AviWriter(path, 20, 12)
    w.append_frames(twin_frames[:2])
    w.append_frames(twin_frames[2:4])
    with pytest.raises(OverflowError, match="holds the 4 frames"):
        w.append_frames(twin_frames[4:])
    assert V.read_avi(path)[3] == twin_frames[:4]


# ------------------------------------------------------------------------------------------------------------------ arguments
def test_argument_errors(V, tmp_path, capsys):
    from globalegomocap_amd import render as R, whole_sequence as ws
    seqs = [np.zeros((2, 15, 3))]
    out, clip = str(tmp_path / "o"), str(tmp_path / "c.avi")
    with pytest.raises(ValueError, match="video_quality"):
        R.write_frames(None, seqs, out, video=clip, video_quality=0)
    with pytest.raises(ValueError, match="video_quality"):
        R.write_frames(None, seqs, out, video=clip, video_quality=101)
    with pytest.raises(ValueError, match="video_fps"):
        R.write_frames(None, seqs, out, video=clip, video_fps=0)
    with pytest.raises(ValueError, match="video_fps"):
        R.write_camera_frames(None, seqs, None, None, out, video=clip, video_fps=-1.0)
    with pytest.raises(ValueError, match="frames=False"):
        R.write_frames(None, seqs, out, frames=False)
    with pytest.raises(ValueError, match="frames=False"):
        R.write_camera_frames(None, seqs, None, None, out, frames=False)
    with pytest.raises(ValueError, match="video_quality"):
        ws._settings("cam.json", video="d", video_quality=0)
    with pytest.raises(ValueError, match="video_fps"):
        ws._settings("cam.json", video_camera="d", video_fps=0.0)
    with pytest.raises(ValueError, match="video_fps"):
        V.AviWriter(clip, 20, 12, fps=0)
    for argv, word in ((["--data_path", "d", "--video", "v", "--video_quality", "0"], "--video_quality"),
                       (["--data_path", "d", "--video", "v", "--video_fps", "0"], "--video_fps")):
        with pytest.raises(SystemExit) as e:
            ws._cli(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
    for argv, word in ((["p.pkl", "--out", out, "--video", "--video_quality", "0"], "--video_quality"),
                       (["p.pkl", "--out", out, "--video", "--video_fps", "-2"], "--video_fps"),
                       (["p.pkl", "--out", out, "--no_frames"], "--no_frames")):
        with pytest.raises(SystemExit) as e:
            R.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
    assert not os.path.exists(out) and not os.path.exists(clip)


def test_the_arguments_are_wired_and_none_writes_nothing(V, tmp_path, monkeypatch):
    from globalegomocap_amd import render as R, report, whole_sequence as ws
    cfg = ws._settings("cam.json", video="a", video_camera="b", video_fps=30.0, video_quality=75, bvh="c")
    assert (cfg.video, cfg.video_camera, cfg.video_fps, cfg.video_quality, cfg.bvh) == ("a", "b", 30.0, 75, "c")
    cfg = ws._settings("cam.json", 0.5)
    assert (cfg.video, cfg.video_camera, cfg.video_fps, cfg.video_quality, cfg.vae_weight) == (None, None, None, None, 0.5)
    with pytest.raises(TypeError):          # the clip options go by keyword only: there is no 28th positional argument
        ws._settings("cam.json", *([None] * 27))
    a = ws._parser().parse_args(["--data_path", "d", "--video", "V", "--video_camera", "C", "--video_fps", "50", "--video_quality", "80"])
    assert (a.video, a.video_camera, a.video_fps, a.video_quality) == ("V", "C", 50.0, 80)
    a = ws._parser().parse_args(["--data_path", "d"])
    assert (a.video, a.video_camera, a.video_fps, a.video_quality) == (None, None, None, None)
    monkeypatch.chdir(tmp_path)
    seqs = (np.zeros((3, 15, 3)), np.zeros((3, 15, 3)), None)
    report.Outputs().write(None, "studio/chunk_0", seqs)
    report.Outputs(video_fps=30, video_quality=50).write(None, "studio/chunk_0", seqs)
    assert os.listdir(str(tmp_path)) == []
    calls = []
    monkeypatch.setattr(R, "write_result_frames", lambda *a, **k: calls.append(("frames", a, k)))
    monkeypatch.setattr(R, "write_result_camera_frames", lambda *a, **k: calls.append(("camera", a, k)))
    cams, heat = np.zeros((5, 4, 4)), np.zeros((5, 2, 2, 15))
    report.Outputs(video="root").write("engine", "data/studio/chunk_0", seqs)
    report.Outputs(video="root", video_camera="cam", video_fps=50, video_quality=70).write("engine", "data/studio/chunk_0", seqs, cams=cams,
                                                                                          heat=heat, first_frame=1)
    assert [c[0] for c in calls] == ["frames", "frames", "camera"]
    assert calls[0][2] == dict(video=os.path.join("root", "studio", "chunk_0", "frames.avi"), video_fps=25, video_quality=90, frames=False)
    assert calls[2][2] == dict(video=os.path.join("cam", "studio", "chunk_0", "camera.avi"), video_fps=50, video_quality=70, frames=False)
    assert calls[2][1][4].shape == (3, 4, 4) and calls[2][1][5].shape == (3, 2, 2, 15) and calls[0][1][:2] == ("engine", None)
