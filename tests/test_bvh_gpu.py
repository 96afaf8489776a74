"""BVH animation files on the device: gem_bvh_rest and gem_bvh_channels against the numpy twin
(tests/bvh_twin.py), the defined corners on axis-aligned skeletons, gem_format_fields against Python's "%15.6f", `write_bvh` read
back, and `bvh=DIR` end to end -- the batch pipeline with and without ground truth, `optimizer.main`, and that nothing else changes."""
import os
import pickle

import numpy as np
import pytest

import bvh_twin as T
from pipeline_checks import SIZE, same_bits as _same_bits, write_recording as _write_recording
from globalegomocap_amd.camera import DEFAULT_CALIBRATION

pytestmark = pytest.mark.gpu

SHAPES = (1, 5, 37, 300)          # 300 frames: five workgroups of gem_bvh_channels, the last one partly filled
CRT = np.concatenate([[1.3], T.euler_matrix(20.0, -35.0, 50.0).reshape(-1), [0.1, -0.2, 0.3]])
ANGLE_TOL = 1e-7                  # degrees: asin amplifies 1e-15 of matrix error by at most 1 / sqrt(2e-10) -> 4e-9 degrees, 25x margin
POS_TOL = 2e-6                    # metres at unit_scale 1: 5e-7 from the root's position, < 1e-7 from at most 7 chained rounded angles


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import prepare
    return prepare._lift_engine(DEFAULT_CALIBRATION, 0)


@pytest.fixture(scope="module")
def B(env):
    from globalegomocap_amd import bvh
    return bvh


@pytest.fixture(scope="module")
def twin300():
    """300 random frames and the twin's channels of them, plain and behind CRT: computed once, never changed."""
    X = T.random_frames(300, seed=2)
    plain, moved = T.channels(X), T.channels(X, CRT)
    for a in (X, plain, moved):
        a.setflags(write=False)
    return X, plain, moved


def _dev(env, a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a))          # (a copy: the fixtures are read-only)
    return (t if dtype is None else t.to(dtype)).to(env.device)


@pytest.mark.parametrize("with_crt", [False, True], ids=["plain", "behind a similarity"])
@pytest.mark.parametrize("n", SHAPES)
def test_rest_lengths_against_the_twin(env, B, twin300, n, with_crt, capsys):
    import torch
    X = twin300[0][:n]
    seq, crt = _dev(env, X), _dev(env, CRT) if with_crt else None
    got, again = B.rest_lengths(env, seq, crt), B.rest_lengths(env, seq, crt)
    assert got.dtype == torch.float64 and tuple(got.shape) == (19,) and torch.equal(got, again)
    got, want = got.cpu().numpy(), T.rest_lengths(X, CRT if with_crt else None)
    has = np.array(T.HAS_REST)
    assert (got[~has] == 0).all() and (want[has] > 0.05).all()
    with capsys.disabled():
        print("rest lengths, %d frames%s: largest relative difference to the twin %.3g" % (n, ", crt" if with_crt else "", np.abs(got[has] / want[has] - 1).max()))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("with_crt", [False, True], ids=["plain", "behind a similarity"])
@pytest.mark.parametrize("n", SHAPES)
def test_channels_against_the_twin(env, B, twin300, n, with_crt, capsys):
    """Local rotations rebuilt from the angles to 1e-12, root positions to rtol 1e-12, the angles themselves to 1e-7 degrees; 64 numbers
    of canary before and after the array stay untouched."""
    import ctypes as C
    import torch
    X, want = twin300[0][:n], twin300[2 if with_crt else 1][:n]
    seq, crt = _dev(env, X), _dev(env, CRT) if with_crt else None
    rest = B.rest_lengths(env, seq, crt)
    buf = torch.full((64 + n * 60 + 64,), -7.0, dtype=torch.float64, device=env.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = env.lib.gem_bvh_channels(C.c_void_p(seq.data_ptr()), n, C.c_void_p(crt.data_ptr() if with_crt else 0), C.c_void_p(rest.data_ptr()),
                                  C.c_double(100.0), C.c_void_p(buf.data_ptr() + 64 * 8), st)
    assert rc == 0, env.lib.gem_last_error()
    host = buf.cpu().numpy()
    assert (host[:64] == -7.0).all() and (host[-64:] == -7.0).all()
    got = host[64:-64].reshape(n, 60)
    assert np.array_equal(got, B.channels(env, seq, crt, rest, 100.0).cpu().numpy())
    angle = np.abs(got[:, 3:] - want[:, 3:]).max()
    matrix = np.abs(T.local_matrices(got) - T.local_matrices(want)).max()
    with capsys.disabled():
        print("channels, %d frames%s: angles %.3g degrees, rebuilt local rotations %.3g, root position %.3g (relative) from the twin"
              % (n, ", crt" if with_crt else "", angle, matrix, np.abs(got[:, :3] / (100.0 * want[:, :3]) - 1).max()))
    assert matrix <= 1e-12
    np.testing.assert_allclose(got[:, :3], 100.0 * want[:, :3], rtol=1e-12, atol=0)
    assert angle <= ANGLE_TOL
    assert (np.abs(want[:, 4::3]) != 90.0).all()          # (no frame in the gimbal branch: the bound above holds)


def test_defined_corners(env, B, capsys):
    """Axis-aligned skeletons: a bone along its rest direction, antiparallel to it (about each of the three axes), of length zero,
    coinciding hips and shoulders, the neck on the hip line, and the gimbal branch with both signs."""
    frames = T.corner_frames()
    X = np.stack(list(frames.values()))
    seq = _dev(env, X)
    rest = B.rest_lengths(env, seq)
    got, want = B.channels(env, seq, None, rest, 1.0).cpu().numpy(), T.channels(X)
    L_got, L_want = T.local_matrices(got), T.local_matrices(want)
    with capsys.disabled():
        for f, name in enumerate(frames):
            print("corner %-42s angles %.3g degrees, local rotations %.3g from the twin" % (name, np.abs(got[f, 3:] - want[f, 3:]).max(), np.abs(L_got[f] - L_want[f]).max()))
    assert np.isfinite(got).all()
    assert np.abs(L_got - L_want).max() <= 1e-12
    np.testing.assert_allclose(got[:, :3], want[:, :3], rtol=1e-12, atol=0)
    assert np.abs(got[:, 3:] - want[:, 3:]).max() <= ANGLE_TOL
    names = list(frames)
    eye = np.eye(3)

    def turned(f):
        return [n for n in range(T.N) if np.abs(L_got[f, n] - eye).max() > 1e-9]
    assert turned(0) == []                                                          # the rest pose: 19 identities
    assert turned(names.index("right elbow bone antiparallel (r = -X)")) == [4, 5]   # a half turn, and the one that undoes it
    assert turned(names.index("left knee bone antiparallel (r = -Y)")) == [15, 16]
    assert turned(names.index("right foot bone antiparallel (r = +Z)")) == [13]
    f = names.index("right elbow bone antiparallel (r = -X)")
    np.testing.assert_allclose(L_got[f, 4], np.diag([-1.0, -1.0, 1.0]), rtol=0, atol=1e-12)          # r near X: about unit(r cross Y) = -Z
    np.testing.assert_allclose(L_got[names.index("left knee bone antiparallel (r = -Y)"), 15], np.diag([-1.0, -1.0, 1.0]), rtol=0, atol=1e-12)          # about unit(r cross X) = Z
    np.testing.assert_allclose(L_got[names.index("right foot bone antiparallel (r = +Z)"), 13], np.diag([-1.0, 1.0, -1.0]), rtol=0, atol=1e-12)
    assert turned(names.index("zero-length right wrist bone")) == []
    f = names.index("coinciding hips")
    assert np.array_equal(L_got[f, 0], eye) and np.array_equal(L_got[f, 11], eye)
    assert np.array_equal(L_got[names.index("coinciding shoulders"), 2], eye)
    assert np.array_equal(L_got[names.index("the neck on the hip line"), 0], eye)
    for name, b in (("gimbal, b = -90", -90.0), ("gimbal, b = +90", 90.0)):
        f = names.index(name)
        assert got[f, 3 + 3 * 11 + 1] == b and got[f, 3 + 3 * 11 + 2] == 0.0 and abs(got[f, 3 + 3 * 11]) <= ANGLE_TOL, name
        assert turned(f) == [11]
    # what the corners are for: the skeleton still comes back (where every bone has a direction)
    for f, name in enumerate(names):
        if "zero-length" in name or "coinciding" in name:
            continue
        r = T.rest_lengths(X[f:f + 1])
        np.testing.assert_allclose(T.fk(got[f:f + 1], T.offsets_of(r)), T.regrow(X[f:f + 1], r), rtol=0, atol=1e-12, err_msg=name)


TABLE = (0.0, -0.0, -1e-9, 0.0078125, 0.0234375, 1.0 - 2.0 ** -53, 123456.5, -9999999.999999, 5e-324, 2.0 ** -30)


def _text(env, B, values, per_line, canary=64):
    import torch
    values = np.asarray(values, dtype=np.float64)
    n = values.size
    buf = torch.full((canary + 16 * n + canary,), 0xA5, dtype=torch.uint8, device=env.device)
    bad = B.new_counter(env.device)
    out = B.format_fields(env, _dev(env, values), per_line, bad, out=buf[canary:canary + 16 * n])
    assert out.data_ptr() == buf.data_ptr() + canary
    host = buf.cpu().numpy()
    assert (host[:canary] == 0xA5).all() and (host[-canary:] == 0xA5).all()
    return host[canary:canary + 16 * n].tobytes(), bad.cpu().numpy().tolist()


def test_format_fields_is_pythons_percent(env, B, capsys):
    """The table of the hard cases, and 1000 random values across the binary exponents -40 .. 23."""
    rng = np.random.default_rng(11)
    random = rng.choice([-1.0, 1.0], 1000) * rng.uniform(0.5, 1.0, 1000) * 2.0 ** rng.integers(-40, 24, 1000)
    assert np.abs(random).max() < 9999999.0
    values = np.concatenate([TABLE, random])
    got, bad = _text(env, B, values, 7)
    want = T.format_fields(values, 7)
    fields = [got[16 * i:16 * i + 16] for i in range(len(values))]
    assert fields[3] == b"       0.007812 " and fields[4] == b"       0.023438 " and fields[1] == b"      -0.000000 " and fields[2] == b"      -0.000000 "
    assert fields[5] == b"       1.000000 " and fields[6] == b"  123456.500000\n" and fields[7] == b"-9999999.999999 " and fields[8] == b"       0.000000 "
    wrong = [i for i in range(len(values)) if fields[i] != want[16 * i:16 * i + 16]]
    with capsys.disabled():
        print("format_fields: %d of %d fields differ from Python's %%15.6f" % (len(wrong), len(values)))
    assert got == want, [(values[i], fields[i]) for i in wrong[:5]]
    assert bad == [0, -1]
    assert _text(env, B, values, 7)[0] == got          # two calls, the same bytes
    assert _text(env, B, values[:5], 1)[0] == T.format_fields(values[:5], 1)
    assert _text(env, B, values[:1], 60)[0] == b"       0.000000 "


@pytest.mark.parametrize("value,field", [(10000000.0, b"*" * 15), (-10000000.0, b"*" * 15), (1e300, b"*" * 15), (float("nan"), b"            nan"),
                                         (float("inf"), b"            inf"), (float("-inf"), b"           -inf")], ids=str)
def test_format_fields_raises_the_counter(env, B, value, field):
    if field[:1] != b"*":
        assert ("%15.6f" % value).encode() == field
    values = np.linspace(-3.0, 3.0, 23)
    values[17] = value          # line 17 // 4 = 4
    got, bad = _text(env, B, values, 4)
    assert bad == [1, 4]
    assert got[16 * 17:16 * 17 + 15] == field
    values[17] = 0.0          # (Python's own field for the value may be wider than 15: the other fields, one by one)
    want = T.format_fields(values, 4)
    assert all(got[16 * i:16 * i + 16] == want[16 * i:16 * i + 16] for i in range(23) if i != 17) and got[16 * 17 + 15:16 * 18] == b" "


def test_format_fields_counts_every_bad_field_and_keeps_the_first_line(env, B):
    import torch
    values = np.zeros(40)
    values[[33, 12, 13, 27]] = (np.nan, 1e9, -np.inf, 1e7)
    got, bad = _text(env, B, values, 5)
    assert bad == [4, 2]
    assert _text(env, B, -np.abs(np.random.default_rng(0).normal(size=9)) * 9999999.999999 / 5, 3)[1] == [0, -1]
    # the counter is the caller's: a second call goes on counting, and an earlier line stays
    counter = B.new_counter(env.device)
    B.format_fields(env, _dev(env, values), 5, counter)
    B.format_fields(env, _dev(env, values[20:]), 5, counter)
    assert counter.cpu().numpy().tolist() == [6, 1]
    # misaligned text: refused before the launch
    buf = torch.full((16 * 40 + 32,), 0x5A, dtype=torch.uint8, device=env.device)
    with pytest.raises(Exception, match="16-byte aligned"):
        B.format_fields(env, _dev(env, values), 5, counter, out=buf[8:8 + 16 * 40])
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all()) and counter.cpu().numpy().tolist() == [6, 1]
    with pytest.raises(TypeError):
        B.format_fields(env, _dev(env, values.astype(np.float32)), 5, counter)
    with pytest.raises(ValueError):
        B.format_fields(env, _dev(env, values), 5, counter, out=buf[:16 * 39])


def test_motion_block_is_the_formatting_of_the_devices_channels(env, B, twin300):
    seq = _dev(env, twin300[0])
    rest = B.rest_lengths(env, seq)
    chan = B.channels(env, seq, None, rest, 100.0)
    bad = B.new_counter(env.device)
    text = B.format_fields(env, chan, 60, bad)
    again = B.format_fields(env, chan, 60, bad)
    got = text.cpu().numpy().tobytes()
    assert len(got) == 300 * 960 and got == T.format_fields(chan.cpu().numpy(), 60) and got == again.cpu().numpy().tobytes()
    assert bad.cpu().numpy().tolist() == [0, -1]
    assert got.count(b"\n") == 300 and all(got[960 * f + 959:960 * f + 960] == b"\n" for f in range(300))


# ------------------------------------------------------------------------------------------------------------------ files
def _check_file(B, path, X, unit_scale, fps, crt=None):
    """The file at `path` against the twin: header, frame count and time, size, and the positions read back against regrow(X)."""
    rest = T.rest_lengths(X, crt)
    got, want = B.read_bvh(path), T.parse(path)
    n = len(X)
    assert got.names == T.NAMES and tuple(got.parents.tolist()) == T.PARENTS and got.motion.shape == (n, 60)
    assert got.channels[0] == T.ROOT_CHANNELS and all(c == T.ROOT_CHANNELS[3:] for c in got.channels[1:])
    assert got.frame_time == float("%.6f" % (1.0 / fps))
    assert np.array_equal(got.motion, want["motion"]) and np.array_equal(got.offsets, want["offsets"])
    data = open(path, "rb").read()
    head = data[:len(data) - 960 * n]
    assert head.endswith(("MOTION\nFrames: %d\nFrame Time: %.6f\n" % (n, 1.0 / fps)).encode())
    np.testing.assert_allclose(got.offsets, T.offsets_of(rest, unit_scale), rtol=1e-12, atol=5.0000001e-7)
    pos = B.joint_positions(got)
    np.testing.assert_allclose(pos, T.parsed_positions(want), rtol=0, atol=1e-9 * unit_scale)
    worst = np.abs(pos - T.regrow(X, rest, crt, unit_scale)).max()
    assert worst <= POS_TOL * unit_scale, worst
    return got, worst


@pytest.mark.parametrize("unit_scale", [1.0, 100.0], ids=["metres", "default scale"])
def test_write_read_round_trip_through_small_buffers(env, B, twin300, tmp_path, monkeypatch, unit_scale, capsys):
    """300 frames through pinned buffers of 128 frames each: three slices, both buffers used again.  write_bvh -> read_bvh ->
    joint_positions is within 2e-6 m of regrow at unit_scale 1, within 2e-6 x 100 file units at the default scale."""
    X = twin300[0]
    monkeypatch.setattr(B, "PINNED_BYTES", 128 * 960)
    B.release()
    try:
        path = str(tmp_path / "deep" / "seq.bvh")
        kw = {} if unit_scale == 100.0 else {"unit_scale": unit_scale}
        assert B.write_bvh(env, X, path, fps=30, **kw) == 300
        got, worst = _check_file(B, path, X, unit_scale, 30)
        with capsys.disabled():
            print("write_bvh -> read_bvh -> joint_positions, unit_scale %g: %.3g file units from regrow(X)" % (unit_scale, worst))
        np.testing.assert_allclose(B.skeleton_from_nodes(got_pos := B.joint_positions(got)), T.joints_of(got_pos))
        # the motion block is the formatting of the device's own channels, slice boundaries included
        seq = _dev(env, X)
        chan = B.channels(env, seq, None, B.rest_lengths(env, seq), unit_scale).cpu().numpy()
        assert open(path, "rb").read()[-960 * 300:] == T.format_fields(chan, 60)
        # aligned to another sequence, one frame, and the same bytes on a second call
        to = 0.9 * (X @ T.euler_matrix(10.0, 20.0, 30.0)) + np.array([0.3, 0.2, 0.1])
        p2, p3 = str(tmp_path / "aligned.bvh"), str(tmp_path / "again.bvh")
        B.write_bvh(env, X, p2, align_to=to, unit_scale=unit_scale)
        B.write_bvh(env, X, p3, align_to=to, unit_scale=unit_scale)
        assert open(p2, "rb").read() == open(p3, "rb").read()
        from globalegomocap_amd.errors import align_sequence
        _check_file(B, p2, align_sequence(X, to), unit_scale, 25)
        B.write_bvh(env, X[:1], str(tmp_path / "one.bvh"), unit_scale=unit_scale)
        _check_file(B, str(tmp_path / "one.bvh"), X[:1], unit_scale, 25)
    finally:
        B.release()


def test_a_bad_frame_raises_and_leaves_no_file(env, B, twin300, tmp_path, monkeypatch):
    monkeypatch.setattr(B, "PINNED_BYTES", 128 * 960)
    B.release()
    try:
        X = twin300[0].copy()
        X[130, 6] = np.nan          # in the second slice
        X[200, 2] = np.nan
        path = str(tmp_path / "nan.bvh")
        with pytest.raises(ValueError, match="frame 130 "):
            B.write_bvh(env, X, path)
        assert not os.path.exists(path)
        with pytest.raises(ValueError, match="frame 0 "):          # a position beyond the field
            B.write_bvh(env, twin300[0], path, unit_scale=1e9)
        assert not os.path.exists(path) and os.listdir(str(tmp_path)) == []
        with pytest.raises(ValueError, match="at least one frame"):
            B.write_bvh(env, twin300[0][:0], path)
        with pytest.raises(ValueError, match="shape"):
            B.write_bvh(env, twin300[0], path, align_to=twin300[0][:5])
        assert os.listdir(str(tmp_path)) == []
        assert B.write_bvh(env, twin300[0], path) == 300          # and the buffers are fit for the next call
        _check_file(B, path, twin300[0], 100.0, 25)
    finally:
        B.release()


def test_cli_on_a_pose_pickle(env, B, twin300, tmp_path):
    X = twin300[0][:5]
    gt = 1.1 * X + 0.01
    pkl = str(tmp_path / "result_pose.pkl")
    with open(pkl, "wb") as f:
        pickle.dump({"estimated_pose": list(X), "optimized_pose": X + 0.01, "gt_pose": list(gt)}, f)
    from globalegomocap_amd.errors import align_sequence
    B.main([pkl, "--out", str(tmp_path / "cli"), "--align", "true", "--fps", "50"])
    assert sorted(os.listdir(str(tmp_path / "cli"))) == ["estimated.bvh", "gt.bvh", "optimized.bvh"]
    _check_file(B, str(tmp_path / "cli" / "estimated.bvh"), align_sequence(X, gt), 100.0, 50)
    _check_file(B, str(tmp_path / "cli" / "gt.bvh"), gt, 100.0, 50)
    B.main([pkl, "--out", str(tmp_path / "plain"), "--unit_scale", "1"])
    _check_file(B, str(tmp_path / "plain" / "optimized.bvh"), X + 0.01, 1.0, 25)
    with open(pkl, "wb") as f:
        pickle.dump({"estimated_pose": list(X), "optimized_pose": X + 0.01}, f)
    B.main([pkl, "--out", str(tmp_path / "two")])
    assert sorted(os.listdir(str(tmp_path / "two"))) == ["estimated.bvh", "optimized.bvh"]
    B.release()


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def chunk_dirs(env, golden, tmp_path_factory):
    """Two chunks of 26 frames with ground truth and the same without, as pickles under <tmp>/with_gt/studio and <tmp>/no_gt/studio."""
    from globalegomocap_amd import prepare as P
    from helpers import sd_from_npz
    tmp = tmp_path_factory.mktemp("bvh")
    n = 2 * SIZE + 1
    hd, dd, traj, gtp = _write_recording(tmp / "rec", n, seed=23)
    with_gt = P.prepare_sequence(traj, hd, dd, gtp, 0, n, fps=25, test_size=SIZE, verbose=False)
    no_gt = P.prepare_sequence(traj, hd, dd, None, 0, n, fps=25, test_size=SIZE, verbose=False, scale=1.7)
    assert len(with_gt) == len(no_gt) == 2
    with_gt.write_chunks(str(tmp / "with_gt" / "studio"))
    no_gt.write_chunks(str(tmp / "no_gt" / "studio"))
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False)
    return dict(tmp=tmp, kw=kw, names=[c.name for c in with_gt.chunks])


@pytest.mark.parametrize("device_metrics", [True, False], ids=["batched report", "per-chunk report"])
def test_bvh_with_ground_truth(B, chunk_dirs, device_metrics):
    import torch
    from globalegomocap_amd import whole_sequence as ws
    from globalegomocap_amd.errors import align_sequence
    tmp, kw = chunk_dirs["tmp"], dict(chunk_dirs["kw"], device_metrics=device_metrics)
    root = str(tmp / "with_gt" / "studio")
    out = tmp / ("b_gt_%d" % device_metrics)
    torch.manual_seed(31)
    off = ws.optimize_directory(root, DEFAULT_CALIBRATION, **kw)
    torch.manual_seed(31)
    on = ws.optimize_directory(root, DEFAULT_CALIBRATION, bvh=str(out), bvh_fps=50, **kw)
    _same_bits(on, off)
    assert on[2].shape == on[3].shape == on[4].shape == (2 * SIZE, 15, 3)
    assert sorted(os.listdir(str(out / "studio"))) == sorted(chunk_dirs["names"])
    for k, name in enumerate(sorted(chunk_dirs["names"], key=ws.natural_key)):
        base, fr = out / "studio" / name, slice(k * SIZE, (k + 1) * SIZE)
        assert sorted(os.listdir(str(base))) == ["estimated.bvh", "gt.bvh", "optimized.bvh"]
        _check_file(B, str(base / "optimized.bvh"), align_sequence(on[3][fr], on[4][fr]), 100.0, 50)
        _check_file(B, str(base / "estimated.bvh"), align_sequence(on[2][fr], on[4][fr]), 100.0, 50)
        _check_file(B, str(base / "gt.bvh"), on[4][fr], 100.0, 50)


def test_bvh_without_ground_truth(B, chunk_dirs):
    import torch
    from globalegomocap_amd import whole_sequence as ws
    tmp, kw = chunk_dirs["tmp"], chunk_dirs["kw"]
    root = str(tmp / "no_gt" / "studio")
    torch.manual_seed(31)
    off = ws.optimize_directory(root, DEFAULT_CALIBRATION, ground_truth=False, **kw)
    torch.manual_seed(31)
    on = ws.optimize_directory(root, DEFAULT_CALIBRATION, ground_truth=False, bvh=str(tmp / "b_no_gt"), **kw)
    _same_bits(on, off)
    for k, name in enumerate(sorted(chunk_dirs["names"], key=ws.natural_key)):
        base, fr = tmp / "b_no_gt" / "studio" / name, slice(k * SIZE, (k + 1) * SIZE)
        assert sorted(os.listdir(str(base))) == ["estimated.bvh", "optimized.bvh"]
        _check_file(B, str(base / "optimized.bvh"), on[3][fr], 100.0, 25)
        _check_file(B, str(base / "estimated.bvh"), on[2][fr], 100.0, 25)


def test_main_writes_the_three_files(env, B, chunk_dirs, tmp_path, monkeypatch):
    """optimizer.main(bvh=DIR): DIR/<dataset>/<chunk>/{estimated,optimized,gt}.bvh; the poses, the errors and the meshes beside them
    are bit for bit what the same call gives without it."""
    import torch
    from globalegomocap_amd import optimizer as gopt, synth
    from globalegomocap_amd.errors import align_sequence
    data = synth.make_sequence(n_frames=SIZE, seed=9)
    d = tmp_path / "studio-x" / "chunk_7"
    d.mkdir(parents=True)
    with open(str(d / "test_data.pkl"), "wb") as f:
        pickle.dump(synth.reference_pickle_dict(data), f)
    monkeypatch.chdir(tmp_path)
    kw = {k: chunk_dirs["kw"][k] for k in ("global_vae_path", "local_vae_path")}
    args = (str(d), DEFAULT_CALIBRATION, 0.0, 0.0, 0.001, 0.01, 0.01, 0.01)
    eps = torch.randn(6, 32, generator=torch.Generator().manual_seed(5))
    off = gopt.main(*args, final_smooth=True, save=True, mesh_root=str(tmp_path / "m_off"), eps=eps, **kw)
    on = gopt.main(*args, final_smooth=True, save=True, mesh_root=str(tmp_path / "m_on"), bvh=str(tmp_path / "anim"), eps=eps, **kw)
    assert list(on[0]) == list(off[0])
    for k in on[0]:
        assert np.array_equal(np.asarray(on[0][k]), np.asarray(off[0][k])), k
    for i in (1, 2, 3, 4):
        assert np.array_equal(np.asarray(on[i]), np.asarray(off[i])), i
    for folder in ("optimized_global_aligned", "input_global_aligned", "gt_global_aligned"):
        a, b = tmp_path / "m_off" / "studio-x" / "chunk_7" / folder, tmp_path / "m_on" / "studio-x" / "chunk_7" / folder
        assert sorted(os.listdir(str(a))) == sorted(os.listdir(str(b))) and len(os.listdir(str(a))) == SIZE
        for name in ("out_0000.ply", "out_%04d.ply" % (SIZE - 1)):
            assert open(str(a / name), "rb").read() == open(str(b / name), "rb").read()
    base = tmp_path / "anim" / "studio-x" / "chunk_7"
    assert sorted(os.listdir(str(base))) == ["estimated.bvh", "gt.bvh", "optimized.bvh"]
    est, opt, gt = np.asarray(on[1]), np.asarray(on[3]), np.asarray(on[4])
    _check_file(B, str(base / "optimized.bvh"), align_sequence(opt, gt), 100.0, 25)
    _check_file(B, str(base / "estimated.bvh"), align_sequence(est, gt), 100.0, 25)
    _check_file(B, str(base / "gt.bvh"), gt, 100.0, 25)
    gopt.main(*args, final_smooth=True, bvh=str(tmp_path / "anim_dev"), bvh_fps=100, device_metrics=True, eps=eps, **kw)
    got = B.read_bvh(str(tmp_path / "anim_dev" / "studio-x" / "chunk_7" / "gt.bvh"))
    assert got.frame_time == 0.01 and got.motion.shape == (SIZE, 60)
    B.release()
