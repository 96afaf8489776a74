"""Skeleton meshes on the device: gem_skeleton_mesh against the numpy twin (tests/mesh_twin.py), its bounds
and its defined corners, gem_sequence_align against `errors.umeyama`, and `save=True` end to end -- the batch pipeline with and
without ground truth, `optimizer.main`, and that nothing else changes with it."""
import os
import pickle

import numpy as np
import pytest

import mesh_twin as T
from pipeline_checks import SIZE, check_folder as _check_folder, same_bits as _same_bits, write_recording as _write_recording
from globalegomocap_amd.camera import DEFAULT_CALIBRATION

pytestmark = pytest.mark.gpu

ATOL = 1e-12          # metres: the project's float64 tolerance; the two rotation forms differ by at most 5.4e-14 beyond 0.1 rad from the axis
BLOCK = 349920
CRT = (1.3, None, np.array([0.1, -0.2, 0.3]))          # R: a rotation by 0.7 rad about (1, 2, -1), filled in below


def _rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


CRT = (CRT[0], _rotation((1.0, 2.0, -1.0), 0.7), CRT[2])


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import prepare
    return prepare._lift_engine(DEFAULT_CALIBRATION, 0)


def synth_poses(n, seed=9):
    """`synth` poses in a world frame: the camera frame has the wearer's legs along its z axis, which is the one direction the
    kernel test wants every bone away from."""
    from globalegomocap_amd import synth
    s = synth.make_sequence(n_frames=n, seed=seed, with_heatmaps=False)
    return np.asarray(s["estimated_local_skeleton"], dtype=np.float64) @ _rotation((1.0, 0.3, 0.2), 1.0) + np.array([0.3, 1.2, -0.4])


def assert_generic_bones(poses):
    """Every bone of MESH_LINES at least 0.1 rad from +-z and longer than 1 cm."""
    from globalegomocap_amd.skeleton import MESH_LINES
    for a, b in MESH_LINES:
        d = poses[:, b] - poses[:, a]
        h = np.linalg.norm(d, axis=-1)
        angle = np.arctan2(np.hypot(d[:, 0], d[:, 1]), np.abs(d[:, 2]))
        assert (h > 0.01).all() and (angle >= 0.1).all(), ((a, b), h.min(), angle.min())


@pytest.fixture(scope="module")
def twin5():
    """Five frames of synthetic poses and the twin's meshes of them, plain and behind CRT: computed once, never changed."""
    poses = synth_poses(5)
    assert_generic_bones(poses)
    assert_generic_bones(np.stack([CRT[0] * (p @ CRT[1]) + CRT[2] for p in poses]))
    plain = [T.frame_mesh(p) for p in poses]
    moved = [T.frame_mesh(p, CRT) for p in poses]
    for x in [poses] + [m[0] for m in plain + moved]:
        x.setflags(write=False)
    return poses, plain, moved


def _crt_tensor(dev):
    import torch
    return torch.from_numpy(np.concatenate([[CRT[0]], CRT[1].reshape(-1), CRT[2]])).to(dev)


def _check_blocks(blocks, want, what):
    worst = 0.0
    for f, (wv, wc, _) in enumerate(want):
        v, c = T.parse_vertex_block(blocks[f, :BLOCK])
        worst = max(worst, float(np.abs(v - wv).max()))
        np.testing.assert_allclose(v, wv, rtol=0, atol=ATOL, err_msg="%s frame %d" % (what, f))
        assert np.array_equal(c, wc), (what, f)
    print("%s: largest vertex difference to the twin %.3g m" % (what, worst))


@pytest.mark.parametrize("with_crt", [False, True], ids=["plain", "behind a similarity"])
def test_kernel_against_the_twin(env, twin5, with_crt, capsys):
    import torch
    poses, plain, moved = twin5
    seq = torch.from_numpy(poses[:3].copy()).to(env.device)
    crt = _crt_tensor(env.device) if with_crt else None
    got = env.skeleton_mesh(seq, crt)
    again = env.skeleton_mesh(seq, crt)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, BLOCK) and got.is_cuda
    with capsys.disabled():
        _check_blocks(got.cpu().numpy(), (moved if with_crt else plain)[:3], "kernel, 3 frames%s" % (", crt" if with_crt else ""))
    assert torch.equal(got, again)
    from globalegomocap_amd import meshes
    assert torch.equal(meshes.vertex_blocks(env, poses[:3]), env.skeleton_mesh(seq))


@pytest.mark.parametrize("F,gap", [(1, 0), (5, 0), (5, 64), (1, 4096)])
def test_shapes_and_bounds(env, twin5, F, gap, capsys):
    """F = 1 and 5, strides larger than the block: 64 bytes of canary before the buffer, after it and in every gap stay untouched."""
    import torch
    poses, plain, _ = twin5
    stride = BLOCK + gap
    buf = torch.full((64 + F * stride + 64,), 0xA5, dtype=torch.uint8, device=env.device)
    view = buf[64:64 + F * stride].view(F, stride)
    assert view.data_ptr() % 16 == 0
    out = env.skeleton_mesh(torch.from_numpy(poses[:F].copy()).to(env.device), None, out=view)
    assert out.data_ptr() == view.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:64] == 0xA5).all() and (host[-64:] == 0xA5).all()
    rows = host[64:-64].reshape(F, stride)
    assert (rows[:, BLOCK:] == 0xA5).all()
    with capsys.disabled():
        _check_blocks(rows, plain[:F], "F = %d, stride = block + %d" % (F, gap))


def test_misaligned_buffers_are_refused_without_a_launch(env):
    import ctypes as C
    import torch
    from globalegomocap_amd import _capi
    lib = env.lib
    seq = torch.from_numpy(synth_poses(2)).to(env.device)
    buf = torch.full((2 * BLOCK + 256,), 0x5A, dtype=torch.uint8, device=env.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for base, stride, word in ((8, BLOCK, b"aligned"), (0, BLOCK + 8, b"multiple of 16"), (0, BLOCK - 16, b"at least"), (4, BLOCK + 4, b"")):
        rc = lib.gem_skeleton_mesh(C.c_void_p(seq.data_ptr()), 2, None, C.c_void_p(buf.data_ptr() + base), stride, st)
        assert rc != 0 and word in lib.gem_last_error(), (base, stride)
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())
    with pytest.raises(ValueError):
        env.skeleton_mesh(seq, None, out=buf[:2 * (BLOCK - 16)].view(2, BLOCK - 16))
    with pytest.raises(_capi.GemError, match="multiple of 16"):
        env.skeleton_mesh(seq, None, out=buf[:2 * (BLOCK + 8)].view(2, BLOCK + 8))
    with pytest.raises(TypeError):
        env.skeleton_mesh(seq.float())
    with pytest.raises(ValueError):
        env.skeleton_mesh(seq[:, :14].contiguous())
    with pytest.raises(TypeError):
        env.sequence_align(seq, seq.cpu())
    with pytest.raises(ValueError):
        env.sequence_align(seq, seq[:1])


@pytest.mark.parametrize("n_frames", [3, 98], ids=["45 points", "1470 points"])
def test_sequence_align_against_umeyama(env, n_frames, capsys):
    import torch
    from globalegomocap_amd.errors import umeyama
    src = synth_poses(n_frames, seed=5)
    rng = np.random.default_rng(n_frames)
    dst = 0.8 * (src @ _rotation((0.3, -1.0, 0.5), 1.1)) + np.array([0.4, 0.1, -0.7]) + rng.normal(0.0, 0.01, src.shape)
    s_d, d_d = torch.from_numpy(src).to(env.device), torch.from_numpy(dst).to(env.device)
    got = env.sequence_align(s_d, d_d)
    again = env.sequence_align(s_d, d_d)
    assert got.dtype == torch.float64 and tuple(got.shape) == (13,) and torch.equal(got, again)
    got = got.cpu().numpy()
    c, R, t = umeyama(src.reshape(-1, 3), dst.reshape(-1, 3))
    want = np.concatenate([[c], R.reshape(-1), t])
    with capsys.disabled():
        print("sequence_align, %d points: largest relative difference to errors.umeyama %.3g" % (n_frames * 15, np.abs(got / want - 1).max()))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def test_defined_corners(env, capsys):
    """One frame with a bone exactly along +z, one exactly along -z, one with 1 + c = 2^-41, one of length zero and a NaN joint."""
    import torch
    from globalegomocap_amd.skeleton import MESH_LINES
    pose = synth_poses(1, seed=2)[0]
    pose[2] = pose[1] + np.array([0.0, 0.0, 0.25])                          # line (1, 2): +z
    pose[5] = pose[4] - np.array([0.0, 0.0, 0.25])                          # line (4, 5): -z
    pose[7] = (0.5, 0.25, 0.75)
    bz = -(1.0 - 2.0 ** -41)
    pose[8] = pose[7] + 0.25 * np.array([np.sqrt(1.0 - bz * bz), 0.0, bz])  # line (7, 8): 1 + c = 2^-41
    pose[10] = pose[9]                                                      # line (9, 10): no length
    pose[14] = np.nan                                                       # joint 14: its sphere and line (13, 14)
    d = pose[8] - pose[7]
    c1 = 1 + d[2] / np.sqrt(d @ d)
    assert 0.99 * 2.0 ** -41 < c1 < 1.01 * 2.0 ** -41, c1
    d = pose[2] - pose[1]
    assert d[0] == 0 and d[1] == 0 and d[2] > 0
    d = pose[5] - pose[4]
    assert d[0] == 0 and d[1] == 0 and d[2] < 0
    buf = torch.full((64 + BLOCK + 64,), 0xA5, dtype=torch.uint8, device=env.device)
    env.skeleton_mesh(torch.from_numpy(pose[None].copy()).to(env.device), None, out=buf[64:64 + BLOCK].view(1, BLOCK))
    host = buf.cpu().numpy()
    assert (host[:64] == 0xA5).all() and (host[-64:] == 0xA5).all()
    v, col = T.parse_vertex_block(host[64:-64])
    wv, wc, _ = T.frame_mesh(pose)
    parts = T.part_slices()
    nan_parts = [14, 15 + list(MESH_LINES).index((13, 14))]
    for k, (v0, nv, _, _) in enumerate(parts):
        if k in nan_parts:
            assert np.isnan(v[v0:v0 + nv]).all(), k
        else:
            assert np.isfinite(v[v0:v0 + nv]).all(), k
    with capsys.disabled():
        print("corners: largest vertex difference to the twin %.3g m" % np.nanmax(np.abs(v - wv)))
    np.testing.assert_allclose(v, wv, rtol=0, atol=ATOL, equal_nan=True)
    assert np.array_equal(col, wc)
    # the -z bone: the cylinder template turned by diag(1, -1, -1)
    for line, R in (((4, 5), np.diag([1.0, -1.0, -1.0])), ((7, 8), np.diag([1.0, -1.0, -1.0])), ((1, 2), np.eye(3)), ((9, 10), np.eye(3))):
        v0, nv, _, _ = parts[15 + list(MESH_LINES).index(line)]
        a, b = pose[line[0]], pose[line[1]]
        tpl, _ = T.cylinder(0.005, np.linalg.norm(b - a))
        np.testing.assert_allclose(v[v0:v0 + nv], tpl @ R.T + (a + b) / 2, rtol=0, atol=ATOL, err_msg=str(line))
    v0, nv, _, _ = parts[15 + list(MESH_LINES).index((9, 10))]
    assert np.ptp(v[v0 + 2:v0 + nv, 2]) == 0          # all five rings coincide


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def chunk_dirs(env, golden, tmp_path_factory):
    """One chunk of 26 frames with ground truth and the same without, as pickles under <tmp>/with_gt/studio and <tmp>/no_gt/studio."""
    from globalegomocap_amd import prepare as P
    from helpers import sd_from_npz
    tmp = tmp_path_factory.mktemp("meshes")
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


@pytest.mark.parametrize("device_metrics", [True, False], ids=["batched report", "per-chunk report"])
def test_save_with_ground_truth(chunk_dirs, device_metrics):
    import torch
    from globalegomocap_amd import whole_sequence as ws
    from globalegomocap_amd.errors import align_sequence
    tmp, kw = chunk_dirs["tmp"], dict(chunk_dirs["kw"], device_metrics=device_metrics)
    root = str(tmp / "with_gt" / "studio")
    out = tmp / ("m_gt_%d" % device_metrics)
    torch.manual_seed(31)
    off = ws.optimize_directory(root, DEFAULT_CALIBRATION, **kw)
    torch.manual_seed(31)
    on = ws.optimize_directory(root, DEFAULT_CALIBRATION, save=True, mesh_root=str(out), **kw)
    _same_bits(on, off)
    base = out / "studio" / chunk_dirs["name"]
    assert sorted(os.listdir(str(base))) == ["gt_global_aligned", "input_global_aligned", "optimized_global_aligned"]
    assert on[2].shape == on[3].shape == on[4].shape == (SIZE, 15, 3)
    _check_folder(str(base / "optimized_global_aligned"), align_sequence(on[3], on[4]))
    _check_folder(str(base / "input_global_aligned"), align_sequence(on[2], on[4]))
    _check_folder(str(base / "gt_global_aligned"), on[4])


def test_save_without_ground_truth(chunk_dirs):
    import torch
    from globalegomocap_amd import whole_sequence as ws
    tmp, kw = chunk_dirs["tmp"], chunk_dirs["kw"]
    root = str(tmp / "no_gt" / "studio")
    torch.manual_seed(31)
    off = ws.optimize_directory(root, DEFAULT_CALIBRATION, ground_truth=False, **kw)
    torch.manual_seed(31)
    on = ws.optimize_directory(root, DEFAULT_CALIBRATION, ground_truth=False, save=True, mesh_root=str(tmp / "m_no_gt"), **kw)
    _same_bits(on, off)
    base = tmp / "m_no_gt" / "studio" / chunk_dirs["name"]
    assert sorted(os.listdir(str(base))) == ["input_global", "optimized_global"]
    _check_folder(str(base / "optimized_global"), on[3])
    _check_folder(str(base / "input_global"), on[2])


def test_main_writes_the_reference_tree(env, chunk_dirs, tmp_path, monkeypatch):
    """optimizer.main(save=True): out/<dataset>/<chunk>/... under the working directory, as at optimizer.py:486-504."""
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
    off = gopt.main(*args, final_smooth=True, eps=eps, **kw)
    assert not (tmp_path / "out").exists()
    on = gopt.main(*args, final_smooth=True, save=True, eps=eps, **kw)
    assert list(on[0]) == list(off[0])
    for k in on[0]:
        assert np.array_equal(np.asarray(on[0][k]), np.asarray(off[0][k])), k
    for i in (1, 2, 3, 4):
        assert np.array_equal(np.asarray(on[i]), np.asarray(off[i])), i
    base = tmp_path / "out" / "studio-x" / "chunk_7"
    assert sorted(os.listdir(str(base))) == ["gt_global_aligned", "input_global_aligned", "optimized_global_aligned"]
    est, opt, gt = np.asarray(on[1]), np.asarray(on[3]), np.asarray(on[4])
    _check_folder(str(base / "optimized_global_aligned"), align_sequence(opt, gt))
    _check_folder(str(base / "input_global_aligned"), align_sequence(est, gt))
    _check_folder(str(base / "gt_global_aligned"), gt)
    # and under another root when asked; the module's own reader reads what was written
    gopt.main(*args, final_smooth=True, save=True, mesh_root=str(tmp_path / "elsewhere"), device_metrics=True, eps=eps, **kw)
    from globalegomocap_amd import meshes
    v, c, t = meshes.read_ply(str(tmp_path / "elsewhere" / "studio-x" / "chunk_7" / "gt_global_aligned" / "out_0000.ply"))
    tv, tc, tt = T.read_ply(str(base / "gt_global_aligned" / "out_0000.ply"))
    assert np.array_equal(v, tv) and np.array_equal(c, tc) and np.array_equal(t, tt)


def test_write_meshes_through_small_buffers(env, twin5, tmp_path, monkeypatch):
    """Five frames through pinned buffers of two frames each: three batches, both buffers used again; the CLI on a pose pickle."""
    from globalegomocap_amd import meshes
    poses, plain, moved = twin5
    monkeypatch.setattr(meshes, "PINNED_BYTES", 2 * BLOCK)
    meshes.release()
    try:
        assert meshes.write_meshes(env, poses, str(tmp_path / "five"), pattern="m_%02d.ply") == 5
        assert sorted(os.listdir(str(tmp_path / "five"))) == ["m_%02d.ply" % f for f in range(5)]
        for f in range(5):
            v, c, t = T.read_ply(str(tmp_path / "five" / ("m_%02d.ply" % f)))
            np.testing.assert_allclose(v, plain[f][0], rtol=0, atol=ATOL)
            assert np.array_equal(c, plain[f][1]) and np.array_equal(t, plain[f][2])
    finally:
        meshes.release()
    pkl = str(tmp_path / "result_pose.pkl")
    with open(pkl, "wb") as f:
        pickle.dump({"estimated_pose": list(poses[:2]), "optimized_pose": poses[:2] + 0.01, "gt_pose": list(poses[:2] * 1.1)}, f)
    meshes.main([pkl, "--out", str(tmp_path / "cli"), "--align", "true"])
    assert sorted(os.listdir(str(tmp_path / "cli"))) == ["gt_global_aligned", "input_global_aligned", "optimized_global_aligned"]
    from globalegomocap_amd.errors import align_sequence
    _check_folder(str(tmp_path / "cli" / "input_global_aligned"), align_sequence(poses[:2], poses[:2] * 1.1))
    meshes.main([pkl, "--out", str(tmp_path / "cli_plain")])
    assert sorted(os.listdir(str(tmp_path / "cli_plain"))) == ["gt_global", "input_global", "optimized_global"]
    _check_folder(str(tmp_path / "cli_plain" / "optimized_global"), poses[:2] + 0.01)
    meshes.release()
