"""Looking at a trained VAE on the device: gem_latent_paths and gem_latent_report against the numpy twin
(tests/vae_inspect_twin.py), fed random arrays directly, and `vae_inspect.Inspector` end to end on a tiny VAE -- the table of a
reconstruction pass against the twin applied to the engine's own encoder / decoder outputs, and the files of the three writers."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_twin
import vae_inspect_twin as T
from helpers import TINY

pytestmark = pytest.mark.gpu

N_COORDS, N_JOINTS = 450, 15          # a window of 10 frames
DIMS = (32, 100, 2048)                # 100: neither a multiple of the wave size nor of a 4-wide vector access


@pytest.fixture(scope="module")
def lib():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import _capi
    return _capi.load_library()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_paths(lib, za, zb, steps, mode):
    import torch
    from globalegomocap_amd import _capi
    a, b = _dev(za), _dev(zb)
    out = torch.full((za.shape[0], steps, za.shape[1]), float("nan"), device="cuda", dtype=torch.float32)
    _capi.check(lib.gem_latent_paths(_p(a), _p(b), za.shape[0], za.shape[1], steps, mode, _p(out), _stream()), lib)
    return out.cpu().numpy()


def device_report(lib, mu, logvar, x=None, rec=None, cols=None, count=None):
    import torch
    from globalegomocap_amd import _capi
    B, D = mu.shape
    rows = torch.full((B, 5), -7.0, device="cuda", dtype=torch.float64)
    held = [None if a is None else _dev(a) for a in (mu, logvar, x, rec)]          # (alive until the rows have been read back)
    _capi.check(lib.gem_latent_report(_p(held[0]), _p(held[1]), _p(held[2]), _p(held[3]), B, D, N_COORDS, N_JOINTS, _p(rows), _p(cols),
                                      _p(count), _stream()), lib)
    return rows.cpu().numpy()


def _pairs(P, D, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(P, D)).astype(np.float32), rng.normal(size=(P, D)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ gem_latent_paths
@pytest.mark.parametrize("D", DIMS)
def test_linear_paths_are_numpys_float32_arithmetic_bitwise(lib, D):
    for P in (1, 3):
        for S in (2, 3, 6):          # 2: no interior step
            za, zb = _pairs(P, D, 100 * P + S)
            got = device_paths(lib, za, zb, S, 0)
            want = T.paths(za, zb, S, "linear")
            assert got.dtype == np.float32 and got.shape == (P, S, D)
            assert np.array_equal(got[:, 0].view(np.uint32), za.view(np.uint32)), (P, S)          # the ends: the inputs' bits
            assert np.array_equal(got[:, S - 1].view(np.uint32), zb.view(np.uint32)), (P, S)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (P, S, int((got != want).sum()))
    # (at S = 6 the formula itself would not give b: the copy is what is being tested)
    za, zb = _pairs(3, D, 1)
    assert not np.array_equal(za + np.float32(1.0) * (zb - za), zb)


@pytest.mark.parametrize("D", DIMS)
def test_spherical_paths_within_one_ulp_of_the_twin(lib, D):
    for P in (1, 3):
        for S in (2, 3, 6):
            za, zb = _pairs(P, D, 200 * P + S)          # independent Gaussian draws: the angle is near pi / 2, far from the switch
            assert not any(T.takes_fallback(a, b) for a, b in zip(za, zb))
            got = device_paths(lib, za, zb, S, 1)
            want = T.paths(za, zb, S, "spherical")
            assert np.array_equal(got[:, 0].view(np.uint32), za.view(np.uint32)) and np.array_equal(got[:, S - 1].view(np.uint32), zb.view(np.uint32))
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            print("spherical D=%d P=%d S=%d: %d of %d entries differ, largest %.3g ulp" % (D, P, S, int((got != want).sum()), got.size,
                                                                                          float((err / np.spacing(np.abs(want))).max())))
            assert (err <= np.spacing(np.abs(want))).all(), (P, S)
            if S > 2 and D == 2048:          # not the straight line: the middle keeps the ends' norm
                mid, lin = got[:, S // 2].astype(np.float64), T.paths(za, zb, S, "linear")[:, S // 2].astype(np.float64)
                assert (np.linalg.norm(mid, axis=1) > 1.2 * np.linalg.norm(lin, axis=1)).all()


@pytest.mark.parametrize("D", DIMS)
def test_spherical_paths_fall_back_to_the_straight_line_bitwise(lib, D):
    a, b = _pairs(1, D, 5)
    za = np.concatenate([a, a, np.zeros_like(a), b])          # b = a, b = -a, a = 0, and an ordinary pair beside them
    zb = np.concatenate([a, -a, b, a])
    assert [T.takes_fallback(x, y) for x, y in zip(za, zb)] == [True, True, True, False]
    for S in (3, 6):
        got, lin = device_paths(lib, za, zb, S, 1), device_paths(lib, za, zb, S, 0)
        assert np.array_equal(got[:3].view(np.uint32), lin[:3].view(np.uint32)), S
        assert np.array_equal(lin.view(np.uint32), T.paths(za, zb, S, "linear").view(np.uint32))
        assert not np.array_equal(got[3], lin[3])


def test_latent_paths_refuses_bad_arguments(lib):
    import torch
    z = torch.zeros(2, 32, device="cuda")
    out = torch.zeros(2, 6, 32, device="cuda")
    for P, D, S, mode, word in ((0, 32, 6, 0, "n_pairs"), (2, 0, 6, 0, "latent_dim"), (2, 32, 1, 0, "n_steps"), (2, 32, 6, 2, "mode"),
                                (2, 32, 6, -1, "mode")):
        assert lib.gem_latent_paths(_p(z), _p(z), P, D, S, mode, _p(out), _stream()) != 0
        assert word in lib.gem_last_error().decode()
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0          # nothing was launched


# ------------------------------------------------------------------------------------------------------------------ gem_latent_report
def _report_case(B, D, seed):
    """Encoder-like outputs with the rows that stress the arithmetic: logvar = -30 (sigma = 3e-7), logvar = +10 (sigma^2 = 22026)
    and |mu| = 1e3; with fewer than five rows they are entries of the one row instead."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(size=(B, D)).astype(np.float32)
    lv = (0.5 * rng.normal(size=(B, D)) - 1.0).astype(np.float32)
    if B >= 5:
        lv[1], lv[2] = -30.0, 10.0
        mu[3] = 1e3 * np.sign(mu[3])
    else:
        lv[:, 0::7], lv[:, 1::7] = -30.0, 10.0
        mu[:, 2::7] = 1e3 * np.sign(mu[:, 2::7])
    x = rng.normal(size=(B, N_COORDS)).astype(np.float32)
    rec = (x + 0.05 * rng.normal(size=(B, N_COORDS))).astype(np.float32)
    return mu, lv, x, rec


def _check_rows(got, want, D, what):
    np.testing.assert_allclose(got[:, :3], want[:, :3], rtol=1e-12, atol=1e-12 * D, err_msg=str(what))
    np.testing.assert_allclose(got[:, 3:], want[:, 3:], rtol=1e-14, atol=0, err_msg=str(what))


@pytest.mark.parametrize("D", DIMS)
def test_report_rows_against_the_twin(lib, D):
    for B in (1, 5, 67):
        mu, lv, x, rec = _report_case(B, D, 10 * B + D)
        got, want = device_report(lib, mu, lv, x, rec), T.report_rows(mu, lv, x, rec)
        rel = np.abs(got - want) / np.abs(want)
        print("report D=%d B=%d: largest relative difference per entry %s" % (D, B, rel.max(axis=0)))
        assert np.isfinite(want).all()
        _check_rows(got, want, D, (B, D))
        bare = device_report(lib, mu, lv)          # without x / rec: the last two NaN, the rest the same bits
        assert np.isnan(bare[:, 3:]).all() and np.array_equal(bare[:, :3].view(np.uint64), got[:, :3].view(np.uint64))
        half = device_report(lib, mu, lv, x, None)
        assert np.isnan(half[:, 3:]).all() and np.array_equal(half[:, :3].view(np.uint64), got[:, :3].view(np.uint64))


def _two_calls(lib, D):
    import torch
    cols = torch.zeros(3, D, device="cuda", dtype=torch.float64)
    count = torch.zeros(1, device="cuda", dtype=torch.int64)
    cases = [_report_case(5, D, 1), _report_case(67, D, 2)]
    rows = [device_report(lib, *c, cols=cols, count=count) for c in cases]
    return cases, rows, cols.cpu().numpy(), int(count.cpu())


@pytest.mark.parametrize("D", DIMS)
def test_report_accumulators_over_two_calls_and_the_same_bits_again(lib, D):
    cases, rows, cols, count = _two_calls(lib, D)
    mu, lv = np.concatenate([c[0] for c in cases]), np.concatenate([c[1] for c in cases])
    want = T.report_cols(mu, lv)
    print("accumulators D=%d: largest relative difference %s" % (D, (np.abs(cols - want) / np.abs(want)).max(axis=1)))
    assert count == 72
    np.testing.assert_allclose(cols, want, rtol=1e-12, atol=0)
    for c, r in zip(cases, rows):          # (the rows do not change with the accumulators)
        _check_rows(r, T.report_rows(*c), D, D)
    _, rows2, cols2, count2 = _two_calls(lib, D)          # the whole sequence again, on fresh buffers
    assert count2 == 72 and np.array_equal(cols.view(np.uint64), cols2.view(np.uint64))
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(rows, rows2))


def test_report_count_alone_and_bad_arguments(lib):
    import torch
    mu, lv, x, rec = _report_case(5, 32, 3)
    count = torch.full((1,), 7, device="cuda", dtype=torch.int64)
    device_report(lib, mu, lv, count=count)
    assert int(count.cpu()) == 12
    t, rows = _dev(mu), torch.zeros(5, 5, device="cuda", dtype=torch.float64)
    for B, D, nc, nj, word in ((0, 32, 450, 15, "n_windows"), (5, 0, 450, 15, "latent_dim"), (5, 32, 449, 15, "n_coords"), (5, 32, 450, 0, "n_coords")):
        assert lib.gem_latent_report(_p(t), _p(t), _p(t), _p(t), B, D, nc, nj, _p(rows), None, None, _stream()) != 0
        assert word in lib.gem_last_error().decode()
    assert lib.gem_latent_report(_p(t), _p(t), None, None, 5, 32, 0, 0, None, None, None, _stream()) != 0


# ------------------------------------------------------------------------------------------------------------------ Inspector
N_WINDOWS, BATCH = 150, 64          # two full batches and a partial one


@pytest.fixture(scope="module")
def tiny(lib):
    from globalegomocap_amd import synth, vae, vae_inspect
    ins = vae_inspect.Inspector(vae.synthetic_state_dict(TINY, seed=3, gain=2.0), max_windows=BATCH)
    windows = synth.make_training_windows(N_WINDOWS, TINY.seq_len, 11)
    yield ins, windows
    ins.close()


@pytest.fixture(scope="module")
def tiny_twin(tiny):
    """The twin applied to the engine's own encoder / decoder outputs, read back batch by batch: computed once, never changed."""
    import torch
    ins, windows = tiny
    rows, mus, lvs = [], [], []
    for lo in range(0, N_WINDOWS, BATCH):
        x = torch.from_numpy(windows[lo:lo + BATCH]).cuda()
        mu, lv, z = ins.engine.encode(0, x)
        rec = ins.engine.decode(0, z)
        mu, lv, rec = mu.cpu().numpy(), lv.cpu().numpy(), rec.cpu().numpy().reshape(len(mu), -1)
        rows.append(T.report_rows(mu, lv, windows[lo:lo + BATCH].reshape(len(mu), -1), rec))
        mus.append(mu)
        lvs.append(lv)
    return np.concatenate(rows), np.concatenate(mus), np.concatenate(lvs)


def test_inspector_reads_the_shape_off_the_state_dict(tiny):
    ins, _ = tiny
    assert ins.shape == TINY and (ins.T, ins.D) == (10, 32)


def test_reconstruction_table_against_the_twin(tiny, tiny_twin):
    ins, windows = tiny
    want, mu, lv = tiny_twin
    rep = ins.reconstruct(windows, batch_size=BATCH)
    assert rep.table.shape == (N_WINDOWS, 5) and rep.count == N_WINDOWS and rep.keys == ins.engine.REPORT_KEYS
    assert np.isfinite(rep.table).all() and (rep.table[:, 4] >= rep.table[:, 3]).all() and (rep.table[:, 3] > 0).all()
    _check_rows(rep.table, want, TINY.latent_dim, "tiny")
    assert rep.means["mpjpe"] == float(rep.table[:, 3].mean())
    np.testing.assert_allclose(rep.sums, T.report_cols(mu, lv), rtol=1e-12, atol=1e-12)
    var = T.var_mu(mu)
    np.testing.assert_allclose(rep.var_mu, var, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(rep.mean_mu, mu.astype(np.float64).mean(axis=0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(rep.mean_var, np.exp(lv.astype(np.float64)).mean(axis=0), rtol=1e-12)
    middle = float(np.sort(var)[TINY.latent_dim // 2 - 1: TINY.latent_dim // 2 + 1].mean())          # between two dimensions: half are above
    for threshold in (0.01, middle):
        assert rep.active_units(threshold) == int((var > threshold).sum()), threshold
    assert rep.active_units(middle) == TINY.latent_dim // 2
    assert rep.worst(3) == [int(i) for i in np.argsort(-want[:, 3], kind="stable")[:3]]
    # another batch size: the same windows in the same rows.  (The encoder and decoder may take another kernel for another batch
    # shape, whose float32 outputs differ in their last bits, 1e-6 relative: 1e-3 passes that and not a misplaced row.)
    again = ins.reconstruct(windows, batch_size=37)
    assert again.count == N_WINDOWS
    np.testing.assert_allclose(again.table, want, rtol=1e-3, atol=0)
    np.testing.assert_allclose(again.sums, rep.sums, rtol=1e-3, atol=1e-3)


def test_reconstruction_refined_columns(tiny, tiny_twin):
    import torch
    ins, windows = tiny
    rep = ins.reconstruct(windows, batch_size=BATCH, refine=True)
    assert rep.table.shape == (N_WINDOWS, 7) and np.isfinite(rep.table).all()
    _check_rows(rep.table[:, :5], tiny_twin[0], TINY.latent_dim, "refined")
    x = torch.from_numpy(windows[:BATCH]).cuda()
    rec = ins.engine.decode(0, ins.engine.encode(0, x)[0])
    mu2, lv2, _ = ins.engine.encode(0, rec.reshape(BATCH, TINY.seq_len, -1))
    want = T.report_rows(mu2.cpu().numpy(), lv2.cpu().numpy())
    np.testing.assert_allclose(rep.table[:BATCH, 5:], want[:, :2], rtol=1e-12, atol=1e-12 * TINY.latent_dim)
    assert set(rep.means) == set(rep.keys) and "vae refined mu error is: {}".format(rep.means["refined_mu_error"]) in rep.lines()


def test_sampled_posterior_is_a_function_of_the_seed(tiny):
    ins, windows = tiny
    a, b = (ins.reconstruct(windows, batch_size=BATCH, posterior="sample", seed=4) for _ in range(2))
    assert np.array_equal(a.table.view(np.uint64), b.table.view(np.uint64)) and np.array_equal(a.sums.view(np.uint64), b.sums.view(np.uint64))
    c = ins.reconstruct(windows, batch_size=BATCH, posterior="sample", seed=5)
    assert not np.array_equal(a.table[:, 3], c.table[:, 3])
    # the encoder does not see the noise: the latent columns are the posterior mean's
    assert np.array_equal(a.table[:, :3].view(np.uint64), c.table[:, :3].view(np.uint64))


def test_engine_methods_check_their_arguments(tiny):
    import torch
    ins, _ = tiny
    eng, D = ins.engine, TINY.latent_dim
    z = torch.zeros(2, D, device="cuda")
    with pytest.raises(ValueError):
        eng.latent_paths(z, z, 1)
    with pytest.raises(ValueError):
        eng.latent_paths(z, z, 6, mode="cubic")
    with pytest.raises(ValueError):
        eng.latent_paths(z, z[:1], 6)
    with pytest.raises(ValueError):
        eng.latent_report(z, z, x=torch.zeros(2, 10, 45, device="cuda"))
    with pytest.raises(TypeError):
        eng.latent_report(z, z.double())
    with pytest.raises(ValueError):
        eng.latent_report(z, z, cols=torch.zeros(3, D + 1, device="cuda", dtype=torch.float64))
    assert tuple(eng.latent_paths(z[0], z[1], 4, "spherical").shape) == (1, 4, D)
    big = torch.randn(3 * ins.max_windows, D, device="cuda")          # not limited by max_windows
    assert tuple(eng.latent_report(big, big).shape) == (3 * ins.max_windows, 5)
    assert tuple(eng.latent_paths(big, big.flip(0), 3).shape) == (3 * ins.max_windows, 3, D)


# ------------------------------------------------------------------------------------------------------------------ the writers
def _sphere_centres(path):
    v, c, t = mesh_twin.read_ply(path)
    return v[:15 * 762].reshape(15, 762, 3).mean(axis=1)


def test_samples_are_the_seeded_draw_and_their_meshes(tiny, tmp_path):
    import torch
    from globalegomocap_amd import meshes, vae_inspect
    ins, _ = tiny
    z, poses = ins.sample(3, seed=2)
    torch.manual_seed(2)
    assert torch.equal(z.cpu(), torch.randn(3, TINY.latent_dim))
    assert tuple(poses.shape) == (3, 10, 15, 3)
    np.testing.assert_allclose(poses.cpu().numpy(), ins.engine.decode(0, z).cpu().numpy(), rtol=1e-4, atol=1e-5)
    assert ins.write_samples(str(tmp_path)) == 30
    assert sorted(os.listdir(tmp_path)) == ["sample_0", "sample_1", "sample_2"]
    want = poses.cpu().numpy().astype(np.float64)
    for i, files in enumerate(vae_inspect.sample_paths(str(tmp_path), 3, 10)):
        assert sorted(os.listdir(os.path.dirname(files[0]))) == sorted("%d.ply" % j for j in range(10))
        for j, path in enumerate(files):
            np.testing.assert_allclose(_sphere_centres(path), want[i, j], rtol=0, atol=1e-9, err_msg=path)          # test_meshes_gpu's tolerance
    v, c, t = meshes.read_ply(os.path.join(str(tmp_path), "sample_2", "9.ply"))
    assert v.shape == (mesh_twin.N_VERTICES, 3) and t.shape == (mesh_twin.N_TRIANGLES, 3)


def test_interpolation_folders_and_frames(tiny, tmp_path):
    import torch
    from globalegomocap_amd import render, vae_inspect
    ins, windows = tiny
    z, poses = ins.interpolate(windows[3], windows[90], steps=4, seed=6)
    assert tuple(z.shape) == (4, TINY.latent_dim) and tuple(poses.shape) == (4, 10, 15, 3)
    # the ends are the two windows' latents, drawn a then b (interpolant.py:101-102); between them the reference's straight line
    eps_a, eps_b = vae_inspect.draw_pair_eps(1, TINY.latent_dim, 6)
    x = torch.from_numpy(windows[[3, 90]]).cuda()
    za = ins.engine.encode(0, x[:1], eps_a)[2]
    zb = ins.engine.encode(0, x[1:], eps_b)[2]
    assert torch.equal(z[0], za[0]) and torch.equal(z[3], zb[0])
    assert np.array_equal(z.cpu().numpy(), T.linear_path(za[0].cpu().numpy(), zb[0].cpu().numpy(), 4))
    np.testing.assert_allclose(poses[0].cpu().numpy(), ins.engine.decode(0, za)[0].cpu().numpy(), rtol=1e-4, atol=1e-5)
    n = ins.write_interpolation(str(tmp_path), render=True, size=(160, 120))
    assert n == 4 * (10 + 10 + 1)
    assert sorted(os.listdir(tmp_path)) == ["0", "1", "2", "3"]
    want = poses.cpu().numpy().astype(np.float64)
    for s, files in enumerate(vae_inspect.interpolation_paths(str(tmp_path), 4, 10)):
        assert sorted(f for f in os.listdir(os.path.dirname(files[0])) if f.endswith(".ply")) == ["out_%04d.ply" % j for j in range(10)]
        for j in (0, 9):
            np.testing.assert_allclose(_sphere_centres(files[j]), want[s, j], rtol=0, atol=1e-9, err_msg=files[j])
    for j in range(10):          # folder 0 is the mesh of decode(z_a)
        np.testing.assert_allclose(_sphere_centres(os.path.join(str(tmp_path), "0", "out_%04d.ply" % j)), want[0, j], rtol=0, atol=1e-9)
    img = render.read_png(os.path.join(str(tmp_path), "2", "frame_0005.png"))
    assert img.shape == (120, 160, 3) and (img != 255).any() and (img == 255).any()
    assert render.read_png(os.path.join(str(tmp_path), "2", "overview_step.png")).shape == (120, 160, 3)
    # the deterministic alternative, and P pairs at once along the great circle
    zm, _ = ins.interpolate(windows[3], windows[90], steps=3, posterior="mean")
    assert torch.equal(zm[0], ins.engine.encode(0, x[:1])[0][0])
    zp, pp = ins.interpolate(windows[:2], windows[5:7], steps=5, mode="spherical", posterior="mean")
    assert tuple(zp.shape) == (2, 5, TINY.latent_dim) and tuple(pp.shape) == (2, 5, 10, 15, 3)


def test_reconstructions_are_drawn_over_their_inputs(tiny, tmp_path):
    from globalegomocap_amd import render
    ins, windows = tiny
    rep = ins.reconstruct(windows, batch_size=BATCH)
    ids = rep.worst(2)
    assert ins.write_reconstructions(ids, str(tmp_path), size=(160, 120)) == 2 * (10 + 2)
    assert sorted(os.listdir(tmp_path)) == sorted("window_%d" % i for i in ids)
    img = render.read_png(os.path.join(str(tmp_path), "window_%d" % ids[0], "frame_0000.png")).reshape(-1, 3).astype(int)
    assert img.shape[0] == 160 * 120
    r, g, b = img[:, 0], img[:, 1], img[:, 2]
    # the input in (shaded) green (44, 160, 44), the reconstruction in blue (31, 119, 180); the background is white
    assert ((g > 2 * r) & (g > 2 * b)).any() and ((b > g) & (g > 2 * r)).any() and (img.sum(axis=1) == 765).any()
