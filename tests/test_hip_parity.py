"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the committed golden
vectors of the reference.  Run on a MI355X with `pytest -m gpu`."""
import os
import pickle

import numpy as np
import pytest

from globalegomocap_amd import synth, vae as vae_schema
from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
from oracle import np_oracle as O
from helpers import TINY, FULL, oracle_camera, heat_from_centres, sd_from_npz, oracle_stage_losses
from energy_f64 import terms64, bilinear

pytestmark = pytest.mark.gpu

W_LOCAL = (1e-6, 1e-5, 1e-2, 0.0, 1e-2)      # (w3d, smooth, bone, vae, reproj)   optimizer.py:355-358
W_GLOBAL = (1e-2, 1e-3, 1e-2, 0.0, 0.0)      # optimizer.py:352-353
W_ALL = (7e-3, 2e-2, 5e-2, 3e-3, 4e-2)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch


def _engine(shape, max_windows=16):
    from globalegomocap_amd.engine import WindowEngine
    return WindowEngine(shape, FisheyeCamera.from_json(DEFAULT_CALIBRATION), max_windows=max_windows)


def _ew(w):
    from globalegomocap_amd.engine import energy_weights
    return energy_weights(*w)


def _check_parts_at_device_pose(parts_dev, X_dev, pose0, mb, heat_w, cam):
    """The energy code alone, whatever the decoder's precision: the five parts against float64 (tests/energy_f64.py) AT THE POSE THE
    DEVICE DECODED, 1e-5 relative per term (test_energy_terms_gpu.py, check (a)).  The reprojection term gets, on top, what the fp32
    texel coordinate can cost on THESE heat-maps: the callers' random-weight decoders put the joints 5 .. 8 texels from their Gaussian
    peaks (E_reproj ~ 1e-5 .. 1e-3), where a sample changes by r / sigma^2 ~ 3 of its value per texel; u = ux * rho + cx and the
    three steps to the texel coordinate each round to half an ulp of a number below 1024 (6.1e-5 px): 4 * 0.5 * 6.1e-5 px * 63 / 1024
    = 7.5e-6 texel per axis, times the sum of the samples' |slopes| (the fp32 oracle itself is 1.7e-5 of the term from float64 here)."""
    p64, _, (ix, iy) = terms64(X_dev, pose0, mb, heat_w, cam, O.PARENTS)
    np.testing.assert_allclose(parts_dev[:4], p64[:4], rtol=1e-5, atol=0)
    _, dix, diy = bilinear(np.asarray(heat_w), ix.ravel(), iy.ravel())
    slack = 7.5e-6 * float(np.sum(np.abs(dix) + np.abs(diy)))
    assert abs(parts_dev[4] - p64[4]) <= 1e-5 * abs(p64[4]) + slack, (parts_dev[4], p64[4], slack)


def test_library_is_the_hip_one(torch_cuda):
    from globalegomocap_amd import _capi
    lib = _capi.load_library()
    assert lib.gem_version() == 1
    assert os.path.basename(_capi.LIB_PATH) == "libgem_hip.so"


def test_operators_against_reference_golden(torch_cuda, golden):
    """encode / decode / energies / dL/dz of the tiny network vs the reference's own numbers."""
    g = golden("ops_tiny")
    sd = vae_schema.synthetic_state_dict(TINY, int(g["weights_seed"]))
    eng = _engine(TINY)
    eng.load_vae(0, sd)
    pose = g["pose"]
    mu, logvar, z = eng.encode(0, pose.reshape(1, 10, 45))
    np.testing.assert_allclose(mu.cpu().numpy(), g["mu"], rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(logvar.cpu().numpy(), g["logvar"], rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(z.cpu().numpy(), g["mu"], rtol=1e-4, atol=5e-6)       # eps=None -> z = mu
    X = eng.decode(0, g["z"])
    np.testing.assert_allclose(X[0].cpu().numpy(), g["X"], rtol=1e-4, atol=5e-6)
    mb = eng.mean_bone_length(pose)
    np.testing.assert_allclose(mb.cpu().numpy(), g["mean_bone"], rtol=1e-5, atol=1e-6)
    heat = heat_from_centres(g["heat_centres"])
    for tag, w in (("local", W_LOCAL), ("global", W_GLOBAL), ("allterms", W_ALL)):
        E, parts, dz, X2 = eng.energy_grad(0, g["z"], pose[None], mb, _ew(w), heat, np.zeros(1, np.int32))
        parts = parts.cpu().numpy()[0]
        ref_parts = g["parts_" + tag]
        k = 5 if w[4] != 0 else 4
        np.testing.assert_allclose(parts[:k], ref_parts[:k], rtol=5e-5, atol=1e-7)
        ref_tot = float(g["total_" + tag])
        assert abs(float(E[0]) - ref_tot) <= 5e-5 * abs(ref_tot) + 1e-8
        ref = g["dz_" + tag]
        assert np.abs(dz.cpu().numpy() - ref).max() <= 5e-4 * np.abs(ref).max()


@pytest.mark.parametrize("shape,seed,B", [(TINY, 11, 5), (FULL, 5, 3)])
def test_energy_and_gradient_against_oracle(torch_cuda, shape, seed, B):
    sd = vae_schema.synthetic_state_dict(shape, seed)
    eng = _engine(shape, max_windows=8)
    eng.load_vae(1, sd)
    vae = O.fold_vae(sd)
    cam = oracle_camera()
    seq = synth.make_sequence(n_frames=8 * (B - 1) + 10, seed=21)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    starts = (8 * np.arange(B)).astype(np.int32)
    pose = np.stack([est[s:s + 10] for s in starts])
    rng = np.random.default_rng(3)
    mu, _ = O.encode(vae, pose.reshape(B, 10, 45))
    z = (mu + 0.1 * rng.normal(size=mu.shape)).astype(np.float32)
    mb = O.mean_bone_length(est)
    # make the decoded pose land on the heat-maps for one window so that the reprojection term is alive
    for w in (W_LOCAL, W_GLOBAL, W_ALL):
        E, parts, dz, X = eng.energy_grad(1, z, pose, mb, _ew(w), heat, starts)
        for b in range(B):
            Xo, acts = O.decode(vae, z[b:b + 1], keep=True)
            f, p, dX = O.energy_and_grad(Xo[0], pose[b], mb, O.Weights(*w), cam, heat[starts[b]:starts[b] + 10])
            dzo = O.decode_backward(vae, dX[None], acts)[0]
            np.testing.assert_allclose(X[b].cpu().numpy(), Xo[0], rtol=2e-4, atol=2e-5)
            np.testing.assert_allclose(parts[b].cpu().numpy(), p, rtol=2e-4, atol=1e-6)
            assert abs(float(E[b]) - f) <= 2e-4 * abs(f) + 1e-7
            assert np.abs(dz[b].cpu().numpy() - dzo).max() <= 2e-3 * np.abs(dzo).max() + 1e-8


def test_reprojection_term_alive_and_edge_samples(torch_cuda):
    """Poses placed exactly under the heat-map peaks, at the image border and outside the image."""
    sd = vae_schema.synthetic_state_dict(TINY, 11)
    eng = _engine(TINY)
    eng.load_vae(0, sd)
    vae = O.fold_vae(sd)
    cam = oracle_camera()
    seq = synth.make_sequence(n_frames=10, seed=5, noise=0.0)
    pose = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    z = np.zeros((1, 32), np.float32)
    X = O.decode(vae, z)[0]
    # heat-maps centred on the *decoded* pose so that E_reproj ~ -150 and its gradient is non-trivial
    from globalegomocap_amd.camera import FisheyeCamera
    uv = FisheyeCamera.from_json(DEFAULT_CALIBRATION).project_numpy(X.reshape(-1, 3).astype(np.float64)).reshape(10, 15, 2)
    ix, iy = synth.heatmap_coords(uv)
    heat2 = synth.gaussian_heatmaps(ix + 0.3, iy - 0.2)
    mb = O.mean_bone_length(pose)
    E, parts, dz, Xg = eng.energy_grad(0, z, pose[None], mb, _ew(W_ALL), heat2, np.zeros(1, np.int32))
    f, p, dX = O.energy_and_grad(X, pose, mb, O.Weights(*W_ALL), cam, heat2)
    assert abs(p[4]) > 1.0            # the term is alive (mostly inside the image)
    np.testing.assert_allclose(parts[0].cpu().numpy(), p, rtol=2e-4, atol=1e-6)
    Xo, acts = O.decode(vae, z, keep=True)
    dzo = O.decode_backward(vae, dX[None], acts)[0]
    assert np.abs(dz[0].cpu().numpy() - dzo).max() <= 2e-3 * np.abs(dzo).max()


def test_lbfgs_stage_against_reference_golden(torch_cuda, golden):
    g = golden("lbfgs_tiny")
    pose, heat = g["pose"], heat_from_centres(g["heat_centres"])
    for tag, prefix, w in (("local", "local/", W_LOCAL), ("global", "global/", W_GLOBAL),
                           ("globalstrong", "global/", (1.0, 0.1, 0.01, 0.0, 0.0))):
        eng = _engine(TINY)
        eng.load_vae(0, sd_from_npz(g, prefix))
        mb = eng.mean_bone_length(pose.astype(np.float32))
        out, stats = eng.optimize_stage(0, pose[None], mb, g[tag + "_eps"][None], _ew(w), heat, np.zeros(1, np.int32))
        st = stats.cpu().numpy()[0]
        ref_evals = len(g[tag + "_trace"])
        assert st[3] == 1
        assert abs(int(st[1]) - ref_evals) <= 3, (tag, st, ref_evals)
        err = np.linalg.norm(out[0].cpu().numpy() - g[tag + "_out"], axis=-1).mean()
        assert err < 0.5e-3, (tag, err)              # 0.5 mm
        loss = np.array([st[2]], dtype=np.int32).view(np.float32)[0]
        assert abs(loss - g[tag + "_trace"].min()) <= 2e-3 * abs(g[tag + "_trace"].min()) + 1e-6


def test_lbfgs_stage_full_size_against_oracle_and_golden(torch_cuda, golden):
    g = golden("lbfgs_full")
    sd = vae_schema.synthetic_state_dict(FULL, int(g["weights_seed"]))
    eng = _engine(FULL, max_windows=4)
    eng.load_vae(0, sd)
    pose, heat = g["pose"], heat_from_centres(g["heat_centres"])
    mb = eng.mean_bone_length(pose.astype(np.float32))
    # default weights: the reference stops at its first test (g.d > -1e-6); so must we
    for tag, w in (("local", W_LOCAL), ("global", W_GLOBAL)):
        out, stats = eng.optimize_stage(0, pose[None], mb, g[tag + "_eps"][None], _ew(w), heat, np.zeros(1, np.int32))
        st = stats.cpu().numpy()[0]
        assert st[1] == 1 and st[3] == 1
        np.testing.assert_allclose(out[0].cpu().numpy(), g[tag + "_out"], rtol=2e-3, atol=2e-5)
    # strong weights: a long run on a random-init network (late iterates are chaotic): the closure values follow the
    # reference's trace while the trajectories are still together, and the run achieves the reference's energy
    for tag, w in (("localstrong", (1e-1, 1e-1, 1.0, 1e-3, 1e-2)), ("globalstrong", (1.0, 1e-1, 1.0, 0.0, 0.0))):
        out, stats = eng.optimize_stage(0, pose[None], mb, g[tag + "_eps"][None], _ew(w), heat, np.zeros(1, np.int32))
        tr = eng.read_trace(1)[0]
        st = stats.cpu().numpy()[0]
        loss = np.array([st[2]], dtype=np.int32).view(np.float32)[0]
        ref = g[tag + "_trace"]
        assert st[3] == 1 and st[1] >= 20 and int(np.isfinite(tr).sum()) == st[1]
        # (random-init weights: the directional derivatives are cancellation-dominated, the third trial step already
        # depends on their last digits; the tight full-size trace checks are in test_hip_full_size.py)
        np.testing.assert_allclose(tr[:2], ref[:2], rtol=2e-5, atol=1e-7, err_msg=tag)
        np.testing.assert_allclose(tr[:4], ref[:4], rtol=2e-3, atol=1e-7, err_msg=tag)
        print("full-size random-init %s: evals %d / %d, final loss %.6e / %.6e" % (tag, st[1], len(ref), loss, ref.min()))
        assert abs(int(st[1]) - len(ref)) <= 3, (tag, st[1], len(ref))
        assert abs(loss - ref.min()) <= 0.05 * abs(ref.min()), (tag, loss, ref.min())


def test_batch_is_independent_of_its_neighbours(torch_cuda, golden):
    """A window optimised alone and inside a ragged batch gives the same result (bitwise)."""
    g = golden("lbfgs_tiny")
    sd = sd_from_npz(g, "local/")
    eng = _engine(TINY, max_windows=16)
    eng.load_vae(0, sd)
    seq = synth.make_sequence(n_frames=58, seed=9)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    starts = np.array([0, 8, 16, 24, 32, 40, 48], np.int32)        # last window ends at the last frame
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = eng.mean_bone_length(est)
    rng = np.random.default_rng(1)
    eps = rng.normal(size=(7, 32)).astype(np.float32)
    out_all, st_all = eng.optimize_stage(0, pose, mb, eps, _ew(W_LOCAL), heat, starts)
    out_one, st_one = eng.optimize_stage(0, pose[6:7], mb, eps[6:7], _ew(W_LOCAL), heat, starts[6:7])
    assert np.array_equal(out_all[6].cpu().numpy(), out_one[0].cpu().numpy())
    assert np.array_equal(st_all[6].cpu().numpy(), st_one[0].cpu().numpy())
    # B = 0 is a no-op
    out0, st0 = eng.optimize_stage(0, pose[:0], mb, eps[:0], _ew(W_LOCAL), heat, starts[:0])
    assert out0.shape[0] == 0


def test_rigid_transforms_and_window_pipeline(torch_cuda, golden, tmp_path):
    """main() mirror on the reference's golden pipeline run (tiny fitted VAEs, 100 frames, 12 windows)."""
    import torch
    from globalegomocap_amd import optimizer as gopt
    g = golden("pipeline_tiny")
    lt = golden("lbfgs_tiny")
    data = synth.make_sequence(n_frames=100, seed=int(g["seq_seed"]))
    d = tmp_path / "chunk0"
    d.mkdir()
    with open(d / "test_data.pkl", "wb") as f:
        pickle.dump({k: data[k] for k in ("estimated_local_skeleton", "gt_global_skeleton", "camera_pose_list", "heatmap_list")}, f)
    torch.manual_seed(int(g["eps_seed"]))
    eps = torch.randn(24, 32)
    res = gopt.main(str(d), DEFAULT_CALIBRATION, 0.0, 0.0, float(g["smooth"]), 0.01, float(g["weight_3d"]), 0.01,
                    final_smooth=True, global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"),
                    eps=eps, return_stats=True)
    errors, est_seq, mid_local, opt_seq, gt_seq, stats = res
    assert (stats["status"] == 1).all()
    assert opt_seq.shape == (98, 15, 3)
    np.testing.assert_allclose(np.asarray(est_seq), g["est_smooth"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(np.asarray(gt_seq), g["gt_smooth"], rtol=1e-9, atol=1e-12)
    mid = np.linalg.norm(np.asarray(mid_local) - g["mid_local_smooth"], axis=-1).mean()
    fin = np.linalg.norm(opt_seq - g["opt_smooth"], axis=-1).mean()
    assert mid < 0.5e-3 and fin < 0.5e-3, (mid, fin)
    # headline accuracy gate: |MPJPE_hip - MPJPE_reference| <= 0.5 mm on optimized_global_mpjpe
    assert abs(errors["optimized_global_mpjpe"] - float(g["err_smooth/optimized_global_mpjpe"])) < 0.5e-3
    for k in ("original_global_mpjpe", "original_camera_pos_error", "original_aligned_global_mpjpe",
              "aligned_original_mpjpe", "bone_length_aligned_original_mpjpe"):
        assert abs(errors[k] - float(g["err_smooth/" + k])) < 1e-9, k


def test_single_window_interface(torch_cuda, golden):
    """BodyPoseOptimizer.optimize_pose_seq_pytorch_LBFGS drop-in call, eps from the global torch RNG."""
    import torch
    from globalegomocap_amd.optimizer import BodyPoseOptimizer
    g = golden("lbfgs_tiny")
    pose, heat = g["pose"], heat_from_centres(g["heat_centres"])
    bpo = BodyPoseOptimizer(DEFAULT_CALIBRATION, torch.from_numpy(pose).float(), sd_from_npz(g, "local/"), seq_len=10,
                            network_seq_len=10, latent_dim=32)
    bpo.set_weights(vae_weight=0.0, gmm_weight=0.0, smooth_weight=1e-5, bone_length_weight=1e-2, weight_3d=1e-6,
                    reproj_weight=1e-2)
    torch.manual_seed(1234)
    out = bpo.optimize_pose_seq_pytorch_LBFGS(pose, heat, pose.copy())
    assert out.dtype == np.float32 and out.shape == (10, 15, 3)
    assert np.linalg.norm(out - g["local_out"], axis=-1).mean() < 0.5e-3
    with pytest.raises(RuntimeError):
        BodyPoseOptimizer(DEFAULT_CALIBRATION, torch.from_numpy(pose).float(), sd_from_npz(g, "local/"), seq_len=10,
                          network_seq_len=10, latent_dim=2048)


def test_window_pipeline_with_rotating_cameras_against_oracle(torch_cuda, golden):
    """gem_optimize_windows (both stages + fp64 rigid transforms) on SLAM-like jittered cameras."""
    import torch
    from globalegomocap_amd.engine import WindowEngine, stats_to_numpy
    from globalegomocap_amd.sequence import window_starts
    lt = golden("lbfgs_tiny")
    sd_l, sd_g = sd_from_npz(lt, "local/"), sd_from_npz(lt, "global/")
    data = synth.make_sequence(n_frames=34, seed=13, cam_jitter=(1.0, 0.004))
    est = np.asarray(data["estimated_local_skeleton"])
    cams = np.asarray(data["camera_pose_list"])
    heat = np.asarray(data["heatmap_list"], dtype=np.float32)
    starts = window_starts(34)                       # 0, 8, 16, 24
    B = len(starts)
    eng = _engine(TINY, max_windows=8)
    eng.load_vae(0, sd_l)
    eng.load_vae(1, sd_g)
    dev = eng.device
    rng = np.random.default_rng(5)
    eps = rng.normal(size=(2 * B, 32)).astype(np.float32)
    w_l, w_g = (1e-4, 1e-3, 1e-2, 0.0, 1e-2), (1.0, 0.1, 1e-2, 0.0, 0.0)
    pose_d = torch.as_tensor(est, dtype=torch.float32, device=dev).contiguous()
    mb = eng.mean_bone_length(pose_d).reshape(1, 15).expand(B, 15).contiguous()
    e3 = torch.as_tensor(eps.reshape(B, 2, 32))
    mid, glob, stats = eng.optimize_windows(pose_d, torch.as_tensor(cams, dtype=torch.float64, device=dev).contiguous(),
                                            torch.as_tensor(heat, device=dev).contiguous(),
                                            torch.as_tensor(starts, dtype=torch.int32, device=dev), mb,
                                            e3[:, 0].contiguous().to(dev), e3[:, 1].contiguous().to(dev), _ew(w_l), _ew(w_g))
    st = stats_to_numpy(stats)
    assert (st["status"] == 1).all()
    ref = O.optimize_sequence(data, O.fold_vae(sd_l), O.fold_vae(sd_g), oracle_camera(), eps, O.Weights(*w_l), O.Weights(*w_g))
    from globalegomocap_amd.sequence import merge_batches
    got_opt, got_mid = merge_batches(glob.cpu().numpy()), merge_batches(mid.cpu().numpy())
    d_mid = np.linalg.norm(got_mid - ref["mid_local"], axis=-1).mean()
    d_opt = np.linalg.norm(got_opt - ref["opt"], axis=-1).mean()
    assert d_mid < 1e-3 and d_opt < 1e-3, (d_mid, d_opt)
    gt = ref["gt"]
    assert abs(np.linalg.norm(got_opt - gt, axis=-1).mean() - np.linalg.norm(ref["opt"] - gt, axis=-1).mean()) < 0.5e-3


def test_full_size_batch_properties_at_baseline_size(torch_cuda):
    """BASELINE configs[1] size (240 windows, D=2048): size-independent properties of the batched optimiser."""
    import torch
    from globalegomocap_amd.engine import stats_to_numpy
    from globalegomocap_amd.sequence import window_starts
    sd = vae_schema.synthetic_state_dict(FULL, 5)
    n_chunks, B = 20, 240
    eng = _engine(FULL, max_windows=B)
    eng.load_vae(0, sd)
    seq = synth.make_sequence_device(n_chunks * 100, seed=77, device=eng.device)
    starts = np.concatenate([c * 100 + window_starts(100) for c in range(n_chunks)]).astype(np.int32)
    est = seq["est_local_np"].astype(np.float32)
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = eng.mean_bone_length(est[:100])
    rng = np.random.default_rng(9)
    eps = rng.normal(size=(B, 2048)).astype(np.float32)
    w = _ew((1e-1, 1e-1, 1.0, 1e-3, 1e-2))                     # strong weights: the random-init net iterates
    mu, lv, z0 = eng.encode(0, pose.reshape(B, 10, 45), eps)
    E0, _, _, _ = eng.energy_grad(0, z0, pose, mb, w, seq["heat"], starts)
    out, stats = eng.optimize_stage(0, pose, mb, eps, w, seq["heat"], starts)
    st = stats_to_numpy(stats)
    assert (st["status"] == 1).all()
    assert (st["func_evals"] <= 32).all() and (st["n_iter"] <= 25).all() and (st["func_evals"] >= 1).all()
    # Armijo: the accepted loss never exceeds the loss at z0
    assert (st["final_loss"] <= E0.cpu().numpy().astype(np.float32) * (1 + 1e-6) + 1e-6).all()
    assert st["func_evals"].mean() > 20
    # determinism and permutation equivariance (windows are independent): bitwise
    out2, stats2 = eng.optimize_stage(0, pose, mb, eps, w, seq["heat"], starts)
    assert torch.equal(out, out2) and torch.equal(stats, stats2)
    perm = rng.permutation(B)
    out3, stats3 = eng.optimize_stage(0, pose[perm], mb, eps[perm], w, seq["heat"], starts[perm])
    assert torch.equal(out3, out[torch.as_tensor(perm, device=out.device)])
    assert np.isfinite(out.cpu().numpy()).all()


@pytest.mark.parametrize("mode,tol_x,tol_e,tol_g", [("bf16x3", 2e-5, 2e-4, 2e-3), ("bf16", 3e-3, 5e-2, 1.5e-1)])
def test_precision_modes_energy_and_gradient(torch_cuda, mode, tol_x, tol_e, tol_g):
    """Wide products in split-bf16 (fp32-grade) and plain bf16 against the fp32 oracle, full-size network.
    (bf16, round 4: the narrow layers run in bf16 at EVERY batch size now -- the multi-window tail with one row tile per workgroup
    replaced the fp32 one-window tail below 256 windows -- so a 4-window call carries the bf16 mode's full rounding: the worst
    gradient entry moved from 7 % to 10 % of the largest one; the gate on it went from 0.10 to 0.15.)"""
    sd = vae_schema.synthetic_state_dict(FULL, 5)
    eng = _engine(FULL, max_windows=8)
    eng.load_vae(0, sd)
    eng.set_precision(mode)
    vae = O.fold_vae(sd)
    cam = oracle_camera()
    B = 4
    seq = synth.make_sequence(n_frames=8 * (B - 1) + 10, seed=33)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    starts = (8 * np.arange(B)).astype(np.int32)
    pose = np.stack([est[s:s + 10] for s in starts])
    rng = np.random.default_rng(4)
    mu, _ = O.encode(vae, pose.reshape(B, 10, 45))
    z = (mu + 0.1 * rng.normal(size=mu.shape)).astype(np.float32)
    mb = O.mean_bone_length(est)
    mu_d, lv_d, _ = eng.encode(0, pose.reshape(B, 10, 45))
    assert np.abs(mu_d.cpu().numpy() - mu).max() <= 50 * tol_x * max(1.0, np.abs(mu).max())
    E, parts, dz, X = eng.energy_grad(0, z, pose, mb, _ew(W_ALL), heat, starts)
    for b in range(B):
        Xo, acts = O.decode(vae, z[b:b + 1], keep=True)
        f, p, dX = O.energy_and_grad(Xo[0], pose[b], mb, O.Weights(*W_ALL), cam, heat[starts[b]:starts[b] + 10])
        dzo = O.decode_backward(vae, dX[None], acts)[0]
        assert np.abs(X[b].cpu().numpy() - Xo[0]).max() <= tol_x * max(1.0, np.abs(Xo[0]).max())
        assert abs(float(E[b]) - f) <= tol_e * abs(f) + 1e-7
        assert np.abs(dz[b].cpu().numpy() - dzo).max() <= tol_g * np.abs(dzo).max() + 1e-8
        _check_parts_at_device_pose(parts[b].cpu().numpy(), X[b].cpu().numpy(), pose[b], mb, heat[starts[b]:starts[b] + 10], cam)


@pytest.mark.parametrize("mode,tol_mm", [("bf16x3", 0.5), ("bf16", 1.5)])
def test_precision_modes_window_pipeline_mpjpe(torch_cuda, golden, tmp_path, mode, tol_mm):
    """main() mirror in the faster arithmetic modes against the reference's golden run."""
    import torch
    from globalegomocap_amd import optimizer as gopt
    g = golden("pipeline_tiny")
    lt = golden("lbfgs_tiny")
    data = synth.make_sequence(n_frames=100, seed=int(g["seq_seed"]))
    d = tmp_path / "chunk0"
    d.mkdir()
    with open(d / "test_data.pkl", "wb") as f:
        pickle.dump({k: data[k] for k in ("estimated_local_skeleton", "gt_global_skeleton", "camera_pose_list", "heatmap_list")}, f)
    torch.manual_seed(int(g["eps_seed"]))
    eps = torch.randn(24, 32)
    opt = gopt.SequenceOptimizer(DEFAULT_CALIBRATION, sd_from_npz(lt, "global/"), sd_from_npz(lt, "local/"), max_windows=12)
    opt.engine.set_precision(mode)
    errors = gopt.main(str(d), DEFAULT_CALIBRATION, 0.0, 0.0, float(g["smooth"]), 0.01, float(g["weight_3d"]), 0.01,
                       final_smooth=True, eps=eps, optimizer=opt)[0]
    ref = float(g["err_smooth/optimized_global_mpjpe"])
    assert abs(errors["optimized_global_mpjpe"] - ref) * 1e3 < tol_mm, (mode, errors["optimized_global_mpjpe"], ref)


@pytest.mark.parametrize("shape,seed,B", [(TINY, 11, 4), (FULL, 5, 3)])
def test_unfused_layer_path(torch_cuda, monkeypatch, shape, seed, B):
    """Large batches run the narrow layers as batched GEMMs + the stand-alone energy kernel instead of the fused
    tail kernel; force that path (GEM_NO_TAIL) and compare it with the oracle and with the fused path."""
    sd = vae_schema.synthetic_state_dict(shape, seed)
    vae = O.fold_vae(sd)
    cam = oracle_camera()
    seq = synth.make_sequence(n_frames=8 * (B - 1) + 10, seed=41)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    starts = (8 * np.arange(B)).astype(np.int32)
    pose = np.stack([est[s:s + 10] for s in starts])
    rng = np.random.default_rng(6)
    mu, _ = O.encode(vae, pose.reshape(B, 10, 45))
    z = (mu + 0.1 * rng.normal(size=mu.shape)).astype(np.float32)
    mb = O.mean_bone_length(est)
    eps = rng.normal(size=(B, shape.latent_dim)).astype(np.float32)
    w = (1e-1, 1e-1, 1.0, 1e-3, 1e-2)
    results = {}
    for tag, no_tail in (("fused", False), ("batched", True)):
        monkeypatch.setenv("GEM_DEV", "1")       # developer switches are honoured only with GEM_DEV=1
        if no_tail:
            monkeypatch.setenv("GEM_NO_TAIL", "1")
        else:
            monkeypatch.delenv("GEM_NO_TAIL", raising=False)
        eng = _engine(shape, max_windows=8)
        eng.load_vae(0, sd)                      # the path is chosen when the weights are loaded
        E, parts, dz, X = eng.energy_grad(0, z, pose, mb, _ew(W_ALL), heat, starts)
        out, stats = eng.optimize_stage(0, pose, mb, eps, _ew(w), heat, starts)
        results[tag] = (E.cpu().numpy(), dz.cpu().numpy(), X.cpu().numpy(), out.cpu().numpy(), stats.cpu().numpy())
    E, dz, X, out, st = results["batched"]
    for b in range(B):
        Xo, acts = O.decode(vae, z[b:b + 1], keep=True)
        f, p, dX = O.energy_and_grad(Xo[0], pose[b], mb, O.Weights(*W_ALL), cam, heat[starts[b]:starts[b] + 10])
        dzo = O.decode_backward(vae, dX[None], acts)[0]
        np.testing.assert_allclose(X[b], Xo[0], rtol=2e-4, atol=2e-5)
        assert abs(E[b] - f) <= 2e-4 * abs(f) + 1e-7
        assert np.abs(dz[b] - dzo).max() <= 2e-3 * np.abs(dzo).max() + 1e-8
    assert (st[:, 3] == 1).all()
    # both paths do the same arithmetic up to summation order
    np.testing.assert_allclose(results["fused"][0], E, rtol=1e-5)
    assert np.abs(results["fused"][1] - dz).max() <= 1e-4 * np.abs(dz).max()


@pytest.mark.parametrize("T", [12, 16])
def test_fused_tail_with_windows_longer_than_its_thread_count(torch_cuda, monkeypatch, T):
    """Windows of T >= 12 frames hold more than 512 pose values (T*15*3 = 540 / 720): the fused tail's one-element-per-thread
    parking of the energy inputs does not cover them, so it must leave them to energy_window's own global reads.  The fused
    path against the batched layers + stand-alone energy kernel (GEM_NO_TAIL), and against the oracle."""
    shape = vae_schema.VAEShape(latent_dim=32, seq_len=T, hidden=(16, 16, 32, 32, 64))
    sd = vae_schema.synthetic_state_dict(shape, 13)
    vae = O.fold_vae(sd, seq_len=T)
    cam = oracle_camera()
    B = 3
    seq = synth.make_sequence(n_frames=8 * (B - 1) + T, seed=43)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    starts = (8 * np.arange(B)).astype(np.int32)
    pose = np.stack([est[s:s + T] for s in starts])
    rng = np.random.default_rng(7)
    mu, _ = O.encode(vae, pose.reshape(B, T, 45))
    z = (mu + 0.1 * rng.normal(size=mu.shape)).astype(np.float32)
    mb = O.mean_bone_length(est)
    res = {}
    monkeypatch.setenv("GEM_DEV", "1")
    for tag, no_tail in (("fused", False), ("batched", True)):
        if no_tail:
            monkeypatch.setenv("GEM_NO_TAIL", "1")
        else:
            monkeypatch.delenv("GEM_NO_TAIL", raising=False)
        eng = _engine(shape, max_windows=4)
        eng.load_vae(0, sd)
        E, parts, dz, X = eng.energy_grad(0, z, pose, mb, _ew(W_ALL), heat, starts)
        res[tag] = (E.cpu().numpy(), parts.cpu().numpy(), dz.cpu().numpy(), X.cpu().numpy())
        eng.close()
    E, parts, dz, X = res["fused"]
    for b in range(B):
        Xo, acts = O.decode(vae, z[b:b + 1], keep=True)
        f, p, dX = O.energy_and_grad(Xo[0], pose[b], mb, O.Weights(*W_ALL), cam, heat[starts[b]:starts[b] + T])
        dzo = O.decode_backward(vae, dX[None], acts)[0]
        np.testing.assert_allclose(X[b], Xo[0], rtol=2e-4, atol=2e-5)
        assert abs(E[b] - f) <= 2e-4 * abs(f) + 1e-7, (b, E[b], f)
        assert np.abs(dz[b] - dzo).max() <= 2e-3 * np.abs(dzo).max() + 1e-8
    np.testing.assert_allclose(E, res["batched"][0], rtol=1e-5)
    np.testing.assert_allclose(parts, res["batched"][1], rtol=1e-5, atol=1e-9)
    assert np.abs(dz - res["batched"][2]).max() <= 1e-4 * np.abs(dz).max()


@pytest.mark.parametrize("T", [9, 12, 16])
def test_fp32_tail_shared_shape_with_other_window_lengths(torch_cuda, monkeypatch, T):
    """The 4-wave shape of the fused fp32 tail carves its LDS buffers for the window's T rows (9 .. 16 rows: one window per
    workgroup) instead of 16: 300 windows of T frames (more workgroups than CUs) against the 8-wave shape -- bitwise poses and
    gradients, energies to 1e-13 -- and against the oracle on the first windows.  T >= 12: the energy inputs are not parked in LDS."""
    torch = torch_cuda
    shape = vae_schema.VAEShape(latent_dim=32, seq_len=T, hidden=(16, 16, 32, 32, 64))
    sd = vae_schema.synthetic_state_dict(shape, 13)
    vae = O.fold_vae(sd, seq_len=T)
    cam = oracle_camera()
    B = 300
    seq = synth.make_sequence(n_frames=120, seed=43)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    rng = np.random.default_rng(7)
    starts = rng.integers(0, 120 - T, B).astype(np.int32)
    pose = np.stack([est[s:s + T] for s in starts])
    mu, _ = O.encode(vae, pose[:8].reshape(8, T, 45))
    z = (np.tile(mu, (B // 8 + 1, 1))[:B] + 0.1 * rng.normal(size=(B, shape.latent_dim))).astype(np.float32)
    mb = O.mean_bone_length(est)
    res = {}
    monkeypatch.setenv("GEM_DEV", "1")
    for tag, waves in (("shared", None), ("one_per_cu", "8")):
        if waves:
            monkeypatch.setenv("GEM_TAIL_WAVES", waves)
        else:
            monkeypatch.delenv("GEM_TAIL_WAVES", raising=False)
        eng = _engine(shape, max_windows=B)
        eng.load_vae(0, sd)
        eng.profile_enable(True)
        E, parts, dz, X = eng.energy_grad(0, z, pose, mb, _ew(W_ALL), heat, starts)
        torch.cuda.synchronize()
        names = eng.profile_kernels(1)
        res[tag] = (E.cpu().numpy(), parts.cpu().numpy(), dz.cpu().numpy(), X.cpu().numpy(), names)
        eng.close()
    a, b = res["shared"], res["one_per_cu"]
    assert ", 4>" in a[4] and ", 8>" in b[4], (a[4], b[4])
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2])
    np.testing.assert_allclose(a[0], b[0], rtol=1e-13)
    for k in range(2):
        Xo, acts = O.decode(vae, z[k:k + 1], keep=True)
        f, p, dX = O.energy_and_grad(Xo[0], pose[k], mb, O.Weights(*W_ALL), cam, heat[starts[k]:starts[k] + T])
        dzo = O.decode_backward(vae, dX[None], acts)[0]
        np.testing.assert_allclose(a[3][k], Xo[0], rtol=2e-4, atol=2e-5)
        assert abs(a[0][k] - f) <= 2e-4 * abs(f) + 1e-7, (k, a[0][k], f)
        assert np.abs(a[2][k] - dzo).max() <= 2e-3 * np.abs(dzo).max() + 1e-8


def test_graph_cache_is_dropped_when_the_weights_are_reloaded(torch_cuda):
    """A captured call bakes the weight pointers into its kernel arguments: gem_load_vae on a loaded stage frees and re-allocates
    them, so it must drop the graph cache (else the next identical call replays kernels on freed / stale weights).  Graphs on,
    capture + replay with weights A, reload weights B, call again with the same signature: the result must be B's eager
    result.  optimize_stage stages its small inputs in engine-owned buffers, so plain numpy inputs replay as well."""
    torch = torch_cuda
    sd_a, sd_b = vae_schema.synthetic_state_dict(TINY, 11), vae_schema.synthetic_state_dict(TINY, 12)
    B = 6
    seq = synth.make_sequence(n_frames=8 * (B - 1) + 10, seed=44)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = torch.as_tensor(np.asarray(seq["heatmap_list"], dtype=np.float32), device="cuda")
    starts = (8 * np.arange(B)).astype(np.int32)
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = O.mean_bone_length(est)
    eps = np.random.default_rng(9).normal(size=(B, TINY.latent_dim)).astype(np.float32)
    w = _ew((1e-2, 1e-2, 1e-1, 1e-3, 1e-2))
    eager = {}
    for tag, sd in (("a", sd_a), ("b", sd_b)):
        e = _engine(TINY, max_windows=8)
        e.load_vae(0, sd)
        out, st = e.optimize_stage(0, pose, mb, eps, w, heat, starts)
        eager[tag] = (out.clone(), st.clone())
        e.close()
    assert not torch.equal(eager["a"][0], eager["b"][0])
    eng = _engine(TINY, max_windows=8)
    eng.load_vae(0, sd_a)
    eng.enable_graphs(True)
    for k in range(3):                       # eager, capture, replay
        out, st = eng.optimize_stage(0, pose, mb, eps, w, heat, starts)
        torch.cuda.synchronize()
        assert torch.equal(out, eager["a"][0]) and torch.equal(st, eager["a"][1]), k
    gs = eng.graph_stats()
    assert gs["captures"] == 1 and gs["replays"] == 2, gs
    eng.load_vae(0, sd_b)                    # same signature from here on, other weights behind (possibly) the same pointers
    for k in range(3):
        out, st = eng.optimize_stage(0, pose, mb, eps, w, heat, starts)
        torch.cuda.synchronize()
        assert torch.equal(out, eager["b"][0]) and torch.equal(st, eager["b"][1]), k
    gs = eng.graph_stats()
    assert gs["captures"] == 2 and gs["replays"] == 4, gs
    eng.set_texel_cache(False)               # part of the signature as well: eager again, same numbers (the cache is bitwise neutral)
    out, st = eng.optimize_stage(0, pose, mb, eps, w, heat, starts)
    torch.cuda.synchronize()
    assert torch.equal(out, eager["b"][0]) and eng.graph_stats()["replays"] == 4
    eng.close()


def test_graph_replay_survives_freed_and_reallocated_inputs(torch_cuda):
    """A captured call holds the ADDRESS of the caller's heat-map tensor.  The caller drops that tensor and allocates another of the
    same size (torch's caching allocator hands back the same address): without the engine's pin (WindowEngine._pin) the old graph
    would be replayed on a buffer it does not own -- on ROCm 7.2 that ended in a GPU memory fault.  With the pin
    the old tensor stays alive, so the new one gets a NEW address, the call is a new signature, and its result is the eager result
    for the new heat maps.  `drop_graphs()` releases the pins; MAX_PINNED + 1 distinct inputs drop every captured call."""
    import weakref
    torch = torch_cuda
    B = 6
    seqs = [synth.make_sequence(n_frames=8 * (B - 1) + 10, seed=70 + i) for i in range(2)]
    est = np.asarray(seqs[0]["estimated_local_skeleton"], dtype=np.float32)
    starts = (8 * np.arange(B)).astype(np.int32)
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = O.mean_bone_length(est)
    eps = np.random.default_rng(9).normal(size=(B, TINY.latent_dim)).astype(np.float32)
    w = _ew((1e-2, 1e-2, 1e-1, 1e-3, 1e-2))
    heats = [np.asarray(s["heatmap_list"], dtype=np.float32) for s in seqs]
    ref = _engine(TINY, max_windows=8)
    ref.load_vae(0, vae_schema.synthetic_state_dict(TINY, 11))
    eager = [ref.optimize_stage(0, pose, mb, eps, w, torch.as_tensor(h, device="cuda"), starts)[0].clone() for h in heats]
    ref.close()
    assert not torch.equal(eager[0], eager[1])
    eng = _engine(TINY, max_windows=8)
    eng.load_vae(0, vae_schema.synthetic_state_dict(TINY, 11))
    eng.enable_graphs(True)
    heat = torch.as_tensor(heats[0], device="cuda")
    addr0, alive = heat.data_ptr(), weakref.ref(heat)
    for k in range(3):                                   # eager, capture, replay
        out = eng.optimize_stage(0, pose, mb, eps, w, heat, starts)[0]
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]), k
    del heat
    assert alive() is not None, "the engine must keep a captured call's inputs alive"
    heat = torch.as_tensor(heats[1], device="cuda")
    assert heat.data_ptr() != addr0
    for k in range(3):
        out = eng.optimize_stage(0, pose, mb, eps, w, heat, starts)[0]
        torch.cuda.synchronize()
        assert torch.equal(out, eager[1]), k
    assert eng.graph_stats()["captures"] == 2
    eng.drop_graphs()
    assert alive() is None and len(eng._pinned) == 0
    out = eng.optimize_stage(0, pose, mb, eps, w, heat, starts)[0]       # eager again after the drop, graphs still enabled
    torch.cuda.synchronize()
    assert torch.equal(out, eager[1])
    keep = [torch.as_tensor(heats[i % 2], device="cuda") for i in range(eng.MAX_PINNED + 1)]
    for i, h in enumerate(keep):
        out = eng.optimize_stage(0, pose, mb, eps, w, h, starts)[0]
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i % 2]), i
    assert len(eng._pinned) <= eng.MAX_PINNED
    eng.close()


@pytest.mark.parametrize("net,B", [("tiny", 3), ("tiny", 21), ("full", 8), ("full", 21), ("full", 40), ("structured", 40)])
def test_bf16_multi_window_tail_against_the_batched_bf16_layers(torch_cuda, monkeypatch, golden, net, B):
    """bf16 decoder mode: the multi-window fused tail (csrc/tail_bf16.hip: 8 windows = five 16-row MFMA tiles per workgroup,
    bf16 weights and activations in registers / LDS, fp32 accumulate and fp32 energies) against the SAME layers as batched bf16
    GEMMs + the stand-alone energy kernel (GEM_BATCHED_NARROW).  Both paths round at the same points (bf16 activations and
    gradients between layers, the same bf16 weights, the same composed front layer), so they agree up to the fp32 summation order
    -- i.e. to ~1e-7, except where that order flips one bf16 rounding (rare; one flip moves one activation by 2^-8 of its value).
    Ragged batches (a last workgroup with 5 of 8 windows, B = 3: one partial workgroup) included; whole stages as well."""
    from globalegomocap_amd.engine import stats_to_numpy
    torch = torch_cuda
    if net == "tiny":
        g = golden("lbfgs_tiny")
        shape, sd = TINY, sd_from_npz(g, "local/")
    elif net == "full":
        shape, sd = FULL, vae_schema.synthetic_state_dict(FULL, 5)
    else:
        shape, sd = FULL, vae_schema.structured_state_dict(FULL, 7, feature_offset=0.0)
    vae = O.fold_vae(sd)
    seq = synth.make_sequence(n_frames=200, seed=36)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = torch.as_tensor(np.asarray(seq["heatmap_list"], dtype=np.float32), device="cuda")
    rng = np.random.default_rng(B)
    starts = rng.integers(0, 190, B).astype(np.int32)
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = O.mean_bone_length(est)
    mu, _ = O.encode(vae, pose.reshape(B, 10, 45))
    z = (mu + 0.1 * rng.normal(size=mu.shape)).astype(np.float32)
    eps = rng.normal(size=(B, shape.latent_dim)).astype(np.float32)
    res = {}
    monkeypatch.setenv("GEM_DEV", "1")
    for tag in ("tail16", "batched"):
        if tag == "tail16":
            monkeypatch.setenv("GEM_TAIL16", "1")
            monkeypatch.delenv("GEM_BATCHED_NARROW", raising=False)
        else:
            monkeypatch.setenv("GEM_TAIL16", "0")
            monkeypatch.setenv("GEM_BATCHED_NARROW", "1")
        eng = _engine(shape, max_windows=B)
        eng.load_vae(0, sd)
        eng.set_precision("bf16")
        E, parts, dz, X = eng.energy_grad(0, z, pose, mb, _ew(W_ALL), heat, starts)
        _, _, dz_s, _ = eng.energy_grad(0, z, pose, mb, _ew(W_ALL[:4] + (0.0,)), heat, starts)      # smooth energy (no texel edges)
        out, stats = eng.optimize_stage(0, pose, mb, eps, _ew((1e-6, 1e-5, 1e-2, 0.0, 1e-2)), heat, starts)
        torch.cuda.synchronize()
        res[tag] = (E.cpu().numpy(), dz.cpu().numpy(), X.cpu().numpy(), dz_s.cpu().numpy(), out.cpu().numpy(), stats_to_numpy(stats))
        eng.close()
    (Ea, dza, Xa, dsa, outa, sta), (Eb, dzb, Xb, dsb, outb, stb) = res["tail16"], res["batched"]
    qx = np.quantile(np.abs(Xa - Xb).ravel() / max(1.0, np.abs(Xb).max()), [0.5, 0.99])
    assert qx[0] <= 1e-6 and qx[1] <= 4e-3, qx                      # (99 %: a flipped rounding of a signal channel is 2^-8 of ~3)
    np.testing.assert_allclose(Ea, Eb, rtol=2e-2)
    for a_, b_ in ((dza, dzb), (dsa, dsb)):
        qg = np.quantile(np.abs(a_ - b_).ravel() / np.abs(b_).max(), [0.5, 0.99])
        assert qg[0] <= 1e-5 and qg[1] <= 2e-2, qg
    cos = [float(np.dot(dsa[k], dsb[k]) / (np.linalg.norm(dsa[k]) * np.linalg.norm(dsb[k]) + 1e-30)) for k in range(B)]
    assert min(cos) > 0.9995, min(cos)
    assert sta["finished"].all() and stb["finished"].all() and not sta["degenerate"].any()
    assert abs(sta["func_evals"].mean() - stb["func_evals"].mean()) <= 3.0
    # fp32 oracle, first windows: decoded pose and energy at bf16 accuracy
    for k in range(min(B, 3)):
        Xo = O.decode(vae, z[k:k + 1])[0]
        assert np.abs(Xa[k] - Xo).max() <= 8e-3 * max(1.0, np.abs(Xo).max()), k


@pytest.mark.parametrize("net", ["full", "structured"])
def test_fp32_tail_shapes_compute_the_same(torch_cuda, monkeypatch, net):
    """The fp32 fused tail (csrc/tail.hip) runs a window as one 8-wave workgroup per CU up to 256 windows and as 4-wave workgroups,
    three per CU (LDS buffers of T instead of 16 rows), beyond (up to ten per CU; then the batched narrow layers + energy kernel take over).  Both shapes walk K in the same
    order for every output element and run the same energy arithmetic per element: decoded poses and latent gradients of 600 windows
    are BITWISE the same, the fp64 energies agree to 1e-13 (their partial sums are combined over 4 instead of 8 wavefronts), and a
    whole stage finishes with the same poses.  Against the batched layers: rounding level; against the fp32 oracle: first windows."""
    from globalegomocap_amd.engine import stats_to_numpy
    torch = torch_cuda
    shape = FULL
    sd = vae_schema.synthetic_state_dict(FULL, 5) if net == "full" else vae_schema.structured_state_dict(FULL, 7, feature_offset=0.0)
    vae = O.fold_vae(sd)
    B = 600
    seq = synth.make_sequence(n_frames=200, seed=37)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = torch.as_tensor(np.asarray(seq["heatmap_list"], dtype=np.float32), device="cuda")
    rng = np.random.default_rng(B)
    starts = rng.integers(0, 190, B).astype(np.int32)
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = O.mean_bone_length(est)
    mu, _ = O.encode(vae, pose[:64].reshape(64, 10, 45))
    z = (np.tile(mu, (B // 64 + 1, 1))[:B] + 0.1 * rng.normal(size=(B, shape.latent_dim))).astype(np.float32)
    eps = rng.normal(size=(B, shape.latent_dim)).astype(np.float32)
    cam = oracle_camera()
    res = {}
    monkeypatch.setenv("GEM_DEV", "1")
    for tag, env in (("shared_cu", {}), ("one_per_cu", {"GEM_TAIL_WAVES": "8"}), ("batched", {"GEM_TAIL_CAP": "0"})):
        for k in ("GEM_TAIL_WAVES", "GEM_TAIL_CAP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = _engine(shape, max_windows=B)
        eng.load_vae(0, sd)
        eng.profile_enable(True)
        E, parts, dz, X = eng.energy_grad(0, z, pose, mb, _ew(W_ALL), heat, starts)
        torch.cuda.synchronize()
        names = eng.profile_kernels(1)                   # family 1 = the fused tail (empty when the batched layers ran)
        eng.profile_enable(False)
        out, stats = eng.optimize_stage(0, pose, mb, eps, _ew((1e-6, 1e-5, 1e-2, 0.0, 1e-2)), heat, starts)
        torch.cuda.synchronize()
        res[tag] = (E.cpu().numpy(), parts.cpu().numpy(), dz.cpu().numpy(), X.cpu().numpy(), out.cpu().numpy(), stats_to_numpy(stats), names)
        eng.close()
    a, b, c = res["shared_cu"], res["one_per_cu"], res["batched"]
    assert "decoder_tail_kernel<5, 4>" in a[6] and "decoder_tail_kernel<5, 8>" in b[6] and "decoder_tail_kernel" not in c[6], (a[6], b[6], c[6])
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2])
    np.testing.assert_allclose(a[0], b[0], rtol=1e-13)
    np.testing.assert_allclose(a[1], b[1], rtol=1e-12, atol=1e-300)
    assert a[5]["finished"].all() and b[5]["finished"].all()
    assert np.array_equal(a[5]["func_evals"], b[5]["func_evals"])
    np.testing.assert_allclose(a[4], b[4], rtol=0, atol=1e-6)
    np.testing.assert_allclose(a[0], c[0], rtol=1e-5)
    np.testing.assert_allclose(a[1], c[1], rtol=1e-5, atol=1e-9)
    # (another summation order in the batched layers: a pre-activation at rounding distance from 0 takes the other LeakyReLU slope
    # in a few of the 600 windows -- the structured weights have many exact-zero features)
    qg = np.quantile(np.abs(a[2] - c[2]).ravel() / np.abs(c[2]).max(), [0.5, 0.999, 1.0])
    assert qg[0] <= 1e-5 and qg[1] <= 1e-3 and qg[2] <= 2e-2, qg
    for k in range(3):
        Xo, acts = O.decode(vae, z[k:k + 1], keep=True)
        f, p, dX = O.energy_and_grad(Xo[0], pose[k], mb, O.Weights(*W_ALL), cam, np.asarray(seq["heatmap_list"], dtype=np.float32)[starts[k]:starts[k] + 10])
        dzo = O.decode_backward(vae, dX[None], acts)[0]
        np.testing.assert_allclose(a[3][k], Xo[0], rtol=2e-4, atol=2e-5)
        assert abs(a[0][k] - f) <= 2e-4 * abs(f) + 1e-7, (k, a[0][k], f)
        assert np.abs(a[2][k] - dzo).max() <= 2e-3 * np.abs(dzo).max() + 1e-8


def test_bf16_tail_row_tile_variants_compute_the_same(torch_cuda, monkeypatch):
    """The bf16 tail is launched with 2 .. 5 row tiles per workgroup (3 .. 8 windows) and one or two workgroups per CU depending on the
    batch (tail_bf16.hip: tail_bf16_row_tiles).  Every variant runs the same products in the same order on a window's rows: energies,
    their parts, decoded poses AND latent gradients of 1100 windows are BITWISE the same whichever variant computes them, and what was
    seen (which windows differ, by how much, on which card) is recorded (see below) (GEM_TAIL16_NRT forces
    one: two tiles = 367 workgroups, two per CU; three = 275; four = 184 and five = 138, one per CU), and the batch's own choice is
    one of them."""
    torch = torch_cuda
    shape, sd = FULL, vae_schema.structured_state_dict(FULL, 7, feature_offset=0.0)
    B = 1100
    seq = synth.make_sequence(n_frames=200, seed=41)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = torch.as_tensor(np.asarray(seq["heatmap_list"], dtype=np.float32), device="cuda")
    rng = np.random.default_rng(B)
    starts = rng.integers(0, 190, B).astype(np.int32)
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = O.mean_bone_length(est)
    z = rng.normal(size=(B, shape.latent_dim)).astype(np.float32) * 0.3
    monkeypatch.setenv("GEM_DEV", "1")
    monkeypatch.setenv("GEM_TAIL16", "1")
    res = {}
    for nrt in (None, 1, 2, 3, 4, 5):
        if nrt is None:
            monkeypatch.delenv("GEM_TAIL16_NRT", raising=False)
        else:
            monkeypatch.setenv("GEM_TAIL16_NRT", str(nrt))
        eng = _engine(shape, max_windows=B)
        eng.load_vae(0, sd)
        eng.set_precision("bf16")
        E, parts, dz, X = eng.energy_grad(0, z, pose, mb, _ew(W_ALL), heat, starts)
        torch.cuda.synchronize()
        res[nrt] = (E.cpu().numpy(), parts.cpu().numpy(), dz.cpu().numpy(), X.cpu().numpy())
        eng.close()
    from helpers import record_observation
    report = {}
    for nrt in (None, 1, 3, 4, 5):
        (Ea, pa, dza, Xa), (Eb, pb, dzb, Xb) = res[nrt], res[2]
        assert np.array_equal(Ea, Eb) and np.array_equal(pa, pb) and np.array_equal(Xa, Xb), nrt
        # dE/dz: round 5 saw ONE of the 1100 windows leave the instantiations with 3 .. 5 row tiles with a single bf16 rounding of its
        # gradient falling the other way.  Round 6 ran it to ground: under hipcc's default -ffp-contract=fast which a*b+c of the energy
        # terms becomes a fused multiply-add depends on what the SLP vectoriser / unroller did to the INSTANTIATION, so the row-tile
        # variants could round differently (a build with SLP on: 3 of 8192 windows, deterministically; -ffp-contract=on / off: none;
        # profiles/contract_ab_r06.txt).  The library is built with -ffp-contract=on now: bitwise by construction, asserted again.
        # The test still RECORDS what it sees and on which card (profiles/observations_r06/).
        same = (dza == dzb).all(axis=1)
        bad = np.flatnonzero(~same)
        report[str(nrt)] = {"windows_differing": int(bad.size), "indices": bad[:16].tolist(),
                            "max_abs_over_largest": float(np.abs(dza - dzb).max() / np.abs(dzb).max())}
    record_observation("bf16_tail_row_tile_variants", {"windows": B, "against_row_tiles": 2, "dz_by_row_tiles": report,
                                                       "bitwise": all(v["windows_differing"] == 0 for v in report.values())})
    for nrt, v in report.items():
        assert v["windows_differing"] == 0, (nrt, v)
    assert np.array_equal(res[None][2], res[2][2]) or np.array_equal(res[None][2], res[3][2])          # the batch's own choice is one of them
    assert np.isfinite(res[2][0]).all() and np.abs(res[2][2]).max() > 0


@pytest.mark.parametrize("T,B", [(12, 13), (16, 7), (5, 19)])
def test_bf16_multi_window_tail_with_other_window_lengths(torch_cuda, monkeypatch, T, B):
    """The bf16 tail packs G = min(8, 80 // T) windows into its 80 rows and uses the run-time-shaped energy code for anything but
    10 x 15: windows of 12 frames (6 per workgroup, 72 rows), 16 (5, 80 rows) and 5 (8, 40 rows) against the batched bf16 layers +
    stand-alone energy kernel, ragged last workgroups included."""
    torch = torch_cuda
    shape = vae_schema.VAEShape(latent_dim=32, seq_len=T, hidden=(16, 16, 32, 32, 64))
    sd = vae_schema.synthetic_state_dict(shape, 17)
    seq = synth.make_sequence(n_frames=200, seed=38)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = torch.as_tensor(np.asarray(seq["heatmap_list"], dtype=np.float32), device="cuda")
    rng = np.random.default_rng(T)
    starts = rng.integers(0, 200 - T, B).astype(np.int32)
    pose = np.stack([est[s:s + T] for s in starts])
    mb = O.mean_bone_length(est)
    z = rng.normal(size=(B, 32)).astype(np.float32)
    res = {}
    monkeypatch.setenv("GEM_DEV", "1")
    for tag in ("tail16", "batched"):
        if tag == "tail16":
            monkeypatch.setenv("GEM_TAIL16", "1")
            monkeypatch.delenv("GEM_BATCHED_NARROW", raising=False)
        else:
            monkeypatch.setenv("GEM_TAIL16", "0")
            monkeypatch.setenv("GEM_BATCHED_NARROW", "1")
        eng = _engine(shape, max_windows=B)
        eng.load_vae(0, sd)
        eng.set_precision("bf16")
        E, parts, dz, X = eng.energy_grad(0, z, pose, mb, _ew(W_ALL), heat, starts)
        torch.cuda.synchronize()
        res[tag] = (E.cpu().numpy(), parts.cpu().numpy(), dz.cpu().numpy(), X.cpu().numpy())
        eng.close()
    (Ea, Pa, dza, Xa), (Eb, Pb, dzb, Xb) = res["tail16"], res["batched"]
    assert np.abs(Xa - Xb).max() <= 1e-5 * max(1.0, np.abs(Xb).max())
    # (the tail's energy code -- energy_pairs.h -- uses 1-ulp reciprocals / square roots and fp32 per-lane partial sums; the
    # reprojection term is a sum of ~T*J samples of either sign that nearly cancel: absolute tolerance on the scale of one sample)
    np.testing.assert_allclose(Ea, Eb, rtol=2e-5)
    np.testing.assert_allclose(Pa, Pb, rtol=2e-5, atol=2e-6)
    assert np.abs(dza - dzb).max() <= 1e-3 * np.abs(dzb).max()


def test_projections_outside_the_heatmap_and_error_paths(torch_cuda):
    """Joints that project outside the 64x64 heat-map sample zeros (grid_sample padding); bad calls raise."""
    from globalegomocap_amd import _capi
    sd = vae_schema.synthetic_state_dict(TINY, 11)
    eng = _engine(TINY, max_windows=4)
    eng.load_vae(0, sd)
    vae = O.fold_vae(sd)
    cam = oracle_camera()
    rng = np.random.default_rng(8)
    # final conv bias shifted sideways: the decoded skeleton leaves the image on the right / bottom for part of the joints
    sd2 = dict(sd)
    b = np.array(sd["final_layer.3.bias"], dtype=np.float32).reshape(15, 3).copy()
    # the fisheye maps the whole front half-space inside the image circle; joints BEHIND the camera plane
    # (z < 0, theta > 0) land beyond it, i.e. outside the 64x64 map on every side
    b[:, 0] = np.linspace(-1.5, 1.5, 15)
    b[:, 1] = np.where(np.arange(15) % 2 == 0, 1.2, -1.2)
    b[:, 2] = np.linspace(-0.8, 0.6, 15)
    sd2["final_layer.3.bias"] = b.reshape(-1)
    eng.load_vae(0, sd2)
    vae2 = O.fold_vae(sd2)
    z = rng.normal(size=(2, 32)).astype(np.float32)
    seq = synth.make_sequence(n_frames=18, seed=2)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = rng.uniform(0, 1, size=(18, 64, 64, 15)).astype(np.float32)      # dense heat-maps: borders matter
    starts = np.array([0, 8], np.int32)
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = O.mean_bone_length(est)
    E, parts, dz, X = eng.energy_grad(0, z, pose, mb, _ew(W_ALL), heat, starts)
    n_out = 0
    for k in range(2):
        Xo, acts = O.decode(vae2, z[k:k + 1], keep=True)
        uv = O.fisheye_project(cam, Xo[0].reshape(-1, 3))
        ix, iy = O.heat_coords(uv, 64, 64)
        n_out += int(((ix < 0) | (ix > 63) | (iy < 0) | (iy > 63)).sum())
        f, p, dX = O.energy_and_grad(Xo[0], pose[k], mb, O.Weights(*W_ALL), cam, heat[starts[k]:starts[k] + 10])
        np.testing.assert_allclose(parts[k].cpu().numpy(), p, rtol=5e-4, atol=1e-5)
        dzo = O.decode_backward(vae2, dX[None], acts)[0]
        assert np.abs(dz[k].cpu().numpy() - dzo).max() <= 5e-3 * np.abs(dzo).max() + 1e-8
    assert n_out > 10                      # the case really exercises out-of-map samples
    # error behaviour: clear messages, no aborts
    with pytest.raises(ValueError):
        eng.decode(0, np.zeros((5, 32), np.float32))                        # more windows than max_windows
    with pytest.raises(_capi.GemError, match="not loaded"):
        eng.decode(1, np.zeros((1, 32), np.float32))                        # stage without weights
    with pytest.raises(_capi.GemError, match="heat-maps"):
        eng.optimize_stage(0, pose, mb, np.zeros((2, 32), np.float32), _ew(W_ALL))   # reproj weight without heat-maps
    with pytest.raises(RuntimeError):
        eng.load_vae(0, {k: v for k, v in sd.items() if k != "fc_mu.bias"})


def test_joint_on_the_optical_axis_raises_like_the_reference(torch_cuda):
    """FishEyeCalibrated.py:124-127 raises Exception('norm is zero!'); the mirror turns the NaN energy into it."""
    import torch
    from globalegomocap_amd.optimizer import BodyPoseOptimizer
    sd = dict(vae_schema.synthetic_state_dict(TINY, 11))
    for k in list(sd):                       # a decoder that outputs exactly its final bias: every joint at (0, 0, 1)
        if k.startswith(("decoder", "final_layer")) and k.endswith(".weight") and np.asarray(sd[k]).ndim == 3:
            sd[k] = np.zeros_like(sd[k])
    sd["final_layer.3.bias"] = np.tile(np.array([0.0, 0.0, 1.0], np.float32), 15)
    pose = synth.rest_skeleton()[None].repeat(10, 0).astype(np.float32)
    bpo = BodyPoseOptimizer(DEFAULT_CALIBRATION, torch.from_numpy(pose), sd, seq_len=10, network_seq_len=10, latent_dim=32)
    bpo.set_weights(vae_weight=0.0, gmm_weight=0.0, smooth_weight=1e-5, bone_length_weight=1e-2, weight_3d=1e-6, reproj_weight=1e-2)
    with pytest.raises(Exception, match="norm is zero"):
        bpo.optimize_pose_seq_pytorch_LBFGS(pose, np.zeros((10, 64, 64, 15), np.float32), pose.copy())


def test_history_ring_wraps_like_torch(torch_cuda, golden):
    """history_size smaller than the iteration count: the (s, y) ring drops its oldest pair (lbfgs.py:  old_dirs.pop(0))."""
    from globalegomocap_amd import _capi
    g = golden("lbfgs_tiny")
    sd = sd_from_npz(g, "local/")
    pose, heat = g["pose"], heat_from_centres(g["heat_centres"])
    eng = _engine(TINY)
    eng.load_vae(0, sd)
    mb = eng.mean_bone_length(pose.astype(np.float32))
    opts = _capi.default_lbfgs_opts()
    opts.history = 4
    out, stats = eng.optimize_stage(0, pose[None], mb, g["local_eps"][None], _ew(W_LOCAL), heat, np.zeros(1, np.int32), opts=opts)
    vae = O.fold_vae(sd)
    ref, st = O.optimize_stage(vae, oracle_camera(), O.Weights(*W_LOCAL), pose, heat, O.mean_bone_length(pose.astype(np.float32)),
                               g["local_eps"], O.LBFGSOptions(history=4))
    s = stats.cpu().numpy()[0]
    assert s[3] == 1 and abs(int(s[1]) - st["func_evals"]) <= 3
    assert np.linalg.norm(out[0].cpu().numpy() - ref, axis=-1).mean() < 0.5e-3
    # and it is a different optimisation from the full-history one
    out_full, _ = eng.optimize_stage(0, pose[None], mb, g["local_eps"][None], _ew(W_LOCAL), heat, np.zeros(1, np.int32))
    assert not np.array_equal(out_full.cpu().numpy(), out.cpu().numpy())


def test_other_window_length_and_camera(torch_cuda):
    """seq_len = 8 (4 windows per tail workgroup) with the 14-coefficient calibration file."""
    from globalegomocap_amd.camera import ALT_CALIBRATION
    from globalegomocap_amd.engine import WindowEngine
    shape = vae_schema.VAEShape(latent_dim=48, seq_len=8, hidden=(16, 32, 32, 64, 64))
    sd = vae_schema.synthetic_state_dict(shape, 17)
    cam_h = FisheyeCamera.from_json(ALT_CALIBRATION)
    eng = WindowEngine(shape, cam_h, max_windows=8)
    eng.load_vae(0, sd)
    vae = O.fold_vae(sd, seq_len=8)
    cam = oracle_camera(ALT_CALIBRATION)
    B = 5
    seq = synth.make_sequence(n_frames=6 * (B - 1) + 8, seed=19, camera=cam_h)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    starts = (6 * np.arange(B)).astype(np.int32)
    pose = np.stack([est[s:s + 8] for s in starts])
    rng = np.random.default_rng(2)
    mu, lv = O.encode(vae, pose.reshape(B, 8, 45))
    mu_d, lv_d, _ = eng.encode(0, pose.reshape(B, 8, 45))
    np.testing.assert_allclose(mu_d.cpu().numpy(), mu, rtol=2e-4, atol=2e-5)
    z = (mu + 0.1 * rng.normal(size=mu.shape)).astype(np.float32)
    mb = O.mean_bone_length(est)
    E, parts, dz, X = eng.energy_grad(0, z, pose, mb, _ew(W_ALL), heat, starts)
    for b in range(B):
        Xo, acts = O.decode(vae, z[b:b + 1], keep=True)
        f, p, dX = O.energy_and_grad(Xo[0], pose[b], mb, O.Weights(*W_ALL), cam, heat[starts[b]:starts[b] + 8])
        dzo = O.decode_backward(vae, dX[None], acts)[0]
        np.testing.assert_allclose(X[b].cpu().numpy(), Xo[0], rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose(parts[b].cpu().numpy(), p, rtol=2e-4, atol=1e-6)
        assert np.abs(dz[b].cpu().numpy() - dzo).max() <= 2e-3 * np.abs(dzo).max() + 1e-8
    eps = rng.normal(size=(B, 48)).astype(np.float32)
    w = (1e-1, 1e-1, 1.0, 1e-3, 1e-2)
    out, stats = eng.optimize_stage(0, pose, mb, eps, _ew(w), heat, starts)
    st = stats.cpu().numpy()
    assert (st[:, 3] == 1).all()
    # random-init weights + strong energy weights: a long chaotic run, so compare what it achieves, not where it ends
    from globalegomocap_amd.engine import stats_to_numpy
    sn = stats_to_numpy(stats)
    tr = eng.read_trace(B)
    for b in (0, B - 1):
        ref, so, losses = oracle_stage_losses(vae, cam, O.Weights(*w), pose[b], heat[starts[b]:starts[b] + 8], mb, eps[b])
        np.testing.assert_allclose(tr[b, :4], losses[:4], rtol=2e-4, atol=1e-7)
        np.testing.assert_allclose(tr[b, :6], losses[:6], rtol=5e-3, atol=1e-6)
        print("seq_len 8 window %d: evals %d / %d, final loss %.6e / %.6e" % (b, sn["func_evals"][b], so["func_evals"], sn["final_loss"][b], so["loss"]))
        assert abs(sn["final_loss"][b] - so["loss"]) <= 0.05 * abs(so["loss"]), (b, sn["final_loss"][b], so["loss"])
        assert abs(int(sn["func_evals"][b]) - so["func_evals"]) <= 6


def test_two_engines_on_two_streams_do_not_interfere(torch_cuda):
    """BASELINE configs[2] regime (several sequences in flight on one GPU): two handles, two HIP streams, calls
    interleaved so that their kernels overlap on the device; each result must be bitwise what the engine produces
    alone (no shared scratch, no hidden global state in the library)."""
    import torch
    from globalegomocap_amd.sequence import window_starts
    shapes = (FULL, TINY)
    Bs = (48, 36)
    engs, args, alone = [], [], []
    for k, (shape, B) in enumerate(zip(shapes, Bs)):
        eng = _engine(shape, max_windows=B)
        eng.load_vae(0, vae_schema.synthetic_state_dict(shape, 20 + k))
        eng.load_vae(1, vae_schema.synthetic_state_dict(shape, 30 + k))
        n_chunks = B // 12
        seq = synth.make_sequence_device(n_chunks * 100, seed=50 + k, device=eng.device)
        starts = np.concatenate([c * 100 + window_starts(100) for c in range(n_chunks)]).astype(np.int32)
        f0 = torch.as_tensor(starts, device=eng.device)
        mb = eng.mean_bone_length(seq["est_local"][:100]).reshape(1, 15).expand(B, 15).contiguous()
        g = torch.Generator().manual_seed(60 + k)
        eps = torch.randn(2, B, shape.latent_dim, generator=g).to(eng.device)
        a = (seq["est_local"], seq["cams"], seq["heat"], f0, mb, eps[0].contiguous(), eps[1].contiguous(),
             _ew((1e-1, 1e-1, 1.0, 1e-3, 1e-2)), _ew((1e-1, 1e-2, 1.0, 0.0, 0.0)))
        engs.append(eng); args.append(a)
        mid, glob, stats = eng.optimize_windows(*a)
        alone.append((mid.clone(), glob.clone(), stats.clone()))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = [[], []]
    for rep in range(3):
        for k in (0, 1):
            with torch.cuda.stream(streams[k]):
                got[k].append(engs[k].optimize_windows(*args[k]))
    torch.cuda.synchronize()
    for k in (0, 1):
        for mid, glob, stats in got[k]:
            assert torch.equal(mid, alone[k][0]) and torch.equal(glob, alone[k][1]) and torch.equal(stats, alone[k][2])


@pytest.mark.parametrize("mode,tol_x,tol_e,tol_g", [("f32", 5e-5, 2e-4, 2e-3), ("bf16x3", 5e-5, 2e-4, 2e-3), ("bf16", 3e-3, 5e-2, 4e-1)])
def test_large_batch_tile_kernels_against_oracle(torch_cuda, mode, tol_x, tol_e, tol_g):
    """BASELINE configs[3] regime (thousands of windows per GPU): the 128x128-tile GEMM kernels that take over at large
    batch (fp32, split-bf16, bf16) on 1664 windows, spot-checked against the oracle on windows spread over the batch
    (first / middle / last row tiles, tile edges) plus bitwise agreement between identical windows.  (The gradients of
    this random-init network are cancellation-dominated, ~1e-4: plain bf16 gets them to a few tens of percent in
    max-norm -- its acceptance criterion is the final MPJPE, tested above -- the other two modes to 2e-3.)"""
    import torch
    sd = vae_schema.synthetic_state_dict(FULL, 5)
    B = 1664                                            # 13 x 40 dec_in tiles of 128x128: above every big-tile threshold
    eng = _engine(FULL, max_windows=B)
    eng.load_vae(0, sd)
    eng.set_precision(mode)
    vae = O.fold_vae(sd)
    cam = oracle_camera()
    seq = synth.make_sequence(n_frames=200, seed=34)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    rng = np.random.default_rng(6)
    starts = rng.integers(0, 190, B).astype(np.int32)
    starts[1] = starts[0]                               # an identical pair inside one tile and one across tiles
    starts[1000] = starts[0]
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = O.mean_bone_length(est)
    eps = rng.normal(size=(B, 2048)).astype(np.float32)
    eps[1] = eps[0]; eps[1000] = eps[0]
    mu_d, lv_d, z_d = eng.encode(0, pose.reshape(B, 10, 45), eps)
    E, parts, dz, X = eng.energy_grad(0, z_d, pose, mb, _ew(W_ALL), heat, starts)
    assert torch.equal(X[0], X[1]) and torch.equal(X[0], X[1000]) and torch.equal(dz[0], dz[1]) and torch.equal(dz[0], dz[1000])
    z = z_d.cpu().numpy()
    for b in (0, 127, 128, 831, 1535, 1663):
        Xo, acts = O.decode(vae, z[b:b + 1], keep=True)
        f, p, dX = O.energy_and_grad(Xo[0], pose[b], mb, O.Weights(*W_ALL), cam, heat[starts[b]:starts[b] + 10])
        dzo = O.decode_backward(vae, dX[None], acts)[0]
        assert np.abs(X[b].cpu().numpy() - Xo[0]).max() <= tol_x * max(1.0, np.abs(Xo[0]).max()), b
        assert abs(float(E[b]) - f) <= tol_e * abs(f) + 1e-7, b
        assert np.abs(dz[b].cpu().numpy() - dzo).max() <= tol_g * np.abs(dzo).max() + 1e-8, b
        _check_parts_at_device_pose(parts[b].cpu().numpy(), X[b].cpu().numpy(), pose[b], mb, heat[starts[b]:starts[b] + 10], cam)


@pytest.mark.parametrize("lr,max_iter,tol_change", [(1.0, 5, 1e-6), (2.0, 1, 1e-6), (0.5, 33, 1e-9), (2.0, 12, 1e-3)])
def test_optimiser_options_against_oracle(torch_cuda, golden, lr, max_iter, tol_change):
    """torch.optim.LBFGS arguments other than the reference's (lr, max_iter and the derived max_eval, tolerance_change):
    every exit of LBFGS.step and of the line search has to fire where the oracle's does."""
    from globalegomocap_amd import _capi
    g = golden("lbfgs_tiny")
    sd = sd_from_npz(g, "local/")
    pose, heat = g["pose"], heat_from_centres(g["heat_centres"])
    eng = _engine(TINY)
    eng.load_vae(0, sd)
    mb = eng.mean_bone_length(pose.astype(np.float32))
    opts = _capi.default_lbfgs_opts(lr, max_iter, tol_change)
    out, stats = eng.optimize_stage(0, pose[None], mb, g["local_eps"][None], _ew(W_LOCAL), heat, np.zeros(1, np.int32), opts=opts)
    ref, st = O.optimize_stage(O.fold_vae(sd), oracle_camera(), O.Weights(*W_LOCAL), pose, heat,
                               O.mean_bone_length(pose.astype(np.float32)), g["local_eps"],
                               O.LBFGSOptions(lr=lr, max_iter=max_iter, max_eval=max_iter * 5 // 4, tol_change=tol_change))
    s = stats.cpu().numpy()[0]
    assert s[3] == 1
    assert abs(int(s[1]) - st["func_evals"]) <= 2 and abs(int(s[0]) - st["n_iter"]) <= 2, (s, st)
    assert int(s[1]) <= max_iter * 5 // 4 + 1
    # (the 41-evaluation run at lr 0.5 crosses heat-map texel edges: single-window pose within the kink tolerance of DESIGN 5.1)
    assert np.linalg.norm(out[0].cpu().numpy() - ref, axis=-1).mean() < (1.5e-3 if max_iter > 25 else 0.5e-3)


def test_zero_weights_stop_at_the_first_evaluation_and_return_the_decoded_start(torch_cuda, golden):
    """All energy weights zero: loss and gradient vanish, LBFGS.step leaves after one evaluation (max|g| <= tol_grad) and the
    stage returns decode(z0), for one window and for a full engine."""
    g = golden("lbfgs_tiny")
    sd = sd_from_npz(g, "local/")
    pose = g["pose"]
    B = 16
    eng = _engine(TINY, max_windows=B)
    eng.load_vae(0, sd)
    mb = eng.mean_bone_length(pose.astype(np.float32))
    rng = np.random.default_rng(2)
    eps = rng.normal(size=(B, 32)).astype(np.float32)
    poses = np.repeat(pose[None], B, axis=0) + rng.normal(0, 0.01, (B, 10, 15, 3))
    out, stats = eng.optimize_stage(0, poses, mb, eps, _ew((0, 0, 0, 0, 0)))
    s = stats.cpu().numpy()
    assert (s[:, 3] == 1).all() and (s[:, 1] == 1).all() and (s[:, 0] == 0).all()
    _, _, z0 = eng.encode(0, poses.reshape(B, 10, 45), eps)
    np.testing.assert_allclose(out.cpu().numpy(), eng.decode(0, z0).cpu().numpy(), rtol=0, atol=2e-6)
    one, s1 = eng.optimize_stage(0, poses[:1], mb, eps[:1], _ew((0, 0, 0, 0, 0)))
    np.testing.assert_allclose(one.cpu().numpy(), out[:1].cpu().numpy(), rtol=0, atol=2e-6)


@pytest.mark.parametrize("mode,B,tol_x,tol_e,tol_g", [("f32", 64, 2e-5, 1e-4, 1e-3), ("f32", 1344, 2e-5, 1e-4, 1e-3), ("bf16", 64, 3e-3, 5e-2, 4e-1)])
def test_composed_front_layer_against_the_two_layers_it_replaces(torch_cuda, monkeypatch, mode, B, tol_x, tol_e, tol_g):
    """decoder_input followed by the first decoder conv (no activation between them: SeqConvVAE.py:62,67-75,131-135) runs as ONE
    composed linear layer (compose_front, weights.hip; weights composed in fp64 at load time).  The same engine with
    GEM_NO_FRONT=1 keeps the two layers: decoded pose, energies and dE/dz of both must agree to rounding (fp32: summation order;
    bf16: one rounding of the composed weights against two bf16 products with a bf16 intermediate), in the tail path (64
    windows) and in the all-batched path (1344 windows), and a whole stage must end at the same energies."""
    import torch
    from globalegomocap_amd.engine import stats_to_numpy
    sd = vae_schema.synthetic_state_dict(FULL, 5)
    seq = synth.make_sequence(n_frames=200, seed=36)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    rng = np.random.default_rng(10)
    starts = rng.integers(0, 190, B).astype(np.int32)
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = O.mean_bone_length(est)
    eps = rng.normal(size=(B, 2048)).astype(np.float32)
    res = {}
    monkeypatch.setenv("GEM_DEV", "1")           # developer switches are honoured only with GEM_DEV=1
    for tag in ("composed", "separate"):
        if tag == "separate":
            monkeypatch.setenv("GEM_NO_FRONT", "1")
        else:
            monkeypatch.delenv("GEM_NO_FRONT", raising=False)
        eng = _engine(FULL, max_windows=B)
        eng.load_vae(0, sd)                      # the layers are composed when the weights are loaded
        eng.set_precision(mode)
        mu_d, lv_d, z_d = eng.encode(0, pose.reshape(B, 10, 45), eps)
        E, parts, dz, X = eng.energy_grad(0, z_d, pose, mb, _ew(W_ALL), heat, starts)
        n_stage = min(B, 64)
        out, stats = eng.optimize_stage(0, pose[:n_stage], mb, eps[:n_stage], _ew((1e-6, 1e-5, 1e-2, 0.0, 1e-2)), heat, starts[:n_stage])
        res[tag] = (E.cpu().numpy(), dz.cpu().numpy(), X.cpu().numpy(), stats_to_numpy(stats))
        eng.close()
    (Ec, dzc, Xc, stc), (Es, dzs, Xs, sts) = res["composed"], res["separate"]
    assert np.abs(Xc - Xs).max() <= tol_x * max(1.0, np.abs(Xs).max())
    np.testing.assert_allclose(Ec, Es, rtol=tol_e)
    # dE/dz per window: a pre-activation that is zero to rounding may take the other LeakyReLU branch in one of the two
    # evaluations (a kink of the network, not an error of either): allow that for 1 % of the windows
    rel = np.abs(dzc - dzs).max(axis=1) / np.abs(dzs).max(axis=1)
    assert np.quantile(rel, 0.99) <= tol_g and rel.max() <= max(0.25, tol_g), (np.sort(rel)[-5:], tol_g)
    assert (stc["status"] == 1).all() and (sts["status"] == 1).all()
    np.testing.assert_allclose(stc["final_loss"], sts["final_loss"], rtol=5e-3 if mode == "f32" else 5e-2)
    if mode == "f32":
        vae = O.fold_vae(sd)
        z = z_d.cpu().numpy()
        for b in (0, B // 2, B - 1):              # and both agree with the oracle
            Xo, acts = O.decode(vae, z[b:b + 1], keep=True)
            f, p_, dX = O.energy_and_grad(Xo[0], pose[b], mb, O.Weights(*W_ALL), oracle_camera(), heat[starts[b]:starts[b] + 10])
            dzo = O.decode_backward(vae, dX[None], acts)[0]
            assert np.abs(Xc[b] - Xo[0]).max() <= 5e-5 * max(1.0, np.abs(Xo[0]).max()), b
            assert abs(float(Ec[b]) - f) <= 2e-4 * abs(f) + 1e-7, b
            assert np.abs(dzc[b] - dzo).max() <= 2e-3 * np.abs(dzo).max() + 1e-8, b


@pytest.mark.parametrize("B", [240, 229, 175, 100])
def test_one_sequence_batches_take_the_row_streaming_gemm(torch_cuda, B):
    """BASELINE configs[1] regime (one sequence: 100..256 windows in a batch): the decoder_input products run in the
    weight-streaming few-rows kernel (csrc/gemm_rows.h: all rows against one 64-column weight tile per workgroup, row tiles of
    16 dealt over 2..4 row blocks, K quarters per wave summed through LDS).  One evaluation spot-checked against the oracle on
    windows at row-tile / row-block edges, bitwise agreement of identical windows that sit in different row blocks -- for one
    evaluation and for a whole stage (row count shrinking on the device as windows finish).  The reference-pinned check of
    this kernel is tests/test_hip_full_size.py::test_full_size_stages_in_a_one_sequence_batch_against_reference_golden."""
    import torch
    from globalegomocap_amd.engine import stats_to_numpy
    sd = vae_schema.synthetic_state_dict(FULL, 5)
    eng = _engine(FULL, max_windows=B)
    eng.load_vae(0, sd)
    vae = O.fold_vae(sd)
    cam = oracle_camera()
    seq = synth.make_sequence(n_frames=200, seed=35)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    rng = np.random.default_rng(8)
    starts = rng.integers(0, 190, B).astype(np.int32)
    starts[B - 1] = starts[0]; starts[B // 2] = starts[0]                  # the same window in three row blocks
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = O.mean_bone_length(est)
    eps = rng.normal(size=(B, 2048)).astype(np.float32)
    eps[B - 1] = eps[0]; eps[B // 2] = eps[0]
    mu_d, lv_d, z_d = eng.encode(0, pose.reshape(B, 10, 45), eps)
    E, parts, dz, X = eng.energy_grad(0, z_d, pose, mb, _ew(W_ALL), heat, starts)
    for b in (B // 2, B - 1):
        assert torch.equal(X[0], X[b]) and torch.equal(dz[0], dz[b]) and torch.equal(z_d[0], z_d[b]), b
    z = z_d.cpu().numpy()
    mu_o, lv_o = O.encode(vae, pose[:1].reshape(1, 10, 45))
    assert np.abs(mu_d[0].cpu().numpy() - mu_o[0]).max() <= 1e-4 * max(1.0, np.abs(mu_o).max())
    for b in sorted({0, 15, 16, 79, 80, B // 2, B - 17, B - 1}):
        Xo, acts = O.decode(vae, z[b:b + 1], keep=True)
        f, p_, dX = O.energy_and_grad(Xo[0], pose[b], mb, O.Weights(*W_ALL), cam, heat[starts[b]:starts[b] + 10])
        dzo = O.decode_backward(vae, dX[None], acts)[0]
        assert np.abs(X[b].cpu().numpy() - Xo[0]).max() <= 5e-5 * max(1.0, np.abs(Xo[0]).max()), b
        assert abs(float(E[b]) - f) <= 2e-4 * abs(f) + 1e-7, b
        assert np.abs(dz[b].cpu().numpy() - dzo).max() <= 2e-3 * np.abs(dzo).max() + 1e-8, b
    # a whole stage: the rows in use shrink on the device while it runs
    w = _ew((1e-1, 1e-1, 1.0, 1e-3, 1e-2))
    out, stats = eng.optimize_stage(0, pose, mb, eps, w, heat, starts)
    st = stats_to_numpy(stats)
    assert (st["status"] == 1).all() and st["func_evals"].mean() > 20
    for b in (B // 2, B - 1):
        assert torch.equal(out[0], out[b]) and torch.equal(stats[0], stats[b]), b
    assert np.isfinite(out.cpu().numpy()).all()


def test_fused_compaction_is_bitwise_the_compact_kernel(torch_cuda, tmp_path):
    """In the one-sequence fp32 rounds the first launch of a round (gemm_rows.h, FUSE) re-packs the windows that are still
    iterating itself; GEM_NO_FUSED_COMPACT=1 (read once per process) keeps compact_kernel.  Both are stable partitions, so whole
    stages -- local and global, 64 / 240 / 300 windows -- must come out bit for bit the same (tools/check_fused_compaction.py,
    one child process per setting)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for tag, extra in (("fused", {}), ("kernel", {"GEM_NO_FUSED_COMPACT": "1", "GEM_DEV": "1"})):
        env = dict(os.environ, **extra)
        env.pop("GEM_NO_FUSED_COMPACT", None) if not extra else None
        path = str(tmp_path / ("%s.npz" % tag))
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_fused_compaction.py"), path], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(path))
    a, b = outs
    assert set(a.files) == set(b.files) and len(a.files) == 12
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
    assert (a["stats_240_0"][:, 3] == 1).all() and a["stats_240_0"][:, 1].mean() > 25


@pytest.mark.parametrize("B", [400, 1280, 1536, 2560, 4096])
def test_batches_between_the_regimes_agree_with_a_small_batch(torch_cuda, B):
    """400..2560 windows in fp32: too many rows for the few-rows GEMM, still few enough workgroups for the fused tail (its 4-wave
    shape, three workgroups per CU) -- the composed front layer runs in the tiled kernels, its slabs go to the tail, compact_kernel
    re-packs the windows; 4096 windows: the batched narrow layers + the stand-alone energy kernel.  The first 40 windows must come
    out as they do in a 40-window batch (the 8-wave tail): same evaluation counts, energies to 1e-5, poses to 0.01 mm."""
    from globalegomocap_amd.engine import stats_to_numpy
    sd = vae_schema.synthetic_state_dict(FULL, 5)
    seq = synth.make_sequence(n_frames=200, seed=36)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    rng = np.random.default_rng(10)
    starts = rng.integers(0, 190, B).astype(np.int32)
    pose = np.stack([est[s:s + 10] for s in starts])
    eps = rng.normal(size=(B, 2048)).astype(np.float32)
    big, small = _engine(FULL, max_windows=B), _engine(FULL, max_windows=40)
    big.load_vae(0, sd)
    small.load_vae(0, sd)
    mb = big.mean_bone_length(est)
    _, _, z = big.encode(0, pose.reshape(B, 10, 45), eps)
    E, _, dz, X = big.energy_grad(0, z, pose, mb, _ew(W_ALL), heat, starts)
    Es, _, dzs, Xs = small.energy_grad(0, z[:40], pose[:40], mb, _ew(W_ALL), heat, starts[:40])
    np.testing.assert_allclose(X[:40].cpu().numpy(), Xs.cpu().numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(E[:40].cpu().numpy(), Es.cpu().numpy(), rtol=1e-6)
    assert np.abs((dz[:40] - dzs).cpu().numpy()).max() <= 1e-4 * np.abs(dzs.cpu().numpy()).max()
    w = _ew((1e-6, 1e-5, 1e-2, 0.0, 1e-2))
    out, stats = big.optimize_stage(0, pose, mb, eps, w, heat, starts)
    outs, stats_s = small.optimize_stage(0, pose[:40], mb, eps[:40], w, heat, starts[:40])
    st, ss = stats_to_numpy(stats), stats_to_numpy(stats_s)
    assert (st["status"] == 1).all()
    assert (st["func_evals"][:40] == ss["func_evals"]).sum() >= 38
    np.testing.assert_allclose(st["final_loss"][:40], ss["final_loss"], rtol=1e-5)
    assert np.linalg.norm((out[:40] - outs).cpu().numpy(), axis=-1).mean() < 0.01e-3
    big.close()
    small.close()


def test_mid_size_batch_runs_the_fused_tail_in_several_waves(torch_cuda):
    """300..1280 windows: more tail workgroups than CUs.  One evaluation against the same windows in a small batch, and a
    whole stage whose duplicated windows (first 40 = last 40, i.e. different workgroup waves) must agree bitwise."""
    import torch
    from globalegomocap_amd.engine import stats_to_numpy
    sd = vae_schema.synthetic_state_dict(FULL, 5)
    B, n_dup = 300, 40
    eng = _engine(FULL, max_windows=B)
    eng.load_vae(0, sd)
    seq = synth.make_sequence_device(400, seed=78, device=eng.device)
    rng = np.random.default_rng(11)
    starts = rng.integers(0, 390, B).astype(np.int32)
    starts[B - n_dup:] = starts[:n_dup]
    est = seq["est_local_np"].astype(np.float32)
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = eng.mean_bone_length(est[:100])
    eps = rng.normal(size=(B, 2048)).astype(np.float32)
    eps[B - n_dup:] = eps[:n_dup]
    w = _ew((1e-1, 1e-1, 1.0, 1e-3, 1e-2))
    _, _, z0 = eng.encode(0, pose.reshape(B, 10, 45), eps)
    E, parts, dz, X = eng.energy_grad(0, z0, pose, mb, w, seq["heat"], starts)
    small = _engine(FULL, max_windows=64)
    small.load_vae(0, sd)
    Es, _, dzs, Xs = small.energy_grad(0, z0[:64], pose[:64], mb, w, seq["heat"], starts[:64])
    np.testing.assert_allclose(X[:64].cpu().numpy(), Xs.cpu().numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(E[:64].cpu().numpy(), Es.cpu().numpy(), rtol=2e-5)
    assert np.abs((dz[:64] - dzs).cpu().numpy()).max() <= 2e-3 * np.abs(dzs.cpu().numpy()).max()
    assert torch.equal(X[:n_dup], X[B - n_dup:]) and torch.equal(dz[:n_dup], dz[B - n_dup:])
    out, stats = eng.optimize_stage(0, pose, mb, eps, w, seq["heat"], starts)
    st = stats_to_numpy(stats)
    assert (st["status"] == 1).all() and st["func_evals"].mean() > 20
    assert torch.equal(out[:n_dup], out[B - n_dup:]) and torch.equal(stats[:n_dup], stats[B - n_dup:])
    assert (st["final_loss"] <= E.cpu().numpy().astype(np.float32) * (1 + 1e-6) + 1e-6).all()
    assert np.isfinite(out.cpu().numpy()).all()


def test_stage_sweep_against_oracle(torch_cuda, golden):
    """Randomised sweep of whole stages against the CPU oracle: different windows of a sequence, noise, energy weights
    (local with reprojection / global without) and history sizes, fitted tiny VAEs.

    Energies and evaluation counts have to agree for every stage.  Final poses: a stage whose trajectory crosses a kink of the
    energy on the other side than the oracle's (a heat-map texel edge in the local stage, a LeakyReLU kink of the fitted
    decoder in the long, flat global stages) ends up to 1-2 mm away at the same energy, so every stage must be
    within 2 mm and most of them within 0.05 mm."""
    from globalegomocap_amd import _capi
    g = golden("lbfgs_tiny")
    diffs = {True: [], False: []}
    for seed in range(8):
        rng = np.random.default_rng(1000 + seed)
        local = bool(seed % 2 == 0)
        sd = sd_from_npz(g, "local/" if local else "global/")
        seq = synth.make_sequence(n_frames=60, seed=200 + seed)
        est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
        heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
        f0 = int(rng.integers(0, 50))
        pose = est[f0:f0 + 10] if local else (est[f0:f0 + 10] + np.array([0.004, 0, 0], np.float32) * np.arange(10, dtype=np.float32)[:, None, None])
        w = (1e-6, 1e-5, 1e-2, 0.0, 1e-2) if local else (1e-2, 1e-3, 1e-2, 0.0, 0.0)
        w = tuple(float(x * rng.uniform(0.5, 2.0)) for x in w)
        eps = rng.normal(size=32).astype(np.float32)
        hist = int(rng.choice([100, 100, 6, 3]))
        eng = _engine(TINY)
        eng.load_vae(0, sd)
        mb = eng.mean_bone_length(est)
        opts = _capi.default_lbfgs_opts()
        opts.history = hist
        out, stats = eng.optimize_stage(0, pose[None], mb, eps[None], _ew(w), heat, np.array([f0], np.int32), opts=opts)
        ref, st = O.optimize_stage(O.fold_vae(sd), oracle_camera(), O.Weights(*w), pose, heat[f0:f0 + 10], O.mean_bone_length(est), eps,
                                   O.LBFGSOptions(history=hist))
        s = stats.cpu().numpy()[0]
        loss = float(np.array([s[2]], dtype=np.int32).view(np.float32)[0])
        diff = float(np.linalg.norm(out[0].cpu().numpy() - ref, axis=-1).mean())
        print("seed %d %s hist %d: evals %d / %d, loss %.6e / %.6e, mean joint diff %.3f mm" %
              (seed, "local" if local else "global", hist, int(s[1]), st["func_evals"], loss, st["loss"], diff * 1e3))
        assert s[3] == 1
        assert abs(int(s[1]) - st["func_evals"]) <= 3, (s, st["func_evals"], st["n_iter"])
        assert abs(loss - st["loss"]) <= 2e-3 * abs(st["loss"]) + 1e-7
        assert diff < 2e-3, (seed, diff)
        diffs[local].append(diff)
        eng.close()
    # measured (gpurun_out/r02_pytest*.log): local stages 0.000-0.001 mm unless a texel edge is crossed differently (then
    # ~1.3 mm); global stages of the fitted tiny VAEs 0.0-1.5 mm, one or two evaluations apart
    assert np.median(diffs[True]) < 0.05e-3, diffs[True]
    assert np.median(diffs[False]) < 1.5e-3, diffs[False]


def test_texel_block_cache_does_not_change_a_bit(torch_cuda, golden):
    """The reprojection term re-reads the four texels under a joint from a per-window record while the joint stays in the same
    texel block: a whole local stage (tiny and full-size VAE) with the cache on and off must agree bitwise."""
    import torch
    from globalegomocap_amd.sequence import window_starts
    g = golden("lbfgs_tiny")
    for shape, sd, B in ((TINY, sd_from_npz(g, "local/"), 12), (FULL, vae_schema.structured_state_dict(FULL, 7), 24)):
        eng = _engine(shape, max_windows=B)
        eng.load_vae(0, sd)
        seq = synth.make_sequence(n_frames=8 * (B - 1) + 10, seed=91, cam_jitter=(0.3, 0.002))
        est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
        heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
        starts = (8 * np.arange(B)).astype(np.int32)
        pose = np.stack([est[s:s + 10] for s in starts])
        mb = eng.mean_bone_length(est)
        eps = np.random.default_rng(3).normal(size=(B, shape.latent_dim)).astype(np.float32)
        res = []
        for on in (True, False, True):
            eng.set_texel_cache(on)
            out, stats = eng.optimize_stage(0, pose, mb, eps, _ew(W_LOCAL), heat, starts)
            res.append((out.clone(), stats.clone(), eng.read_trace(B)))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2], equal_nan=True)
        assert torch.equal(res[0][0], res[2][0])
        assert res[0][1].cpu().numpy()[:, 1].mean() > 20         # the stages really iterate
        eng.close()


def test_empty_batches_are_no_ops(torch_cuda):
    """B = 0 (a rank whose shard is empty, a chunk shorter than one window): every entry point returns empty outputs, launches
    nothing that could fault, and leaves the engine usable."""
    import torch
    from globalegomocap_amd.engine import WindowEngine, energy_weights
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    eng = WindowEngine(TINY, max_windows=16)
    sd = vae_schema.synthetic_state_dict(TINY, 1)
    eng.load_vae(0, sd)
    eng.load_vae(1, sd)
    seq = synth.make_sequence_device(30, seed=1, device=eng.device, camera=FisheyeCamera.from_json(DEFAULT_CALIBRATION))
    f0 = torch.zeros(0, dtype=torch.int32, device=eng.device)
    none = torch.zeros(0, TINY.latent_dim, device=eng.device)
    wl, wg = energy_weights(1e-6, 1e-5, 1e-2, 0, 1e-2), energy_weights(1e-2, 1e-3, 1e-2, 0, 0)
    mid, glob, stats = eng.optimize_windows(seq["est_local"], seq["cams"], seq["heat"], f0, torch.zeros(0, 15, device=eng.device), none, none, wl, wg)
    assert tuple(mid.shape) == (0, 10, 15, 3) and tuple(glob.shape) == (0, 10, 15, 3) and stats.shape[0] == 0
    assert tuple(eng.decode(0, none).shape) == (0, 10, 15, 3)
    assert tuple(eng.encode(0, torch.zeros(0, 10, 45, device=eng.device))[0].shape) == (0, TINY.latent_dim)
    # ... and a real call afterwards still works
    f1 = torch.as_tensor([0, 8], dtype=torch.int32, device=eng.device)
    mb = eng.mean_bone_length(seq["est_local"]).reshape(1, 15).expand(2, 15).contiguous()
    e2 = torch.randn(2, TINY.latent_dim, device=eng.device)
    _, g2, st = eng.optimize_windows(seq["est_local"], seq["cams"], seq["heat"], f1, mb, e2, e2, wl, wg)
    torch.cuda.synchronize()
    assert torch.isfinite(g2).all()
    eng.close()


def test_no_call_leaves_state_behind_for_the_next(torch_cuda):
    """One engine, the TINY network, B = 5: energy_grad returns the same bits (E, parts, dz, X) before anything else, after an
    optimize_stage in f32, after an optimize_stage in bf16, and after a gem_lbfgs_debug_begin + one advance that is then abandoned.
    What a call runs is decided by that call alone (its route and its rounds' sets are values handed down, stage.hip), so the
    evaluation must not be able to tell what ran on the handle before it."""
    import torch
    B = 5
    sd = vae_schema.synthetic_state_dict(TINY, 11)
    eng = _engine(TINY, max_windows=8)
    eng.load_vae(0, sd)
    seq = synth.make_sequence(n_frames=8 * (B - 1) + 10, seed=21)
    est = np.asarray(seq["estimated_local_skeleton"], dtype=np.float32)
    heat = np.asarray(seq["heatmap_list"], dtype=np.float32)
    starts = (8 * np.arange(B)).astype(np.int32)
    pose = np.stack([est[s:s + 10] for s in starts])
    mb = eng.mean_bone_length(est)
    rng = np.random.default_rng(5)
    z = rng.normal(size=(B, TINY.latent_dim)).astype(np.float32)
    eps = rng.normal(size=(B, TINY.latent_dim)).astype(np.float32)

    def evaluation():
        out = eng.energy_grad(0, z, pose, mb, _ew(W_ALL), heat, starts)
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in out]

    def same(after, what):
        for name, a, b in zip(("E", "parts", "dz", "X"), first, after):
            assert np.isfinite(a).all() and a.tobytes() == b.tobytes(), (what, name, float(np.abs(a - b).max()))

    first = evaluation()
    assert np.abs(first[2]).max() > 0
    eng.optimize_stage(0, pose, mb, eps, _ew(W_ALL), heat, starts)
    same(evaluation(), "after an f32 stage")
    eng.set_precision("bf16")
    eng.optimize_stage(0, pose, mb, eps, _ew(W_ALL), heat, starts)
    eng.set_precision("f32")
    same(evaluation(), "after a bf16 stage")
    for slots in (2, 1):          # slots handed out by lbfgs_advance (two alternating sets), then compact_kernel between the rounds
        eng.lbfgs_debug_begin(z, slots)
        eng.lbfgs_debug_advance(first[0], first[2], None, 0)
        same(evaluation(), "after an abandoned run of the solver alone (slots = %d)" % slots)
    eng.close()
