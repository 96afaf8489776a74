"""The fp32 fused tail (csrc/tail.hip) is compiled per bound on the tiles a wave owns (TailArgs::maxnt) and requests its weight
fragments ahead of the layer that uses them.  Neither changes a single MFMA of any output element: the 8-wave shape against the
4-wave shape (bitwise poses and dE/dz, energies to 1e-13), both against the batched layers (GEM_NO_TAIL) at the tolerances of
test_hip_parity.test_unfused_layer_path, through energy_grad (finished input matrix) and through a stage (split-K slab input, rounds).
Widths: the shipped tail 256->128->64->64->64->45 (12, 6 and 3 K blocks per layer, one and two tiles per wave), several windows per
workgroup (T = 8, 5), and a tail with a 512-column adjoint, which needs the 4-tile instantiation."""
import numpy as np
import pytest

from globalegomocap_amd import synth, vae as vae_schema
from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

W_ALL = (7e-3, 2e-2, 5e-2, 3e-3, 4e-2)
W_STAGE = (1e-1, 1e-1, 1.0, 1e-3, 1e-2)
DEFAULT_WIDTHS = (64, 64, 128, 256, 512)
SWITCHES = ("GEM_TAIL_WAVES", "GEM_NO_TAIL")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch


@pytest.fixture(scope="module")
def sequence():
    seq = synth.make_sequence(n_frames=80, seed=47)
    return np.asarray(seq["estimated_local_skeleton"], dtype=np.float32), np.asarray(seq["heatmap_list"], dtype=np.float32)


def _run(torch, monkeypatch, shape, sd, inputs, env):
    """energy_grad + one stage with the developer switches of `env`; the fused tail's kernel names of the energy_grad call."""
    from globalegomocap_amd.engine import WindowEngine, energy_weights, stats_to_numpy
    z, pose, mb, eps, heat, starts = inputs
    monkeypatch.setenv("GEM_DEV", "1")               # developer switches are honoured only with GEM_DEV=1
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = WindowEngine(shape, FisheyeCamera.from_json(DEFAULT_CALIBRATION), max_windows=8)
    eng.load_vae(0, sd)                              # the path is chosen when the weights are loaded
    eng.profile_enable(True)
    E, parts, dz, X = eng.energy_grad(0, z, pose, mb, energy_weights(*W_ALL), heat, starts)
    torch.cuda.synchronize()
    names = eng.profile_kernels(1)                   # family 1 = the fused tail (empty when the batched layers ran)
    eng.profile_enable(False)
    out, stats = eng.optimize_stage(0, pose, mb, eps, energy_weights(*W_STAGE), heat, starts)
    torch.cuda.synchronize()
    res = dict(E=E.cpu().numpy(), dz=dz.cpu().numpy(), X=X.cpu().numpy(), out=out.cpu().numpy(), stats=stats_to_numpy(stats), names=names)
    eng.close()
    return res


def _inputs(shape, sequence, B, seed):
    est, heat = sequence
    T = shape.seq_len
    rng = np.random.default_rng(seed)
    starts = (8 * np.arange(B)).astype(np.int32)
    pose = np.stack([est[s:s + T] for s in starts])
    z = (0.3 * rng.normal(size=(B, shape.latent_dim))).astype(np.float32)
    eps = rng.normal(size=(B, shape.latent_dim)).astype(np.float32)
    return z, pose, O.mean_bone_length(est), eps, heat, starts


def _same_up_to_summation_order(fused, batched):
    """test_unfused_layer_path's comparison of the fused tail with the batched layers"""
    assert "decoder_tail_kernel" in fused["names"] and "decoder_tail_kernel" not in batched["names"], (fused["names"], batched["names"])
    np.testing.assert_allclose(fused["E"], batched["E"], rtol=1e-5)
    assert np.abs(fused["dz"] - batched["dz"]).max() <= 1e-4 * np.abs(batched["dz"]).max()
    assert fused["stats"]["finished"].all() and batched["stats"]["finished"].all()


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T", [10, 16])
def test_default_widths_both_shapes_and_batched_layers(torch_cuda, monkeypatch, sequence, T, B):
    """The shipped tail.  T = 10: the 4-wave shape exists (three LDS carves fit a CU); T = 16: GEM_TAIL_WAVES=4 leaves the 8-wave
    shape (the carves do not fit), and the comparison of the two runs holds all the same."""
    shape = vae_schema.VAEShape(latent_dim=64, seq_len=T, hidden=DEFAULT_WIDTHS)
    sd = vae_schema.synthetic_state_dict(shape, 5)
    inputs = _inputs(shape, sequence, B, 100 + T + B)
    w8 = _run(torch_cuda, monkeypatch, shape, sd, inputs, {"GEM_TAIL_WAVES": "8"})
    w4 = _run(torch_cuda, monkeypatch, shape, sd, inputs, {"GEM_TAIL_WAVES": "4"})
    batched = _run(torch_cuda, monkeypatch, shape, sd, inputs, {"GEM_NO_TAIL": "1"})
    assert "TailTiles<2>::decoder_tail_kernel<5, 8>" in w8["names"], w8["names"]
    if T == 10:
        assert "TailTiles<2>::decoder_tail_kernel<5, 4>" in w4["names"], w4["names"]
    assert np.array_equal(w8["X"], w4["X"]) and np.array_equal(w8["dz"], w4["dz"])
    np.testing.assert_allclose(w8["E"], w4["E"], rtol=1e-13)
    assert np.array_equal(w8["stats"]["func_evals"], w4["stats"]["func_evals"])
    np.testing.assert_allclose(w8["out"], w4["out"], rtol=0, atol=1e-6)
    _same_up_to_summation_order(w8, batched)
    _same_up_to_summation_order(w4, batched)


@pytest.mark.parametrize("T", [8, 5])
def test_several_windows_per_workgroup(torch_cuda, monkeypatch, sequence, T):
    """Two (T = 8) and three (T = 5) windows per workgroup: the one-wave-per-window energy path; B = 7 leaves the last workgroup
    partly filled."""
    shape = vae_schema.VAEShape(latent_dim=64, seq_len=T, hidden=DEFAULT_WIDTHS)
    sd = vae_schema.synthetic_state_dict(shape, 5)
    inputs = _inputs(shape, sequence, 7, 200 + T)
    fused = _run(torch_cuda, monkeypatch, shape, sd, inputs, {})
    batched = _run(torch_cuda, monkeypatch, shape, sd, inputs, {"GEM_NO_TAIL": "1"})
    assert "TailTiles<2>::decoder_tail_kernel<5, 8>" in fused["names"], fused["names"]
    _same_up_to_summation_order(fused, batched)


def test_four_tile_route(torch_cuda, monkeypatch, sequence):
    """A tail whose adjoint of 512 -> 128 is 512 columns wide runs the instantiation compiled for four tiles per wave; the default
    widths run the one compiled for two."""
    shape = vae_schema.VAEShape(latent_dim=64, seq_len=10, hidden=(64, 128, 512, 512))
    sd = vae_schema.synthetic_state_dict(shape, 5)
    inputs = _inputs(shape, sequence, 3, 300)
    fused = _run(torch_cuda, monkeypatch, shape, sd, inputs, {})
    batched = _run(torch_cuda, monkeypatch, shape, sd, inputs, {"GEM_NO_TAIL": "1"})
    assert "TailTiles<4>::decoder_tail_kernel" in fused["names"] and "TailTiles<2>" not in fused["names"], fused["names"]
    _same_up_to_summation_order(fused, batched)
    default = vae_schema.VAEShape(latent_dim=64, seq_len=10, hidden=DEFAULT_WIDTHS)
    ran = _run(torch_cuda, monkeypatch, default, vae_schema.synthetic_state_dict(default, 5), _inputs(default, sequence, 3, 301), {})
    assert "TailTiles<2>::decoder_tail_kernel" in ran["names"] and "TailTiles<4>" not in ran["names"], ran["names"]
