"""The case table of the training-step shape sweep and the allowances measured on the CPU -- shared by
tests/test_train_f64_cpu.py (which measures them) and tests/test_train_shapes_gpu.py (which uses four times them)."""
from collections import namedtuple

import numpy as np

from globalegomocap_amd import synth, vae as vae_schema

Case = namedtuple("Case", "name T hidden D B form")
S = (24, 40, 96)

# B of the two "direct" rows is written for 256 compute units; the GPU test derives it from the card (direct_batches)
CASES = [
    Case("t3-b2", 3, S, 72, 2, "mean"),
    Case("t5-h64-d5-b33", 5, (64,), 5, 33, "sum"),
    Case("t8-7x8-d33-b64", 8, (8,) * 7, 33, 64, "sum"),
    Case("t8-b128", 8, S, 72, 128, "mean"),
    Case("t8-b129", 8, S, 72, 129, "mean"),
    Case("t16-b64", 16, S, 72, 64, "mean"),
    Case("t16-b65", 16, S, 72, 65, "sum"),
    Case("t12-b213", 12, S, 72, 213, "mean"),
    Case("t12-b214", 12, S, 72, 214, "mean"),
    Case("t16-b160", 16, S, 72, 160, "mean"),
    Case("t10-b257", 10, S, 72, 257, "mean"),
    Case("t16-direct", 16, (64, 512), 130, 256, "mean"),
    Case("t16-direct-ragged", 16, (64, 512), 130, 200, "mean"),
    Case("t6-full-b9", 6, (64, 64, 128, 256, 512), 64, 9, "mean"),
    Case("t6-full-b90", 6, (64, 64, 128, 256, 512), 64, 90, "sum"),
]
LR, WEIGHT_DECAY, KLD_WEIGHT = 1e-3, 1e-4, 0.02

# fp32 CPU port (oracle.torch_port.TrainPort) against the float64 restatement that adopts the port's LeakyReLU signs, worst over
# CASES (tests/test_train_f64_cpu.py::test_allowances measures them and asserts that they hold):
#   gradients |d| <= A max|ref_k| + B gmax, ".0.bias" tensors (exact zero gradient) |d| <= B0 gmax, LeakyReLU inputs
#   |d| <= C max(1, max|ref|), losses relative LOSS, running statistics |d| <= STAT max(1, max|ref|)
PORT_A, PORT_B, PORT_B0, PORT_C, PORT_LOSS, PORT_STAT = 2e-5, 2e-7, 1.5e-6, 1e-5, 2.5e-7, 1e-7


def shape_of(case):
    return vae_schema.VAEShape(latent_dim=case.D, seq_len=case.T, hidden=tuple(case.hidden))


def direct_batches(n_cu):
    """(first batch whose fc backward-data product runs without slabs, a ragged batch on the same route) for the (64, 512) network
    at T = 16: linear_bwd_data takes one slab when (pad64(B) / 64) * (K / 64) >= 2 n_cu, K = 16 * 512."""
    tiles_k = 16 * 512 // 64
    b = 64 * max(1, -(-2 * n_cu // tiles_k))
    return b, b - 56


def inputs(case, steps=2, batch=None):
    """(shape, initial state dict, poses [steps,B,T,45], eps [steps,B,D]): unmodified synth.make_training_windows / initial_state_dict."""
    from globalegomocap_amd.vae_train import initial_state_dict
    B = batch or case.B
    shape = shape_of(case)
    seed = 100 + CASES.index(case)
    init = initial_state_dict(shape, seed)
    poses = synth.make_training_windows(steps * B, case.T, seed + 1).reshape(steps, B, case.T, 45)
    eps = np.random.default_rng(seed + 2).standard_normal((steps, B, case.D)).astype(np.float32)
    return shape, init, poses, eps
