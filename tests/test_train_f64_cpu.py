"""tests/train_f64.py (the training step in float64) pinned from four sides, without a GPU, and the allowances of
tests/test_train_shapes_gpu.py measured.

  * without masks it is the CPU port (oracle.torch_port.TrainPort, itself pinned to the reference's own run) on train_tiny.npz' cases;
  * its gradients are its own central differences (T in {3, 7, 16}, one and seven blocks, both loss forms);
  * its Adam is torch.optim.Adam in float64 over two steps;
  * allowances: the fp32 port against the restatement that adopts the port's LeakyReLU signs, over train_cases.CASES.

Measured here (torch CPU, one thread), worst over the 15 cases (test_allowances prints the table per case with `-s`):
  gradients          a = 1.81e-5 (x max|ref_k|)  +  b = a / 100 = 1.81e-7 (x gmax): the 7-block, 8-channel network; every other
                     case <= 8.5e-6                                            [the condition: a <= 5e-5, b <= 5e-7]
  ".0.bias" tensors  b0 = 1.13e-6 (x gmax)
  LeakyReLU inputs   c = 8.2e-6 (x max(1, max|ref|))
  losses             2.1e-7 relative
  running statistics 8.1e-8 (x max(1, max|ref|))
  LeakyReLU sign flips of the port against float64 WITHOUT adoption: one, in one case (t16-direct, 2.9e6 activations); left in,
  that case's gradients deviate by 1.3e-2 of a tensor's maximum instead of 4.4e-6 (the reason for the adoption).
train_cases.PORT_* hold these rounded up; the GPU test allows four times them."""
import numpy as np
import pytest
import torch

import train_f64 as F64
from train_cases import CASES, KLD_WEIGHT, PORT_A, PORT_B, PORT_B0, PORT_C, PORT_LOSS, PORT_STAT, inputs
from globalegomocap_amd import synth, vae as vae_schema
from globalegomocap_amd.vae_train import initial_state_dict
from helpers import train_golden_case


def port_step(init, seq_len, poses, eps, w, form):
    """One gradient-only step of the fp32 port with the input of every LeakyReLU recorded: (losses, grads, {block: pre [B,T,c]},
    running statistics)."""
    from oracle.torch_port import TrainPort
    port = TrainPort(init, seq_len=seq_len)
    pre = {}
    blocks = [("encoder.%d" % i, b) for i, b in enumerate(port.net.encoder)] + [("decoder.%d" % i, b) for i, b in enumerate(port.net.decoder)]
    hooks = [b[2].register_forward_hook(lambda m, a, o, k=k: pre.__setitem__(k, a[0].detach().permute(0, 2, 1).numpy().copy())) for k, b in blocks]
    hooks.append(port.net.final_layer[2].register_forward_hook(
        lambda m, a, o: pre.__setitem__("final_layer", a[0].detach().permute(0, 2, 1).numpy().copy())))
    losses = port.step(poses, eps, w, form="M_N" if form == "mean" else "kl_weight", update=False)
    for h in hooks:
        h.remove()
    sd = port.state_dict()
    return losses, port.gradients(), pre, {k: v for k, v in sd.items() if "running" in k}


@pytest.mark.parametrize("case", ["mn", "sum"])
def test_restatement_is_the_port_on_the_reference_cases(golden, case):
    """No masks: the same function as the port, which tests/test_oracle_golden.py pins to the unmodified reference's own steps.
    Losses to 1e-5; gradients at the allowance the device step has had against the port (2e-4 max|ref_k| + 5e-7 gmax: it covers a
    LeakyReLU sign flip of the fp32 side), LeakyReLU inputs and running statistics to 1e-5."""
    torch.set_num_threads(1)
    c = train_golden_case(golden("train_tiny"), case)
    form = "sum" if c["form"] == "kl_weight" else "mean"
    losses, grads, pre, running = port_step(c["init"], c["shape"].seq_len, c["poses"][0], c["eps"][0], c["w"], form)
    r = F64.forward_backward(c["init"], c["shape"].seq_len, c["poses"][0], c["eps"][0], c["w"], form)
    np.testing.assert_allclose(losses, r["losses"], rtol=1e-5)
    np.testing.assert_allclose(r["losses"], c["losses"][0], rtol=2e-5)
    assert list(r["grads"]) == list(grads)
    gmax = max(float(np.abs(v).max()) for v in r["grads"].values())
    for k, v in r["grads"].items():
        d = float(np.abs(grads[k] - v).max())
        assert d <= (5e-6 * gmax if k.endswith(".0.bias") else 2e-4 * np.abs(v).max() + 5e-7 * gmax), (k, d)
    for k, v in r["pre"].items():
        assert np.abs(pre[k] - v).max() <= 1e-5 * max(1.0, np.abs(v).max()), k
    for k, v in r["running"].items():
        assert np.abs(running[k] - v).max() <= 1e-5 * max(1.0, np.abs(v).max()), k


@pytest.mark.parametrize("form", ["mean", "sum"])
@pytest.mark.parametrize("n_hidden", [1, 7])
@pytest.mark.parametrize("T", [3, 7, 16])
def test_gradients_are_the_central_differences(T, n_hidden, form):
    """Two sampled entries of every tensor: (L(p + h) - L(p - h)) / 2h at h = 1e-5 with the LeakyReLU branches held where they are
    at p (masks), so that no difference straddles a kink.  float64: truncation ~ h^2, rounding ~ 1e-16 L / h -- allowed 1e-6 of the
    entry plus 1e-7 of the largest gradient."""
    shape = vae_schema.VAEShape(latent_dim=5, seq_len=T, hidden=(8,) * n_hidden)
    sd = initial_state_dict(shape, 40 + T)
    rng = np.random.default_rng(T * 10 + n_hidden)
    # (statistics away from their initial 0 / 1 and BatchNorm affine parameters away from 1 / 0: every term is live)
    for k in sd:
        if k.endswith(".1.weight"):
            sd[k] = rng.uniform(0.7, 1.3, sd[k].shape).astype(np.float32)
        elif k.endswith(".1.bias"):
            sd[k] = rng.uniform(-0.2, 0.2, sd[k].shape).astype(np.float32)
    B = 3
    poses = synth.make_training_windows(B, T, 50 + T)
    eps = rng.standard_normal((B, 5))
    base = F64.forward_backward(sd, T, poses, eps, KLD_WEIGHT, form)
    masks = {k: v > 0 for k, v in base["pre"].items()}
    gmax = max(float(np.abs(v).max()) for v in base["grads"].values())
    h = 1e-5
    for k, g in base["grads"].items():
        for idx in rng.integers(0, g.size, 2):
            vals = []
            for sgn in (1.0, -1.0):
                sd2 = dict(sd)
                a = np.asarray(sd[k], np.float64).copy()
                a.reshape(-1)[idx] += sgn * h
                sd2[k] = a
                vals.append(F64.loss_only(sd2, T, poses, eps, KLD_WEIGHT, form, masks))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g.reshape(-1)[idx]) <= 1e-6 * abs(fd) + 1e-7 * gmax, (k, int(idx), fd, float(g.reshape(-1)[idx]))


def test_adam_is_torch_adam_in_float64():
    rng = np.random.default_rng(0)
    p0 = rng.standard_normal(257)
    g = rng.standard_normal((2, 257)) * np.array([1.0, 1e-6])[:, None]
    q = torch.nn.Parameter(torch.as_tensor(p0.copy()))
    opt = torch.optim.Adam([q], lr=1e-3, weight_decay=1e-4)
    p, m, v = p0, np.zeros(257), np.zeros(257)
    for s in range(2):
        q.grad = torch.as_tensor(g[s].copy())
        opt.step()
        p_prev = p
        p, m, v = F64.adam_step(p, g[s], m, v, s + 1, 1e-3, 1e-4)
        st = opt.state[q]
        np.testing.assert_allclose(p, q.detach().numpy(), rtol=0, atol=1e-15)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-14, atol=1e-300)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-14, atol=1e-300)
        np.testing.assert_array_equal(p, F64.adam_apply(p_prev, m, v, s + 1, 1e-3))


MEASURED = {}


def test_allowances(capsys):
    """The fp32 port against float64 with the port's LeakyReLU signs adopted, over every case of the table: the smallest (a, b) on
    the ray a = 100 b (the ratio of the condition a <= 5e-5, b <= 5e-7) such that every gradient tensor is within a max|ref_k| + b
    gmax, and the smallest b0, c, loss and statistics deviations.  Asserts the issue's condition and that train_cases.PORT_* (what
    the GPU test multiplies by four) cover what is measured."""
    torch.set_num_threads(1)
    worst = dict(a=0.0, b0=0.0, c=0.0, loss=0.0, stat=0.0, flips=0, raw=0.0)
    rows = []
    for case in CASES:
        shape, init, poses, eps = inputs(case, steps=1)
        losses, grads, pre, running = port_step(init, case.T, poses[0], eps[0], KLD_WEIGHT, case.form)
        masks = {k: v > 0 for k, v in pre.items()}
        r = F64.forward_backward(init, case.T, poses[0], eps[0], KLD_WEIGHT, case.form, masks)
        free = F64.forward_backward(init, case.T, poses[0], eps[0], KLD_WEIGHT, case.form)
        gmax = max(float(np.abs(v).max()) for v in r["grads"].values())
        a = b0 = raw = 0.0
        for k, v in r["grads"].items():
            d = float(np.abs(grads[k] - v).max())
            if k.endswith(".0.bias"):
                b0 = max(b0, d / gmax)
            else:
                a = max(a, d / (np.abs(v).max() + 0.01 * gmax))
                raw = max(raw, float(np.abs(grads[k] - free["grads"][k]).max()) / (np.abs(v).max() + 0.01 * gmax))
        c = max(float(np.abs(pre[k] - v).max()) / max(1.0, float(np.abs(v).max())) for k, v in r["pre"].items())
        flips = sum(int(((free["pre"][k] > 0) != masks[k]).sum()) for k in masks)
        # an adopted sign that float64 would not have taken sits at an input of rounding size
        for k, v in r["pre"].items():
            bad = (v > 0) != masks[k]
            assert not bad.any() or np.abs(v[bad]).max() <= 4 * PORT_C * max(1.0, float(np.abs(v).max())), (case.name, k)
        loss = max(abs(x - y) / abs(y) for x, y in zip(losses, r["losses"]))
        stat = max(float(np.abs(running[k] - v).max()) / max(1.0, float(np.abs(v).max())) for k, v in r["running"].items())
        rows.append((case.name, a, b0, c, loss, stat, flips, raw))
        for key, val in (("a", a), ("b0", b0), ("c", c), ("loss", loss), ("stat", stat), ("flips", flips), ("raw", raw)):
            worst[key] = max(worst[key], val)
    MEASURED.update(worst)
    with capsys.disabled():
        print("\ncase: a (b = a / 100), b0, c, loss, stat, sign flips without adoption, a without adoption")
        for row in rows:
            print("  %-20s %.2e %.2e %.2e %.2e %.2e %d %.2e" % row)
        print("  worst: " + ", ".join("%s=%.3g" % kv for kv in worst.items()))
    assert worst["a"] <= 5e-5 and worst["a"] / 100 <= 5e-7, worst          # the issue's condition on the port
    assert worst["a"] <= PORT_A and worst["a"] / 100 <= PORT_B and worst["b0"] <= PORT_B0 and worst["c"] <= PORT_C, worst
    assert worst["loss"] <= PORT_LOSS and worst["stat"] <= PORT_STAT, worst
