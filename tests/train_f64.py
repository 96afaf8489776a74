"""The VAE training step in float64 -- TEST INFRASTRUCTURE: a plain functional restatement with torch on the CPU of what
gem_trainer_step computes (csrc/train.hip): the train-mode forward (Conv1d / ConvTranspose1d k=3 s=1 p=1, BatchNorm1d batch
statistics, LeakyReLU 0.01), both forms of the VAE loss (mean-squared / summed squared error + kld_weight * KL), the backward by
autograd, the running statistics (momentum, unbiased variance) and Adam with the weight decay folded into the gradient.

LeakyReLU sign adoption: in fp32 an activation within rounding of zero may take the other branch than in float64, and the
gradients of the two runs then differ by far more than rounding (one flip among 1e4 .. 1e6 activations moves single gradient
entries by 1e-4 .. 1e-2 of their tensor's maximum).  `masks` hands this restatement the branch another run took, per block:
where a mask is given the block computes where(mask, v, 0.01 v) instead of where(v > 0, v, 0.01 v), so that both sides
differentiate the same piecewise-linear function and what is left between them is rounding.

Keys are those of the checkpoint schema (globalegomocap_amd.vae.VAEShape.schema); blocks are named by their prefix
("encoder.0", ..., "decoder.0", ..., "final_layer").  Activations are handed in and out as [B, T, channels]."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

SLOPE = 0.01
BN_EPS = 1e-5


def block_names(sd):
    """(encoder block prefixes, decoder block prefixes incl. 'final_layer') of a state dict."""
    enc, i = [], 0
    while "encoder.%d.0.weight" % i in sd:
        enc.append("encoder.%d" % i)
        i += 1
    dec, i = [], 0
    while "decoder.%d.0.weight" % i in sd:
        dec.append("decoder.%d" % i)
        i += 1
    return enc, dec + ["final_layer"]


def parameter_keys(sd):
    return [k for k in sd if not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))]


def forward_backward(sd, seq_len, poses, eps, kld_weight, form="mean", masks=None, momentum=0.1, need_grad=True):
    """One train-mode forward (and backward) in float64.  sd: state dict (numpy / tensors), poses [B,T,C], eps [B,D];
    form "mean" (F.mse_loss) or "sum" (summed squared error); masks: {block prefix: bool [B,T,channels]} or None.
    Returns a dict: losses (loss, recon, kld), grads {key: array}, pre / out {block: [B,T,c]} (LeakyReLU inputs / block outputs),
    pose [B,T,C], mu, logvar, running {key: array} (the statistics after this forward)."""
    t64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))          # noqa: E731
    keys = parameter_keys(sd)
    p = OrderedDict((k, t64(sd[k]).clone().requires_grad_(need_grad)) for k in keys)
    x = t64(poses)
    e = t64(eps)
    B, T, C = x.shape
    assert T == seq_len
    enc, dec = block_names(sd)
    masks = masks or {}
    pre, out, running = OrderedDict(), OrderedDict(), OrderedDict()
    n = B * T

    def bn_act(name, y):
        mean = y.mean(dim=(0, 2))
        var = ((y - mean[None, :, None]) ** 2).mean(dim=(0, 2))                 # biased: what normalises the batch
        v = p[name + ".1.weight"][None, :, None] * ((y - mean[None, :, None]) / torch.sqrt(var + BN_EPS)[None, :, None]) + p[name + ".1.bias"][None, :, None]
        m = masks.get(name)
        m = (v > 0) if m is None else torch.as_tensor(np.asarray(m, bool)).permute(0, 2, 1)
        o = torch.where(m, v, SLOPE * v)
        pre[name], out[name] = v.detach().permute(0, 2, 1).numpy().copy(), o.detach().permute(0, 2, 1).numpy().copy()
        unbiased = var.detach() * (n / (n - 1.0)) if n > 1 else var.detach()
        running[name + ".1.running_mean"] = ((1 - momentum) * t64(sd[name + ".1.running_mean"]) + momentum * mean.detach()).numpy()
        running[name + ".1.running_var"] = ((1 - momentum) * t64(sd[name + ".1.running_var"]) + momentum * unbiased).numpy()
        return o

    h = x.permute(0, 2, 1)
    for name in enc:
        h = bn_act(name, F.conv1d(h, p[name + ".0.weight"], p[name + ".0.bias"], padding=1))
    flat = h.flatten(1)
    mu = flat @ p["fc_mu.weight"].T + p["fc_mu.bias"]
    logvar = flat @ p["fc_var.weight"].T + p["fc_var.bias"]
    z = e * torch.exp(0.5 * logvar) + mu
    h = (z @ p["decoder_input.weight"].T + p["decoder_input.bias"]).view(B, -1, T)
    for name in dec:
        h = bn_act(name, F.conv_transpose1d(h, p[name + ".0.weight"], p[name + ".0.bias"], padding=1))
    rec = F.conv1d(h, p["final_layer.3.weight"], p["final_layer.3.bias"], padding=1).permute(0, 2, 1)
    sq = ((rec - x) ** 2).sum()
    recon = sq / (B * T * C) if form == "mean" else sq
    kld = (-0.5 * (1 + logvar - mu ** 2 - logvar.exp()).sum(dim=1)).mean()
    loss = recon + kld_weight * kld
    grads = OrderedDict()
    if need_grad:
        for k, g in zip(keys, torch.autograd.grad(loss, [p[k] for k in keys])):
            grads[k] = g.numpy().copy()
    return dict(losses=(float(loss.detach()), float(recon.detach()), float(kld.detach())), grads=grads, pre=pre, out=out, pose=rec.detach().numpy().copy(),
                mu=mu.detach().numpy().copy(), logvar=logvar.detach().numpy().copy(), running=running)


def loss_only(sd, seq_len, poses, eps, kld_weight, form="mean", masks=None):
    return forward_backward(sd, seq_len, poses, eps, kld_weight, form, masks, need_grad=False)["losses"][0]


def adam_moments(g, p, m, v, weight_decay, b1=0.9, b2=0.999):
    """torch.optim.Adam's moments after one more gradient: the L2 weight decay is added to the gradient first."""
    g = np.asarray(g, np.float64) + weight_decay * np.asarray(p, np.float64)
    return b1 * np.asarray(m, np.float64) + (1 - b1) * g, b2 * np.asarray(v, np.float64) + (1 - b2) * g * g


def adam_apply(p, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """The parameter after Adam's update from the moments `m`, `v` of step number `step` (1 for the first)."""
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return np.asarray(p, np.float64) - (lr / bc1) * np.asarray(m, np.float64) / (np.sqrt(np.asarray(v, np.float64)) / np.sqrt(bc2) + eps)


def adam_step(p, g, m, v, step, lr, weight_decay, b1=0.9, b2=0.999, eps=1e-8):
    """(p, m, v) after step number `step` of torch.optim.Adam(lr, betas, eps, weight_decay) on gradient g."""
    m1, v1 = adam_moments(g, p, m, v, weight_decay, b1, b2)
    return adam_apply(p, m1, v1, step, lr, b1, b2, eps), m1, v1
