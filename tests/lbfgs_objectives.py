"""Analytic objectives for the lock-step L-BFGS tests (CPU: torch.optim.LBFGS against the oracle's machine; GPU:
lbfgs_advance_kernel against its twin).  All arithmetic is torch float32 with seeded float32 constants, so the CPU and GPU
tests feed the optimisers the same kind of (f, g): a float32 value and a float32 autograd gradient.

`make(name, D, seed, scale, device)` returns `(fun, x0)`: `fun(x [D] f32) -> (f 0-dim f32, g [D] f32)`, `x0 [D] f32`.
"""
import math

import torch

NAMES = ("quad", "rosen", "logcosh", "sines", "leaky", "quartic", "optimum", "tiny")


def _consts(D, seed, device):
    gen = torch.Generator().manual_seed(1000 + seed)
    c = torch.randn(D, generator=gen, dtype=torch.float32)
    u = torch.rand(D, generator=gen, dtype=torch.float32)
    return c.to(device), u.to(device)


def _value(name, D, c, u):
    if name == "quad":            # ill-conditioned quadratic, eigenvalues logspace(0, 4)
        eig = torch.logspace(0, 4, D, dtype=torch.float32, device=c.device)
        return lambda x: 0.5 * (eig * (x - c) ** 2).sum() / D
    if name == "rosen":           # chained Rosenbrock
        return lambda x: (100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2).sum() / D
    if name == "logcosh":         # log cosh(a x - c) (stable form) + quartic
        a = 0.5 + 2.0 * u

        def f(x):
            z = (a * x - c).abs()
            return (z + torch.nn.functional.softplus(-2.0 * z) - math.log(2.0)).sum() / D + 0.1 * (x ** 4).sum() / D
        return f
    if name == "sines":           # quadratic + sines: non-convex along most search directions
        w = 0.2 + u
        return lambda x: (0.5 * w * x ** 2).sum() / D + 1.5 * torch.sin(3.0 * x + c).sum() / D
    if name == "leaky":           # squared LeakyReLU(0.2) + smoothness of neighbouring coordinates
        return lambda x: (torch.nn.functional.leaky_relu(x - c, 0.2) ** 2).sum() / D + 0.5 * ((x[1:] - x[:-1]) ** 2).sum() / D
    if name == "quartic":         # steep quartic (started from x0 = 2: the first steps overshoot); its minimum lies away from
        k = 0.5 + u               # the origin, so that max|trial| stays of order one while it converges
        return lambda x: (k * (x - 0.5 * c) ** 4).sum()
    if name == "optimum":         # started at its optimum: the gradient of the first evaluation is exactly zero
        return lambda x: 0.5 * ((x - c) ** 2).sum()
    if name == "tiny":            # value scaled by 1e-9: max|g| <= tolerance_grad
        k = 1.0 + 9.0 * u
        return lambda x: 1e-9 * (0.5 * k * (x - c) ** 2).sum() / D
    raise KeyError(name)


def make(name, D, seed=0, scale=1.0, device="cpu"):
    c, u = _consts(D, seed, device)
    value = _value(name, D, c, u)
    gen = torch.Generator().manual_seed(2000 + seed)
    if name == "quartic":
        x0 = torch.full((D,), 2.0, dtype=torch.float32)
    elif name == "optimum":
        x0 = c.cpu().clone()
    else:
        x0 = scale * torch.randn(D, generator=gen, dtype=torch.float32)

    def fun(x):
        xr = x.detach().clone().requires_grad_(True)
        f = value(xr)
        g, = torch.autograd.grad(f, xr)
        return f.detach(), g

    return fun, x0.to(device)
