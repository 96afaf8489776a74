"""A numpy twin of the two latent-space kernels, written from their definitions in float64 -- except the
straight path, which is the reference's own expression (networks/interpolant.py:126) on float32 arrays."""
import numpy as np


def linear_path(a, b, steps):
    """[steps, D] float32: the end points themselves, between them `first_z + (i / (steps - 1.)) * (second_z - first_z)` as numpy
    computes it on float32 arrays (the Python float is weak: rounded to float32, then three float32 operations)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    out = np.empty((steps, a.shape[0]), dtype=np.float32)
    out[0], out[steps - 1] = a, b
    for i in range(1, steps - 1):
        out[i] = a + (i / (steps - 1.)) * (b - a)
    assert out.dtype == np.float32
    return out


def takes_fallback(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.sqrt((a * a).sum()), np.sqrt((b * b).sum())
    if na == 0.0 or nb == 0.0:
        return True
    w = np.arccos(np.clip((a * b).sum() / (na * nb), -1.0, 1.0))
    return not np.sin(w) >= 1e-6


def spherical_path(a, b, steps):
    """[steps, D] float32: (sin((1 - t) w) a + sin(t w) b) / sin w in float64, rounded once; the straight path where the great
    circle is not defined."""
    if takes_fallback(a, b):
        return linear_path(a, b, steps)
    a32, b32 = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    na, nb = np.sqrt((a * a).sum()), np.sqrt((b * b).sum())
    w = np.arccos(np.clip((a * b).sum() / (na * nb), -1.0, 1.0))
    out = np.empty((steps, a.shape[0]), dtype=np.float32)
    out[0], out[steps - 1] = a32, b32
    for i in range(1, steps - 1):
        t = float(i) / (steps - 1)
        out[i] = ((np.sin((1.0 - t) * w) * a + np.sin(t * w) * b) / np.sin(w)).astype(np.float32)
    return out


def paths(za, zb, steps, mode):
    f = {"linear": linear_path, "spherical": spherical_path}[mode]
    return np.stack([f(a, b, steps) for a, b in zip(za, zb)])


def report_rows(mu, logvar, x=None, rec=None):
    """[B,5] float64: sum mu^2, sum (exp(logvar / 2) - 1)^2, -1/2 sum (1 + logvar - mu^2 - exp(logvar)), and over the window's
    points (x, rec [B, n_points * 3]) the mean and the maximum of |rec - x|; NaN for the last two without x / rec."""
    mu, lv = np.asarray(mu, dtype=np.float32).astype(np.float64), np.asarray(logvar, dtype=np.float32).astype(np.float64)
    out = np.full((mu.shape[0], 5), np.nan)
    out[:, 0] = (mu * mu).sum(axis=1)
    out[:, 1] = ((np.exp(0.5 * lv) - 1.0) ** 2).sum(axis=1)
    out[:, 2] = -0.5 * (1.0 + lv - mu * mu - np.exp(lv)).sum(axis=1)
    if x is not None and rec is not None:
        x = np.asarray(x, dtype=np.float32).astype(np.float64).reshape(mu.shape[0], -1, 3)
        rec = np.asarray(rec, dtype=np.float32).astype(np.float64).reshape(mu.shape[0], -1, 3)
        d = rec - x
        dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        out[:, 3], out[:, 4] = dist.mean(axis=1), dist.max(axis=1)
    return out


def report_cols(mu, logvar):
    """[3,D] float64: sum_n mu_d, sum_n mu_d^2, sum_n exp(logvar_d)."""
    mu, lv = np.asarray(mu, dtype=np.float32).astype(np.float64), np.asarray(logvar, dtype=np.float32).astype(np.float64)
    return np.stack([mu.sum(axis=0), (mu * mu).sum(axis=0), np.exp(lv).sum(axis=0)])


def var_mu(mu):
    """Var_n[mu_d], the population variance."""
    mu = np.asarray(mu, dtype=np.float32).astype(np.float64)
    m = mu.mean(axis=0)
    return np.maximum((mu * mu).mean(axis=0) - m * m, 0.0)
