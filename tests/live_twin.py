"""numpy twins of live mode: the One-Euro filter in the reference's arithmetic, vectorised over the
coordinates, and the emit schedule -- which frames a window makes final, what is held, what `flush` adds, what is dropped."""
import math

import numpy as np

T, OVERLAP, STRIDE = 10, 2, 8


def smoothing_factor(t_e, cutoff):
    r = 2 * math.pi * cutoff * t_e
    return r / (r + 1)


class OneEuro:
    """The filter's state over any number of coordinates; the first frame passes through."""

    def __init__(self, params):
        self.min_cutoff, self.beta, self.d_cutoff = (float(v) for v in params)
        self.t_prev = self.x_prev = self.dx_prev = None

    def __call__(self, t, x):
        x = np.asarray(x, dtype=np.float64)
        if self.t_prev is None:
            self.t_prev, self.x_prev, self.dx_prev = float(t), x.copy(), np.zeros_like(x)
            return x.copy()
        t_e = float(t) - self.t_prev
        a_d = smoothing_factor(t_e, self.d_cutoff)
        dx = (x - self.x_prev) / t_e
        dx_hat = a_d * dx + (1 - a_d) * self.dx_prev
        cutoff = self.min_cutoff + self.beta * np.abs(dx_hat)
        a = smoothing_factor(t_e, cutoff)
        x_hat = a * x + (1 - a) * self.x_prev
        self.t_prev, self.x_prev, self.dx_prev = float(t), x_hat, dx_hat
        return x_hat


def one_euro(seq, times, params, n_chunks=1):
    """`seq` [n_chunks*F, ...] filtered along the frames of every chunk, fresh state per chunk."""
    seq, times = np.asarray(seq, dtype=np.float64), np.asarray(times, dtype=np.float64)
    out, F = np.empty_like(seq), len(seq) // n_chunks
    for c in range(n_chunks):
        f = OneEuro(params)
        for i in range(c * F, (c + 1) * F):
            out[i] = f(times[i], seq[i])
    return out


class EmitSchedule:
    """The stream as live mode emits it: `window(G)` takes window w's result [10, ...] and returns the 8 frames [8w, 8w + 8) it
    makes final; `flush()` returns the two held frames."""

    def __init__(self):
        self.held, self.n_windows = None, 0

    def window(self, G):
        G = np.asarray(G)
        out = G[:STRIDE].copy()
        if self.held is not None:
            out[:OVERLAP] = (self.held + G[:OVERLAP]) / 2
        self.held = G[STRIDE:].copy()
        self.n_windows += 1
        return out

    def flush(self):
        held, self.held = self.held, None
        return held if held is not None else np.empty((0,))


def n_windows(n_pushed):
    return len(range(0, n_pushed - T + 1, STRIDE))


def dropped(n_pushed):
    """Frames of a stream of `n_pushed` that belong to no complete window."""
    w = n_windows(n_pushed)
    return n_pushed - (w * STRIDE + OVERLAP if w else 0)


def stream(windows):
    """All windows of a stream through the schedule, then the flush: what a session returns in total."""
    s = EmitSchedule()
    parts = [s.window(G) for G in windows]
    tail = s.flush()
    return np.concatenate(parts + [tail]) if len(parts) else tail
