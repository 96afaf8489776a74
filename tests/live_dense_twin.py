"""numpy twins of dense live mode ("Dense live mode"): a window every k frames, every frame the mean of all
windows that cover it -- written frame by frame, independently of `sequence.merge_dense` -- the emit schedule of a dense session
(what a window settles, what it gives to `now`, what `flush` adds, what is dropped) and the estimated frames in the kernel's order of
operations."""
import numpy as np

import live_twin as LT

T = LT.T


def n_windows(n_pushed, k):
    return len(range(0, n_pushed - T + 1, k))


def dropped(n_pushed, k):
    """Frames of a stream of `n_pushed` that belong to no complete window at stride k."""
    w = n_windows(n_pushed, k)
    return n_pushed - ((w - 1) * k + T if w else 0)


def covering(f, n, k, t=T):
    """The windows, of n at stride k, that cover frame f, oldest first."""
    return [w for w in range(n) if w * k <= f < w * k + t]


def counts(n, k, t=T):
    return np.array([len(covering(f, n, k, t)) for f in range((n - 1) * k + t)])


def merge_dense(windows, k, n_chunks=1):
    """[n_chunks*wpc, T, ...] at stride k -> [n_chunks, (wpc-1) k + T, ...]: frame by frame ((G_a + G_b) + ...) / count, oldest first."""
    w = np.asarray(windows, dtype=np.float64)
    wpc, t = w.shape[0] // n_chunks, w.shape[1]
    out = np.empty((n_chunks, (wpc - 1) * k + t) + w.shape[2:])
    for c in range(n_chunks):
        G = w[c * wpc:(c + 1) * wpc]
        for f in range(out.shape[1]):
            cover = covering(f, wpc, k, t)
            acc = G[cover[0], f - cover[0] * k].copy()
            for i in cover[1:]:
                acc = acc + G[i, f - i * k]
            out[c, f] = acc / len(cover)
    return out


class DenseSchedule:
    """The stream as a dense session emits it: `window(G)` takes window w's result [10, ...] and returns (the k frames [k w, k w + k)
    it settles, its `now` frames: all 10 of window 0, else its last k); `flush()` returns the 10 - k held frames."""

    def __init__(self, k):
        self.k, self.n_windows, self.sums = k, 0, {}          # frame -> [sum so far, count]

    def window(self, G):
        G, k, w = np.asarray(G, dtype=np.float64), self.k, self.n_windows
        for i in range(T):
            f = k * w + i
            if f in self.sums:
                self.sums[f] = [self.sums[f][0] + G[i], self.sums[f][1] + 1]
            else:
                self.sums[f] = [G[i].copy(), 1]
        settled = np.stack([self._take(k * w + i) for i in range(k)])
        self.n_windows += 1
        return settled, (G.copy() if w == 0 else G[T - k:].copy())

    def _take(self, f):
        s, c = self.sums.pop(f)
        return s / c

    def flush(self):
        held = [self._take(f) for f in sorted(self.sums)]
        return np.stack(held) if held else np.empty((0,))


def stream(windows, k):
    """All windows of a stream through the schedule, then the flush -> (settled [(n-1) k + 10, ...], now [(n-1) k + 10, ...])."""
    s = DenseSchedule(k)
    got = [s.window(G) for G in windows]
    return np.concatenate([g[0] for g in got] + [s.flush()]), np.concatenate([g[1] for g in got])


def estimated(cams, pose):
    """cams [n,4,4] f64 . pose [n,15,3] f32 in the emit kernels' order: ((M0 p0 + M1 p1) + M2 p2) + M3 in f64, nothing fused."""
    M, p = np.asarray(cams, dtype=np.float64)[:, None, :3, :], np.asarray(pose, dtype=np.float32).astype(np.float64)[:, :, None, :]
    return ((M[..., 0] * p[..., 0] + M[..., 1] * p[..., 1]) + M[..., 2] * p[..., 2]) + M[..., 3]
