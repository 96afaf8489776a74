"""Sliding-window bookkeeping of the sequence pipeline (host side, numpy).

Window starts, overlap averaging and the final Gaussian smoothing follow the reference's `main()`
(`optimizer.py:370,425-450`); the window optimisation itself is one batched device call
(`WindowEngine.optimize_windows`).
"""
import numpy as np

SEQ_LEN = 10       # optimizer.py:328
OVERLAP = 2        # optimizer.py:330


def window_starts(n_frames, seq_len=SEQ_LEN, overlap=OVERLAP):
    """range(0, N - seq_len + 1, seq_len - overlap)  (optimizer.py:370); the last N-2.. frames of a
    100-frame chunk are never optimised (D7)."""
    return np.arange(0, n_frames - seq_len + 1, seq_len - overlap, dtype=np.int32)


def cut_windows(frames, starts, seq_len=SEQ_LEN):
    frames = np.asarray(frames)
    return np.stack([frames[s:s + seq_len] for s in starts]) if len(starts) else frames[:0].reshape((0, seq_len) + frames.shape[1:])


def merge_batches(windows, overlap=OVERLAP):
    """Average the `overlap` frames shared by neighbouring windows (optimizer.py:425-437)."""
    w = np.asarray(windows)
    if overlap == 0:
        return np.concatenate(w)
    parts = [w[0][:-overlap]]
    for i in range(len(w) - 1):
        parts.append((w[i][-overlap:] + w[i + 1][:overlap]) / 2)
        parts.append(w[i + 1][overlap:-overlap])
    parts.append(w[-1][-overlap:])
    return np.concatenate(parts)


def merge_chunks(windows, n_chunks, overlap=OVERLAP):
    """merge_batches for n_chunks chunks of equally many windows at once: [n_chunks*wpc, T, ...] -> [n_chunks, fpc, ...]
    (same arithmetic per element as merge_batches, vectorised over the chunks)."""
    w = np.asarray(windows)
    wpc, T = w.shape[0] // n_chunks, w.shape[1]
    w = w.reshape((n_chunks, wpc, T) + w.shape[2:])
    if overlap == 0:
        return w.reshape((n_chunks, wpc * T) + w.shape[3:])
    step = T - overlap
    out = np.empty((n_chunks, wpc * step + overlap) + w.shape[3:], dtype=w.dtype)
    out[:, :step] = w[:, 0, :step]
    for i in range(1, wpc):
        out[:, i * step:i * step + overlap] = (w[:, i - 1, -overlap:] + w[:, i, :overlap]) / 2
        out[:, i * step + overlap:(i + 1) * step] = w[:, i, overlap:step]
    out[:, wpc * step:] = w[:, -1, -overlap:]
    return out


def dense_counts(n_windows, stride, seq_len=SEQ_LEN):
    """How many of `n_windows` windows, `stride` frames from one another, cover each of the (n_windows - 1) * stride + seq_len frames."""
    count = np.zeros((n_windows - 1) * stride + seq_len, dtype=np.int64)
    for i in range(n_windows):
        count[i * stride:i * stride + seq_len] += 1
    return count


def merge_dense(windows, stride, n_chunks=None):
    """Every frame the mean of ALL windows that cover it, for windows `stride` frames from one another (1 <= stride <= T; live mode's
    dense path and `WindowEngine.merge_dense`): ((G_a[i_a] + G_b[i_b]) + ...) / count over the covering windows
    oldest first, in float64.  [n, T, ...] -> [(n - 1) * stride + T, ...]; with n_chunks, [n_chunks*wpc, T, ...] -> [n_chunks, fpc, ...]
    per chunk.  For stride >= T / 2 these are the bits of merge_batches / merge_chunks with overlap = T - stride."""
    w = np.asarray(windows, dtype=np.float64)
    chunks = 1 if n_chunks is None else int(n_chunks)
    if w.ndim < 2 or chunks < 1 or w.shape[0] == 0 or w.shape[0] % chunks:
        raise ValueError("merge_dense: windows of shape %s do not split into %d chunks" % (w.shape, chunks))
    wpc, T, stride = w.shape[0] // chunks, w.shape[1], int(stride)
    if not 1 <= stride <= T:
        raise ValueError("merge_dense: the stride is between 1 and %d frames, got %d" % (T, stride))
    w = w.reshape((chunks, wpc, T) + w.shape[2:])
    count = dense_counts(wpc, stride, T)
    out = np.empty((chunks, len(count)) + w.shape[3:], dtype=np.float64)
    seen = 0          # frames below `seen` have been reached by a window before this one
    for i in range(wpc):
        a = i * stride
        old = max(0, min(seen - a, T))
        out[:, a:a + old] += w[:, i, :old]
        out[:, a + old:a + T] = w[:, i, old:]          # (taken as it is: 0 + x would lose the sign of -0)
        seen = a + T
    out /= count.reshape((1, -1) + (1,) * (out.ndim - 2))
    return out[0] if n_chunks is None else out


def cover_starts(n_frames, seq_len=SEQ_LEN, stride=SEQ_LEN - OVERLAP):
    """The window table of a recording optimised as one motion: range(0, N - seq_len + 1, stride), plus
    N - seq_len when the last regular window ends before N, so that EVERY frame lies in a window.  1 <= stride <= seq_len - 2 and
    N >= seq_len, else ValueError.  For N = stride * k + seq_len this is the regular table alone (`window_starts` at stride 8)."""
    n_frames, seq_len, stride = int(n_frames), int(seq_len), int(stride)
    if not 1 <= stride <= seq_len - 2:
        raise ValueError("cover_starts: the stride is between 1 and %d frames, got %d" % (seq_len - 2, stride))
    if n_frames < seq_len:
        raise ValueError("cover_starts: %d frames cannot hold a %d-frame window" % (n_frames, seq_len))
    starts = list(range(0, n_frames - seq_len + 1, stride))
    if starts[-1] + seq_len < n_frames:
        starts.append(n_frames - seq_len)
    return np.asarray(starts, dtype=np.int32)


def check_cover(starts, seq_len=SEQ_LEN):
    """ValueError unless the windows [s, s + seq_len) of `starts` cover [0, starts[-1] + seq_len) without a hole, each start once and in
    order: starts[0] == 0, strictly ascending, no step longer than seq_len.  -> the starts as an int64 array."""
    s = np.asarray(starts).reshape(-1).astype(np.int64)
    if len(s) == 0 or s[0] != 0:
        raise ValueError("a window table starts at frame 0, got %s" % (s[:1].tolist(),))
    step = np.diff(s)
    if (step <= 0).any():
        raise ValueError("window starts must be strictly ascending (starts %s are not)" % s[1:][step <= 0][:4].tolist())
    if (step > seq_len).any():
        raise ValueError("no %d-frame window covers the frames before the starts %s" % (seq_len, s[1:][step > seq_len][:4].tolist()))
    return s


def merge_cover(windows, starts, want_spread=False):
    """Every frame the mean of ALL windows that cover it, for windows at any starts `check_cover` accepts (the definition
    `WindowEngine.merge_cover` is held to): ((G_a + G_b) + ...) / count over the covering windows oldest first, in
    float64; a frame's first window is taken as it is (0 + x would lose the sign of -0).  [B, T, J, 3] -> (merged [starts[-1] + T, J, 3],
    count [N] int32); with want_spread also spread [N]: the largest Euclidean distance, over joints and covering windows, between a
    window's joint and the merged joint -- how far the windows that cover a frame disagree about it; 0.0 where count is 1.  At
    `window_starts` these are the bits of merge_batches, at a constant stride those of merge_dense."""
    w = np.asarray(windows, dtype=np.float64)
    if w.ndim != 4 or w.shape[3] != 3:
        raise ValueError("merge_cover: windows must be [B, T, J, 3], got %s" % (w.shape,))
    T = w.shape[1]
    s = check_cover(starts, T)
    if len(s) != w.shape[0]:
        raise ValueError("merge_cover: %d starts for %d windows" % (len(s), w.shape[0]))
    n = int(s[-1]) + T
    out = np.empty((n,) + w.shape[2:], dtype=np.float64)
    count = np.zeros(n, dtype=np.int32)
    seen = 0          # frames below `seen` have been reached by a window before this one
    for i, a in enumerate(s.tolist()):
        old = max(0, min(seen - a, T))
        out[a:a + old] += w[i, :old]
        out[a + old:a + T] = w[i, old:]
        count[a:a + T] += 1
        seen = a + T
    out /= count.reshape(-1, 1, 1)
    if not want_spread:
        return out, count
    spread = np.zeros(n, dtype=np.float64)
    for i, a in enumerate(s.tolist()):
        d = w[i] - out[a:a + T]
        d = d * d
        spread[a:a + T] = np.maximum(spread[a:a + T], np.sqrt((d[..., 0] + d[..., 1]) + d[..., 2]).max(axis=1))
    spread[count == 1] = 0.0
    return out, count, spread


def final_smooth(seq):
    """scipy gaussian_filter1d(sigma=1, axis=0) (optimizer.py:448-450)."""
    from scipy.ndimage import gaussian_filter1d
    return gaussian_filter1d(np.asarray(seq), sigma=1, axis=0)


def relative_global_numpy(local, cams):
    """float64 host twin of the device transform, for the *unoptimised* sequences that main() also
    returns (utils/utils.py:99-112): X_rel[t] = C0^-1 C_t X_loc[t], per window."""
    local = np.asarray(local, dtype=np.float64)
    cams = np.asarray(cams, dtype=np.float64)
    M = np.matmul(np.linalg.inv(cams[:, 0])[:, None], cams)
    return np.matmul(local, np.swapaxes(M[..., :3, :3], -1, -2)) + M[..., None, :3, 3]


def to_global_numpy(rel, cams):
    """X_glob = C0 X_rel (optimizer.py:302-308), per window, float64."""
    rel = np.asarray(rel, dtype=np.float64)
    c0 = np.asarray(cams, dtype=np.float64)[:, 0]
    return np.matmul(rel, np.swapaxes(c0[:, None, :3, :3], -1, -2)) + c0[:, None, None, :3, 3]
