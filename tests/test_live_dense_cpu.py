"""Dense live mode on the host ("Dense live mode"): the twins against `sequence.merge_batches` / `merge_chunks`,
`sequence.merge_dense` against the twin, coverage counts, the generalised `_pieces` and `dropped_frames`, argument errors, the
bindings of include/gem_live_dense.h."""
import os
import re

import numpy as np
import pytest

import live_twin as LT
import live_dense_twin as DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_windows", [1, 2, 5])
def test_twin_settled_stream_at_stride_8_is_merge_batches(n_windows):
    from globalegomocap_amd.sequence import merge_batches
    G = np.random.default_rng(n_windows).normal(size=(n_windows, 10, 15, 3))
    G[0, 0, 0, 0] = -0.0                                                  # a first window is taken as it is, sign of zero included
    want = np.asarray(merge_batches(G, 2))
    s, old = DT.DenseSchedule(8), LT.EmitSchedule()
    for w in range(n_windows):
        settled, now = s.window(G[w])
        assert settled.shape == (8, 15, 3) and np.array_equal(settled, want[8 * w:8 * w + 8]) and np.array_equal(settled, old.window(G[w]))
        assert np.array_equal(now, G[w] if w == 0 else G[w, 2:])
    assert np.array_equal(s.flush(), want[8 * n_windows:])
    settled, now = DT.stream(G, 8)
    assert settled.tobytes() == want.tobytes() and len(now) == 8 * n_windows + 2


@pytest.mark.parametrize("stride", [5, 6, 7, 8])
@pytest.mark.parametrize("n_chunks,wpc", [(1, 1), (1, 2), (2, 12)])
def test_merge_dense_at_small_overlaps_is_merge_chunks(stride, n_chunks, wpc):
    from globalegomocap_amd.sequence import merge_dense, merge_chunks, merge_batches
    G = np.random.default_rng(10 * stride + wpc).normal(size=(n_chunks * wpc, 10, 15, 3))
    want = merge_chunks(G, n_chunks, 10 - stride)
    got = merge_dense(G, stride, n_chunks)
    assert got.shape == want.shape == (n_chunks, (wpc - 1) * stride + 10, 15, 3) and got.tobytes() == want.tobytes()
    assert merge_dense(G[:wpc], stride).tobytes() == np.asarray(merge_batches(G[:wpc], 10 - stride)).tobytes()


@pytest.mark.parametrize("stride", [1, 2, 3, 4, 5, 8, 10])
@pytest.mark.parametrize("n_chunks,wpc", [(1, 1), (2, 2), (2, 12)])
def test_merge_dense_is_the_twin(stride, n_chunks, wpc):
    from globalegomocap_amd.sequence import merge_dense
    G = np.random.default_rng(stride).normal(size=(n_chunks * wpc, 10, 45))
    want = DT.merge_dense(G, stride, n_chunks)
    assert merge_dense(G, stride, n_chunks).tobytes() == want.tobytes()
    # a chunk is merged on its own; the schedule's two streams are the same sums
    if n_chunks == 2:
        assert merge_dense(G[wpc:], stride).tobytes() == want[1].tobytes()
    if stride <= 8:
        settled, now = DT.stream(G[:wpc], stride)
        assert settled.tobytes() == want[0].tobytes()
        assert now.tobytes() == np.concatenate([G[0]] + [g[10 - stride:] for g in G[1:wpc]]).tobytes()


@pytest.mark.parametrize("stride", [1, 3, 8, 10])
@pytest.mark.parametrize("wpc", [1, 2, 12])
def test_coverage_counts(stride, wpc):
    from globalegomocap_amd.sequence import dense_counts
    count = dense_counts(wpc, stride)
    F = (wpc - 1) * stride + 10
    assert count.shape == (F,) and np.array_equal(count, DT.counts(wpc, stride)) and count.sum() == 10 * wpc
    # closed form: the windows w with w*stride <= f < w*stride + 10, 0 <= w < wpc
    f = np.arange(F)
    lo, hi = np.maximum(0, -(-(f - 9) // stride)), np.minimum(wpc - 1, f // stride)
    assert np.array_equal(count, hi - lo + 1) and count.min() >= 1 and count.max() == min(wpc, -(-10 // stride))
    assert np.array_equal(count, count[::-1])                             # the two ends of a stream ramp alike
    # a merge of all-ones windows is all ones whatever the counts, a merge of windows holding their own index is the mean index
    from globalegomocap_amd.sequence import merge_dense
    assert np.array_equal(merge_dense(np.ones((wpc, 10, 2)), stride), np.ones((F, 2)))
    idx = np.broadcast_to(np.arange(wpc, dtype=np.float64)[:, None, None], (wpc, 10, 1))
    np.testing.assert_allclose(merge_dense(idx, stride)[:, 0], (lo + hi) / 2, rtol=1e-15)


@pytest.mark.parametrize("stride", range(1, 9))
def test_pieces_end_where_a_window_completes(stride):
    from globalegomocap_amd import live
    n_total = 37
    for k in (1, 5, 8, 13, 10):
        at = 0
        while at < n_total:
            step = min(k, n_total - at)
            pieces = live._pieces(at, step, stride)
            assert pieces[0][0] == 0 and pieces[-1][1] == step and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
            for a, b in pieces:
                assert 1 <= b - a <= 8
                # no completing frame stride*w + 9 strictly inside a piece: it may only be the piece's last frame
                inside = [f for f in range(at + a, at + b - 1) if f >= 9 and (f - 9) % stride == 0]
                assert not inside, (stride, at, k, pieces)
            # and every completing frame in the push ends a piece
            ends = {at + b - 1 for _, b in pieces}
            assert all(f in ends for f in range(at, at + step) if f >= 9 and (f - 9) % stride == 0)
            at += step
    assert live._pieces(3, 13) == live._pieces(3, 13, 8)                  # the default is today's stride


def test_dropped_frames_against_the_twin():
    from globalegomocap_amd import live
    for k in range(1, 9):
        for n in range(0, 41):
            want = DT.dropped(n, k)
            assert live.dropped_frames(n, k) == want == ((n - 10) % k if n >= 10 else n), (n, k)
            if k == 8:
                assert live.dropped_frames(n) == want == LT.dropped(n) and DT.n_windows(n, 8) == LT.n_windows(n)
            # settled + flushed + dropped frames are the stream
            w = DT.n_windows(n, k)
            assert (w * k + (10 - k) if w else 0) + want == n


def test_argument_errors():
    from globalegomocap_amd import live, sequence
    from globalegomocap_amd.live import LiveOptimizer
    for bad in (0, 9, -1, 2.0, "8", None, True):
        with pytest.raises(ValueError, match="stride"):
            live.check_stride(bad)
        # the session refuses it first of all: no checkpoint is read, no device touched (the paths do not exist)
        with pytest.raises(ValueError, match="stride"):
            LiveOptimizer("/nonexistent/camera.json", "/nonexistent/g.pth", "/nonexistent/l.pth", stride=bad)
    assert [live.check_stride(k) for k in range(1, 9)] == list(range(1, 9)) and live.check_stride(np.int64(3)) == 3
    G = np.zeros((4, 10, 3))
    for bad in (0, 11, -2):
        with pytest.raises(ValueError, match="stride"):
            sequence.merge_dense(G, bad)
    with pytest.raises(ValueError, match="chunks"):
        sequence.merge_dense(G, 2, 3)
    with pytest.raises(ValueError, match="chunks"):
        sequence.merge_dense(G[:0], 2)
    p = live._parser()
    a = p.parse_args(["--slam", "t", "--heatmaps", "H", "--depths", "D", "--start", "0", "--end", "10", "--stride", "1", "--now"])
    assert a.stride == 1 and a.now is True
    d = p.parse_args(["--slam", "t", "--heatmaps", "H", "--depths", "D", "--start", "0", "--end", "10"])
    assert d.stride == 8 and d.now is False
    with pytest.raises(SystemExit):
        live._cli(["--slam", "t", "--heatmaps", "H", "--depths", "D", "--start", "0", "--end", "10", "--stride", "9"])


def test_every_symbol_of_the_dense_header_is_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(ROOT, "include", "gem_live_dense.h")).read()
    declared = set(re.findall(r"\b(gem_[a-z0-9_]+)\s*\(", header))
    assert declared == {"gem_live_window_at", "gem_live_emit_dense", "gem_merge_dense"} == set(_capi.DENSE_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name)
        n_args = len(re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header).group(1).split(","))
        assert len(_capi.DENSE_SIGNATURES[name][1]) == n_args, name
    assert not set(_capi.DENSE_SIGNATURES) & set(_capi.SIGNATURES)
    consts = dict(re.findall(r"#define (GEM_LIVE_[A-Z_]+) (\d+)", header))
    assert (int(consts["GEM_LIVE_DENSE_SLOTS"]), int(consts["GEM_LIVE_DENSE_DOUBLES"])) == (_capi.LIVE_DENSE_SLOTS, _capi.LIVE_DENSE_DOUBLES)
    # the documented layout adds up: 16 scalars, the counts, the filter's two rows, the sums and the estimated frames of every slot
    assert _capi.LIVE_DENSE_DOUBLES == 16 + _capi.LIVE_DENSE_SLOTS + 2 * 48 + 2 * _capi.LIVE_DENSE_SLOTS * 48
    assert '#include "gem_live_dense.h"' in open(os.path.join(ROOT, "include", "gem_hip.h")).read()
