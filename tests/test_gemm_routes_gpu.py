"""Every kernel the two GEMM dispatch functions can reach, one layer at a time, against the float64 twin (gemm_twin.py).

Each case of gemm_twin.CASES goes through gem_gemm_debug_run (launch_gemm or gemm_bf16a, the library's own load-time weight
images, its own reduce pass where the consumer takes slabs) and must
  * report exactly the kernels the planners' rules name for it (a case never quietly tests a neighbouring route),
  * leave every guard untouched: the 256 rows behind C, C's rows past a device row count, while A's spare rows and A's rows past
    the device row count are NaN (nothing of them may reach a live element),
  * exact variant (integers |.| <= 4, masks +-1): EQUAL the twin, fp32 or bf16 bits, in all three precision modes -- every
    partial sum is an integer below 2^24, so no order of accumulation and no hi/lo split can change it;
  * rounded variant (standard normal, K <= 256): stay within gemm_twin.bound_out, the derived fp32 accumulation bound; bf16
    outputs equal bf16(twin) bit for bit except where the twin lies within that bound of a rounding boundary (one of the two
    neighbours then, and at most 5 % of a case: gemm_twin.rounded_scale says which cases have this variant and why).
"""
import numpy as np
import pytest

import gemm_twin as G

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC17FC1          # a NaN as fp32 and as either bf16 half


class Rig:
    def __init__(self):
        import torch
        from globalegomocap_amd.engine import WindowEngine
        from globalegomocap_amd.vae import VAEShape
        if not torch.cuda.is_available():
            pytest.fail("gpu tests need a HIP device")
        self.torch = torch
        self.eng = WindowEngine(VAEShape(latent_dim=64, hidden=(16, 32), seq_len=10), max_windows=640)
        self.dev = self.eng.device
        self.n_cu = torch.cuda.get_device_properties(self.dev).multi_processor_count

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    assert r.n_cu == G.N_CU, "the case table is laid out for %d compute units" % G.N_CU
    yield r
    r.close()


def run_case(rig, k, kind):
    torch, eng = rig.torch, rig.eng
    plan = G.plan_case(k)
    A, w, bias, aux, rmap = G.case_inputs(k, kind)
    m = G.live_rows(k)
    a_rows = A.shape[0]
    tw = G.gemm_twin(A, w, bias, k.epi, m, k.T, aux, rmap, G.case_mode(k))

    eng.set_precision("bf16" if k.route == "a" else k.precision)
    dA = torch.full((a_rows + G.GUARD_ROWS, k.K), float("nan"), device=rig.dev, dtype=torch.float32)
    live_a = a_rows if rmap is not None else m           # without a row map the rows past the device count are dead as well
    dA[:live_a] = torch.from_numpy(A[:live_a]).to(rig.dev)
    rows_total = k.M + G.GUARD_ROWS
    dC = torch.full((rows_total * k.N,), SENTINEL, device=rig.dev, dtype=torch.int32)
    d_aux = torch.from_numpy(aux).to(rig.dev) if aux is not None else None
    d_map = torch.from_numpy(rmap).to(rig.dev) if rmap is not None else None
    d_rows = None
    if k.rows is not None:
        d_rows = torch.tensor([k.rows // k.T, k.rows] if k.taps == 3 else [k.rows, k.rows * k.T], device=rig.dev, dtype=torch.int32)
    layer = eng.gemm_debug_layer(w, bias)
    try:
        names, info = eng.gemm_debug_run(layer, dA[:a_rows], dC, k.M, k.epi, route=1 if k.route == "a" else 0, T=k.T, aux=d_aux,
                                         rows=d_rows, row_map=d_map, defer=k.defer, out_bf16=k.out_bf16, allow_split=k.allow_split,
                                         family=k.family)
    finally:
        eng.gemm_debug_layer_free(layer)
    raw = dC.cpu().numpy()

    # ---- the route
    assert sorted(names) == plan.kernels, (names, plan)
    assert any(k.want in n for n in names), (k.want, names)
    assert info[0] == (plan.n_slices if plan.deferred else 0), (info, plan)
    if plan.deferred:
        assert info[1] == plan.dyn_W, (info, plan)
    assert bool(info[2]) == plan.c_bf16, (info, plan)

    # ---- guards
    if plan.c_bf16:
        half = rows_total * k.N // 2          # the bf16 matrix fills the first half of the buffer
        assert np.all(raw[half:] == np.int32(SENTINEL)), "wrote behind the bf16 output"
        bits = raw[:half].view(np.uint16).reshape(rows_total, k.N)
        assert np.all(bits[m:] == 0x7FC1), "rows past the live rows were written"
        dev_bits = bits[:m]
        dev = G.bf16_widen(dev_bits)
    else:
        mat = raw.reshape(rows_total, k.N)
        assert np.all(mat[m:] == np.int32(SENTINEL)), "rows past the live rows were written"
        dev = mat[:m].view(np.float32)
    assert not np.isnan(dev).any(), "NaN (a guard row or an unwritten element) in a live row"

    # ---- the numbers
    if kind == "exact":
        assert np.array_equal(tw.pre.astype(np.float32).astype(np.float64), tw.pre)
        if plan.c_bf16:
            assert np.array_equal(dev_bits, G.bf16_bits(tw.out32)), "max |dev - twin| = %g" % np.abs(dev - tw.out32).max()
        else:
            assert np.array_equal(dev, tw.out32), "max |dev - twin| = %g at %s" % (
                np.abs(dev - tw.out32).max(), np.unravel_index(np.abs(dev - tw.out32).argmax(), dev.shape))
        return
    bnd = G.bound_out(tw, k.epi, aux)
    if plan.c_bf16:
        unsure = G.bf16_uncertain(tw.out, bnd)
        want = G.bf16_bits(tw.out.astype(np.float32))
        lo, hi = G.bf16_widen(G.bf16_bits((tw.out - bnd).astype(np.float32))), G.bf16_widen(G.bf16_bits((tw.out + bnd).astype(np.float32)))
        print("ROUTE", k.id, kind, "uncertain share %.4f" % unsure.mean(), "bits differing %d" % int((dev_bits != want).sum()))
        assert unsure.mean() <= 0.05
        assert np.array_equal(dev_bits[~unsure], want[~unsure])
        assert np.all((dev >= lo) & (dev <= hi))
    else:
        ratio = np.abs(dev.astype(np.float64) - tw.out) / np.maximum(bnd, np.finfo(np.float64).tiny)
        print("ROUTE", k.id, kind, "worst |dev - twin| / bound = %.4f" % ratio.max())
        assert np.all(np.abs(dev.astype(np.float64) - tw.out) <= bnd)


@pytest.mark.parametrize("k", G.CASES, ids=[k.id for k in G.CASES])
def test_route_exact(rig, k):
    run_case(rig, k, "exact")


ROUNDED = [k for k in G.CASES if G.rounded_scale(k) is not None]


@pytest.mark.parametrize("k", ROUNDED, ids=[k.id for k in ROUNDED])
def test_route_rounded(rig, k):
    run_case(rig, k, "rounded")


def test_bad_arguments_are_error_returns(rig):
    """Every check of gem_gemm_debug_run on its error return; nothing is launched."""
    from globalegomocap_amd._capi import GemError
    torch, eng = rig.torch, rig.eng
    eng.set_precision("f32")
    lin = eng.gemm_debug_layer(np.zeros((1, 64, 64), np.float32), np.zeros(64, np.float32))
    conv = eng.gemm_debug_layer(np.zeros((3, 64, 96), np.float32), np.zeros(64, np.float32))
    A = torch.zeros(64, 96, device=rig.dev)
    Cb = torch.zeros(64 * 64, device=rig.dev)
    i32 = lambda v: torch.tensor(v, device=rig.dev, dtype=torch.int32)
    bad = [
        dict(layer=lin, M=20, epi=4),                                         # no such epilogue
        dict(layer=lin, M=20, epi=G.EPI_MASK, aux=Cb),                        # the mask belongs to convs
        dict(layer=conv, M=20, epi=G.EPI_MASK, T=10),                         # ... and needs aux
        dict(layer=lin, M=0, epi=0),
        dict(layer=lin, M=640 * 10 + 1, epi=0),                               # more rows than max_windows * seq_len
        dict(layer=conv, M=25, epi=0, T=10),                                  # M % T
        dict(layer=conv, M=20, epi=0, T=10, row_map=i32(list(range(20)))),    # row maps gather linear layers only
        dict(layer=lin, M=20, epi=0, row_map=i32([0] * 19 + [64])),           # entry outside A
        dict(layer=lin, M=20, epi=0, row_map=i32([-1] + [0] * 19)),
        dict(layer=lin, M=20, epi=0, rows=i32([21, 21])),                     # device row count above M
        dict(layer=lin, M=20, epi=0, rows=i32([0, 0])),
        dict(layer=conv, M=20, epi=0, T=10, rows=i32([2, 19])),               # second entry is not m * T
        dict(layer=conv, M=20, epi=0, T=5, route=1),                          # gemm_bf16a reads the handle's window length
        dict(layer=conv, M=20, epi=0, T=10, route=1),                         # K = 96 is not padded for the bf16 kernels
        dict(layer=lin, M=20, epi=0, out_bf16=True),                          # gemm_bf16a's options on launch_gemm
        dict(layer=lin, M=20, epi=0, route=1, defer=True),                    # slabs without allow_split
        dict(layer=lin, M=20, epi=0, route=2),
        dict(layer=lin, M=20, epi=0, family=4),
        dict(layer=lin, M=65, epi=0),                                         # A has 64 rows
    ]
    try:
        for kw in bad:
            kw = dict(kw)
            layer = kw.pop("layer")
            with pytest.raises(GemError, match="gem_gemm_debug_run"):
                eng.gemm_debug_run(layer, A, Cb, kw.pop("M"), kw.pop("epi"), **kw)
        assert not Cb.any().item()                                            # nothing ran
        eng.gemm_debug_layer_free(conv)
        with pytest.raises(GemError, match="not a layer of this handle"):
            eng.gemm_debug_run(conv, A, Cb, 20, 0, T=10)
        with pytest.raises(GemError, match="not a layer of this handle"):
            eng.gemm_debug_layer_free(conv)
        with pytest.raises(GemError, match="gem_gemm_debug_layer_create"):
            eng.gemm_debug_layer(np.zeros((2, 64, 64), np.float32), np.zeros(64, np.float32))
        with pytest.raises(GemError, match="gem_gemm_debug_layer_create"):
            eng.gemm_debug_layer(np.zeros((1, 64, 48), np.float32), np.zeros(64, np.float32))
    finally:
        eng.gemm_debug_layer_free(lin)
