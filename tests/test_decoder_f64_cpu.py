"""The float64 decoder twin (tests/decoder_f64.py) against the fp32 oracle and against its own central differences; what fp32
needs on the case table of tests/test_decoder_tails_gpu.py; the conditions on that table's inputs; the table's reach.

What fp32 needs: the fp32 numpy oracle (fp32 storage, fp32 products) against the twin, largest over the 25 fp32 cases
    pose, of max|X| per window                      2.24e-7     device allowance (4 x)  9.0e-7
    pre-activations, of the max per layer, window   9.22e-7     (the margin below is 8 x the case's own figure)
    dE/dz, of max|dE/dz| per window                 4.03e-6     device allowance (4 x)  1.6e-5
and, over the 12 stage cases, the energy at z0 = latent_from_pose(pose, eps) under W_ALL
    energy, of sum_k |w_k part_k| per window        6.34e-7     device allowance (4 x)  2.5e-6
No LeakyReLU mask of the oracle differs from the twin's in any case.  (The energy is measured against the sum of the terms'
magnitudes: relative to |E| itself two stage cases showed 2.9e-5 and 6.2e-5, from one window each whose negative reprojection
term cancels the other four to E = 0.06 out of magnitudes summing to 6 -- cancellation in the sum, not error in the decoder.)
decoder_f64.MEASURED records the figures; the tests below re-measure them and accept 0.5 .. 1.25 of the record (another BLAS
may sum an fp32 dot product in another order).

LeakyReLU margin.  The condition: no pre-activation of any window lies within 8 x the case's own fp32 pre-activation deviation of
zero, relative to the largest of its layer and window.  Every case's seed is the first from 0 at which (a) the twin's smallest
relative pre-activation is at least decoder_f64.MARGIN = 1.5e-5 -- 16 x the largest deviation on the table, a figure of the
float64 twin alone, so the choice does not move with the BLAS; the cases then keep 22 x .. 310 x their own deviation -- and (b)
every pair of the float64 poses keeps 2e-4 texel from a texel line (twice the distance at which the device test may leave a
window out).  The widest chains needed up to 22 seeds."""
import numpy as np
import pytest

import decoder_f64 as D
import gemm_twin as G
from oracle import np_oracle as O

_id = lambda c: "%s-T%d-B%d" % ("x".join(str(h) for h in c.hidden), c.T, c.B)
_DEV = {}


def _deviations(case):
    if case not in _DEV:
        _DEV[case] = D.oracle_deviations(D.make_inputs(case))
    return _DEV[case]


@pytest.mark.parametrize("case", D.FP32_CASES, ids=_id)
def test_oracle_within_the_measured_deviation_and_the_inputs_keep_their_margin(case):
    dev = _deviations(case)
    print("DECODER_F64 " + _id(case), dev)
    assert dev["flips"] == 0
    for k in ("pose", "pre", "dz"):
        assert dev[k] <= 1e-5, (k, dev[k], "fp32 should not need this much: find out why before any gate moves")
        assert dev[k] <= 1.25 * D.MEASURED[k], (k, dev[k])
    assert D.margin_condition(dev) and D.seed_is_good(dev) and D.inputs_are_good(D.make_inputs(case)), dev
    assert D.MARGIN >= 16.0 * dev["pre"], dev
    for seed in range(case.seed):
        assert not D.inputs_are_good(D.make_inputs(case, seed)), ("an earlier seed meets the conditions", seed)


def test_the_recorded_measurement_is_what_the_table_gives():
    for k in ("pose", "pre", "dz"):
        worst = max(_deviations(c)[k] for c in D.FP32_CASES)
        assert 0.5 * D.MEASURED[k] <= worst <= 1.25 * D.MEASURED[k], (k, worst, D.MEASURED[k])
    worst = max(D.oracle_energy_deviation(D.make_inputs(c)) for c in D.STAGE_CASES)
    assert 0.5 * D.MEASURED["energy"] <= worst <= 1.25 * D.MEASURED["energy"], worst
    assert D.GATES == {k: 4.0 * v for k, v in D.MEASURED.items()}


@pytest.mark.parametrize("hidden,T", [((64,), 3), ((64, 128), 10), (D.CHAINS_2[5], 16), ((64, 512, 512), 10), (D.CHAINS_4[5], 3)],
                         ids=lambda v: "x".join(str(h) for h in v) if isinstance(v, tuple) else "T%d" % v)
def test_adjoint_against_central_differences(hidden, T):
    """The decoder is piecewise linear in z: away from a kink central differences are exact up to rounding."""
    inp = D.make_inputs(D.Case(hidden, T, 2, 0, (None,)))
    twin, z = inp["twin"], inp["z"].astype(np.float64)
    rng = np.random.default_rng(5)
    dec = twin.decode(z)
    c = rng.normal(size=dec.X.shape)
    dz = twin.adjoint(c, dec.pre)
    h = 1e-7
    for _ in range(6):
        d = rng.normal(size=z.shape)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        up, dn = twin.decode(z + h * d), twin.decode(z - h * d)
        assert all(np.array_equal(a > 0, b > 0) for a, b in zip(up.pre, dn.pre)), "the step crosses a LeakyReLU kink"
        num = ((up.X - dn.X) * c).reshape(2, -1).sum(axis=1) / (2 * h)
        ana = (dz * d).sum(axis=1)
        assert np.abs(num - ana).max() <= 1e-6 * np.linalg.norm(dz, axis=1).max(), (num, ana)


def test_twin_reproduces_the_oracle_layer_by_layer_on_the_shipped_shape():
    """Independent of the table's figures: activations, pose and adjoint of the oracle on the default widths, at 2e-6."""
    inp = D.make_inputs(D.Case(D.CHAINS_2[4], 10, 3, 7, (None,)))
    Xo, acts = O.decode(inp["vae"], inp["z"], keep=True)
    for a, p in zip(acts, inp["dec"].pre):
        assert D.relative_deviation(a, np.where(p > 0, p, D.SLOPE * p)).max() <= 2e-6
    assert D.relative_deviation(Xo, inp["dec"].X).max() <= 2e-6
    dX = np.random.default_rng(1).normal(size=Xo.shape).astype(np.float32)
    assert D.relative_deviation(O.decode_backward(inp["vae"], dX, acts), inp["twin"].adjoint(dX, inp["dec"].pre)).max() <= 2e-5


def test_the_cases_reach_every_instantiation():
    names = {D.predict(c.hidden, c.T, c.B, w).kernel for c in D.FP32_CASES for w in c.waves}
    want = {"TailTiles<2>::decoder_tail_kernel<%d, %d>" % (nl, w) for nl in range(1, 7) for w in (8, 4)}
    want |= {"TailTiles<4>::decoder_tail_kernel<%d, 8>" % nl for nl in range(1, 7)}
    assert len(want) == 18 and names >= want | {None}, want - names
    # the tile walk's switches (L.N > 16 W, L.N > 32 W) from both sides, in every instantiation family: layer widths (forward N
    # and adjoint K) met under <2>::<., 8>, <2>::<., 4> and <4>::<., 8>
    widths = {}
    for c in D.FP32_CASES:
        for w in c.waves:
            t = D.predict(c.hidden, c.T, c.B, w)
            if t.kernel:
                widths.setdefault((t.maxnt, t.waves), set()).update(v for kn in D.decoder_layers(c.hidden)[t.start:] for v in kn)
    assert widths[(2, 8)] == {64, 128, 256} and widths[(2, 4)] == {64, 128, 256} and widths[(4, 8)] == {64, 128, 256, 512}, widths
    # a case that asks for the 4-wave shape gets it
    assert all(D.predict(c.hidden, c.T, c.B, "4").waves == 4 for c in D.FP32_CASES if "4" in c.waves)
    # several windows per workgroup and the window lengths, per chain length
    reach = {(c.T, D.predict(c.hidden, c.T, c.B).NL) for c in D.FP32_CASES}
    assert reach >= {(T, nl) for T in (5, 8) for nl in (1, 3, 6)} | {(T, nl) for T in (16, 3) for nl in (2, 6)}
    assert all(c.B % (16 // c.T) for c in D.FP32_CASES if c.T in (5, 8)), "the last workgroup must be ragged"
    seven = D.predict(D.SEVEN_BLOCKS, 10, 4)
    assert seven.start == 2 and not seven.front and seven.NL == 6
    assert D.predict(D.REFUSED, 10, 4) == D.Tail(-1, 0, 0, 0, None, False, False)
    # the stages: every chain length under both tile bounds, and the front product leaves split-K slabs to the tail
    stages = set()
    for c in D.STAGE_CASES:
        t = D.predict(c.hidden, c.T, c.B)
        assert t.front and c.B * c.T >= 48
        route = G.plan_launch_gemm("f32", 1, c.T * D.decoder_layers(c.hidden)[0][1], D.pad64(c.latent), G.EPI_BIAS_LRELU, c.B, rows=True,
                                   defer=True, family=0)
        assert route.deferred and route.n_slices > 1, (c, route)
        stages.add((t.maxnt, t.NL))
    assert stages == {(m, nl) for m in (2, 4) for nl in range(1, 7)}
    # the bf16 tail: chain lengths 1 .. 6 at T = 10 and T = 5
    for T in (10, 5):
        got = {D.predict(c.hidden, c.T, c.B).NL for c in D.BF16_CASES if c.T == T and D.predict(c.hidden, c.T, c.B).bf16}
        assert got == set(range(1, 7)), (T, got)
    assert all(D.predict(c.hidden, c.T, c.B).bf16 for c in D.BF16_CASES)
    # (the six-layer TailTiles<2> chain itself is refused by the bf16 planner at T = 10: why another chain stands in)
    assert not D.predict(D.CHAINS_2[5], 10, 11).bf16
