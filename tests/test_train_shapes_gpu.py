"""The VAE training step (gem_trainer_step, csrc/train.hip) held to float64 over the shapes it accepts: window lengths 3 .. 16,
one to seven blocks, latent widths that are no multiple of 4 / 64, and the row counts at which the step changes kernels --
every route asserted through gem_trainer_route before the case runs, so that the table cannot drift from the dispatch.

Reference: tests/train_f64.py, which adopts the device's LeakyReLU signs (mask = block output > 0): both sides differentiate the
same piecewise-linear function, and the allowances are rounding-level -- four times what the fp32 CPU port needs against the
same reference (tests/test_train_f64_cpu.py, train_cases.PORT_*); the factor covers summation orders the port does not have
(slabs, strips, MFMA accumulation).  Per check, the allowance and [the largest deviation observed on an MI355X over all cases, both
modes and both steps, as a share of that allowance]:

  losses (loss, recon, KLD)        1e-6 relative                                                                    [0.30]
  block outputs, final pose        4e-5 max(1, max|ref|)                                                            [0.27]
  adopted signs float64 disagrees  each at |v_ref| <= 4e-5 max(1, max|ref|) [0.016]; share <= 1e-4 of the activations, a
                                   condition, not a measurement [1.7e-5 of the activations]
  gradients in the arena           8e-5 max|ref_k| + 8e-7 gmax; ".0.bias" tensors (exact zero gradient) 6e-6 gmax    [0.33]
  first moments, both modes        (1 - b1) x the gradient allowance + one fp32 ulp of m + 2^-24 |g| (b1, 1 - b1 in fp32)  [0.33]
  second moments                   (1 - b2) (2 |g| x allowance + allowance^2) + one ulp of v + 2^-24 g^2             [0.49]
  running statistics               4e-7 max(1, max|ref|)                                                            [0.22]
  parameters                       against float64 Adam on the device's OWN moments: 2^-22 |p0| + 2^-19 lr           [0.25]
  arenas                           pack_arena(unpack_arena(x)) == x bitwise: nothing is written into padding

After the second step the float64 gradient is taken at the device's own parameters after the first, and the moments are checked
against b m1_device + (1 - b) g2: the refreshed adjoint images, the step count in both bias corrections, the moment carry-over.
test_zz_record prints the largest deviation of every check as a share of its allowance (pytest -s)."""
import numpy as np
import pytest

import train_f64 as F64
from train_cases import (CASES, KLD_WEIGHT, LR, WEIGHT_DECAY, PORT_A, PORT_B, PORT_B0, PORT_C, PORT_LOSS, PORT_STAT, direct_batches,
                         inputs, shape_of)
from globalegomocap_amd import vae as vae_schema
from helpers import FULL

pytestmark = pytest.mark.gpu

A, B_, B0, C_, LOSS, STAT = 4 * PORT_A, 4 * PORT_B, 4 * PORT_B0, 4 * PORT_C, 4 * PORT_LOSS, 4 * PORT_STAT
B1, B2 = 0.9, 0.999
LINEAR_WEIGHTS = ("fc_mu.weight", "fc_var.weight", "decoder_input.weight")
RECORD = {}          # check -> largest deviation / allowance seen


def _note(check, share):
    RECORD[check] = max(RECORD.get(check, 0.0), float(share))


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def expected_route(case, B, n_cu):
    """What the table says the case reaches, as the fields of VAETrainer.route that must hold (n_cu-dependent ones only on the
    256 compute units they were written for)."""
    rows = B * case.T
    want = {"bn_forward": 0 if rows <= 2560 else 2, "bn_backward": 1 if rows <= 1024 else 2,
            "linear_weight_grad_slabs": 1 if B <= 256 else 2, "n_encoder": len(case.hidden), "n_decoder": len(case.hidden) + 1}
    if B > 64:
        want.update(strip_decoder_input=0, strip_fc=0, encoder_top_dz=0)
    name = case.name
    if name == "t5-h64-d5-b33":          # five n tiles: no even strip for decoder_input; fc (2 Dp / 64 = 2 tiles) stays fused
        want.update(strip_decoder_input=0, strip_fc=2, encoder_top_dz=1)
    elif name in ("t3-b2", "t8-7x8-d33-b64", "t16-b64", "t6-full-b9"):
        want.update(encoder_top_dz=1)
    elif name == "t16-direct":
        want.update(bwd_data_slabs_fc=1)
    elif name == "t16-direct-ragged":
        want.update(bwd_data_slabs_fc=-1)
    return want


def check_route(tr, case, B):
    n_cu = _n_cu()
    r = tr.route(B)
    assert r["n_cu"] == n_cu
    for k, v in expected_route(case, B, n_cu).items():
        assert r[k] == v, (case.name, k, r)
    if B <= 64 and case.name != "t5-h64-d5-b33":
        assert r["strip_decoder_input"] > 0 and r["strip_fc"] > 0, r
    if case.name.startswith("t6-full") and n_cu == 256:
        # encoder.4 (K = 256 -> N = 512): 2 x 16 tiles at 54 rows (eight waves), 17 x 16 = 272 tiles at 540 rows (four waves);
        # decoder.0 (K = 512 -> N = 256): eight waves at both
        assert r["conv_waves"][4] == ((8, 8) if B == 9 else (4, 8)), r
        assert r["conv_waves"][5][0] == 8 and r["conv_waves"][0] == (2, 0), r
    if case.name == "t8-7x8-d33-b64":
        assert len(r["conv_waves"]) == 15
    return r


def _tensor_allow(k, ref, gmax):
    return B0 * gmax if k.endswith(".0.bias") else A * float(np.abs(ref).max()) + B_ * gmax


_REF_CACHE = {}


def _reference(key, sd, case, poses, eps, masks):
    """The float64 step at `sd` with the device's signs; the first step's is shared by the two modes (same forward, same signs)."""
    hit = _REF_CACHE.get(key)
    if hit is not None and all(np.array_equal(hit[0][k], masks[k]) for k in masks):
        return hit[1]
    r = F64.forward_backward(sd, case.T, poses, eps, KLD_WEIGHT, case.form, masks)
    if key is not None:
        _REF_CACHE.clear()
        _REF_CACHE[key] = (masks, r)
    return r


def check_step(tr, case, shape, sd_before, m_before, v_before, step, poses, eps, losses, update, tag):
    """Everything a step leaves behind against float64 at `sd_before` (the device's own state before the step)."""
    from globalegomocap_amd.vae_train import pack_arena, unpack_arena
    enc_o, dec_o = tr.layer_outputs()
    enc_names, dec_names = F64.block_names(sd_before)
    outs = dict(zip(enc_names + dec_names, enc_o + dec_o[:-1]))
    masks = {k: v > 0 for k, v in outs.items()}
    ref = _reference((case.name, len(poses)) if step == 1 and update else None, sd_before, case, poses, eps, masks)
    # losses
    for x, y in zip(losses, ref["losses"]):
        _note("losses", abs(x - y) / abs(y) / LOSS)
        assert abs(x - y) <= LOSS * abs(y), (tag, losses, ref["losses"])
    # block outputs, the final pose, and the adopted signs
    n_act = n_bad = 0
    for k, o in list(outs.items()) + [("pose", dec_o[-1])]:
        r = ref["pose"] if k == "pose" else ref["out"][k]
        lim = C_ * max(1.0, float(np.abs(r).max()))
        d = float(np.abs(o - r).max())
        _note("outputs", d / lim)
        assert d <= lim, (tag, k, d, lim)
        if k != "pose":
            pre = ref["pre"][k]
            bad = (pre > 0) != masks[k]
            n_act += bad.size
            n_bad += int(bad.sum())
            if bad.any():
                lim = C_ * max(1.0, float(np.abs(pre).max()))
                _note("adopted signs", float(np.abs(pre[bad]).max()) / lim)
                assert np.abs(pre[bad]).max() <= lim, (tag, k, float(np.abs(pre[bad]).max()))
    _note("sign share", n_bad / n_act / 1e-4)
    assert n_bad <= 1e-4 * n_act, (tag, n_bad, n_act)
    # gradients left in the arena
    gmax = max(float(np.abs(v).max()) for v in ref["grads"].values())
    grads = tr.gradients()
    assert set(grads) == set(ref["grads"]) - (set(LINEAR_WEIGHTS) if update == 2 else set()), tag
    for k, g in grads.items():
        lim = _tensor_allow(k, ref["grads"][k], gmax)
        d = float(np.abs(np.asarray(g, np.float64) - ref["grads"][k]).max())
        _note("gradients", d / lim)
        assert d <= lim, (tag, "gradient", k, d, lim)
    # running statistics
    sd_after = tr.state_dict()
    for k, r in ref["running"].items():
        lim = STAT * max(1.0, float(np.abs(r).max()))
        d = float(np.abs(np.asarray(sd_after[k], np.float64) - r).max())
        _note("running statistics", d / lim)
        assert d <= lim, (tag, k, d, lim)
    if not update:
        return sd_after, m_before, v_before
    # moments of ALL tensors (this is what sees the linear layers' weight gradients in the loop mode), then the parameters
    opt = tr.optimizer_state()
    assert opt["step"] == step
    for k, g in ref["grads"].items():
        p0 = np.asarray(sd_before[k], np.float64)
        gg = g + WEIGHT_DECAY * p0
        lim_g = _tensor_allow(k, g, gmax)
        m = np.asarray(opt["exp_avg"][k], np.float64)
        v = np.asarray(opt["exp_avg_sq"][k], np.float64)
        m_ref = B1 * m_before[k] + (1 - B1) * gg
        v_ref = B2 * v_before[k] + (1 - B2) * gg * gg
        lim_m = (1 - B1) * lim_g + np.spacing(np.abs(m).astype(np.float32)).astype(np.float64) + 2.0 ** -24 * np.abs(gg)
        lim_v = (1 - B2) * (2 * np.abs(gg) * lim_g + lim_g ** 2) + np.spacing(np.abs(v).astype(np.float32)).astype(np.float64) + 2.0 ** -24 * gg * gg
        _note("first moments", float((np.abs(m - m_ref) / lim_m).max()))
        _note("second moments", float((np.abs(v - v_ref) / lim_v).max()))
        assert (np.abs(m - m_ref) <= lim_m).all(), (tag, "exp_avg", k, float((np.abs(m - m_ref) / lim_m).max()))
        assert (np.abs(v - v_ref) <= lim_v).all(), (tag, "exp_avg_sq", k, float((np.abs(v - v_ref) / lim_v).max()))
        p_ref = F64.adam_apply(p0, m, v, step, LR)
        lim_p = 2.0 ** -22 * np.abs(p0) + 2.0 ** -19 * LR
        dp = np.abs(np.asarray(sd_after[k], np.float64) - p_ref)
        _note("parameters", float((dp / lim_p).max()))
        assert (dp <= lim_p).all(), (tag, "parameter", k, float((dp / lim_p).max()))
    # nothing in the padding of the three arenas
    S = tr._down(2)
    for what in (0, 3, 4):
        x = tr._down(what)
        full = unpack_arena(x, shape, S)
        np.testing.assert_array_equal(pack_arena(full, shape)[0].view(np.uint32), x.view(np.uint32), err_msg="%s arena %d" % (tag, what))
    return sd_after, {k: np.asarray(v, np.float64) for k, v in opt["exp_avg"].items()}, {k: np.asarray(v, np.float64) for k, v in opt["exp_avg_sq"].items()}


def run_case(case, B):
    from globalegomocap_amd.vae_train import VAETrainer
    shape, init, poses, eps = inputs(case, steps=2, batch=B)
    for update in (1, 2):
        tr = VAETrainer(shape, batch_size=B, lr=LR, weight_decay=WEIGHT_DECAY, state_dict=init, recon_reduction=case.form)
        try:
            check_route(tr, case, B)
            sd = dict(tr.state_dict())
            zeros = {k: np.zeros(np.shape(v)) for k, v in sd.items()}
            m, v = zeros, zeros
            for s in range(2):
                losses = tr.step(poses[s], KLD_WEIGHT, eps=eps[s], keep_gradients=update == 1)
                sd, m, v = check_step(tr, case, shape, sd, m, v, s + 1, poses[s], eps[s], losses, update, "%s update %d step %d" % (case.name, update, s + 1))
        finally:
            tr.close()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_training_step_against_float64(case):
    B = case.B
    if case.name.startswith("t16-direct"):
        B = direct_batches(_n_cu())[0 if case.name == "t16-direct" else 1]
    run_case(case, B)


def test_gradient_only_step_leaves_parameters_and_moments_alone():
    """update = 0: gradients as in the other modes, parameters and both moments bitwise untouched, num_batches_tracked advanced
    (a train-mode forward), the Adam step count not."""
    from globalegomocap_amd.vae_train import VAETrainer
    case = CASES[1]
    shape, init, poses, eps = inputs(case, steps=2)
    tr = VAETrainer(shape, batch_size=case.B, lr=LR, weight_decay=WEIGHT_DECAY, state_dict=init, recon_reduction=case.form)
    try:
        tr.step(poses[0], KLD_WEIGHT, eps=eps[0])          # (moments that are not zero)
        before = [tr._down(w).copy() for w in (0, 3, 4)]
        sd = dict(tr.state_dict())
        losses = tr.step(poses[1], KLD_WEIGHT, eps=eps[1], update=False)
        check_step(tr, case, shape, sd, None, None, 1, poses[1], eps[1], losses, 0, "update 0")
        for w, x in zip((0, 3, 4), before):
            np.testing.assert_array_equal(tr._down(w).view(np.uint32), x.view(np.uint32))
        assert int(tr.state_dict()["encoder.0.1.num_batches_tracked"]) == 2 and tr.steps == 1
    finally:
        tr.close()


def test_eight_blocks_are_refused_and_the_next_trainer_works():
    """n_hidden = 8 would need 17 entries of the weight-gradient table's 16: gem_trainer_create says so and leaves nothing behind."""
    from globalegomocap_amd import _capi
    from globalegomocap_amd.vae_train import VAETrainer
    with pytest.raises(_capi.GemError, match="more conv layers"):
        VAETrainer(vae_schema.VAEShape(latent_dim=33, seq_len=8, hidden=(8,) * 8), batch_size=4)
    run_case(CASES[0], CASES[0].B)


def test_full_size_trainer_steps_at_a_batch_that_is_no_multiple_of_64():
    """The shipped network at batch 400 on 256 compute units: the fc layer's backward-data product runs without slabs
    (7 x 80 tiles >= 2 n_cu) and its 448 padded rows pass through the slab buffer (this batch used to be refused).  A gradient-only
    step and a training-loop step from the same parameters: finite, the same losses, and -- the same kernels on the same inputs --
    the same bits in every gradient the loop mode leaves."""
    from globalegomocap_amd import synth
    from globalegomocap_amd.vae_train import VAETrainer, initial_state_dict
    batch = 400
    poses = synth.make_training_windows(batch, FULL.seq_len, 6)
    eps = np.random.default_rng(6).standard_normal((batch, FULL.latent_dim)).astype(np.float32)
    tr = VAETrainer(FULL, batch_size=batch, lr=LR, weight_decay=1e-5, state_dict=initial_state_dict(FULL, 9))
    try:
        r = tr.route(batch)
        if r["n_cu"] == 256:
            assert r["bwd_data_slabs_fc"] == -1 and r["bwd_data_slabs_decoder_input"] == 3, r
        l0 = tr.step(poses, 0.01, eps=eps, update=False)
        g0 = tr.gradients()
        l2 = tr.step(poses, 0.01, eps=eps, keep_gradients=False)
        g2 = tr.gradients()
    finally:
        tr.close()
    assert np.isfinite(l0).all() and l0 == l2
    assert set(g0) - set(g2) == set(LINEAR_WEIGHTS)
    for k, v in g0.items():
        assert np.isfinite(v).all() and float(np.abs(v).max()) > 0, k
        if k in g2:
            np.testing.assert_array_equal(g2[k], v, err_msg=k)


def test_zz_record(capsys):
    """Prints the largest deviation of every check above as a share of its allowance (needs the cases to have run: pytest -s)."""
    with capsys.disabled():
        print("\nlargest deviation / allowance per check: " + ", ".join("%s %.3g" % kv for kv in sorted(RECORD.items())))
    assert all(v <= 1.0 for v in RECORD.values())
