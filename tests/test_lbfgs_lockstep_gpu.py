"""lbfgs_advance_kernel against its twin, lock-step, through gem_lbfgs_debug_* (harness: lbfgs_lockstep.py).

Every round the objectives are evaluated in torch float32 on the card at the KERNEL's trial points and the same (f, g) goes to
the kernel and to one twin per window (lbfgs_twin.PairwiseTwin, pinned to torch.optim.LBFGS by test_lbfgs_lockstep_cpu.py).
Asserted per round and window: phase, n_iter, evals, ls_iter, hist_count, low, high, insuf equal; loss equal; t, gtd, H_diag,
x + t d and the trial point within the allowance; padding columns zero; the duplicate window bitwise window 0; a finished window
frozen; the slot table a permutation of [0, count) over the live windows.

Allowance (relative; vectors to max|trial|): MARGIN * spread + FLOOR, capped at 2e-4, where `spread` is measured per case and
quantity on the CPU in the same run: the twin against the twin with float64 dot products (what another summation order costs).
FLOOR = 8 * 2^-24.  MARGIN = 16 was set from the ratios deviation / max(spread, FLOOR) of the first run on an MI355X, which
profiles/lbfgs_lockstep.txt records per case and quantity: worst 3.14 (H_diag, D = 4096), 2.3 (t), 1.5 (trial point), most below
1.5; the spreads themselves were 4e-7 .. 2.2e-5.  The margin covers the kernel's other summation tree (float32 partial sums per
thread, float64 across threads) and the fused multiply-adds of -ffp-contract=on, with a factor five in hand.

bf16 precision: the kernel writes only the bf16 trial point; it is compared with the twin's trial point rounded to bf16 with one
bf16 ulp allowed per element (what exceeds the ulp is held to the fp32 rule); x, d and the scalars are held to the fp32 rule.
With the bf16 ring (D = 2048) the twins adopt the kernel's x, d, t after each round's comparison (lbfgs_lockstep.run says why).

Windows moved off a rounding tie: lbfgs_lockstep.MOVED (none).
"""
import ctypes as C
import json

import numpy as np
import pytest

import lbfgs_lockstep as L
from helpers import TINY, heat_from_centres, sd_from_npz

pytestmark = pytest.mark.gpu

MARGIN = 16.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch


def observe(torch, name, rec):
    """One JSON line per case in the test log (what profiles/lbfgs_lockstep.txt is made from)."""
    line = json.dumps({"case": name, "device": torch.cuda.get_device_properties(0).name, "rounds": rec["rounds"],
                       "finish_round": rec["finish_round"], "max_pairs": rec["max_pairs"],
                       "spread": rec["spread"], "dev": rec["dev"], "ratio": rec["ratio"]}, sort_keys=True)
    print("OBSERVATION lbfgs_lockstep " + line)


def lockstep(torch, case, opts, name, **kw):
    drv = L.KernelDriver(case[0], case[1] == "bf16", case[2], opts, case[3])
    try:
        rec = L.run(drv, case, opts, **kw)
    finally:
        drv.close()
    observe(torch, name, rec)
    return rec


def hold_to_allowance(rec):
    for k in L.KEYS:
        allowed = L.allowance(rec["spread"][k], MARGIN)
        assert rec["dev"][k] <= allowed, "%s: kernel %.3g from the twin, allowed %.3g (twin against float64-dot twin: %.3g)" \
            % (k, rec["dev"][k], allowed, rec["spread"][k])


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_kernel_follows_its_twin_in_lock_step(torch_cuda, case):
    rec = lockstep(torch_cuda, case, L.options(case[4]), L.case_id(case))
    hold_to_allowance(rec)
    assert rec["rounds"] > 8 and len(set(rec["finish_round"])) >= 4, rec["finish_round"]          # the windows finish in different rounds


def test_other_optimiser_options(torch_cuda):
    # With c2 = 0.5 the zoom phase narrows its brackets far more often than with 0.9, and a twin that interpolates between its OWN
    # step lengths but the shared f values amplifies a rounding difference of t by t / (bracket width): on the CPU the twin and its
    # float64-dot version part ways within 25-40 rounds for 57 of 60 seeds of every objective but one.  So in this case the twins adopt
    # the kernel's x, d and t after each round's comparison (as with the bf16 ring): every round is then checked on its own.
    case = (300, "f32", 1, 0, 100)
    opts = L.options(100, lr=0.5, max_iter=33, max_eval=41, tol_change=1e-9, c2=0.5)
    hold_to_allowance(lockstep(torch_cuda, case, opts, "options-" + L.case_id(case), adopt=True))


def test_nan_value_is_latched_and_stays_in_its_window(torch_cuda):
    # window 1 is handed f = NaN in round 3 (a VALUE the kernel is written to latch: bit 1 of the window's status comes from
    # nan_seen); the run ends, and every other window is bitwise what it is without the NaN, in every round
    case = (520, "f32", 2, 3, 5)
    opts = L.options(case[4])
    clean = lockstep(torch_cuda, case, opts, "nan-clean-" + L.case_id(case))
    dirty = lockstep(torch_cuda, case, opts, "nan-" + L.case_id(case), nan_at=(1, 3))
    assert clean["finish_round"][1] > 4, "window 1 must still iterate in round 3"
    assert not clean["nan_seen"].any()
    assert list(dirty["nan_seen"]) == [0, 1] + [0] * (L.B - 2)
    others = [b for b in range(L.B) if b != 1]
    assert len(dirty["history"]) >= max(clean["finish_round"][b] for b in others) + 1
    for r, (a, b) in enumerate(zip(clean["history"], dirty["history"])):
        for k in a:
            assert np.array_equal(a[k][others], b[k][others], equal_nan=True), "round %d: %s of another window changed" % (r, k)


def test_bad_arguments_are_refused_with_a_message(torch_cuda):
    from globalegomocap_amd import _capi
    from globalegomocap_amd.engine import _ptr, _stream
    torch = torch_cuda
    opts = L.options(5)
    with pytest.raises(_capi.GemError, match="4096"):          # beyond the widest instantiation (refused when the handle is made,
        drv = L.KernelDriver(4097, False, 0, opts, 0, max_windows=2)          # at the latest by the first advance)
        drv.begin([np.zeros(4097, np.float32)] * 2)
        drv.advance(np.zeros(2), torch.zeros(1, 2, 4097))
    drv = L.KernelDriver(48, False, 0, opts, 0, max_windows=4)
    eng, lib = drv.eng, drv.eng.lib
    x0 = torch.zeros(8, 48, device=eng.device)
    f = torch.zeros(8, device=eng.device, dtype=torch.float64)
    with pytest.raises(_capi.GemError, match="max_windows"):
        _capi.check(lib.gem_lbfgs_debug_begin(eng._h, 5, _ptr(x0), 0, _stream()), lib)
    with pytest.raises(_capi.GemError, match="slots"):
        _capi.check(lib.gem_lbfgs_debug_begin(eng._h, 4, _ptr(x0), 3, _stream()), lib)
    with pytest.raises(_capi.GemError, match="gem_lbfgs_debug_begin"):          # no run in progress
        _capi.check(lib.gem_lbfgs_debug_advance(eng._h, 4, C.byref(drv.opts), _ptr(f), _ptr(x0), 0, _stream()), lib)
    eng.lbfgs_debug_begin(x0[:4], 0)
    far = _capi.default_lbfgs_opts(max_iter=40)          # beyond the ring of 32 pairs
    with pytest.raises(_capi.GemError, match="max_iter"):
        _capi.check(lib.gem_lbfgs_debug_advance(eng._h, 4, C.byref(far), _ptr(f), _ptr(x0), 0, _stream()), lib)
    with pytest.raises(_capi.GemError, match="n_slabs"):          # refused before a byte of g is read
        _capi.check(lib.gem_lbfgs_debug_advance(eng._h, 4, C.byref(drv.opts), _ptr(f), _ptr(x0), 1 << 30, _stream()), lib)
    with pytest.raises(_capi.GemError, match="max_windows"):
        _capi.check(lib.gem_lbfgs_debug_advance(eng._h, 5, C.byref(drv.opts), _ptr(f), _ptr(x0), 0, _stream()), lib)
    eng.lbfgs_debug_advance(f[:4], x0[:4], drv.opts, 0)          # the run is still usable: zero gradients finish every window
    assert list(eng.lbfgs_debug_read(4)["phase"]) == [L.DONE] * 4
    drv.close()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_a_stage_after_a_debug_run_gives_the_bits_of_a_fresh_handle(torch_cuda, golden, precision):
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    from globalegomocap_amd.engine import WindowEngine, energy_weights
    g = golden("lbfgs_tiny")
    pose, heat = g["pose"], heat_from_centres(g["heat_centres"])
    B = 12
    poses = np.repeat(pose[None], B, axis=0) + 1e-3 * np.arange(B, dtype=np.float32)[:, None, None, None]
    eps = np.repeat(g["local_eps"][None], B, axis=0)
    outs = []
    for debug_first in (False, True):
        eng = WindowEngine(TINY, FisheyeCamera.from_json(DEFAULT_CALIBRATION), max_windows=16)
        eng.set_precision(precision)
        if debug_first:
            case = (TINY.latent_dim, precision, 2, 3, 5)
            opts = L.options(5)
            L.run(L.KernelDriver(case[0], precision == "bf16", 2, opts, 3, engine=eng), case, opts)
        eng.load_vae(0, sd_from_npz(g, "local/"))
        mb = eng.mean_bone_length(pose.astype(np.float32))
        out, stats = eng.optimize_stage(0, poses, mb, eps, energy_weights(1e-6, 1e-5, 1e-2, 0.0, 1e-2), heat, np.zeros(B, np.int32))
        outs.append((out.cpu().numpy(), stats.cpu().numpy()))
        eng.close()
    assert np.all(outs[0][1][:, 3] == 1)
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    assert np.array_equal(outs[0][1], outs[1][1])
