"""The oracle's L-BFGS machine against torch.optim.LBFGS, lock-step (CPU).

A free-running L-BFGS is chaotic: two correct implementations drift apart within a few iterations, which is why the stage tests
allow +-3 evaluations.  Here both sides consume the SAME (f, g) in every round -- torch's closure evaluates the objective at
the machine's trial point and hands the result to both -- so only rounding separates them and every branch decision must agree.

Tolerance: 2e-4 relative to max|trial|.  Measured over 180 cases of this kind the worst deviation was 5.7e-5 (another BLAS
summation order moves it); a wrong branch, flag or interpolation bound is off by orders of magnitude more.
"""
import functools

import numpy as np
import pytest
import torch

from oracle.np_oracle import LBFGSMachine, LBFGSOptions
import lbfgs_lockstep
import lbfgs_objectives as objectives
from lbfgs_twin import Dot64Machine, PairwiseTwin

TOL = 2e-4
DIMS = (45, 520, 2048, 3000)
HISTORIES = (100, 5, 2)
OPTIONS = ((2.0, 25, 31), (1.0, 12, 15))
CASES = [(name, D, hist, opt) for name in objectives.NAMES for D in DIMS for hist in HISTORIES for opt in OPTIONS]
# cases in which torch and the machine part ways on a rounding tie of a branch decision (at most one in ten may be listed)
DROPPED = []
assert len(DROPPED) * 10 <= len(CASES)

PHASES = ("INIT", "BRACKET", "ZOOM", "DONE")
ALL_TRANSITIONS = {("INIT", "BRACKET"), ("INIT", "DONE"), ("BRACKET", "BRACKET"), ("BRACKET", "ZOOM"), ("BRACKET", "DONE"),
                   ("ZOOM", "BRACKET"), ("ZOOM", "ZOOM"), ("ZOOM", "DONE")}


def options(lr, max_iter, max_eval, hist):
    return LBFGSOptions(lr=lr, max_iter=max_iter, max_eval=max_eval, history=hist, tol_grad=1e-7, tol_change=1e-6)


def rel_dev(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))


@functools.lru_cache(maxsize=None)
def run_case(name, D, hist, opt):
    lr, max_iter, max_eval = opt
    seed = DIMS.index(D) * 7 + HISTORIES.index(hist)
    fun, x0 = objectives.make(name, D, seed=seed, scale=1.0)
    machine = LBFGSMachine(x0.numpy(), options(lr, max_iter, max_eval, hist))
    x = x0.clone().requires_grad_(True)
    optim = torch.optim.LBFGS([x], lr=lr, max_iter=max_iter, max_eval=max_eval, tolerance_grad=1e-7, tolerance_change=1e-6,
                              history_size=hist, line_search_fn="strong_wolfe")
    rec = {"devs": [], "transitions": set(), "full_ring": False, "late_call": False}

    def closure():
        rec["late_call"] |= machine.phase == machine.DONE      # torch asks for an evaluation the machine does not want
        rec["devs"].append(rel_dev(x.detach().numpy(), machine.trial))
        f, g = fun(torch.from_numpy(machine.trial))
        before = machine.phase
        machine.advance(float(f), g.numpy())
        rec["transitions"].add((PHASES[before], PHASES[machine.phase]))
        rec["full_ring"] |= len(machine.S) == hist
        x.grad = g.clone()
        return f

    optim.step(closure)
    st = optim.state[x]
    rec.update(done=machine.phase == machine.DONE, n_iter=(st["n_iter"], machine.n_iter), evals=(st["func_evals"], machine.evals),
               final=rel_dev(x.detach().numpy(), machine.x), calls=len(rec["devs"]))
    return rec


@pytest.mark.parametrize("name,D,hist,opt", [c for c in CASES if c not in DROPPED],
                         ids=lambda v: str(v).replace(" ", ""))
def test_machine_follows_torch_lbfgs_in_lock_step(name, D, hist, opt):
    rec = run_case(name, D, hist, opt)
    assert not rec["late_call"], "torch called the closure after the machine had finished"
    assert rec["done"], "torch stopped calling while the machine still wants an evaluation"
    assert max(rec["devs"]) <= TOL, "trial points apart by %.3g in closure call %d" % (max(rec["devs"]), int(np.argmax(rec["devs"])))
    assert rec["n_iter"][0] == rec["n_iter"][1]
    assert rec["evals"][0] == rec["evals"][1] == rec["calls"]
    assert rec["final"] <= TOL


def test_every_phase_transition_and_a_full_ring_are_reached():
    recs = [run_case(*c) for c in CASES if c not in DROPPED]
    seen = set().union(*(r["transitions"] for r in recs))
    assert seen >= ALL_TRANSITIONS, "not reached: %s" % sorted(ALL_TRANSITIONS - seen)
    assert any(r["full_ring"] for r in recs)


# ---- the twins the GPU test compares the kernel with, lock-step against the machine --------------------------------------------
def lockstep(lead, others, fun, max_rounds):
    """Feed every machine the (f, g) evaluated at `lead`'s trial point; returns per follower the worst deviation of its trial point
    and whether all integer states agreed in every round."""
    worst, same = [0.0] * len(others), True
    for _ in range(max_rounds):
        if lead.phase == lead.DONE:
            break
        f, g = fun(torch.from_numpy(lead.trial))
        f, g = float(f), g.numpy()
        lead.advance(f, g)
        for i, m in enumerate(others):
            m.advance(f, g)
            same &= (m.phase, m.n_iter, m.evals, len(m.S)) == (lead.phase, lead.n_iter, lead.evals, len(lead.S))
            worst[i] = max(worst[i], rel_dev(m.trial, lead.trial))
    return worst, same


@pytest.mark.parametrize("D,hist", [(45, 100), (520, 5), (520, 2), (2048, 3), (3000, 5)])
def test_pairwise_and_float64_dot_twins_follow_the_machine(D, hist):
    # the kernel's pairwise two-loop recursion (cadj cross term) and float64 reductions are the machine's arithmetic up to rounding:
    # same branches in every round, trial points within the tolerance of the torch comparison
    for name in objectives.NAMES:
        fun, x0 = objectives.make(name, D, seed=3, scale=1.0)
        o = options(2.0, 25, 31, hist)
        lead = LBFGSMachine(x0.numpy(), o)
        worst, same = lockstep(lead, [PairwiseTwin(x0.numpy(), o), Dot64Machine(x0.numpy(), o), PairwiseTwin(x0.numpy(), o, dot64=True)],
                               fun, 32)
        assert same, name
        assert max(worst) <= TOL, (name, worst)


@pytest.mark.parametrize("case", lbfgs_lockstep.CASES, ids=lbfgs_lockstep.case_id)
def test_gpu_lockstep_cases_lead_both_twins_through_the_same_branches(case):
    # the harness of test_lbfgs_lockstep_gpu.py with float64-dot twins in the kernel's place: the twin and the float64-dot twin
    # agree on every branch for the inputs of every GPU case (no rounding ties), every window finishes, and the batch reaches the
    # ring wrap; with it the harness itself is exercised without a GPU
    opts = lbfgs_lockstep.options(case[4])
    rec = lbfgs_lockstep.run(lbfgs_lockstep.StandInDriver(case[0], case[1] == "bf16", case[2], opts), case, opts)
    assert rec["rounds"] > 8 and len(set(rec["finish_round"])) >= 4, rec["finish_round"]
    assert rec["max_pairs"] == min(case[4], 24) or case[4] == 100
    for k in lbfgs_lockstep.KEYS:          # the stand-in IS the float64-dot twin
        assert rec["dev"][k] == rec["spread"][k] or (k == "trial" and case[1] == "bf16")


def test_gpu_lockstep_case_with_other_options_on_the_stand_in():
    # test_lbfgs_lockstep_gpu.py::test_other_optimiser_options with the stand-in (twins adopting the driver's x, d, t each round)
    case = (300, "f32", 1, 0, 100)
    opts = lbfgs_lockstep.options(100, lr=0.5, max_iter=33, max_eval=41, tol_change=1e-9, c2=0.5)
    rec = lbfgs_lockstep.run(lbfgs_lockstep.StandInDriver(case[0], False, case[2], opts), case, opts, adopt=True)
    assert rec["rounds"] > 33 and max(rec["spread"].values()) < 2e-5
