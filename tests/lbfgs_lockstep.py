"""Lock-step harness: lbfgs_advance_kernel (through gem_lbfgs_debug_*) against its twins, round by round.

A batch holds B = 9 windows: the eight objectives of lbfgs_objectives with different seeds and start scales (so that the windows
finish in different rounds) and a duplicate of window 0.  Every round the objectives are evaluated at the DRIVER's trial points and
the same (f, g) goes to the driver, to one twin per window and to one twin with float64 dot products per window.

The driver is the kernel (`KernelDriver`, GPU tests) or a stand-in made of float64-dot twins (`StandInDriver`, CPU: proves that the
chosen inputs lead both twins through the same branches and exercises this harness without a GPU).
"""
import numpy as np
import torch

import lbfgs_objectives as objectives
from lbfgs_twin import INT_FIELDS, PairwiseTwin, bf16_round, bf16_ulp, state_of
from oracle.np_oracle import LBFGSOptions

F32 = np.float32
B = 9
# (objective, seed, start scale) per window; window 8 duplicates window 0
# (seeds chosen on the CPU so that, in every case below, the twin and its float64-dot version stay within 2e-5 of each other: some
# seeds meet an ill-conditioned interpolation that turns rounding into 1e-3 .. 1e-1 of the step length without any branch differing)
WINDOWS = (("quad", 3, 1.0), ("rosen", 3, 0.7), ("logcosh", 4, 1.5), ("sines", 0, 2.0), ("leaky", 0, 1.0), ("quartic", 5, 1.0),
           ("optimum", 6, 1.0), ("tiny", 7, 1.0), ("quad", 3, 1.0))
# windows whose seed was moved because the kernel and the twin parted on a genuine rounding tie: {case id: (window, new seed)};
# at most one per case
MOVED = {}

# (latent, precision, slots, n_slabs, history)
CASES = ((32, "f32", 0, 0, 100),          # Dp 64, <1>
         (48, "f32", 1, 0, 5),            # Dp 64, padding live
         (100, "f32", 2, 4, 100),         # Dp 128: half the threads idle
         (300, "f32", 1, 0, 2),           # Dp 320, <2>
         (520, "f32", 2, 3, 5),           # Dp 576, <4>: partial vector strip
         (1024, "f32", 0, 1, 100),        # <4> exact
         (1500, "f32", 2, 8, 5),          # Dp 1536, <8, false>
         (2048, "f32", 2, 4, 100),        # <8, true>
         (2048, "f32", 2, 4, 3),
         (2048, "bf16", 2, 9, 100),       # <8, true, true>: bf16 ring; nine slabs cross the eight-per-trip loop
         (2048, "bf16", 2, 9, 3),
         (520, "bf16", 2, 0, 5),          # bf16 trial point, fp32 ring
         (2049, "f32", 1, 2, 5),          # Dp 2112, <16>
         (4096, "f32", 2, 4, 100))        # <16> exact

DONE = 3
FLOOR = 8 * 2.0 ** -24          # a few float32 ulps
CAP = 2e-4                      # a wrong branch or a dropped term shows at 1e-3 and above
KEYS = ("trial", "x+td", "t", "gtd", "H_diag")


def case_id(c):
    return "D%d-%s-slots%d-slabs%d-hist%d" % c


def pad64(n):
    return (n + 63) // 64 * 64


def options(hist, lr=2.0, max_iter=25, max_eval=31, tol_change=1e-6, c2=0.9):
    return LBFGSOptions(lr=lr, max_iter=max_iter, max_eval=max_eval, history=hist, tol_grad=1e-7, tol_change=tol_change, c2=c2)


def _rel(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        return 0.0 if np.array_equal(a, b, equal_nan=True) else float("inf")
    s = float(np.max(np.abs(b))) if scale is None else scale
    return float(np.max(np.abs(a - b))) / max(s, 1e-300)


class StandInDriver:
    """The debug entry points played by float64-dot twins (no padding, no real slots: the slot tables imitate the three modes)."""

    def __init__(self, D, bf16, slots, opts):
        self.D, self.bf16, self.slots, self.opts = D, bf16, slots, opts
        self.device = "cpu"

    def begin(self, x0):
        ring = self.bf16 and pad64(self.D) == 2048
        self.m = [PairwiseTwin(x, self.opts, bf16_ring=ring, dot64=True) for x in x0]
        self.slot_of = np.arange(len(self.m), dtype=np.int32)
        self.nan = np.zeros(len(self.m), dtype=np.int32)

    def read(self):
        st = {k: np.array([state_of(m)[k] for m in self.m]) for k in INT_FIELDS + ("t", "loss", "gtd", "H_diag")}
        trial = np.stack([m.trial for m in self.m])
        st.update(x=np.stack([m.x for m in self.m]), d=np.stack([getattr(m, "d", np.zeros_like(m.x)) for m in self.m]),
                  trial=bf16_round(trial) if self.bf16 else trial, slot_of=self.slot_of.copy(),
                  count=int(sum(m.phase != DONE for m in self.m)) if self.slots else len(self.m),
                  pad_nonzero=np.zeros(len(self.m), dtype=np.int32), nan_seen=self.nan.copy())
        st["trial_dev"] = torch.from_numpy(st["trial"])
        return st

    def advance(self, f, rows):
        rows = rows.numpy()
        for b, m in enumerate(self.m):
            if m.phase == DONE:
                continue
            g = np.zeros(self.D, dtype=F32)
            for z in range(rows.shape[0]):
                g = (g + rows[z, self.slot_of[b]]).astype(F32)
            self.nan[b] |= int(f[b] != f[b])
            m.advance(f[b], g)
        live = [b for b, m in enumerate(self.m) if m.phase != DONE]
        if self.slots == 1:
            self.slot_of[live] = np.arange(len(live), dtype=np.int32)
        elif self.slots == 2:
            self.slot_of[live] = np.arange(len(live), dtype=np.int32)[::-1]


class KernelDriver:
    """The kernels behind gem_lbfgs_debug_*: a tiny VAE shape with the case's latent size, no weights loaded."""

    def __init__(self, D, bf16, slots, opts, n_slabs, max_windows=B, engine=None):
        from globalegomocap_amd import _capi
        from globalegomocap_amd.engine import WindowEngine
        from globalegomocap_amd.vae import VAEShape
        self.eng = engine or WindowEngine(VAEShape(latent_dim=D, hidden=(16, 32), seq_len=10), max_windows=max_windows)
        self.eng.set_precision("bf16" if bf16 else "f32")
        self.slots, self.n_slabs, self.device = slots, n_slabs, self.eng.device
        self.opts = _capi.GemLbfgsOpts(lr=opts.lr, max_iter=opts.max_iter, max_eval=opts.max_eval, history=opts.history, reserved=0,
                                       tol_grad=opts.tol_grad, tol_change=opts.tol_change, c1=opts.c1, c2=opts.c2,
                                       ls_tol_change=opts.ls_tol_change)

    def begin(self, x0):
        self.n = len(x0)
        self.eng.lbfgs_debug_begin(np.stack(x0), self.slots)

    def read(self):
        st = self.eng.lbfgs_debug_read(self.n)
        st["trial_dev"] = st["trial"]
        for k in ("x", "d", "trial"):
            st[k] = st[k].cpu().numpy()
        return st

    def advance(self, f, rows):
        self.eng.lbfgs_debug_advance(f, rows, self.opts, self.n_slabs)

    def close(self):
        self.eng.close()


def split_slabs(g, n, gen):
    """n float32 slabs and their float32 sum in slab order (what the kernel computes): the gradient both sides consume."""
    if n <= 1:
        return g[None], g
    w = torch.rand(n - 1, 1, generator=gen, dtype=torch.float32).to(g.device) * (2.0 / n)
    parts = w * g[None]
    acc = torch.zeros_like(g)
    for p in parts:
        acc = acc + p
    slabs = torch.cat([parts, (g - acc)[None]])
    total = torch.zeros_like(g)
    for p in slabs:
        total = total + p
    return slabs, total


def run(driver, case, opts, nan_at=None, windows=WINDOWS, adopt=False):
    """Runs one case to the end, asserting everything that must hold exactly and the hard cap; returns the observations
    (`dev`: driver against twin, `spread`: twin against float64-dot twin, per quantity, worst over windows and rounds).
    adopt: the twins take over the driver's x, d and t after each round's comparison (always with the bf16 ring, see below)."""
    D, precision, slots, n_slabs, hist = case
    bf16 = precision == "bf16"
    ring = bf16 and pad64(D) == 2048
    dev = driver.device
    made = [objectives.make(name, D, seed=seed, scale=scale, device=dev) for name, seed, scale in windows]
    funs, x0 = [m[0] for m in made], [m[1].cpu().numpy() for m in made]
    nb = len(windows)
    twins = [PairwiseTwin(x, opts, bf16_ring=ring) for x in x0]
    twins64 = [PairwiseTwin(x, opts, bf16_ring=ring, dot64=True) for x in x0]
    rec = {"dev": dict.fromkeys(KEYS, 0.0), "spread": dict.fromkeys(KEYS, 0.0), "transitions": set(), "rounds": 0, "history": [],
           "max_pairs": 0, "finish_round": [None] * nb, "nan_seen": None}
    frozen, poisoned = {}, set()
    driver.begin(x0)

    def vec(m):
        return (m.x + F32(getattr(m, "t", 0.0)) * getattr(m, "d", np.zeros_like(m.x))).astype(F32)

    def note(table, key, value, what):
        assert value <= CAP, "%s of %s apart by %.3g (cap %.1g)" % (key, what, value, CAP)
        table[key] = max(table[key], value)

    def check(st, rnd):
        raw = {k: np.asarray(st[k]).copy() for k in INT_FIELDS + ("t", "loss", "gtd", "H_diag", "x", "d", "trial")}
        rec["history"].append(raw)
        assert not np.any(st["pad_nonzero"]), "round %d: padding columns not zero: %s" % (rnd, st["pad_nonzero"])
        for b in range(nb):
            what = "window %d (%s) before round %d" % (b, windows[b][0], rnd)
            if b in frozen:          # a finished window no longer changes
                for k, v in frozen[b].items():
                    assert np.array_equal(raw[k][b], v, equal_nan=True), "%s: %s changed after the window had finished" % (what, k)
            elif st["phase"][b] == DONE:
                frozen[b] = {k: raw[k][b].copy() for k in raw}
                rec["finish_round"][b] = rnd
            if b in poisoned:
                continue
            m, m64 = twins[b], twins64[b]
            sm, s64 = state_of(m), state_of(m64)
            got = {k: int(st[k][b]) for k in INT_FIELDS}
            want = {k: int(sm[k]) for k in INT_FIELDS}
            want["hist_count"] = min(want["hist_count"], 32)
            assert got == want, ("%s: kernel and twin took different branches\n kernel %s t=%r gtd=%r loss=%r\n twin   %s t=%r gtd=%r loss=%r"
                                 % (what, got, st["t"][b], st["gtd"][b], st["loss"][b], want, sm["t"], sm["gtd"], sm["loss"]))
            assert {k: int(s64[k]) for k in INT_FIELDS} == {k: int(sm[k]) for k in INT_FIELDS}, \
                "%s: the two twins part ways on a rounding tie: move this window's seed" % what
            assert float(st["loss"][b]) == float(sm["loss"]), "%s: loss %r != %r" % (what, st["loss"][b], sm["loss"])
            live = sm["phase"] != DONE
            for k in ("t", "gtd", "H_diag"):
                if k == "t" and not live:          # (a window that finishes at the top of an iteration: the kernel has stored the
                    continue                       # iteration's first step length already, the machine has not)
                note(rec["dev"], k, _rel(st[k][b], sm[k]), what)
                note(rec["spread"], k, _rel(s64[k], sm[k]), what)
            scale = max(float(np.max(np.abs(m.trial))), 1e-30)
            note(rec["dev"], "x+td", _rel(st["x"][b] + F32(st["t"][b]) * st["d"][b] if live else st["x"][b], vec(m) if live else m.x, scale), what)
            note(rec["spread"], "x+td", _rel(vec(m64) if live else m64.x, vec(m) if live else m.x, scale), what)
            note(rec["spread"], "trial", _rel(m64.trial, m.trial, scale), what)
            if bf16:          # the kernel writes the bf16 trial point only: one bf16 ulp per element for the rounding of two fp32
                # values that differ in their last bits; what is beyond that ulp is held to the fp32 rule
                want_t = bf16_round(m.trial)
                over = np.abs(st["trial"][b].astype(np.float64) - want_t) - bf16_ulp(np.maximum(np.abs(want_t), np.abs(st["trial"][b])))
                note(rec["dev"], "trial", max(float(over.max()), 0.0) / scale, what)
            else:
                note(rec["dev"], "trial", _rel(st["trial"][b], m.trial, scale), what)
            if (ring or adopt) and live:
                # bf16 ring: rounding a stored pair turns a last-bit difference of s = t d into a whole bf16 ulp of that element
                # (2^-8 of it; twin against float64-dot twin: 2.4e-3 of max|trial| within five rounds), which no rounding-level
                # allowance covers.  So here both twins adopt the driver's x, d and t once the round has been compared: s is then
                # the driver's bit for bit (y is anyway: both sides hold the same gradients), the rings are equal, and every round
                # is checked on its own under the fp32 rule.
                for tw in (m, m64):
                    tw.x, tw.t = st["x"][b].copy(), float(st["t"][b])
                    if hasattr(tw, "d"):
                        tw.d = st["d"][b].copy()
        if not poisoned & {0, nb - 1}:          # the duplicate window is bitwise window 0
            for k, v in raw.items():
                assert np.array_equal(v[nb - 1], v[0], equal_nan=True), "round %d: %s of the duplicate window differs from window 0" % (rnd, k)
        live = [b for b in range(nb) if st["phase"][b] != DONE]
        if slots == 0:
            assert np.array_equal(st["slot_of"], np.arange(nb))
        else:
            assert st["count"] == len(live), "round %d: live count %d, %d windows iterate" % (rnd, st["count"], len(live))
            assert sorted(int(st["slot_of"][b]) for b in live) == list(range(len(live))), \
                "round %d: slots %s of the live windows %s are no permutation" % (rnd, st["slot_of"], live)
        return live

    for rnd in range(opts.max_eval + 1):
        st = driver.read()
        live = check(st, rnd)
        if not live:
            break
        rec["rounds"] = rnd + 1
        f = np.zeros(nb, dtype=np.float64)
        rows = torch.zeros(max(n_slabs, 1), nb, D, dtype=torch.float32, device=dev)
        fed = {}
        for b in live:
            fb, g = funs[b](st["trial_dev"][b])
            # (cut by a generator seeded from the window's seed and the round: the duplicate window gets window 0's slabs)
            slabs, total = split_slabs(g, n_slabs, torch.Generator().manual_seed(100 * rnd + windows[b][1]))
            rows[:, int(st["slot_of"][b])] = slabs
            f[b] = float(fb)
            if nan_at == (b, rnd):
                f[b] = float("nan")
                poisoned.add(b)
            fed[b] = total.cpu().numpy()
        driver.advance(f, rows)
        for b in live:
            if b in poisoned:
                continue
            before = twins[b].phase
            twins[b].advance(f[b], fed[b])
            twins64[b].advance(f[b], fed[b])
            rec["transitions"].add((before, twins[b].phase))
            rec["max_pairs"] = max(rec["max_pairs"], len(twins[b].S))
    else:
        st = driver.read()
        live = check(st, opts.max_eval + 1)
        assert not [b for b in live if b not in poisoned], "windows %s still iterate after max_eval + 1 rounds" % live
    rec["nan_seen"] = np.asarray(st["nan_seen"]).copy()
    rec["ratio"] = {k: rec["dev"][k] / max(rec["spread"][k], FLOOR) for k in KEYS}
    return rec


def allowance(spread, margin):
    return min(CAP, margin * spread + FLOOR)
