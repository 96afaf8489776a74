"""Twins of lbfgs_advance_kernel (csrc/lbfgs.hip) built on the oracle's LBFGSMachine.

The machine itself is the twin of the fp32 instantiations: same state machine, same float32 vectors, float64 scalars;
its sequential two-loop recursion and the kernel's pairwise one differ by rounding only.

  Dot64Machine     the machine with float64 dot products: the stand-in for the kernel's reductions (float32 products summed
                   in float64 wave sums).  The distance machine <-> Dot64Machine is what a different summation order costs;
                   the GPU test scales its allowance from it.
  PairwiseTwin     the kernel's two-loop recursion, two pairs per reduction through cadj = s_k . y_(k+1); with
                   `bf16_ring=True` the stored (s, y) are rounded to bf16 (nearest even) while ro, H_diag and cadj come from
                   the unrounded new pair -- the `<8, true, true>` instantiation (bf16 precision at D = 2048).
  RoundedSequential  sequential loops over bf16-rounded pairs: NOT the kernel (it differs by one bf16 rounding inside cadj);
                   kept to measure that distance.
"""
import numpy as np

from oracle.np_oracle import LBFGSMachine

F32 = np.float32


def bf16_round(a):
    """float32 -> nearest-even bf16, returned as float32."""
    b = np.ascontiguousarray(a, dtype=F32).view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(F32)


def bf16_ulp(a):
    """Spacing of bf16 numbers at |a| (float32 array): 2^(e - 7)."""
    m = np.maximum(np.abs(np.asarray(a, dtype=F32)), F32(2.0 ** -126))
    return np.exp2(np.floor(np.log2(m.astype(np.float64))) - 7.0)


def _dot64(a, b):
    return float(np.dot(a.astype(np.float64), b.astype(np.float64)))


class Dot64Machine(LBFGSMachine):
    _dot = staticmethod(_dot64)


class PairwiseTwin(LBFGSMachine):
    def __init__(self, x0, opt=None, bf16_ring=False, dot64=False):
        super().__init__(x0, opt)
        self.bf16_ring = bf16_ring
        self.cadj = []          # cadj[k] = S[k] . Y[k+1] (stored S, unrounded new Y), k-th oldest pair
        if dot64:
            self._dot = _dot64

    def _store_pair(self, s, y):
        if len(self.cadj) > len(self.S):          # the machine dropped the oldest pair
            self.cadj.pop(0)
        if self.S:
            self.cadj[-1] = self._dot(self.S[-1], y)
        self.cadj.append(0.0)
        if self.bf16_ring:
            s, y = bf16_round(s), bf16_round(y)
        self.Y.append(y); self.S.append(s)

    def _two_loop(self, g):
        S, Y, ro, c = self.S, self.Y, self.ro, self.cadj
        k = len(S)
        al = [0.0] * k
        q = (-g).astype(F32)
        for a in range(k - 1, -1, -2):            # pair (a, a - 1): both dot products against the same q
            b = a - 1
            al[a] = self._dot(S[a], q) * ro[a]
            fa = F32(al[a])
            if b >= 0:
                al[b] = (self._dot(S[b], q) - float(fa) * c[b]) * ro[b]
                q = (q - (fa * Y[a] + F32(al[b]) * Y[b])).astype(F32)
            else:
                q = (q - fa * Y[a]).astype(F32)
        q = (q * F32(self.H_diag)).astype(F32)
        for a in range(0, k, 2):                  # pair (a, a + 1)
            b = a + 1
            cfa = F32(al[a] - self._dot(Y[a], q) * ro[a])
            if b < k:
                cfb = F32(al[b] - (self._dot(Y[b], q) + float(cfa) * c[a]) * ro[b])
                q = (q + (cfa * S[a] + cfb * S[b])).astype(F32)
            else:
                q = (q + cfa * S[a]).astype(F32)
        return q


class RoundedSequential(LBFGSMachine):
    def _store_pair(self, s, y):
        self.Y.append(bf16_round(y)); self.S.append(bf16_round(s))


INT_FIELDS = ("phase", "n_iter", "evals", "ls_iter", "hist_count", "low", "high", "insuf")


def state_of(m):
    """The machine's scalars under the names of gem_lbfgs_debug_state (attributes the machine has not set yet read as the
    kernel's initial values)."""
    return {"phase": m.phase, "n_iter": m.n_iter, "evals": m.evals, "ls_iter": getattr(m, "ls_iter", 0),
            "hist_count": len(m.S), "low": getattr(m, "low", 0), "high": getattr(m, "high", 1),
            "insuf": int(getattr(m, "insuf", False)), "t": getattr(m, "t", 0.0), "loss": getattr(m, "loss", 0.0),
            "gtd": getattr(m, "gtd", 0.0), "H_diag": m.H_diag}
