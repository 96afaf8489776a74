"""One layer of the GEMM dispatch functions, stated in numpy float64, the planners' rules, and the route case table.

    C = epi( sum_tap shift_tap(A) . W[tap]^T + bias ),   row = window * T + frame

A shifted row that leaves its window is zero; rows go through `row_map` when one is given (linear layers); EPI_MASK multiplies
by aux > 0 ? 1 : 0.01; LeakyReLU is one fp32 multiply by 0.01f.  The bf16 modes round the operands as the kernels do (round to
nearest even; hi = bf16(x), lo = bf16(x - hi); product a_hi w_hi + a_hi w_lo + a_lo w_hi) and then sum in float64: every term
is exact in fp32, so a device result may differ from the twin by fp32 accumulation only (`bound`).

The planners below restate the dispatch rules of csrc/gemm_f32.hip, gemm_bf16.hip, decoder_bf16.hip and gemm_rows.h so that the
case table can say, without a device, which kernel every case must reach; the GPU test compares that with the name the library
reports, so a drift between the two shows as a failing case, never as a case that quietly tests a neighbouring route.
"""
from collections import namedtuple

import numpy as np

F32, F64 = np.float32, np.float64
SLOPE = F32(0.01)
EPI_BIAS, EPI_BIAS_LRELU, EPI_MASK, EPI_NONE = 0, 1, 2, 3
N_CU = 256
SPLITK_ELEMS = 16 << 20          # the split-K scratch of a handle with a small latent (gem_create)
BIG_MIN_ROWS = 5376
GUARD_ROWS = 256                 # the tallest row tile of any kernel here (gemm_big.h)


# ------------------------------------------------------------------------------------------------ bf16
def bf16_bits(x):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even; finite inputs."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_widen(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def bf16_round(x):
    return bf16_widen(bf16_bits(x))


def split_hi_lo(x):
    x = np.asarray(x, dtype=F32)
    hi = bf16_round(x)
    return hi, bf16_round((x - hi).astype(F32))


# ------------------------------------------------------------------------------------------------ the contract
def shifted_rows(A, tap, taps, T, M, row_map=None):
    """[M, K] float64: the rows the product of tap `tap` reads (zeros where the shifted frame leaves the window)."""
    A = np.asarray(A)
    if taps == 1:
        src = np.arange(M) if row_map is None else np.asarray(row_map)[:M]
        return A[src].astype(F64)
    out = np.zeros((M, A.shape[1]), dtype=F64)
    r = np.arange(M)
    tt = r % T + tap - 1
    ok = (tt >= 0) & (tt < T)
    out[ok] = A[r[ok] + tap - 1]
    return out


def operand_products(mode):
    """(a part, w part) pairs summed by a precision mode: 'f32', 'bf16x3' (hi/lo split), 'bf16' (both operands rounded)."""
    return {"f32": [("x", "x")], "bf16": [("hi", "hi")], "bf16x3": [("lo", "hi"), ("hi", "lo"), ("hi", "hi")]}[mode]


def _parts(x, mode):
    x = np.asarray(x, dtype=F32)
    if mode == "f32":
        return {"x": x}
    hi, lo = split_hi_lo(x)
    return {"hi": hi, "lo": lo}


Twin = namedtuple("Twin", "pre out out32 absum n_terms")


def apply_epi(pre, epi, aux=None):
    if epi == EPI_BIAS_LRELU:
        return np.where(pre > 0, pre, pre * pre.dtype.type(SLOPE))
    if epi == EPI_MASK:
        return pre * np.where(np.asarray(aux) > 0, pre.dtype.type(1), pre.dtype.type(SLOPE))
    return pre


def gemm_twin(A, w, bias, epi, M, T=1, aux=None, row_map=None, mode="f32"):
    """pre = sum + bias in float64 (operands rounded as `mode` says), out = epi(pre) in float64, out32 = epi applied in fp32 to
    fp32(pre) (what a device computes when pre is exact), absum = sum |a||w| + |bias| per element, n_terms = taps * K * products."""
    w = np.asarray(w, dtype=F32)
    taps, N, K = w.shape
    wp = _parts(w, mode)
    pre = np.zeros((M, N), dtype=F64)
    absum = np.zeros((M, N), dtype=F64)
    prods = operand_products(mode)
    for tap in range(taps):
        a = shifted_rows(A, tap, taps, T, M, row_map)
        ap = _parts(a.astype(F32), mode)
        for pa, pw in prods:
            x, y = ap[pa].astype(F64), wp[pw][tap].astype(F64)
            pre += x @ y.T
            absum += np.abs(x) @ np.abs(y).T
    if epi in (EPI_BIAS, EPI_BIAS_LRELU):
        b = np.asarray(bias, dtype=F32).astype(F64)
        pre += b[None]
        absum += np.abs(b)[None]
    aux_m = None if aux is None else np.asarray(aux)[:M]
    out = apply_epi(pre, epi, aux_m)
    out32 = apply_epi(pre.astype(F32), epi, aux_m).astype(F32)
    return Twin(pre, out, out32, absum, taps * K * len(prods))


def bound(tw):
    """|device - twin| per element when the device sums the same (fp32-exact) terms in fp32, in any order, adds the bias, applies
    the epilogue: (n_terms + 8) * 2^-24 * (sum |a||w| + |bias|).  n - 1 additions of partial sums no larger than the absolute
    sum cost at most one half-ulp each; the 8 covers the slab sums, the bias add, the LeakyReLU multiply and the twin's own
    rounding of `pre` to fp32."""
    return (tw.n_terms + 8) * 2.0 ** -24 * tw.absum


def bound_out(tw, epi, aux=None):
    """`bound` carried through the epilogue, never larger than it: an element on the 0.01 branch of LeakyReLU or of the mask has
    its error scaled by 0.01 as well (the multiply's own rounding is one of the 8).  An element whose `pre` lies within the bound
    of zero may take either LeakyReLU branch on the device and keeps the whole bound."""
    b = bound(tw)
    if epi == EPI_BIAS_LRELU:
        return np.where(tw.pre < -b, b * F64(SLOPE), b)
    if epi == EPI_MASK:
        return b * np.where(np.asarray(aux)[:b.shape[0]] > 0, 1.0, F64(SLOPE))
    return b


def bf16_uncertain(out, bnd):
    """Elements whose twin value lies within `bnd` of a bf16 rounding boundary: rounding the device's fp32 value may go either way."""
    lo, hi = bf16_bits((out - bnd).astype(F32)), bf16_bits((out + bnd).astype(F32))
    return lo != hi


# ------------------------------------------------------------------------------------------------ the planners' rules
def cdiv(a, b):
    return (a + b - 1) // b


def pick_splitk(blocks, n_tiles, slab_elems, n_cu=N_CU, cap=SPLITK_ELEMS):
    if blocks >= 3 * n_cu:
        return 1
    best, best_score = 1, -1.0
    for sk in range(1, 9):
        if sk > 1 and (n_tiles // sk < 6 or sk * slab_elems > cap):
            break
        wgs = blocks * sk
        per_cu = cdiv(wgs, n_cu)
        score = wgs / float(per_cu * n_cu)
        if per_cu < 2:
            score *= 0.6
        score -= 0.01 * sk
        if score > best_score:
            best_score, best = score, sk
    return best


RowsPlan = namedtuple("RowsPlan", "n_rb n_split per fill cost")


def rows_plan_for(M, N, K, rt_max, n_cu, allow_split, cap, ldc):
    best = RowsPlan(0, 0, 0, 0.0, 1e30)
    if N % 64 or K % 64 or M <= 0:
        return best
    R, n_ct, nk = cdiv(M, 16), N // 64, K // 64
    first = cdiv(R, rt_max)
    for n_rb in range(first, R + 1):
        rpb = cdiv(R, n_rb)
        if rpb < 3 and n_rb > first:
            break
        for sk in range(1, (8 if allow_split else 1) + 1):
            if n_rb * n_ct * sk > n_cu:
                break
            if sk > 1 and (nk // sk < 4 or sk * M * ldc > cap):
                break
            per = cdiv(nk, sk)
            slab_units = sk * (M * N * 8.0 / 3.0e12) / 0.214e-6 if sk > 1 else 0.0
            cost = (rpb + 0.7) * per + slab_units
            if cost < best.cost:
                best = RowsPlan(n_rb, sk, per, R * n_ct * nk / float(n_cu * rpb * per), cost)
    return best


def rows_plan(M, N, K, slabs, n_cu=N_CU, cap=SPLITK_ELEMS):
    """(plan, use8) when the few-rows kernel takes a linear layer with M rows, else None."""
    if M < 48 or N % 64 or K % 64:
        return None
    p5 = rows_plan_for(M, N, K, 5, n_cu, slabs, cap, N)
    p8 = rows_plan_for(M, N, K, 8, n_cu, slabs, cap, N)
    use8 = p8.n_rb > 0 and (p5.n_rb == 0 or p8.cost < p5.cost - 1e-9)
    p = p8 if use8 else p5
    return (p, use8) if p.n_rb != 0 and p.fill >= 0.75 else None


Route = namedtuple("Route", "kernels n_slices dyn_W deferred c_bf16 detail")


def _bool(b):
    return "true" if b else "false"


def plan_launch_gemm(precision, taps, N, K, epi, M, rows=False, defer=False, family=-1, n_cu=N_CU, cap=SPLITK_ELEMS):
    """What launch_gemm does with a layer: kernel name, K slices of a static cut, workgroups of a device-side cut (0: none),
    whether slabs are left to the consumer."""
    if precision != "f32":
        nprod = 3 if precision == "bf16x3" else 1
        if N % 128 == 0 and cdiv(M, 128) * (N // 128) >= 256:
            return Route(["gem::gemm_bf16_big_kernel<%d, %d, %d>" % (taps, epi, nprod)], 1, 0, False, False, "bf16 big")
        n_tiles = taps * (K // 64)
        blocks = (N // 64) * cdiv(M, 64)
        per = cdiv(n_tiles, pick_splitk(blocks, n_tiles, M * N, n_cu, cap))
        z = cdiv(n_tiles, per)
        dyn = blocks * z if rows and z > 1 and blocks * z * 64 * 64 <= cap else 0
        return Route(["gem::gemm_bf16_kernel<%d, %d, %d>" % (taps, epi, nprod)], z, dyn, bool(defer and z > 1), False,
                     "bf16 small per=%d" % per)
    if taps == 1 and epi != EPI_MASK:
        rp = rows_plan(M, N, K, defer, n_cu, cap)
        if rp:
            p, use8 = rp
            return Route(["gem::rows::gemm_rows_kernel<%d, %d, false>" % ((3, 8) if use8 else (4, 5))], p.n_split, 0, p.n_split > 1,
                         False, "rows n_rb=%d per=%d" % (p.n_rb, p.per))
    big_blocks = cdiv(M, 128) * (N // 128)
    if N % 128 == 0 and big_blocks >= 3 * n_cu // 2 and not defer:
        return Route(["gem::glds::gemm_glds_kernel<true, %d, %d, 128, 128, false, 16, 2>" % (taps, epi)], 1, 0, False, False, "glds f32")
    r = 2 if N % 128 == 0 and big_blocks >= 512 else 1
    tag = 0
    if taps == 1:
        tag = 1 if (epi == EPI_BIAS and family == 0) or epi == EPI_BIAS_LRELU else 0
    n_tiles = taps * (K // 32)
    blocks = (N // (64 * r)) * cdiv(M, 64 * r)
    per = cdiv(n_tiles, pick_splitk(blocks, n_tiles, M * N, n_cu, cap))
    z = cdiv(n_tiles, per)
    dyn = blocks * z if rows and r == 1 and z > 1 and blocks * z * 64 * 64 <= cap else 0
    return Route(["gem::gemm_f32_kernel<%d, %d, %d, %d, %d, 32>" % (taps, epi, r, r, tag)], z, dyn, bool(defer and z > 1 and r == 1),
                 False, "tile per=%d" % per)


def plan_gemm_bf16a(taps, N, K, epi, M, out_bf16, allow_split, family=-1, rows=False, defer=False, n_cu=N_CU, cap=SPLITK_ELEMS):
    bn = 128 if N % 128 == 0 else 64
    tiles = cdiv(M, 128) * (N // bn)
    k_tiles = taps * (K // 64)
    fits = taps == 1 and ((epi == EPI_BIAS_LRELU and out_bf16 and N % 320 == 0) or (epi == EPI_NONE and not out_bf16 and N % 256 == 0))
    use_big = family == 0 and M >= BIG_MIN_ROWS and fits
    n_split = 1
    if allow_split and epi != EPI_MASK:
        sk = min(2 * n_cu // tiles, k_tiles // 4, 8)
        while sk > 1 and sk * M * N > cap:
            sk -= 1
        if sk > 1:
            n_split = cdiv(k_tiles, cdiv(k_tiles, sk))
    kernels = []
    if use_big:
        kernels.append("gem::big::gemm_big_kernel<4, 4, 4, 5, 1, true>" if epi == EPI_BIAS_LRELU else "gem::big::gemm_big_kernel<4, 4, 4, 4, 3, false>")
    if not use_big or rows:
        kernels.append("gem::glds::gemm_glds_kernel<false, %d, %d, 128, %d, %s, 16, 2>" % (taps, epi, bn, _bool(out_bf16 and n_split == 1)))
    deferred = bool(defer and n_split > 1)
    return Route(sorted(kernels), n_split, 0, deferred, bool(out_bf16 and not deferred), "bf16a bn=%d" % bn)


# ------------------------------------------------------------------------------------------------ the case table
# route 'g' = launch_gemm (in the precision mode named), 'a' = gemm_bf16a.  rows: the device row count m (rows of a linear layer,
# rows = windows * T of a conv), None = on the host.  rmap: a row map that permutes and repeats rows.  want: a substring of the
# kernel name the case is meant to reach (checked against the planner here and against the library's report on the device).
Case = namedtuple("Case", "id route precision taps N K epi M T rows rmap defer out_bf16 allow_split family want slices dyn")


def _c(id, route, precision, taps, N, K, epi, M, T=1, rows=None, rmap=False, defer=False, out_bf16=False, allow_split=False,
       family=-1, want="", slices=None, dyn=None):
    return Case(id, route, precision, taps, N, K, epi, M, T, rows, rmap, defer, out_bf16, allow_split, family, want, slices, dyn)


def _cases():
    c = []
    names = {EPI_BIAS: "bias", EPI_BIAS_LRELU: "lrelu", EPI_MASK: "mask", EPI_NONE: "none"}
    # 64x64 fp32 tile, single pass: linear layers over the row-tile edges, convs whose window borders fall inside a row tile
    i = 0
    for M in (1, 63, 64, 65, 130):
        for N in (64, 192):
            epi = (EPI_BIAS, EPI_NONE, EPI_BIAS_LRELU)[i % 3]
            c.append(_c("tile64-lin-M%d-N%d-%s" % (M, N, names[epi]), "g", "f32", 1, N, 64, epi, M, rmap=(i % 4 == 3),
                        want="gemm_f32_kernel<1, %d, 1, 1, " % epi, slices=1))
            i += 1
    c.append(_c("tile64-lin-front-tag", "g", "f32", 1, 64, 64, EPI_BIAS, 65, family=0, want="gemm_f32_kernel<1, 0, 1, 1, 1, 32>", slices=1))
    i = 0
    for B in (1, 6, 7, 13):
        for T in (9, 10, 16):
            epi = (EPI_BIAS, EPI_BIAS_LRELU, EPI_MASK, EPI_NONE)[i % 4]
            c.append(_c("tile64-conv-B%d-T%d-%s" % (B, T, names[epi]), "g", "f32", 3, (64, 192)[(i // 4 + i) % 2], 64, epi, B * T, T,
                        want="gemm_f32_kernel<3, %d, 1, 1, 0, 32>" % epi, slices=1))
            i += 1
    # static split-K with an uneven cut: taps * K / 32 = 13 (7 + 6) and 15 (8 + 7), every epilogue (they move into the reduce pass)
    for epi in (EPI_BIAS, EPI_BIAS_LRELU, EPI_NONE):
        c.append(_c("split13-lin-%s" % names[epi], "g", "f32", 1, 192, 416, epi, 130, want="gemm_f32_kernel<1, ", slices=2))
    for epi in (EPI_BIAS, EPI_BIAS_LRELU, EPI_MASK, EPI_NONE):
        c.append(_c("split15-conv-%s" % names[epi], "g", "f32", 3, 192, 160, epi, 130, 10, want="gemm_f32_kernel<3, ", slices=2))
    c.append(_c("split13-lin-defer", "g", "f32", 1, 192, 416, EPI_BIAS_LRELU, 130, defer=True, want="gemm_f32_kernel<1, ", slices=2))
    # the same shapes with the row count on the device: the cut is made there
    for m in (1, 129, 130):
        c.append(_c("dyn13-lin-m%d" % m, "g", "f32", 1, 192, 416, EPI_BIAS_LRELU, 130, rows=m, want="gemm_f32_kernel<1, ", slices=2, dyn=2))
    for m in (1, 12, 13):
        c.append(_c("dyn15-conv-m%d" % m, "g", "f32", 3, 192, 160, EPI_MASK, 130, 10, rows=m * 10, defer=(m == 12),
                    want="gemm_f32_kernel<3, ", slices=2, dyn=2))
    # few-rows kernel: both geometries, M at the minimum, M % 16 in {0, 1, 15}, direct and slabs, row map, device row count
    c.append(_c("rows45-M48", "g", "f32", 1, 12288, 64, EPI_BIAS, 48, want="gemm_rows_kernel<4, 5, false>", slices=1))
    c.append(_c("rows45-M65-map", "g", "f32", 1, 13056, 64, EPI_BIAS_LRELU, 65, rmap=True, want="gemm_rows_kernel<4, 5, false>", slices=1))
    c.append(_c("rows45-M79-rows", "g", "f32", 1, 13056, 128, EPI_NONE, 79, rows=50, rmap=True, want="gemm_rows_kernel<4, 5, false>", slices=1))
    c.append(_c("rows45-M97-two-row-blocks", "g", "f32", 1, 8192, 64, EPI_BIAS, 97, rows=96, want="gemm_rows_kernel<4, 5, false>", slices=1))
    c.append(_c("rows38-M128", "g", "f32", 1, 16384, 64, EPI_BIAS, 128, want="gemm_rows_kernel<3, 8, false>", slices=1))
    c.append(_c("rows38-M113-rows", "g", "f32", 1, 16384, 64, EPI_BIAS_LRELU, 113, rows=97, rmap=True, want="gemm_rows_kernel<3, 8, false>", slices=1))
    c.append(_c("rows-slabs-M64", "g", "f32", 1, 2048, 2112, EPI_BIAS, 64, defer=True, want="gemm_rows_kernel<", slices=None))
    c.append(_c("rows-slabs-M127-rows", "g", "f32", 1, 2048, 2112, EPI_NONE, 127, rows=100, defer=True, want="gemm_rows_kernel<", slices=None))
    # fp32 LDS-DMA kernel (>= 384 tiles of 128 x 128) and the 128 x 128 register-staged tile (>= 512 tiles, consumer takes slabs)
    c.append(_c("glds-lin-M897", "g", "f32", 1, 6144, 64, EPI_BIAS_LRELU, 897, want="gemm_glds_kernel<true, 1, ", slices=1))
    c.append(_c("glds-conv-M1000", "g", "f32", 3, 6144, 64, EPI_MASK, 1000, 10, want="gemm_glds_kernel<true, 3, ", slices=1))
    c.append(_c("glds-conv-M1024-rows", "g", "f32", 3, 6144, 64, EPI_BIAS, 1024, 16, rows=1008, want="gemm_glds_kernel<true, 3, ", slices=1))
    c.append(_c("tile128-conv-M897", "g", "f32", 3, 8192, 64, EPI_BIAS_LRELU, 897, 13, defer=True, want="gemm_f32_kernel<3, 1, 2, 2, 0, 32>", slices=1))
    c.append(_c("tile128-lin-M1000", "g", "f32", 1, 8192, 64, EPI_BIAS, 1000, defer=True, want="gemm_f32_kernel<1, 0, 2, 2, 0, 32>", slices=1))
    c.append(_c("tile128-conv-M1024", "g", "f32", 3, 8192, 64, EPI_MASK, 1024, 16, defer=True, want="gemm_f32_kernel<3, 2, 2, 2, 0, 32>", slices=1))
    # ... and the instantiations of the two that the cases above leave out (one M each)
    for taps, epi in ((1, EPI_BIAS), (1, EPI_NONE), (3, EPI_BIAS_LRELU), (3, EPI_NONE)):
        c.append(_c("glds-%s-%s" % ("lin" if taps == 1 else "conv", names[epi]), "g", "f32", taps, 6144, 64, epi, 900, 10 if taps == 3 else 1,
                    want="gemm_glds_kernel<true, %d, %d, " % (taps, epi), slices=1))
    for taps, epi, fam, tag in ((1, EPI_BIAS, 0, 1), (1, EPI_NONE, -1, 0), (1, EPI_BIAS_LRELU, -1, 1), (3, EPI_BIAS, -1, 0), (3, EPI_NONE, -1, 0)):
        c.append(_c("tile128-%s-%s-tag%d" % ("lin" if taps == 1 else "conv", names[epi], tag), "g", "f32", taps, 8192, 64, epi, 900,
                    10 if taps == 3 else 1, defer=True, family=fam, want="gemm_f32_kernel<%d, %d, 2, 2, %d, 32>" % (taps, epi, tag), slices=1))
    # launch_gemm_bf16: small and big kernel, one and three products, static and device-side cuts
    for prec in ("bf16x3", "bf16"):
        np_ = 3 if prec == "bf16x3" else 1
        c.append(_c("%s-small-lin-M65" % prec, "g", prec, 1, 192, 64, EPI_BIAS_LRELU, 65, want="gemm_bf16_kernel<1, 1, %d>" % np_, slices=1))
        c.append(_c("%s-small-conv-B7-T9" % prec, "g", prec, 3, 64, 128, EPI_MASK, 63, 9, want="gemm_bf16_kernel<3, 2, %d>" % np_, slices=1))
        c.append(_c("%s-split13-lin" % prec, "g", prec, 1, 192, 832, EPI_BIAS, 130, want="gemm_bf16_kernel<1, 0, %d>" % np_, slices=2))
        c.append(_c("%s-split15-conv-defer" % prec, "g", prec, 3, 192, 320, EPI_BIAS_LRELU, 130, 10, defer=True,
                    want="gemm_bf16_kernel<3, 1, %d>" % np_, slices=2))
        for m in (1, 129, 130):
            c.append(_c("%s-dyn13-lin-m%d" % (prec, m), "g", prec, 1, 192, 832, EPI_NONE, 130, rows=m, rmap=(m == 129),
                        want="gemm_bf16_kernel<1, 3, %d>" % np_, slices=2, dyn=2))
        c.append(_c("%s-big-lin-M1000" % prec, "g", prec, 1, 4096, 64, EPI_BIAS, 1000, want="gemm_bf16_big_kernel<1, 0, %d>" % np_, slices=1))
        c.append(_c("%s-big-conv-M897-rows" % prec, "g", prec, 3, 4096, 64, EPI_MASK, 897, 13, rows=884,
                    want="gemm_bf16_big_kernel<3, 2, %d>" % np_, slices=1))
        # ... and the remaining instantiations of the two kernels
        for taps, epi in ((3, EPI_BIAS), (3, EPI_NONE)):
            c.append(_c("%s-small-conv-%s" % (prec, names[epi]), "g", prec, 3, 192, 64, epi, 70, 10, want="gemm_bf16_kernel<3, %d, %d>" % (epi, np_),
                        slices=1))
        for taps, epi in ((1, EPI_NONE), (1, EPI_BIAS_LRELU), (3, EPI_BIAS), (3, EPI_BIAS_LRELU), (3, EPI_NONE)):
            c.append(_c("%s-big-%s-%s" % (prec, "lin" if taps == 1 else "conv", names[epi]), "g", prec, taps, 4096, 64, epi, 900,
                        10 if taps == 3 else 1, want="gemm_bf16_big_kernel<%d, %d, %d>" % (taps, epi, np_), slices=1))
    # gemm_bf16a: BN 64 / 128, bf16 / fp32 output, taps 1 / 3, all four epilogues, both reduce passes
    for i, epi in enumerate((EPI_BIAS, EPI_BIAS_LRELU, EPI_MASK, EPI_NONE)):
        for N in (192, 256):
            for ob in (False, True):
                c.append(_c("bf16a-conv-N%d-%s-%s" % (N, names[epi], "b" if ob else "f"), "a", "bf16", 3, N, 64, epi, 130, 10, out_bf16=ob,
                            want="gemm_glds_kernel<false, 3, %d, 128, %d, %s" % (epi, 128 if N == 256 else 64, _bool(ob)), slices=1))
    for i, epi in enumerate((EPI_BIAS, EPI_BIAS_LRELU, EPI_NONE)):
        for N in (192, 256):
            for ob in (False, True):
                c.append(_c("bf16a-lin-N%d-%s-%s" % (N, names[epi], "b" if ob else "f"), "a", "bf16", 1, N, 64, epi, (129, 257)[i % 2],
                            rmap=(i == 1), rows=(100 if i == 2 and ob else None), out_bf16=ob,
                            want="gemm_glds_kernel<false, 1, %d, 128, %d, %s" % (epi, 128 if N == 256 else 64, _bool(ob)), slices=1))
    c.append(_c("bf16a-split-conv-reduce-bf16", "a", "bf16", 3, 192, 320, EPI_BIAS_LRELU, 130, 10, out_bf16=True, allow_split=True,
                want="gemm_glds_kernel<false, 3, 1, 128, 64, false", slices=3))
    c.append(_c("bf16a-split-lin-reduce-f32", "a", "bf16", 1, 256, 832, EPI_BIAS, 129, allow_split=True, rows=77,
                want="gemm_glds_kernel<false, 1, 0, 128, 128, false", slices=3))
    c.append(_c("bf16a-split-lin-defer", "a", "bf16", 1, 256, 832, EPI_NONE, 129, allow_split=True, defer=True, out_bf16=True,
                want="gemm_glds_kernel<false, 1, 3, 128, 128, false", slices=3))
    c.append(_c("bf16a-mask-never-splits", "a", "bf16", 3, 192, 320, EPI_MASK, 130, 10, out_bf16=True, allow_split=True,
                want="gemm_glds_kernel<false, 3, 2, 128, 64, true", slices=1))
    # gemm_big.h: both instantiations, around the hand-over at 5376 rows, row count on the host and on the device (both kernels
    # are enqueued then and each looks at the count: exactly one of them must write)
    for N, epi, ob in ((320, EPI_BIAS_LRELU, True), (256, EPI_NONE, False)):
        for M in (5376, 5377, 5632):
            c.append(_c("big-N%d-M%d" % (N, M), "a", "bf16", 1, N, 64, epi, M, out_bf16=ob, family=0,
                        want="gemm_big_kernel<4, 4, 4, %d, %d, %s>" % (5 if N == 320 else 4, epi, _bool(ob)), slices=1))
        for m in (5375, 5376):
            c.append(_c("big-N%d-rows%d" % (N, m), "a", "bf16", 1, N, 64, epi, 5632, rows=m, out_bf16=ob, family=0,
                        want="gemm_big_kernel<4, 4, 4, %d, %d, %s>" % (5 if N == 320 else 4, epi, _bool(ob)), slices=1))
        c.append(_c("big-N%d-M5375-small-kernel" % N, "a", "bf16", 1, N, 64, epi, 5375, out_bf16=ob, family=0,
                    want="gemm_glds_kernel<false, 1, %d, 128, %d, %s" % (epi, 128 if N == 256 else 64, _bool(ob)), slices=1))
    return c


CASES = _cases()


def plan_case(k):
    rows = k.rows is not None
    if k.route == "g":
        return plan_launch_gemm(k.precision, k.taps, k.N, k.K, k.epi, k.M, rows, k.defer, k.family)
    return plan_gemm_bf16a(k.taps, k.N, k.K, k.epi, k.M, k.out_bf16, k.allow_split, k.family, rows, k.defer)


def case_mode(k):
    """The operand rounding of the twin for a case."""
    return "bf16" if k.route == "a" else k.precision


def rounded_scale(k):
    """Scale of the standard-normal A and w of a case's rounded variant (the bias keeps scale 1), or None when the case has none.
    K <= 256 throughout.  Where the output is bf16, the share of elements within `bound_out` of a rounding boundary has to stay
    under 5 %; that share is about 2 * bound / ulp_bf16(|out|) ~ n_terms^1.5 * 2^-16 / |out| * |sum|, a property of the term count
    alone when the output is the bare sum, so: with a bias the operands are scaled by 1/16 (the output is then of the bias's size,
    the accumulation error of the sum's), without one only taps * K <= 64 stays under the cap and the longer sums have the exact
    variant only (the same epilogues are covered with fp32 output on the other column width)."""
    if k.K > 256:
        return None
    if not plan_case(k).c_bf16:
        return 1.0
    if k.epi in (EPI_BIAS, EPI_BIAS_LRELU):
        return 1.0 / 16
    return 1.0 if k.taps * k.K <= 64 else None


def case_inputs(k, kind, seed=0):
    """Host inputs of a case: kind 'exact' (integers |.| <= 4, masks from {-1, 1}) or 'rounded' (standard normal, A and w times
    `rounded_scale`).  With a row map A has 7 rows more than M, so that some are never read."""
    import zlib
    rng = np.random.default_rng([seed, zlib.crc32(k.id.encode()), 0 if kind == "exact" else 1])
    a_rows = k.M + (7 if k.rmap else 0)
    if kind == "exact":
        draw = lambda sc, *s: rng.integers(-4, 5, size=s).astype(F32)
    else:
        draw = lambda sc, *s: (rng.standard_normal(size=s) * sc).astype(F32)
    sc = rounded_scale(k) if kind == "rounded" else 1.0
    A, w, bias = draw(sc, a_rows, k.K), draw(sc, k.taps, k.N, k.K), draw(1.0, k.N)
    aux = rng.choice(np.array([-1, 1], dtype=F32), size=(k.M, k.N)) if k.epi == EPI_MASK else None
    rmap = None
    if k.rmap:          # a permutation of the rows with some repeated and some never read
        rmap = rng.permutation(a_rows)[:k.M].astype(np.int32)
        rmap[1::5] = rmap[0]
    return A, w, bias, aux, rmap


def live_rows(k):
    return k.M if k.rows is None else k.rows
