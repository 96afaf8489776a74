"""The VAE decoder and its adjoint in float64, and which fused tail a network shape gets -- TEST INFRASTRUCTURE.

Decoder.  decoder_input (a linear layer whose output index is channel * T + frame), then three-tap convolutions in time with
zero padding, every one but the last followed by LeakyReLU(0.01); the last one's 45 outputs are the pose.  `Decoder64` holds the
folded weights of oracle/np_oracle.py::fold_vae (BatchNorm folded in, rounded to fp32: the values the device loads) widened to
float64 and works in float64 from there on: nothing follows the fp32 staging of the oracle or of the device code.  The adjoint
uses the twin's OWN LeakyReLU masks (pre-activation > 0).  tests/test_decoder_f64_cpu.py holds it to the oracle and to its own
central differences; tests/test_decoder_tails_gpu.py holds every instantiation of the fused tails to it.

Planner.  `decoder_layers` .. `predict` restate, without a device, which kernel a shape reaches (csrc/weights.hip: gem_load_vae;
csrc/tail.hip: plan_tail, tail_can_share_cu, plan_tail_for, launch_tail; csrc/tail_bf16.hip: plan_tail_bf16; csrc/stage.hip:
plan_route), as tests/gemm_twin.py restates the GEMM planners: the GPU test asserts the predicted name against the one the
library reports, so a drift between the two is a failing case, never a case that quietly runs a neighbouring kernel."""
from collections import namedtuple

import numpy as np

F64 = np.float64
SLOPE = 0.01
LDS_CU = 160 * 1024
TAIL_ROWS, TAIL_WAVES, TAIL_WAVES_SHARED, TAIL_MAX_LAYERS = 16, 8, 4, 6
MAX_JOINTS = 16
N_CU = 256


# ---- the decoder ------------------------------------------------------------------------------------------------------------------
def _shift(x, d):
    """x [B,T,C] -> y with y[:, t] = x[:, t + d], zero where t + d leaves the window."""
    y = np.zeros_like(x)
    T = x.shape[1]
    lo, hi = max(0, -d), min(T, T - d)
    y[:, lo:hi] = x[:, lo + d:hi + d]
    return y


def _conv(x, taps, bias):
    """out[t] = bias + sum_k x[t + k - 1] @ taps[k]"""
    return bias + sum(np.einsum("btc,cn->btn", _shift(x, k - 1), taps[k]) for k in range(3))


def _conv_adjoint(g, taps):
    """d/dx of <g, _conv(x)>: dx[s] = sum_k g[s - k + 1] @ taps[k]^T"""
    return sum(np.einsum("btn,cn->btc", _shift(g, 1 - k), taps[k]) for k in range(3))


Decoded = namedtuple("Decoded", "X pre")        # pose [B,T,15,3]; pre-activations of the LeakyReLU layers, each [B,T,C_i]


class Decoder64:
    def __init__(self, vae):
        self.T = int(vae.T)
        self.W_in, self.b_in = (np.asarray(a, dtype=F64) for a in vae.dec_in)
        self.layers = [(np.asarray(t, dtype=F64), np.asarray(b, dtype=F64)) for t, b in vae.dec]

    def decode(self, z):
        z = np.asarray(z, dtype=F64)
        B = z.shape[0]
        h = (z @ self.W_in.T + self.b_in).reshape(B, -1, self.T).transpose(0, 2, 1)
        pre = []
        for taps, bias in self.layers[:-1]:
            p = _conv(h, taps, bias)
            pre.append(p)
            h = np.where(p > 0, p, SLOPE * p)
        X = _conv(h, *self.layers[-1])
        return Decoded(X.reshape(B, self.T, -1, 3), pre)

    def adjoint(self, dX, pre):
        """dE/dX [B,T,15,3] -> dE/dz [B,D] at the point whose pre-activations are `pre`."""
        B = dX.shape[0]
        g = _conv_adjoint(np.asarray(dX, dtype=F64).reshape(B, self.T, -1), self.layers[-1][0])
        for (taps, _), p in zip(reversed(self.layers[:-1]), reversed(pre)):
            g = _conv_adjoint(g * np.where(p > 0, 1.0, SLOPE), taps)
        return g.transpose(0, 2, 1).reshape(B, -1) @ self.W_in


def relative_margin(pre):
    """Smallest |pre-activation| relative to the largest of its layer and window: [B]."""
    return np.min([np.abs(p).reshape(p.shape[0], -1).min(axis=1) / np.abs(p).reshape(p.shape[0], -1).max(axis=1) for p in pre], axis=0)


def relative_deviation(a, ref):
    """max |a - ref| / max |ref| per window: [B]."""
    B = ref.shape[0]
    return np.abs(np.asarray(a, dtype=F64) - ref).reshape(B, -1).max(axis=1) / np.abs(ref).reshape(B, -1).max(axis=1)


# ---- which tail a shape gets ------------------------------------------------------------------------------------------------------
def pad64(c):
    return (c + 63) // 64 * 64


def decoder_layers(hidden, channels=45):
    """(K, N) of every decoder conv as the device holds it (feature dimensions padded to 64), in execution order."""
    rev = [pad64(c) for c in reversed(hidden)]
    return [(rev[i], rev[i + 1]) for i in range(len(rev) - 1)] + [(rev[-1], rev[-1]), (rev[-1], pad64(channels))]


def tail_carve(layers, start, T, J=15, shared=False):
    """plan_tail: LDS bytes of the fp32 chain that starts at conv `start`, 0 where it is refused; and its tile bound."""
    n = len(layers) - start
    if start < 0 or n < 1 or n > TAIL_MAX_LAYERS or T > TAIL_ROWS:
        return 0, 0
    chain = layers[start:]
    if any(v not in (64, 128, 256, 512) for kn in chain for v in kn):
        return 0, 0
    G = TAIL_ROWS // T
    if shared and G != 1:
        return 0, 0
    rows = G * T if shared else TAIL_ROWS
    maxnt = 4 if not shared and max(max(kn) for kn in chain) > 32 * TAIL_WAVES else 2
    widths = [chain[0][0]] + [kn[1] for kn in chain]
    off = sum(rows * (w + 4) for w in widths)
    off += 2 * rows * (max(widths[1:]) + 4)
    off += G * 4 * ((T * J * 3 + 3) // 4 * 4)
    off += 64
    if G == 1:
        off += (T * J * 3 + 2 * J + J * MAX_JOINTS + 3) // 4 * 4
    return 4 * off, maxnt


def tail_start(layers, T, J=15):
    """gem_load_vae: the first start >= 1 whose carve fits one CU, -1 where every chain is refused."""
    for st in range(1, len(layers)):
        b, _ = tail_carve(layers, st, T, J)
        if b and b <= LDS_CU:
            return st
    return -1


def can_share_cu(layers, start, T, J=15):
    b, _ = tail_carve(layers, start, T, J, shared=True)
    return bool(b) and 3 * b <= LDS_CU and all(v <= 64 * TAIL_WAVES_SHARED for kn in layers[start:] for v in kn)


def tail_bf16_bytes(layers, start, T, J=15, nrt=5):
    """plan_tail_bf16: LDS bytes of the bf16 tail for the chain from `start` with `nrt` row tiles, 0 where it is refused."""
    n = len(layers) - start
    if start < 1 or n < 1 or n > 6 or T < 3 or T > 16 or nrt < 1 or nrt > 5 or 16 * nrt < T:
        return 0
    chain = layers[start:]
    if any(v not in (64, 128, 256) for kn in chain for v in kn) or chain[-1][1] != 64 or J * 3 > 64 or J > MAX_JOINTS:
        return 0
    rows = 16 * nrt
    G = min(8, rows // T)
    escr = (T * J * 3 + 3) // 4 * 4
    width = [chain[0][0]] + [kn[1] for kn in chain]
    ld = lambda w: 2 * w + 32
    size = [0, 0]
    for j, w in enumerate(width):
        size[j & 1] = max(size[j & 1], rows * ld(w))
    xb = (n - 1) & 1
    size[xb] = max(size[xb], rows * ld(width[n - 1]) + G * escr * 4)
    off = size[0] + size[1]
    for j in range(n):
        off += rows * (width[0] // 8 if j == 0 else width[j] // 4)
    off = (off + 15) // 16 * 16 + 1024 + 64
    off += G * MAX_JOINTS * 4 + (MAX_JOINTS + 1) * MAX_JOINTS * 4
    off = (off + 15) // 16 * 16 + 8 * 4
    if nrt <= 3:
        off += G * T * J * 5 * 4
    off = (off + 15) // 16 * 16 + 64
    return off if off <= 80 * 1024 else 0


Tail = namedtuple("Tail", "start NL maxnt waves kernel bf16 front")


def predict(hidden, T, B, waves_env=None, n_cu=N_CU):
    """The fp32 route of a call with B windows: Tail(start, NL, MAXNT, W, kernel name | None = the batched layers, whether the bf16
    tail exists for the chain, whether decoder_input and conv 0 were composed into one front product).  waves_env: the value of the
    developer switch GEM_TAIL_WAVES, None = unset."""
    layers = decoder_layers(hidden)
    st = tail_start(layers, T)
    if st < 0:
        return Tail(-1, 0, 0, 0, None, False, False)
    wgs = (B + 16 // T - 1) // (16 // T)
    share = can_share_cu(layers, st, T)
    bf16 = bool(tail_bf16_bytes(layers, st, T))
    if wgs > (10 if share else 5) * n_cu:
        return Tail(st, len(layers) - st, 0, 0, None, bf16, st == 1)
    shared = (wgs > n_cu and share) if waves_env is None else (int(waves_env) == TAIL_WAVES_SHARED and share)
    _, maxnt = tail_carve(layers, st, T, shared=shared)
    W = TAIL_WAVES_SHARED if shared else TAIL_WAVES
    return Tail(st, len(layers) - st, maxnt, W, "TailTiles<%d>::decoder_tail_kernel<%d, %d>" % (maxnt, len(layers) - st, W), bf16, st == 1)


# ---- the case table ---------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "hidden T B seed waves latent", defaults=(64,))      # waves: values of GEM_TAIL_WAVES to run (None: unset)

CHAINS_2 = ((64,), (64, 128), (64, 64, 128), (64, 64, 128, 256), (64, 64, 128, 256, 512), (64, 64, 64, 128, 256, 512))
CHAINS_4 = ((512,), (512, 512), (64, 512, 512), (64, 128, 512, 512), (64, 64, 128, 512, 512), (64, 64, 64, 128, 512, 512))
SEVEN_BLOCKS = (64, 64, 64, 64, 128, 256, 512)
REFUSED = (192, 192)            # 192 columns: no chain of this decoder passes plan_tail
W_ALL = (7e-3, 2e-2, 5e-2, 3e-3, 4e-2)
W_3D = (1.0, 0.0, 0.0, 0.0, 0.0)
HEAT = 64
LINE_ROOM = 2e-4                # texels: the float64 poses keep twice the distance from a texel line at which a window is left out
# The smallest |pre-activation| a case's inputs may have, relative to the largest of its layer and window: 16 x 9.2e-7, the largest
# fp32 pre-activation deviation on the table.  The condition is that no pre-activation lies within 8 x THE CASE'S OWN fp32 deviation
# of zero; choosing the seeds by this fixed figure of the float64 twin alone keeps the choice the same on every machine (the fp32
# oracle's deviation moves with the BLAS's summation order) and leaves every case at least 2 x the condition (22 x .. 310 x measured).
MARGIN = 1.5e-5


# fp32, through energy_grad.  Seeds: the first from 0 at which `seed_is_good` holds (test_decoder_f64_cpu.py asserts it, and that no
# earlier seed does).
FP32_CASES = (
    # every instantiation: TailTiles<2>::<NL, 8> and <NL, 4>, NL = 1 .. 6 (T = 10: one window per workgroup, the shared shape exists)
    Case(CHAINS_2[0], 10, 5, 2, ("8", "4")), Case(CHAINS_2[1], 10, 5, 1, ("8", "4")), Case(CHAINS_2[2], 10, 5, 14, ("8", "4")),
    Case(CHAINS_2[3], 10, 5, 1, ("8", "4")), Case(CHAINS_2[4], 10, 5, 7, ("8", "4")), Case(CHAINS_2[5], 10, 5, 2, ("8", "4")),
    # TailTiles<4>::<NL, 8>, NL = 1 .. 6: a 512-wide layer inside the chain
    Case(CHAINS_4[0], 10, 3, 2, (None,)), Case(CHAINS_4[1], 10, 3, 0, (None,)), Case(CHAINS_4[2], 10, 3, 1, (None,)),
    Case(CHAINS_4[3], 10, 3, 21, (None,)), Case(CHAINS_4[4], 10, 3, 6, (None,)), Case(CHAINS_4[5], 10, 3, 3, (None,)),
    # a 256-wide layer and a 256-wide adjoint in a four-tile chain: the two-tile walk of TailTiles<4> (L.N == 32 W, the switch's edge)
    Case((64, 256, 512, 512), 10, 3, 10, (None,)),
    # several windows per workgroup (T = 5: three, T = 8: two), the last workgroup ragged; NL = 1, 3, 6
    Case((64,), 5, 7, 0, (None,)), Case((64, 64, 128), 5, 7, 0, (None,)), Case(CHAINS_2[5], 5, 7, 0, (None,)),
    Case((64,), 8, 7, 0, (None,)), Case((64, 512, 512), 8, 7, 18, (None,)), Case(CHAINS_4[5], 8, 7, 5, (None,)),
    # the longest and the shortest window; NL = 2, 6
    Case((64, 128), 16, 3, 2, ("8", "4")), Case((512, 512), 3, 8, 2, (None,)),
    Case(CHAINS_4[5], 16, 3, 5, (None,)), Case(CHAINS_2[5], 3, 8, 1, (None,)),
    # seven blocks: the chain starts behind conv 1 -- no composed front, mask_first from a batched layer's output
    Case(SEVEN_BLOCKS, 10, 4, 9, ("8", "4")),
    # no chain passes plan_tail: the batched layers, same gates
    Case(REFUSED, 10, 4, 6, (None,)),
)
# one stage per chain length and tile bound: the front product's split-K slabs are summed by the tail (latent 512: K is cut)
STAGE_CASES = tuple(Case(h, 10, 5, 0, (None,), 512) for h in CHAINS_2 + CHAINS_4)
# bf16 tail, chain lengths 1 .. 6: the TailTiles<2> chains where plan_tail_bf16 accepts them (the six-layer chain ending in 256
# columns needs more than 80 KB at T = 10: a narrower six-layer chain stands in), row tiles 1 and 5
BF16_CASES = tuple(Case(h, 10, 11, 0, (None,)) for h in CHAINS_2[:5] + ((64, 64, 64, 64, 128, 256),)) + \
    tuple(Case(h, 5, 11, 0, (None,)) for h in CHAINS_2)

# What fp32 needs (measured by test_decoder_f64_cpu.py over FP32_CASES / STAGE_CASES: the fp32 numpy oracle against the twin) and
# the device's allowance, 4 x each: an MFMA 16x16x4 chain and the slab sums add in another order than numpy's dot product, not
# with more error (the convention of the training sweep).
MEASURED = dict(pose=2.24e-7, pre=9.22e-7, dz=4.03e-6, energy=6.34e-7)
GATES = {k: 4.0 * v for k, v in MEASURED.items()}
BF16_POSE_GATE = 3e-3           # test_hip_parity.test_precision_modes_energy_and_gradient: of max(1, max|X|)

_NETS = {}


def net(hidden, T, latent=64):
    """(shape, state dict, folded oracle VAE, float64 decoder, the walk's poses): random weights (seed 13, gain 1.7), the last
    layer's bias = the walk's mean pose, as test_energy_terms_gpu._net builds its networks."""
    from globalegomocap_amd import synth, vae as vae_schema
    from oracle import np_oracle as O
    key = (tuple(hidden), T, latent)
    if key not in _NETS:
        shape = vae_schema.VAEShape(latent_dim=latent, seq_len=T, hidden=tuple(hidden))
        est = np.asarray(synth.make_sequence(n_frames=T + 16, seed=21, with_heatmaps=False)["estimated_local_skeleton"], np.float32)
        sd = vae_schema.synthetic_state_dict(shape, 13, gain=1.7)
        sd["final_layer.3.bias"] = est.mean(axis=0).reshape(45).astype(np.float32)
        vae = O.fold_vae(sd, seq_len=T)
        _NETS[key] = (shape, sd, vae, Decoder64(vae), est)
    return _NETS[key]


def oracle_camera():
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    from oracle import np_oracle as O
    c = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    return O.Camera(poly=np.asarray(c.poly_w2c), cx=c.cx, cy=c.cy)


def make_inputs(case, seed=None):
    """The inputs of a case: windows cut from the walk (+- 1 cm), per-window mean bone lengths, heat-maps of uniform-random texels,
    z = the oracle encoder's mean + 0.1 N(0, 1); the twin's decode of z."""
    from globalegomocap_amd.skeleton import KINEMATIC_PARENTS
    from oracle import np_oracle as O
    shape, sd, vae, twin, est = net(case.hidden, case.T, case.latent)
    T, B = case.T, case.B
    rng = np.random.default_rng(case.seed if seed is None else seed)
    F = est.shape[0]
    starts = rng.integers(0, F - T + 1, B).astype(np.int32)
    pose = (np.stack([est[s:s + T] for s in starts]) + rng.normal(0.0, 0.01, (B, T, 15, 3))).astype(np.float32)
    parents = tuple(KINEMATIC_PARENTS)
    bones = np.linalg.norm(est - est[:, list(parents)], axis=-1).mean(axis=0)
    mb = (bones[None] * rng.uniform(0.9, 1.1, (B, 15))).astype(np.float32)
    heat = rng.random((F, HEAT, HEAT, 15), dtype=np.float32)
    mu, _ = O.encode(vae, pose.reshape(B, T, 45))
    z = (mu + 0.1 * rng.normal(size=mu.shape)).astype(np.float32)
    eps = rng.normal(size=mu.shape).astype(np.float32)
    return dict(case=case, T=T, B=B, shape=shape, sd=sd, vae=vae, twin=twin, parents=parents, starts=starts, pose=pose, mb=mb, heat=heat,
                z=z, eps=eps, cam=oracle_camera(), dec=twin.decode(z))


Cotangents = namedtuple("Cotangents", "E scale dX ix iy")


def energy_cotangents(inp, X, weights):
    """terms64 at the poses X [B,T,15,3]: Cotangents(E = weights . parts [B], scale = sum_k |weights[k] parts[k]| [B] -- the
    reprojection term is negative and cancels most of the others under W_ALL, so an energy's rounding is measured against the sum
    of the magnitudes, as test_energy_terms_gpu does --, dX = sum_k weights[k] dE_k/dX [B,T,15,3], texel coordinates ix, iy [B,T,15])."""
    from energy_f64 import terms64
    w = np.asarray(weights, dtype=F64)
    E, sc, dX, ix, iy = [], [], [], [], []
    for b in range(inp["B"]):
        s = inp["starts"][b]
        p, g, (x, y) = terms64(X[b], inp["pose"][b], inp["mb"][b], inp["heat"][s:s + inp["T"]], inp["cam"], inp["parents"])
        E.append(p @ w); sc.append(np.abs(p * w).sum()); dX.append(np.tensordot(w, g, axes=1)); ix.append(x); iy.append(y)
    return Cotangents(np.asarray(E), np.asarray(sc), np.stack(dX), np.stack(ix), np.stack(iy))


def oracle_deviations(inp):
    """What fp32 needs: the fp32 oracle (numpy, fp32 storage and products) against the twin on the case's inputs.  Returns
    dict(pose, pre, dz: the largest relative deviation over the windows; flips: LeakyReLU masks that differ; margin: the smallest
    pre-activation of the twin relative to its layer's and window's largest; line: the smallest distance of a pair of the twin's
    poses to a texel line)."""
    from energy_f64 import texel_line_distance
    from oracle import np_oracle as O
    vae, twin, dec, z = inp["vae"], inp["twin"], inp["dec"], inp["z"]
    h = np.transpose((z @ vae.dec_in[0].T + vae.dec_in[1]).astype(np.float32).reshape(z.shape[0], -1, vae.T), (0, 2, 1))
    pre32 = []
    for taps, b in vae.dec[:-1]:                   # the oracle's own layer functions, keeping what decode() drops
        p = O._conv3(np.ascontiguousarray(h), taps, b)
        pre32.append(p)
        h = O._lrelu(p)
    Xo, acts = O.decode(vae, z, keep=True)
    assert all(np.array_equal(a, O._lrelu(p)) for a, p in zip(acts, pre32))
    out = dict(pose=float(relative_deviation(Xo, dec.X).max()),
               pre=float(max(relative_deviation(p32, p64).max() for p32, p64 in zip(pre32, dec.pre)) if pre32 else 0.0),
               flips=int(sum(((p32 > 0) != (p64 > 0)).sum() for p32, p64 in zip(pre32, dec.pre))),
               margin=float(relative_margin(dec.pre).min()) if dec.pre else 1.0)
    dzs = []
    for w in (W_3D, W_ALL):
        dX = energy_cotangents(inp, Xo, w).dX
        dzs.append(relative_deviation(O.decode_backward(vae, dX.astype(np.float32), acts), twin.adjoint(dX, dec.pre)).max())
    out["dz"] = float(max(dzs))
    c = energy_cotangents(inp, dec.X, W_ALL)
    out["line"] = float(texel_line_distance(c.ix, c.iy).min())
    return out


def oracle_energy_deviation(inp, weights=W_ALL):
    """The fp32 oracle's energy at its own decode of z0 = latent_from_pose(pose, eps) against weights . terms64 at the twin's decode
    of the same z0: the largest |difference| / sum_k |w_k part_k| over the windows."""
    from oracle import np_oracle as O
    B, T = inp["B"], inp["T"]
    z0 = O.latent_from_pose(inp["vae"], inp["pose"].reshape(B, T, 45), inp["eps"])
    ref = energy_cotangents(inp, inp["twin"].decode(z0).X, weights)
    Xo = O.decode(inp["vae"], z0)
    E32 = [O.energy_and_grad(Xo[b], inp["pose"][b], inp["mb"][b], O.Weights(*weights), inp["cam"],
                             inp["heat"][inp["starts"][b]:inp["starts"][b] + T])[0] for b in range(B)]
    return float((np.abs(np.asarray(E32, dtype=F64) - ref.E) / ref.scale).max())


def seed_is_good(dev):
    """How a case's seed is chosen: every pre-activation of the twin at least MARGIN away from zero (relative), every pair LINE_ROOM
    away from a texel line.  Both are figures of the float64 twin alone."""
    return dev["margin"] >= MARGIN and dev["line"] >= LINE_ROOM


def inputs_are_good(inp):
    """seed_is_good from the inputs alone (no fp32 oracle: what a scan over seeds evaluates)."""
    from energy_f64 import texel_line_distance
    if inp["dec"].pre and relative_margin(inp["dec"].pre).min() < MARGIN:
        return False
    c = energy_cotangents(inp, inp["dec"].X, W_ALL)
    return bool(texel_line_distance(c.ix, c.iy).min() >= LINE_ROOM)


def margin_condition(dev):
    """The condition on a case's inputs: no pre-activation of the twin within 8 x the fp32 deviation of that case of zero, so that
    no implementation in fp32 takes the other LeakyReLU branch."""
    return dev["margin"] >= 8.0 * dev["pre"]
