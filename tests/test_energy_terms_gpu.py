"""Every device form of the window energy, term by term, against the float64 reference (tests/energy_f64.py) evaluated AT THE POSE
THE DEVICE DECODED -- so that only the energy code's own fp32 rounding is left between the two, in every precision mode.

The forms (csrc/energy_device.h: energy_window; csrc/energy_pairs.h: pair_terms) and the route that reaches each (read from
energy.hip, tail.hip, tail_bf16.hip; `energy_form` below restates it, `test_the_cases_reach_every_form` keeps the table complete):

  batched narrow layers + energy_kernel         T == 10: energy_window<true, 64, 10, 15>     else energy_window<true> (run time)
    (fp32 / bf16x3: GEM_TAIL_CAP=0; bf16: GEM_BATCHED_NARROW, gradient rows leave as bf16: gdst_b)
  fp32 fused tail, 16 // T == 1 (T = 9 .. 16)   T == 10: energy_window<true, THREADS, 10, 15> else energy_window<true, THREADS>
    THREADS = 512 (GEM_TAIL_WAVES=8) or 256 (the shape that shares a CU, GEM_TAIL_WAVES=4)
  fp32 fused tail, 16 // T >= 2 (T = 3 .. 8)    energy_window<false>: several windows per workgroup, one wavefront each
  bf16 tail, T == 10, 1 .. 3 row tiles          energy_pairs_wg<10, 15> (1 / 3 / 4 windows per workgroup)
  bf16 tail, T == 10, 4 / 5 row tiles           energy_pairs<10, 15, 3> (6 / 8 windows, one wavefront each)
  bf16 tail, T != 10                            energy_pairs<0, 0, 4>
(the one-wavefront-per-window form of energy_window belongs to SHORT windows, not to the shape that shares a CU -- that one needs
one window per workgroup --, and one row tile of ten frames runs energy_pairs_wg, not energy_pairs<10, 15, 3>.)
Every case confirms its route by kernel name (profile_kernels): a route that fell back would fail, not pass on other code.

The pose `energy_grad` returns is bit for bit the fp32 pose the energy code read, on every route: the batched layers write
ws.dec_act.back() and energy_kernel reads it (stage.hip: energy_args, decoder_bf16.hip: evaluate_bf16); the fp32 tail's last layer
stores one value `v` to LDS act[NL] and to Xp (tail.hip); the bf16 tail's last layer stores `v` to the dense LDS pose and to Xp
(tail_bf16.hip); gem_energy_grad copies ws.dec_act.back() out (unpack_pose_kernel: a plain copy).

Inputs.  Decoders whose last layer's bias is the walk's mean pose (random weights otherwise, the usual seeds, gain 1.7): the
decoded pose is that pose +- 10 .. 25 cm, windows 5 .. 10 cm apart, so bones have real lengths and the pairs land on the
heat-maps.  Heat-maps of uniform-random texels (neighbouring texels unrelated); per-window mean bone lengths; a second camera
placement whose principal point is moved so that the map's border runs through the joints (shares asserted from the returned
pose); the reference's skeleton and a star-shaped one (five and four children: the fourth-and-later-child loop of pair_terms).
Seven calls per case with one z: one-hot weights for each term, W_ALL, the production W_LOCAL.

Checks.  (a) parts and E against float64 at the returned pose, 1e-5 relative per term; parts bitwise the same in all seven calls
(the reprojection part is computed only where its weight is non-zero: 0.0 elsewhere).  (b) fp32 / bf16x3: each term's dE/dz against
the oracle's decoder adjoint applied to the float64 dE_k/dX, 2e-3 of max|dz_k|; the weighted calls against the weighted sum.  (c)
bf16: the tail's per-term dE/dz against the batched bf16 layers' (same rounding points), row-tile variants pairwise.

Measured on an MI355X (largest over the cases of a form).  (a) |part - float64| / |float64| per term (3-D, smoothness, bone, vae,
reprojection), gate 1e-5:
  energy_window<true,64,10,15>          8e-09 3e-08 2e-07 7e-09 6e-07      (+ gdst_b, bf16 mode: 1e-08 3e-08 2e-07 7e-09 4e-07)
  energy_window<true> (run time)        1e-08 5e-08 1e-07 1e-08 1e-06
  energy_window<true,512,10,15>         8e-09 2e-08 2e-07 6e-09 4e-07      <true,256,10,15>: 6e-09 1e-08 1e-07 6e-09 3e-07
  energy_window<true,512> / <true,256>  1e-08 2e-08 4e-08 4e-09 1e-06
  energy_window<false>                  2e-08 6e-08 9e-08 8e-09 5e-07
  energy_pairs_wg<10,15>, <10,15,3>     1e-08 3e-08 3e-07 1e-08 5e-07      (the same bits in both)
  energy_pairs<0,0,4>                   2e-08 5e-08 2e-07 2e-08 9e-07
(b) |dz_k - reference| / max|reference| per window, gate 2e-3: fp32 at most 2e-06 for the four smooth terms and 1.4e-05 for the
reprojection term on every form; bf16x3 at most 1.9e-05; the weighted calls against the weighted sums at most 1.5e-06 (bf16x3
1.9e-05).  No window had to be skipped.
(c) bf16 tail against the batched bf16 layers, per term and call: median 0, 99 % quantile at most 2.8e-3 (gate 2e-2; the bone
term of the star skeleton), smallest per-window cosine 0.999989 (gate 0.9995); row-tile variants pairwise: every quantile 0,
cosine 1 - 1e-7.  No single term came near a gate that was set for the sum.
Mutations of pair_terms tried on scratch builds (not kept): the stencil offset op2 reading the frame itself at t = T - 3 and
xa / xb swapped in one texel read fail every bf16 case here, and also the tail-against-batched tests that existed before; the
fourth-and-later-child subtraction dropped fails the three star cases here and nothing else in the suite.  Of energy_window: the
gather of a_(t+1) dropped at t = T - 3 fails every case here and half of test_hip_parity.py; heat_tap's right-border mask off
by one (x0i + 1 <= W) fails the five cases here whose shifted placement meets the right border and nothing in test_hip_parity.py.
"""
import dataclasses
import json
import re

import numpy as np
import pytest

from globalegomocap_amd import synth, vae as vae_schema
from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
from globalegomocap_amd.skeleton import KINEMATIC_PARENTS
from oracle import np_oracle as O
from helpers import TINY, FULL
from energy_f64 import terms64, texel_line_distance, project, heat_coords, TERMS

pytestmark = pytest.mark.gpu

W_LOCAL = (1e-6, 1e-5, 1e-2, 0.0, 1e-2)      # optimizer.py:355-358
W_ALL = (7e-3, 2e-2, 5e-2, 3e-3, 4e-2)
ONE_HOT = tuple(tuple(1.0 if i == k else 0.0 for i in range(5)) for k in range(5))
CALLS = ONE_HOT + (W_ALL, W_LOCAL)
STAR_PARENTS = (0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 6, 7, 8, 9, 10)      # joint 0: five children, joint 1: four
SKELETONS = {"kin": tuple(KINEMATIC_PARENTS), "star": STAR_PARENTS}
HEAT = 64
N_FRAMES_EXTRA = 16
FWD_GATE, GRAD_GATE = 1e-5, 2e-3
BF16_GATES = dict(median=1e-5, q99=2e-2, cos=0.9995)       # test_bf16_multi_window_tail_against_the_batched_bf16_layers

ROUTES = {
    "f32_batched": dict(precision="f32", env={"GEM_TAIL_CAP": "0"}),
    "f32_tail": dict(precision="f32", env={"GEM_TAIL_WAVES": "8"}),
    "f32_tail_shared": dict(precision="f32", env={"GEM_TAIL_WAVES": "4"}),
    "x3_batched": dict(precision="bf16x3", env={"GEM_TAIL_CAP": "0"}),
    "x3_tail": dict(precision="bf16x3", env={"GEM_TAIL_WAVES": "8"}),
    "bf16_batched": dict(precision="bf16", env={"GEM_TAIL16": "0", "GEM_BATCHED_NARROW": "1"}),
}
for _n in range(1, 6):
    ROUTES["bf16_tail_%d" % _n] = dict(precision="bf16", env={"GEM_TAIL16": "1", "GEM_TAIL16_NRT": str(_n)})
ROUTE_SWITCHES = ("GEM_TAIL_CAP", "GEM_TAIL_WAVES", "GEM_TAIL16", "GEM_TAIL16_NRT", "GEM_BATCHED_NARROW", "GEM_NO_TAIL")


def energy_form(route, T):
    """Which instantiation of the energy code the route runs for windows of T frames (see the module docstring)."""
    if route.endswith("batched"):
        return "energy_window<true,64,10,15>" + ("+gdst_b" if route.startswith("bf16") else "") if T == 10 else "energy_window<true>"
    if route.startswith("bf16_tail"):
        nrt = int(route[-1])
        return "energy_pairs<0,0,4>" if T != 10 else "energy_pairs_wg<10,15>" if nrt <= 3 else "energy_pairs<10,15,3>"
    if 16 // T >= 2:
        return "energy_window<false>"
    threads = 256 if route.endswith("shared") else 512
    return "energy_window<true,%d,10,15>" % threads if T == 10 else "energy_window<true,%d>" % threads


def check_kernel_names(route, names):
    """The kernels of family 1 (fused tails, energy kernel) the calls launched."""
    if route.endswith("batched"):
        assert "energy_kernel" in names and "decoder_tail" not in names, (route, names)
    elif route.startswith("bf16_tail"):
        m = re.search(r"decoder_tail_bf16_kernel<\w+, *(\d)", names)
        assert m and m.group(1) == route[-1] and "energy_kernel" not in names and "decoder_tail_kernel" not in names, (route, names)
    else:
        m = re.search(r"decoder_tail_kernel<\d, *(\d)>", names)
        waves = "4" if route.endswith("shared") else "8"
        assert m and m.group(1) == waves and "energy_kernel" not in names and "bf16_kernel" not in names, (route, names)


# (net, T, windows, skeleton, camera, seed, routes).  Windows: ragged against every grouping the routes use (fp32 tail: 16 // T per
# workgroup; bf16 tail: min(8, 16 * tiles // T)).  Seeds: bit 0 / bit 1 send the shifted placement to the right / bottom border (else
# left / top); the fp32 seeds are the first of their kind at which no pair of the ORACLE-decoded poses lies within 1e-3 texel of a
# texel line, so that the skipped-window cap of check (b) (1e-4, see _near_line) holds with room on the device's poses.
FP32_CASES = [
    ("tiny", 10, 5, "kin", "default", 5, ("f32_batched", "f32_tail", "f32_tail_shared", "x3_tail")),
    ("tiny", 10, 11, "star", "shifted", 90, ("f32_batched", "f32_tail", "x3_batched")),
    ("small", 12, 7, "kin", "shifted", 27, ("f32_batched", "f32_tail", "f32_tail_shared")),
    ("small", 16, 3, "kin", "default", 24, ("f32_batched", "f32_tail")),
    ("small", 5, 7, "kin", "shifted", 5, ("f32_batched", "f32_tail")),
    ("small", 5, 10, "star", "default", 6, ("f32_tail",)),
    ("small", 3, 13, "kin", "default", 15, ("f32_batched", "f32_tail")),
    ("full", 10, 3, "kin", "shifted", 44, ("f32_tail",)),
]
BF16_CASES = [
    ("tiny", 10, 13, "kin", "default", 11, ("bf16_tail_1", "bf16_tail_2", "bf16_tail_3", "bf16_tail_5")),
    ("tiny", 10, 11, "star", "shifted", 12, ("bf16_tail_1", "bf16_tail_2", "bf16_tail_3", "bf16_tail_4")),
    ("small", 12, 7, "kin", "shifted", 13, ("bf16_tail_1", "bf16_tail_3")),
    ("small", 16, 5, "star", "default", 14, ("bf16_tail_1", "bf16_tail_2")),
    ("small", 5, 19, "star", "shifted", 15, ("bf16_tail_1", "bf16_tail_2")),
    ("small", 3, 9, "kin", "default", 16, ("bf16_tail_1", "bf16_tail_2")),
    ("full", 10, 24, "kin", "shifted", 17, ("bf16_tail_1", "bf16_tail_2", "bf16_tail_5")),
]
_id = lambda c: "%s-T%d-B%d-%s-%s" % c[:5]


def test_the_cases_reach_every_form():
    reached = {energy_form(r, c[1]) for c in FP32_CASES for r in c[6]}
    reached |= {energy_form(r, c[1]) for c in BF16_CASES for r in c[6] + ("bf16_batched",)}
    assert reached >= {"energy_window<true,64,10,15>", "energy_window<true>", "energy_window<true,512,10,15>", "energy_window<true,512>",
                       "energy_window<true,256,10,15>", "energy_window<true,256>", "energy_window<false>",
                       "energy_window<true,64,10,15>+gdst_b", "energy_pairs_wg<10,15>", "energy_pairs<10,15,3>", "energy_pairs<0,0,4>"}
    star = {energy_form(r, c[1]).split("<")[0] for cases in (FP32_CASES, BF16_CASES) for c in cases if c[3] == "star" for r in c[6]}
    assert star >= {"energy_window", "energy_pairs_wg", "energy_pairs"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
_NETS = {}


def _net(net, T):
    """(shape, state dict, folded oracle VAE, the walk's poses): the usual random weights, the last layer's bias = the walk's mean pose."""
    if (net, T) not in _NETS:
        shape = {"tiny": TINY, "full": FULL}.get(net) or vae_schema.VAEShape(latent_dim=32, seq_len=T, hidden=(16, 16, 32, 32, 64))
        assert shape.seq_len == T
        est = np.asarray(synth.make_sequence(n_frames=T + N_FRAMES_EXTRA, seed=21, with_heatmaps=False)["estimated_local_skeleton"], np.float32)
        sd = vae_schema.synthetic_state_dict(shape, {"tiny": 11, "full": 5}.get(net, 13), gain=1.7)
        sd["final_layer.3.bias"] = est.mean(axis=0).reshape(45).astype(np.float32)
        _NETS[(net, T)] = (shape, sd, O.fold_vae(sd, seq_len=T), est)
    return _NETS[(net, T)]


def _classes(ix, iy):
    """(inside, in the one-texel band around the map and still touching it, fully outside) of every pair."""
    out = (ix < -1) | (ix >= HEAT) | (iy < -1) | (iy >= HEAT)
    inside = (ix >= 0) & (ix < HEAT - 1) & (iy >= 0) & (iy < HEAT - 1)
    return inside, ~inside & ~out, out


def _shifted_camera(cam, X, right, bottom):
    """The placement (principal point moved by whole quarter texels, towards the right / bottom border or the left / top one) that
    puts the map's border through the joints of the oracle-decoded poses X: the one with the most room above 20 % inside / 10 % in
    the border band / 10 % outside."""
    ix, iy = heat_coords(project(cam, X.reshape(-1, 3).astype(np.float64))[0], HEAT, HEAT)
    s = np.arange(0.0, 50.0, 0.25)
    x, y = ix[None] + (s if right else -s)[:, None], iy[None] + (s if bottom else -s)[:, None]
    xin, yin = ((x >= 0) & (x < HEAT - 1)).astype(np.float64), ((y >= 0) & (y < HEAT - 1)).astype(np.float64)
    xon, yon = ((x >= -1) & (x < HEAT)).astype(np.float64), ((y >= -1) & (y < HEAT)).astype(np.float64)
    n = ix.size
    inside, on = xin @ yin.T / n, xon @ yon.T / n
    score = np.minimum(np.minimum(inside / 0.2, (on - inside) / 0.1), (1.0 - on) / 0.1)
    i, j = np.unravel_index(np.argmax(score), score.shape)
    assert score[i, j] >= 1.5, score[i, j]
    return O.Camera(poly=cam.poly, cx=cam.cx + (s[i] if right else -s[i]) * 1024.0 / (HEAT - 1),
                    cy=cam.cy + (s[j] if bottom else -s[j]) * 1024.0 / (HEAT - 1))


def _inputs(case):
    net, T, B, skel, placement, seed = case[:6]
    shape, sd, vae, est = _net(net, T)
    parents = SKELETONS[skel]
    rng = np.random.default_rng(seed)
    F = est.shape[0]
    starts = rng.integers(0, F - T + 1, B).astype(np.int32)
    pose = (np.stack([est[s:s + T] for s in starts]) + rng.normal(0.0, 0.01, (B, T, 15, 3))).astype(np.float32)
    bones = np.linalg.norm(est - est[:, list(parents)], axis=-1).mean(axis=0)
    mb = (bones[None] * rng.uniform(0.9, 1.1, (B, 15))).astype(np.float32)
    heat = rng.random((F, HEAT, HEAT, 15), dtype=np.float32)
    mu, _ = O.encode(vae, pose.reshape(B, T, 45))
    z = (mu + 0.1 * rng.normal(size=mu.shape)).astype(np.float32)
    Xo, acts = O.decode(vae, z, keep=True)
    c = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    cam = O.Camera(poly=np.asarray(c.poly_w2c), cx=c.cx, cy=c.cy)
    if placement == "shifted":
        cam = _shifted_camera(cam, Xo, right=bool(seed & 1), bottom=bool(seed & 2))
    return dict(T=T, B=B, shape=shape, sd=sd, vae=vae, parents=parents, starts=starts, pose=pose, mb=mb, heat=heat, z=z, Xo=Xo, acts=acts,
                cam=cam, placement=placement)


# ---- the device -------------------------------------------------------------------------------------------------------------------
_DEVICE_ERROR = []


def _device_run(torch, monkeypatch, inp, route):
    """The seven calls on one route: E [7,B], parts [7,B,5], dz [7,B,D], X [B,T,15,3] (asserted bitwise the same in all seven).
    After a call that ended in a device or library error nothing more is started on the GPU by this module."""
    if _DEVICE_ERROR:
        pytest.fail("not run: an earlier case met a device error: %s" % _DEVICE_ERROR[0])
    try:
        return _seven_calls(torch, monkeypatch, inp, route)
    except AssertionError:
        raise
    except Exception as e:          # noqa: BLE001
        _DEVICE_ERROR.append(repr(e))
        raise


def _seven_calls(torch, monkeypatch, inp, route):
    from globalegomocap_amd import engine as engine_mod
    monkeypatch.setenv("GEM_DEV", "1")
    for k in ROUTE_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route]["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(engine_mod, "KINEMATIC_PARENTS", inp["parents"])      # (read when the engine is built)
    fc = dataclasses.replace(FisheyeCamera.from_json(DEFAULT_CALIBRATION), cx=float(inp["cam"].cx), cy=float(inp["cam"].cy))
    eng = engine_mod.WindowEngine(inp["shape"], fc, max_windows=inp["B"])
    eng.load_vae(0, inp["sd"])
    eng.set_precision(ROUTES[route]["precision"])
    eng.profile_enable(True)
    heat = torch.as_tensor(inp["heat"], device="cuda")
    E, parts, dz, X = [], [], [], None
    for w in CALLS:
        e, p, g, x = eng.energy_grad(0, inp["z"], inp["pose"], inp["mb"], engine_mod.energy_weights(*w), heat, inp["starts"])
        torch.cuda.synchronize()
        E.append(e.cpu().numpy()); parts.append(p.cpu().numpy()); dz.append(g.cpu().numpy())
        x = x.cpu().numpy()
        assert X is None or np.array_equal(X, x), "the decoded pose depends on the energy weights"
        X = x
    names = eng.profile_kernels(1)
    eng.close()
    check_kernel_names(route, names)
    return dict(E=np.stack(E), parts=np.stack(parts), dz=np.stack(dz), X=X, names=names)


# ---- the checks -------------------------------------------------------------------------------------------------------------------
def _reference(inp, X):
    """terms64 at the returned pose of every window: parts [B,5], dE_k/dX [5,B,T,15,3], texel coordinates [B,T,15] each."""
    parts, grads, ix, iy = [], [], [], []
    for b in range(inp["B"]):
        s = inp["starts"][b]
        p, g, (x, y) = terms64(X[b], inp["pose"][b], inp["mb"][b], inp["heat"][s:s + inp["T"]], inp["cam"], inp["parents"])
        parts.append(p); grads.append(g); ix.append(x); iy.append(y)
    return np.stack(parts), np.stack(grads, axis=1), np.stack(ix), np.stack(iy)


def _check_placement(inp, ix, iy, problems):
    inside, band, out = (c.mean() for c in _classes(ix, iy))
    if inp["placement"] == "shifted":
        if not (inside >= 0.2 and band >= 0.1 and out >= 0.1):
            problems.append(("border shares", inside, band, out))
    elif not inside >= 0.9:
        problems.append(("default placement: pairs inside", inside))
    return dict(inside=round(float(inside), 3), band=round(float(band), 3), outside=round(float(out), 3))


def _check_forward(res, ref_parts, problems):
    """(a): parts, their independence of the weights, E.  Returns the largest relative deviation per term."""
    parts, E = res["parts"], res["E"]
    with_reproj = [i for i, w in enumerate(CALLS) if w[4] != 0.0]
    for i, w in enumerate(CALLS):
        if not np.array_equal(parts[i][:, :4], parts[0][:, :4]):
            problems.append(("parts 0..3 differ between calls", i))
        if w[4] == 0.0 and parts[i][:, 4].any():
            problems.append(("reprojection part without its weight", i))
        if w[4] != 0.0 and not np.array_equal(parts[i][:, 4], parts[with_reproj[0]][:, 4]):
            problems.append(("reprojection part differs between calls", i))
    dev = np.concatenate([parts[0][:, :4], parts[with_reproj[0]][:, 4:]], axis=1)
    rel = np.abs(dev - ref_parts) / np.abs(ref_parts)
    for k in range(5):
        if not rel[:, k].max() <= FWD_GATE:
            problems.append(("part", TERMS[k], "window", int(rel[:, k].argmax()), float(rel[:, k].max()), "gate", FWD_GATE))
    for i, w in enumerate(CALLS):
        wv = np.asarray(w)
        p_dev = np.where(wv != 0, parts[i], 0.0)
        scale = np.abs(ref_parts * wv).sum(axis=1)
        if not (np.abs(E[i] - p_dev @ wv) <= 1e-12 * scale).all():
            problems.append(("E is not the weighted sum of the device's parts", i))
        if not (np.abs(E[i] - ref_parts @ wv) <= FWD_GATE * scale).all():
            problems.append(("E against float64", i, float((np.abs(E[i] - ref_parts @ wv) / scale).max())))
    return [float(v) for v in rel.max(axis=0)]


def _near_line(ix, iy, B):
    """Windows with a pair within 1e-4 texel of a texel line (float64, from the returned pose): there an fp32 floor may fall on the
    other side than numpy's, so the window is left out of the reprojection-bearing gradient comparisons; at most one in eight."""
    skip = (texel_line_distance(ix, iy).reshape(B, -1) < 1e-4).any(axis=1)
    return skip


def _check_gradient_fp32(inp, res, ref_grads, skip, problems):
    """(b): per-term dE/dz against the oracle's decoder adjoint of the float64 dE_k/dX; the weighted calls against the weighted sums."""
    B = inp["B"]
    if skip.sum() * 8 > B:
        problems.append(("windows near a texel line", int(skip.sum()), "of", B))
    worst = []
    for k in range(5):
        ref = O.decode_backward(inp["vae"], ref_grads[k].astype(np.float32), inp["acts"])
        keep = ~skip if k == 4 else np.ones(B, bool)
        err = np.abs(res["dz"][k] - ref)[keep].max(axis=1) / np.abs(ref)[keep].max(axis=1)
        worst.append(float(err.max()))
        if not err.max() <= GRAD_GATE:
            problems.append(("dz", TERMS[k], "window", int(np.flatnonzero(keep)[err.argmax()]), float(err.max()), "gate", GRAD_GATE))
    for i in (5, 6):
        mix = np.tensordot(np.asarray(CALLS[i]), res["dz"][:5].astype(np.float64), axes=1)
        err = np.abs(res["dz"][i] - mix)[~skip].max(axis=1) / np.abs(mix)[~skip].max(axis=1)
        worst.append(float(err.max()))
        if not err.max() <= GRAD_GATE:
            problems.append(("dz of call", i, "against the weighted sum of the one-hot calls", float(err.max())))
    return worst


def _bf16_statistics(a, b):
    """[median, 99 % quantile] of |a - b| / max|b| and the smallest per-window cosine."""
    q = np.quantile(np.abs(a - b).ravel() / np.abs(b).max(), [0.5, 0.99])
    cos = [float(np.dot(a[w], b[w]) / (np.linalg.norm(a[w]) * np.linalg.norm(b[w]) + 1e-30)) for w in range(a.shape[0])]
    return float(q[0]), float(q[1]), min(cos)


def _check_gradient_bf16(name, a, b, problems):
    """(c): one implementation against another fed the same rounding points, per call."""
    out = []
    for i in range(len(CALLS)):
        med, q99, cos = _bf16_statistics(a["dz"][i], b["dz"][i])
        out.append((med, q99, cos))
        if not (med <= BF16_GATES["median"] and q99 <= BF16_GATES["q99"] and cos > BF16_GATES["cos"]):
            problems.append((name, "call", i, "median", med, "q99", q99, "cos", cos))
    return out


@pytest.mark.parametrize("case", FP32_CASES, ids=_id)
def test_fp32_routes_term_by_term(torch_cuda, monkeypatch, case):
    inp = _inputs(case)
    problems, report = [], {}
    for route in case[6]:
        res = _device_run(torch_cuda, monkeypatch, inp, route)
        ref_parts, ref_grads, ix, iy = _reference(inp, res["X"])
        rec = dict(form=energy_form(route, inp["T"]), shares=_check_placement(inp, ix, iy, problems))
        here = []
        rec["parts"] = _check_forward(res, ref_parts, here)
        rec["dz"] = _check_gradient_fp32(inp, res, ref_grads, _near_line(ix, iy, inp["B"]), here)
        problems += [(route,) + tuple(p) for p in here]
        report[route] = rec
    print("ENERGY_TERMS " + json.dumps({"case": _id(case), "routes": report}))
    assert not problems, problems


@pytest.mark.parametrize("case", BF16_CASES, ids=_id)
def test_bf16_routes_term_by_term(torch_cuda, monkeypatch, case):
    inp = _inputs(case)
    problems, report, results = [], {}, {}
    for route in ("bf16_batched",) + case[6]:
        res = results[route] = _device_run(torch_cuda, monkeypatch, inp, route)
        ref_parts, _, ix, iy = _reference(inp, res["X"])
        here = []
        rec = dict(form=energy_form(route, inp["T"]), shares=_check_placement(inp, ix, iy, here))
        rec["parts"] = _check_forward(res, ref_parts, here)
        problems += [(route,) + tuple(p) for p in here]
        report[route] = rec
    tails = case[6]
    for i, route in enumerate(tails):
        report[route]["vs_batched"] = _check_gradient_bf16(route + " against the batched layers", results[route], results["bf16_batched"], problems)
        for other in tails[i + 1:]:
            report[route]["vs_" + other] = _check_gradient_bf16(route + " against " + other, results[route], results[other], problems)
    print("ENERGY_TERMS " + json.dumps({"case": _id(case), "routes": report}))
    assert not problems, problems
