"""Every instantiation of the fused decoder tails against the float64 decoder twin (tests/decoder_f64.py), over every chain length.

The fp32 tail is compiled 18 times, TailTiles<MAXNT>::decoder_tail_kernel<NL, W> (csrc/tail.hip: NL = 1 .. 6 fused layers, W = 8
waves or 4 for the shape that shares a CU, MAXNT = 2 or 4 tiles per wave); its layer loops unroll per NL, its weight prefetch
hands each layer its successor with edge rules at both ends of the chain, its tile walk switches on the layer width.  The bf16
tail (csrc/tail_bf16.hip) takes its chain length at run time and carries weight fragments across layer boundaries in a register
ring whose phase depends on the chain.  decoder_f64.FP32_CASES reaches all 18 (test_decoder_f64_cpu.py asserts it), BF16_CASES
chain lengths 1 .. 6; every case PREDICTS its kernel from the shape (decoder_f64.predict, restated from the planners) and asserts
the prediction against the name the library reports, so a shape that fell back to other code fails.

fp32, through energy_grad (two calls with one z: the one-hot 3-D term -- a dense, smooth cotangent -- and W_ALL on heat-maps of
random texels):
  pose   against the twin's pose, of max|X| per window, allowance GATES["pose"] = 9.0e-7
  dE/dz  against the twin's adjoint (its own LeakyReLU masks) of energy_f64.terms64's dE/dX AT THE DEVICE'S POSE, of max|dE/dz|
         per window, allowance GATES["dz"] = 1.6e-5; W_ALL: windows with a pair within 1e-4 texel of a texel line are left out,
         at most one in eight (the seeds leave out none)
  where both wave shapes exist, pose and dE/dz are bitwise equal between them.
The allowances are 4 x what the fp32 numpy oracle needs on the same inputs (test_decoder_f64_cpu.py measures it); the inputs
keep every pre-activation 8 x that deviation away from zero, so no window is left out on account of a LeakyReLU branch.
The slab hand-over, one stage per chain length and MAXNT (latent 512, so that the front product is cut along K and leaves its
slabs to the tail, which sums them and applies bias and LeakyReLU while staging): round 0's closure value against the float64
energy of the twin's pose at the z the device's encoder returned, of sum_k |w_k part_k|, allowance GATES["energy"] = 2.5e-6.
bf16: the tail with 1 and 5 row tiles against the batched bf16 layers (same rounding points) at test_energy_terms_gpu.BF16_GATES,
the pose of every route against the twin at 3e-3 of max(1, max|X|).

Every case takes 0.1 .. 0.3 s on an MI355X.  No window had to be left out of any fp32 comparison.

Measured on an MI355X, as shares of the allowances (largest over the cases of a family; the smallest in brackets):
                                    pose          dE/dz, 3-D term   dE/dz, W_ALL
  TailTiles<2>::<NL, 8>, <NL, 4>    0.34 (0.09)   0.17 (0.04)       0.49 (0.23)       (the two wave shapes: the same bits, every case)
  TailTiles<4>::<NL, 8>             0.72 (0.10)   0.19 (0.09)       0.62 (0.21)
  batched layers (refused shape)    0.40          0.07              0.38
  stage, round 0's closure value    0.31 (0.06)   front product gem::gemm_f32_kernel<1, 1, 1, 1, 1, 32>, K cut in 2, in all 12
  bf16, pose against the twin       0.63 of 3e-3 (the batched layers and the tail alike)
  bf16, tail against batched        median 0; 99 % quantile at most 2.8e-3 (gate 2e-2); smallest cosine 0.99997 (gate 0.9995);
                                    1 and 5 row tiles: the same figures to every digit, all 12 cases
Nothing in the sweep was wrong: all 18 fp32 instantiations and bf16 chains 1 .. 6 compute what the twin computes.
One bf16 case (64x64x128x256x512, T = 5) first missed the cosine gate under W_ALL (0.99933; 99 % quantile 1.8e-2) while its 3-D
call sat at 0.99999: in ONE of its 11 windows a pair of the tail's pose falls into another texel of the random heat-maps than the
batched layers' pose, so the two sides were handed different dE/dX.  Without that window: 1.3e-3 and 0.999997.  Hence the
texel rule between the two routes in test_bf16_tail_over_the_chain_lengths (at most one window in eight, reported per case; no
other case leaves one out); BF16_GATES are unchanged.

Mutations of tail.hip tried on scratch builds (not kept), fp32 cases and stages:
  the prefetch behind the last forward layer takes a.bwd[0] instead of a.bwd[NL - 1]: red in all 20 tail cases with NL >= 2 (dE/dz;
    with NL = 1 the two are the same layer); the stages stay green -- round 0's closure value is forward arithmetic only.
  the switch L.N > 32 * W in tail_gemm moved to L.N > 64 * W (a wide layer walks two tiles too few): red in the two <NL, 4> cases
    with a 256-wide layer, in all 11 TailTiles<4> cases, and in the stage of 512x512.  The issue's form of this mutation, `>=`,
    makes a layer of exactly 32 W columns walk tiles PAST its weights and past its row of g_out: an out-of-bounds kernel, not run
    on a device.  The cases that meet that edge are in the table (a 128-wide layer under W = 4; a 256-wide layer and adjoint under
    TailTiles<4>: 64x256x512x512, added for it -- test_decoder_f64_cpu.py asserts the widths met per family).
  the mask of layer 0 dropped (mask_first ignored): red in all 24 tail cases (dE/dz), green in the refused shape and the stages.
The device's LeakyReLU masks are not read anywhere: the margin condition on the inputs makes that unnecessary.
"""
import json
import re

import numpy as np
import pytest

import decoder_f64 as D
import gemm_twin as G
from energy_f64 import texel_line_distance
from test_energy_terms_gpu import BF16_GATES, _bf16_statistics

pytestmark = pytest.mark.gpu

ROUTE_SWITCHES = ("GEM_TAIL_CAP", "GEM_TAIL_WAVES", "GEM_TAIL16", "GEM_TAIL16_NRT", "GEM_BATCHED_NARROW", "GEM_NO_TAIL", "GEM_NO_FRONT")
CALLS = (D.W_3D, D.W_ALL)
_id = lambda c: "%s-T%d-B%d" % ("x".join(str(h) for h in c.hidden), c.T, c.B)
_INPUTS = {}
_DEVICE_ERROR = []


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch


def _inputs(case):
    """Computed once per case and left unchanged."""
    if case not in _INPUTS:
        _INPUTS[case] = D.make_inputs(case)
    return _INPUTS[case]


def _on_device(fn, *args):
    """After a call that ended in a device or library error nothing more is started on the GPU by this module."""
    if _DEVICE_ERROR:
        pytest.fail("not run: an earlier case met a device error: %s" % _DEVICE_ERROR[0])
    try:
        return fn(*args)
    except AssertionError:
        raise
    except Exception as e:          # noqa: BLE001
        _DEVICE_ERROR.append(repr(e))
        raise


def _engine(monkeypatch, inp, env, precision):
    from globalegomocap_amd import engine as engine_mod
    from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
    monkeypatch.setenv("GEM_DEV", "1")               # developer switches are honoured only with GEM_DEV=1
    for k in ROUTE_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = engine_mod.WindowEngine(inp["shape"], FisheyeCamera.from_json(DEFAULT_CALIBRATION), max_windows=inp["B"])
    eng.load_vae(0, inp["sd"])                       # the route is chosen when the weights are loaded
    eng.set_precision(precision)
    eng.profile_enable(True)
    return eng, engine_mod.energy_weights


def _two_calls(torch, monkeypatch, inp, env, precision):
    """energy_grad under the one-hot 3-D weights and under W_ALL: X [B,T,15,3] (the same bits in both), dz [2,B,D], kernel names."""
    eng, weights = _engine(monkeypatch, inp, env, precision)
    heat = torch.as_tensor(inp["heat"], device="cuda")
    dz, X = [], None
    for w in CALLS:
        _, _, g, x = eng.energy_grad(0, inp["z"], inp["pose"], inp["mb"], weights(*w), heat, inp["starts"])
        torch.cuda.synchronize()
        dz.append(g.cpu().numpy())
        x = x.cpu().numpy()
        assert X is None or np.array_equal(X, x), "the decoded pose depends on the energy weights"
        X = x
    names = eng.profile_kernels(1)
    eng.close()
    return dict(X=X, dz=np.stack(dz), names=names)


def _one_stage(torch, monkeypatch, inp):
    eng, weights = _engine(monkeypatch, inp, {}, "f32")
    heat = torch.as_tensor(inp["heat"], device="cuda")
    z = eng.encode(0, inp["pose"], inp["eps"])[2].cpu().numpy()
    eng.profile_kernels(0)                           # (the encoder's products: not the stage's)
    _, stats = eng.optimize_stage(0, inp["pose"], inp["mb"], inp["eps"], weights(*D.W_ALL), heat, inp["starts"])
    torch.cuda.synchronize()
    res = dict(z=z, status=stats.cpu().numpy()[:, 3], trace=eng.read_trace(inp["B"]), front=eng.profile_kernels(0), names=eng.profile_kernels(1))
    eng.close()
    return res


def _tail_kernels(names):
    return set(re.findall(r"TailTiles<\d>::decoder_tail_kernel<\d, \d>", names))


def _check_fp32_names(tail, names):
    if tail.kernel is None:
        assert "energy_kernel" in names and "decoder_tail" not in names, names
    else:
        assert _tail_kernels(names) == {tail.kernel} and "energy_kernel" not in names and "bf16_kernel" not in names, (tail.kernel, names)


@pytest.mark.parametrize("case", D.FP32_CASES, ids=_id)
def test_fp32_tail_against_the_float64_decoder(torch_cuda, monkeypatch, case):
    inp = _inputs(case)
    twin, dec, B = inp["twin"], inp["dec"], inp["B"]
    problems, report, results = [], {}, {}
    for waves in case.waves:
        tail = D.predict(case.hidden, case.T, B, waves)
        res = results[waves] = _on_device(_two_calls, torch_cuda, monkeypatch, inp, {} if waves is None else {"GEM_TAIL_WAVES": waves}, "f32")
        _check_fp32_names(tail, res["names"])
        pose = D.relative_deviation(res["X"], dec.X)
        rec = dict(kernel=tail.kernel, pose=float(pose.max() / D.GATES["pose"]))
        if not pose.max() <= D.GATES["pose"]:
            problems.append((waves, "pose", "window", int(pose.argmax()), float(pose.max()), "allowance", D.GATES["pose"]))
        for i, (w, key) in enumerate(zip(CALLS, ("dz_3d", "dz_all"))):
            cot = D.energy_cotangents(inp, res["X"], w)
            keep = np.ones(B, bool)
            if key == "dz_all":
                keep = ~(texel_line_distance(cot.ix, cot.iy).reshape(B, -1) < 1e-4).any(axis=1)
                if (~keep).sum() * 8 > B:
                    problems.append((waves, "windows near a texel line", int((~keep).sum()), "of", B))
            err = D.relative_deviation(res["dz"][i], twin.adjoint(cot.dX, dec.pre))
            rec[key] = float(err[keep].max() / D.GATES["dz"]) if keep.any() else None
            if keep.any() and not err[keep].max() <= D.GATES["dz"]:
                problems.append((waves, key, "window", int(np.flatnonzero(keep)[err[keep].argmax()]), float(err[keep].max()), "allowance", D.GATES["dz"]))
        report[str(waves)] = rec
    if len(case.waves) == 2:
        a, b = (results[w] for w in case.waves)
        if not (np.array_equal(a["X"], b["X"]) and np.array_equal(a["dz"], b["dz"])):
            problems.append(("the two wave shapes differ", float(np.abs(a["X"] - b["X"]).max()), float(np.abs(a["dz"] - b["dz"]).max())))
    print("DECODER_TAILS " + json.dumps({"case": _id(case), "share_of_allowance": report}))
    assert not problems, problems


@pytest.mark.parametrize("case", D.STAGE_CASES, ids=_id)
def test_slab_hand_over_in_a_stage(torch_cuda, monkeypatch, case):
    inp = _inputs(case)
    tail = D.predict(case.hidden, case.T, case.B)
    front = G.plan_launch_gemm("f32", 1, case.T * D.decoder_layers(case.hidden)[0][1], D.pad64(case.latent), G.EPI_BIAS_LRELU, case.B,
                               rows=True, defer=True, family=0)
    assert front.deferred, front
    res = _on_device(_one_stage, torch_cuda, monkeypatch, inp)
    assert _tail_kernels(res["names"]) == {tail.kernel}, (tail.kernel, res["names"])
    assert front.kernels[0] in res["front"], (front, res["front"])
    assert (res["status"] == 1).all(), ("a window did not finish", res["status"])
    ref = D.energy_cotangents(inp, inp["twin"].decode(res["z"]).X, D.W_ALL)
    err = np.abs(res["trace"][:, 0] - ref.E) / ref.scale
    print("DECODER_TAILS " + json.dumps({"case": _id(case), "stage": dict(kernel=tail.kernel, front=front.kernels[0], slices=front.n_slices,
                                                                            share_of_allowance=float(err.max() / D.GATES["energy"]))}))
    assert err.max() <= D.GATES["energy"], (err, D.GATES["energy"])


def _texels(inp, X):
    """The texel (floor of the heat-map coordinates) of every pair of the poses X: [B,T,15,2] integers."""
    c = D.energy_cotangents(inp, X, D.W_ALL)
    return np.stack([np.floor(c.ix), np.floor(c.iy)], axis=-1).astype(np.int64)


def _check_bf16_names(nrt, names):
    if nrt is None:
        assert "energy_kernel" in names and "decoder_tail" not in names, names
    else:
        m = re.search(r"decoder_tail_bf16_kernel<\w+, *(\d)", names)
        assert m and int(m.group(1)) == nrt and "energy_kernel" not in names and "decoder_tail_kernel" not in names, (nrt, names)


@pytest.mark.parametrize("case", D.BF16_CASES, ids=_id)
def test_bf16_tail_over_the_chain_lengths(torch_cuda, monkeypatch, case):
    inp = _inputs(case)
    tail = D.predict(case.hidden, case.T, case.B)
    assert tail.bf16, tail
    X64 = inp["dec"].X
    problems, report, results = [], {"chain": tail.NL}, {}
    for nrt in (None, 1, 5):
        env = {"GEM_TAIL16": "0", "GEM_BATCHED_NARROW": "1"} if nrt is None else {"GEM_TAIL16": "1", "GEM_TAIL16_NRT": str(nrt)}
        res = results[nrt] = _on_device(_two_calls, torch_cuda, monkeypatch, inp, env, "bf16")
        _check_bf16_names(nrt, res["names"])
        res["texel"] = texel = _texels(inp, res["X"])
        err = np.abs(res["X"] - X64).reshape(case.B, -1).max(axis=1) / np.maximum(1.0, np.abs(X64).reshape(case.B, -1).max(axis=1))
        rec = report["batched" if nrt is None else "nrt%d" % nrt] = dict(pose=float(err.max() / D.BF16_POSE_GATE))
        if not err.max() <= D.BF16_POSE_GATE:
            problems.append((nrt, "pose", float(err.max())))
        if nrt is not None:
            # W_ALL: the texel-line rule between the two routes.  Their poses differ where a bf16 rounding fell the other way (1e-4 ..
            # 1e-3 m, up to 0.03 texel); a window in which a pair then reads another texel patch of the random heat-maps has another
            # dE/dX on the two sides, which says nothing about the adjoint: left out, at most one in eight.
            apart = (texel != results[None]["texel"]).reshape(case.B, -1).any(axis=1)
            rec["windows_in_other_texels"] = int(apart.sum())
            if apart.sum() * 8 > case.B:
                problems.append((nrt, "windows whose pairs fall into other texels than the batched layers'", int(apart.sum()), "of", case.B))
            for i, key in enumerate(("dz_3d", "dz_all")):
                keep = ~apart if key == "dz_all" else np.ones(case.B, bool)
                med, q99, cos = _bf16_statistics(res["dz"][i][keep], results[None]["dz"][i][keep])
                if not keep.all():
                    rec[key + "_every_window"] = _bf16_statistics(res["dz"][i], results[None]["dz"][i])
                rec[key] = (med, q99, cos)
                if not (med <= BF16_GATES["median"] and q99 <= BF16_GATES["q99"] and cos > BF16_GATES["cos"]):
                    problems.append((nrt, key, "median", med, "q99", q99, "cos", cos))
    print("DECODER_TAILS " + json.dumps({"case": _id(case), "bf16": report}))
    assert not problems, problems
