"""Foot-skate clean-up on the device: gem_foot_lock against the numpy twin (tests/foot_lock_twin.py) on both
sides of the LDS switch and with both branches of the blend length, in a batch of separately allocated sequences with canaries around
the outputs; the bitwise-copy guarantees on the device's output; two calls give the same bytes; `lock_feet` and the command line; and
`foot_lock=True` end to end through the batch pipeline.

The twin is given the n and d BYTES of the device's ground record, so the comparison does not inherit the plane's 5e-14.  Tolerance
1e-10: the knee's s = sqrt(l1^2 - c^2) amplifies an error of 1e-15 in D by l / s; with D at least 1e-9 from l1 + l2 (MARGIN), s >= 3e-5
and the amplified error stays below 2e-11; every other quantity is a short fixed chain of operations with errors near 1e-15."""
import functools

import numpy as np
import pytest

import foot_lock_twin as T
from pipeline_checks import SIZE, sphere_centres, write_recording as _write_recording
from globalegomocap_amd.camera import DEFAULT_CALIBRATION

pytestmark = pytest.mark.gpu

TOL = 1e-10
MARGIN = 1e-9                  # no compared quantity of a test input may lie this close to tau_v, +-tau_h, l1 +- l2 or 1 + stretch
MARGIN_DEGENERATE = 0.5e-9     # ... and a direction's length not this close to the 1e-9 below which it is none (an exact 0 lies 1e-9 away)
MARGIN_SNAP = 0.5e-12          # ... and an anchor's height not this close to the 1e-12 below which it is on the plane
LAG = 5
BLENDS = (3, 8)
CANARY = -7.25


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import prepare
    return prepare._lift_engine(DEFAULT_CALIBRATION, 0)


@pytest.fixture(scope="module")
def L(env):
    from globalegomocap_amd import foot_lock
    return foot_lock


@functools.lru_cache(maxsize=None)
def _input(name):
    x = T.case_input(name)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _twin(name, blend, plane, options=()):
    """The twin's result on a case at the plane whose four doubles are the bytes `plane`: computed once, never changed."""
    nd = np.frombuffer(plane, dtype=np.float64)
    return T.lock(_input(name), nd[:3], nd[3], lag=LAG, blend=blend, **dict(options))


def _dev(env, a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(env.device)


def _run(env, L, names, blend, outputs=None, inputs=None, **options):
    """ground + lock on the device -> (the outputs on the host, the lock records, the ground records)."""
    from globalegomocap_amd import ground
    seqs = [_dev(env, _input(n)) for n in names] if inputs is None else inputs
    g = ground.ground_call(env, seqs, LAG)
    outs, rec = L.lock_call(env, seqs, g, LAG, blend=blend, outputs=outputs, **options)
    return [o.cpu().numpy() for o in outs], rec.cpu().numpy(), g.cpu().numpy()


def _record(row):
    from globalegomocap_amd import _capi
    return _capi.GemFootLockRecord.from_buffer_copy(np.ascontiguousarray(row).tobytes())


def _compare(name, blend, out, row, g_row, capsys, options=()):
    assert int(g_row[0]) == 0, name
    e = _twin(name, blend, g_row[2:6].tobytes(), options)
    assert e["margin"] > MARGIN and e["margin_degenerate"] > MARGIN_DEGENERATE and e["margin_snap"] > MARGIN_SNAP, \
        (name, e["margin"], e["margin_degenerate"], e["margin_snap"])
    r = _record(row)
    assert int(r.status) == e["status"], (name, r.status)
    for k in T.COUNTS:
        assert getattr(r, k) == e[k], (name, blend, k, getattr(r, k), e[k])
    worst = {k: abs(getattr(r, k) - e[k]) for k in T.FLOATS}
    worst["joints"] = float(np.abs(out - e["sequence"]).max())
    with capsys.disabled():
        print("%s, blend %d: %d + %d runs, %d lengthened, %d unreachable; largest differences from the twin: %s"
              % (name, blend, e["runs_right"], e["runs_left"], e["lengthened"], e["unreachable"], ", ".join("%s %.1e" % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v <= TOL, (name, blend, k, v)
    # the bitwise guarantees, on the device's output
    x = _input(name)
    others = [j for j in range(15) if j not in T.MOVED]
    assert np.array_equal(out[:, others].view(np.uint64), x[:, others].view(np.uint64)), name
    for side, (hip, kn, an, ft) in enumerate(T.LEGS):
        still = ~(e["delta"][:, side] != 0.0).any(axis=1)
        assert np.array_equal(out[still, kn:ft + 1].view(np.uint64), x[still, kn:ft + 1].view(np.uint64)), (name, side)
    if e["status"] == T.NO_CONTACT:
        assert np.array_equal(out.view(np.uint64), x.view(np.uint64)), name
    return e


@pytest.mark.parametrize("blend", BLENDS)
@pytest.mark.parametrize("name", list(T.WALKER_CASES) + list(T.LONG_STANCE) + list(T.HAND_MADE))
def test_device_against_the_twin(env, L, name, blend, capsys):
    outs, rec, g = _run(env, L, [name], blend)
    e = _compare(name, blend, outs[0], rec[0], g[0], capsys)
    if name in ("3 frames", "6 frames"):
        assert e["status"] == T.NO_CONTACT
    if name == "98 frames without noise":
        assert np.array_equal(outs[0].view(np.uint64), _input(name).view(np.uint64)) and e["delta_max"] == 0.0 and rec[0][5] == 0
    if name in T.LONG_STANCE:          # (the workgroup sums these two anchors)
        assert max(b - a + 1 for a, b in e["runs"][0]) == max(b - a + 1 for a, b in e["runs"][1]) + 4 == 1692 and e["runs_right"] == 16
    if name == "hip raised":
        assert e["kind"][T.HAND_FRAME, 0] == 2 and e["unreachable"] == 1
    if name == "target too near":
        assert e["kind"][T.HAND_FRAME, 0] == 3 and e["unreachable"] == 1


def test_the_gaps_take_both_branches_of_the_blend_length(env, L):
    """With blend 8 the walkers' gaps lie on both sides of 2 * blend."""
    from globalegomocap_amd import ground
    gaps = set()
    for name in ("98 frames", "the first length in the work buffer"):
        g = ground.ground_call(env, [_dev(env, _input(name))], LAG).cpu().numpy()[0]
        for runs in _twin(name, 8, g[2:6].tobytes())["runs"]:
            gaps |= {b[0] - a[1] for a, b in zip(runs, runs[1:])}
    assert min(gaps) < 16 <= max(gaps), sorted(gaps)


def test_a_batch_with_canaries_and_the_same_bytes_twice(env, L, capsys):
    import torch
    from globalegomocap_amd import _capi
    names = ["98 frames", "standing", "3 frames", "knee on the line", "the first length in the work buffer", "hip raised", "target too near",
             "513 frames"]
    inputs = [_dev(env, _input(n)) for n in names]
    nan = np.array(_input("40 frames"))
    nan[17, 13, 1] = np.nan
    inputs.insert(3, _dev(env, nan))          # its ground has no body direction: BAD_GROUND, copied, between two good neighbours
    blocks = [torch.full((len(x) + 2, 15, 3), CANARY, dtype=torch.float64, device=env.device) for x in inputs]
    outs, rec, g = _run(env, L, None, 3, outputs=[b[1:-1] for b in blocks], inputs=inputs)
    for b in blocks:
        edge = b.cpu().numpy()
        assert (edge[0] == CANARY).all() and (edge[-1] == CANARY).all()
    assert int(rec[3][0]) == _capi.FOOT_LOCK_BAD_GROUND and int(g[3][0]) == _capi.GROUND_NO_BODY and rec[3][15] == 40
    assert np.array_equal(outs[3].view(np.uint64), nan.view(np.uint64))
    assert int(rec[2][0]) == _capi.FOOT_LOCK_NO_CONTACT
    keep = [i for i in range(len(inputs)) if i != 3]
    for i, name in zip(keep, names):
        _compare(name, 3, outs[i], rec[i], g[i], capsys)
    # alone or in the batch: the same bytes; and a second call gives the same bytes again
    alone = _run(env, L, ["standing"], 3)
    assert alone[0][0].tobytes() == outs[1].tobytes() and alone[1][0].tobytes() == rec[1].tobytes()
    again = _run(env, L, None, 3, inputs=inputs)
    assert again[1].tobytes() == rec.tobytes()
    for a, b in zip(again[0], outs):
        assert a.tobytes() == b.tobytes()


def test_options_reach_the_kernel(env, L, capsys):
    for options in (dict(snap=False), dict(stretch=0.0), dict(min_run=6), dict(min_run=1)):
        outs, rec, g = _run(env, L, ["98 frames"], 3, **options)
        _compare("98 frames", 3, outs[0], rec[0], g[0], capsys, tuple(sorted(options.items())))


def test_lock_feet_and_refusals(env, L):
    import torch
    from globalegomocap_amd import _capi, ground
    x = _input("98 frames")
    found = L.lock_feet(env, x)
    outs, rec, g = _run(env, L, ["98 frames"], 3)
    assert found.status == "ok" and np.array_equal(found.sequence.cpu().numpy(), outs[0]) and found.record.tobytes() == rec[0].tobytes()
    assert found.ground.source == "plane" and found.slide_after_speed <= found.slide_before_speed / 10.0
    assert found.slide_before_speed == 25.0 * found.slide_before and found.frames == 98 and found.runs == (int(rec[0][1]), int(rec[0][2]))
    both = L.lock_feet(env, [x, _input("3 frames")], fps=50.0, lag=LAG, blend=3)
    assert [b.status for b in both] == ["ok", "no_contact"] and np.array_equal(both[0].sequence.cpu().numpy(), outs[0])
    assert np.array_equal(both[1].sequence.cpu().numpy(), _input("3 frames")) and both[0].fps == 50.0
    # a ground made elsewhere
    est = ground.estimate_ground(env, x)
    assert np.array_equal(L.lock_feet(env, x, ground=est).sequence.cpu().numpy(), outs[0])
    assert L.lock_feet(env, [x, x], ground=[est, est])[1].ground is est
    nan = np.array(x)
    nan[17, 13, 1] = np.nan
    with pytest.raises(ValueError, match="sequence 1 .*ground"):
        L.lock_feet(env, [x, nan])
    with pytest.raises(ValueError, match="no sequence"):
        L.lock_feet(env, [])
    with pytest.raises(TypeError, match="ground"):
        L.lock_feet(env, x, ground="yes")
    d = _dev(env, x)
    grec = ground.ground_call(env, [d], LAG)
    with pytest.raises(_capi.GemError, match="in place"):
        L.lock_call(env, [d], grec, LAG, outputs=[d])
    with pytest.raises(_capi.GemError, match="n_sequences"):
        L.lock_call(env, [], torch.empty(0, 48, dtype=torch.float64, device=env.device), LAG)
    for bad, word in ((dict(lag=0), "lag"), (dict(lag=5, tau_v=0.0), "tau_v"), (dict(lag=5, tau_h=float("nan")), "tau_h"), (dict(lag=5, min_run=0), "min_run"),
                      (dict(lag=5, blend=0), "blend"), (dict(lag=5, stretch=-0.1), "stretch")):
        with pytest.raises(_capi.GemError, match="gem_foot_lock: " + word):
            L.lock_call(env, [d], grec, **bad)


def test_cli_on_a_pose_pickle(env, L, tmp_path, capsys):
    import json
    import pickle
    x, clean = _input("98 frames"), _input("98 frames without noise")
    pkl, out = str(tmp_path / "result_pose.pkl"), str(tmp_path / "o" / "locked.pkl")
    with open(pkl, "wb") as f:
        pickle.dump({"estimated_pose": list(x), "optimized_pose": np.array(x), "mid_optimized_pose": list(clean)}, f)
    found = L._cli([pkl, "--out", out, "--sequence", "both", "--json", str(tmp_path / "o" / "lock.json")])
    text = capsys.readouterr().out
    assert list(found) == ["optimized", "estimated"] and "slide (m/s)" in text and "skate (m/s)" in text and "penetration (m)" in text
    d = pickle.load(open(out, "rb"))
    want = L.lock_feet(env, x).sequence.cpu().numpy()
    assert isinstance(d["optimized_pose"], np.ndarray) and isinstance(d["estimated_pose"], list) and len(d["estimated_pose"]) == 98
    assert np.array_equal(d["optimized_pose"], want) and np.array_equal(np.array(d["estimated_pose"]), want)
    assert np.array_equal(np.array(d["mid_optimized_pose"]), clean)
    j = json.load(open(str(tmp_path / "o" / "lock.json")))
    assert sorted(j) == ["estimated", "optimized"] and j["optimized"]["ground_after"]["skate"] <= j["optimized"]["ground_before"]["skate"] / 10.0
    L._cli([pkl, "--out", out])
    d = pickle.load(open(out, "rb"))
    assert np.array_equal(d["optimized_pose"], want) and np.array_equal(np.array(d["estimated_pose"]), x)


def test_outputs_write_the_locked_sequence(env, L, tmp_path):
    """`Outputs.write` on a walker with stances (the pipeline's small synthetic chunks have none): the optimised meshes stand on the
    locked sequence, which differs from the input; the estimated files are those of a call without the switch."""
    import filecmp
    import os
    from globalegomocap_amd import bvh, meshes, report
    x = _input("40 frames")
    want = L.lock_feet(env, x)
    locked = want.sequence.cpu().numpy()
    assert want.status == "ok" and want.changed > 20 and np.abs(locked - x).max() > 0.01
    for tag, switch in (("off", {}), ("on", dict(foot_lock=True))):
        o = report.Outputs(mesh_root=str(tmp_path / tag / "m"), bvh=str(tmp_path / tag / "b"), **switch)
        assert o.write(env, "d/studio/chunk_0", (x, _dev(env, x), None)) is None
    for tag, opt in (("off", x), ("on", locked)):
        base = tmp_path / tag / "m" / "studio" / "chunk_0"
        for f in (0, 17, 39):
            np.testing.assert_allclose(sphere_centres(str(base / "optimized_global" / ("out_%04d.ply" % f))), opt[f], rtol=0, atol=1e-9)
            np.testing.assert_allclose(sphere_centres(str(base / "input_global" / ("out_%04d.ply" % f))), x[f], rtol=0, atol=1e-9)
    for f in sorted(os.listdir(str(tmp_path / "off" / "m" / "studio" / "chunk_0" / "input_global"))):
        assert filecmp.cmp(str(tmp_path / "off" / "m" / "studio" / "chunk_0" / "input_global" / f),
                           str(tmp_path / "on" / "m" / "studio" / "chunk_0" / "input_global" / f), shallow=False), f
    same = [filecmp.cmp(str(tmp_path / "off" / "b" / "studio" / "chunk_0" / f), str(tmp_path / "on" / "b" / "studio" / "chunk_0" / f), shallow=False)
            for f in ("estimated.bvh", "optimized.bvh")]
    assert same == [True, False]
    meshes.release()
    bvh.release()


def test_foot_lock_end_to_end(env, L, golden, tmp_path, capsys):
    """optimize_directory(bvh=DIR, save=True, save_pose=DIR) on two chunks of 26 frames without and with foot_lock=True: without, the
    files are those of a call that does not name the switch; with it the `estimated` files are unchanged, the `optimized` meshes
    stand on `lock_feet`'s sequence, and result_pose.pkl holds foot_locked_pose beside an unchanged optimized_pose."""
    import filecmp
    import os
    import pickle
    import torch
    from globalegomocap_amd import prepare as P, whole_sequence as ws
    from helpers import sd_from_npz
    n = 2 * SIZE + 1
    hd, dd, traj, gtp = _write_recording(tmp_path / "rec", n, seed=23)
    rec = P.prepare_sequence(traj, hd, dd, None, 0, n, fps=25, test_size=SIZE, verbose=False, scale=1.0)
    root = str(tmp_path / "no_gt" / "studio")
    rec.write_chunks(root)
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False, ground_truth=False, save=True)
    runs = {}
    for tag, extra in (("plain", {}), ("off", dict(foot_lock=False)), ("on", dict(foot_lock=True))):
        torch.manual_seed(31)
        base = tmp_path / tag
        runs[tag] = ws.optimize_directory(root, DEFAULT_CALIBRATION, bvh=str(base / "b"), mesh_root=str(base / "m"), save_pose=str(base / "p"), **dict(kw, **extra))

    def files(tag):
        found = []
        for folder, _, names in os.walk(str(tmp_path / tag)):
            found += [os.path.relpath(os.path.join(folder, f), str(tmp_path / tag)) for f in names]
        return sorted(found)
    assert files("plain") == files("off") == files("on") and len(files("plain")) > 2 * (2 * SIZE + 2)
    for f in files("plain"):
        assert filecmp.cmp(str(tmp_path / "plain" / f), str(tmp_path / "off" / f), shallow=False), f
        if "input_global" in f or f.endswith("estimated.bvh"):
            assert filecmp.cmp(str(tmp_path / "plain" / f), str(tmp_path / "on" / f), shallow=False), f
    for k in (2, 3):
        assert np.array_equal(runs["on"][k], runs["plain"][k]) and np.array_equal(runs["off"][k], runs["plain"][k])
    names = sorted((c.name for c in rec.chunks), key=ws.natural_key)
    for k, name in enumerate(names):
        r_on, r_off = runs["on"][1][k], runs["plain"][1][k]
        assert list(r_on) == list(r_off) + ["foot_lock"] and "foot_lock" not in runs["on"][0] and "foot_lock" not in runs["off"][1][k]
        for key in r_off:
            assert np.array_equal(np.asarray(r_on[key]), np.asarray(r_off[key])), key
        opt = runs["plain"][3][k * SIZE:(k + 1) * SIZE]
        want = L.lock_feet(env, opt)
        assert r_on["foot_lock"] == want.as_dict()
        with capsys.disabled():
            print("%s: %s" % (name, want.line()))
        locked = want.sequence.cpu().numpy()
        for f in (0, SIZE - 1):
            c = sphere_centres(str(tmp_path / "on" / "m" / "studio" / name / "optimized_global" / ("out_%04d.ply" % f)))
            np.testing.assert_allclose(c, locked[f], rtol=0, atol=1e-9)
        d_on = pickle.load(open(str(tmp_path / "on" / "p" / name / "result_pose.pkl"), "rb"))
        d_off = pickle.load(open(str(tmp_path / "plain" / "p" / name / "result_pose.pkl"), "rb"))
        assert sorted(d_on) == sorted(list(d_off) + ["foot_locked_pose"])
        assert np.array_equal(np.asarray(d_on["optimized_pose"]), np.asarray(d_off["optimized_pose"]))
        assert np.array_equal(np.asarray(d_on["foot_locked_pose"]), locked) and type(d_on["foot_locked_pose"]) is type(d_on["optimized_pose"])
    ws.release_pools()
