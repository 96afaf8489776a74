"""The ground plane from foot contacts on the device: gem_ground_plane against the numpy twin
(tests/ground_twin.py) on both sides of its LDS switch, in a batch of separately allocated sequences and behind a transform that is
applied first; two calls give the same bytes; gem_similarity_compose against numpy; the writers' `move`; and `upright=True` end to
end through the batch pipeline."""
import functools

import numpy as np
import pytest

import ground_twin as T
from pipeline_checks import SIZE, sphere_centres, write_recording as _write_recording
from globalegomocap_amd.camera import DEFAULT_CALIBRATION
from globalegomocap_amd.synth_walk import _rotvec_matrix

pytestmark = pytest.mark.gpu

# An eigenvector's error is about eps |S| / (lambda_mid - lambda_min): on these inputs 2e-16 * 2 m^2 / 0.01 m^2 = 4e-14, and the sums
# of at most 2 100 terms of size 1 differ by their order by less than 1e-12: three and two orders of magnitude below the tolerance.
TOL = 1e-10
MARGIN = 1e-9          # no compared quantity of a test input may lie this close to its threshold: an inlier could flip otherwise
LDS = 1024             # _capi.GROUND_LDS_FRAMES: a longer sequence keeps its foot points in the work buffer
CRT_IN = np.concatenate([[1.0], _rotvec_matrix((0.4, -0.8, 1.1)).reshape(-1), [0.7, -1.9, 0.3]])
CASES = {          # name: (frames, the walker's parameters)
    "6 frames, one pair per foot": (6, {}),
    "40 frames": (40, dict(noise=0.03, seed=1)),
    "98 frames": (98, dict(noise=0.03, seed=0)),
    "98 frames without noise": (98, {}),
    "513 frames": (513, dict(noise=0.03, seed=4)),
    "the last length in LDS": (LDS, dict(noise=0.03, seed=5)),
    "the first length in the work buffer": (LDS + 1, dict(noise=0.03, seed=6)),
    "standing": (98, dict(stand=[(0, 98)], noise=0.01, seed=7)),
    "3 frames": (3, {}),
}
COUNTS = ("points", "inliers", "contact_right", "contact_left", "skate_pairs", "frames", "lag")


@functools.lru_cache(maxsize=None)
def _case(name, moved=False):
    """(the walker's sequence, the twin's estimate of it): computed once, never changed."""
    F, kw = CASES[name]
    x = T.walker_world(F, **kw)[0]
    e = T.estimate(x, crt_in=CRT_IN if moved else None)
    x.setflags(write=False)
    return x, e


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
def G(env):
    from globalegomocap_amd import ground
    return ground


def _dev(env, a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(env.device)


def _record(row):
    from globalegomocap_amd import _capi
    return _capi.GemGroundRecord.from_buffer_copy(np.ascontiguousarray(row).tobytes())


def _compare(row, e, name, capsys):
    from globalegomocap_amd import _capi
    r = _record(row)
    assert int(r.status) == e["status"] == 0, name
    assert _capi.GROUND_SOURCES[int(r.source)] == T.SOURCES[e["source"]], name
    want = dict(e, contact_right=e["contact_frames"][0], contact_left=e["contact_frames"][1])
    for k in COUNTS:
        assert getattr(r, k) == want[k], (name, k, getattr(r, k), want[k])
    worst = {}
    for k in ("n", "d", "u0", "tilt_cos", "rms", "spread", "extent", "skate", "penetration", "lift_max", "crt"):
        worst[k] = float(np.abs(np.array(getattr(r, k)) - np.asarray(e[k])).max())
    with capsys.disabled():
        print("%s: %s, largest differences from the twin: %s" % (name, T.SOURCES[e["source"]], ", ".join("%s %.1e" % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v <= TOL, (name, k, v)


def test_the_inputs_keep_clear_of_the_thresholds():
    for name in CASES:
        assert _case(name)[1]["margin"] > MARGIN, name
    assert _case("98 frames", True)[1]["margin"] > MARGIN
    assert [T.SOURCES[_case(n)[1]["source"]] for n in ("98 frames", "standing", "3 frames", "6 frames, one pair per foot")] == \
        ["plane", "body_normal", "body", "body"]
    assert _case("6 frames, one pair per foot")[1]["points"] == 2


@pytest.mark.parametrize("name", [n for n in CASES if n not in ("standing", "3 frames")])
def test_device_against_the_twin(env, G, name, capsys):
    x, e = _case(name)
    rows = G.ground_call(env, [_dev(env, x)], 5).cpu().numpy()
    _compare(rows[0], e, name, capsys)
    g = G.estimate_ground(env, x)
    assert g.source == T.SOURCES[e["source"]] and g.points == e["points"] and g.frames == len(x)
    np.testing.assert_allclose(g.crt.cpu().numpy(), e["crt"], rtol=0, atol=TOL)
    assert abs(g.skate - 25.0 * e["skate"]) <= 25.0 * TOL and abs(g.tilt_deg - T.angle_deg(e["n"], e["u0"])) < 1e-7


def test_a_batch_of_separate_allocations_and_the_same_bytes_twice(env, G, capsys):
    names = ["98 frames", "standing", "3 frames", "the first length in the work buffer", "513 frames"]
    seqs = [_dev(env, _case(n)[0]) for n in names]
    rows = G.ground_call(env, seqs, 5)
    again = G.ground_call(env, seqs, 5)
    host = rows.cpu().numpy()
    assert host.tobytes() == again.cpu().numpy().tobytes()
    for row, n in zip(host, names):
        _compare(row, _case(n)[1], "batch: " + n, capsys)
    found = G.estimate_ground(env, [_case(n)[0] for n in names[:3]], foot_height=0.03)
    assert [g.source for g in found] == ["plane", "body_normal", "body"]
    np.testing.assert_allclose(found[0].crt_host, T.estimate(_case(names[0])[0], foot_height=0.03)["crt"], rtol=0, atol=TOL)


def test_a_transform_applied_first(env, G, capsys):
    x, e = _case("98 frames", True)
    rows = G.ground_call(env, [_dev(env, x)], 5, moved_by=[_dev(env, CRT_IN)]).cpu().numpy()
    _compare(rows[0], e, "98 frames behind a transform", capsys)
    g = G.estimate_ground(env, x, moved_by=_dev(env, CRT_IN))
    np.testing.assert_allclose(g.crt.cpu().numpy(), e["crt"], rtol=0, atol=TOL)
    # the upright sequence does not depend on where the input stood
    plain = G.estimate_ground(env, x)
    a = G.upright_sequence(env, x, plain).cpu().numpy()
    b = G.upright_sequence(env, T.apply(CRT_IN, x), g).cpu().numpy()
    np.testing.assert_allclose(a, T.upright(x, _case("98 frames")[1]["crt"]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(b, a, rtol=0, atol=1e-9)


def test_refusals(env, G):
    import torch
    from globalegomocap_amd import _capi
    x = _case("40 frames")[0]
    with pytest.raises(_capi.GemError, match="empty table"):
        G.ground_call(env, [], 5)
    for bad in (dict(lag=0), dict(lag=5, tau_v=0.0), dict(lag=5, tau_h=float("nan")), dict(lag=5, min_points=2), dict(lag=5, min_spread=-1.0)):
        with pytest.raises(_capi.GemError, match="gem_ground_plane"):
            G.ground_call(env, [_dev(env, x)], **bad)
    # a sequence that cannot be used sets its own record and leaves its neighbours alone
    nan = np.array(x)
    nan[17, 13, 1] = np.nan
    empty = torch.empty(0, 15, 3, dtype=torch.float64, device=env.device)
    rows = G.ground_call(env, [_dev(env, x), _dev(env, nan), empty, _dev(env, np.zeros((12, 15, 3))), _dev(env, x)], 5).cpu().numpy()
    assert [int(r[0]) for r in rows] == [0, _capi.GROUND_NO_BODY, _capi.GROUND_BAD_SEQUENCE, _capi.GROUND_NO_BODY, 0]
    assert rows[0].tobytes() == rows[4].tobytes() and not rows[2][1:].any()
    with pytest.raises(ValueError, match="sequence 1 .*no body direction"):
        G.estimate_ground(env, [x, nan])
    with pytest.raises(ValueError, match="no sequence"):
        G.estimate_ground(env, [])


def test_compose_against_numpy(env, G):
    rng = np.random.default_rng(11)
    a = np.stack([np.concatenate([[rng.uniform(0.5, 2.0)], _rotvec_matrix(rng.normal(size=3)).reshape(-1), rng.normal(size=3)]) for _ in range(70)])
    b = np.stack([np.concatenate([[rng.uniform(0.5, 2.0)], _rotvec_matrix(rng.normal(size=3)).reshape(-1), rng.normal(size=3)]) for _ in range(70)])
    got = G.compose(env, _dev(env, a), _dev(env, b)).cpu().numpy()
    want = np.stack([T.compose(x, y) for x, y in zip(a, b)])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
    one = G.compose(env, _dev(env, a[3]), _dev(env, b[3])).cpu().numpy()
    assert one.shape == (13,) and np.array_equal(one, got[3])
    with pytest.raises(ValueError, match="one shape"):
        G.compose(env, _dev(env, a), _dev(env, b[:5]))


def test_the_writers_move(env, G, tmp_path):
    from globalegomocap_amd import bvh, meshes
    x, e = _case("98 frames without noise")
    g = G.estimate_ground(env, x)
    # BVH: frame 0's root stands over the origin, at the hips' height above the contacts
    path = str(tmp_path / "up.bvh")
    bvh.write_bvh(env, x[:20], path, move=g.crt)
    got = bvh.read_bvh(path)
    hip_height = float(0.5 * (x[0, 7] + x[0, 11]) @ e["n"] - e["d"])
    assert 0.7 < hip_height < 1.1
    np.testing.assert_allclose(got.motion[0, :3], [0.0, hip_height * 100.0, 0.0], rtol=0, atol=1e-5)
    moved = T.upright(x[:20], e["crt"])
    np.testing.assert_allclose(got.motion[:, :3], 100.0 * 0.5 * (moved[:, 7] + moved[:, 11]), rtol=0, atol=1e-5)
    # behind an alignment: the two are composed on the device
    target = T.apply(CRT_IN, x[:20])
    bvh.write_bvh(env, x[:20], str(tmp_path / "both.bvh"), align_to=target, move=g.crt)
    both = T.upright(target, e["crt"])
    np.testing.assert_allclose(bvh.read_bvh(str(tmp_path / "both.bvh")).motion[:, :3], 100.0 * 0.5 * (both[:, 7] + both[:, 11]), rtol=0, atol=1e-5)
    # without `move` the file is what it is today; the identity moves nothing
    bvh.write_bvh(env, x[:20], str(tmp_path / "plain.bvh"))
    bvh.write_bvh(env, x[:20], str(tmp_path / "none.bvh"), move=None)
    bvh.write_bvh(env, x[:20], str(tmp_path / "identity.bvh"), move=_dev(env, np.concatenate([[1.0], np.eye(3).reshape(-1), np.zeros(3)])))
    plain = open(str(tmp_path / "plain.bvh"), "rb").read()
    assert plain == open(str(tmp_path / "none.bvh"), "rb").read() == open(str(tmp_path / "identity.bvh"), "rb").read()
    with pytest.raises(TypeError, match="move"):
        bvh.write_bvh(env, x[:20], str(tmp_path / "bad.bvh"), move=g.crt_host)
    # meshes: every joint's sphere sits on the moved joint
    lay = meshes.layout()
    blocks = meshes.vertex_blocks(env, x[:3], move=g.crt).cpu().numpy()
    rec = np.dtype([("p", "<f8", 3), ("c", "u1", 3)])
    for f in range(3):
        v = np.frombuffer(blocks[f, :lay.vertex_bytes].tobytes(), dtype=rec)["p"]
        centres = v[:15 * 762].reshape(15, 762, 3).mean(axis=1)
        np.testing.assert_allclose(centres, T.upright(x[f], e["crt"]), rtol=0, atol=1e-6)
    assert np.array_equal(meshes.vertex_blocks(env, x[:3]).cpu().numpy(), meshes.vertex_blocks(env, x[:3], move=None).cpu().numpy())
    bvh.release()


def test_cli_on_a_pose_pickle(env, G, tmp_path, capsys):
    import json
    import pickle
    x = _case("98 frames")[0]
    clean = _case("98 frames without noise")[0]
    pkl = str(tmp_path / "result_pose.pkl")
    with open(pkl, "wb") as f:
        pickle.dump({"estimated_pose": list(x), "optimized_pose": np.array(clean), "mid_optimized_pose": list(x)}, f)
    found = G._cli([pkl, "--json", str(tmp_path / "o" / "ground.json")])
    out = capsys.readouterr().out
    assert list(found) == ["estimated", "optimized"] and "skate (m/s)" in out and "angle between the normals" in out
    assert found["optimized"].skate == 0.0 and found["estimated"].skate > 0.1
    d = json.load(open(str(tmp_path / "o" / "ground.json")))
    assert sorted(d) == ["estimated", "normal_angle_deg", "optimized"] and d["optimized"]["source"] == "plane"
    assert abs(d["normal_angle_deg"] - T.angle_deg(_case("98 frames")[1]["n"], _case("98 frames without noise")[1]["n"])) < 1e-6


def test_upright_end_to_end(env, G, golden, tmp_path):
    """optimize_directory(bvh=DIR, save=True, upright=True) on two chunks of 26 frames: every chunk's result has its ground record,
    the poses and errors are bit for bit those of the call without it, and a chunk's BVH and PLY files stand in one frame."""
    import torch
    from globalegomocap_amd import bvh, prepare as P, whole_sequence as ws
    from helpers import sd_from_npz
    n = 2 * SIZE + 1
    hd, dd, traj, gtp = _write_recording(tmp_path / "rec", n, seed=23)
    rec = P.prepare_sequence(traj, hd, dd, gtp, 0, n, fps=25, test_size=SIZE, verbose=False)
    root = str(tmp_path / "with_gt" / "studio")
    rec.write_chunks(root)
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False)
    torch.manual_seed(31)
    off = ws.optimize_directory(root, DEFAULT_CALIBRATION, **kw)
    torch.manual_seed(31)
    on = ws.optimize_directory(root, DEFAULT_CALIBRATION, bvh=str(tmp_path / "b"), save=True, mesh_root=str(tmp_path / "m"), upright=True, **kw)
    assert list(on[0]) == list(off[0]) and len(on[1]) == len(off[1]) == 2
    for k in off[0]:
        assert np.array_equal(np.asarray(on[0][k]), np.asarray(off[0][k])), k
    for r_on, r_off in zip(on[1], off[1]):
        assert list(r_on) == list(r_off) + ["ground"] and "ground" not in on[0]
        assert r_on["ground"]["source"] in ("plane", "body_normal", "body") and len(r_on["ground"]["crt"]) == 13
        for k in r_off:
            assert np.array_equal(np.asarray(r_on[k]), np.asarray(r_off[k])), k
    for i in (2, 3, 4):
        assert np.array_equal(on[i], off[i])
    names = sorted((c.name for c in rec.chunks), key=ws.natural_key)
    for k, name in enumerate(names):
        gt = on[4][k * SIZE:(k + 1) * SIZE]
        crt = np.array(on[1][k]["ground"]["crt"])
        np.testing.assert_allclose(crt, G.estimate_ground(env, gt).crt_host, rtol=0, atol=0)          # (estimated from the ground truth)
        want = 0.5 * (T.apply(crt, gt[0, 7]) + T.apply(crt, gt[0, 11]))
        assert abs(want[0]) < 1e-9 and abs(want[2]) < 1e-9
        for file, folder in (("gt.bvh", "gt_global_aligned"), ("optimized.bvh", "optimized_global_aligned"), ("estimated.bvh", "input_global_aligned")):
            root_pos = bvh.read_bvh(str(tmp_path / "b" / "studio" / name / file)).motion[0, :3] / 100.0
            c = sphere_centres(str(tmp_path / "m" / "studio" / name / folder / "out_0000.ply"))
            np.testing.assert_allclose(root_pos, 0.5 * (c[7] + c[11]), rtol=0, atol=1e-7, err_msg=name + " " + file)
            if file == "gt.bvh":
                np.testing.assert_allclose(root_pos, want, rtol=0, atol=1e-7)
    ws.release_pools()
