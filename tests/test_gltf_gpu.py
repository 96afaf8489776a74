"""glTF files on the device: gem_gltf_animation and gem_gltf_rest_mesh against the numpy twin
(tests/gltf_twin.py) -- the sign scan across every workgroup boundary, the defined corners --, `write_gltf` read back and skinned, its
determinism and its refusal of a bad frame, and `gltf=DIR` end to end: the batch pipeline with and without ground truth, with
`upright` and `foot_lock`, the command line, and that nothing else changes."""
import os
import pickle

import numpy as np
import pytest

import bvh_twin as B
import gltf_twin as T
from pipeline_checks import SIZE, same_bits as _same_bits, write_recording as _write_recording
from globalegomocap_amd.camera import DEFAULT_CALIBRATION

pytestmark = pytest.mark.gpu

SHAPES = (1, 2, 63, 64, 65, 300)          # a workgroup of gem_gltf_animation writes 63 frames, one of the BVH kernels 64: 300 is five groups
SEEDS = (0, 1, 2, 3)
CRT = np.concatenate([[1.3], B.euler_matrix(20.0, -35.0, 50.0).reshape(-1), [0.1, -0.2, 0.3]])
# both sides agree in float64 to about 1e-12 (what the BVH tests hold their matrices to); one rounding to float32 of a number of at
# most 1 then differs by at most one step, 2^-24; a translation likewise by one step of its own size, 2^-23 relative
Q_TOL, P_RTOL = 2.0 ** -24 + 1e-12, 2.0 ** -23


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
    from globalegomocap_amd import gltf
    return gltf


@pytest.fixture(scope="module")
def twin():
    """name -> (X, times, translation, rotations [15,F,4]) of the twin, made once per input and never changed: `random_frames(300,
    seed)` plain and behind CRT, and the walker that turns twice.  A prefix of the frames has a prefix of the arrays."""
    made = {}

    def get(name):
        if name not in made:
            kind, with_crt = name
            X = T.turning_walker(130) if kind == "walker" else B.random_frames(300, seed=kind)
            crt = CRT if with_crt else None
            _, c = T.canonical_quaternions(X, crt)
            dots = (c[1:] * c[:-1]).sum(-1)
            lead = np.array([next(v for v in q if v != 0) for q in c[0]])
            # the signs cannot hang on last-bit differences: no dot near 0, no leading component of frame 0 near 0
            assert np.abs(dots).min() > 1e-6 and lead.min() > 1e-6, (name, np.abs(dots).min(), lead.min())
            arrays = (X,) + T.animation_arrays(X, crt, 30.0)
            for a in arrays:
                a.setflags(write=False)
            made[name] = arrays + (int((dots[:, 0] < 0).sum()),)
        return made[name]
    return get


def _dev(env, a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a))          # (a copy: the fixtures are read-only)
    return (t if dtype is None else t.to(dtype)).to(env.device)


def _block(env, G, X, crt, fps, canary=64):
    """The device's animation block of X between two canaries -> (times, translation, rotations, bad), and the padding as it was."""
    import torch
    n = G.layout(len(X)).block_bytes
    buf = torch.full((canary + n + canary,), 0xA5, dtype=torch.uint8, device=env.device)
    out, bad = G.animation(env, _dev(env, X), None if crt is None else _dev(env, crt), fps, out=buf[canary:canary + n])
    assert out.data_ptr() == buf.data_ptr() + canary
    host = buf.cpu().numpy()
    assert (host[:canary] == 0xA5).all() and (host[-canary:] == 0xA5).all()
    block = host[canary:canary + n].copy()
    off, size = T.block_offsets(len(X))
    F = len(X)
    assert (block[4 * F:off[1]] == 0xA5).all() and (block[off[1] + 12 * F:off[2]] == 0xA5).all()          # the padding is not written
    block[4 * F:off[1]] = 0
    block[off[1] + 12 * F:off[2]] = 0
    return T.parse_block(block.tobytes(), F) + (bad.cpu().numpy().tolist(),)


def _compare(got, want, F, what, capsys):
    times, tr, rot, bad = got
    _, w_times, w_tr, w_rot = want[:4]
    assert bad == [0, -1], what
    assert np.array_equal(times.view(np.uint32), w_times[:F].view(np.uint32)), what          # bit for bit
    q_err = np.abs(rot.astype(np.float64) - w_rot[:, :F].astype(np.float64)).max()
    with capsys.disabled():
        print("%s: quaternion components %.3g (%.2f steps of 2^-24), translation %.3g (relative) from the twin"
              % (what, q_err, q_err * 2.0 ** 24, np.abs(tr.astype(np.float64) / w_tr[:F].astype(np.float64) - 1).max()))
    np.testing.assert_allclose(tr, w_tr[:F], rtol=P_RTOL, atol=0, err_msg=what)
    assert q_err <= Q_TOL, what
    q = rot.astype(np.float64)
    assert np.abs(np.sqrt((q * q).sum(-1)) - 1).max() <= 1e-6
    if F > 1:
        assert ((q[:, 1:] * q[:, :-1]).sum(-1) >= -1e-6).all(), "the sign is continuous from key to key"


@pytest.mark.parametrize("with_crt", [False, True], ids=["plain", "behind a similarity"])
@pytest.mark.parametrize("F", SHAPES)
def test_animation_against_the_twin(env, G, twin, F, with_crt, capsys):
    """times bit for bit, translations to one float32 step, quaternion components to 2^-24 + 1e-12, on four inputs whose Hips flip
    their canonical sign 19 to 30 times in 300 frames (and five other nodes theirs), across every workgroup boundary."""
    for seed in SEEDS:
        want = twin((seed, with_crt))
        assert F < 300 or (19 <= want[4] <= 30 if not with_crt else 14 <= want[4] <= 18)          # (the Hips' flips: what the inputs are chosen for)
        got = _block(env, G, want[0][:F], CRT if with_crt else None, 30.0)
        _compare(got, want, F, "%d frames of seed %d%s" % (F, seed, ", crt" if with_crt else ""), capsys)
        if seed == 0:          # two calls, the same bytes
            again = _block(env, G, want[0][:F], CRT if with_crt else None, 30.0)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got[:3], again[:3]))


def test_animation_of_a_walker_that_turns_twice(env, G, twin, capsys):
    want = twin(("walker", False))
    assert want[4] == 2
    got = _block(env, G, want[0], None, 30.0)
    _compare(got, want, 130, "the turning walker", capsys)
    q = got[2].astype(np.float64)
    assert (q[:, 1:] * q[:, :-1]).sum(-1).min() > 0.98


def test_defined_corners(env, G, capsys):
    """`bvh_twin.corner_frames()`, each a sequence of one frame: half turns give w = 0, where the canonical sign comes from x, y or z."""
    frames = B.corner_frames()
    zero_w = 0
    for name, x in frames.items():
        X = x[None]
        times, tr, rot, bad = _block(env, G, X, None, 25.0)
        w_times, w_tr, w_rot = T.animation_arrays(X, None, 25.0)
        assert bad == [0, -1] and times[0] == 0 and np.isfinite(rot).all(), name
        np.testing.assert_allclose(tr, w_tr, rtol=P_RTOL, atol=0, err_msg=name)
        err = np.abs(rot.astype(np.float64) - w_rot.astype(np.float64)).max()
        with capsys.disabled():
            print("corner %-42s quaternion components %.3g from the twin" % (name, err))
        assert err <= Q_TOL, name
        lead = [next((v for v in (q[3], q[0], q[1], q[2]) if v != 0), 0.0) for q in rot[:, 0]]
        assert min(lead) > 0, name
        zero_w += int((rot[:, 0, 3] == 0).sum())
    assert zero_w >= 4          # the antiparallel bones and the node behind each that undoes the half turn


def test_animation_counts_bad_frames_and_refuses_bad_arguments(env, G):
    import torch
    X = B.random_frames(100, seed=5)
    X[41, 3] = np.nan
    X[77, 9, 1] = np.inf
    *_, bad = _block(env, G, X, None, 25.0)
    assert bad == [2, 41]
    seq = _dev(env, X)
    buf = torch.zeros(G.layout(100).block_bytes + 32, dtype=torch.uint8, device=env.device)
    with pytest.raises(Exception, match="16-byte aligned"):
        G.animation(env, seq, None, 25.0, out=buf[8:8 + G.layout(100).block_bytes])
    for fps in (0.0, -1.0, float("nan")):
        with pytest.raises(Exception, match="fps"):
            G.animation(env, seq, None, fps)
    with pytest.raises(ValueError):
        G.animation(env, seq, None, 25.0, out=buf[:64])
    torch.cuda.synchronize()
    assert not bool(buf.any())
    block, bad = G.animation(env, seq[:0], None, 25.0)
    assert block.numel() == 0 and bad.cpu().tolist() == [0, -1]


@pytest.mark.parametrize("with_crt", [False, True], ids=["plain", "behind a similarity"])
def test_rest_mesh_against_the_twin(env, G, twin, with_crt, capsys):
    import torch
    X = twin((2, False))[0]
    crt = CRT if with_crt else None
    rest = B.rest_lengths(X, crt)
    buf = torch.full((64 + T.N_VERTICES * 32 + 64,), 0xA5, dtype=torch.uint8, device=env.device)
    block, bounds = G.rest_mesh(env, _dev(env, rest), out=buf[64:64 + T.N_VERTICES * 32])
    again, bounds2 = G.rest_mesh(env, _dev(env, rest))
    host = buf.cpu().numpy()
    assert (host[:64] == 0xA5).all() and (host[-64:] == 0xA5).all() and torch.equal(block, again) and torch.equal(bounds, bounds2)
    pos, nr, J, W = T.parse_vertices(host[64:-64].tobytes())
    w_pos, w_nr, w_J, w_W = T.rest_mesh(rest)
    w32 = w_pos.astype(np.float32)
    # one float32 step of the coordinate (1e-12: the float64 difference of a coordinate next to zero)
    steps = np.abs(pos.astype(np.float64) - w32.astype(np.float64)) / (np.spacing(np.abs(w32)).astype(np.float64) + 1e-12)
    n_err = np.abs(nr.astype(np.float64) - w_nr).max()
    with capsys.disabled():
        print("rest mesh%s: positions %.2f float32 steps, normals %.3g from the twin" % (", crt" if with_crt else "", steps.max(), n_err))
    assert steps.max() <= 1.0
    assert np.array_equal(J, w_J) and np.array_equal(W, w_W)
    assert n_err <= Q_TOL and np.abs(np.sqrt((nr.astype(np.float64) ** 2).sum(-1)) - 1).max() <= 1e-6
    b = bounds.cpu().numpy()
    assert b.dtype == np.float32 and np.array_equal(b[:3], pos.min(axis=0)) and np.array_equal(b[3:], pos.max(axis=0))
    # the binding table in words: spheres on their joints' nodes, single-node cylinders, the two torso lines blended
    assert (W[:15 * 762, 0] == 255).all() and sorted(set(J[:15 * 762, 0].tolist())) == sorted(T.NODE_OF_JOINT)
    cyl = lambda l: slice(15 * 762 + 102 * l, 15 * 762 + 102 * (l + 1))          # noqa: E731
    assert set(J[cyl(14), 0].tolist()) == {0} and set(J[cyl(0), 0].tolist()) == {3} and set(J[cyl(8), 0].tolist()) == {11}
    for l in (6, 7):
        assert sorted(set(W[cyl(l), 1].tolist())) == [0, 64, 128, 191, 255]


def _written(G, path):
    data = open(path, "rb").read()
    doc, arrays = T.check_container(data)
    return data, doc, G.read_glb(path)


def _check_skeleton(G, parsed, name, X, frames=(0,), crt=None):
    """The skeleton `name` of a file against the twin on X: `joint_positions` at every key and the skinned cap centres of every
    cylinder at `frames` lie on `regrow`'s joints.  1e-5 + 2^-23 max|position| metres: at most 7 chained float32 quaternions (about
    2.4e-7 rad each) on a lever under 2 m give about 3e-6 m, plus the root's float32 rounding."""
    rest = B.rest_lengths(X, crt)
    want = B.joints_of(B.regrow(X, rest, crt))
    tol = 1e-5 + 2.0 ** -23 * np.abs(want).max()
    got = G.joint_positions(parsed, name)
    worst = np.abs(got - want).max()
    assert got.shape == want.shape and worst <= tol, (name, worst, tol)
    lines = np.array(T.M.LINES)
    for f in frames:
        v = T.skin(parsed, name, f)[T.cap_centres()]
        worst = max(worst, np.abs(v[:, 0] - want[f, lines[:, 1]]).max(), np.abs(v[:, 1] - want[f, lines[:, 0]]).max())
    assert worst <= tol, (name, worst, tol)
    return worst


def test_skinning_closes_the_loop_and_the_file_is_deterministic(env, G, twin, tmp_path, monkeypatch, capsys):
    """300 frames, three skeletons, two of them aligned to the third: a valid container; every cylinder's cap centres, skinned, and
    `joint_positions` lie on `regrow`'s joints; a second call and a call through small pinned buffers give the same bytes."""
    from globalegomocap_amd.errors import align_sequence
    X, Y, Z = twin((0, False))[0], twin((1, False))[0], twin((2, False))[0]
    seqs = {"estimated": X, "optimized": _dev(env, Y), "gt": Z}
    to = {"estimated": Z, "optimized": Z}
    p1, p2, p3 = str(tmp_path / "deep" / "a.glb"), str(tmp_path / "b.glb"), str(tmp_path / "c.glb")
    G.release()
    try:
        assert G.write_gltf(env, seqs, p1, fps=30, align_to=to) == 300
        assert G.write_gltf(env, seqs, p2, fps=30, align_to=to) == 300
        monkeypatch.setattr(G, "PINNED_BYTES", 100000)          # 21 slices, both buffers used again and again
        G.release()
        assert G.write_gltf(env, seqs, p3, fps=30, align_to=to) == 300
        data, doc, parsed = _written(G, p1)
        assert data == open(p2, "rb").read() == open(p3, "rb").read()
        assert len(data) < 12 + 8 + 65536 + 8 + 154800 + 3 * (1216 + 414720 + 256 * 300 + 32) and sorted(os.listdir(str(tmp_path))) == ["b.glb", "c.glb", "deep"]
        assert [m["name"] for m in doc["meshes"]] == ["estimated", "optimized", "gt"]
        for name, seq in (("estimated", align_sequence(X, Z)), ("optimized", align_sequence(Y, Z)), ("gt", Z)):
            worst = _check_skeleton(G, parsed, name, seq, frames=(0, 150, 299))
            with capsys.disabled():
                print("write_gltf -> read_glb, %s: joints and skinned cap centres %.3g m from regrow" % (name, worst))
        # the blocks in the file are the device's own
        times, tr, rot, _ = _block(env, G, Z, None, 30.0)
        ch = doc["animations"][0]["channels"]
        gt_rot = [parsed.accessors[doc["animations"][0]["samplers"][c["sampler"]]["output"]] for c in ch[33:48]]
        assert np.array_equal(np.stack(gt_rot), rot) and np.array_equal(parsed.accessors[doc["animations"][0]["samplers"][0]["input"]][:, 0], times)
        # a move behind the alignment, one frame
        mv = _dev(env, CRT)
        G.write_gltf(env, {"only": X[:1]}, p2, move=mv, colours={"only": (10, 20, 30)})
        _check_skeleton(G, _written(G, p2)[2], "only", B.move(X[:1], CRT))
    finally:
        G.release()


def test_a_bad_frame_raises_and_leaves_no_file(env, G, tmp_path):
    X = B.random_frames(100, seed=7)
    bad = X.copy()
    bad[41, 6] = np.nan
    bad[60, 2] = np.nan
    path = str(tmp_path / "nan.glb")
    try:
        with pytest.raises(ValueError, match="frame 41 "):
            G.write_gltf(env, {"estimated": X, "optimized": bad}, path)
        assert os.listdir(str(tmp_path)) == []
        with pytest.raises(ValueError, match="at least one frame"):
            G.write_gltf(env, {"estimated": X[:0]}, path)
        with pytest.raises(ValueError, match="equally many"):
            G.write_gltf(env, {"estimated": X, "optimized": X[:5]}, path)
        with pytest.raises(ValueError, match="shape"):
            G.write_gltf(env, {"estimated": X}, path, align_to=X[:5])
        with pytest.raises(ValueError, match="does not hold"):
            G.write_gltf(env, {"estimated": X}, path, align_to={"gt": X})
        assert os.listdir(str(tmp_path)) == []
        assert G.write_gltf(env, {"estimated": X}, path) == 100          # and the buffers are fit for the next call
        _check_skeleton(G, _written(G, path)[2], "estimated", X)
    finally:
        G.release()


def test_cli_on_a_pose_pickle(env, G, twin, tmp_path):
    X = twin((2, False))[0][:5]
    gt = 1.1 * X + 0.01
    pkl = str(tmp_path / "result_pose.pkl")
    with open(pkl, "wb") as f:
        pickle.dump({"estimated_pose": list(X), "optimized_pose": X + 0.01, "gt_pose": list(gt)}, f)
    from globalegomocap_amd.errors import align_sequence
    out = str(tmp_path / "cli" / "five.glb")
    G.main([pkl, "--out", out, "--align", "true", "--fps", "50"])
    data, doc, parsed = _written(G, out)
    assert [s["name"] for s in doc["skins"]] == ["estimated", "optimized", "gt"]
    assert parsed.accessors[doc["animations"][0]["samplers"][0]["input"]][:, 0].tolist() == [np.float32(f / 50.0) for f in range(5)]
    _check_skeleton(G, parsed, "estimated", align_sequence(X, gt))
    _check_skeleton(G, parsed, "gt", gt)
    with open(pkl, "wb") as f:
        pickle.dump({"estimated_pose": list(X), "optimized_pose": X + 0.01}, f)
    G.main([pkl, "--out", str(tmp_path / "two.glb")])
    data, doc, parsed = _written(G, str(tmp_path / "two.glb"))
    assert [s["name"] for s in doc["skins"]] == ["estimated", "optimized"]
    _check_skeleton(G, parsed, "optimized", X + 0.01)
    G.release()


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def chunk_dirs(env, golden, tmp_path_factory):
    """Two chunks of 26 frames with ground truth and the same without, as pickles under <tmp>/with_gt/studio and <tmp>/no_gt/studio."""
    from globalegomocap_amd import prepare as P
    from helpers import sd_from_npz
    tmp = tmp_path_factory.mktemp("gltf")
    n = 2 * SIZE + 1
    hd, dd, traj, gtp = _write_recording(tmp / "rec", n, seed=23)
    with_gt = P.prepare_sequence(traj, hd, dd, gtp, 0, n, fps=25, test_size=SIZE, verbose=False)
    no_gt = P.prepare_sequence(traj, hd, dd, None, 0, n, fps=25, test_size=SIZE, verbose=False, scale=1.7)
    assert len(with_gt) == len(no_gt) == 2
    with_gt.write_chunks(str(tmp / "with_gt" / "studio"))
    no_gt.write_chunks(str(tmp / "no_gt" / "studio"))
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"), verbose=False)
    return dict(tmp=tmp, kw=kw, names=[c.name for c in with_gt.chunks])


def test_gltf_with_ground_truth(G, chunk_dirs):
    import torch
    from globalegomocap_amd import whole_sequence as ws
    from globalegomocap_amd.errors import align_sequence
    tmp, kw = chunk_dirs["tmp"], chunk_dirs["kw"]
    root, out = str(tmp / "with_gt" / "studio"), tmp / "g_gt"
    torch.manual_seed(31)
    off = ws.optimize_directory(root, DEFAULT_CALIBRATION, **kw)
    torch.manual_seed(31)
    on = ws.optimize_directory(root, DEFAULT_CALIBRATION, gltf=str(out), gltf_fps=50, **kw)
    _same_bits(on, off)
    assert sorted(os.listdir(str(out / "studio"))) == sorted(chunk_dirs["names"])
    for k, name in enumerate(sorted(chunk_dirs["names"], key=ws.natural_key)):
        base, fr = out / "studio" / name, slice(k * SIZE, (k + 1) * SIZE)
        assert os.listdir(str(base)) == ["result.glb"]
        data, doc, parsed = _written(G, str(base / "result.glb"))
        assert [s["name"] for s in doc["skins"]] == ["estimated", "optimized", "gt"]
        assert doc["accessors"][doc["animations"][0]["samplers"][0]["input"]]["max"] == [float(np.float32((SIZE - 1) / 50.0))]
        _check_skeleton(G, parsed, "estimated", align_sequence(on[2][fr], on[4][fr]), frames=(0, SIZE - 1))
        _check_skeleton(G, parsed, "optimized", align_sequence(on[3][fr], on[4][fr]))
        _check_skeleton(G, parsed, "gt", on[4][fr])


def test_gltf_without_ground_truth(G, chunk_dirs):
    import torch
    from globalegomocap_amd import whole_sequence as ws
    tmp, kw = chunk_dirs["tmp"], chunk_dirs["kw"]
    root = str(tmp / "no_gt" / "studio")
    torch.manual_seed(31)
    off = ws.optimize_directory(root, DEFAULT_CALIBRATION, ground_truth=False, **kw)
    torch.manual_seed(31)
    on = ws.optimize_directory(root, DEFAULT_CALIBRATION, ground_truth=False, gltf=str(tmp / "g_no_gt"), **kw)
    _same_bits(on, off)
    for k, name in enumerate(sorted(chunk_dirs["names"], key=ws.natural_key)):
        fr = slice(k * SIZE, (k + 1) * SIZE)
        data, doc, parsed = _written(G, str(tmp / "g_no_gt" / "studio" / name / "result.glb"))
        assert [s["name"] for s in doc["skins"]] == ["estimated", "optimized"]
        assert doc["accessors"][doc["animations"][0]["samplers"][0]["input"]]["max"] == [float(np.float32((SIZE - 1) / 25.0))]
        _check_skeleton(G, parsed, "optimized", on[3][fr], frames=(0,))
        _check_skeleton(G, parsed, "estimated", on[2][fr])


def test_gltf_upright_with_locked_feet(G, chunk_dirs):
    """`gltf=DIR, upright=True, foot_lock=True`: the optimised skeleton is `foot_locked_pose` stood upright -- frame 0's hip midpoint
    over x = z = 0 --, the estimated one the estimated sequence in the same frame; poses and reports as without the three."""
    import torch
    import ground_twin
    from globalegomocap_amd import whole_sequence as ws
    tmp, kw = chunk_dirs["tmp"], chunk_dirs["kw"]
    root = str(tmp / "no_gt" / "studio")
    torch.manual_seed(31)
    off = ws.optimize_directory(root, DEFAULT_CALIBRATION, ground_truth=False, **kw)
    torch.manual_seed(31)
    on = ws.optimize_directory(root, DEFAULT_CALIBRATION, ground_truth=False, gltf=str(tmp / "g_up"), upright=True, foot_lock=True,
                               save_pose=str(tmp / "p_up"), **kw)
    for i in (2, 3):
        assert np.array_equal(on[i], off[i])
    for k, name in enumerate(sorted(chunk_dirs["names"], key=ws.natural_key)):
        r_on, r_off = on[1][k], off[1][k]
        assert sorted(r_on) == sorted(list(r_off) + ["foot_lock", "ground"])
        for key in r_off:
            assert np.array_equal(np.asarray(r_on[key]), np.asarray(r_off[key])), key
        crt = np.array(r_on["ground"]["crt"])
        locked = np.asarray(pickle.load(open(str(tmp / "p_up" / name / "result_pose.pkl"), "rb"))["foot_locked_pose"])
        data, doc, parsed = _written(G, str(tmp / "g_up" / "studio" / name / "result.glb"))
        _check_skeleton(G, parsed, "optimized", ground_twin.apply(crt, locked), frames=(0,))
        _check_skeleton(G, parsed, "estimated", ground_twin.apply(crt, on[2][k * SIZE:(k + 1) * SIZE]))
        hips = G.joint_positions(parsed, "optimized")[0, [7, 11]].mean(axis=0)
        assert abs(hips[0]) < 1e-6 and abs(hips[2]) < 1e-6 and hips[1] > 0
    ws.release_pools()


def test_main_writes_the_file(env, G, chunk_dirs, tmp_path, monkeypatch):
    """optimizer.main(gltf=DIR): DIR/<dataset>/<chunk>/result.glb; the poses and the errors are bit for bit those of the call without it."""
    import torch
    from globalegomocap_amd import optimizer as gopt, synth
    from globalegomocap_amd.errors import align_sequence
    data = synth.make_sequence(n_frames=SIZE, seed=9)
    d = tmp_path / "studio-x" / "chunk_7"
    d.mkdir(parents=True)
    with open(str(d / "test_data.pkl"), "wb") as f:
        pickle.dump(synth.reference_pickle_dict(data), f)
    monkeypatch.chdir(tmp_path)
    kw = {k: chunk_dirs["kw"][k] for k in ("global_vae_path", "local_vae_path")}
    args = (str(d), DEFAULT_CALIBRATION, 0.0, 0.0, 0.001, 0.01, 0.01, 0.01)
    eps = torch.randn(6, 32, generator=torch.Generator().manual_seed(5))
    off = gopt.main(*args, final_smooth=True, eps=eps, **kw)
    on = gopt.main(*args, final_smooth=True, gltf=str(tmp_path / "scene"), eps=eps, **kw)
    assert list(on[0]) == list(off[0])
    for k in on[0]:
        assert np.array_equal(np.asarray(on[0][k]), np.asarray(off[0][k])), k
    for i in (1, 2, 3, 4):
        assert np.array_equal(np.asarray(on[i]), np.asarray(off[i])), i
    base = tmp_path / "scene" / "studio-x" / "chunk_7"
    assert os.listdir(str(base)) == ["result.glb"]
    parsed = _written(G, str(base / "result.glb"))[2]
    est, opt, gt = np.asarray(on[1]), np.asarray(on[3]), np.asarray(on[4])
    _check_skeleton(G, parsed, "optimized", align_sequence(opt, gt))
    _check_skeleton(G, parsed, "estimated", align_sequence(est, gt))
    _check_skeleton(G, parsed, "gt", gt)
    G.release()
