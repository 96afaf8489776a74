"""glTF files of skinned, animated skeletons, the part that needs no GPU: the library's layout and argument
errors, the numpy twin (tests/gltf_twin.py) against the BVH twin's local rotations and its own sign rules, `gltf.build_document` with
twin-made blocks held to the container's rules, `gltf.read_glb` / `joint_positions` on such a file, and the wiring."""
import os
import struct

import numpy as np
import pytest

import bvh_twin as B
import gltf_twin as T

CRT = np.concatenate([[1.3], B.euler_matrix(20.0, -35.0, 50.0).reshape(-1), [0.1, -0.2, 0.3]])
COLOURS = {"estimated": (214, 39, 40), "optimized": (31, 119, 180), "gt": (44, 160, 44)}


@pytest.fixture(scope="module")
def G():
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import gltf
    return gltf


@pytest.fixture(scope="module")
def frames37():
    X = B.random_frames(37, seed=1)
    X.setflags(write=False)
    return X


def _file_bytes(G, sequences, fps=25, crt=None):
    """A file as `write_gltf` lays it out, every device-made section from the twin."""
    F = len(next(iter(sequences.values())))
    skeletons, made = [], {}
    for name, X in sequences.items():
        rest = B.rest_lengths(X, crt)
        made["%s/vertices" % name], bounds = T.rest_mesh_bytes(rest)
        made["%s/animation" % name] = T.animation_block(X, crt, fps)
        skeletons.append((name, rest, bounds, COLOURS[name]))
    doc, sections, total = G.build_document(skeletons, F, fps)
    return T.assemble(doc, sections, total, made)


def test_layout_numbers(G):
    import ctypes as C
    from globalegomocap_amd import _capi
    lib = _capi.load_library()
    for F in (0, 1, 2, 3, 4, 37, 64, 300, 100000):
        out = (C.c_int64 * _capi.GLTF_LAYOUT)()
        assert lib.gem_gltf_layout(F, out) == 0
        lay = G.layout(F)
        assert tuple(out)[:6] == (19, 15, 12960, 25800, 32, 414720) == tuple(lay)[:6]
        assert lay.rotating_nodes == T.ROTATING == (0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17)
        off, size = T.block_offsets(F)
        assert list(lay.offsets) == off and lay.block_bytes == size and lay.frame_bytes == T.FRAME_BYTES == 256
        assert len(lay.offsets) == 17 and all(o % 16 == 0 for o in lay.offsets) and size % 16 == 0
        sizes = [4 * F, 12 * F] + [16 * F] * 15
        assert sum(sizes) == 256 * F          # the payload: 256 bytes per frame
        assert all(lay.offsets[i] + sizes[i] <= (lay.offsets[i + 1] if i < 16 else size) for i in range(17))
        assert size - 256 * F < 32          # (two arrays are padded, each by less than 16 bytes)
    assert (12960 * 32, 12960 < 1 << 16) == (lay.vertex_bytes, True)


def test_the_c_abi_refuses_bad_arguments_before_any_launch(G):
    import ctypes as C
    import re
    from globalegomocap_amd import _capi
    lib = _capi.load_library()
    out = (C.c_int64 * _capi.GLTF_LAYOUT)()
    assert lib.gem_gltf_layout(-1, out) != 0 and b"n_frames" in lib.gem_last_error()
    assert lib.gem_gltf_layout(3, None) != 0 and b"null" in lib.gem_last_error()
    ok = C.c_void_p(4096)
    assert lib.gem_gltf_animation(None, -1, None, 25.0, None, None, None) != 0 and b"n_frames" in lib.gem_last_error()
    assert lib.gem_gltf_animation(None, 3, None, 25.0, None, None, None) != 0 and b"null" in lib.gem_last_error()
    assert lib.gem_gltf_animation(ok, 3, None, 25.0, ok, None, None) != 0 and b"null" in lib.gem_last_error()
    assert lib.gem_gltf_animation(None, 0, None, 25.0, None, None, None) == 0
    for fps in (0.0, -25.0, float("nan"), float("inf")):
        assert lib.gem_gltf_animation(ok, 3, None, fps, ok, ok, None) != 0 and b"fps" in lib.gem_last_error(), fps
    assert lib.gem_gltf_animation(ok, 3, None, 25.0, C.c_void_p(4096 + 8), ok, None) != 0 and b"16-byte aligned" in lib.gem_last_error()
    assert lib.gem_gltf_rest_mesh(None, None, None, None) != 0 and b"null" in lib.gem_last_error()
    assert lib.gem_gltf_rest_mesh(ok, C.c_void_p(4096 + 4), ok, None) != 0 and b"16-byte aligned" in lib.gem_last_error()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gem_hip.h")).read()
    for name, n_args in (("gem_gltf_layout", 2), ("gem_gltf_animation", 7), ("gem_gltf_rest_mesh", 4)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == n_args == len(_capi.SIGNATURES[name][1]), name
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "globalegomocap_amd", "csrc", "errors.hip")).read()
    assert src.count('#include "gltf.h"') == 1 and src.index('#include "bvh.h"') < src.index('#include "gltf.h"')


def test_twin_quaternions_are_the_bvh_twins_local_rotations(frames37, capsys):
    """Rebuilt into matrices they equal `frame_locals` to 1e-12, plain, behind a similarity and on the defined corners (half turns: w = 0)."""
    corners = np.stack(list(B.corner_frames().values()))
    worst = 0.0
    for X, crt in ((frames37, None), (frames37, CRT), (corners, None)):
        P, c = T.canonical_quaternions(X, crt)
        for f, x in enumerate(B.move(X, crt)):
            p, L = B.frame_locals(x)
            assert np.array_equal(P[f], p)
            worst = max(worst, np.abs(T.matrices(c[f]) - L[list(T.ROTATING)]).max())
        lead = np.array([[next((v for v in q if v != 0), 0.0) for q in row] for row in c])
        assert (lead > 0).all() and np.abs((c * c).sum(-1) - 1).max() <= 1e-12
    with capsys.disabled():
        print("twin: quaternions rebuilt into matrices - frame_locals %.3g" % worst)
    assert worst <= 1e-12
    # the corners do meet the rule for w = 0: half turns, whose sign comes from x, y or z
    assert (T.canonical_quaternions(corners)[1][..., 0] == 0).any()
    for R, want in ((np.diag([-1.0, -1.0, 1.0]), (0, 0, 0, 1)), (np.diag([1.0, -1.0, -1.0]), (0, 1, 0, 0)), (np.diag([-1.0, 1.0, -1.0]), (0, 0, 1, 0)),
                    (np.eye(3), (1, 0, 0, 0))):
        assert tuple(T.canonical(T.shepperd(R))) == want
    assert tuple(T.canonical(np.array([-0.0, 0.0, -0.5, 0.5]))) == (0.0, 0.0, 0.5, -0.5)


def test_sign_continuity_on_a_walker_that_turns_twice(capsys):
    X = T.turning_walker(130)
    P, c = T.canonical_quaternions(X)
    flips = [f for f in range(1, 130) if (c[f, 0] * c[f - 1, 0]).sum() < 0]
    assert flips == [16, 81]          # the Hips' canonical sign: once per full turn
    s = T.continuity_signs(c)
    assert (s[:16, 0] == 1).all() and (s[16:81, 0] == -1).all() and (s[81:, 0] == 1).all() and (s[:, 1:] == 1).all()
    q = T.quaternions(X)[1]
    dots = (q[1:] * q[:-1]).sum(-1)
    with capsys.disabled():
        print("turning walker: smallest consecutive dot after the scan %.4f (before: %.4f)" % (dots.min(), (c[1:] * c[:-1]).sum(-1).min()))
    assert dots.min() > 0.98
    # a dot of 0 or NaN does not flip
    z = np.array([[[1.0, 0, 0, 0]], [[0, 1.0, 0, 0]], [[np.nan, 0, 0, 0]], [[0, -1.0, 0, 0]], [[0, 1.0, 0, 0]]])
    assert T.continuity_signs(z)[:, 0].tolist() == [1, 1, 1, 1, -1]


@pytest.mark.parametrize("F", [1, 2, 37])
@pytest.mark.parametrize("n_skeletons", [1, 2, 3])
def test_build_document_with_twin_blocks_is_a_valid_container(G, frames37, n_skeletons, F):
    names = ("estimated", "optimized", "gt")[:n_skeletons]
    seqs = {n: frames37[:F] + 0.01 * i for i, n in enumerate(names)}
    data = _file_bytes(G, seqs, fps=30)
    doc, arrays = T.check_container(data)
    assert len(doc["skins"]) == n_skeletons and len(doc["nodes"]) == 20 * n_skeletons and len(doc["scenes"][0]["nodes"]) == 2 * n_skeletons
    assert [m["name"] for m in doc["materials"]] == list(names)
    lay = G.layout(F)
    assert len(data) % 4 == 0 and doc["buffers"][0]["byteLength"] == 154800 + n_skeletons * (1216 + lay.vertex_bytes + lay.block_bytes)
    for si, name in enumerate(names):
        rest = B.rest_lengths(seqs[name])
        nodes = doc["nodes"][20 * si:20 * si + 19]
        assert [n["name"] for n in nodes] == ["%s/%s" % (name, x) for x in B.NAMES]
        np.testing.assert_array_equal(np.array([n["translation"] for n in nodes]), B.offsets_of(rest))
        assert [sorted(c - 20 * si for c in n.get("children", [])) for n in nodes] == [list(k) for k in B.KIDS]
        ibm = arrays[doc["skins"][si]["inverseBindMatrices"]].reshape(19, 4, 4)
        np.testing.assert_array_equal(ibm[:, 3, :3], (-T.rest_nodes(rest)).astype(np.float32))
        assert np.array_equal(ibm[:, :3, :3], np.tile(np.eye(3, dtype=np.float32), (19, 1, 1)))
        rgb = doc["materials"][si]["pbrMetallicRoughness"]["baseColorFactor"]
        srgb = [255 * (12.92 * c if c <= 0.0031308 else 1.055 * c ** (1 / 2.4) - 0.055) for c in rgb[:3]]
        np.testing.assert_allclose(srgb, COLOURS[name], atol=1e-9)
    chans = doc["animations"][0]["channels"]
    assert [c["target"]["path"] for c in chans] == (["translation"] + ["rotation"] * 15) * n_skeletons
    assert [c["target"]["node"] for c in chans] == [20 * si + n for si in range(n_skeletons) for n in (0,) + T.ROTATING]
    tri = arrays[doc["meshes"][0]["primitives"][0]["indices"]].reshape(-1, 3)
    assert np.array_equal(tri, T.M.frame_mesh(np.zeros((15, 3)) + np.arange(15)[:, None])[2])


def test_build_document_refuses(G):
    rest, bounds = np.ones(19), np.zeros(6)
    with pytest.raises(ValueError, match="at least one frame"):
        G.build_document([("a", rest, bounds, (1, 2, 3))], 0, 25)
    with pytest.raises(ValueError, match="fps"):
        G.build_document([("a", rest, bounds, (1, 2, 3))], 3, 0)
    with pytest.raises(ValueError, match="names"):
        G.build_document([("a", rest, bounds, (1, 2, 3))] * 2, 3, 25)
    with pytest.raises(ValueError, match="no numbers"):
        G.build_document([("a", rest * np.nan, bounds, (1, 2, 3))], 3, 25)


def test_read_glb_round_trip_and_joint_positions(G, frames37, tmp_path, capsys):
    seqs = {"estimated": frames37, "optimized": frames37[::-1] * 1.1}
    data = _file_bytes(G, seqs, fps=50, crt=CRT)
    path = str(tmp_path / "twin.glb")
    with open(path, "wb") as f:
        f.write(data)
    parsed = G.read_glb(path)
    doc, arrays = T.check_container(data)
    assert parsed.json == doc and len(parsed.accessors) == len(arrays)
    for i, a in arrays.items():
        got = parsed.accessors[i]
        assert np.array_equal(got.reshape(len(a), -1), a) and got.dtype == a.dtype, i
    worst = 0.0
    for name, X in seqs.items():
        rest = B.rest_lengths(X, CRT)
        want = B.joints_of(B.regrow(X, rest, CRT))
        got = G.joint_positions(parsed, name)
        assert got.shape == (37, 15, 3)
        tol = 1e-5 + 2.0 ** -23 * np.abs(want).max()
        worst = max(worst, np.abs(got - want).max())
        assert np.abs(got - want).max() <= tol
        # the cap centres of every cylinder, skinned, are the joints the line joins
        lines = np.array(T.M.LINES)
        for f in (0, 36):
            v = T.skin(parsed, name, f)[T.cap_centres()]
            assert np.abs(v[:, 0] - want[f, lines[:, 1]]).max() <= tol and np.abs(v[:, 1] - want[f, lines[:, 0]]).max() <= tol
    with capsys.disabled():
        print("twin's file: joint_positions - regrow(X) %.3g m" % worst)
    with pytest.raises(ValueError, match="no skeleton"):
        G.joint_positions(parsed, "gt")


def test_read_glb_refuses_what_is_out_of_bounds(G, frames37, tmp_path):
    data = _file_bytes(G, {"estimated": frames37[:2]})
    n_json = struct.unpack_from("<I", data, 12)[0]
    cases = {
        "truncated": data[:-4],
        "a truncated header": data[:10],
        "a wrong magic": b"glTf" + data[4:],
        "a wrong version": data[:4] + struct.pack("<I", 1) + data[8:],
        "a total length beyond the file": data[:8] + struct.pack("<I", len(data) + 4) + data[12:],
        "a JSON chunk length beyond the file": data[:12] + struct.pack("<I", len(data)) + data[16:],
        "a BIN chunk length beyond the file": data[:20 + n_json] + struct.pack("<I", len(data)) + data[24 + n_json:],
        "a chunk header cut": data[:20 + n_json + 4],
        "BIN first": data[:16] + struct.pack("<I", 0x004E4942) + data[20:],
        "an accessor beyond its view": data.replace(b'"count":77400', b'"count":77408'),          # (the index accessor)
    }
    assert cases["an accessor beyond its view"] != data
    for name, bad in cases.items():
        p = str(tmp_path / "bad.glb")
        with open(p, "wb") as f:
            f.write(bad)
        with pytest.raises(ValueError):
            G.read_glb(p)
            pytest.fail("read_glb accepted: " + name)


def test_cli_argument_errors(G, tmp_path, capsys):
    import pickle
    frames = [np.zeros((15, 3)) for _ in range(3)]
    no_gt = str(tmp_path / "no_gt.pkl")
    with open(no_gt, "wb") as f:
        pickle.dump({"estimated_pose": frames, "optimized_pose": np.asarray(frames)}, f)
    out = str(tmp_path / "o.glb")
    for argv, word in (([no_gt, "--out", out, "--align", "true"], "gt_pose"), ([no_gt], "--out"), (["--out", out], "pose_pickle"),
                       ([no_gt, "--out", out, "--fps", "0"], "--fps"), ([no_gt, "--out", out, "--fps", "fast"], "--fps")):
        with pytest.raises(SystemExit) as e:
            G.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    with pytest.raises(ValueError, match="ground-truth"):
        G.write_result_gltf(None, str(tmp_path / "d"), frames, frames, None, align=True)
    assert sorted(os.listdir(str(tmp_path))) == ["no_gt.pkl"]


def test_the_argument_is_wired_and_none_writes_nothing(G, tmp_path, monkeypatch):
    import inspect
    from globalegomocap_amd import optimizer, report, whole_sequence as ws
    cfg = ws._settings("cam.json", gltf="somewhere", gltf_fps=30.0)
    assert cfg.gltf == "somewhere" and cfg.gltf_fps == 30.0 and cfg.outputs == report.Outputs(gltf="somewhere", gltf_fps=30.0)
    assert ws._settings("cam.json").gltf is None and ws._settings("cam.json").gltf_fps is None
    assert ws._settings("cam.json", gltf_fps=30.0).outputs == report.Outputs()
    with pytest.raises(ValueError, match="gltf_fps"):
        ws._settings("cam.json", gltf="g", gltf_fps=0.0)
    for fn in (ws._settings, optimizer.main):
        par = inspect.signature(fn).parameters
        for name in ("gltf", "gltf_fps"):
            assert par[name].kind is inspect.Parameter.KEYWORD_ONLY and par[name].default is None, (fn, name)
    a = ws._parser().parse_args(["--data_path", "d", "--gltf", "G", "--gltf_fps", "50"])
    assert a.gltf == "G" and a.gltf_fps == 50.0
    a = ws._parser().parse_args(["--data_path", "d"])
    assert a.gltf is None and a.gltf_fps is None
    # the record: truthy with a root alone, equal and hashed by all its values, frozen
    o = report.Outputs(gltf="root")
    assert o and not report.Outputs() and not report.Outputs(gltf_fps=30) and o.gltf == "root" and o.gltf_fps is None
    assert o == report.Outputs(gltf="root") and o != report.Outputs() and o != report.Outputs(gltf="root", gltf_fps=30) and hash(o) == hash(report.Outputs(gltf="root"))
    assert "gltf='root'" in repr(o) and not o.needs_frames
    with pytest.raises(Exception):
        o.gltf = "elsewhere"
    monkeypatch.chdir(tmp_path)
    seqs = (np.zeros((3, 15, 3)), np.ones((3, 15, 3)), None)
    report.Outputs(gltf=None, gltf_fps=30).write(None, "studio/chunk_0", seqs)
    assert os.listdir(str(tmp_path)) == []
    calls = []
    monkeypatch.setattr(G, "write_result_gltf", lambda *a, **k: calls.append((a, k)))
    report.Outputs(gltf="root").write("engine", "data/studio/chunk_0", seqs)
    report.Outputs(gltf="root", gltf_fps=50).write("engine", "data/studio/chunk_0", seqs)
    assert [c[0][:2] for c in calls] == [("engine", os.path.join("root", "studio", "chunk_0"))] * 2
    assert [c[1] for c in calls] == [{"fps": 25}, {"fps": 50}] and calls[0][0][2] is seqs[0] and calls[0][0][3] is seqs[1] and calls[0][0][4] is None


def test_upright_and_foot_lock_reach_the_file_as_they_reach_the_bvh_files(G, monkeypatch):
    from globalegomocap_amd import bvh, foot_lock, ground, report
    calls = []
    monkeypatch.setattr(G, "write_result_gltf", lambda *a, **k: calls.append(("gltf", a, k)))
    monkeypatch.setattr(bvh, "write_result_bvh", lambda *a, **k: calls.append(("bvh", a, k)))
    monkeypatch.setattr(ground, "estimate_ground", lambda engine, reference, **k: "the estimate")

    class Lock:
        sequence = "the locked sequence"
    monkeypatch.setattr(foot_lock, "lock_feet", lambda *a, **k: Lock())
    seqs = (np.zeros((3, 15, 3)), np.ones((3, 15, 3)), None)
    assert report.Outputs(gltf="g", upright=True, foot_lock=True).write("engine", "d/studio/chunk_0", seqs) == "the estimate"
    assert len(calls) == 1 and calls[0][1][3] == "the locked sequence" and calls[0][2] == {"fps": 25, "upright": "the estimate"}
    del calls[:]
    report.Outputs(gltf="g", bvh="b", upright=True, foot_lock=True).write("engine", "d/studio/chunk_0", seqs)
    assert [c[0] for c in calls] == ["bvh", "gltf"] and calls[0][1][2:] == calls[1][1][2:] and calls[0][2] == calls[1][2]
