"""Skeleton meshes, the part that needs no GPU: the file layout, the header, the face block against the
numpy twin (tests/mesh_twin.py) and as a surface, `meshes.read_ply`'s strictness, and the argument errors of the entry points."""
import pickle

import numpy as np
import pytest

import mesh_twin as T


@pytest.fixture(scope="module")
def M():
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import meshes
    return meshes


@pytest.fixture(scope="module")
def faces(M):
    header, face_block = M.constant()
    return T.parse_face_block(face_block)


def generic_pose():
    from globalegomocap_amd import synth
    return synth.rest_skeleton() + np.random.default_rng(3).normal(0.0, 0.02, (15, 3))


def test_layout_and_header(M):
    import ctypes as C
    from globalegomocap_amd import _capi
    from globalegomocap_amd.skeleton import MESH_LINES
    lib = _capi.load_library()
    out = (C.c_int64 * 6)()
    assert lib.gem_skeleton_mesh_layout(out) == 0
    assert tuple(out) == (12960, 25800, len(T.HEADER), 349920, 335400, len(T.HEADER) + 349920 + 335400)
    assert tuple(M.layout()) == tuple(out) and M.layout().file_bytes == 685320 + len(T.HEADER)
    header, face_block = M.constant()
    assert header == T.HEADER and len(face_block) == 335400
    assert lib.gem_version() == 1
    assert [tuple(l) for l in MESH_LINES] == T.LINES and len(MESH_LINES) == 15
    assert lib.gem_skeleton_mesh_constant(None, None) != 0 and b"null" in lib.gem_last_error()


def test_face_block_is_the_twins(faces):
    _, _, want = T.frame_mesh(generic_pose())
    assert faces.shape == want.shape == (T.N_TRIANGLES, 3) and np.array_equal(faces, want)


def test_every_part_is_a_closed_outward_surface(faces):
    """Every edge shared by exactly two triangles, 30 connected parts, Euler characteristic 2 each, and -- with the twin's vertices
    for a generic pose -- a positive signed volume per part (faces point outward)."""
    verts, _, _ = T.frame_mesh(generic_pose())
    # connected parts over the whole face block: union-find over the vertices
    parent = np.arange(T.N_VERTICES)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in faces.tolist():
        ra, rb, rc = find(a), find(b), find(c)
        parent[rb] = ra
        parent[rc] = ra
    roots = {find(v) for v in range(T.N_VERTICES)}
    assert len(roots) == 30
    for k, (v0, nv, t0, nt) in enumerate(T.part_slices()):
        tri = faces[t0:t0 + nt]
        assert tri.min() == v0 and tri.max() == v0 + nv - 1, k
        assert len({find(v) for v in range(v0, v0 + nv)}) == 1, k
        edges = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
        assert (edges[:, 0] != edges[:, 1]).all(), k
        und, counts = np.unique(np.sort(edges, axis=1), axis=0, return_counts=True)
        assert (counts == 2).all(), (k, counts.min(), counts.max())
        # an orientable surface: every directed edge once
        assert len(np.unique(edges, axis=0)) == len(edges), k
        assert nv - len(und) + nt == 2, (k, nv, len(und), nt)
        p = verts[tri] - verts[v0:v0 + nv].mean(axis=0)
        volume = np.einsum("ni,ni->", p[:, 0], np.cross(p[:, 1], p[:, 2])) / 6
        ideal = 4 / 3 * np.pi * 0.02 ** 3 if k < 15 else np.pi * 0.005 ** 2 * np.linalg.norm(verts[v0] - verts[v0 + 1])
        assert 0.9 * ideal < volume < ideal, (k, volume, ideal)


def _write(path, M, vertex_block):
    header, face_block = M.constant()
    with open(path, "wb") as f:
        f.write(header + vertex_block + face_block)


def twin_vertex_block(pose):
    v, c, _ = T.frame_mesh(pose)
    rec = np.zeros((T.N_VERTICES, 27), dtype=np.uint8)
    rec[:, :24] = v.astype("<f8").view(np.uint8).reshape(T.N_VERTICES, 24)
    rec[:, 24:] = c
    return rec.tobytes()


def test_read_ply(M, tmp_path):
    pose = generic_pose()
    block = twin_vertex_block(pose)
    good = str(tmp_path / "good.ply")
    _write(good, M, block)
    v, c, t = M.read_ply(good)
    wv, wc, wt = T.frame_mesh(pose)
    assert v.dtype == np.float64 and c.dtype == np.uint8 and t.dtype == np.uint32
    assert np.array_equal(v, wv) and np.array_equal(c, wc) and np.array_equal(t, wt)
    tv, tc, tt = T.read_ply(good)
    assert np.array_equal(tv, v) and np.array_equal(tc, c) and np.array_equal(tt, t)
    data = open(good, "rb").read()
    header, _ = M.constant()
    cases = {
        "truncated": data[:-1],
        "too long": data + b"\0",
        "wrong vertex count": data.replace(b"element vertex 12960", b"element vertex 12961"),
        "wrong face count": data.replace(b"element face 25800", b"element face 25799"),
        "ascii": data.replace(b"format binary_little_endian 1.0", b"format ascii 1.0"),
        "big-endian": data.replace(b"binary_little_endian", b"binary_big_endian"),
        "float positions": data.replace(b"property double x", b"property float x"),
        "no ply": b"plx" + data[3:],
        "a quad": data[:len(header) + 349920] + b"\4" + data[len(header) + 349920 + 1:],
        "an index past the vertices": data[:-4] + (12960).to_bytes(4, "little"),
    }
    for name, bad in cases.items():
        p = str(tmp_path / "bad.ply")
        with open(p, "wb") as f:
            f.write(bad)
        with pytest.raises(ValueError):
            M.read_ply(p)
            pytest.fail("read_ply accepted: " + name)


def test_visualization_is_still_refused(tmp_path):
    from globalegomocap_amd import optimizer
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    with pytest.raises(NotImplementedError, match="save"):
        optimizer.main(str(tmp_path), DEFAULT_CALIBRATION, 0.0, 0.0, 0.001, 0.01, 0.01, 0.01, visualization=True)
    with pytest.raises(NotImplementedError, match="save"):
        optimizer.main(str(tmp_path), DEFAULT_CALIBRATION, 0.0, 0.0, 0.001, 0.01, 0.01, 0.01, visualization=True, save=True)


def test_cli_argument_errors(M, tmp_path, capsys):
    frames = [np.zeros((15, 3)) for _ in range(3)]
    no_gt = str(tmp_path / "no_gt.pkl")
    with open(no_gt, "wb") as f:
        pickle.dump({"estimated_pose": frames, "optimized_pose": np.asarray(frames), "mid_optimized_pose": frames}, f)
    no_opt = str(tmp_path / "no_opt.pkl")
    with open(no_opt, "wb") as f:
        pickle.dump({"estimated_pose": frames}, f)
    for argv, word in (([no_gt, "--out", str(tmp_path / "o"), "--align", "true"], "gt_pose"),
                       ([no_gt], "--out"),
                       (["--out", str(tmp_path / "o")], "pose_pickle"),
                       ([no_opt, "--out", str(tmp_path / "o")], "optimized_pose")):
        with pytest.raises(SystemExit) as e:
            M.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    assert not (tmp_path / "o").exists()
    from globalegomocap_amd import whole_sequence as ws
    cfg = ws._settings("cam.json", save=True, mesh_root="somewhere")
    assert cfg.save is True and cfg.mesh_root == "somewhere"
    assert ws._settings("cam.json").save is False and ws._settings("cam.json").mesh_root == "out"
    with pytest.raises(ValueError, match="ground-truth"):
        M.write_result_meshes(None, str(tmp_path / "o"), frames, frames, None, align=True)
