"""CPU-only checks of the data preparation (globalegomocap_amd/prepare.py): the library's MAT-file scanner against
scipy.io.loadmat, the files it refuses on purpose, its robustness against damaged files, and the host-side logic (listing order,
ground-truth indexing, chunk loop, the pickle's containers) against the reference's golden run (tests/golden/prepare.npz,
tools/make_golden_prepare.py)."""
import os
import pickle
import struct
import zlib

import numpy as np
import pytest
import scipy.io as sio


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import prepare
    return prepare


def _assert_same(got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert np.array_equal(got, ref, equal_nan=got.dtype.kind in "fc")
    assert got.flags.f_contiguous == ref.flags.f_contiguous


def test_struct_layout_of_the_scanner_result():
    import ctypes as C
    from globalegomocap_amd import _capi
    assert C.sizeof(_capi.GemMatArray) == 4 * 8 + 6 * 4 + 4 * 8 and _capi.GemMatArray.dims.offset == 56


# ------------------------------------------------------------------------------------------------ the scanner against loadmat
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(64, 64, 15), (1, 15)])
def test_mat_scanner_against_loadmat(P, tmp_path, dtype, shape):
    """For every accepted file: the bytes at the reported offset, read with the reported type and dims in column-major order, are
    loadmat's array.  Names of 1 and 4 characters use the small-data-element form (savemat packs them into the tag)."""
    from globalegomocap_amd import _capi
    rng = np.random.default_rng(5)
    for name in ("h", "heat", "heatm", "heatmap12"):
        for front in (False, True):
            for comp in (False, True):
                a = rng.standard_normal(shape).astype(dtype)
                d = {"zz_front": np.arange(7.0).reshape(1, 7)} if front else {}
                d[name] = a
                path = str(tmp_path / "x.mat")
                sio.savemat(path, d, do_compression=comp)
                ref = sio.loadmat(path)[name]
                buf = open(path, "rb").read()
                rc, out, why = P.mat_scan(buf, name)
                assert rc == 0, why
                if comp:
                    assert out.compressed == 1 and 128 <= out.offset and out.offset + out.nbytes <= len(buf)
                    image, start = None, 0
                    while image is None:          # (the variable in front is an element of its own: resume behind it)
                        raw = zlib.decompress(buf[out.offset:out.offset + out.nbytes])
                        rc2, got, why = P.mat_scan(raw, name, bare=True)
                        if rc2 == _capi.MAT_NOT_FOUND:
                            start = out.next
                            rc, out, why = P.mat_scan(buf, name, start)
                            assert rc == 0 and out.compressed == 1, why
                            continue
                        assert rc2 == 0 and not got.compressed, why
                        image, out = raw, got
                else:
                    assert out.compressed == 0
                    image = buf
                assert out.storage == (_capi.MI_SINGLE if dtype is np.float32 else _capi.MI_DOUBLE)
                assert out.mat_class == (7 if dtype is np.float32 else 6)
                dims = tuple(out.dims[:out.ndim])
                assert dims == shape and out.nbytes == int(np.prod(shape)) * np.dtype(dtype).itemsize
                assert 0 <= out.offset and out.offset + out.nbytes <= len(image)
                _assert_same(np.frombuffer(image, dtype=dtype, count=int(np.prod(shape)), offset=out.offset).reshape(dims, order="F"), ref)
                got, how = P.read_mat_array(path, name)
                assert how == "native"
                _assert_same(got, ref)


def test_the_fact_the_device_path_rests_on(P, tmp_path):
    """savemat({'heatmap': float32[64,64,15]}) writes a 245 960-byte file whose payload (tag miSINGLE, 245 760) starts at byte 200,
    column-major."""
    a = np.random.default_rng(0).random((64, 64, 15), dtype=np.float32)
    path = str(tmp_path / "h.mat")
    sio.savemat(path, {"heatmap": a})
    buf = open(path, "rb").read()
    rc, out, why = P.mat_scan(buf, "heatmap")
    assert rc == 0 and (len(buf), out.offset, out.nbytes) == (245960, 200, 245760), why
    assert struct.unpack_from("<II", buf, 192) == (7, 245760)
    assert np.array_equal(np.frombuffer(buf, np.float32, 64 * 64 * 15, 200).reshape(15, 64, 64), a.transpose(2, 1, 0))


# ------------------------------------------------------------------------------------------------ refused on purpose
def _refused(P, tmp_path, buf, name, loadable=True):
    rc, _, why = P.mat_scan(buf, name)
    assert rc == 2 and why.strip(), (rc, why)          # GEM_MAT_UNSUPPORTED, with a reason
    path = str(tmp_path / "r.mat")
    with open(path, "wb") as f:
        f.write(buf)
    if loadable:
        ref = sio.loadmat(path)[name]
        got, how = P.read_mat_array(path, name)
        assert how == "loadmat"
        if hasattr(ref, "toarray"):
            assert (got != ref).nnz == 0
        elif ref.dtype.names or ref.dtype == object:
            assert got.dtype == ref.dtype and got.shape == ref.shape
        else:
            _assert_same(got, ref)
    return why


def test_files_outside_the_subset_are_refused_with_a_reason_and_read_by_loadmat(P, tmp_path):
    def saved(d, **kw):
        path = str(tmp_path / "s.mat")
        sio.savemat(path, d, **kw)
        return bytearray(open(path, "rb").read())
    # a double array that MATLAB stored as miUINT8: savemat writes a uint8 array (class uint8 = 9, tag miUINT8); its class byte is
    # patched to mxDOUBLE (6).  loadmat (mat_dtype=False) returns it in its storage type.
    buf = saved({"depth": np.arange(15, dtype=np.uint8).reshape(1, 15)})
    assert buf[128 + 8 + 8] == 9
    buf[128 + 8 + 8] = 6
    why = _refused(P, tmp_path, bytes(buf), "depth")
    assert "stored in another type" in why
    assert sio.loadmat(str(tmp_path / "r.mat"))["depth"].dtype == np.uint8
    # complex, sparse, struct, logical, character, integer classes
    for value, word in ((np.arange(6.0).reshape(2, 3) * (1 + 2j), "complex"), (__import__("scipy.sparse").sparse.eye(3).tocsc(), "sparse"),
                        ({"a": np.arange(3.0)}, "struct"), (np.array([[True, False]]), "class"), ("text", "character"),
                        (np.arange(6, dtype=np.int32).reshape(2, 3), "class")):
        why = _refused(P, tmp_path, bytes(saved({"v": value})), "v")
        assert word in why, why
    # big-endian: a little-endian file with the marker swapped cannot be read by anyone; build the header only
    buf = saved({"v": np.arange(3.0)})
    big = bytearray(buf)
    big[124:128] = b"\x01\x00MI"
    assert "big-endian" in _refused(P, tmp_path, bytes(big), "v", loadable=False)
    # a v4 header (a zero among the first four bytes), an HDF5 signature, version 0x0200
    v4 = bytearray(buf)
    v4[0:4] = b"\x00\x00\x00\x00"
    assert "v4" in _refused(P, tmp_path, bytes(v4), "v", loadable=False)
    path = str(tmp_path / "four.mat")
    sio.savemat(path, {"v": np.arange(3.0).reshape(1, 3)}, format="4")
    raw4 = open(path, "rb").read()
    assert "v4" in _refused(P, tmp_path, raw4, "v")
    assert "HDF5" in _refused(P, tmp_path, b"\x89HDF\r\n\x1a\n" + bytes(600), "v", loadable=False)
    v73 = bytearray(buf)
    v73[124:126] = b"\x00\x02"
    assert "HDF5" in _refused(P, tmp_path, bytes(v73), "v", loadable=False)
    # a name that is not there: its own return code
    rc, _, why = P.mat_scan(bytes(buf), "w")
    assert rc == 3 and "no variable" in why


# ------------------------------------------------------------------------------------------------ robustness
def test_mat_scanner_survives_damaged_files(P, tmp_path):
    """Single-byte and truncation mutations over the WHOLE file.  Allowed: a refusal, an error return, or an accepted array whose
    reported range lies inside [0, len) and whose length is the product of its dims times the item size; where loadmat also reads
    the mutated file without raising, the two arrays are equal.  Zero violations."""
    import subprocess
    import sys
    rng = np.random.default_rng(11)
    cases = []
    for name, a, front, comp in (("depth", rng.random((1, 15)), False, False), ("d", rng.random((1, 15)).astype(np.float32), True, False),
                                 ("heatmap", rng.random((4, 4, 3)).astype(np.float32), False, False),
                                 ("heatmap", rng.random((4, 4, 3)), True, True)):
        d = {"zz": np.arange(3.0).reshape(1, 3)} if front else {}
        d[name] = a
        path = str(tmp_path / "m.mat")
        sio.savemat(path, d, do_compression=comp)
        cases.append((name, open(path, "rb").read()))
    n_mut, accepted = 0, []
    for ci, (name, buf) in enumerate(cases):
        muts = []
        for pos in range(len(buf)):          # every byte of the file once, with a random other value ...
            muts.append((pos, int((buf[pos] + rng.integers(1, 256)) % 256), len(buf)))
        for pos in range(116, min(len(buf), 260)):          # ... the header's tail and the tags more thoroughly ...
            for v in (0, 1, 2, 5, 6, 7, 9, 14, 15, 0x80, 0xff):
                if v != buf[pos]:
                    muts.append((pos, v, len(buf)))
        for cut in list(range(0, min(len(buf), 300))) + rng.integers(0, len(buf), 40).tolist():          # ... and truncations
            muts.append((None, None, int(cut)))
        for pos, v, cut in muts:
            m = bytearray(buf[:cut])
            if pos is not None:
                m[pos] = v
            m = bytes(m)
            n_mut += 1
            hit = P.locate(m, name)
            if hit is None:
                continue
            image, off, dt, dims = hit
            nbytes = int(np.prod(dims, dtype=np.int64)) * np.dtype(dt).itemsize
            assert 0 <= off and off + nbytes <= len(image), (pos, v, cut)
            k = len(accepted)
            with open(str(tmp_path / ("mut%d.mat" % k)), "wb") as f:
                f.write(m)
            np.save(str(tmp_path / ("mut%d.npy" % k)), P.array_at(image, off, dt, dims))
            accepted.append((ci, name, pos, v, cut))
    # loadmat on the accepted files, in a child process: scipy's own reader is not safe against damaged files (it can take the
    # interpreter down on a damaged variable IN FRONT of the wanted one, which the library's scanner steps over unread); a file
    # on which it crashes counts as one it does not read
    verdict, at = {}, 0
    while at < len(accepted):
        r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path), str(at), str(len(accepted))] + [a[1] for a in accepted[at:]],
                           capture_output=True, text=True)
        for line in r.stdout.split():
            k, _, what = line.partition(":")
            verdict[int(k)] = what
        if r.returncode == 0:
            break
        at = max(verdict, default=at - 1) + 2          # (the file after the last one reported took the child down)
        verdict[at - 1] = "crash"
    assert len(verdict) == len(accepted)
    differ = [accepted[k] for k, w in verdict.items() if w == "differ"]
    assert not differ, differ
    n_both = sum(w == "same" for w in verdict.values())
    assert n_mut > 3000 and len(accepted) > 100 and n_both > 100, (n_mut, len(accepted), n_both)


_CHILD = """
import sys, warnings
import numpy as np
import scipy.io as sio
root, first, last = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
warnings.simplefilter("ignore")
for k in range(first, last):
    got = np.load("%s/mut%d.npy" % (root, k))
    try:
        ref = sio.loadmat("%s/mut%d.mat" % (root, k))[sys.argv[4 + k - first]]
    except Exception:
        print("%d:raise" % k, flush=True)
        continue
    same = got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True)
    print("%d:%s" % (k, "same" if same else "differ"), flush=True)
"""


# ------------------------------------------------------------------------------------------------ host-side logic against the golden
def test_payload_tables_special_cases(P, tmp_path):
    """`payload_tables` on host data alone: where every frame's payloads lie after the reader threads' pass.  The special cases: a
    float64 heat-map (kept for the pickle), a compressed and a loadmat'ed heat-map (they travel behind the block), a depth of several
    rows inside the block and one that came through loadmat (first row only).  Reading the tables back must give loadmat's arrays."""
    from globalegomocap_amd import _capi, staging
    rng = np.random.default_rng(5)
    heats =[rng.random((8, 6, 15), dtype=np.float32), rng.random((8, 6, 15)), rng.random((8, 6, 15), dtype=np.float32),
             rng.integers(0, 200, (8, 6, 15)).astype(np.uint8)]                       # (uint8: outside the scanner's subset -> loadmat)
    depths = [rng.random((1, 15)), rng.random((3, 15)), rng.random((1, 15)).astype(np.float32), rng.integers(0, 9, (2, 15)).astype(np.int32)]
    n, paths = len(heats), []
    for k, (name, arrays) in enumerate(((P.HEAT_NAME, heats), (P.DEPTH_NAME, depths))):
        for f, a in enumerate(arrays):
            paths.append(str(tmp_path / ("%s_%d.mat" % (name, f))))
            sio.savemat(paths[-1], {name: a}, do_compression=(k == 0 and f == 2))
    sizes = np.array([os.path.getsize(q) for q in paths], dtype=np.int64)
    at, room, total = staging.side_by_side(sizes, 16)
    assert (at % 16 == 0).all() and (room >= sizes + 8).all() and total == at[-1] + room[-1]
    block = np.zeros(total, dtype=np.uint8)
    found, rcs = (_capi.GemMatArray * (2 * n))(), np.zeros(2 * n, dtype=np.int32)
    extra, sent = P._read_range(_capi.load_library(), P._c_paths(paths), 0, 2 * n, at, sizes, n, block, found, rcs, paths)
    assert sent is None and sorted(e[0] for e in extra) == [2, 3, 7] and rcs.tolist() == [0, 0, -1, -1, 0, 0, 0, -1]
    where, kinds, shape, heat_files, parts, end = P.payload_tables(n, paths, at, found, rcs, extra, block)
    assert shape == (8, 6, 15) and end >= total and all(total <= o and o + len(b) <= end for o, b in parts)
    image = np.zeros(end, dtype=np.uint8)
    image[:total] = block
    for o, b in parts:
        image[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    for f in range(n):
        ref_h, ref_d = sio.loadmat(paths[f])[P.HEAT_NAME], sio.loadmat(paths[n + f])[P.DEPTH_NAME][0]
        dt = np.float64 if kinds[f] & _capi.MAT_HEAT_F64 else np.float32
        got = np.frombuffer(image, dtype=dt, count=ref_h.size, offset=int(where[f])).reshape(ref_h.shape, order="F")
        assert np.array_equal(got.astype(np.float32), ref_h.astype(np.float32)), f
        dt = np.float32 if kinds[f] & _capi.MAT_DEPTH_F32 else np.float64
        assert np.array_equal(np.frombuffer(image, dtype=dt, count=15, offset=int(where[n + f])).astype(np.float64), ref_d.astype(np.float64)), f
        if ref_h.dtype == np.float32:
            assert heat_files[f] is None
        else:
            _assert_same(heat_files[f], ref_h)
    assert kinds.tolist() == [0, _capi.MAT_HEAT_F64, _capi.MAT_DEPTH_F32, 0]
    sio.savemat(paths[0], {P.HEAT_NAME: heats[0][:, :5]})          # one heat-map of another shape (a smaller file: its room still holds it)
    sizes[0] = os.path.getsize(paths[0])
    rcs[:] = 0
    extra, _ = P._read_range(_capi.load_library(), P._c_paths(paths), 0, 2 * n, at, sizes, n, block, found, rcs, paths)
    with pytest.raises(ValueError, match="one shape"):
        P.payload_tables(n, paths, at, found, rcs, extra, block)


def test_listing_order_and_slice(P, golden, tmp_path):
    g = golden("prepare")
    names = [str(x) for x in g["names"]]
    for n in names:
        open(str(tmp_path / n), "wb").close()
    assert sorted(names) != sorted(names, key=__import__("globalegomocap_amd.whole_sequence", fromlist=["x"]).natural_key)
    a, b = (int(v) for v in g["range_a"])
    got = [os.path.basename(p) for p in P.list_frames(str(tmp_path), a, b)]
    assert got == ["frame_%d.mat" % k for k in range(a, b)]          # an index into the naturally sorted listing
    os.remove(str(tmp_path / "frame_0.mat"))                          # ... not a frame id: one file less shifts the window
    assert [os.path.basename(p) for p in P.list_frames(str(tmp_path), a, b)][0] == "frame_%d.mat" % (a + 1)


def test_gt_indexing_and_restricted_unpickler(P, golden, tmp_path):
    g = golden("prepare")
    gt = [np.array(x) for x in g["gt"]]
    path = str(tmp_path / "gt.pkl")
    with open(path, "wb") as f:
        pickle.dump(gt, f)
    pose_gt = P.read_gt(path)
    ms = int(g["mat_start_frame"])
    for tag in ("a", "b", "loop0", "loop1"):
        a, b = (int(v) for v in g["range_" + tag])
        assert a != ms or tag == "loop0"
        clip = P.gt_clip(pose_gt, a, b, ms)
        assert isinstance(clip, list) and all(c is pose_gt[i - ms] for c, i in zip(clip, range(a, b)))          # untouched
        np.testing.assert_array_equal(np.asarray(clip), g["gt_global_skeleton_" + tag])

    class Evil:
        def __reduce__(self):
            return (os.system, ("true",))
    with open(path, "wb") as f:
        pickle.dump([Evil()], f)
    with pytest.raises(pickle.UnpicklingError):
        P.read_gt(path)


def test_chunk_loop_bounds(P, golden):
    g = golden("prepare")
    t0, t1, size = (int(v) for v in g["loop"])
    assert (t1 - t0) % size == 0
    spans = P.chunk_spans(t0, t1, size)
    assert len(spans) == int(g["loop_chunks"]) == (t1 - t0) // size - 1          # the dropped last chunk
    assert spans == [tuple(int(v) for v in g["range_loop%d" % k]) for k in range(len(spans))]
    assert P.chunk_spans(551, 3300, 100)[0] == (551, 651) and P.chunk_spans(551, 3300, 100)[-1] == (3151, 3251)
    assert P.chunk_spans(0, 100, 100) == [] and P.chunk_spans(0, 101, 100) == [(0, 100)]


def test_missing_trajectory_frames_raise(P, golden):
    g = golden("prepare")
    rows = g["rows"]
    text = "\n".join(" ".join("%.9f" % v for v in r) for r in rows)
    fps = int(g["fps"])
    P.check_trajectory(text, 3, 15, fps)
    text = "\n".join(" ".join("%.9f" % v for v in r) for k, r in enumerate(rows) if k not in (7, 9))
    with pytest.raises(ValueError, match=r"\[7, 9\]"):
        P.check_trajectory(text, 3, 15, fps)
    P.check_trajectory(text, 10, 27, fps)


def test_chunk_dict_containers_dtypes_and_order(P, golden, tmp_path):
    """Recording.chunk_dict built from the golden's arrays: keys and their order, lists of per-frame arrays, dtypes and order flags
    as the reference pickled them; the file loads with plain pickle.load; the project's own reader takes its native path."""
    from globalegomocap_amd import synth_recording as S
    g = golden("prepare")
    tag = "a"
    a, b = (int(v) for v in g["range_" + tag])
    heat64 = S.paraboloid_heatmaps(g["centres"], g["radii"])
    assert S.sha256(heat64) == str(g["heat_sha256"])
    as64 = g["as_float64"]
    files = [heat64[k].copy(order="F") if as64[k] else None for k in range(a, b)]
    gt_list = [np.array(x) for x in g["gt_global_skeleton_" + tag]]
    chunk = P.RecordingChunk(a, b, heat64[a:b].astype(np.float32), g["estimated_local_skeleton_" + tag], g["estimated_global_skeleton_" + tag],
                             g["camera_pose_list_" + tag], g["gt_global_skeleton_" + tag], gt_list=gt_list, heat_files=files)
    rec = P.Recording([chunk])
    d = rec.chunk_dict(0)
    assert list(d) == [str(k) for k in g["keys_" + tag]] == list(P.PICKLE_KEYS)
    flag = lambda x: [x.dtype.str, "F" if (x.flags.f_contiguous and not x.flags.c_contiguous) else "C"]      # noqa: E731
    for k in P.PICKLE_KEYS:
        assert isinstance(d[k], list) and len(d[k]) == b - a
        assert [flag(x) for x in d[k]] == g[k + "_flags_" + tag].tolist(), k
    assert d["gt_global_skeleton"] is gt_list
    for k in P.PICKLE_KEYS[:4]:
        np.testing.assert_array_equal(np.asarray(d[k]), g[k + "_" + tag])
    assert [S.sha256(np.ascontiguousarray(x)) for x in d["heatmap_list"]] == g["heatmap_list_sha256_" + tag].tolist()
    out = rec.write_chunks(str(tmp_path))
    assert out == [str(tmp_path / ("data_start_%d_end_%d" % (a, b)))]
    with open(os.path.join(out[0], "test_data.pkl"), "rb") as f:
        raw = f.read()
    assert raw[0] == 0x80 and raw[1] == pickle.DEFAULT_PROTOCOL
    back = pickle.loads(raw)
    assert list(back) == list(P.PICKLE_KEYS)
    assert [flag(x) for x in back["estimated_local_skeleton"]] == g["estimated_local_skeleton_flags_" + tag].tolist()
    assert [flag(x) for x in back["heatmap_list"]] == g["heatmap_list_flags_" + tag].tolist()
    from globalegomocap_amd.whole_sequence import parse_chunk
    c = parse_chunk(out[0], native=True)
    np.testing.assert_array_equal(c["est_local"], g["estimated_local_skeleton_" + tag])
    np.testing.assert_array_equal(c["cams"], g["camera_pose_list_" + tag])
    np.testing.assert_array_equal(c["gt"], g["gt_global_skeleton_" + tag])
    assert c["n"] == b - a


def test_scale_from_head_joints_is_the_scale_from_whole_skeletons(golden):
    """slam.camera_pose_list_from_heads against slam.camera_pose_list (pinned by tests/golden/slam.npz) and against the reference's
    cameras in prepare.npz (1e-12, the SLAM preparation's tolerance)."""
    from globalegomocap_amd import slam
    g = golden("prepare")
    text = "\n".join(" ".join("%.9f" % v for v in r) for r in g["rows"])
    fps = int(g["fps"])
    for tag in ("a", "b", "loop0", "loop1"):
        a, b = (int(v) for v in g["range_" + tag])
        loc, gt = g["estimated_local_skeleton_" + tag], g["gt_global_skeleton_" + tag]
        m0, R0, t0 = slam.camera_pose_list(text, loc, gt, a, b, fps)
        m1, R1, t1 = slam.camera_pose_list_from_heads(text, loc[:, 0], gt[:, 0], a, b, fps)
        assert np.array_equal(m0, m1) and np.array_equal(R0, R1) and np.array_equal(t0, t1)
        np.testing.assert_allclose(m1, g["camera_pose_list_" + tag], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the two preparation command lines
SHARED_OPTIONS = ("slam", "gt", "scale", "bridge", "start", "end", "fps", "mat_start", "test_size", "out", "camera", "optimize")
OWN_ARGUMENTS = {"prepare": ["--heatmaps", "h", "--depths", "d"], "detections": ["--keypoints", "k"]}


def test_the_preparation_parsers_share_their_options():
    from globalegomocap_amd import detections, prepare
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION
    parsers = {"prepare": prepare._parser(), "detections": detections._parser()}
    actions = {m: {a.dest: a for a in p._actions} for m, p in parsers.items()}
    for dest in SHARED_OPTIONS:
        a, b = actions["prepare"][dest], actions["detections"][dest]
        assert (a.option_strings, a.default, a.help, a.required, a.nargs, a.const, a.metavar) == \
            (b.option_strings, b.default, b.help, b.required, b.nargs, b.const, b.metavar), dest
    a = actions["prepare"]
    assert (a["fps"].default, a["test_size"].default, a["camera"].default, a["bridge"].const) == (25, 100, DEFAULT_CALIBRATION, 1.0)
    assert all(a[d].default is None for d in ("gt", "scale", "bridge", "mat_start", "out")) and a["optimize"].default is False
    full = ["--slam", "t", "--scale", "auto", "--bridge", "0.4", "--start", "3", "--end", "90", "--fps", "30", "--mat_start", "2", "--test_size", "20",
            "--out", "o", "--camera", "c.json", "--optimize"]
    parsed = {m: vars(p.parse_args(OWN_ARGUMENTS[m] + full)) for m, p in parsers.items()}
    want = dict(slam="t", gt=None, scale="auto", bridge=0.4, start=3, end=90, fps=30.0, mat_start=2, test_size=20, out="o", camera="c.json",
                optimize=True)
    for m in parsers:
        assert {d: parsed[m][d] for d in SHARED_OPTIONS} == want, m
    # the commands that take both routes declare the same options: `continuous` the track's, `slam_scale` the depth route's
    from globalegomocap_amd import continuous, slam_scale
    declared = lambda x: (x.option_strings, x.default, x.required, x.nargs, x.const, x.metavar, x.type, x.choices)      # noqa: E731
    other = {x.dest: x for x in continuous._parser()._actions}
    for dest in ("slam", "gt", "scale", "knot", "stiffness", "bridge", "start", "end", "fps", "mat_start", "camera"):
        assert declared(a[dest]) == declared(other[dest]), dest
        assert dest == "gt" or a[dest].help == other[dest].help, dest
    other = {x.dest: x for x in slam_scale._parser()._actions}
    for dest in ("depths", "depth_from", "bones", "neck_depth", "min_peak"):
        assert declared(a[dest]) == declared(other[dest]), dest


@pytest.mark.parametrize("module", ["prepare", "detections"])
def test_the_preparation_command_lines_refuse_what_they_refused(module, capsys):
    """Before any file is opened."""
    import importlib
    m = importlib.import_module("globalegomocap_amd." + module)
    base = OWN_ARGUMENTS[module] + ["--slam", "t", "--start", "0", "--end", "9"]
    for argv, message in ((base + ["--gt", "g", "--bridge", "--out", "o"],
                           "error: --bridge needs --scale: with --gt every chunk has its own scale and there is no common world to bridge in"),
                          (base + ["--scale", "1"], "error: nothing to do: give --out, --optimize or both"),
                          (base + ["--gt", "g", "--scale", "1", "--out", "o"], "error: argument --scale: not allowed with argument --gt"),
                          (base + ["--out", "o"], "error: one of the arguments --gt --scale is required")):
        with pytest.raises(SystemExit) as e:
            m._cli(argv)
        assert e.value.code == 2 and capsys.readouterr().err.rstrip().endswith(message), argv


def _stub_recording(P, mpjpe=(None, None), reports=False):
    """Two chunks of host-only stubs: nothing of them is on a device, and nothing but their frame range and error is printed."""
    from globalegomocap_amd import _capi, slam_bridge, slam_scale
    chunks = [P.RecordingChunk(a, a + 26, None, np.zeros((26, 15, 3)), None, None, None, initial_mpjpe=e) for a, e in zip((0, 26), mpjpe)]
    if not reports:
        return P.Recording(chunks)
    scale = slam_scale.ScaleEstimate(np.arange(_capi.SCALE_REPORT_DOUBLES + 3 * 2, dtype=np.float64))
    bridge = slam_bridge.BridgeReport(np.zeros(_capi.BRIDGE_RECORD_DOUBLES), np.zeros(52, dtype=bool), [], 25, 1.0)
    return P.Recording(chunks, np.zeros((2, 4, 4)), scale.scale, scale, bridge)


def test_the_report_printer(capsys):
    from globalegomocap_amd import prepare as P
    running = ["running test sequence from 0 to 26", "running test sequence from 26 to 52"]

    def lines(rec, **kw):
        capsys.readouterr()
        P.print_report(rec, **kw)
        return capsys.readouterr().out.splitlines()
    rec = _stub_recording(P, reports=True)
    reports = [rec.scale_report.line(), rec.bridge_report.line()]
    assert reports[0].startswith("SLAM scale estimate: ") and reports[1].startswith("SLAM bridge: 0 of 0 frames invented in 0 gaps")
    assert lines(rec) == reports + running          # (`prepare_sequence`, `detections`)
    assert lines(rec, sequence=False) == reports          # (`main`)
    rec = _stub_recording(P)
    assert lines(rec) == running and lines(rec, sequence=False) == []
    rec = _stub_recording(P, mpjpe=(0.0625, 0.125))
    assert lines(rec) == [running[0], "The initial mpjpe is: 0.0625", running[1], "The initial mpjpe is: 0.125"]
    assert lines(rec, sequence=False) == ["The initial mpjpe is: 0.0625", "The initial mpjpe is: 0.125"]
