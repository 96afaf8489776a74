"""Data preparation on the device (globalegomocap_amd/prepare.py): gem_mat_frames bit for bit against loadmat, `main` and the
chunk loop against the unmodified reference's run (tests/golden/prepare.npz, tools/make_golden_prepare.py), the round trip
through the project's own chunk reader, and optimize_recording against write_chunks + optimize_directory."""
import os
import pickle

import numpy as np
import pytest
import scipy.io as sio

from globalegomocap_amd.camera import DEFAULT_CALIBRATION

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import prepare
    return prepare


def _flag(x):
    return [x.dtype.str, "F" if (x.flags.f_contiguous and not x.flags.c_contiguous) else "C"]


def _special_values(rng, shape, dtype):
    a = rng.standard_normal(shape).astype(dtype)
    flat = a.reshape(-1)
    flat[:6] = [np.nan, -0.0, 0.0, np.inf, -np.inf, 1.0]
    if dtype is np.float32:
        flat[6:10] = np.array([1e-40, -1e-42, 1.4e-45, -1.4e-45], dtype=np.float32)          # denormals
    else:
        # float64 values on and next to float32 ties: 1 + 2^-24 is the tie between 1 and 1 + 2^-23 (to even: 1), 1 + 3 * 2^-24 the
        # tie between 1 + 2^-23 and 1 + 2^-22 (to even: the latter); their neighbours round away from the tie; float64 denormals
        # and values below float32's smallest denormal flush to (signed) zero, 2^-149 * 0.5 is a tie that goes to zero
        t = 2.0 ** -24
        flat[6:16] = [1 + t, 1 + 3 * t, np.nextafter(1 + t, 2), np.nextafter(1 + t, 0), np.nextafter(1 + 3 * t, 2), np.nextafter(1 + 3 * t, 0),
                      5e-324, -1e-310, 2.0 ** -150, np.nextafter(2.0 ** -150, 1)]
        flat[16:18] = [3.5e38, -1e39]                                                          # beyond float32: +-inf
    return a


def test_mat_frames_bit_for_bit_against_loadmat(P, tmp_path):
    """A mixed batch in ONE launch: float32 and float64 heat-maps, inflated elements, payloads at different offsets (names of other
    lengths cannot be used for the heat-map itself, so a variable in front of it moves the payload), file images at ODD arena
    offsets, depths stored as double and as single; NaN, -0.0, denormals, float64 values that round across a float32 tie."""
    import torch
    rng = np.random.default_rng(3)
    n, J = 9, 15
    arena, where_h, where_d, kinds, ref_h, ref_d = bytearray(b"\x00" * 3), [], [], [], [], []

    def put(path, name, turn):
        """The file's image (or its inflated element) into the arena at an odd offset -> the payload's place and type."""
        hit = P.locate(open(path, "rb").read(), name)
        assert hit is not None
        image, off, dt, dims = hit
        while len(arena) % 8 != (1, 3, 5, 7)[turn % 4]:          # an odd offset, another residue every time
            arena.append(0xEE)
        base = len(arena)
        arena.extend(bytes(image))
        return base + off, dt

    for f in range(n):
        dt = np.float64 if f % 3 == 1 else np.float32
        h = _special_values(rng, (64, 64, J), dt)
        ddt = np.float32 if f % 4 == 2 else np.float64
        d = rng.uniform(0.2, 3.0, (1, J)).astype(ddt)
        d[0, :3] = [np.nan, -0.0, 1e-40 if ddt is np.float32 else 1e-310]
        hp, dp = str(tmp_path / ("h%d.mat" % f)), str(tmp_path / ("d%d.mat" % f))
        front = {"a" * (1 + f): np.arange(1.0 + f).reshape(1, -1)} if f % 2 else {}          # a variable in front: other payload offsets
        sio.savemat(hp, dict(front, heatmap=h), do_compression=(f % 4 == 3))
        sio.savemat(dp, dict(front, depth=d), do_compression=(f % 4 == 3))
        oh, th = put(hp, "heatmap", f)
        od, td = put(dp, "depth", f + 1)
        assert th is dt and td is ddt
        where_h.append(oh); where_d.append(od)
        kinds.append((1 if dt is np.float64 else 0) | (2 if ddt is np.float32 else 0))
        ref_h.append(torch.from_numpy(np.ascontiguousarray(sio.loadmat(hp)["heatmap"])).float().numpy())
        ref_d.append(sio.loadmat(dp)["depth"][0].astype(np.float64))
    assert len({w % 8 for w in where_h}) > 2 and any(w % 2 for w in where_h) and set(kinds) >= {0, 1, 2}
    dev = torch.device("cuda", 0)
    image_len = len(arena)
    arena.extend(b"\x00" * 16)
    arena_d = torch.from_numpy(np.frombuffer(bytes(arena), dtype=np.uint8).copy()).to(dev)
    heat = torch.full((n, 64, 64, J), 7.0, dtype=torch.float32, device=dev)
    depth = torch.full((n, J), 7.0, dtype=torch.float64, device=dev)
    P.mat_frames(arena_d, image_len, torch.tensor(where_h, dtype=torch.int64, device=dev), torch.tensor(where_d, dtype=torch.int64, device=dev),
                 torch.tensor(kinds, dtype=torch.int32, device=dev), heat, depth)
    torch.cuda.synchronize()
    got_h, got_d = heat.cpu().numpy(), depth.cpu().numpy()
    for f in range(n):
        assert np.array_equal(got_h[f].view(np.uint32), ref_h[f].view(np.uint32)) or \
            np.array_equal(got_h[f], ref_h[f], equal_nan=True) and np.array_equal(np.signbit(got_h[f]), np.signbit(ref_h[f])), f
        assert np.array_equal(got_d[f], ref_d[f], equal_nan=True) and np.array_equal(np.signbit(got_d[f]), np.signbit(ref_d[f])), f
    # a generic geometry takes the kernel's run-time path
    h = rng.standard_normal((2, 20, 12, 5)).astype(np.float32)
    blob, wh, wd = bytearray(b"\x00"), [], []
    for f in range(2):
        wh.append(len(blob)); blob.extend(np.asfortranarray(h[f]).tobytes(order="F"))
        wd.append(len(blob)); blob.extend(np.arange(5.0).tobytes())
    ilen = len(blob)
    blob.extend(b"\x00" * 16)
    heat2 = torch.empty((2, 20, 12, 5), dtype=torch.float32, device=dev)
    depth2 = torch.empty((2, 5), dtype=torch.float64, device=dev)
    P.mat_frames(torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).to(dev), ilen, torch.tensor(wh, device=dev), torch.tensor(wd, device=dev),
                 torch.zeros(2, dtype=torch.int32, device=dev), heat2, depth2)
    assert np.array_equal(heat2.cpu().numpy(), h) and np.array_equal(depth2.cpu().numpy(), np.tile(np.arange(5.0), (2, 1)))


def _golden_recording(golden, root):
    from globalegomocap_amd import synth_recording as S
    g = golden("prepare")
    heat64 = S.paraboloid_heatmaps(g["centres"], g["radii"])
    assert S.sha256(heat64) == str(g["heat_sha256"]), "the recipe that rebuilds the golden's pixels has drifted"
    paths = S.write_recording(str(root), heat64, g["depth"], [str(x) for x in g["names"]], g["as_float64"], g["compressed"], g["rows"], g["gt"])
    return g, heat64, paths


def _check_chunk(g, tag, d, mpjpe, heatmap_dir):
    """One chunk dict against the reference's, each quantity under the tolerance DESIGN.md section 6 holds it to."""
    names = sorted(os.listdir(heatmap_dir), key=__import__("globalegomocap_amd.whole_sequence", fromlist=["x"]).natural_key)
    a, b = (int(v) for v in g["range_" + tag])
    assert list(d) == [str(k) for k in g["keys_" + tag]]
    for k in d:
        assert isinstance(d[k], list) and len(d[k]) == b - a, k
        assert [_flag(x) for x in d[k]] == g[k + "_flags_" + tag].tolist(), k
    for f, x in enumerate(d["heatmap_list"]):          # exact: what loadmat returns for that file
        ref = sio.loadmat(os.path.join(heatmap_dir, names[a + f]))["heatmap"]
        assert x.dtype == ref.dtype and np.array_equal(x, ref) and _flag(x) == _flag(ref)
    figures = {}
    for k, tol in (("gt_global_skeleton", 0.0), ("estimated_local_skeleton", 1e-9), ("camera_pose_list", 1e-12), ("estimated_global_skeleton", 1e-9)):
        err = float(np.abs(np.asarray(d[k]) - g[k + "_" + tag]).max())
        figures[k] = err
        print("prepare %s %s: max abs difference %.3e (limit %.0e)" % (tag, k, err, tol))
    rel = abs(mpjpe - float(g["mpjpe_" + tag])) / float(g["mpjpe_" + tag])
    print("prepare %s initial mpjpe: %.15g against %.15g, relative %.3e (limit 1e-9)" % (tag, mpjpe, float(g["mpjpe_" + tag]), rel))
    assert figures["gt_global_skeleton"] == 0.0
    assert figures["estimated_local_skeleton"] <= 1e-9
    assert figures["camera_pose_list"] <= 1e-12
    assert figures["estimated_global_skeleton"] <= 1e-9
    assert rel <= 1e-9


def test_main_against_the_reference(P, golden, tmp_path, capsys):
    g, _, (hd, dd, traj, gtp) = _golden_recording(golden, tmp_path / "rec")
    for tag in ("a", "b"):
        a, b = (int(v) for v in g["range_" + tag])
        out_dir = str(tmp_path / ("out_" + tag))
        P.main(traj, hd, dd, gtp, a, b, out_dir, fps=int(g["fps"]), mat_start_frame=int(g["mat_start_frame"]))
        printed = capsys.readouterr().out
        assert "The initial mpjpe is: " in printed
        mpjpe = float(printed.split("The initial mpjpe is: ")[1].split()[0])
        with open(os.path.join(out_dir, "test_data.pkl"), "rb") as f:
            raw = f.read()
        d = pickle.loads(raw)                              # plain pickle.load, the same five keys in order
        assert list(d) == list(P.PICKLE_KEYS) and raw[1] == int(g["protocol_" + tag])
        with capsys.disabled():
            _check_chunk(g, tag, d, mpjpe, hd)


def test_chunk_loop_against_the_reference_and_round_trip(P, golden, tmp_path):
    import torch
    from globalegomocap_amd import whole_sequence as ws
    g, _, (hd, dd, traj, gtp) = _golden_recording(golden, tmp_path / "rec")
    t0, t1, size = (int(v) for v in g["loop"])
    rec = P.prepare_sequence(traj, hd, dd, gtp, t0, t1, fps=int(g["fps"]), mat_start_frame=int(g["mat_start_frame"]), test_size=size,
                             out_root=str(tmp_path / "chunks"), verbose=False)
    assert len(rec) == int(g["loop_chunks"]) == (t1 - t0) // size - 1          # the span is a multiple of test_size: the last chunk is dropped
    assert set(os.listdir(str(tmp_path / "chunks"))) == {"data_start_%d_end_%d" % (t0 + k * size, t0 + (k + 1) * size) for k in range(len(rec))}
    for k, c in enumerate(rec.chunks):
        assert c.heat.is_cuda and c.heat.dtype == torch.float32 and tuple(c.heat.shape) == (size, 64, 64, 15)
        for t, shape in ((c.est_local, (size, 15, 3)), (c.est_global, (size, 15, 3)), (c.cams, (size, 4, 4)), (c.gt, (size, 15, 3))):
            assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape
        _check_chunk(g, "loop%d" % k, rec.chunk_dict(k), c.initial_mpjpe, hd)
        # the project's own reader returns the same arrays from the written file (these chunks mix float32 and float64 heat-maps,
        # which its native path leaves to pickle.load by design; the native path itself is checked below)
        path = str(tmp_path / "chunks" / c.name)
        parsed = ws.parse_chunk(path, native=True)
        assert np.array_equal(parsed["est_local"], c.est_local.cpu().numpy()) and np.array_equal(parsed["cams"], c.cams.cpu().numpy())
        assert np.array_equal(parsed["gt"], c.gt.cpu().numpy())
        loaded = ws.load_chunk(path, torch.device("cuda", 0))
        loaded["heat_ready"].synchronize()
        assert torch.equal(loaded["heat"], c.heat)
    # round trip through the native path of the project's reader: recordings of ONE heat-map class (all float32, all float64)
    from globalegomocap_amd import synth_recording as S
    heat64 = S.paraboloid_heatmaps(g["centres"], g["radii"])
    for kind, as64 in (("f32", np.zeros(len(heat64), bool)), ("f64", np.ones(len(heat64), bool))):
        hd2, dd2, traj2, gtp2 = S.write_recording(str(tmp_path / ("rec_" + kind)), heat64, g["depth"], [str(x) for x in g["names"]], as64,
                                                  g["compressed"], g["rows"], g["gt"])
        rec2 = P.prepare_sequence(traj2, hd2, dd2, gtp2, t0, t1, fps=int(g["fps"]), mat_start_frame=int(g["mat_start_frame"]), test_size=size,
                                  out_root=str(tmp_path / ("chunks_" + kind)), verbose=False)
        for c in rec2.chunks:
            path = str(tmp_path / ("chunks_" + kind) / c.name)
            parsed = ws.parse_chunk(path, native=True)
            assert "heat_offsets" in parsed and "heat_list" not in parsed          # the native path, no fallback
            assert parsed["heat_fortran"] == 1 and parsed["heat_dtype"] == (1 if kind == "f64" else 0) and parsed["n"] == size
            assert np.array_equal(parsed["est_local"], c.est_local.cpu().numpy()) and np.array_equal(parsed["cams"], c.cams.cpu().numpy())
            assert np.array_equal(parsed["gt"], c.gt.cpu().numpy())
            loaded = ws.load_chunk(path, torch.device("cuda", 0))
            loaded["heat_ready"].synchronize()
            assert torch.equal(loaded["heat"], c.heat)
    # the documented difference: a trajectory without a frame of the range
    rows = [r for k, r in enumerate(g["rows"]) if k != 12]
    bad = str(tmp_path / "bad_traj.txt")
    with open(bad, "w") as f:
        f.write("\n".join(" ".join("%.9f" % v for v in r) for r in rows) + "\n")
    with pytest.raises(ValueError, match="12"):
        P.prepare_sequence(bad, hd, dd, gtp, t0, t1, fps=int(g["fps"]), mat_start_frame=int(g["mat_start_frame"]), test_size=size, verbose=False)


def test_files_outside_the_scanners_subset_go_through_loadmat(P, tmp_path):
    """A heat-map file the scanner refuses (an integer class) and a depth file stored as single: `frames_to_device` returns what
    loadmat + .float() give, and keeps the heat-map in the file's own type for the pickle."""
    import torch
    rng = np.random.default_rng(8)
    hs, ds = [], []
    for f in range(3):
        h = rng.integers(0, 200, (64, 64, 15)).astype(np.uint8) if f == 1 else rng.random((64, 64, 15)).astype(np.float32)
        d = rng.uniform(0.3, 2.0, (1, 15)).astype(np.float32 if f == 2 else np.float64)
        hs.append(str(tmp_path / ("h%d.mat" % f))); ds.append(str(tmp_path / ("d%d.mat" % f)))
        sio.savemat(hs[-1], {"heatmap": h}); sio.savemat(ds[-1], {"depth": d})
    heat, depth, kept = P.frames_to_device(hs, ds)
    for f in range(3):
        ref = sio.loadmat(hs[f])["heatmap"]
        assert torch.equal(heat[f].cpu(), torch.from_numpy(np.ascontiguousarray(ref)).float())
        assert np.array_equal(depth[f].cpu().numpy(), sio.loadmat(ds[f])["depth"][0].astype(np.float64))
        assert (kept[f] is None) == (f != 1)
    assert kept[1].dtype == np.uint8 and np.array_equal(kept[1], sio.loadmat(hs[1])["heatmap"])


def test_optimize_recording_is_bitwise_write_chunks_plus_optimize_directory(P, golden, tmp_path, capsys):
    """Three chunks of 26 frames (three windows each), fitted synthetic VAEs, the noise drawn from the same seed on both routes:
    the device-resident recording and the pickles written from it give bitwise equal poses and error reports."""
    import torch
    from globalegomocap_amd import synth_recording as S, whole_sequence as ws
    from helpers import sd_from_npz
    size, n_chunks = 26, 3
    n = size * n_chunks + 1
    par = S.random_parameters(n, seed=23)
    # depths and centres that make a plausible body in front of the camera are not needed: the optimiser runs on whatever it is given
    heat64 = S.paraboloid_heatmaps(par["centres"], par["radii"])
    names = ["f_%d.mat" % k for k in range(n)]
    hd, dd, traj, gtp = S.write_recording(str(tmp_path / "rec"), heat64, par["depth"], names, np.arange(n) % 7 == 3, np.arange(n) % 5 == 1,
                                          par["rows"], par["gt"])
    rec = P.prepare_sequence(traj, hd, dd, gtp, 0, n, fps=25, test_size=size, verbose=False)
    assert len(rec) == n_chunks
    lt = golden("lbfgs_tiny")
    kw = dict(global_vae_path=sd_from_npz(lt, "global/"), local_vae_path=sd_from_npz(lt, "local/"))
    torch.manual_seed(31)
    a = ws.optimize_recording(rec, DEFAULT_CALIBRATION, **kw)
    out_a = capsys.readouterr().out
    root = str(tmp_path / "chunks")
    rec.write_chunks(root)
    torch.manual_seed(31)
    b = ws.optimize_directory(root, DEFAULT_CALIBRATION, **kw)
    out_b = capsys.readouterr().out
    assert len(a[1]) == len(b[1]) == n_chunks
    for x, y in zip(a[2:], b[2:]):                          # estimated, optimised, ground-truth sequences
        assert x.shape == y.shape == (n_chunks * size, 15, 3) and np.array_equal(x, y)
    assert list(a[0]) == list(b[0])
    for k in a[0]:
        assert np.array_equal(np.asarray(a[0][k]), np.asarray(b[0][k])), k
    for ra, rb in zip(a[1], b[1]):
        for k in ra:
            assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k
    # the same printed summary (the `running data:` lines name the chunks, not directories)
    tail = lambda s: [l for l in s.splitlines() if not l.startswith("running data:")]      # noqa: E731
    assert tail(out_a) == tail(out_b) and out_a.count("running data:") == n_chunks
    assert np.isfinite(a[3]).all()
