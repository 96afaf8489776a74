"""The SLAM bridge on the device: gem_slam_bridge against the numpy twin (tests/bridge_twin.py) on walker
trajectories with lines removed, with canaries around every output; all cases enqueued as one batch (no synchronisation between the
calls) and again alone, with the same bytes; a recording without lost frames gives the cameras it gives without the option; and
`prepare(..., bridge=)` end to end through the optimiser, which without the option refuses the recording.

Tolerance 1e-9 (metres, and per rotation entry): the pentadiagonal system's condition number grows like m^4, about 1.7e7 at 64
unknowns, so two orders of solving it may differ by that much times 1e-16 of the solved quantity -- which is the OFFSET from a straight
line, centimetres, not the position.  The mask and the record's integer fields agree exactly."""
import functools

import numpy as np
import pytest

import bridge_twin as T
from pipeline_checks import SIZE, write_recording as _write_recording
from globalegomocap_amd.camera import DEFAULT_CALIBRATION

pytestmark = pytest.mark.gpu

TOL = 1e-9
CANARY = -7.25
CANARY_BYTE = 0xA5
PAD = 16


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import prepare
    return prepare._lift_engine(DEFAULT_CALIBRATION, 0)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(poses, mask, systems as frame indices, chunk starts, the twin's result): computed once, never changed."""
    from globalegomocap_amd import slam_bridge as B
    n, lost, starts = T.CASES[name]
    w, rows = T.walker_rows(n, seed=3, lost=lost)
    poses, mask = B.relative_rows(rows, 0, n, 25.0, 1.0)
    systems = B.find_gaps(w["frame_ids"][mask], 0, n, 64)
    assert systems == T.systems_of(mask)
    for x in (poses, mask):
        x.setflags(write=False)
    return poses, mask, systems, starts, T.bridge(poses, mask, starts)


def _blocks(env, n, nc):
    """Canaried blocks and the views the call writes into."""
    import torch
    f64 = lambda *s: torch.full(s, CANARY, dtype=torch.float64, device=env.device)          # noqa: E731
    blocks = [f64(n + 2, 4, 4), f64(n + 2, 4, 4), f64(nc + 2, 4, 4), torch.full((n + 2 * PAD,), CANARY_BYTE, dtype=torch.uint8, device=env.device),
              f64(16 + 2 * PAD)]
    views = (blocks[0][1:-1], blocks[1][1:-1], blocks[2][1:-1], blocks[3][PAD:-PAD], blocks[4][PAD:-PAD])
    return blocks, views


def _enqueue(env, name):
    from globalegomocap_amd import slam_bridge as B
    poses, mask, systems, starts, _ = _case(name)
    blocks, views = _blocks(env, len(mask), len(starts))
    B.bridge_call(env.device, poses, mask, systems, starts, outputs=views)
    return blocks


def _read(blocks):
    """-> (G, cams, origins, bridged, record) on the host, the canaries checked."""
    host = [b.cpu().numpy() for b in blocks]
    for h in host[:3]:
        assert (h[0] == CANARY).all() and (h[-1] == CANARY).all()
    assert (host[3][:PAD] == CANARY_BYTE).all() and (host[3][-PAD:] == CANARY_BYTE).all()
    assert (host[4][:PAD] == CANARY).all() and (host[4][-PAD:] == CANARY).all()
    return host[0][1:-1], host[1][1:-1], host[2][1:-1], host[3][PAD:-PAD], host[4][PAD:-PAD]


def _compare(name, got, capsys):
    from globalegomocap_amd import _capi
    G, cams, origins, bridged, record = got
    e = _case(name)[4]
    r = _capi.GemBridgeRecord.from_buffer_copy(np.ascontiguousarray(record).tobytes())
    assert np.array_equal(bridged, e["bridged"]), name
    for k in T.COUNTS:
        assert getattr(r, k) == e[k], (name, k, getattr(r, k), e[k])
    assert (record[9:] == 0.0).all()
    worst = {"G": np.abs(G - e["G"]).max(), "cams": np.abs(cams - e["cams"]).max(), "origins": np.abs(origins - e["origins"]).max()}
    worst.update({k: abs(getattr(r, k) - e[k]) for k in T.FLOATS})
    with capsys.disabled():
        print("%s: %d lost in %d gaps, %d systems; largest differences from the twin: %s"
              % (name, e["lost"], e["gaps"], e["systems"], ", ".join("%s %.1e" % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v <= TOL, (name, k, v)
    assert np.isfinite(G).all() and np.isfinite(cams).all()


@pytest.mark.parametrize("name", list(T.CASES))
def test_device_against_the_twin(env, name, capsys):
    poses, mask, systems, starts, e = _case(name)
    _compare(name, _read(_enqueue(env, name)), capsys)
    if name.startswith("40 frames"):
        assert systems == [(5, 7)] and e["lost"] == 6 and e["gaps"] == 2 and e["systems"] == 1
    if name.startswith("200 frames"):
        assert e["longest_gap"] == 64 and systems == [(70, 64)]
    if name.startswith("130 frames"):
        assert not mask[65] and starts == (0, 65)          # the second chunk's first camera is itself invented


def test_one_batch_and_alone_give_the_same_bytes(env, capsys):
    import torch
    names = list(T.CASES)
    batch = [_enqueue(env, n) for n in names]          # (six calls behind one another on the stream, nothing read in between)
    torch.cuda.synchronize()
    together = [_read(b) for b in batch]
    for name, got in zip(names, together):
        _compare(name, got, capsys)
        alone = _read(_enqueue(env, name))
        for a, b in zip(alone, got):
            assert a.tobytes() == b.tobytes(), name


def test_refusals_reach_python(env):
    from globalegomocap_amd import _capi, slam_bridge as B
    poses, mask, systems, starts, _ = _case("40 frames, two gaps around one tracked frame")
    with pytest.raises(_capi.GemError, match="h_systems: 6 lost frames"):
        B.bridge_call(env.device, poses, mask, [], starts)
    with pytest.raises(_capi.GemError, match="h_chunk_starts must begin with 0"):
        B.bridge_call(env.device, poses, mask, systems, (3,))
    with pytest.raises(ValueError, match="outputs"):
        B.bridge_call(env.device, poses, mask, systems, starts, outputs=_blocks(env, 39, 1)[1])


def _without_lines(traj, lost, out):
    """The trajectory file `traj` without the lines of the frame ids [a, b) of `lost` (25 fps) -> the new file's path."""
    from globalegomocap_amd import slam
    with open(traj) as f:
        lines = [l for l in f.read().splitlines() if l.strip()]
    ids = slam.frame_ids(lines, 25)
    assert len(ids) == len(lines)
    keep = [l for l, i in zip(lines, ids) if not any(a <= i < b for a, b in lost)]
    with open(out, "w") as f:
        f.write("\n".join(keep) + "\n")
    return str(out)


def test_without_lost_frames_the_option_changes_nothing(env, tmp_path):
    from globalegomocap_amd import prepare as P
    n = 2 * SIZE + 1
    hd, dd, traj, gtp = _write_recording(tmp_path / "rec", n, seed=23)
    kw = dict(fps=25, test_size=SIZE, verbose=False, scale=1.7)
    plain = P.prepare_sequence(traj, hd, dd, None, 0, n, **kw)
    bridged = P.prepare_sequence(traj, hd, dd, None, 0, n, bridge=1.0, **kw)
    assert plain.bridge_report is None and plain.bridged is None and len(plain) == len(bridged) == 2
    r = bridged.bridge_report
    assert (r.lost, r.gaps, r.systems, r.frames, r.status) == (0, 0, 0, 2 * SIZE, 0) and not np.concatenate(bridged.bridged).any()
    for a, b in zip(plain.cams, bridged.cams):
        assert np.abs(a.cpu().numpy() - b.cpu().numpy()).max() <= 1e-12
    assert np.abs(plain.origins - bridged.origins).max() <= 1e-12
    for a, b in zip(plain.est_global, bridged.est_global):
        assert np.abs(a.cpu().numpy() - b.cpu().numpy()).max() <= 1e-11


def test_bridge_end_to_end(env, golden, tmp_path, capsys):
    """Two chunks of 26 frames whose trajectory lacks five lines inside the first chunk: refused without the option (today's
    ValueError), prepared and optimised with it; `Recording.bridged` marks exactly the five frames; the bridged cameras are the
    twin's."""
    import torch
    from globalegomocap_amd import prepare as P, slam, slam_bridge as B, whole_sequence as ws
    from helpers import sd_from_npz
    n = 2 * SIZE + 1
    hd, dd, traj, gtp = _write_recording(tmp_path / "rec", n, seed=23)
    holed = _without_lines(traj, [(10, 15)], tmp_path / "holed.txt")
    kw = dict(fps=25, test_size=SIZE, verbose=False, scale=1.0)
    with pytest.raises(ValueError, match=r"no line for frame ids \[10, 11, 12, 13, 14\]"):
        P.prepare_sequence(holed, hd, dd, None, 0, n, **kw)
    with pytest.raises(ValueError, match=r"no line for frame ids \[10, 11, 12, 13, 14\]"):
        P.prepare_sequence(holed, hd, dd, None, 0, n, bridge=None, **kw)
    with pytest.raises(ValueError, match=r"at most 3 lost frames.*ids \[10, 15\): 5 frames"):
        P.prepare_sequence(holed, hd, dd, None, 0, n, bridge=0.1, **kw)
    with pytest.raises(ValueError, match="no common world"):
        P.prepare_sequence(holed, hd, dd, gtp, 0, n, fps=25, test_size=SIZE, verbose=False, bridge=1.0)
    rec = P.prepare_sequence(holed, hd, dd, None, 0, n, bridge=1.0, **kw)
    want = np.zeros(2 * SIZE, dtype=bool)
    want[10:15] = True
    assert len(rec) == 2 and [len(b) for b in rec.bridged] == [SIZE, SIZE] and np.array_equal(np.concatenate(rec.bridged), want)
    r = rec.bridge_report
    assert (r.lost, r.gaps, r.systems, r.longest_gap, r.frames, r.gap_ids) == (5, 1, 1, 5, 2 * SIZE, [(10, 5)])
    with capsys.disabled():
        print(r.line())
    with open(holed) as f:
        rows = slam.trajectory_rows(f.read())
    poses, mask = B.relative_rows(rows, 0, 2 * SIZE, 25, 1.0)
    e = T.bridge(poses, mask, (0, SIZE))
    cams = np.concatenate([c.cpu().numpy() for c in rec.cams])
    assert np.abs(cams - e["cams"]).max() <= TOL and np.abs(rec.origins - e["origins"]).max() <= TOL
    # the tracked frames' cameras are those of the whole trajectory
    whole = P.prepare_sequence(traj, hd, dd, None, 0, n, **kw)
    full = np.concatenate([c.cpu().numpy() for c in whole.cams])
    assert np.abs(cams[~want] - full[~want]).max() <= 1e-12 and np.abs(cams[want] - full[want]).max() > 1e-6
    lt = golden("lbfgs_tiny")
    torch.manual_seed(31)
    out = ws.optimize_recording(rec, DEFAULT_CALIBRATION, ground_truth=False, global_vae_path=sd_from_npz(lt, "global/"),
                                local_vae_path=sd_from_npz(lt, "local/"), verbose=False)
    for i in (2, 3):
        assert out[i].shape == (2 * SIZE, 15, 3) and np.isfinite(out[i]).all()
    # the pickles hold bridged cameras as ordinary cameras
    dirs = rec.write_chunks(str(tmp_path / "chunks"))
    import pickle
    with open(dirs[0] + "/test_data.pkl", "rb") as f:
        d = pickle.load(f)
    assert list(d) == list(P.PICKLE_KEYS[1:]) and len(d["camera_pose_list"]) == SIZE
    assert np.abs(np.array(d["camera_pose_list"]) - e["cams"][:SIZE]).max() <= TOL
    ws.release_pools()


def test_auto_scale_pairs_only_tracked_frames(env, tmp_path, capsys):
    """The detection route with scale="auto" and a gap: the estimator is given the tracked rows only and pairs rows whose frame ids lie
    `lag` apart, so no pair reaches across the gap; the noise-free walker still fixes its scale to the bound the estimator's own
    detection-route test holds it to (tests/test_slam_scale_gpu.py), and the recording is bit for bit the one the number gives."""
    import torch
    from test_slam_scale_cpu import LAG, NOISY_BOUND
    from globalegomocap_amd import detections, synth_walk as W
    from globalegomocap_amd.camera import FisheyeCamera
    n, fps, scale, lost = 120, 25, 1.7, (40, 52)
    w = W.walk(n, scale=scale)
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    kp = np.concatenate([cam.project_numpy(w["local"].reshape(-1, 3)).reshape(n, 15, 2), np.ones((n, 15, 1))], axis=2)
    keep = np.ones(n, dtype=bool)
    keep[lost[0]:lost[1]] = False
    traj = str(tmp_path / "traj.txt")
    with open(traj, "w") as f:
        f.write("\n".join(" ".join(repr(float(v)) for v in r) for r in w["rows"][keep]) + "\n")
    det = {"keypoints": kp, "depth": w["depth"]}
    spans = [(0, 60), (60, 120)]
    with pytest.raises(ValueError, match="no line for frame ids"):
        detections.recording_from_detections(traj, det, None, "auto", spans, fps, min_pairs=30)
    rec = detections.recording_from_detections(traj, det, None, "auto", spans, fps, min_pairs=30, bridge=True)
    ids = np.flatnonzero(keep)
    est = rec.scale_report
    assert est.pairs == int((ids[LAG:] - ids[:-LAG] == LAG).sum()) == n - (lost[1] - lost[0]) - 2 * LAG
    assert rec.scale == est.scale and rec.bridge_report.lost == 12 and np.array_equal(np.concatenate(rec.bridged), ~keep)
    with capsys.disabled():
        print("scale %r (true %r, relative error %.3g); %s" % (rec.scale, scale, abs(rec.scale / scale - 1), rec.bridge_report.line()))
    assert abs(rec.scale / scale - 1) <= NOISY_BOUND
    same = detections.recording_from_detections(traj, det, None, rec.scale, spans, fps, bridge=1.0)
    assert same.scale is None and same.scale_report is None
    for a, b in zip(same.chunks, rec.chunks):
        assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("heat", "est_local", "est_global", "cams"))
    # the bridged cameras against the walker's true ones, at the estimated scale: the bounds tests/test_slam_bridge_cpu.py holds the twin to on longer gaps
    cams = np.concatenate([np.einsum("ij,njk->nik", o, c.cpu().numpy()) for o, c in zip(rec.origins, rec.cams)])
    pos, rot = T.errors(cams, T.relative_truth(w), np.flatnonzero(~keep))
    assert pos.max() <= 0.08 and rot.max() <= 12.0


def test_bridge_and_auto_scale_on_the_mat_route(env, tmp_path, capsys):
    """`prepare` with scale="auto" and `bridge=` together: three 26-frame chunks of the pose network's files that carry a walker (the
    recording of tests/test_slam_scale_gpu.py's prepare test), the trajectory without the lines of frame ids 30 .. 34, inside the second
    chunk.  The estimate is made on the tracked frames alone and is the twin's on the lifted poses (whose discrete decisions must be
    MARGIN from flipping: with this hole the smallest margin, the cost gap, is 1.1e-2), no pair reaches across the gap, exactly the five
    frames are marked, and the recording is bit for bit the one the number gives."""
    import torch
    import slam_scale_twin as ST
    from test_slam_scale_cpu import LAG
    from test_slam_scale_gpu import MARGIN, RTOL
    from globalegomocap_amd import prepare as P, slam, slam_scale as S, synth, synth_recording as R, synth_walk as W
    from globalegomocap_amd.camera import FisheyeCamera
    n, fps, size, min_pairs, lost = 78, 25, 26, 10, (30, 35)
    w = W.walk(n, scale=0.6)
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    ix, iy = synth.heatmap_coords(cam.project_numpy(w["local"].reshape(-1, 3)).reshape(n, 15, 2))
    centres = np.floor(np.stack([ix, iy], -1)) + np.array([0.3, 0.2])          # (no ties: the peak pixel is unique)
    heat64 = R.paraboloid_heatmaps(centres, np.full((n, 15), 5.0))
    hd, dd, traj, _ = R.write_recording(str(tmp_path / "rec"), heat64, w["depth"], ["f_%d.mat" % k for k in range(n)], None, None, w["rows"], None)
    holed = _without_lines(traj, [lost], tmp_path / "holed.txt")
    kw = dict(fps=fps, test_size=size, verbose=False)
    with pytest.raises(ValueError, match=r"no line for frame ids \[30, 31, 32, 33, 34\]"):
        P.prepare_sequence(holed, hd, dd, None, 0, n + 1, scale="auto", min_pairs=min_pairs, **kw)
    rec = P.prepare_sequence(holed, hd, dd, None, 0, n + 1, scale="auto", min_pairs=min_pairs, bridge=True, **kw)
    spans = P.chunk_spans(0, n + 1, size)
    keep = np.ones(n, dtype=bool)
    keep[lost[0]:lost[1]] = False
    assert len(rec) == 3 and spans == [(0, 26), (26, 52), (52, 78)]
    assert [len(b) for b in rec.bridged] == [size] * 3 and np.array_equal(np.concatenate(rec.bridged), ~keep)
    assert (rec.bridge_report.lost, rec.bridge_report.gaps, rec.bridge_report.gap_ids) == (5, 1, [(30, 5)])
    # the twin on the tracked frames' lifted poses, with the poses of the whole trajectory
    with open(traj) as f:
        Rm, c, ids = S.selected_poses(slam.trajectory_rows(f.read()), spans, fps)
    x = np.concatenate([ch.est_local.cpu().numpy() for ch in rec.chunks])
    cuts = np.concatenate([[0], np.cumsum([int(keep[a:b].sum()) for a, b in spans])])
    want = ST.estimate(x[keep], Rm[keep], c[keep], ids[keep], S.default_lag(fps), min_pairs=min_pairs, chunk_starts=cuts)
    m = want["margins"]
    assert m["cost_gap"] > MARGIN and m["tau"] > MARGIN and m["sides"] > MARGIN and m["informative"] > MARGIN, m
    est, tracked = rec.scale_report, np.flatnonzero(keep)
    with capsys.disabled():
        print("\nbridge + auto: %s; twin %r (relative difference %.3g), margins %s" % (est.line(), want["scale"], abs(est.scale / want["scale"] - 1), m))
    assert est.pairs == int((tracked[LAG:] - tracked[:-LAG] == LAG).sum()) == n - (lost[1] - lost[0]) - 2 * LAG
    assert (est.pairs, est.inliers, est.informative) == (want["pairs"], want["inliers"], want["informative"])
    assert rec.scale == est.scale and abs(est.scale / want["scale"] - 1) <= RTOL
    same = P.prepare_sequence(holed, hd, dd, None, 0, n + 1, scale=rec.scale, bridge=1.0, **kw)
    assert same.scale is None and same.scale_report is None and np.array_equal(same.origins, rec.origins)
    for a, b in zip(same.chunks, rec.chunks):
        for k in ("heat", "est_local", "est_global", "cams"):
            p, q = getattr(a, k), getattr(b, k)
            assert p.dtype == q.dtype and torch.equal(p, q), k
