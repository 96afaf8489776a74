"""The SLAM bridge without a GPU: `find_gaps` on hand-made id lists, the numpy twin (tests/bridge_twin.py) on a
motion it must bridge exactly and on the walker of the table in section 6o, the host-side refusals of gem_slam_bridge, the wiring of
`bridge=` and `--bridge`, and that nothing changes without the option."""
import ctypes
import functools
import inspect
import json
import os
import re

import numpy as np
import pytest

import bridge_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ids(n, lost=(), first=0):
    keep = np.ones(n, dtype=bool)
    for a, b in lost:
        keep[a - first:b - first] = False
    return np.arange(first, first + n)[keep]


# ------------------------------------------------------------------------------------------------------------------ find_gaps
def test_find_gaps_on_hand_made_id_lists():
    from globalegomocap_amd import slam_bridge as B
    assert B.find_gaps(_ids(20), 0, 20, 25) == []
    assert B.find_gaps(_ids(20, [(7, 10)]), 0, 20, 25) == [(7, 3)]
    assert B.find_gaps(_ids(30, [(105, 108), (109, 112)], first=100), 100, 130, 25) == [(105, 7)]          # one tracked frame between: ONE system
    assert B.find_gaps(_ids(30, [(105, 108), (110, 112)], first=100), 100, 130, 25) == [(105, 3), (110, 2)]          # two: two systems
    assert B.find_gaps(_ids(30, [(5, 6), (7, 8), (9, 10), (20, 21)]), 0, 30, 1) == [(5, 5), (20, 1)]
    # ids outside the span and in any order do not matter
    ids = np.concatenate([[300, 2], _ids(20, [(57, 60)], first=50)[::-1]])
    assert B.find_gaps(ids, 50, 70, 3) == [(57, 3)]
    assert B.gap_list(B.tracked_mask(_ids(12, [(0, 2), (5, 6), (10, 12)]), 0, 12)) == [(0, 2), (5, 1), (10, 2)]
    assert B.max_gap_frames(1.0, 25) == 25 and B.max_gap_frames(0.5, 25) == 13 and B.max_gap_frames(0.1, 24) == 2
    with pytest.raises(ValueError, match="positive"):
        B.max_gap_frames(0.0, 25)


def test_find_gaps_refusals_name_what_the_user_needs():
    from globalegomocap_amd import slam_bridge as B
    with pytest.raises(ValueError, match=r"first tracked id is 12, the last 29 .*--start 12 --end 30"):
        B.find_gaps(_ids(20, [(10, 12)], first=10), 10, 30, 25)
    with pytest.raises(ValueError, match=r"first tracked id is 10, the last 26 .*--start 10 --end 27"):
        B.find_gaps(_ids(20, [(27, 30)], first=10), 10, 30, 25)
    with pytest.raises(ValueError, match=r"at most 5 lost frames.*ids \[20, 26\): 6 frames, ids \[40, 50\): 10 frames"):
        B.find_gaps(_ids(60, [(10, 15), (20, 26), (40, 50)]), 0, 60, 5)
    B.find_gaps(_ids(60, [(10, 15)]), 0, 60, 5)
    with pytest.raises(ValueError, match=r"hard cap is 64.*ids \[10, 75\): 65 frames"):
        B.find_gaps(_ids(100, [(10, 75)]), 0, 100, 1000)
    B.find_gaps(_ids(100, [(10, 74)]), 0, 100, 1000)
    with pytest.raises(ValueError, match=r"several lines for frame ids \[4, 9\]"):
        B.find_gaps(np.concatenate([_ids(20), [9, 4]]), 0, 20, 25)
    with pytest.raises(ValueError, match=r"one system of more than 64 unknowns"):
        B.find_gaps(_ids(100, [(10, 50), (51, 80)]), 0, 100, 64)
    with pytest.raises(ValueError, match="no line for any frame id"):
        B.find_gaps(_ids(20), 40, 50, 25)
    assert T.systems_of(B.tracked_mask(_ids(30, [(5, 8), (9, 12), (20, 22)]), 0, 30)) == [(5, 7), (20, 2)]


# ------------------------------------------------------------------------------------------------------------------ the twin
def _steady(n, lost):
    """Constant velocity, constant angular velocity about one axis -> (poses [n,7], tracked, the true matrices)."""
    t = np.arange(n, dtype=np.float64)
    axis = np.array([0.36, -0.48, 0.8])
    half = 0.5 * 0.031 * t
    quat = np.concatenate([np.sin(half)[:, None] * axis, np.cos(half)[:, None]], axis=1)
    trans = np.array([0.3, -0.2, 0.1]) + t[:, None] * np.array([0.048, 0.002, -0.013])
    tracked = np.ones(n, dtype=bool)
    for a, b in lost:
        tracked[a:b] = False
    G = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        G[k, :3, :3] = T.quat_matrix(T.unit(quat[k]))
    G[:, :3, 3] = trans
    poses = np.concatenate([trans, quat], axis=1)
    poses[~tracked] = np.nan          # (rows of lost frames are ignored)
    return poses, tracked, G


@pytest.mark.parametrize("lost", [((5, 6),), ((10, 40),), ((3, 6), (7, 9), (10, 11), (30, 94)), ((1, 3), (96, 99))])
def test_a_steady_motion_is_bridged_exactly(lost):
    poses, tracked, G = _steady(100, lost)
    r = T.bridge(poses, tracked, (0, 37))
    assert np.abs(r["G"][:, :3, 3] - G[:, :3, 3]).max() <= 1e-12
    assert np.abs(r["G"][:, :3, :3] - G[:, :3, :3]).max() <= 1e-12
    assert r["lost"] == sum(b - a for a, b in lost) and r["gaps"] == len(lost) and r["longest_gap"] == max(b - a for a, b in lost)
    assert np.array_equal(r["bridged"], (~tracked).astype(np.uint8)) and r["offset_max"] <= 1e-12
    # chunks: origins[k] cams[f] is the frame in the span's frame
    for k, (a, b) in enumerate(((0, 37), (37, 100))):
        assert np.abs(np.einsum("ij,njk->nik", r["origins"][k], r["cams"][a:b]) - r["G"][a:b]).max() <= 1e-12
        assert np.abs(r["cams"][a] - np.eye(4)).max() <= 1e-15


def test_slerp_branches():
    q0 = T.unit(np.array([0.1, 0.2, -0.3, 0.9]))
    q, theta = T.slerp(q0, -q0, 0.3)          # the same rotation with the other sign: nothing to interpolate
    assert theta == 0.0 and np.abs(q - q0).max() <= 1e-16
    near = T.unit(q0 + np.array([3e-9, 0.0, 0.0, 0.0]))
    q, theta = T.slerp(q0, near, 0.5)
    assert theta < T.SMALL_ANGLE and abs(np.sqrt((q * q).sum()) - 1.0) <= 1e-15
    far = T.unit(np.array([0.5, -0.1, 0.4, 0.6]))
    q, theta = T.slerp(q0, far, 0.25)
    step, _ = T.slerp(q0, far, 0.5)
    again, _ = T.slerp(q0, step, 0.5)
    assert theta > 0.1 and np.abs(q - again).max() <= 1e-15


@functools.lru_cache(maxsize=None)
def _walker(lost):
    from globalegomocap_amd import slam_bridge as B
    w, rows = T.walker_rows(220, seed=3, lost=lost)
    poses, mask = B.relative_rows(rows, 0, 220, 25.0, 1.0)
    return w, poses, mask, T.bridge(poses, mask)


# the bounds are the figures of the numpy study that preceded the kernel (camera position error mean / max, rotation error
# mean / max over the lost frames) with margin for the twin's own slerp; the study's figures and the twin's:
#   [80,100)                 study 2.45 cm / 5.74 cm, 3.10 / 4.07 degrees;    twin 2.45 cm / 5.74 cm, 3.10 / 4.07 degrees
#   [60,68) and [130,160)    study 1.99 cm / 5.67 cm, 5.52 / 10.65 degrees;   twin 1.99 cm / 5.67 cm, 5.52 / 10.65 degrees
@pytest.mark.parametrize("lost", [((80, 100),), ((60, 68), (130, 160))])
def test_the_walker_of_the_table_is_within_its_bounds(lost, capsys):
    w, poses, mask, r = _walker(lost)
    truth = T.relative_truth(w)
    pos, rot = T.errors(r["G"], truth, np.flatnonzero(~mask))
    with capsys.disabled():
        print("walk(220, seed=3), lost %s: position error mean %.2f cm max %.2f cm, rotation error mean %.2f max %.2f degrees; record: offset %.3f m, "
              "angle %.2f degrees, distance %.3f m" % (list(lost), 100 * pos.mean(), 100 * pos.max(), rot.mean(), rot.max(), r["offset_max"],
                                                        np.degrees(r["angle_max"]), r["translation_max"]))
    assert pos.max() <= 0.08 and rot.max() <= 12.0
    tp, tr = T.errors(r["G"], truth, np.flatnonzero(mask))
    assert tp.max() <= 1e-12 and tr.max() <= 1e-5          # (arccos near 1)


def test_without_lost_frames_the_twin_gives_the_cameras_of_today():
    from globalegomocap_amd import prepare, slam_bridge as B
    w, rows = T.walker_rows(60, seed=3)
    spans = [(0, 25), (25, 50), (50, 60)]
    for scale in (1.0, 2.5):
        cams, origins = prepare.scaled_cameras(rows, spans, 25.0, scale)
        poses, mask = B.relative_rows(rows, 0, 60, 25.0, scale)
        r = T.bridge(poses, mask, [a for a, _ in spans])
        assert mask.all() and r["lost"] == 0 and r["systems"] == 0
        assert np.abs(r["cams"] - np.concatenate(cams)).max() <= 1e-12 and np.abs(r["origins"] - origins).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ wiring
def test_without_the_option_a_missing_id_is_still_refused(monkeypatch, tmp_path):
    from globalegomocap_amd import prepare
    w, rows = T.walker_rows(30, lost=((11, 13),))
    with pytest.raises(ValueError, match=r"no line for frame ids \[11, 12\]"):
        prepare.check_trajectory(rows, 0, 30, 25.0)
    spans_signature = inspect.signature(prepare.prepare_spans)
    assert spans_signature.parameters["bridge"].default is None
    from globalegomocap_amd import detections
    assert inspect.signature(detections.recording_from_detections).parameters["bridge"].default is None
    # the wrappers have no default of their own: what they are not given, `prepare_spans` is not given either
    got = []

    def spans(*args, **kwargs):
        got.append(kwargs)
        spans_signature.bind(*args, **kwargs)
        return prepare.Recording([])
    monkeypatch.setattr(prepare, "prepare_spans", spans)
    prepare.prepare_sequence("t", "h", "d", None, 0, 30, scale=1.0)
    with pytest.raises(IndexError):          # (`main` writes chunk 0 of what it is given back)
        prepare.main("t", "h", "d", None, 0, 30, str(tmp_path), 25, scale=1.0)
    assert got == [{"scale": 1.0}] * 2


def test_the_option_is_refused_with_ground_truth_and_parsed_on_both_command_lines(tmp_path):
    from globalegomocap_amd import detections, prepare, slam_bridge as B
    assert B.bridge_arg(None) is None and B.bridge_arg(True) == 1.0 and B.bridge_arg(0.4) == 0.4 and B.bridge_arg(None, "gt.pkl") is None
    with pytest.raises(ValueError, match="no common world"):
        B.bridge_arg(1.0, "gt.pkl")
    with pytest.raises(ValueError, match="positive"):
        B.bridge_arg(-1.0)
    with pytest.raises(ValueError, match="no common world"):          # (before any file is opened)
        prepare.prepare_sequence("none.txt", "h", "d", "gt.pkl", 0, 60, bridge=1.0)
    with pytest.raises(ValueError, match="no common world"):
        detections.recording_from_detections("none.txt", np.zeros((4, 15, 2)), "gt.pkl", None, [(0, 4)], bridge=0.5)
    common = ["--slam", "t", "--start", "0", "--end", "9", "--scale", "1"]
    for parser, extra in ((prepare._parser(), ["--heatmaps", "h", "--depths", "d"]), (detections._parser(), ["--keypoints", "k"])):
        assert parser.parse_args(common + extra).bridge is None
        assert parser.parse_args(common + extra + ["--bridge"]).bridge == 1.0
        assert parser.parse_args(common + extra + ["--bridge", "0.4"]).bridge == 0.4
    with pytest.raises(ValueError, match="without a hole"):
        B.contiguous_span([(0, 10), (12, 20)])
    assert B.contiguous_span([(5, 10), (10, 20)]) == (5, 20)


def test_the_gap_lister_needs_no_device(tmp_path, capsys):
    from globalegomocap_amd import slam_bridge as B
    w, rows = T.walker_rows(80, lost=((20, 23), (24, 30), (50, 70)))
    traj = tmp_path / "traj.txt"
    traj.write_text("\n".join(" ".join(repr(float(v)) for v in r) for r in rows) + "\n")
    out = B._cli(["--slam", str(traj), "--start", "0", "--end", "80", "--fps", "25", "--max_gap", "0.5", "--json", str(tmp_path / "o" / "gaps.json")])
    text = capsys.readouterr().out
    assert out["lost"] == 29 and out["gaps"] == [[20, 3], [24, 6], [50, 20]] and out["accepted"] is False and "ids [50, 70): 20 frames" in out["refusal"]
    assert "29 of 80 frame ids have no line, in 3 gaps" in text and "needs --bridge 0.80" in text and "refuses" in text
    assert json.load(open(str(tmp_path / "o" / "gaps.json"))) == out
    out = B._cli(["--slam", str(traj), "--start", "0", "--end", "80", "--max_gap", "1"])
    assert out["accepted"] is True and out["systems"] == [[20, 10], [50, 20]]


def test_record_layout_and_declarations():
    from globalegomocap_amd import _capi
    assert ctypes.sizeof(_capi.GemBridgeRecord) == 8 * _capi.BRIDGE_RECORD_DOUBLES == 128
    names = [f[0] for f in _capi.GemBridgeRecord._fields_]
    assert tuple(names[:9]) == T.RECORD and names[9] == "reserved"
    header = open(os.path.join(ROOT, "include", "gem_hip.h")).read()
    for name, value in (("GEM_BRIDGE_MAX_GAP", _capi.BRIDGE_MAX_GAP), ("GEM_BRIDGE_MAX_SPAN", _capi.BRIDGE_MAX_SPAN),
                        ("GEM_BRIDGE_RECORD_DOUBLES", _capi.BRIDGE_RECORD_DOUBLES), ("GEM_BRIDGE_NOT_SOLVED", _capi.BRIDGE_NOT_SOLVED)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert T.MAX_GAP == _capi.BRIDGE_MAX_GAP == 64
    struct = re.search(r"typedef struct gem_bridge_record \{(.*?)\} gem_bridge_record;", header, re.S).group(1)
    declared = re.findall(r"\b([a-z_]+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    assert declared == names
    for name, n_args in (("gem_slam_bridge_work", 1), ("gem_slam_bridge", 18)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == n_args == len(_capi.SIGNATURES[name][1]), name


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import _capi
    return _capi.load_library()


def test_every_refusal_of_the_host_entry_point(lib):
    P = ctypes.c_void_p
    assert lib.gem_slam_bridge_work(40) == 8 * (20 * 8 + 8) and lib.gem_slam_bridge_work(1) == 8 * 16
    for n in (0, (1 << 20) + 1):
        assert lib.gem_slam_bridge_work(n) == -1 and b"gem_slam_bridge_work: n" in lib.gem_last_error()
    fake = 1 << 20          # device addresses are never read by the host checks: no launch happens behind a refusal
    n = 40
    mask = np.ones(n, dtype=np.uint8)
    mask[5:8] = 0
    mask[9:12] = 0
    mask[20:22] = 0
    good_systems = np.array([[5, 7], [20, 2]], dtype=np.int32)
    good_starts = np.array([0, 15], dtype=np.int32)
    names = ("d_poses", "h_tracked", "d_tracked", "h_systems", "d_systems", "n_systems", "h_chunk_starts", "d_chunk_starts", "n_chunks", "n", "d_G",
             "d_cams", "d_origins", "d_bridged", "d_work", "work_bytes", "d_record")

    def call(mask=mask, systems=good_systems, starts=good_starts, **k):
        systems, starts = np.ascontiguousarray(systems, dtype=np.int32), np.ascontiguousarray(starts, dtype=np.int32)
        a = dict(d_poses=fake, h_tracked=mask.ctypes.data, d_tracked=fake * 2, h_systems=systems.ctypes.data, d_systems=fake * 3, n_systems=len(systems),
                 h_chunk_starts=starts.ctypes.data, d_chunk_starts=fake * 4, n_chunks=len(starts), n=len(mask), d_G=fake * 5, d_cams=fake * 6,
                 d_origins=fake * 7, d_bridged=fake * 8, d_work=fake * 9, work_bytes=lib.gem_slam_bridge_work(len(mask)), d_record=fake * 10)
        a.update(k)
        args = [a[x] if x in ("n_systems", "n_chunks", "n", "work_bytes") else P(a[x]) for x in names]
        rc = lib.gem_slam_bridge(*(args + [None]))
        return rc, lib.gem_last_error().decode()

    refusals = [(dict(n=0), "n must lie"), (dict(n=(1 << 20) + 1), "n must lie"), (dict(n_systems=-1), "n_systems"), (dict(n_systems=21), "n_systems"),
                (dict(n_chunks=0), "n_chunks"), (dict(n_chunks=41), "n_chunks"), (dict(h_systems=None), "h_systems is null"),
                (dict(d_systems=None), "d_systems is null"), (dict(d_G=fake + 4), "d_G must be 8-byte aligned"),
                (dict(d_poses=fake + 1), "d_poses must be 8-byte aligned"), (dict(d_record=fake + 2), "d_record must be 8-byte aligned"),
                (dict(d_systems=fake + 2), "d_systems must be 4-byte aligned"), (dict(d_chunk_starts=fake + 1), "d_chunk_starts must be 4-byte aligned"),
                (dict(work_bytes=8), "d_work holds 8 bytes")]
    refusals += [({k: None}, k + " is null") for k in names if k[:2] in ("d_", "h_") and k not in ("h_systems", "d_systems")]
    for k, word in refusals:
        rc, msg = call(**k)
        assert rc == 1 and msg.startswith("gem_slam_bridge: ") and word in msg, (k, msg)
    for lost_end in (0, n - 1):
        m = mask.copy()
        m[lost_end] = 0
        rc, msg = call(mask=m)
        assert rc == 1 and "h_tracked: the first and the last frame must be tracked" in msg
    for starts, word in (([1, 15], "begin with 0"), ([0, 15, 15], "chunk 2"), ([0, 40], "chunk 1")):
        rc, msg = call(starts=starts)
        assert rc == 1 and "h_chunk_starts" in msg and word in msg, msg
    for systems, word in (([[5, 3], [9, 3], [20, 2]], "system 1 must lie at least two tracked frames behind"), ([[5, 7]], "2 lost frames of h_tracked lie in no system"),
                          ([[5, 7], [20, 3]], "system 1 must begin and end with a lost frame"), ([[4, 8], [20, 2]], "system 0 must begin and end"),
                          ([[5, 7], [20, 0]], "system 1 does not lie inside"), ([[5, 7], [38, 2]], "system 1 does not lie inside"),
                          ([[0, 7], [20, 2]], "system 0 does not lie inside")):
        rc, msg = call(systems=systems)
        assert rc == 1 and "h_systems" in msg and word in msg, (systems, msg)
    m = np.ones(30, dtype=np.uint8)
    m[5:8] = 0
    m[10:12] = 0
    rc, msg = call(mask=m, systems=[[5, 7]], starts=[0])
    assert rc == 1 and "system 0 holds two tracked frames in a row" in msg
    long = np.ones(200, dtype=np.uint8)
    long[10:75] = 0
    rc, msg = call(mask=long, systems=[[10, 65]], starts=[0])
    assert rc == 1 and "system 0 is longer than 64 lost frames" in msg
    comb = np.ones(300, dtype=np.uint8)
    comb[10:140:2] = 0          # 65 lost frames with single tracked frames between them: 129 frames
    rc, msg = call(mask=comb, systems=[[10, 129]], starts=[0])
    assert rc == 1 and "system 0 is longer than 127 frames" in msg
