"""Host side of the motion-window data path (globalegomocap_amd/motion_data.py) against the reference's own dataset code, recorded
in tests/golden/motion_windows.npz by tools/make_golden_motion.py: window counts, the float64 host twin, file selection, the
restricted pickle reader, the errors, the CLI's flags.  No GPU."""
import os
import pickle

import numpy as np
import pytest

from globalegomocap_amd import motion_data as M
from motion_fixture import cases, sequences, ulps, write_pickles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_GLOBAL_SH = ["--log_dir", "cnn_global_full_dataset_latent_2048_len_10_kl_0.5", "--train_data_path", "/data/EgocentricAMASS",
                   "--latent_dim", "2048", "--kl_weight", "0.5", "--seq_length", "10", "--batch_size", "64", "--new_dataset", "False",
                   "--with_mo2cap2_data", "False", "--fps", "25", "--network", "cnn"]


def _host_dataset(g, poses, fn, ws, fps, slide, path):
    seqs = [M.sequence_arrays(M.read_motion_pickle(os.path.join(str(path), name)), poses == "global", name) for name, _ in sequences(g)]
    return M.MotionWindows(seqs, poses, fn, ws, fps, slide, device="cpu")


def test_host_twin_matches_the_reference_windows(golden, tmp_path):
    g = golden("motion_windows")
    write_pickles(g, tmp_path)
    seen = set()
    for c, poses, fn, ws, fps, slide in cases(g):
        seen.add((poses, ws, fps, slide))
        ds = _host_dataset(g, poses, fn, ws, fps, slide, tmp_path)
        counts = g["case%d/counts" % c]
        assert ds.counts.tolist() == counts.tolist() and len(ds) == counts.sum(), (c, ds.counts, counts)
        ref = g["case%d/windows" % c]
        got = ds.windows_numpy(g["case%d/ids" % c])
        assert got.dtype == np.float32 and got.shape == ref.shape
        if poses == "local":
            assert np.array_equal(got, ref), c                                  # a copy and one float32 rounding
        else:
            assert ulps(got, ref).max() <= 1.0, (c, ulps(got, ref).max())        # the parity contract: 1 float32 ulp
    assert {p for p, *_ in seen} == {"global", "local"} and {s for *_, s in seen} == {True, False}
    # the edges the fixture was built to hold: a sequence of exactly total * timer frames has no window, one frame more has one
    ds = _host_dataset(g, "global", 10, 2, 25, True, tmp_path)
    assert ds.counts[-2:].tolist() == [0, 1]


def test_from_directory_reads_the_reference_files_in_listing_order(golden, tmp_path):
    g = golden("motion_windows")
    write_pickles(g, tmp_path, protocol=2)                     # (protocol 2 writes array data through _codecs.encode)
    order = {name: k for k, (name, _) in enumerate(sequences(g))}
    for c, poses, fn, ws, fps, slide in cases(g):
        ds = M.MotionWindows.from_directory(str(tmp_path), poses, fn, ws, fps, slide, split="all", device="cpu")
        assert ds.names == os.listdir(str(tmp_path))
        assert ds.counts.tolist() == [int(g["case%d/counts" % c][order[n]]) for n in ds.names]


def test_timer_rounds_halves_to_even_and_zero_is_refused():
    assert M.frame_rate_timer(75.0, 30) == 2 and M.frame_rate_timer(59.94, 25) == 2 and M.frame_rate_timer(120, 25) == 5
    assert M.frame_rate_timer(45, 30) == 2                  # 1.5 -> 2
    with pytest.raises(ValueError, match="frame step of 0"):
        M.frame_rate_timer(10, 25)
    pose = np.zeros((40, 15, 3))
    with pytest.raises(ValueError, match="frame step of 0"):
        M.MotionWindows([(pose, None, None, 12.0)], "local", 10, device="cpu")


def test_file_selection_matches_the_reference(golden):
    g = golden("motion_windows")
    listing = g["select/listing"].tolist()
    names = g["select/seq_names"].tolist()
    for split in ("train", "test"):
        for tag, sn in (("all", None), ("seqnames", names)):
            key = "select/%s_%s" % (split, tag)
            assert M.select_files(listing, split, sn) == g[key].tolist(), key
            bal = M.select_files(listing, split, sn, balance=True, rng=np.random.default_rng(3))
            assert len(bal) == int(g[key + "_balanced_count"]), key
            # balanced: every non-walking file, then walking ones drawn by the generator (seeded: reproducible)
            others = [p for p in g[key].tolist() if "walk" not in p.lower()]
            assert bal[:len(others)] == others and all("walk" in p.lower() for p in bal[len(others):])
            assert bal == M.select_files(listing, split, sn, balance=True, rng=np.random.default_rng(3))
    sel = M.select_files(listing, "all", names)
    assert len(sel) > len(set(sel))                          # a file matching two names is taken twice, like the reference


def test_malformed_sequences_are_refused():
    rng = np.random.default_rng(0)
    poses = [rng.normal(size=(15, 3)) for _ in range(30)]
    cams = [{"loc": rng.normal(size=3), "rot": rng.normal(size=4)} for _ in range(30)]
    M.sequence_arrays({"local_pose_list": poses, "cam_list": cams, "frame_rate": 25}, True)
    with pytest.raises(ValueError, match="29 cameras for 30 poses"):
        M.sequence_arrays({"local_pose_list": poses, "cam_list": cams[:-1], "frame_rate": 25}, True)
    with pytest.raises(ValueError, match=r"local_pose_list\[3\] has shape \(16, 3\)"):
        M.sequence_arrays({"local_pose_list": poses[:3] + [np.zeros((16, 3))] + poses[4:], "cam_list": cams, "frame_rate": 25}, True)
    with pytest.raises(ValueError, match="zero norm"):
        M.sequence_arrays({"local_pose_list": poses, "cam_list": cams[:-1] + [{"loc": np.zeros(3), "rot": np.zeros(4)}],
                           "frame_rate": 25}, True)
    # local windows do not read the cameras (local_dataset.py never touches cam_list)
    M.sequence_arrays({"local_pose_list": poses, "frame_rate": 25}, False)


_CALLS = []


def _record_call(*a):
    _CALLS.append(a)
    return a


class _Payload:
    def __reduce__(self):
        return (_record_call, ("constructed",))


def test_restricted_reader_refuses_foreign_globals_and_constructs_nothing(tmp_path, monkeypatch):
    monkeypatch.delenv(M.TRUST_ENV, raising=False)
    path = str(tmp_path / "seq.pkl")
    with open(path, "wb") as f:
        pickle.dump({"local_pose_list": [np.zeros((15, 3))], "cam_list": [], "frame_rate": 25, "extra": _Payload()}, f)
    _CALLS.clear()
    with pytest.raises(pickle.UnpicklingError, match="_record_call"):
        M.read_motion_pickle(path)
    assert _CALLS == []
    monkeypatch.setenv(M.TRUST_ENV, "1")                   # the checkpoint loader's switch
    assert M.read_motion_pickle(path)["extra"] == ("constructed",) and len(_CALLS) == 1
    monkeypatch.delenv(M.TRUST_ENV)
    assert M.read_motion_pickle(path, trust=True)["frame_rate"] == 25
    # numpy content written under either numpy generation's module path is allowed
    ok = str(tmp_path / "ok.pkl")
    with open(ok, "wb") as f:
        pickle.dump({"a": np.arange(6.0).reshape(2, 3), "s": np.float64(59.94), "f": np.zeros(2, np.float32)}, f, protocol=2)
    d = M.read_motion_pickle(ok)
    assert d["s"] == 59.94 and d["a"].shape == (2, 3) and d["f"].dtype == np.float32


def test_cli_parses_train_global_sh_and_refuses_what_it_cannot_do(tmp_path, golden, capsys):
    from globalegomocap_amd import vae_train
    a = vae_train._parser().parse_args(TRAIN_GLOBAL_SH)
    assert a.network == "cnn" and a.with_mo2cap2_data is False and a.new_dataset is False and a.fps == 25 and a.poses == "global"
    assert a.slide_window_step == 1 and a.seq_names is None
    with pytest.raises(SystemExit):
        vae_train._cli(TRAIN_GLOBAL_SH[:-1] + ["mlp"])
    assert "--network mlp is not available" in capsys.readouterr().err
    argv = list(TRAIN_GLOBAL_SH)
    argv[argv.index("--with_mo2cap2_data") + 1] = "True"
    with pytest.raises(SystemExit):
        vae_train._cli(argv)
    assert "--seq_names" in capsys.readouterr().err
    # a directory whose training split holds fewer windows than one batch: refused before anything touches the device
    g = golden("motion_windows")
    write_pickles(g, tmp_path)
    for k, (name, d) in enumerate(sequences(g)[:5]):            # 12 files: the training split ([:-10]) is two of them
        with open(str(tmp_path / ("copy%d_" % k + name)), "wb") as f:
            pickle.dump(d, f)
    argv = list(TRAIN_GLOBAL_SH)
    argv[argv.index("--train_data_path") + 1] = str(tmp_path)
    with pytest.raises(SystemExit):
        vae_train._cli(argv + ["--test_data_path", str(tmp_path)])
    assert "fewer than one batch" in capsys.readouterr().err
