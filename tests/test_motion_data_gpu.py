"""The device side of the motion-window data path: gem_motion_cameras / gem_motion_windows (csrc/motion_windows.h) against the
reference's windows (tests/golden/motion_windows.npz) and the host twin, the trainer fed from a MotionWindows, and the CLI end to end
from a directory of motion pickles."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from globalegomocap_amd import motion_data as M, synth, vae as vae_schema
from motion_fixture import cases, sequences, ulps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dataset(g, poses, fn, ws, fps, slide):
    seqs = [M.sequence_arrays(d, poses == "global", name) for name, d in sequences(g)]
    return M.MotionWindows(seqs, poses, fn, ws, fps, slide)


def _check(got, ref, poses, what):
    assert got.shape == ref.shape, what
    if poses == "local":
        assert np.array_equal(got, ref), what
    else:
        assert ulps(got, ref).max() <= 1.0, (what, ulps(got, ref).max())


def test_device_windows_against_the_reference_and_the_host_twin(golden):
    import torch
    g = golden("motion_windows")
    rng = np.random.default_rng(5)
    for c, poses, fn, ws, fps, slide in cases(g):
        ds = _dataset(g, poses, fn, ws, fps, slide)
        n = len(ds)
        # the reference's recorded windows (first and last of every sequence, a few at random)
        _check(ds.batch(g["case%d/ids" % c]).cpu().numpy(), g["case%d/windows" % c], poses, ("fixture", c))
        # every window in one launch against the twin, and against the same windows in launches of 64 ids
        every = ds.materialize()
        _check(every.cpu().numpy(), ds.windows_numpy(np.arange(n)), poses, ("all", c))
        parts = torch.cat([ds.batch(torch.arange(i, min(i + 64, n), device=ds.device)) for i in range(0, n, 64)])
        assert torch.equal(parts, every), c
        # random ids with repeats and the edge windows, out-of-range ids (NaN rows) in the same launch
        ids = np.concatenate([rng.integers(0, n, size=50), ds.window0[:-1][ds.counts > 0], ds.window0[1:][ds.counts > 0] - 1])
        bad = np.array([n, n + 7, -1, 1 << 40])
        mixed = np.concatenate([ids, bad])
        rng.shuffle(mixed)
        out = ds.batch(torch.as_tensor(mixed, device=ds.device)).cpu().numpy()
        valid = (mixed >= 0) & (mixed < n)
        assert np.isnan(out[~valid]).all() and (~valid).sum() == len(bad)
        _check(out[valid], ds.windows_numpy(mixed[valid]), poses, ("random", c))
        # into a caller's buffer
        buf = torch.full((8, ds.seq_len, 45), 7.0, device=ds.device)
        assert ds.batch(torch.arange(8, device=ds.device), out=buf) is buf and torch.equal(buf, every[:8])


def test_device_cameras_match_scipy():
    import torch
    from scipy.spatial.transform import Rotation
    from globalegomocap_amd import _capi
    rng = np.random.default_rng(1)
    q = rng.normal(size=(1000, 4)) * rng.uniform(0.01, 100, size=(1000, 1))
    q[:100, 3] = rng.normal(size=100) * 1e-9                 # near half turns
    loc = rng.normal(size=(1000, 3)) * 10
    lib = _capi.load_library()
    dq, dl = torch.as_tensor(q, device="cuda"), torch.as_tensor(loc, device="cuda")
    cam = torch.empty((1000, 3, 4), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    import ctypes as C
    _capi.check(lib.gem_motion_cameras(dl.data_ptr(), dq.data_ptr(), 1000, cam.data_ptr(), C.c_void_p(s)), lib)
    ref = Rotation.from_quat(q).as_matrix()
    got = cam.cpu().numpy()
    assert np.abs(got[:, :, :3] - ref).max() <= 4e-16 and np.array_equal(got[:, :, 3], loc)


def _synthetic_sequences(n_seq, frames, seed, rate=25.0):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_seq):
        cams = synth.jitter_cameras(synth.make_cameras(frames, step=0.02), rng, rot_deg=10.0, trans_m=0.1)
        from scipy.spatial.transform import Rotation
        q = Rotation.from_matrix(cams[:, :3, :3]).as_quat()
        out.append({"local_pose_list": [p for p in synth.make_motion(frames, rng, t0=rng.uniform(0, 10)).astype(np.float32)],
                    "cam_list": [{"loc": l, "rot": r} for l, r in zip(cams[:, :3, 3], q)], "frame_rate": rate})
    return out


@pytest.mark.parametrize("poses", ["global", "local"])
def test_fit_from_motion_windows_equals_fit_from_the_materialised_windows(poses):
    import torch
    from globalegomocap_amd.vae_train import VAETrainer, initial_state_dict
    shape = vae_schema.VAEShape(latent_dim=64, hidden=(32, 64))
    seqs = [M.sequence_arrays(d, poses == "global") for d in _synthetic_sequences(4, 90, 3)]
    ds = M.MotionWindows(seqs, poses, 10)
    assert len(ds) == 4 * 80
    data = ds.materialize().cpu().numpy()         # (an array input: fit uploads it once, as before)
    results = []
    for src in (ds, data):
        tr = VAETrainer(shape, batch_size=64, lr=2e-3, seed=4, state_dict=initial_state_dict(shape, 4))
        try:
            lines = []
            hist = tr.fit(src, epochs=2, kl_weight=0.5, test_windows=src, log_step=1, seed=9, log=lines.append)
            torch.cuda.synchronize()
            results.append((hist, lines, tr.state_dict(), tr.optimizer_state()))
        finally:
            tr.close()
    (h0, l0, sd0, o0), (h1, l1, sd1, o1) = results
    assert len(h0) == 2 * 5 - 1 and h0 == h1 and l0 == l1 and any(l.startswith("eval loss is: ") for l in l0)
    for k in sd0:
        assert np.array_equal(np.asarray(sd0[k]), np.asarray(sd1[k])), k
    assert o0["step"] == o1["step"] == 10
    for m in ("exp_avg", "exp_avg_sq"):
        for k in o0[m]:
            assert np.array_equal(o0[m][k], o1[m][k]), (m, k)


def test_cli_trains_from_a_directory_of_motion_pickles(tmp_path):
    from globalegomocap_amd.vae import load_checkpoint, VAEShape
    from globalegomocap_amd.engine import WindowEngine
    data = tmp_path / "EgocentricAMASS"
    data.mkdir()
    for k, d in enumerate(_synthetic_sequences(12, 60, 11, rate=50.0)):
        with open(str(data / ("seq_%02d.pkl" % k)), "wb") as f:
            pickle.dump(d, f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "globalegomocap_amd.vae_train", "--log_dir", "run", "--train_data_path", str(data), "--latent_dim", "32",
           "--kl_weight", "0.5", "--seq_length", "10", "--batch_size", "16", "--new_dataset", "False", "--with_mo2cap2_data", "False",
           "--fps", "25", "--network", "cnn", "--poses", "local", "--epoch", "1", "--log_step", "2"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "80 training windows from 2 files" in r.stdout and "400 test windows" in r.stdout, r.stdout
    assert "eval loss is: " in r.stdout
    ck = os.path.join(str(tmp_path), "logs", "run", "checkpoints", "0.pth.tar")
    sd = load_checkpoint(ck)
    shape = VAEShape(latent_dim=32)
    assert [k for k in sd if not k.endswith("num_batches_tracked")] == list(shape.schema())
    eng = WindowEngine(shape, max_windows=16)
    try:
        eng.load_vae(0, sd)
    finally:
        eng.close()
