"""the VAE training step on the device (gem_trainer_*, csrc/train.hip) against the unmodified
reference's own steps (tests/golden/train_tiny.npz) and against the CPU port (oracle/torch_port.TrainPort) at full size."""
import os

import numpy as np
import pytest

from globalegomocap_amd import synth, vae as vae_schema
from helpers import FULL, train_golden_case

pytestmark = pytest.mark.gpu


def _close(a, b, rtol, scale_atol, msg):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=scale_atol * max(1e-30, float(np.abs(b).max())), err_msg=msg)


LINEAR_WEIGHTS = ("fc_mu.weight", "fc_var.weight", "decoder_input.weight")


@pytest.mark.parametrize("loop_mode", [False, True])
@pytest.mark.parametrize("case", ["mn", "sum"])
def test_training_steps_against_the_reference_run(golden, case, loop_mode):
    """Three to four steps of the unmodified reference (ConvVAE + torch.optim.Adam at its eps = 1e-8, tests/golden/train_tiny.npz)
    in both step modes of the trainer: update = 1 (every gradient left in the arena) and update = 2 = the training loop's mode (what
    VAETrainer.fit and fit_vae_device run: the linear layers' weight gradients formed inside their Adam step) -- losses, the
    gradients the mode leaves, parameters, Adam moments and running statistics against the reference's."""
    from globalegomocap_amd.vae_train import VAETrainer
    c = train_golden_case(golden("train_tiny"), case)
    tr = VAETrainer(c["shape"], batch_size=c["batch"], lr=c["lr"], weight_decay=c["wd"], state_dict=c["init"],
                    recon_reduction="sum" if c["form"] == "kl_weight" else "mean")
    try:
        for s in range(c["steps"]):
            out = tr.step(c["poses"][s], c["w"], eps=c["eps"][s], keep_gradients=not loop_mode)
            np.testing.assert_allclose(out, c["losses"][s], rtol=5e-5)
            if s == 0:
                g = tr.gradients()
                assert set(g) == set(c["grad0"]) - (set(LINEAR_WEIGHTS) if loop_mode else set())
                gmax = max(float(np.abs(v).max()) for v in c["grad0"].values())
                for k, v in g.items():
                    r = c["grad0"][k]
                    # (".0.bias": a conv bias in front of a BatchNorm -- its exact gradient is zero, both sides hold rounding noise)
                    lim = 5e-6 * gmax if k.endswith(".0.bias") else 1e-4 * np.abs(r).max() + 2e-7 * gmax
                    assert np.abs(np.asarray(v, np.float64) - r).max() <= lim, k
        sd = tr.state_dict()
        assert int(sd["encoder.0.1.num_batches_tracked"]) == c["steps"]
        # The bias of a conv that feeds a BatchNorm has an exactly zero gradient (the batch mean is subtracted): what torch and the
        # kernels hold there is rounding noise of the size 1e-9, which Adam's normalisation turns into steps of the size lr in either (in opposite
        # directions at worst, and a step after a sign flip can exceed lr: hence 4 lr per step).
        # (and the running mean of that BatchNorm follows the bias)
        noise = lambda k: k.endswith(".0.bias") or k.endswith("running_mean")        # noqa: E731
        for k, v in c["final"].items():
            d = np.abs(np.asarray(sd[k], np.float64) - v).max()
            if k.endswith("running_var"):
                assert d <= 1e-4 * max(1.0, float(np.abs(v).max())), (k, d)
                continue
            assert d <= (4 * c["steps"] * c["lr"] if noise(k) else 1e-5 + 0.02 * c["lr"]), (k, d)
        opt = tr.optimizer_state()
        assert opt["step"] == c["steps"]
        for k, v in c["exp_avg"].items():
            if not noise(k):
                _close(opt["exp_avg"][k], v, 2e-3, 1e-4, "exp_avg " + k)
                _close(opt["exp_avg_sq"][k], c["exp_avg_sq"][k], 4e-3, 2e-4, "exp_avg_sq " + k)
    finally:
        tr.close()


@pytest.mark.parametrize("loop_mode", [False, True])
def test_full_size_training_step_against_the_reference_run(golden, loop_mode):
    """ONE device step at D = 2048, batch 8, against the unmodified reference's own step (tests/golden/train_full.npz, made by
    oracle/make_golden_train.py --full from networks/train.py:77-83 + SeqConvVAE.py:191-219): losses, every tensor's gradient
    2-norm and 256 sampled entries at 1e-4, the sampled parameters after Adam, the BatchNorm running statistics -- in both step
    modes (loop_mode = gem_trainer_step update = 2, the mode the training loop runs; its linear-layer weight gradients are never
    written out, their PARAMETERS after the step are compared like everyone else's)."""
    from globalegomocap_amd.vae_train import VAETrainer
    from helpers import train_full_case, check_full_training_step
    c = train_full_case(golden("train_full"))
    tr = VAETrainer(c["shape"], batch_size=64, lr=c["lr"], weight_decay=c["wd"], state_dict=c["init"])
    try:
        losses = tr.step(c["poses"], c["w"], eps=c["eps"], keep_gradients=not loop_mode)
        sd = tr.state_dict()
        grads = tr.gradients()
        assert all((k in grads) != loop_mode for k in LINEAR_WEIGHTS)
        check_full_training_step(c, losses, grads, sd, sd, loss_rtol=5e-5, grad_tol=1e-4)
        if loop_mode:          # nothing hands out the incomplete arena as if it were whole
            from globalegomocap_amd import _capi
            with pytest.raises(_capi.GemError, match="incomplete"):
                tr.arena_tensor(1)
    finally:
        tr.close()


@pytest.mark.parametrize("batch", [96, 256])
def test_step_modes_agree_on_the_linear_layers_between_65_and_256_windows(batch):
    """For 64 < B <= 256 both step modes run the SAME backward-data kernels for the linear layers (the fused dX form of update = 2 is
    for B <= 64 only); what differs is where the weight gradient is summed -- into the arena (gemm_tn + adam_kernel, update = 1) or
    inside the Adam step (gemm_tn_adam_kernel, update = 2: other strip order over the rows).  At the reference's eps = 1e-8, after one
    step: identical losses (same forward), parameters of fc_mu | fc_var and decoder_input within a thousandth of the step lr (measured:
    1 ulp, 9e-10), first moments to 1e-5 of their largest entry, second moments to 1e-5 relative."""
    from globalegomocap_amd.vae_train import VAETrainer, initial_state_dict, unpack_arena
    init = initial_state_dict(FULL, 9)
    poses = synth.make_training_windows(batch, FULL.seq_len, 6)
    eps = np.random.default_rng(6).standard_normal((batch, FULL.latent_dim)).astype(np.float32)
    lr = 1e-3
    a = VAETrainer(FULL, batch_size=batch, lr=lr, weight_decay=1e-5, state_dict=init)
    b = VAETrainer(FULL, batch_size=batch, lr=lr, weight_decay=1e-5, state_dict=init)
    try:
        la = a.step(poses, 0.01, eps=eps)
        lb = b.step(poses, 0.01, eps=eps, keep_gradients=False)
        np.testing.assert_array_equal(la, lb)
        for what in (0, 3, 4):
            ua, ub = unpack_arena(a._down(what), FULL), unpack_arena(b._down(what), FULL)
            for k in LINEAR_WEIGHTS:
                x, y = np.asarray(ua[k], np.float64), np.asarray(ub[k], np.float64)
                if what == 0:
                    assert np.abs(x - y).max() <= 1e-3 * lr, (k, float(np.abs(x - y).max()))
                    assert np.abs(x - np.asarray(init[k], np.float64)).max() > 0.5 * lr          # (the step really moved them)
                else:
                    assert np.abs(x - y).max() <= 1e-5 * np.abs(x).max(), (what, k, float(np.abs(x - y).max()), float(np.abs(x).max()))
    finally:
        a.close(); b.close()


def test_full_size_training_step_against_the_port():
    import torch
    from globalegomocap_amd.vae_train import VAETrainer, initial_state_dict
    from oracle.torch_port import TrainPort
    B = 24
    init = initial_state_dict(FULL, 11)
    poses = synth.make_training_windows(2 * B, FULL.seq_len, 3).reshape(2, B, FULL.seq_len, 45)
    eps = np.random.default_rng(1).standard_normal((2, B, FULL.latent_dim)).astype(np.float32)
    port = TrainPort(init, lr=1e-4, weight_decay=1e-5)
    tr = VAETrainer(FULL, batch_size=64, lr=1e-4, weight_decay=1e-5, state_dict=init)
    try:
        for s in range(2):
            ref = port.step(poses[s], eps[s], 0.25 * B / 1000.0)
            out = tr.step(poses[s], 0.25 * B / 1000.0, eps=eps[s])
            np.testing.assert_allclose(out, ref, rtol=1e-4)
            g, gr = tr.gradients(), port.gradients()
            gmax = max(float(np.abs(v).max()) for v in gr.values())
            for k, v in gr.items():
                d = np.abs(np.asarray(g[k], np.float64) - v).max()
                # (second step: both sides have taken an Adam step, which moves EVERY entry by ~lr whatever the size of its gradient --
                # entries whose gradient is rounding noise land differently, and the next gradients differ by a percent or so in
                # single entries: compared in the 2-norm there)
                if s == 0:
                    assert d <= (5e-6 * gmax if k.endswith(".0.bias") else 1e-3 * np.abs(v).max() + 1e-6 * gmax), (s, k, d, np.abs(v).max())
                elif not k.endswith(".0.bias"):
                    assert np.linalg.norm(np.asarray(g[k], np.float64) - v) <= 3e-2 * np.linalg.norm(v) + 1e-6 * gmax, (s, k)
        sd, sr = tr.state_dict(), port.state_dict()
        for k, v in sr.items():
            d = np.abs(np.asarray(sd[k], np.float64) - v).max()
            if k.endswith("running_var"):
                assert d <= 1e-5 * max(1.0, np.abs(v).max()), (k, d)
            elif k.endswith(".0.bias") or k.endswith("running_mean"):              # zero-gradient biases in front of a BatchNorm: Adam amplifies rounding noise
                assert d <= 4 * 2 * 1e-4, (k, d)
            else:
                # after two Adam steps an entry has moved by at most 2 lr; entries whose gradient is far above rounding (all but a few
                # percent of a tensor) agree to a twentieth of lr
                assert d <= 2 * 1e-4 * 1.01 and np.mean(np.abs(np.asarray(sd[k], np.float64) - v) > 0.05 * 1e-4) < 5e-2, (k, d)
    finally:
        tr.close()


def test_fit_lowers_the_loss_and_writes_the_reference_checkpoint_schema(tmp_path):
    import torch
    from globalegomocap_amd.engine import WindowEngine
    from globalegomocap_amd.vae_train import VAETrainer
    shape = vae_schema.VAEShape(latent_dim=64, hidden=(32, 64))
    data = synth.make_training_windows(640, shape.seq_len, 1)
    tr = VAETrainer(shape, batch_size=64, lr=2e-3, seed=2)
    try:
        lines = []
        first = tr.step(data[:64], 1e-3, update=False)
        hist = tr.fit(data, epochs=6, kl_weight=0.01, log_step=20, checkpoint_dir=str(tmp_path), log=lines.append)
        last = tr.step(data[:64], 1e-3, update=False)
        assert last[1] < 0.5 * first[1], (first, last)
        assert len(hist) == 2 and hist[1][2] < hist[0][2]           # 60 steps, logged at counts 20 and 40 like train.py:88-95
        assert any(l.startswith("eval loss is: ") for l in lines)
        ck = torch.load(os.path.join(str(tmp_path), "5.pth.tar"), map_location="cpu", weights_only=False)
        assert ck["epoch"] == 6 and ck["eval_result"] > 0
        keys = [k for k in ck["state_dict"] if not k.endswith("num_batches_tracked")]
        assert keys == list(shape.schema())
        # the checkpoint loads into the optimiser's engine (optimizer.py:59-60) and reconstructs like the trainer's eval pass
        eng = WindowEngine(shape, max_windows=64)
        eng.load_vae(0, ck["state_dict"])
        x = torch.as_tensor(data[:64])
        rec = eng.decode(0, eng.encode(0, x)[0]).cpu()
        err = (rec - x.reshape(64, shape.seq_len, 15, 3)).norm(dim=-1).mean().item()
        assert abs(err - ck["eval_result"]) < 0.5 * ck["eval_result"] + 0.02
        eng.close()
    finally:
        tr.close()


def test_checkpoint_carries_torch_adam_state_and_resumes_bitwise(tmp_path):
    """networks/train.py:102-108 saves `optimizer.state_dict()`: the checkpoint's 'optimizer' entry must load into
    torch.optim.Adam over a network with the reference's parameter order (here the CPU port's MotionVAE: same names, same
    order), and a fresh trainer that loads the checkpoint continues exactly where the first one stands: next step bitwise equal.
    BatchNorm's num_batches_tracked counts train-mode forwards (gradient-only passes included), like torch's."""
    import torch
    from globalegomocap_amd.vae_train import VAETrainer, initial_state_dict
    from oracle.torch_port import TrainPort
    shape = vae_schema.VAEShape(latent_dim=64, hidden=(32, 64))
    data = synth.make_training_windows(256, shape.seq_len, 7)
    eps = np.random.default_rng(3).standard_normal((3, 64, shape.latent_dim)).astype(np.float32)
    tr = VAETrainer(shape, batch_size=64, lr=1e-3, weight_decay=1e-4, seed=5)
    tr2 = None
    try:
        tr.step(data[:64], 0.01, eps=eps[0], update=False)                  # a gradient-only pass: a forward, not a step
        tr.fit(data, epochs=1, kl_weight=0.01, checkpoint_dir=str(tmp_path), log=lambda *a: None, test_windows=False)
        ck = torch.load(os.path.join(str(tmp_path), "0.pth.tar"), map_location="cpu", weights_only=False)
        assert int(ck["state_dict"]["encoder.0.1.num_batches_tracked"]) == 5 and tr.steps == 4
        port = TrainPort(initial_state_dict(shape, 5), lr=1.0)
        port.opt.load_state_dict(ck["optimizer"])                            # torch accepts the schema
        st = port.opt.state_dict()
        assert st["param_groups"][0]["lr"] == 1e-3 and st["param_groups"][0]["weight_decay"] == 1e-4
        names = [k for k, _ in port.net.named_parameters()]
        own = tr.optimizer_state()
        for i, k in enumerate(names):
            assert float(st["state"][i]["step"]) == 4.0
            np.testing.assert_array_equal(st["state"][i]["exp_avg"].numpy(), own["exp_avg"][k], err_msg=k)
            np.testing.assert_array_equal(st["state"][i]["exp_avg_sq"].numpy(), own["exp_avg_sq"][k], err_msg=k)
        tr2 = VAETrainer(shape, batch_size=64, lr=7.0, seed=99)              # (everything that matters comes from the file)
        assert tr2.load_checkpoint(os.path.join(str(tmp_path), "0.pth.tar")) == 1
        assert tr2.steps == 4 and tr2.forwards == 5
        a = tr.step(data[64:128], 0.01, eps=eps[1])
        b = tr2.step(data[64:128], 0.01, eps=eps[1])
        assert a == b
        sa, sb = tr.state_dict(), tr2.state_dict()
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    finally:
        tr.close()
        if tr2 is not None:
            tr2.close()


def test_trainer_rejects_bad_arguments():
    from globalegomocap_amd import _capi
    from globalegomocap_amd.vae_train import VAETrainer
    shape = vae_schema.VAEShape(latent_dim=64, hidden=(32, 64))
    tr = VAETrainer(shape, batch_size=8)
    try:
        with pytest.raises(_capi.GemError, match="max_windows"):
            tr.step(np.zeros((9, 10, 45), np.float32), 0.1)
        with pytest.raises(_capi.GemError, match="BatchNorm"):
            tr.step(np.zeros((1, 10, 45), np.float32), 0.1)
        with pytest.raises(ValueError):
            tr.step(np.zeros((4, 10, 44), np.float32), 0.1)
        import ctypes as C
        import torch
        x = torch.zeros(4, 10, 45, device="cuda")
        e = torch.zeros(4, 64, device="cuda")
        for bad in (-1, 3):          # (gem_trainer_step: update is 0, 1 or 2 -- nothing else silently behaves like 1)
            assert tr.lib.gem_trainer_step(tr._t, 4, x.data_ptr(), e.data_ptr(), C.byref(tr.opts), bad, None, None) != 0
    finally:
        tr.close()


DP_SCRIPT = """
import os, sys
sys.path.insert(0, %r)
import numpy as np, torch, torch.distributed as dist
from globalegomocap_amd import synth, vae as vae_schema
from globalegomocap_amd.vae_train import VAETrainer, initial_state_dict
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo")
shape = vae_schema.VAEShape(latent_dim=64, hidden=(32, 64))
data = synth.make_training_windows(4 * 16, shape.seq_len, 3).reshape(4, 16, shape.seq_len, 45)     # [step*world + rank]
eps = np.random.default_rng(5).standard_normal((4, 16, shape.latent_dim)).astype(np.float32)
# rank 1 starts from OTHER weights: the initial broadcast must bring rank 0's
tr = VAETrainer(shape, batch_size=16, lr=1e-3, weight_decay=1e-4, state_dict=initial_state_dict(shape, 7 + rank))
tr.broadcast_parameters(0)
out = []
for s in range(2):
    out.append(tr.step_data_parallel(data[s * world + rank], 0.01, eps=eps[s * world + rank]))
sd = tr.state_dict()
np.savez(sys.argv[1] + ".rank%%d.npz" %% rank, losses=np.array(out), **{k: v for k, v in sd.items()})
tr.close()
dist.barrier()
dist.destroy_process_group()
"""


def test_two_rank_data_parallel_steps_equal_the_mean_gradient_step(tmp_path):
    """step_data_parallel on two REAL ranks (torch.distributed.run, gloo, both on the one card of the test box) against one
    process doing what DDP defines: the two ranks' gradients from their own batches (own BatchNorm statistics), their mean,
    one Adam step on it.  The parameters must come out bitwise equal on both ranks and bitwise equal to the emulation."""
    import subprocess
    import sys
    import torch
    from globalegomocap_amd.vae_train import VAETrainer, initial_state_dict, pack_arena
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "dp.py"
    script.write_text(DP_SCRIPT % root)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    import socket
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(script), str(tmp_path / "dp")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    a, b = np.load(str(tmp_path / "dp.rank0.npz")), np.load(str(tmp_path / "dp.rank1.npz"))
    shape = vae_schema.VAEShape(latent_dim=64, hidden=(32, 64))
    data = synth.make_training_windows(4 * 16, shape.seq_len, 3).reshape(4, 16, shape.seq_len, 45)
    eps = np.random.default_rng(5).standard_normal((4, 16, shape.latent_dim)).astype(np.float32)
    # emulation: two trainers = the two ranks; gradients exchanged through the arena views
    t0 = VAETrainer(shape, batch_size=16, lr=1e-3, weight_decay=1e-4, state_dict=initial_state_dict(shape, 7))
    t1 = VAETrainer(shape, batch_size=16, lr=1e-3, weight_decay=1e-4, state_dict=initial_state_dict(shape, 7))
    try:
        import ctypes as C
        from globalegomocap_amd import _capi
        losses = []
        for s in range(2):
            l0 = t0.step(data[2 * s], 0.01, eps=eps[2 * s], update=False)
            l1 = t1.step(data[2 * s + 1], 0.01, eps=eps[2 * s + 1], update=False)
            g0, g1 = t0.arena_tensor(1), t1.arena_tensor(1)
            tot = g0 + g1
            g0.copy_(tot)
            g1.copy_(tot)
            for t in (t0, t1):
                _capi.check(t.lib.gem_trainer_apply(t._t, C.byref(t.opts), 0.5, None), t.lib)
                t.steps += 1
            losses.append([(x + y) / 2 for x, y in zip(l0, l1)])
        torch.cuda.synchronize()
        s0, s1 = t0.state_dict(), t1.state_dict()
        np.testing.assert_allclose(a["losses"], np.array(losses), rtol=1e-12)
        np.testing.assert_array_equal(a["losses"], b["losses"])
        for k in shape.schema():
            if "running" in k:                       # BatchNorm statistics are per rank
                assert np.array_equal(a[k], s0[k]) and np.array_equal(b[k], s1[k]), k
            else:
                assert np.array_equal(a[k], b[k]), k
                assert np.array_equal(a[k], s0[k]), k
        assert not np.array_equal(a["encoder.0.1.running_mean"], b["encoder.0.1.running_mean"])
    finally:
        t0.close()
        t1.close()


@pytest.mark.parametrize("batch", [4, 130, 300])
def test_training_step_against_the_port_at_other_batch_sizes(batch):
    """The code paths the golden batches (9, 12) do not reach, each asserted through gem_trainer_route: 4 windows = 40 rows, a single
    weight-gradient slab written straight into the gradient arena; 130 windows = 1300 rows, the row-block BatchNorm BACKWARD for the
    encoder's last block (more rows than a thread keeps in registers: per-row-block partial sums, two launches) -- the forward
    statistics still come out of the conv epilogues, as for every batch of at most 2560 rows; 300 windows = 3000 rows, the row-block
    BatchNorm forward as well, the linear layers' weight gradients in two slabs and the conv layers' in 16 slabs of more than 64
    rows."""
    from globalegomocap_amd.vae_train import VAETrainer, initial_state_dict
    from oracle.torch_port import TrainPort
    shape = vae_schema.VAEShape(latent_dim=72, hidden=(24, 40, 96))
    init = initial_state_dict(shape, 21)
    poses = synth.make_training_windows(2 * batch, shape.seq_len, 8).reshape(2, batch, shape.seq_len, 45)
    eps = np.random.default_rng(2).standard_normal((2, batch, shape.latent_dim)).astype(np.float32)
    port = TrainPort(init, lr=1e-3, weight_decay=1e-4)
    tr = VAETrainer(shape, batch_size=batch, lr=1e-3, weight_decay=1e-4, state_dict=init)
    try:
        route = tr.route(batch)
        want = {4: dict(bn_forward=0, bn_backward=1, conv_weight_grad_slabs=1, linear_weight_grad_slabs=1),
                130: dict(bn_forward=0, bn_backward=2, conv_weight_grad_slabs=14, linear_weight_grad_slabs=1),
                300: dict(bn_forward=2, bn_backward=2, conv_weight_grad_slabs=16, linear_weight_grad_slabs=2)}[batch]
        assert {k: route[k] for k in want} == want, route
        for s in range(2):
            ref = port.step(poses[s], eps[s], 0.02)
            out = tr.step(poses[s], 0.02, eps=eps[s])
            np.testing.assert_allclose(out, ref, rtol=5e-5)
            g, gr = tr.gradients(), port.gradients()
            gmax = max(float(np.abs(v).max()) for v in gr.values())
            for k, v in gr.items():
                d = np.abs(np.asarray(g[k], np.float64) - v).max()
                # (s = 1: after an Adam step, which moves every entry by ~lr whatever its gradient: 2-norm, see the full-size test)
                if s == 0:
                    assert d <= (5e-6 * gmax if k.endswith(".0.bias") else 2e-4 * np.abs(v).max() + 5e-7 * gmax), (s, k, d, np.abs(v).max())
                elif not k.endswith(".0.bias"):
                    assert np.linalg.norm(np.asarray(g[k], np.float64) - v) <= 3e-2 * np.linalg.norm(v) + 1e-6 * gmax, (s, k)
        sd, sr = tr.state_dict(), port.state_dict()
        for k, v in sr.items():
            if k.endswith("running_var"):
                assert np.abs(np.asarray(sd[k], np.float64) - v).max() <= 1e-4 * max(1.0, float(np.abs(v).max())), k
    finally:
        tr.close()


def test_device_fit_reaches_the_accuracy_of_the_autograd_fit():
    """fit_vae_device (the HIP trainer) against vae_torch.fit_vae (PyTorch autograd on the same card), same recipe on the same
    synthetic motion: what row f.4 is for -- well-conditioned weights in the reference's schema.  (The two differ in their random
    streams, so the reconstruction errors are compared, not the weights.)"""
    from globalegomocap_amd.vae_train import fit_vae_device
    from globalegomocap_amd.vae_torch import fit_vae
    shape = vae_schema.VAEShape(latent_dim=128, hidden=(64, 64, 128))
    win = synth.make_training_windows(2048, shape.seq_len, 4)
    sd_t, e_t = fit_vae(shape, win, steps=600, batch=64, lr=2e-3, kl_weight=0.01, seed=4, device="cuda")
    sd_d, e_d = fit_vae_device(shape, win, steps=600, batch=64, lr=2e-3, kl_weight=0.01, seed=4)
    assert list(sd_d) == list(shape.schema())
    assert e_d < 1.5 * e_t + 2e-3 and e_d < 0.03, (e_d, e_t)


@pytest.mark.parametrize("adam_eps", [1e-8, 1e-6])
def test_training_loop_mode_steps_like_the_default_mode(adam_eps):
    """gem_trainer_step update = 2 (the linear layers' weight gradient formed inside their Adam step, never written to the gradient
    arena; at this batch their backward-data products too: gemm_tn_adam_dx_kernel) against update = 1 on the same batches at full size.

    The two modes sum the backward-data products in a different order (strips of n tiles against slabs), so their gradients differ in
    the last bits, and what becomes of such bits is a property of the optimiser, not of the kernels (each mode by itself is bitwise
    reproducible: tools/train_dbg.py same / same2).  With the reference's eps = 1e-8 Adam's first step moves an entry whose gradient is
    of the order of eps (8 % of the fc weights) by lr g / (|g| + eps), and rounding noise is percent-level relative to such a g.  So:
    the first step's gradients (they have passed through both backward-data products) to 1e-5 of each tensor's maximum; with eps = 1e-6
    -- that amplification switched off -- parameters, moments and running statistics after the FIRST update as tightly as when the modes
    shared their backward-data kernels; and the losses of three successive steps at the gate the device step is held to against the CPU
    port over successive steps (trajectories separate from the third step on: measured 7e-5 / 8e-6 for eps = 1e-8 / 1e-6)."""
    from globalegomocap_amd.vae_train import VAETrainer, initial_state_dict, unpack_arena
    B = 64
    init = initial_state_dict(FULL, 5)
    poses = synth.make_training_windows(3 * B, FULL.seq_len, 4).reshape(3, B, FULL.seq_len, 45)
    eps = np.random.default_rng(3).standard_normal((3, B, FULL.latent_dim)).astype(np.float32)
    a = VAETrainer(FULL, batch_size=B, lr=1e-3, weight_decay=1e-5, eps=adam_eps, state_dict=init)
    b = VAETrainer(FULL, batch_size=B, lr=1e-3, weight_decay=1e-5, eps=adam_eps, state_dict=init)
    try:
        for s in range(3):
            la = a.step(poses[s], 0.01, eps=eps[s])
            lb = b.step(poses[s], 0.01, eps=eps[s], keep_gradients=False)
            np.testing.assert_allclose(lb, la, rtol=1e-7 if s == 0 else 2e-4)          # (first step: the same forward on the same parameters)
            if s > 0:
                continue
            ga, gb = a.gradients(), b.gradients()
            for k in ga:
                if k.endswith(".0.bias") or k.split(".")[0] in ("fc_mu", "fc_var", "decoder_input") and k.endswith("weight"):
                    continue          # (rounding noise around an exact zero; not left in the arena by this mode)
                assert np.abs(ga[k] - gb[k]).max() <= 1e-5 * np.abs(ga[k]).max(), k
            if adam_eps < 1e-7:
                continue
            for what in (0, 3, 4):
                ua, ub = unpack_arena(a._down(what), FULL), unpack_arena(b._down(what), FULL)
                for k in ua:
                    # (".0.bias": a conv bias in front of a BatchNorm -- its exact gradient is zero, both runs hold rounding noise there)
                    if k.endswith(".0.bias"):
                        continue
                    x, y = np.asarray(ua[k], np.float64), np.asarray(ub[k], np.float64)
                    assert np.linalg.norm(x - y) <= (1e-5 if what == 0 else 1e-4) * max(1e-30, np.linalg.norm(x)), (what, k)
            sa, sb = a._down(2).astype(np.float64), b._down(2).astype(np.float64)
            assert np.abs(sa - sb).max() <= 1e-6 * np.abs(sa).max()
        assert a.steps == b.steps == 3
    finally:
        a.close(); b.close()


def test_training_loop_mode_at_a_large_batch():
    """update = 2 beyond one slab of rows (300 windows: the fused kernel walks all 300 rows where the two-kernel path sums two
    slabs) on a small network: the losses of three successive steps against update = 1, and against the port."""
    from globalegomocap_amd.vae_train import VAETrainer, initial_state_dict
    from oracle.torch_port import TrainPort
    shape = vae_schema.VAEShape(latent_dim=72, hidden=(24, 40, 96))
    batch = 300
    init = initial_state_dict(shape, 23)
    poses = synth.make_training_windows(3 * batch, shape.seq_len, 9).reshape(3, batch, shape.seq_len, 45)
    eps = np.random.default_rng(4).standard_normal((3, batch, shape.latent_dim)).astype(np.float32)
    port = TrainPort(init, lr=1e-3, weight_decay=1e-4)
    a = VAETrainer(shape, batch_size=batch, lr=1e-3, weight_decay=1e-4, state_dict=init)
    b = VAETrainer(shape, batch_size=batch, lr=1e-3, weight_decay=1e-4, state_dict=init)
    try:
        for s in range(3):
            ref = port.step(poses[s], eps[s], 0.02)
            la = a.step(poses[s], 0.02, eps=eps[s])
            lb = b.step(poses[s], 0.02, eps=eps[s], keep_gradients=False)
            np.testing.assert_allclose(lb, la, rtol=2e-6)
            np.testing.assert_allclose(lb, ref, rtol=1e-4)
    finally:
        a.close(); b.close()
