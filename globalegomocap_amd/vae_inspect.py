"""Looking at a trained motion VAE: reconstruct, sample, interpolate.

What the reference does with three small scripts that no longer run in its own tree -- `networks/get_latent.py` (sum mu^2 and
sum (sigma - 1)^2 of the encoded windows, before and after a pass through the VAE), `networks/sample.py` (prior draws decoded to
meshes) and `networks/interpolant.py` (two encoded windows and the latent points between them, decoded to folders of meshes) --
over the engine's encoder and decoder, with the part in between on the device: `gem_latent_report` keeps a table of per-window
errors and posterior statistics and the per-dimension sums of a whole pass in HBM until the pass is over, `gem_latent_paths` makes
the latent paths.  The files are `meshes.write_meshes`' and `render.write_frames`'.

    python -m globalegomocap_amd.vae_inspect reconstruct --checkpoint C --windows DIR|FILE.npy [--split test] [--posterior mean|sample]
                                                         [--refine] [--show K --out DIR] [--json FILE]
    python -m globalegomocap_amd.vae_inspect sample      --checkpoint C --num 12 --seed 0 --out DIR [--render] [--size WxH] [--view side|front|top]
    python -m globalegomocap_amd.vae_inspect interpolate --checkpoint C --windows ... --from I --to J [--steps 6] [--mode linear|spherical]
                                                         --out DIR [--render]

One difference from the reference is on purpose.  `sample.py` never calls `.eval()`, so its BatchNorm layers normalise every draw
with the statistics of the 12 samples drawn beside it: what it shows depends on how many it draws.  The engine folds BatchNorm's
running statistics into the weights, so everything here runs the network in eval mode -- the network the optimiser uses.
(`get_latent.py` and `interpolant.py` do call `.eval()`.)
"""
import json
import os

import numpy as np

REPORT_KEYS = ("mu_error", "std_error", "kld", "mpjpe", "max_joint_error")
REFINED_KEYS = ("refined_mu_error", "refined_std_error")
MODES = ("linear", "spherical")
POSTERIORS = ("mean", "sample")
SAMPLE_DIR, SAMPLE_FILE = "sample_{}", "{}.ply"          # sample.py:26,41
PATH_FILE = "out_%04d.ply"                               # interpolant.py:86; the folders are str(step), interpolant.py:117
WINDOW_DIR = "window_{}"
INPUT_RGB, RECONSTRUCTION_RGB = (44, 160, 44), (31, 119, 180)          # green, blue: render.PALETTE's gt and optimized


# ---------------------------------------------------------------------------------------------------- host arithmetic (no GPU)
def draw_latents(n, latent_dim, seed=0):
    """`ConvVAE.sample`'s draw (SeqConvVAE.py:229): torch.randn(n, D) on the CPU.  With the same seed it is the tensor
    `torch.manual_seed(seed); torch.randn(n, D)` gives."""
    import torch
    return torch.randn(int(n), int(latent_dim), generator=torch.Generator(device="cpu").manual_seed(int(seed)))


def draw_pair_eps(n_pairs, latent_dim, seed=0):
    """The reparameterisation noise of `interpolant.py:101-102`: eps for the first window(s), then for the second, from one CPU
    generator -> (eps_a, eps_b), each [n_pairs, D]."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    eps_a = torch.randn(int(n_pairs), int(latent_dim), generator=g)
    return eps_a, torch.randn(int(n_pairs), int(latent_dim), generator=g)


def sample_paths(out_dir, n_samples, seq_len):
    """sample.py:23-26,41: out_dir/sample_{i}/{j}.ply for frame j of draw i."""
    return [[os.path.join(out_dir, SAMPLE_DIR.format(i), SAMPLE_FILE.format(j)) for j in range(seq_len)] for i in range(n_samples)]


def interpolation_paths(out_dir, steps, seq_len):
    """interpolant.py:83-86,116-138: out_dir/{s}/out_%04d.ply for frame j of step s (0 and steps - 1 are the two windows)."""
    return [[os.path.join(out_dir, str(s), PATH_FILE % j) for j in range(seq_len)] for s in range(steps)]


class Report:
    """The outcome of a reconstruction pass.  `table` [N,5] float64 in the order of REPORT_KEYS ([N,7] with the re-encoded
    reconstruction's REFINED_KEYS behind them); `sums` [3,D] float64 = sum_n mu_d, sum_n mu_d^2, sum_n exp(logvar_d); `count` = N."""

    def __init__(self, table, sums, count):
        self.table = np.asarray(table, dtype=np.float64)
        self.sums = np.asarray(sums, dtype=np.float64)
        self.count = int(count)
        if self.table.ndim != 2 or self.table.shape[1] not in (5, 7) or self.sums.ndim != 2 or self.sums.shape[0] != 3:
            raise ValueError("a report is a [N,5] or [N,7] table and [3,D] sums, got %s and %s" % (self.table.shape, self.sums.shape))
        if self.count < 1:
            raise ValueError("a report covers at least one window")

    @property
    def keys(self):
        return REPORT_KEYS + (REFINED_KEYS if self.table.shape[1] == 7 else ())

    def column(self, key):
        return self.table[:, self.keys.index(key)]

    @property
    def means(self):
        """The data set's mean of every column: per window what get_latent.py:57-65 prints per batch, train.py:127-129's MPJPE."""
        return {k: float(self.table[:, i].mean()) for i, k in enumerate(self.keys)}

    @property
    def mean_mu(self):
        return self.sums[0] / self.count

    @property
    def var_mu(self):
        """Var_n[mu_d] = E[mu_d^2] - E[mu_d]^2 (the population variance; never below zero)."""
        m = self.sums[0] / self.count
        return np.maximum(self.sums[1] / self.count - m * m, 0.0)

    @property
    def mean_var(self):
        """E_n[sigma_d^2]: 1 for a dimension that has collapsed onto the prior."""
        return self.sums[2] / self.count

    def active_units(self, threshold=0.01):
        """The number of latent dimensions whose posterior mean moves with the input, Var_n[mu_d] > threshold (Burda et al. 2016)."""
        return int((self.var_mu > threshold).sum())

    def worst(self, k=10):
        """The ids of the k windows with the largest mpjpe, worst first (NaN before everything; ties by id)."""
        e = self.column("mpjpe")
        key = np.where(np.isnan(e), np.inf, e)
        return [int(i) for i in np.argsort(-key, kind="stable")[:max(0, int(k))]]

    def to_json(self):
        return json.dumps({"count": self.count, "keys": list(self.keys), "table": self.table.tolist(), "sums": self.sums.tolist(),
                           "means": self.means, "active_units": self.active_units(), "latent_dim": int(self.sums.shape[1])})

    @classmethod
    def from_json(cls, text):
        d = json.loads(text)
        return cls(np.array(d["table"], dtype=np.float64).reshape(-1, len(d["keys"])), d["sums"], d["count"])

    def lines(self, show=0):
        """What the command prints: the reference's lines (get_latent.py:57-58,64-65; means per window), then the rest."""
        m = self.means
        out = ["mu error is: {}".format(m["mu_error"]), "std error is: {}".format(m["std_error"])]
        if "refined_mu_error" in m:
            out += ["vae refined mu error is: {}".format(m["refined_mu_error"]), "vae refined std error is: {}".format(m["refined_std_error"])]
        out += ["mpjpe is: {}".format(m["mpjpe"]), "kld is: {}".format(m["kld"]),
                "active units: {} of {}".format(self.active_units(), self.sums.shape[1])]
        e, far = self.column("mpjpe"), self.column("max_joint_error")
        out += ["window {}: mpjpe {} max joint error {}".format(i, e[i], far[i]) for i in self.worst(show)]
        return out


def infer_checkpoint_shape(state):
    """`vae.infer_shape` with the window length read off fc_mu (flat = hidden[-1] * seq_len)."""
    from .vae import infer_shape, _np
    i = 0
    while ("encoder.%d.0.weight" % (i + 1)) in state:
        i += 1
    if "encoder.0.0.weight" not in state or "fc_mu.weight" not in state:
        raise KeyError("state_dict has no 'encoder.0.0.weight' / 'fc_mu.weight': not a ConvVAE checkpoint")
    top, flat = int(_np(state["encoder.%d.0.weight" % i]).shape[0]), int(_np(state["fc_mu.weight"]).shape[1])
    return infer_shape(state, seq_len=max(1, flat // top))


# ---------------------------------------------------------------------------------------------------- the device path
class Inspector:
    """A trained VAE (a state_dict in the reference's schema, or the path of a checkpoint) behind an engine, in eval mode."""

    def __init__(self, state_dict_or_checkpoint_path, shape=None, max_windows=256, device=None, trust=None):
        from . import vae
        from .engine import WindowEngine
        state = state_dict_or_checkpoint_path
        if isinstance(state, (str, os.PathLike)):
            state = vae.load_checkpoint(os.fspath(state), trust)
        state = {k: vae._np(v) for k, v in state.items()}
        self.shape = shape or infer_checkpoint_shape(state)
        self.engine = WindowEngine(self.shape, max_windows=int(max_windows), device=device)
        self.engine.load_vae(0, state)
        self.device, self.max_windows = self.engine.device, int(max_windows)
        self.T, self.D = self.shape.seq_len, self.shape.latent_dim
        self._samples = self._paths = self._windows = None

    def close(self):
        self.engine.close()

    # ---- batches
    def _source(self, windows):
        """(n, take(lo, hi) -> [hi - lo, T, 45] f32 on the device, pick(ids) likewise) of a MotionWindows or an [N,T,45] array."""
        import torch
        from .motion_data import MotionWindows
        if isinstance(windows, MotionWindows):
            if windows.seq_len != self.T:
                raise ValueError("the MotionWindows cut windows of %d frames; this VAE takes %d" % (windows.seq_len, self.T))
            windows.upload(self.device)
            if windows.device != self.device:
                raise ValueError("the MotionWindows live on %s; this VAE on %s" % (windows.device, self.device))
            return (len(windows), lambda lo, hi: windows.batch(torch.arange(lo, hi, dtype=torch.int64, device=self.device)),
                    lambda ids: windows.batch(torch.as_tensor(ids, dtype=torch.int64)))
        data = torch.as_tensor(np.asarray(windows.cpu() if torch.is_tensor(windows) else windows), dtype=torch.float32)
        if data.dim() == 2:
            data = data[None]
        if data.dim() == 4:
            data = data.reshape(data.shape[0], data.shape[1], -1)
        if data.dim() != 3 or tuple(data.shape[1:]) != (self.T, self.shape.channels):
            raise ValueError("windows must be [N,%d,%d], got %s" % (self.T, self.shape.channels, tuple(data.shape)))
        return (int(data.shape[0]), lambda lo, hi: data[lo:hi].to(self.device),
                lambda ids: data[torch.as_tensor(ids, dtype=torch.int64)].to(self.device))

    def _decode(self, z):
        """decode over any number of latents, max_windows at a time -> [n,T,15,3] f32 on the device."""
        import torch
        z = z.reshape(-1, self.D)
        if z.shape[0] <= self.max_windows:
            return self.engine.decode(0, z)
        return torch.cat([self.engine.decode(0, z[i:i + self.max_windows]) for i in range(0, z.shape[0], self.max_windows)])

    def _encode(self, x, eps=None):
        import torch
        if x.shape[0] <= self.max_windows:
            return self.engine.encode(0, x, eps)
        parts = [self.engine.encode(0, x[i:i + self.max_windows], None if eps is None else eps[i:i + self.max_windows])
                 for i in range(0, x.shape[0], self.max_windows)]
        return tuple(torch.cat([p[k] for p in parts]) for k in range(3))

    # ---- reconstruct
    def reconstruct(self, windows, batch_size=None, posterior="mean", seed=0, refine=False):
        """Every window through encode -> decode -> latent_report: a `Report`.  windows: a `motion_data.MotionWindows` or an
        [N,T,45] array (what `VAETrainer.evaluate` takes).  posterior "mean" decodes mu; "sample" decodes mu + eps * sigma with eps
        drawn per batch from a CPU generator seeded with `seed`.  refine: the reconstruction is encoded again and its mu_error /
        std_error fill two more columns (get_latent.py:62-65).  The table and the per-dimension sums stay on the device until the
        last batch is enqueued; then they are read back once."""
        import torch
        if posterior not in POSTERIORS:
            raise ValueError("posterior must be one of %s, got %r" % (POSTERIORS, posterior))
        bs = int(batch_size or self.max_windows)
        if not 1 <= bs <= self.max_windows:
            raise ValueError("batch_size must be 1 .. max_windows = %d, got %d" % (self.max_windows, bs))
        n, take, _ = self._source(windows)
        if n < 1:
            raise ValueError("no windows")
        eng, dev = self.engine, self.device
        with torch.cuda.device(dev):
            table = torch.empty(n, 5, device=dev, dtype=torch.float64)
            extra = torch.empty(n, 2, device=dev, dtype=torch.float64) if refine else None
            cols = torch.zeros(3, self.D, device=dev, dtype=torch.float64)
            count = torch.zeros(1, device=dev, dtype=torch.int64)
            g = torch.Generator(device="cpu").manual_seed(int(seed))
            for lo in range(0, n, bs):
                hi = min(lo + bs, n)
                x = take(lo, hi)
                eps = torch.randn(hi - lo, self.D, generator=g).to(dev) if posterior == "sample" else None
                mu, logvar, z = eng.encode(0, x, eps)
                rec = eng.decode(0, z)
                eng.latent_report(mu, logvar, x, rec, cols=cols, count=count, out=table[lo:hi])
                if refine:
                    mu2, logvar2, _ = eng.encode(0, rec.reshape(hi - lo, self.T, -1))
                    extra[lo:hi] = eng.latent_report(mu2, logvar2)[:, :2]
            flat = torch.cat([t.reshape(-1) for t in ([table] + ([extra] if refine else []) + [cols, count.to(torch.float64)])]).cpu().numpy()
        self._windows = windows
        tab = flat[:n * 5].reshape(n, 5)
        at = n * 5
        if refine:
            tab = np.concatenate([tab, flat[at:at + 2 * n].reshape(n, 2)], axis=1)
            at += 2 * n
        return Report(tab, flat[at:at + 3 * self.D].reshape(3, self.D), int(flat[-1]))

    # ---- sample
    def sample(self, n, seed=0):
        """n draws from the prior, decoded: (z [n,D] f32, poses [n,T,15,3] f32) on the device.  z is `draw_latents`' tensor:
        drawn on the CPU and moved, as ConvVAE.sample draws it."""
        import torch
        with torch.cuda.device(self.device):
            z = draw_latents(n, self.D, seed).to(self.device)
            poses = self._decode(z)
        self._samples = poses
        return z, poses

    # ---- interpolate
    def interpolate(self, window_a, window_b, steps=6, mode="linear", posterior="sample", seed=0):
        """The two windows encoded (interpolant.py:101-102: posterior "sample" draws eps for a, then for b, from one CPU
        generator; "mean" takes mu), `steps` latent points from one to the other (`WindowEngine.latent_paths`), all decoded at
        once: (z [steps,D], poses [steps,T,15,3]) on the device for two windows [T,45]; P pairs at once -- [P,T,45] each --
        give (z [P,steps,D], poses [P,steps,T,15,3])."""
        import torch
        if posterior not in POSTERIORS:
            raise ValueError("posterior must be one of %s, got %r" % (POSTERIORS, posterior))
        if mode not in MODES:
            raise ValueError("mode must be one of %s, got %r" % (MODES, mode))
        if int(steps) < 2:
            raise ValueError("a path has at least its two end points (steps >= 2), got %d" % steps)
        with torch.cuda.device(self.device):
            a, b = (torch.as_tensor(np.asarray(w.cpu() if torch.is_tensor(w) else w), dtype=torch.float32) for w in (window_a, window_b))
            single = a.dim() == 2 or (a.dim() == 3 and a.shape[-1] == 3)
            a, b = (w.reshape(-1, self.T, self.shape.channels).to(self.device) for w in (a, b))
            if a.shape != b.shape:
                raise ValueError("the two ends must hold the same number of windows, got %d and %d" % (a.shape[0], b.shape[0]))
            P = a.shape[0]
            eps_a, eps_b = draw_pair_eps(P, self.D, seed) if posterior == "sample" else (None, None)
            za = self._encode(a, None if eps_a is None else eps_a.to(self.device))[2]
            zb = self._encode(b, None if eps_b is None else eps_b.to(self.device))[2]
            z = self.engine.latent_paths(za, zb, int(steps), mode)
            poses = self._decode(z).reshape(P, int(steps), self.T, -1, 3)
        self._paths = poses
        return (z[0], poses[0]) if single else (z, poses)

    # ---- files
    def _render(self, sequences, folder, colours, names, size, view):
        from . import render
        return render.write_frames(self.engine, sequences, folder, colours=colours, size=size or render.DEFAULT_SIZE, view=view, names=names)

    def write_samples(self, out_dir, poses=None, render=False, size=None, view="side"):
        """out_dir/sample_{i}/{j}.ply for frame j of draw i (sample.py:23-26,41) of the last `sample` call (or `poses` [n,T,15,3]);
        render: also frame_%04d.png and one overview per folder.  Returns the number of files."""
        from . import meshes
        poses = self._samples if poses is None else poses
        if poses is None:
            raise ValueError("write_samples: call sample() first, or pass poses")
        files = 0
        for i in range(poses.shape[0]):
            folder = os.path.join(out_dir, SAMPLE_DIR.format(i))
            files += meshes.write_meshes(self.engine, poses[i], folder, pattern=SAMPLE_FILE.replace("{}", "%d"))
            if render:
                files += self._render([poses[i]], folder, [RECONSTRUCTION_RGB], ["sample"], size, view)
        return files

    def write_interpolation(self, out_dir, poses=None, render=False, size=None, view="side"):
        """out_dir/{s}/out_%04d.ply for step s = 0 .. steps-1 (interpolant.py:83-86,116-138) of the last `interpolate` call (or
        `poses` [steps,T,15,3]); P pairs go to out_dir/pair_{p}/{s}/.  render: also frame_%04d.png and one overview per folder."""
        from . import meshes
        poses = self._paths if poses is None else poses
        if poses is None:
            raise ValueError("write_interpolation: call interpolate() first, or pass poses")
        if poses.dim() == 4:
            poses = poses[None]
        files = 0
        for p in range(poses.shape[0]):
            root = out_dir if poses.shape[0] == 1 else os.path.join(out_dir, "pair_{}".format(p))
            for s in range(poses.shape[1]):
                folder = os.path.join(root, str(s))
                files += meshes.write_meshes(self.engine, poses[p, s], folder, pattern=PATH_FILE)
                if render:
                    files += self._render([poses[p, s]], folder, [RECONSTRUCTION_RGB], ["step"], size, view)
        return files

    def write_reconstructions(self, ids, out_dir, windows=None, size=None, view="side"):
        """out_dir/window_{id}/frame_%04d.png (and one overview per sequence) for the windows `ids` of the last `reconstruct` call's
        data (or of `windows`): the input in green and the reconstruction of its posterior mean in blue, in the same frames."""
        import torch
        windows = self._windows if windows is None else windows
        if windows is None:
            raise ValueError("write_reconstructions: call reconstruct() first, or pass windows")
        ids = [int(i) for i in ids]
        if not ids:
            return 0
        n, _, pick = self._source(windows)
        if min(ids) < 0 or max(ids) >= n:
            raise IndexError("window id out of range [0, %d)" % n)
        with torch.cuda.device(self.device):
            x = pick(ids)
            rec = self._decode(self._encode(x)[0])
            x = x.reshape(len(ids), self.T, -1, 3)
            return sum(self._render([x[k], rec[k]], os.path.join(out_dir, WINDOW_DIR.format(i)), [INPUT_RGB, RECONSTRUCTION_RGB],
                                    ["input", "reconstruction"], size, view) for k, i in enumerate(ids))


# ---------------------------------------------------------------------------------------------------- command line
DATASET_FLAGS = ("poses", "seq_names", "with_mo2cap2_data", "data_balance", "slide_window_step", "seq_length", "fps")


def _steps(text):
    import argparse
    try:
        n = int(text)
    except ValueError:
        n = 0
    if n < 2:
        raise argparse.ArgumentTypeError("a path has at least its two end points: --steps >= 2, got %r" % text)
    return n


def _parser():
    import argparse
    import copy
    from . import render, vae_train
    p = argparse.ArgumentParser(prog="python -m globalegomocap_amd.vae_inspect",
                                description="Look at a trained motion VAE on MI355X: reconstruct, sample, interpolate")
    sub = p.add_subparsers(dest="command", required=True)
    dataset = [a for a in vae_train._parser()._actions if a.dest in DATASET_FLAGS]          # vae_train's own flags, not copies of their text

    def common(q, windows):
        q.add_argument("--checkpoint", required=True, help="a checkpoint of vae_train (or of the reference's networks/train.py)")
        q.add_argument("--max_windows", type=int, default=256, help="windows per batch")
        q.add_argument("--trust", action="store_true", help="read a checkpoint or pickles the restricted unpickler refuses")
        if windows:
            q.add_argument("--windows", required=True, metavar="DIR|FILE.npy",
                           help="directory of motion pickles, or a .npy / .npz ('windows') of [n, seq_length, 45] windows")
            q.add_argument("--split", default="test", choices=("train", "test", "all"), help="from a directory: which files")
            for a in dataset:
                a = copy.copy(a)
                a.required = False
                if a.dest == "seq_length":
                    a.default, a.help = None, "from a directory: frames per window (default: the checkpoint's)"
                q._add_action(a)

    def pictures(q):
        q.add_argument("--render", action="store_true", help="also frame_%%04d.png and one overview per folder")
        q.add_argument("--size", default=None, type=render._size, metavar="WxH", help="default 640x480")
        q.add_argument("--view", default="side", choices=render.VIEWS)

    q = sub.add_parser("reconstruct", help="per-window errors and posterior statistics of a data set (get_latent.py)")
    common(q, True)
    q.add_argument("--posterior", default="mean", choices=POSTERIORS)
    q.add_argument("--seed", type=int, default=0)
    q.add_argument("--refine", action="store_true", help="also the statistics of the re-encoded reconstruction")
    q.add_argument("--show", type=int, default=0, metavar="K", help="list the K worst windows (and draw them with --out)")
    q.add_argument("--out", default=None, metavar="DIR")
    q.add_argument("--json", default=None, metavar="FILE")
    q.add_argument("--size", default=None, type=render._size, metavar="WxH", help="default 640x480")
    q.add_argument("--view", default="side", choices=render.VIEWS)
    q = sub.add_parser("sample", help="prior draws decoded to meshes (sample.py)")
    common(q, False)
    q.add_argument("--num", type=int, default=12)
    q.add_argument("--seed", type=int, default=0)
    q.add_argument("--out", required=True, metavar="DIR")
    pictures(q)
    q = sub.add_parser("interpolate", help="two windows and the latent points between them, decoded to meshes (interpolant.py)")
    common(q, True)
    q.add_argument("--from", dest="first", type=int, required=True, metavar="I")
    q.add_argument("--to", dest="second", type=int, required=True, metavar="J")
    q.add_argument("--steps", type=_steps, default=6)
    q.add_argument("--mode", default="linear", choices=MODES)
    q.add_argument("--posterior", default="sample", choices=POSTERIORS)
    q.add_argument("--seed", type=int, default=0)
    q.add_argument("--out", required=True, metavar="DIR")
    pictures(q)
    return p


def _load_windows(a, seq_len, parser):
    from .motion_data import MotionWindows
    if os.path.isdir(a.windows):
        if a.with_mo2cap2_data and not a.seq_names:
            parser.error("--with_mo2cap2_data True needs --seq_names PATH")
        ds = MotionWindows.from_directory(a.windows, poses=a.poses, frame_num=a.seq_length or seq_len, windows_size=a.slide_window_step,
                                          fps=a.fps, slide_window=True, split=a.split, balance=a.data_balance,
                                          seq_names=a.seq_names if a.with_mo2cap2_data else None, seed=0, device="cpu", trust=a.trust)
        if ds.seq_len != seq_len:
            parser.error("%s cuts windows of %d frames, but the checkpoint takes %d" % (a.windows, ds.seq_len, seq_len))
        return ds
    d = np.load(a.windows)
    return np.asarray(d["windows"] if hasattr(d, "files") else d, np.float32).reshape(-1, seq_len, 45)


def main(argv=None):
    p = _parser()
    a = p.parse_args(argv)
    ins = Inspector(a.checkpoint, max_windows=a.max_windows, trust=a.trust or None)
    try:
        if a.command == "sample":
            if a.num < 1:
                p.error("--num must be at least 1")
            ins.sample(a.num, a.seed)
            print("{} files written under {}".format(ins.write_samples(a.out, render=a.render, size=a.size, view=a.view), a.out))
            return
        windows = _load_windows(a, ins.T, p)
        if a.command == "reconstruct":
            if a.show < 0:
                p.error("--show must not be negative")
            rep = ins.reconstruct(windows, posterior=a.posterior, seed=a.seed, refine=a.refine)
            for line in rep.lines(a.show):
                print(line)
            if a.json:
                with open(a.json, "w") as f:
                    f.write(rep.to_json())
            if a.out is not None and a.show > 0:
                print("{} images written under {}".format(ins.write_reconstructions(rep.worst(a.show), a.out, size=a.size, view=a.view), a.out))
            return
        n, _, pick = ins._source(windows)
        for i in (a.first, a.second):
            if not 0 <= i < n:
                p.error("window %d is not one of the %d windows" % (i, n))
        pair = pick([a.first, a.second])
        ins.interpolate(pair[0], pair[1], steps=a.steps, mode=a.mode, posterior=a.posterior, seed=a.seed)
        print("{} files written under {}".format(ins.write_interpolation(a.out, render=a.render, size=a.size, view=a.view), a.out))
    finally:
        ins.close()


if __name__ == "__main__":
    main()
