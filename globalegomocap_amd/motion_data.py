"""Training windows of the motion VAEs from a directory of motion pickles.

The reference's `AMASSDataset` (networks/dataset/global_dataset.py:12-110 for the global VAE, local_dataset.py:15-98 for the
camera-frame one) cuts every sliding window out of every sequence on the host and keeps them all as one float64 array.  Here the
source frames are packed into one float64 arena, uploaded once, and a batch of windows is cut on the device by
`gem_motion_windows` straight into the trainer's input buffer; the cameras are converted once by `gem_motion_cameras`.

File selection (`select_files`) and window counting are pure host functions of the directory listing and the files' lengths;
`MotionWindows.windows_numpy` is a float64 host twin in the reference's own operation order, kept as the tests' CPU reference.
There is no host fallback for `batch` / `materialize`.
"""
import ctypes as C
import io
import os
import pickle

import numpy as np

N_JOINTS = 15
TRUST_ENV = "GEM_TRUST_CHECKPOINTS"          # the switch of vae.load_checkpoint_file


# ------------------------------------------------------------------------------------------------------------------ reading files
def _allowed_globals():
    from .vae import numpy_pickle_globals
    out = {"_codecs.encode": __import__("codecs").encode}      # (how protocol 2 writes bytes: an ndarray's raw data)
    for a in numpy_pickle_globals():
        obj, name = a if isinstance(a, tuple) else (a, "%s.%s" % (a.__module__, a.__qualname__))
        out[name] = obj
    # protocol 5 rebuilds an ndarray through numeric._frombuffer(bytes, dtype, shape, order), under either numpy generation's path
    numeric = getattr(getattr(np, "_core", None), "numeric", None) or np.core.numeric
    if hasattr(numeric, "_frombuffer"):
        for mod in ("numpy.core.numeric", "numpy._core.numeric"):
            out[mod + "._frombuffer"] = numeric._frombuffer
    return out


class _RestrictedUnpickler(pickle.Unpickler):
    """Builtin containers and primitives (opcodes, no globals) plus numpy arrays, dtypes and scalars: any other global is refused
    before it is looked up, so nothing else is constructed."""

    def __init__(self, f, allowed):
        super().__init__(f)
        self._allowed = allowed

    def find_class(self, module, name):
        obj = self._allowed.get("%s.%s" % (module, name))
        if obj is None:
            raise pickle.UnpicklingError("global '%s.%s' is not allowed" % (module, name))
        return obj


def read_motion_pickle(path, trust=None):
    """The dict of one motion pickle through a restricted unpickler (numpy arrays / scalars and builtin containers only).  A file
    that needs anything else is refused unless trust=True or GEM_TRUST_CHECKPOINTS=1."""
    if trust is None:
        trust = os.environ.get(TRUST_ENV) == "1"
    with open(path, "rb") as f:
        raw = f.read()
    try:
        return _RestrictedUnpickler(io.BytesIO(raw), _allowed_globals()).load()
    except pickle.UnpicklingError as e:
        if not trust:
            raise pickle.UnpicklingError("%s holds objects the restricted unpickler refuses (%s); pass trust=True / set %s=1 only "
                                         "for files whose origin you trust" % (path, str(e).splitlines()[0], TRUST_ENV)) from e
    return pickle.loads(raw)


def select_files(listing, split="train", seq_names=None, balance=False, rng=None):
    """`load_pkls`' choice of files (global_dataset.py:43-74) as a pure function of the `os.listdir` listing: with `seq_names`
    every file whose name contains a name, once per matching name (duplicates possible) and in the names' order; train = [:-10],
    test = [-10:], all = everything; `balance` keeps the non-walking files and int(len(non_walking) / 20) of the shuffled walking
    ones after them (the reference's shuffle is unseeded; here `rng`, a numpy.random.Generator, default seed 0)."""
    names = list(listing)
    if seq_names is not None:
        names = [p for s in seq_names for p in listing if s in p]
    if split == "train":
        names = names[:-10]
    elif split == "test":
        names = names[-10:]
    elif split != "all":
        raise ValueError("split must be 'train', 'test' or 'all', not %r" % (split,))
    if balance:
        walking = [p for p in names if "walk" in p.lower()]
        others = [p for p in names if "walk" not in p.lower()]
        (rng if rng is not None else np.random.default_rng(0)).shuffle(walking)
        names = others + walking[:int(1 / 20 * len(others))]
    return names


def frame_rate_timer(frame_rate, fps):
    """round(int(frame_rate) / fps) with Python's round (halves to even: 75 fps at 30 gives 2); 0 is refused, as the reference's
    slice step 0 raises."""
    t = round(int(frame_rate) / fps)
    if t == 0:
        raise ValueError("frame rate %r at fps %r gives a frame step of 0 (round(int(frame_rate) / fps))" % (frame_rate, fps))
    return int(t)


def window_count(n_frames, total, timer, interval):
    """len(range(0, n_frames - total * timer, interval)): the window ending on the last frame is never cut."""
    return len(range(0, n_frames - total * timer, interval))


def sequence_arrays(data, need_cameras, name="sequence"):
    """poses [L,15,3] float64, loc [L,3], quat [L,4] (None without cameras) and the frame rate of one pickle's dict; only
    `local_pose_list`, `cam_list` and `frame_rate` are read."""
    if not isinstance(data, dict) or "local_pose_list" not in data or "frame_rate" not in data:
        raise ValueError("%s: not a motion pickle (a dict with 'local_pose_list', 'cam_list' and 'frame_rate')" % name)
    plist = data["local_pose_list"]
    poses = np.empty((len(plist), N_JOINTS, 3), np.float64)
    for i, p in enumerate(plist):
        a = np.asarray(p)
        if a.shape != (N_JOINTS, 3):
            raise ValueError("%s: local_pose_list[%d] has shape %s, expected (15, 3)" % (name, i, a.shape))
        poses[i] = a
    loc = quat = None
    if need_cameras:
        if "cam_list" not in data:
            raise ValueError("%s: no 'cam_list' (global windows need the cameras)" % name)
        cams = data["cam_list"]
        if len(cams) != len(plist):
            raise ValueError("%s: %d cameras for %d poses" % (name, len(cams), len(plist)))
        loc = np.empty((len(cams), 3), np.float64)
        quat = np.empty((len(cams), 4), np.float64)
        for i, c in enumerate(cams):
            lo, ro = np.asarray(c["loc"], np.float64), np.asarray(c["rot"], np.float64)
            if lo.shape != (3,) or ro.shape != (4,):
                raise ValueError("%s: cam_list[%d] has loc %s / rot %s, expected (3,) / (4,)" % (name, i, lo.shape, ro.shape))
            loc[i], quat[i] = lo, ro
        if len(quat) and not (np.einsum("ij,ij->i", quat, quat) > 0).all():
            raise ValueError("%s: a camera quaternion has zero norm (scipy's from_quat refuses it)" % name)
    return poses, loc, quat, data["frame_rate"]


def camera_matrices_numpy(loc, quat):
    """[n,4,4] float64 = trans_qrot_to_matrix (utils/utils.py:33-42): scipy's Rotation.from_quat(quat).as_matrix() in scipy's own
    operation order (normalised first), loc as the last column, [0, 0, 0, 1] below."""
    q = np.asarray(quat, np.float64)
    nrm = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    x, y, z, w = (q[:, k] / nrm for k in range(4))
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    m = np.zeros((len(q), 4, 4), np.float64)
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw)
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = 2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw)
    m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = 2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2
    m[:, :3, 3] = loc
    m[:, 3, 3] = 1.0
    return m


# ------------------------------------------------------------------------------------------------------------------ the dataset
class MotionWindows:
    """Every window of a set of motion sequences, cut on the device.  `len(ds)` windows of [seq_len, 45] float32: global windows
    (poses="global", seq_len = frame_num) or camera-frame ones (poses="local", seq_len = frame_num * windows_size, the local
    dataset's quirk).  Window ids run over the sequences in file order, and within a sequence over the start frames
    0, interval, 2 * interval, ... (the reference's order)."""

    def __init__(self, sequences, poses="global", frame_num=10, windows_size=1, fps=25, slide_window=True, device=None, names=None):
        """sequences: [(poses [L,15,3], loc [L,3] or None, quat [L,4] or None, frame_rate), ...] as sequence_arrays returns them."""
        import torch
        if poses not in ("global", "local"):
            raise ValueError("poses must be 'global' or 'local', not %r" % (poses,))
        self.poses, self.frame_num, self.windows_size, self.fps = poses, int(frame_num), int(windows_size), fps
        if self.frame_num < 1 or self.windows_size < 1:
            raise ValueError("frame_num and windows_size must be >= 1")
        self.slide_window = bool(slide_window)
        self.total = self.frame_num * self.windows_size
        self.seq_len = self.frame_num if poses == "global" else self.total
        self.names = list(names) if names is not None else None
        S = len(sequences)
        if S == 0:
            raise ValueError("no sequences")
        self.timers = np.array([frame_rate_timer(s[3], fps) for s in sequences], np.int32)
        lengths = np.array([len(s[0]) for s in sequences], np.int64)
        # interval: 1 (slide_window) or total * timer of each sequence (the kernel's interval 0)
        self.interval = 1 if self.slide_window else 0
        self.seq_interval = np.ones(S, np.int64) if self.slide_window else self.total * self.timers.astype(np.int64)
        counts = np.array([window_count(int(L), self.total, int(t), int(iv))
                           for L, t, iv in zip(lengths, self.timers, self.seq_interval)], np.int64)
        self.lengths, self.counts = lengths, counts
        self.frame0 = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        self.window0 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.pose_host = np.concatenate([s[0] for s in sequences]).astype(np.float64, copy=False).reshape(-1, N_JOINTS, 3)
        if poses == "global":
            self.loc_host = np.concatenate([s[1] for s in sequences]).astype(np.float64, copy=False).reshape(-1, 3)
            self.quat_host = np.concatenate([s[2] for s in sequences]).astype(np.float64, copy=False).reshape(-1, 4)
        else:
            self.loc_host = self.quat_host = None
        self.d_pose = self.d_cam = None
        self.device = torch.device("cpu")
        if not (isinstance(device, str) and device == "cpu"):      # (device "cpu": host side only until upload(); batch refuses)
            self.upload(device)

    def upload(self, device=None):
        """Put the frame arena (and, for global windows, the cameras converted by gem_motion_cameras) on `device` (default the
        current CUDA device), once; returns self."""
        import torch
        from . import _capi
        if self.d_pose is not None:
            return self
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.lib = _capi.load_library()
        self.d_pose = torch.from_numpy(np.ascontiguousarray(self.pose_host)).to(dev)
        self.d_frame0 = torch.from_numpy(self.frame0).to(dev)
        self.d_window0 = torch.from_numpy(self.window0).to(dev)
        self.d_timer = torch.from_numpy(self.timers).to(dev)
        self.d_cam = None
        if self.poses == "global":
            loc = torch.from_numpy(np.ascontiguousarray(self.loc_host)).to(dev)
            quat = torch.from_numpy(np.ascontiguousarray(self.quat_host)).to(dev)
            self.d_cam = torch.empty((len(loc), 3, 4), dtype=torch.float64, device=dev)
            with torch.cuda.device(dev):
                s = torch.cuda.current_stream(dev).cuda_stream
                _capi.check(self.lib.gem_motion_cameras(loc.data_ptr(), quat.data_ptr(), len(loc), self.d_cam.data_ptr(), C.c_void_p(s)),
                            self.lib)
            # (loc / quat are freed when the stream has passed the conversion: torch's caching allocator orders reuse on the stream)
        return self

    @classmethod
    def from_directory(cls, path, poses="global", frame_num=10, windows_size=1, fps=25, slide_window=True, split="train", balance=False,
                       seq_names=None, seed=0, device=None, trust=False):
        """The reference's AMASSDataset(data_path=path, frame_num, windows_size, is_train=split == 'train', fps, slide_window,
        balance_distrib=balance, with_mo2cap2_data=seq_names is not None): the files of `select_files(os.listdir(path), ...)`,
        read through the restricted unpickler.  seq_names: a list of names or the path of a .npy holding them (the reference's
        seq_names.npy).  device: a CUDA device (default the current one) or "cpu" for the host side only."""
        if isinstance(seq_names, str):
            seq_names = np.load(seq_names).tolist()
        chosen = select_files(os.listdir(path), split, seq_names, balance, np.random.default_rng(seed))
        if not chosen:
            raise ValueError("%s: no files selected (split %r of %d files)" % (path, split, len(os.listdir(path))))
        seqs = []
        for name in chosen:
            data = read_motion_pickle(os.path.join(path, name), trust=trust or None)
            seqs.append(sequence_arrays(data, poses == "global", name))
        return cls(seqs, poses, frame_num, windows_size, fps, slide_window, device, names=chosen)

    def __len__(self):
        return int(self.window0[-1])

    @property
    def n_frames(self):
        return int(self.lengths.sum())

    def batch(self, ids, out=None):
        """Windows `ids` (int64, any length; a device tensor is used in place) -> [B, seq_len, 45] float32 on the device, enqueued on
        the current stream without a host synchronisation.  An id outside [0, len(self)) gives NaN rows."""
        import torch
        from . import _capi
        if self.d_pose is None:
            raise RuntimeError("this MotionWindows was made with device='cpu': windows are cut on the GPU only (windows_numpy is the "
                               "host reference)")
        ids = torch.as_tensor(ids, dtype=torch.int64).to(self.device).contiguous()
        if ids.dim() != 1:
            raise ValueError("ids must be one-dimensional")
        B = int(ids.shape[0])
        shape = (B, self.seq_len, 3 * N_JOINTS)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor of shape %s on %s" % (shape, self.device))
        s = torch.cuda.current_stream(self.device).cuda_stream
        cam = self.d_cam.data_ptr() if self.d_cam is not None else None
        _capi.check(self.lib.gem_motion_windows(self.d_pose.data_ptr(), cam, self.d_frame0.data_ptr(), self.d_window0.data_ptr(),
                                                self.d_timer.data_ptr(), len(self.timers), self.interval, self.frame_num,
                                                self.windows_size, ids.data_ptr(), B, out.data_ptr(), C.c_void_p(s)), self.lib)
        return out

    def materialize(self):
        """Every window, [len, seq_len, 45] float32 on the device (one launch)."""
        import torch
        return self.batch(torch.arange(len(self), dtype=torch.int64, device=self.device))

    def locate(self, ids):
        """(sequence, first frame within it) of every window id (host)."""
        ids = np.asarray(ids, np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= len(self)):
            raise IndexError("window id out of range [0, %d)" % len(self))
        s = np.searchsorted(self.window0, ids, side="right") - 1
        return s, (ids - self.window0[s]) * self.seq_interval[s]

    def windows_numpy(self, ids):
        """Host float64 twin of `batch` in the reference's operation order (trans_qrot_to_matrix, np.linalg.inv, .dot, transform_pose
        of utils/utils.py:33-97; the window's frames i + k * timer, every windows_size-th kept), returned as float32 like
        `__getitem__`'s .float().  The tests' CPU reference, not a fallback."""
        seq, start = self.locate(ids)
        out = np.empty((len(seq), self.seq_len, 3 * N_JOINTS), np.float32)
        for n, (s, i) in enumerate(zip(seq, start)):
            f = self.frame0[s] + i + np.arange(self.total) * int(self.timers[s])
            if self.poses == "local":
                out[n] = self.pose_host[f].reshape(self.seq_len, -1)
                continue
            cams = camera_matrices_numpy(self.loc_host[f], self.quat_host[f])
            inv0 = np.linalg.inv(cams[0])
            frames = []
            for k in range(0, self.total, self.windows_size):
                m = inv0.dot(cams[k])
                homo = np.concatenate([self.pose_host[f[k]], np.ones((N_JOINTS, 1))], axis=1)
                frames.append(m.dot(homo.T).T[:, :3])
            out[n] = np.asarray(frames).reshape(self.seq_len, -1)
        return out
