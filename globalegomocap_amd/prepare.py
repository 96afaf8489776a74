"""Recordings from the pose network's .mat files: the reference's `MakeDataForOptimization/process_test_data.py` on the device.

The pose network leaves one `heatmap` .mat ([64,64,15]) and one `depth` .mat ([1,15]) per frame.  The reference walks them
frame by frame (loadmat, a 1024 x 1280 x 15 upscale, argmax, un-projection), fits the SLAM scale against the ground truth and
pickles five lists per 100-frame chunk.  Here the files of all chunks go as they are into one block of pinned memory and
from there into HBM (`gem_mat_read`: the library reads and interprets them, no Python object per array), ONE kernel picks
heat-maps and depths out (`gem_mat_frames`), the existing lifting kernel gives `estimated_local_skeleton`, the host fits
the scale per chunk from the head joints alone (`slam.camera_pose_list_from_heads`) and one more kernel applies the scaled
cameras (`gem_prepare_global`).  The result is a `Recording` on the device that `whole_sequence.optimize_recording` consumes
directly; `Recording.write_chunks` writes the reference's `data_start_{a}_end_{b}/test_data.pkl` files when they are wanted.

The reference's quirks are kept (process_test_data.py line numbers):

  * frame files are `natsorted(os.listdir(dir))[start_frame:end_frame]` (:52-53): an index into the LISTING, not a frame id;
  * ground truth is `pose_gt[i - mat_start_frame]` for i in range(start_frame, end_frame) (:44-45), passed through untouched;
  * trajectory lines are selected by frame id round(t * fps) in [start_frame, end_frame) (slam_reader.py);
  * every chunk is prepared on its own: cameras relative to the chunk's first frame, Umeyama scale over its frames only;
  * the chunk loop is range(total_start, total_end - test_size, test_size) (:183): a span that is a multiple of test_size
    loses its last chunk;
  * the pickle: five keys in the order gt_global_skeleton, estimated_global_skeleton, estimated_local_skeleton,
    camera_pose_list, heatmap_list; every value a list of per-frame arrays; estimated_local_skeleton Fortran-ordered float64,
    heatmap_list what loadmat returned (the file's class, Fortran order); default pickle protocol.

One documented difference: a trajectory file without a line for some frame id of [start_frame, end_frame) makes the reference
write lists of different lengths, which its own optimiser cannot read; here that is a ValueError naming the ids.  So is a
listing with fewer files than the range asks for.

    python -m globalegomocap_amd.prepare --slam traj.txt --heatmaps DIR --depths DIR --gt gt.pkl --start 551 --end 3300 \\
        --fps 25 --out DIR [--optimize]

A recording without ground truth gives the SLAM scale instead -- 1 for a metric SLAM, a number the user
knows, or `auto` for a monocular SLAM, whose scale is then estimated from the recording's own foot contacts before the cameras are
made (`slam_scale`), or `drift` for one whose scale creeps over the recording: the scale is then a curve and the
trajectory is rebuilt in metres first: `--scale S|auto|drift` in place of `--gt`, `scale=` in place of `gt_path=`.  The cameras of a chunk are then the reference's
`SLAMReader.read_trajectory(path, start, end, scale)` (`slam.scaled_trajectory`), the chunks carry no ground truth, their pickles
no `gt_global_skeleton`, and since one scale holds for the whole recording its chunks share a world: `Recording.origins`,
`to_recording_frame`.

    python -m globalegomocap_amd.prepare --slam traj.txt --heatmaps DIR --depths DIR --scale 1.0 --start 551 --end 3300 \\
        --fps 25 --out DIR [--optimize]

A trajectory that lacks lines because SLAM lost tracking is still refused -- unless `--bridge [SECONDS]` (`bridge=`) is given on this
route: the missing cameras are then invented kinematically, marked in `Recording.bridged` and accounted for in
`Recording.bridge_report` (`slam_bridge`).

A pose network without a depth head leaves heat-maps only.  `--depth_from bones` in place of `--depths` (`depth="bones"` with
`depth_dir=None`) takes the maps' sub-pixel peaks (`gem_heatmap_peaks`) and solves the depths from the wearer's bone lengths
(`gem_bone_depths`); no depth file is listed or read, and the Recording keeps the network's own maps:

    python -m globalegomocap_amd.prepare --slam traj.txt --heatmaps DIR --depth_from bones [--bones FILE.npy] [--neck_depth M] \\
        [--min_peak P] --scale auto --start 551 --end 3300 --optimize

`--peaks subpixel` with `--depths` keeps the network's depths and lifts at the sub-pixel peak instead of the 16-pixel argmax.
"""
import ctypes as C
import io
import os
import pickle
import zlib
from collections import namedtuple

import numpy as np

from . import _capi
from .staging import Laps, copy_stream, natural_key, padded, reader_pool, side_by_side

HEAT_NAME, DEPTH_NAME = "heatmap", "depth"
PICKLE_KEYS = ("gt_global_skeleton", "estimated_global_skeleton", "estimated_local_skeleton", "camera_pose_list", "heatmap_list")
N_READERS = 8
_ALIGN = 16                      # file images are laid out on 16-byte boundaries, with at least 8 bytes of slack behind each


# ------------------------------------------------------------------------------------------------------------------ host-side logic
def list_frames(directory, start_frame, end_frame):
    """`natsorted(os.listdir(directory))[start_frame:end_frame]` as full paths (process_test_data.py:52-53): the range indexes
    the LISTING.  Every entry counts, whatever it is, as in the reference."""
    names = sorted(os.listdir(directory), key=natural_key)[start_frame:end_frame]
    return [os.path.join(directory, n) for n in names]


def chunk_spans(total_start_frame, total_end_frame, test_size=100):
    """The reference's chunk loop (:183-187): [(start, end)] for start in range(total_start, total_end - test_size, test_size).
    A span that is a multiple of test_size does NOT produce its last chunk."""
    return [(i, i + test_size) for i in range(total_start_frame, total_end_frame - test_size, test_size)]


def read_gt(gt_path):
    """The ground-truth pickle (a sequence of [J,3] arrays, or one [N,J,3] array) through the restricted unpickler: numpy arrays and
    builtin containers only."""
    from .motion_data import _RestrictedUnpickler, _allowed_globals
    with open(gt_path, "rb") as f:
        return _RestrictedUnpickler(io.BytesIO(f.read()), _allowed_globals()).load()


def gt_clip(pose_gt, start_frame, end_frame, mat_start_frame):
    """load_gt_data (:38-48): [pose_gt[i - mat_start_frame] for i in range(start_frame, end_frame)], the arrays untouched (a
    negative index wraps round, as it does there)."""
    return [pose_gt[i - mat_start_frame] for i in range(start_frame, end_frame)]


def check_trajectory(text, start_frame, end_frame, fps):
    """ValueError when the trajectory (its text, or its rows as `slam.trajectory_rows` parses them) has no line, or more than one,
    for a frame id of [start_frame, end_frame)."""
    from . import slam
    ids = slam.frame_ids(text, fps)
    ids = ids[(ids >= start_frame) & (ids < end_frame)]
    missing = sorted(set(range(start_frame, end_frame)) - set(ids.tolist()))
    if missing:
        raise ValueError("the trajectory has no line for frame ids %s of [%d, %d) at %g fps (the reference would write lists of "
                         "different lengths here)" % (missing, start_frame, end_frame, fps))
    if len(ids) != end_frame - start_frame:
        u, c = np.unique(ids, return_counts=True)
        raise ValueError("the trajectory has several lines for frame ids %s" % u[c > 1].tolist())


def gt_or_scale(gt_path, scale):
    """Exactly one of the ground-truth pickle and the SLAM scale must be given: ValueError otherwise.  -> the scale as a float, the
    word "auto" as it is (the scale is then estimated from the recording's foot contacts: `slam_scale`), or
    None on the ground-truth route."""
    if (gt_path is None) == (scale is None):
        raise ValueError("give exactly one of gt_path (the ground truth fixes the SLAM scale) and scale (a recording without ground truth)")
    if scale is None:
        return None
    if isinstance(scale, str) and scale in ("auto", "drift"):
        return scale
    scale = float(scale)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("the SLAM scale must be a positive number, got %r" % scale)
    return scale


class CameraRoute:
    """How a recording's SLAM track becomes cameras, fixed once per call from the route's keywords of the same names: `gt_path` or
    `scale` as `gt_or_scale` leaves it, `bridge` as `slam_bridge.bridge_arg` leaves it, and what the estimators of scale="auto" /
    "drift" take (`slam_scale.estimate_scale`, `estimate_drift`).  ValueError for arguments that do not go together."""
    TAU, MIN_PAIRS, STIFFNESS = 0.10, 50, 1.0          # the estimators' defaults, for this record and the .mat route's signature

    def __init__(self, gt_path=None, scale=None, bridge=None, lag=None, tau=TAU, min_pairs=MIN_PAIRS, knot=None, stiffness=STIFFNESS):
        from .slam_bridge import bridge_arg
        self.gt_path, self.scale, self.bridge = gt_path, gt_or_scale(gt_path, scale), bridge_arg(bridge, gt_path)
        self.lag, self.tau, self.min_pairs, self.knot, self.stiffness = lag, tau, min_pairs, knot, stiffness

    has_gt = property(lambda self: self.scale is None)
    auto = property(lambda self: self.scale == "auto")
    drift = property(lambda self: self.scale == "drift")


def scaled_cameras(rows, spans, fps, scale):
    """The cameras of a recording without ground truth from the trajectory's rows (`slam.trajectory_rows`): per chunk [a, b) of `spans`
    `slam.scaled_trajectory(*slam.parse_trajectory(rows, a, b, fps), scale)` -- the reference's `read_trajectory`, relative to the
    chunk's first frame -- and `origins` [n_chunks,4,4]: each chunk's first camera relative to the first frame of the first chunk,
    at that scale, so that origins[k] @ cams[k][f] is frame f of chunk k in the recording's frame.  -> ([cams per chunk], origins)."""
    from . import slam
    cams = [slam.scaled_trajectory(*slam.parse_trajectory(rows, a, b, fps), scale) for a, b in spans]
    firsts = [slam.parse_trajectory(rows, a, a + 1, fps) for a, _ in spans]
    origins = slam.scaled_trajectory(np.concatenate([t for t, _ in firsts]), np.concatenate([q for _, q in firsts]), scale) if spans \
        else np.empty((0, 4, 4))
    return cams, origins


def to_recording_frame(recording, poses_per_chunk):
    """Per-chunk results (one [n,J,3] array per chunk, each in its chunk's global frame: what the optimiser returns) in the ONE frame
    a recording without ground truth has: R_k X + t_k with `recording.origins[k]`, float64 on the host.  -> a list of arrays."""
    if recording.origins is None:
        raise ValueError("a recording with ground truth has no common frame: every chunk has its own SLAM scale")
    parts = list(poses_per_chunk)
    if len(parts) != len(recording):
        raise ValueError("%d chunks of poses for a recording of %d chunks" % (len(parts), len(recording)))
    return [np.asarray(p, dtype=np.float64) @ o[:3, :3].T + o[:3, 3] for p, o in zip(parts, np.asarray(recording.origins, dtype=np.float64))]


# ------------------------------------------------------------------------------------------------------------------ MAT files
_NP_OF = {_capi.MI_SINGLE: np.float32, _capi.MI_DOUBLE: np.float64}


def mat_scan(buf, name, start=0, bare=False):
    """gem_mat_scan on a bytes-like object -> (return code, GemMatArray, reason)."""
    lib = _capi.load_library()
    view = np.frombuffer(buf, dtype=np.uint8)
    out = _capi.GemMatArray(start=start, bare=1 if bare else 0)
    rc = lib.gem_mat_scan(C.c_void_p(view.ctypes.data if view.size else 0), view.size, name.encode(), C.byref(out))
    return rc, out, ("" if rc == 0 else (lib.gem_last_error() or b"").decode())


def locate(buf, name):
    """Where the array `name` lies in the MAT file image `buf`: (image, offset, numpy dtype, dims) -- `image` is `buf` itself, or
    the inflated element when the variable was stored compressed -- or None when the file is outside the library's subset
    (`mat_scan` tells why).  Compressed elements are inflated with the standard library's zlib."""
    start = 0
    for _ in range(4096):
        rc, a, _why = mat_scan(buf, name, start)
        if rc:
            return None
        if not a.compressed:
            return buf, int(a.offset), _NP_OF[a.storage], tuple(int(d) for d in a.dims[:a.ndim])
        try:
            raw = zlib.decompress(bytes(memoryview(buf)[a.offset:a.offset + a.nbytes]))
        except zlib.error:
            return None
        rc, b, _why = mat_scan(raw, name, 0, bare=True)
        if rc == 0 and not b.compressed:
            return raw, int(b.offset), _NP_OF[b.storage], tuple(int(d) for d in b.dims[:b.ndim])
        if rc != _capi.MAT_NOT_FOUND:
            return None
        start = int(a.next)
        if start >= len(buf):
            return None
    return None


def array_at(image, offset, dtype, dims):
    """The located array as numpy (a Fortran-ordered view of `image`, as loadmat's arrays are)."""
    n = int(np.prod(dims, dtype=np.int64))
    return np.frombuffer(image, dtype=dtype, count=n, offset=offset).reshape(dims, order="F")


def read_mat_array(path, name):
    """`scipy.io.loadmat(path)[name]`: through the library's reader where the file is inside its subset, else through loadmat
    itself (which reproduces the reference by construction).  -> (array, "native" | "loadmat")."""
    with open(path, "rb") as f:
        buf = f.read()
    hit = locate(buf, name)
    if hit is not None:
        return array_at(*hit), "native"
    from scipy.io import loadmat
    return loadmat(path)[name], "loadmat"


# ------------------------------------------------------------------------------------------------------------------ the recording
def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


class RecordingChunk:
    """One chunk [start_frame, end_frame): `heat` [n,H,W,J] f32, `est_local` / `est_global` / `gt` [n,J,3] f64, `cams` [n,4,4] f64
    (device tensors; numpy arrays work for the host-side methods), `gt_list` the ground-truth arrays as the GT pickle holds
    them, `heat_files` per frame None or the heat-map as loadmat returns it (kept for files that are not float32: the device
    copy is float32), `initial_mpjpe`.  A chunk of a recording without ground truth has `gt`, `gt_list` and `initial_mpjpe` None."""

    def __init__(self, start_frame, end_frame, heat, est_local, est_global, cams, gt, gt_list=None, heat_files=None, initial_mpjpe=None):
        self.start_frame, self.end_frame = int(start_frame), int(end_frame)
        self.heat, self.est_local, self.est_global, self.cams, self.gt = heat, est_local, est_global, cams, gt
        self.gt_list = gt_list
        self.heat_files = heat_files
        self.initial_mpjpe = initial_mpjpe
        self.n = len(est_local)

    @property
    def name(self):
        return "data_start_{}_end_{}".format(self.start_frame, self.end_frame)


class Recording:
    """The chunks of one recording, device-resident.  `heat`, `est_local`, `est_global`, `cams`, `gt`: one tensor per chunk.
    `origins` [n_chunks,4,4] float64 (numpy) for a recording without ground truth, whose chunks share a world (`scaled_cameras`,
    `to_recording_frame`); None for a recording with ground truth.  `scale` and `scale_report` (`slam_scale.ScaleEstimate`): the SLAM
    scale a recording prepared with scale="auto" was given and how it was found; with scale="drift" the `slam_scale.DriftEstimate` and
    its `scale_mean`; None on the other routes.  `bridge_report`
    (`slam_bridge.BridgeReport`) and `bridged` (one bool array per chunk: the frames whose camera was invented) for a recording prepared
    with `bridge=`; None without.  `depth_report` (`bone_depth.BoneDepthReport`) for a recording of detections whose depths were solved
    from the bone lengths; None on every other route."""

    def __init__(self, chunks, origins=None, scale=None, scale_report=None, bridge_report=None, depth_report=None):
        self.depth_report = depth_report
        self.chunks = list(chunks)
        self.origins = origins
        self.scale, self.scale_report = scale, scale_report
        self.bridge_report = bridge_report

    @property
    def bridged(self):
        if self.bridge_report is None:
            return None
        cuts = np.concatenate([[0], np.cumsum([c.n for c in self.chunks])])
        return [self.bridge_report.bridged[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]

    def __len__(self):
        return len(self.chunks)

    heat = property(lambda self: [c.heat for c in self.chunks])
    est_local = property(lambda self: [c.est_local for c in self.chunks])
    est_global = property(lambda self: [c.est_global for c in self.chunks])
    cams = property(lambda self: [c.cams for c in self.chunks])
    gt = property(lambda self: [c.gt for c in self.chunks])

    def continuous(self):
        """The recording as ONE chunk over [first start_frame, last end_frame) in the recording's frame: cameras
        origins[k] @ cams_k[f] and `est_global` moved by origins[k] (float64, with torch where the chunks lie), `est_local` and the
        heat-maps laid end to end as they are; `scale`, `scale_report`, `bridge_report` and `depth_report` carried over, `origins` one
        identity.  Needs `origins` (a recording without ground truth: ValueError otherwise, as `to_recording_frame`) and chunks that
        follow one another (ValueError).  A recording of one chunk is returned as it is."""
        import torch
        if len(self.chunks) == 1:
            return self
        if not self.chunks:
            raise ValueError("a recording without chunks")
        if self.origins is None:
            raise ValueError("a recording with ground truth has no common frame: every chunk has its own SLAM scale")
        for p, q in zip(self.chunks[:-1], self.chunks[1:]):
            if p.end_frame != q.start_frame:
                raise ValueError("the chunks must follow one another: [%d, %d) is followed by [%d, %d)" % (p.start_frame, p.end_frame, q.start_frame, q.end_frame))
        origins = np.asarray(self.origins, dtype=np.float64)
        if origins.shape != (len(self.chunks), 4, 4):
            raise ValueError("%s origins for a recording of %d chunks" % (origins.shape, len(self.chunks)))
        first = self.chunks[0]
        tensor = lambda x, dtype: torch.as_tensor(x).to(dtype=dtype)      # noqa: E731
        cams, est_global = [], []
        for c, o in zip(self.chunks, origins):
            k = tensor(c.cams, torch.float64)
            o = torch.from_numpy(o).to(k.device)
            cams.append(torch.matmul(o, k))
            g = tensor(c.est_global, torch.float64).to(k.device)
            est_global.append(torch.matmul(g, o[:3, :3].T) + o[:3, 3])

        def cat(parts, like):          # (an array the chunks hold as numpy stays numpy)
            whole = torch.cat([torch.as_tensor(p) for p in parts]).contiguous()
            return whole if torch.is_tensor(like) else whole.cpu().numpy()
        cams, est_global = cat(cams, first.cams), cat(est_global, first.est_global)
        est_local, heat = cat(self.est_local, first.est_local), cat(self.heat, first.heat)
        files = None
        if any(c.heat_files is not None for c in self.chunks):
            files = [x for c in self.chunks for x in (c.heat_files if c.heat_files is not None else [None] * c.n)]
        one = RecordingChunk(self.chunks[0].start_frame, self.chunks[-1].end_frame, heat, est_local, est_global, cams, None, heat_files=files)
        return Recording([one], np.eye(4)[None], self.scale, self.scale_report, self.bridge_report, self.depth_report)

    def chunk_dict(self, i):
        """Chunk i as the reference pickles it (:149-155): five keys in its order, every value a list of per-frame arrays;
        estimated_local_skeleton Fortran-ordered float64, estimated_global_skeleton and camera_pose_list C-ordered float64,
        heatmap_list [H,W,J] Fortran-ordered in the file's class, the ground truth as the GT pickle held it.  A chunk without
        ground truth gives the other four keys, unchanged."""
        c = self.chunks[i]
        heat = None
        heats = []
        for f in range(c.n):
            kept = c.heat_files[f] if c.heat_files is not None else None
            if kept is None:
                if heat is None:
                    heat = _host(c.heat)
                kept = np.asfortranarray(heat[f])
            heats.append(kept)
        d = {}
        if c.gt_list is not None or c.gt is not None:
            d[PICKLE_KEYS[0]] = c.gt_list if c.gt_list is not None else list(_host(c.gt))
        d[PICKLE_KEYS[1]] = [np.ascontiguousarray(a, dtype=np.float64) for a in _host(c.est_global)]
        d[PICKLE_KEYS[2]] = [np.asfortranarray(a, dtype=np.float64) for a in _host(c.est_local)]
        d[PICKLE_KEYS[3]] = [np.ascontiguousarray(a, dtype=np.float64) for a in _host(c.cams)]
        d[PICKLE_KEYS[4]] = heats
        return d

    def write_chunk(self, i, out_dir):
        """`<out_dir>/test_data.pkl` of chunk i (:142-157; default pickle protocol)."""
        if not os.path.isdir(out_dir):
            os.makedirs(out_dir)
        with open(os.path.join(out_dir, "test_data.pkl"), "wb") as f:
            pickle.dump(self.chunk_dict(i), f)

    def write_chunks(self, out_root):
        """`<out_root>/data_start_{a}_end_{b}/test_data.pkl` for every chunk; returns the directories."""
        dirs = []
        for i, c in enumerate(self.chunks):
            dirs.append(os.path.join(out_root, c.name))
            self.write_chunk(i, dirs[-1])
        return dirs


# ------------------------------------------------------------------------------------------------------------------ the device path
_engines = {}


def _lift_engine(camera_model_path, device):
    """The engine whose handle the lifting kernel runs under (one per calibration and device; its network is never used)."""
    from .camera import FisheyeCamera
    from .engine import WindowEngine
    from .vae import VAEShape
    key = (os.path.abspath(camera_model_path), device)
    if key not in _engines:
        _engines[key] = WindowEngine(VAEShape(latent_dim=64, hidden=(16, 16, 32, 32, 64)), FisheyeCamera.from_json(camera_model_path),
                                     max_windows=1, device=device)
    return _engines[key]


def _c_paths(paths):
    return (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])


def _element(array, i):
    """Pointer to element i of a ctypes array: what a C function sees as the array from there on."""
    return C.cast(C.byref(array, i * C.sizeof(array._type_)), C.POINTER(array._type_))


def _file_sizes(lib, pool, cpaths, readers):
    """The files' sizes (int64 array), one stat each, on the reader threads (gem_files_sizes: the GIL is free)."""
    count = len(cpaths)
    sizes = np.empty(count, dtype=np.int64)

    def stat_range(lo, hi):
        _capi.check(lib.gem_files_sizes(_element(cpaths, lo), hi - lo, C.c_void_p(sizes.ctypes.data + 8 * lo)), lib)
    cut = [count * k // readers for k in range(readers + 1)]
    for j in [pool.submit(stat_range, lo, hi) for lo, hi in zip(cut[:-1], cut[1:]) if hi > lo]:
        j.result()
    return sizes


def _read_range(lib, cpaths, lo, hi, at, sizes, n, block, found, rcs, paths, send=None):
    """Reader thread: files [lo, hi) of the n heat-map files and the n depth files behind them into `block` (a uint8 numpy array; gem_mat_read: the GIL is free); `send(lo, hi)` then starts
    the range's copy to the device, so that it crosses PCIe while other ranges are still being read.  Then the files the scanner
    could not take as they are: compressed elements are inflated here (zlib releases the GIL too), files outside the subset go
    through loadmat.
    -> ([(index, payload bytes, numpy dtype, dims, array as loadmat returns it or None)] for those, what `send` returned)."""
    extra, sent = [], None
    names = (HEAT_NAME, DEPTH_NAME)          # names[i >= n]: the array that file i holds
    for i, j in ((lo, min(hi, n)), (max(lo, n), hi)):          # (the range's heat-map files, then its depth files: one or two calls)
        if i < j:
            _capi.check(lib.gem_mat_read(_element(cpaths, i), j - i, C.c_void_p(at.ctypes.data + 8 * i), C.c_void_p(sizes.ctypes.data + 8 * i),
                                         names[i >= n].encode(), C.c_void_p(block.ctypes.data), block.size, _element(found, i),
                                         C.c_void_p(rcs.ctypes.data + 4 * i)), lib)
    if send is not None and any(rcs[i] == 0 and not found[i].compressed for i in range(lo, hi)):
        sent = send(lo, hi)
    for i in range(lo, hi):
        if rcs[i] == 0 and not found[i].compressed:
            continue
        hit = None
        if rcs[i] == 0:
            hit = locate(block[int(at[i]):int(at[i] + sizes[i])], names[i >= n])
        if hit is not None:
            a = array_at(*hit)
            extra.append((i, a.tobytes(order="F"), a.dtype.type, a.shape, None))
        else:
            from scipy.io import loadmat
            a = loadmat(paths[i])[names[i >= n]]
            dev = a if a.dtype in (np.float32, np.float64) else a.astype(np.float32 if i < n else np.float64)
            extra.append((i, dev.tobytes(order="F"), dev.dtype.type, a.shape, a))
        rcs[i] = -1          # (its payload travels in the extra block)
    return extra, sent


def _read_files(lib, pool, readers, cpaths, at, room, sizes, n, block, found, rcs, paths, send, sent):
    """The reader fan-out: every file into its place in `block`, range by range on the pool's threads (`_read_range`); `sent` is
    handed what each range's `send` returned, in range order.  -> the extra payloads of all ranges."""
    # heat-map files are 2000 times the depth files: the ranges are cut by bytes, not by count; four ranges per reader, so that
    # the first copies start early
    cuts = np.searchsorted(np.cumsum(room), np.linspace(0, block.size, 4 * readers + 1)[1:-1]).tolist()
    bounds = sorted(set([0] + [int(c) for c in cuts] + [len(paths)]))
    jobs = [pool.submit(_read_range, lib, cpaths, lo, hi, at, sizes, n, block, found, rcs, paths, send)
            for lo, hi in zip(bounds[:-1], bounds[1:]) if hi > lo]
    extra = []
    for j in jobs:
        e, ev = j.result()
        extra += e
        if ev is not None:
            sent(ev)
    return extra


def payload_tables(n, paths, at, found, rcs, extra, block, depths=True):
    """Where every frame's payloads lie and what they are -- host data only.  Files [0, n) hold the heat-maps, [n, 2n) the depths;
    `found` / `rcs` are what gem_mat_read left for the files at `at` in `block` (uint8 numpy array: the main block), `extra` the
    payloads `_read_range` made itself (rcs -1).  Payloads that are not in the files as they are get a place BEHIND the block:
    the extra ones, and the first row of a several-row depth (depth = loadmat(...)['depth'][0]).
    -> (where int64 [2n]: byte offsets; kinds int32 [n]: MAT_HEAT_F64 | MAT_DEPTH_F32; (H, W, J); heat_files [n]: None, or the
    heat-map as loadmat returns it where that is not float32 -- the pickle wants it as it is; parts [(offset, bytes)]: what goes
    behind the block; end: the block's length with them).  `depths` False: a recording without depth files -- there are n files, `where`
    is [n] and no frame's kind has a depth bit."""
    total = block.size
    m = 2 * n if depths else n
    where = np.zeros(m, dtype=np.int64)
    dtypes, dims = [None] * m, [None] * m
    heat_files = [None] * n
    for i in range(m):
        if rcs[i] == 0:
            a = found[i]
            where[i], dtypes[i], dims[i] = at[i] + a.offset, _NP_OF[a.storage], tuple(int(d) for d in a.dims[:a.ndim])
    end, parts = total, []
    for i, payload, dt, shape, kept in extra:
        if i >= n and len(shape) == 2 and shape[0] != 1:          # depth = loadmat(...)['depth'][0]: the first ROW
            payload, shape = np.frombuffer(payload, dtype=dt).reshape(shape, order="F")[:1].tobytes(), (1, shape[1])
        where[i], dtypes[i], dims[i] = end, dt, tuple(shape)
        parts.append((end, payload))
        end += padded(len(payload), _ALIGN)
        if i < n and (kept is not None or dt is not np.float32):
            heat_files[i] = kept if kept is not None else np.frombuffer(payload, dtype=dt).reshape(shape, order="F")
    for i in range(n, m):          # a depth array of several rows inside the main block: its first row is strided there
        if rcs[i] == 0 and (len(dims[i]) != 2 or dims[i][0] != 1):
            if len(dims[i]) != 2:
                raise ValueError("%s: 'depth' is not a [1,J] array" % paths[i])
            row = array_at(block, int(where[i]), dtypes[i], dims[i])[:1]
            where[i], dims[i] = end, (1, dims[i][1])
            parts.append((end, row.tobytes()))
            end += padded(row.nbytes, _ALIGN)
    for f in range(n):          # float64 heat-maps inside the main block: the pickle wants them as they are
        if rcs[f] == 0 and dtypes[f] is np.float64:
            heat_files[f] = array_at(block, int(where[f]), np.float64, dims[f]).copy(order="F")
    shapes = {dims[f] for f in range(n)}
    if len(shapes) != 1 or len(next(iter(shapes))) != 3:
        raise ValueError("the heat-maps must all be [H,W,J] arrays of one shape, found %s" % sorted(shapes))
    J = next(iter(shapes))[2]
    if any(dims[i] != (1, J) for i in range(n, m)):
        raise ValueError("every depth file must hold a [1,%d] array" % J)
    kinds = np.array([(_capi.MAT_HEAT_F64 if dtypes[f] is np.float64 else 0) | (_capi.MAT_DEPTH_F32 if depths and dtypes[n + f] is np.float32 else 0)
                      for f in range(n)], dtype=np.int32)
    return where, kinds, next(iter(shapes)), heat_files, parts, end


def _frames_from_arena(arena, total, in_block, where, kinds, shape, parts, end, device, depths=True):
    """Upload + launch: the payloads of `parts` land behind the block's image (`total` bytes of `arena`; `in_block`: whether any
    frame is read from it), in the same arena; the tables go up and ONE gem_mat_frames picks all frames out.  -> (heat, depth; None without `depths`)."""
    import torch
    n, (H, W, J) = len(kinds), shape
    if parts:
        whole = torch.empty(end + 8, dtype=torch.uint8, device=device)
        if in_block:
            whole[:total].copy_(arena[:total])
        side = torch.empty(end - total, dtype=torch.uint8, pin_memory=True)
        sv = side.numpy()
        for o, payload in parts:
            sv[o - total:o - total + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
        whole[total:end].copy_(side, non_blocking=True)
        arena = whole
    tables = torch.from_numpy(np.concatenate([where, kinds.astype(np.int64)])).to(device)
    kinds_d = tables[len(where):].to(torch.int32)
    heat = torch.empty((n, H, W, J), dtype=torch.float32, device=device)
    depth = torch.empty((n, J), dtype=torch.float64, device=device) if depths else None
    mat_frames(arena, end, tables[:n], tables[n:2 * n] if depths else None, kinds_d, heat, depth)
    return heat, depth


def frames_to_device(heat_paths, depth_paths, device=None, readers=N_READERS, timings=None):
    """The frames' .mat files -> (heat [n,H,W,J] f32, depth [n,J] f64, heat_files) on `device`: every file is read once into a
    pinned block (reader threads, `gem_mat_read`), the block crosses PCIe range by range on the readers' two copy streams while
    the other ranges are still being read (one more copy for inflated or loadmat'ed payloads), and ONE launch of `gem_mat_frames`
    picks all frames out.  heat_files[f]: None, or the heat-map as loadmat returns it where the device copy (float32) is not the
    file's own class.  `depth_paths` None: a recording without depth files -- no such file is read or uploaded, `depth` is None."""
    import torch
    lib = _capi.load_library()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n = len(heat_paths)
    depths = depth_paths is not None
    if depths and len(depth_paths) != n:
        raise ValueError("as many depth files as heat-map files are needed (%d / %d)" % (len(depth_paths), n))
    if n == 0:
        return torch.empty((0, 64, 64, 15), device=device), torch.empty((0, 15), dtype=torch.float64, device=device) if depths else None, []
    lap = Laps(timings)          # developer timing (tools/prepare_bench.py)
    paths = list(heat_paths) + (list(depth_paths) if depths else [])
    cpaths = _c_paths(paths)
    readers = max(1, min(readers, len(paths)))
    pool = reader_pool("mat", readers)
    sizes = _file_sizes(lib, pool, cpaths, readers)
    at, room, total = side_by_side(sizes, _ALIGN)
    lap("file sizes (one stat each)")
    pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)          # (torch keeps freed pinned blocks for the next call)
    block = pinned.numpy()
    found = (_capi.GemMatArray * len(paths))()
    rcs = np.zeros(len(paths), dtype=np.int32)
    lap("pinned block")
    arena = torch.empty(total + 8, dtype=torch.uint8, device=device)
    cur = torch.cuda.current_stream()
    allocated = torch.cuda.Event()
    allocated.record(cur)

    def send(lo, hi):
        """Files [lo, hi) of the block to their place in the arena, on one of the two copy streams -> the event behind the copy."""
        st = copy_stream(device)
        b0, b1 = int(at[lo]), int(at[hi - 1] + room[hi - 1])
        st.wait_event(allocated)
        with torch.cuda.stream(st):
            arena[b0:b1].copy_(pinned[b0:b1], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st)
        arena.record_stream(st)
        return ev
    extra = _read_files(lib, pool, readers, cpaths, at, room, sizes, n, block, found, rcs, paths, send, cur.wait_event)
    lap("read + scan (+ inflate / loadmat) on the reader threads")
    where, kinds, shape, heat_files, parts, end = payload_tables(n, paths, at, found, rcs, extra, block, depths)
    lap("payload tables")
    heat, depth = _frames_from_arena(arena, total, bool((rcs == 0).any()), where, kinds, shape, parts, end, device, depths)
    torch.cuda.current_stream().synchronize()          # (the pinned block is released on return)
    lap("copies' tail + gem_mat_frames")
    return heat, depth, heat_files


def mat_frames(arena, image_len, heat_offsets, depth_offsets, kinds, heat, depth):
    """gem_mat_frames on the current stream: arena (uint8 device tensor), int64 / int64 / int32 device tables -> heat, depth.
    `depth_offsets` and `depth` both None: the heat-maps alone."""
    import torch
    lib = _capi.load_library()
    n, H, W, J = heat.shape
    _capi.check(lib.gem_mat_frames(C.c_void_p(arena.data_ptr()), int(image_len), C.c_void_p(heat_offsets.data_ptr()),
                                   C.c_void_p(depth_offsets.data_ptr() if depth_offsets is not None else 0), C.c_void_p(kinds.data_ptr()), n, H, W, J,
                                   C.c_void_p(heat.data_ptr()), C.c_void_p(depth.data_ptr() if depth is not None else 0),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)


def prepare_global(est_local, cams, gt):
    """gem_prepare_global on the current stream: -> (est_global [n,J,3] f64, per-frame mean joint distance to gt [n] f64; None
    without `gt`)."""
    import torch
    lib = _capi.load_library()
    n, J = est_local.shape[0], est_local.shape[1]
    out = torch.empty_like(est_local)
    err = torch.empty(n, dtype=torch.float64, device=est_local.device) if gt is not None else None
    _capi.check(lib.gem_prepare_global(C.c_void_p(est_local.data_ptr()), C.c_void_p(cams.data_ptr()),
                                       C.c_void_p(gt.data_ptr() if gt is not None else 0), n, J,
                                       C.c_void_p(out.data_ptr()), C.c_void_p(err.data_ptr() if err is not None else 0),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)
    return out, err


class RecordingStage:
    """What every route into a `Recording` does once it has the lifted poses `est_local`: fix the SLAM scale, build the cameras, apply
    them (`gem_prepare_global`) and cut the chunks.  One per call.  The route makes it first from its `CameraRoute` (the argument checks),
    reads and checks the trajectory through it, sets `bounds` [(first row, row behind the last)] and `gts` (per chunk the ground-truth
    arrays; unused without ground truth) for its chunks, and then calls `fix_scale` and `recording` -- two steps, because a route may
    enqueue device work between them that the host's camera work then overlaps (the detection route's heat-maps)."""

    def __init__(self, route, spans, fps):
        self.route, self.scale, self.bridge = route, route.scale, route.bridge          # (`scale`: a number once `fix_scale` has run)
        self.spans, self.fps = [(int(a), int(b)) for a, b in spans], fps
        self.rows = self.systems = self.bounds = self.gts = None
        self.cams = self.origins = self.scale_report = self.bridge_report = None

    def read_trajectory(self, slam_result_path):
        from . import slam
        with open(slam_result_path) as f:
            self.rows = slam.trajectory_rows(f.read())          # (parsed once for all chunks)

    def read_gt(self):
        """The ground-truth pickle's poses; None for a recording without ground truth."""
        return read_gt(self.route.gt_path) if self.route.has_gt else None

    def check_trajectory(self):
        """Every span's frame ids have their trajectory line (`check_trajectory`) -- or, with `bridge`, the lost ones can be bridged
        (`slam_bridge.find_gaps`, whose systems are kept for `fix_scale`).  ValueError otherwise."""
        from . import slam, slam_bridge
        if self.bridge is None:
            for a, b in self.spans:
                check_trajectory(self.rows, a, b, self.fps)
        elif self.spans:
            self.systems = slam_bridge.find_gaps(slam.frame_ids(self.rows, self.fps), *slam_bridge.contiguous_span(self.spans),
                                                 slam_bridge.max_gap_frames(self.bridge, self.fps))

    def empty(self):
        """The recording of no spans."""
        return Recording([], None if self.route.has_gt else np.empty((0, 4, 4)))

    def fix_scale(self, engine, est_local, lap=Laps(None)):
        """Everything that can still refuse the recording, and everything that needs a read-back before the cameras exist: "auto"
        becomes a number and a `slam_scale.ScaleEstimate` (with `bridge` from the tracked frames only; ValueError when the recording
        does not fix the scale), "drift" becomes the number 1, a `slam_scale.DriftEstimate` and the trajectory in metres in place of
        `rows`, and with `bridge` the bridged cameras, the origins and the `slam_bridge.BridgeReport` are made;
        the cameras stay on the device.  Nothing to do with ground truth."""
        route = self.route
        if route.has_gt:
            return
        if route.auto or route.drift:
            from .slam_scale import estimate_drift, estimate_scale
            pairs = dict(lag=route.lag, tau=route.tau, min_pairs=route.min_pairs, tracked=self.bridge is not None)
            if route.drift:          # from here on the trajectory is the metric one, at scale 1
                self.scale_report = estimate_drift(est_local, self.rows, self.spans, self.fps, knot=route.knot, stiffness=route.stiffness, **pairs)
                self.scale, self.rows = 1.0, self.scale_report.metric_rows()
            else:
                self.scale_report = estimate_scale(est_local, self.rows, self.spans, self.fps, **pairs)
                self.scale = float(self.scale_report.scale)
        if self.bridge is not None:
            from .slam_bridge import bridge_cameras
            self.cams, self.origins, self.bridge_report = bridge_cameras(engine, self.rows, self.spans, self.fps, self.scale, self.bridge,
                                                                         systems=self.systems)
            lap("lift enqueued + bridged cameras (gem_slam_bridge, report back)")
        elif self.scale_report is not None:
            lap("lift + SLAM scale estimate (gem_slam_scale, report back)")

    def recording(self, est_local, heat, heat_files=None, lap=Laps(None)):
        """The cameras -- per-chunk Umeyama against the ground truth's head track on the host, `scaled_cameras`, or `fix_scale`'s
        bridged ones -- go up, `gem_prepare_global` applies them, and the chunks are cut.  -> Recording."""
        import torch
        from . import slam
        spans, bounds, gt_all = self.spans, self.bounds, None
        if self.route.has_gt:
            heads = est_local[:, 0].cpu().numpy()
            lap("lift + head joints to the host")
            gt_all = np.concatenate([np.asarray(g, dtype=np.float64) for g in self.gts])
            cams = np.concatenate([slam.camera_pose_list_from_heads(self.rows, heads[lo:hi], gt_all[lo:hi, 0], a, b, self.fps)[0]
                                   for (a, b), (lo, hi) in zip(spans, bounds)])
            lap("per-chunk scale and cameras (host)")
        elif self.bridge is None:
            cams, self.origins = scaled_cameras(self.rows, spans, self.fps, self.scale)
            cams = np.concatenate(cams)
            lap("lift enqueued + cameras at the given scale (host)")
        cams_d = torch.cat(self.cams) if self.bridge is not None else torch.from_numpy(cams).to(est_local.device)
        gt_d = None if gt_all is None else torch.from_numpy(gt_all).to(est_local.device)
        est_global, err = prepare_global(est_local, cams_d, gt_d)
        if err is not None:
            err = err.cpu().numpy()
        lap("cameras up + gem_prepare_global" if err is None else "cameras up + gem_prepare_global + errors back")
        chunks = []
        for k, ((a, b), (lo, hi)) in enumerate(zip(spans, bounds)):
            kept = None if heat_files is None else heat_files[lo:hi]
            chunks.append(RecordingChunk(a, b, heat[lo:hi], est_local[lo:hi], est_global[lo:hi], cams_d[lo:hi], None if gt_d is None else gt_d[lo:hi],
                                         gt_list=None if gt_d is None else self.gts[k],
                                         heat_files=kept if kept is not None and any(x is not None for x in kept) else None,
                                         initial_mpjpe=None if err is None else float(np.mean(err[lo:hi]))))
        return Recording(chunks, self.origins, float(self.scale_report.scale) if self.scale_report is not None else None, self.scale_report,
                         self.bridge_report)


def print_report(rec, sequence=True):
    """What a preparation tells about its recording: the scale estimate's line, the bridge's line, and per chunk the reference's
    `running test sequence from a to b` (its chunk loop's; not with `sequence` False) and `The initial mpjpe is: ...` (with ground
    truth)."""
    for report in (rec.depth_report, rec.scale_report, rec.bridge_report):
        if report is not None:
            print(report.line())
    for c in rec.chunks:
        if sequence:
            print("running test sequence from {} to {}".format(c.start_frame, c.end_frame))
        if c.initial_mpjpe is not None:
            print("The initial mpjpe is: {}".format(c.initial_mpjpe))


DepthRoute = namedtuple("DepthRoute", "from_bones subpixel bone_opts min_peak")          # what `depth_route` decides


def depth_route(depth_dir, depth=None, bones=None, neck_depth=None, min_peak=None, peaks=None):
    """The checks of `prepare_spans`' depth arguments, before a device is touched: exactly one of `depth_dir` (the pose network's depth
    files) and depth="bones" (the depths are solved from the bone lengths at the maps' sub-pixel peaks);
    `bones`, `neck_depth` (`bone_depth.options`) and `min_peak` (a finite number >= 0) belong to depth="bones"; `peaks` is None,
    "argmax" (the reference's 16-pixel lift; with depth files only) or "subpixel" (what depth="bones" always uses).
    -> DepthRoute(from_bones, subpixel, bone options or None, min_peak as a float).  ValueError otherwise."""
    if depth is not None and not (isinstance(depth, str) and depth == "bones"):
        raise ValueError('prepare: depth is None (the depth files of depth_dir) or "bones", got %r' % (depth,))
    from_bones = depth is not None
    if from_bones and depth_dir is not None:
        raise ValueError('prepare: depth="bones" takes no depth directory (depth_dir=None)')
    if not from_bones and depth_dir is None:
        raise ValueError('prepare: the joints\' depths are needed: the depth directory, or depth="bones"')
    if not from_bones and (bones is not None or neck_depth is not None or min_peak is not None):
        raise ValueError('prepare: bones=, neck_depth= and min_peak= belong to depth="bones"')
    if peaks not in (None, "argmax", "subpixel"):
        raise ValueError('prepare: peaks is "argmax" or "subpixel", got %r' % (peaks,))
    if from_bones and peaks == "argmax":
        raise ValueError('prepare: depth="bones" needs the sub-pixel peaks (peaks="subpixel" or None)')
    min_peak = 0.0 if min_peak is None else float(min_peak)
    if not (np.isfinite(min_peak) and min_peak >= 0):
        raise ValueError("prepare: min_peak must be a finite number >= 0, got %r" % min_peak)
    bone_opts = None
    if from_bones:
        from . import bone_depth
        bone_opts = bone_depth.options(bones, neck_depth=neck_depth)
    return DepthRoute(from_bones, from_bones or peaks == "subpixel", bone_opts, min_peak)


def solve_bone_depths(engine, kp, bone_opts):
    """Both routes' bone solve with its report: `WindowEngine.bone_depths` of `kp` [n,15,3] -> (depth, solved [n,15], `BoneDepthReport`)."""
    from .bone_depth import summarize
    depth, solved, rms = engine.bone_depths(kp, opts=bone_opts)
    return depth, solved, summarize(solved, rms)


def fill_chunks(engine, est_local, valid, bounds):
    """`fill_missing` within every chunk (rows bounds[k] of the frames), in place: ONE call for chunks of one length, else one per chunk."""
    if len({hi - lo for lo, hi in bounds}) == 1:
        engine.fill_missing(est_local, valid, len(bounds))
    else:
        for lo, hi in bounds:
            engine.fill_missing(est_local[lo:hi], valid[lo:hi], 1)


def lift_peaks(engine, heat, depth, bounds, spans, bone_opts=None, min_peak=0.0):
    """The sub-pixel lift of heat-maps [n,H,W,15] on the device: `heatmap_peaks` -> (with `bone_opts`: `bone_depths`, the confidence
    of every joint the solve did not reach set to 0) -> `lift_keypoints` -> `fill_missing` per chunk (rows bounds[k] of the frames).
    `depth` [n,15]: the network's depths, unused with `bone_opts`.  -> (est_local [n,15,3] f64, `bone_depth.BoneDepthReport` or None).
    A joint with no usable frame in a whole chunk is the detection route's ValueError: one read-back of an [n_chunks,15] mask."""
    import torch
    kp, _ = engine.heatmap_peaks(heat, min_peak=min_peak)
    report = None
    if bone_opts is not None:
        depth, solved, report = solve_bone_depths(engine, kp, bone_opts)
        kp[..., 2] = torch.where(solved.bool(), kp[..., 2], torch.zeros_like(kp[..., 2]))          # (unsolved: a lost detection from here on)
    est_local, _, valid = engine.lift_keypoints(kp, depth)
    seen = torch.stack([valid[lo:hi].bool().any(dim=0) for lo, hi in bounds]).cpu().numpy()
    for row, (a, b) in zip(seen, spans):
        lost = np.nonzero(~row)[0]
        if len(lost):
            raise ValueError("joints %s have no usable detection in the chunk [%d, %d): nothing to interpolate them from" % (lost.tolist(), a, b))
    fill_chunks(engine, est_local, valid, bounds)
    return est_local, report


def prepare_spans(slam_result_path, heatmap_dir, depth_dir, gt_path, spans, fps, mat_start_frame, camera_model_path=None, device=None,
                  timings=None, scale=None, lag=None, tau=CameraRoute.TAU, min_pairs=CameraRoute.MIN_PAIRS, bridge=None, depth=None, bones=None,
                  neck_depth=None, min_peak=None, peaks=None, knot=None, stiffness=CameraRoute.STIFFNESS):
    """Every (start_frame, end_frame) of `spans` as one chunk, each prepared on its own as `main` does, all of them through the
    device together: stage -> gem_mat_frames -> lift -> head joints to the host -> per-chunk scale and cameras -> cameras up ->
    gem_prepare_global.  -> Recording.  `gt_path` None and `scale` given: a recording without ground truth -- the cameras come from
    `scaled_cameras`, nothing goes to the host in between, `mat_start_frame` is not used.  scale="auto": the scale is estimated from the
    lifted poses first (`slam_scale.estimate_scale` with `lag`, `tau`, `min_pairs`; one small record comes back), then the same path runs with it.
    scale="drift": the scale is a curve with knots `knot` frames apart (`stiffness`: of its second differences); the trajectory is rebuilt
    in metres (`slam_scale.DriftEstimate.metric_rows`) and the same path runs with it at scale 1.
    `bridge`: None, or the longest stretch of lost SLAM tracking, in seconds, whose cameras are invented (True: 1 s; `slam_bridge`,
    DESIGN.md section 6o) -- only without ground truth, and the chunks must follow one another.  From the lifted poses on this is
    `RecordingStage`.
    depth="bones" with depth_dir None: a pose network without a depth head.  No depth file is listed, read or
    uploaded; the maps' sub-pixel peaks (`heatmap_peaks`, joints whose peak is below `min_peak` unusable) are given depths by the bone
    solve (`bone_depths` with `bone_depth.options(bones, neck_depth=neck_depth)`), lifted and filled as detections are (`lift_peaks`),
    and the Recording carries the solve's `depth_report`.  Its heat-maps are the files' own.  peaks="subpixel" with a depth directory:
    the network's depths, lifted at the sub-pixel peak instead of the reference's 16-pixel argmax.  Every argument is checked before a
    file or the device is touched: the camera route's (`CameraRoute`), then the depth route's (`depth_route`)."""
    stage = RecordingStage(CameraRoute(gt_path, scale, bridge, lag, tau, min_pairs, knot, stiffness), spans, fps)
    depths = depth_route(depth_dir, depth, bones, neck_depth, min_peak, peaks)
    from_bones = depths.from_bones
    import torch
    from .camera import DEFAULT_CALIBRATION
    lap = Laps(timings)          # developer timing (tools/prepare_bench.py)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    stage.read_trajectory(slam_result_path)
    pose_gt = stage.read_gt()
    heat_names = sorted(os.listdir(heatmap_dir), key=natural_key)
    depth_names = sorted(os.listdir(depth_dir), key=natural_key) if not from_bones else None
    heat_paths, depth_paths, stage.gts, stage.bounds = [], [], [], []
    stage.check_trajectory()
    for a, b in spans:
        hp, dp = heat_names[a:b], depth_names[a:b] if not from_bones else []
        if from_bones and len(hp) != b - a:
            raise ValueError("frames [%d, %d) of the listing are asked for, but %s holds %d files" % (a, b, heatmap_dir, len(heat_names)))
        if not from_bones and (len(hp) != b - a or len(dp) != b - a):
            raise ValueError("frames [%d, %d) of the listings are asked for, but %s holds %d files and %s holds %d" %
                             (a, b, heatmap_dir, len(heat_names), depth_dir, len(depth_names)))
        stage.bounds.append((len(heat_paths), len(heat_paths) + b - a))
        heat_paths += [os.path.join(heatmap_dir, x) for x in hp]
        depth_paths += [os.path.join(depth_dir, x) for x in dp]
        stage.gts.append(gt_clip(pose_gt, a, b, mat_start_frame) if pose_gt is not None else None)
    if not spans:
        return stage.empty()
    lap("listings, ground truth, trajectory")
    with torch.cuda.device(device):
        heat, depth_d, heat_files = frames_to_device(heat_paths, None if from_bones else depth_paths, device, timings=timings)
        lap = Laps(timings)          # (frames_to_device has timed its own phases)
        engine = _lift_engine(camera_model_path or DEFAULT_CALIBRATION, device.index)
        if tuple(heat.shape[1:3]) != tuple(engine.heat_size):
            raise ValueError("heat-maps of %d x %d: the lifting kernel is built for %d x %d" % (tuple(heat.shape[1:3]) + tuple(engine.heat_size)))
        depth_report = None
        if depths.subpixel:
            est_local, depth_report = lift_peaks(engine, heat, depth_d, stage.bounds, stage.spans, depths.bone_opts, depths.min_peak)
        else:
            est_local, _ = engine.lift_skeleton(heat, depth_d)
        stage.fix_scale(engine, est_local, lap)
        rec = stage.recording(est_local, heat, heat_files, lap)
        rec.depth_report = depth_report
        return rec


def main(slam_result_path, heatmap_dir, depth_dir, gt_path, start_frame, end_frame, out_dir, fps, mat_start_frame=None,
         camera_model_path=None, **options):
    """The reference's `main` (:126-165): one chunk [start_frame, end_frame) -> `<out_dir>/test_data.pkl`, and the line
    `The initial mpjpe is: ...`.  Returns the one-chunk Recording (the reference returns nothing).  Without ground truth (`gt_path`
    None, `scale` given) the pickle has four keys and there is no such line; with scale="auto" one line tells the estimate and its
    counts, and a recording that does not fix the scale is a ValueError before anything is written.  `options`: `prepare_spans`'."""
    rec = prepare_spans(slam_result_path, heatmap_dir, depth_dir, gt_path, [(start_frame, end_frame)], fps,
                        start_frame if mat_start_frame is None else mat_start_frame, camera_model_path, **options)
    print_report(rec, sequence=False)
    rec.write_chunk(0, out_dir)
    return rec


def prepare_sequence(slam_result_path, heatmap_dir, depth_dir, gt_path, total_start_frame, total_end_frame, fps=25, mat_start_frame=None,
                     test_size=100, out_root=None, camera_model_path=None, verbose=True, **options):
    """The reference's chunk loop (:176-190): chunks of `test_size` frames from `total_start_frame` (see `chunk_spans` for the
    chunk it drops), `mat_start_frame` defaulting to `total_start_frame` as there.  All chunks go through the device together,
    each prepared on its own.  Returns the Recording; with `out_root`, `data_start_{a}_end_{b}/test_data.pkl` are written too.
    `options`: `prepare_spans`' keywords, handed on as they are; what does not go together is its ValueError, before anything else happens."""
    spans = chunk_spans(total_start_frame, total_end_frame, test_size)
    rec = prepare_spans(slam_result_path, heatmap_dir, depth_dir, gt_path, spans, fps,
                        total_start_frame if mat_start_frame is None else mat_start_frame, camera_model_path, **options)
    if verbose:
        print_report(rec)
    if out_root is not None:
        rec.write_chunks(out_root)
    return rec


def prepare_continuous(slam_result_path, heatmap_dir, depth_dir, gt_path, total_start_frame, total_end_frame, fps=25, mat_start_frame=None,
                       camera_model_path=None, verbose=True, **options):
    """`prepare_sequence` for a recording that is optimised as one motion (`continuous.optimize_continuous`): the
    ONE span [total_start_frame, total_end_frame) as one chunk -- no chunk loop, so no tail is lost, and with a ground truth one Umeyama
    scale over the whole span.  The other arguments as there.  -> a Recording that is continuous already."""
    rec = prepare_spans(slam_result_path, heatmap_dir, depth_dir, gt_path, [(total_start_frame, total_end_frame)], fps,
                        total_start_frame if mat_start_frame is None else mat_start_frame, camera_model_path, **options)
    if verbose:
        print_report(rec)
    return rec


def add_track_options(p, gt_help="ground-truth pickle (it fixes the SLAM scale)", camera=True):
    """The options of every command line that makes a recording's cameras (`prepare`, `detections`, `continuous`): the trajectory, what
    fixes the SLAM scale (`gt_help`: what the command does with a ground truth), the frames and the calibration (camera=False: the
    caller declares `--camera` itself, further down its help).  `track_arguments` turns them into the camera route's keywords."""
    from .camera import DEFAULT_CALIBRATION
    from .slam_scale import add_drift_options, scale_arg
    p.add_argument("--slam", required=True, help="SLAM trajectory: lines `time tx ty tz qx qy qz qw`")
    how = p.add_mutually_exclusive_group(required=True)
    how.add_argument("--gt", default=None, help=gt_help)
    how.add_argument("--scale", type=scale_arg, default=None, help="the SLAM scale of a recording without ground truth (a metric SLAM: 1), "
                                                                  "`auto`: estimate it from the foot contacts, or `drift`: follow a "
                                                                  "scale that creeps over the recording")
    add_drift_options(p)
    p.add_argument("--bridge", nargs="?", type=float, const=1.0, default=None, metavar="SECONDS",
                   help="with --scale: invent the cameras of stretches of lost SLAM tracking up to this long (default 1 s)")
    p.add_argument("--start", required=True, type=int)
    p.add_argument("--end", required=True, type=int)
    p.add_argument("--fps", type=float, default=25)
    p.add_argument("--mat_start", type=int, default=None, help="frame id of the GT pickle's first entry (default: --start)")
    if camera:
        p.add_argument("--camera", default=DEFAULT_CALIBRATION)


def track_arguments(p, a):
    """The parsed options that decide the camera route, as the routes' keywords: `gt_path`, `scale`, `knot` in FRAMES and `stiffness`
    (`slam_scale.drift_options`: the rules of --scale drift, as parser errors), and of `bridge`, `lag`, `tau`, `min_pairs` what the command has."""
    from .slam_scale import drift_options
    return dict({k: getattr(a, k) for k in ("bridge", "lag", "tau", "min_pairs") if hasattr(a, k)}, gt_path=a.gt, scale=a.scale, **drift_options(p, a))


def add_recording_options(p):
    """The options every preparation command line has (`prepare`, `detections`): the track's, the chunks and what to do with them."""
    from .camera import DEFAULT_CALIBRATION
    add_track_options(p, camera=False)
    p.add_argument("--test_size", type=int, default=100)
    p.add_argument("--out", default=None, help="directory for data_start_{a}_end_{b}/test_data.pkl")
    p.add_argument("--camera", default=DEFAULT_CALIBRATION)          # (where these commands' help has always listed it)
    p.add_argument("--optimize", action="store_true", help="optimise the recording right away (no pickle in between)")


def parse_recording_options(p, argv=None):
    """`p.parse_args(argv)` and the checks that go with `add_recording_options`."""
    a = p.parse_args(argv)
    if a.out is None and not a.optimize:
        p.error("nothing to do: give --out, --optimize or both")
    if a.bridge is not None and a.gt is not None:
        p.error("--bridge needs --scale: with --gt every chunk has its own scale and there is no common world to bridge in")
    return a


def add_depth_route_options(p, depth_file=None, peaks=True,
                            depth_from="bones: a pose network without a depth head -- the depths are solved from the bone lengths at the maps' "
                                       "sub-pixel peaks (DESIGN.md section 6r); excludes --depths",
                            min_peak="with --depth_from bones: a joint whose map peaks below P is treated as not detected (default 0)"):
    """Where a heat-map recording's depths come from (`prepare`, `continuous`, `slam_scale`): --depths DIR, or --depth_from bones with
    --bones, --neck_depth and --min_peak; --peaks for the lift with depth files (not with peaks=False).  `depth_file`: the help of a
    `--depth FILE.npy` behind --depths, for a command that takes detections too; `depth_from`, `min_peak`: their help texts."""
    from .bone_depth import add_bone_depth_options
    p.add_argument("--depths", default=None, metavar="DIR", help="directory of per-frame depth .mat files")
    if depth_file is not None:
        p.add_argument("--depth", default=None, metavar="FILE.npy", help=depth_file)
    p.add_argument("--depth_from", default=None, choices=("bones",), help=depth_from)
    add_bone_depth_options(p)
    p.add_argument("--min_peak", type=float, default=None, metavar="P", help=min_peak)
    if peaks:
        p.add_argument("--peaks", default=None, choices=("argmax", "subpixel"), help="with --depths: lift at the reference's 16-pixel argmax "
                                                                                     "(default) or at the sub-pixel peak")


def depth_route_arguments(a, maps=True):
    """The parsed options that decide where the depths come from, as the keywords of the two routes: `depth`, `bones` (the file's array),
    `neck_depth`, and for heat-maps (`maps`; detections have neither) `min_peak` and `peaks`."""
    from .bone_depth import bones_from_args
    kw = dict(depth=a.depth_from, bones=bones_from_args(a), neck_depth=a.neck_depth)
    return dict(kw, min_peak=a.min_peak, peaks=getattr(a, "peaks", None)) if maps else kw


def check_depth_route_options(p, a):
    """The rules of `add_depth_route_options`, as parser errors."""
    if (a.depths is None) == (a.depth_from is None):
        p.error("give exactly one of --depths DIR and --depth_from bones")
    if a.depth_from is None and (a.bones is not None or a.neck_depth is not None or a.min_peak is not None):
        p.error("--bones, --neck_depth and --min_peak belong to --depth_from bones")
    if a.depth_from is not None and a.peaks == "argmax":
        p.error("--depth_from bones uses the sub-pixel peaks: --peaks argmax goes with --depths")
    if a.min_peak is not None and not (np.isfinite(a.min_peak) and a.min_peak >= 0):
        p.error("--min_peak must be a finite number >= 0")


def _parser():
    import argparse
    p = argparse.ArgumentParser(description="recording (.mat files of the pose network) -> chunks for the optimiser")
    p.add_argument("--heatmaps", required=True, help="directory of per-frame heatmap .mat files")
    add_depth_route_options(p)
    add_recording_options(p)
    return p


def _cli(argv=None):
    p = _parser()
    a = parse_recording_options(p, argv)
    check_depth_route_options(p, a)
    rec = prepare_sequence(a.slam, a.heatmaps, a.depths, total_start_frame=a.start, total_end_frame=a.end, fps=a.fps, mat_start_frame=a.mat_start,
                           test_size=a.test_size, out_root=a.out, camera_model_path=a.camera, **track_arguments(p, a), **depth_route_arguments(a))
    if a.optimize:
        from .whole_sequence import optimize_recording
        optimize_recording(rec, a.camera, ground_truth=a.scale is None)


if __name__ == "__main__":
    _cli()
