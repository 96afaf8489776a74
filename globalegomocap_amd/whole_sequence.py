"""Whole-sequence driver: every chunk directory of a sequence in ONE batched device call.

The reference's `optimize_whole_sequence.py` walks the chunk directories of a sequence (natsorted), calls
`main()` on each -- 12 windows, one after the other -- and averages the per-chunk error dicts
(`optimize_whole_sequence.py:48-118`).  Here the library reads the pickles itself (`parse_chunk` / `read_file` /
`gather_heat`: the heat-maps go file -> pinned memory -> HBM without becoming Python objects, loadmat's Fortran order and
float64 are undone by a kernel), all windows of a batch of chunks go through the optimiser together (BASELINE configs[1]: a
2000-frame sequence = 20 chunks = 240 windows per call), batches are pipelined (the next one's files arrive while this one
computes), and the per-chunk merge / smoothing / error report run on the device as well.  How bytes reach the device -- reader
threads, copy streams, pinned buffers -- is `staging`'s business; this module holds the chunk-file reader and the batch pipeline
(`_Pipeline`); what a chunk's report is and the files it may be written to are `report`'s.  Results, keys, printed summary and
the order in which the reparameterisation noise is drawn (chunk by chunk, window by window, local then global) follow the reference.

    python -m globalegomocap_amd.whole_sequence --data_path data/jian3

Chunks without ground truth (`prepare --scale`) go the same way with `ground_truth=False` /
`--ground_truth false`: nothing asks for `gt_global_skeleton`, and in place of the 18 errors every chunk gets the seven entries of
QUALITY_LINES from the device (`WindowEngine.sequence_quality`).  `save_pose=DIR` / `--save_pose DIR` writes the poses of every
chunk to `DIR/<chunk name>/result_pose.pkl` on either route; `save=True` / `--save true` writes every chunk's skeleton meshes under
`mesh_root` (`meshes`); `render=DIR` / `--render DIR` writes every chunk's frames as PNG images under DIR
(`render`); `render_camera=DIR` / `--render_camera DIR` writes every chunk as its camera saw it, the heat-maps
under the reprojected skeletons; `bvh=DIR` / `--bvh DIR` writes every chunk's sequences as BVH animation files
(`bvh`); `video=DIR` / `--video DIR` and `video_camera=DIR` / `--video_camera DIR` write the frames of `render` and
of `render_camera` as one Motion-JPEG clip per chunk, encoded on the device (`video`).

A chunk is the unit of everything here, as in the reference.  A recording as ONE motion -- every frame optimised, one world, one set of
files -- is `continuous.optimize_continuous` (`optimize_recording(..., continuous=True)`).
"""
import ctypes as C
import os
import pickle
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import _capi, staging
from .staging import (Laps, Scratch, cpus_near, drain, natural_key, reader_pool, report_stream, side_by_side, staging_buffer,      # noqa: F401  (cpus_near, natural_key: part of this module's interface)
                      thread_state)
from .optimizer import SequenceOptimizer, GLOBAL_VAE_PATH, LOCAL_VAE_PATH
from .report import (QUALITY_LINES, QUALITY_KEYS, SUMMARY_LINES, Outputs, batch_reports, chunk_reports, report_inputs, result_pose_dict,      # noqa: F401  (the three tables: part of this module's interface)
                     sequence_result)
from .sequence import SEQ_LEN, OVERLAP, window_starts


def list_chunks(data_dir):
    """Chunk directories in the reference's order (`natsorted(os.listdir(data_dir))`, directories only)."""
    names = sorted(os.listdir(data_dir), key=natural_key)
    return [os.path.join(data_dir, n) for n in names if os.path.isdir(os.path.join(data_dir, n))]


# ------------------------------------------------------------------------------------------------------------------ the chunk-file reader
KEYS = ("estimated_local_skeleton", "gt_global_skeleton", "camera_pose_list", "heatmap_list")     # read at optimizer.py:318-324, in this order
_K_EST, _K_GT, _K_CAM, _K_HEAT = range(4)
# A file crosses PCIe in slices of this size: the next one is read while the last one is on its way (4 and
# 32 MB slices measured within noise of 8).
SLICE_BYTES = 8 << 20
_PAD = 4096                      # file images are laid out on 4 KB boundaries, with at least 8 bytes of slack behind each
LOCATED, LISTED, RESIDENT = "located", "listed", "resident"          # how a chunk's heat-maps travel: ParsedChunk["heat_via"]

_C_KEYS = None


class ParsedChunk(dict):
    """One chunk as the pipeline sees it: "est_local" / "gt" / "cams" (dense float64 arrays), "n" frames, "heat_shape" (H, W, J)
    and "heat_via", which says how the heat-maps reach the device:

      LOCATED   `parse_chunk` found them in the file: "heat_offsets" (int64 [n]: where every heat-map's raw data lie),
                "heat_dtype", "heat_fortran", "file_bytes" -- they go file -> pinned memory -> HBM without passing through Python
                (`read_file` + `gather_heat`);
      LISTED    "heat_list", the un-pickled list (files outside the library reader's subset): stacked on the host (`stage_list`);
      RESIDENT  "heat", a float32 device tensor [n,H,W,J] (a `prepare.RecordingChunk`).

    Chunks read from a file also carry "path"."""


def parse_chunk(path, native=True, ground_truth=True):
    """`<chunk>/test_data.pkl` (optimizer.py:315-324) without its heat-maps' data: the small arrays dense, the heat-maps located.
    The library interprets the pickle itself (gem_chunk_open: no Python object per array, no GIL while it runs, nothing the file
    names is imported or called); a file outside its subset -- protocol 2, an entry that is no list of equally shaped float
    arrays -- is un-pickled the ordinary way instead.  KeyError on a missing key, like the reference.  ground_truth=False: the
    ground-truth key is not asked for (a file that has one is fine) and there is no "gt" entry."""
    global _C_KEYS
    file = os.path.join(path, "test_data.pkl")
    if native:
        lib = _capi.load_library()
        if _C_KEYS is None:
            _C_KEYS = {True: (C.c_char_p * len(KEYS))(*[k.encode() for k in KEYS]),
                       False: (C.c_char_p * (len(KEYS) - 1))(*[k.encode() for k in KEYS if k != KEYS[_K_GT]])}
        wanted = [(key, name) for key, name in zip(KEYS, ("est_local", "gt", "cams", None)) if ground_truth or name != "gt"]
        h = C.c_void_p()
        if lib.gem_chunk_open(os.fsencode(file), _C_KEYS[bool(ground_truth)], len(wanted), C.byref(h)) == 0:
            try:
                info = (C.c_int64 * 8)()
                c, ok = ParsedChunk(path=path, heat_via=LOCATED), True
                for k, (key, name) in enumerate(wanted):
                    _capi.check(lib.gem_chunk_info(h, k, info), lib)
                    n, ndim = int(info[0]), int(info[1])
                    if n < 0:
                        raise KeyError(key)
                    if ndim < 0 or (name is None and (n == 0 or ndim != 3)):
                        ok = False                    # ragged, or heat-maps that are not [H,W,J] arrays: the ordinary way
                        break
                    if name is not None:
                        c[name] = np.empty((n,) + tuple(info[4:4 + ndim]), dtype=np.float64)
                        if n:
                            _capi.check(lib.gem_chunk_gather_f64(h, k, c[name].ctypes.data, c[name].size), lib)
                    else:
                        offs = np.empty(n, dtype=np.int64)
                        _capi.check(lib.gem_chunk_offsets(h, k, offs.ctypes.data, n), lib)
                        c.update(n=n, heat_shape=tuple(int(v) for v in info[4:7]), heat_dtype=int(info[2]), heat_fortran=int(info[3]),
                                 heat_offsets=offs, file_bytes=int(lib.gem_chunk_bytes(h)))
                if ok:
                    return c
            finally:
                lib.gem_chunk_close(h)
    with open(file, "rb") as f:
        d = pickle.load(f)
    c = ParsedChunk(path=path, heat_via=LISTED, est_local=np.asarray(d["estimated_local_skeleton"], dtype=np.float64))
    if ground_truth:
        c["gt"] = np.asarray(d["gt_global_skeleton"], dtype=np.float64)
    c["cams"] = np.asarray(d["camera_pose_list"], dtype=np.float64)
    heat = d["heatmap_list"]
    c["heat_list"], c["n"] = heat, len(heat)
    c["heat_shape"] = tuple(np.shape(heat[0])) if len(heat) else (64, 64, 15)
    return c


def read_file(file, device, image, size=None):
    """`file` -> this reader thread's pinned staging buffer -> `image` (uint8 device tensor of at least the file's size + 8), in
    slices, on the thread's own stream (gem_file_stage; the GIL is free for the whole call).  Returns (event, file size): the
    image is complete once the event has passed."""
    lib = _capi.load_library()
    tl = thread_state(device)
    size = os.path.getsize(file) if size is None else size
    k, stage = staging_buffer(tl, size + 8)
    got = C.c_int64()
    rc = lib.gem_file_stage(os.fsencode(file), device.index if device.index is not None else torch.cuda.current_device(),
                            C.c_void_p(stage.data_ptr()), C.c_void_p(image.data_ptr()), min(stage.numel(), image.numel()), SLICE_BYTES,
                            C.byref(got), C.c_void_p(tl.stream.cuda_stream))
    ev = torch.cuda.Event()
    ev.record(tl.stream)
    tl.copied[k] = ev
    _capi.check(rc, lib)
    return ev, got.value


def gather_heat(image, image_len, offsets_d, n, shape, dtype, fortran, dest, stream=None):
    """`n` heat-maps of `shape` (H, W, J) out of a device image of their file(s), `image_len` bytes of it valid: ONE kernel
    (gem_heat_gather) on `stream` (default: the current one) picks the arrays out at `offsets_d` (int64 device tensor [n]), undoes
    loadmat's Fortran order (`fortran`) and rounds float64 (`dtype` 1) to float32 -> dest [n,H,W,J] float32."""
    lib = _capi.load_library()
    H, W, J = shape
    st = stream if stream is not None else torch.cuda.current_stream()
    _capi.check(lib.gem_heat_gather(C.c_void_p(image.data_ptr()), image_len, C.c_void_p(offsets_d.data_ptr()), n, H, W, J,
                                    dtype, fortran, C.c_void_p(dest.data_ptr()), C.c_void_p(st.cuda_stream)), lib)


def stage_list(c, device, dest=None):
    """The ordinary way for files the library's reader declined: the un-pickled heat-map list is stacked into this thread's pinned
    staging buffer and copied to `dest` (or a fresh tensor) on the thread's stream.  Returns (tensor, event)."""
    shape = (c["n"],) + tuple(c["heat_shape"])
    tl = thread_state(device)
    numel = int(np.prod(shape))
    heat = c.pop("heat_list")
    k, stage = staging_buffer(tl, numel * 4)
    view = stage[:numel * 4].view(torch.float32).view(shape)
    if numel:
        if isinstance(heat, (list, tuple)):
            np.stack(heat, out=view.numpy(), casting="same_kind")
        else:
            np.copyto(view.numpy(), np.asarray(heat), casting="same_kind")
    with torch.cuda.stream(tl.stream):
        if dest is not None and tuple(dest.shape) == tuple(shape) and dest.dtype == torch.float32:
            t = dest.copy_(view, non_blocking=True)
        else:
            t = view.to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(tl.stream)
    tl.copied[k] = ev
    return t, ev


def load_chunk(path, device=None, dest=None):
    """`<chunk>/test_data.pkl` as dense arrays: "est_local", "gt", "cams" float64, "heat" float32 [n,H,W,J] -- a numpy array, or
    with `device` a tensor there (`dest` when it has that shape) plus "heat_ready", the event after which it may be read; the
    copies run from the calling thread, on a stream of its own."""
    if device is None:
        c = parse_chunk(path, native=False)
        heat = c.pop("heat_list")
        c["heat"] = np.asarray(heat, dtype=np.float32).reshape((c["n"],) + tuple(c["heat_shape"]))
        return c
    c = parse_chunk(path)
    if c["heat_via"] == LISTED:
        c["heat"], c["heat_ready"] = stage_list(c, device, dest)
        return c
    tl = thread_state(device)
    shape = (c["n"],) + tuple(c["heat_shape"])
    with torch.cuda.stream(tl.stream):
        if tl.image is None or tl.image.numel() < c["file_bytes"] + 8:
            tl.image = torch.empty(c["file_bytes"] + (1 << 20), dtype=torch.uint8, device=device)
        read_file(os.path.join(path, "test_data.pkl"), device, tl.image, c["file_bytes"])
        t = dest if (dest is not None and tuple(dest.shape) == shape and dest.is_contiguous() and dest.dtype == torch.float32) else \
            torch.empty(shape, dtype=torch.float32, device=device)
        gather_heat(tl.image, c["file_bytes"], torch.from_numpy(c["heat_offsets"]).to(device), c["n"], c["heat_shape"], c["heat_dtype"],
                    c["heat_fortran"], t, tl.stream)
        ev = torch.cuda.Event()
        ev.record(tl.stream)
    c["heat"], c["heat_ready"] = t, ev
    return c


class ChunkStream:
    """Chunks in directory order, read `depth` ahead of the consumer by the reader threads: parsed (and with `device`, their
    heat-maps on their way to it) when they are handed out."""

    def __init__(self, paths, depth=8, workers=8, device=None):
        self._paths, self._depth, self._device = list(paths), max(1, depth), device
        self._readers = reader_pool("read", workers)
        self._pending, self._it = [], iter(self._paths)

    def prime(self):
        while len(self._pending) < self._depth:
            p = next(self._it, None)
            if p is None:
                break
            self._pending.append(self._readers.submit(load_chunk, p, self._device))
        return self

    def __iter__(self):
        pending = self._pending
        try:
            while True:
                self.prime()
                if not pending:
                    return
                yield pending.pop(0).result()          # a reader's exception (e.g. KeyError) surfaces here
        finally:
            drain(pending)


def _resident_chunk(c, ground_truth=True):
    """A `prepare.RecordingChunk` as the pipeline's ParsedChunk: the small arrays on the host (float64, the very values a pickle of
    them would hold), the heat-maps where they are.  ground_truth=False: `c.gt` is not looked at (it may be None)."""
    host = lambda t: np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64)      # noqa: E731
    heat = c.heat if hasattr(c.heat, "detach") else torch.as_tensor(np.asarray(c.heat, dtype=np.float32))
    heat = heat.to(torch.device("cuda", torch.cuda.current_device()), dtype=torch.float32).contiguous()
    p = ParsedChunk(heat_via=RESIDENT, est_local=host(c.est_local), cams=host(c.cams), n=int(heat.shape[0]),
                    heat_shape=tuple(heat.shape[1:]), heat=heat)
    if ground_truth:
        if c.gt is None:
            raise KeyError(KEYS[_K_GT])          # (what the chunk's pickle would raise)
        p["gt"] = host(c.gt)
    return p


def _save_pose(out_dir, report, smooth, locked=None):
    """`<out_dir>/result_pose.pkl` of one chunk (`report.result_pose_dict`); locked: the chunk's foot-locked sequence, with --foot_lock."""
    os.makedirs(out_dir, exist_ok=True)
    extra = {} if locked is None else {"locked": locked}
    with open(os.path.join(out_dir, "result_pose.pkl"), "wb") as f:
        pickle.dump(result_pose_dict(report.est, report.opt, report.mid, report.gt, smooth, **extra), f)


# ------------------------------------------------------------------------------------------------------------------ the batch pipeline
# device -> per batch in flight one slot, kept between calls: `frames`, the frame buffer its heat-maps are gathered into; `arena`, the
# images of its files side by side; `scratch`, the Scratch of its small uploads
_heat_pool = {}
_noise_pool = {}
N_BUFFERS = 3                     # batches in flight: one computing, one arriving, one being reported


def _draw_noise(rows, D, slot=0):
    """One `torch.randn(rows[k], D)` per chunk from the global generator, in order (optimizer.py:261: `torch.randn_like` per
    stage call; D5) -- drawn straight into consecutive slices of ONE pinned buffer that is kept between calls (one per batch in
    flight, `slot`): a fresh 0.4 MB tensor per chunk plus their concatenation cost more in first-touch page faults (5 ms per
    240 windows) than in arithmetic, and the pinned block goes to the device in one asynchronous copy.  Returns the block
    [sum(rows), D]."""
    total = int(sum(rows))
    key = (D, torch.get_default_dtype(), slot)
    buf = _noise_pool.get(key)
    if buf is None or buf.shape[0] < total:
        buf = torch.empty(max(total, 1), D)
        if torch.cuda.is_available():
            buf = buf.pin_memory()
        _noise_pool[key] = buf
    r0 = 0
    for r in rows:
        if r:
            torch.randn(r, D, out=buf[r0:r0 + r])
        r0 += r
    return buf[:total]


_Source = namedtuple("_Source", "group what name")          # a chunk of sequence `group`: a chunk directory or a prepare.RecordingChunk; `name` is what verbose=True prints


class _Batch:
    """One device call's worth of chunks on its way through the pipeline (see _Pipeline)."""
    __slots__ = ("index", "sources", "parsing", "chunks", "reading", "images", "noise", "pending", "counts", "prep", "heat", "dests",
                 "listed", "offsets", "report", "weights", "done", "heat_d", "frame_lo")

    def __init__(self, index, sources):
        self.index, self.sources = index, sources
        self.parsing = self.chunks = self.reading = self.images = self.noise = self.pending = self.report = None


def _settings(camera_model_path, vae_weight=0.0, gmm_weight=0.0, smoothness_weight=0.001, bone_length_weight=0.01, weight_3d=0.01,
              reproj_weight=0.01, final_smooth=True, merge=True, global_vae_path=GLOBAL_VAE_PATH, local_vae_path=LOCAL_VAE_PATH,
              chunks_per_batch=None, optimizer=None, device_metrics=True, verbose=True, seq_len=SEQ_LEN, overlap=OVERLAP, timings=None,
              per_sequence=False, ground_truth=True, save_pose=None, save=False, mesh_root="out", render=None, render_camera=None, bvh=None,
              bvh_fps=None, *, video=None, video_camera=None, video_fps=None, video_quality=None, upright=False, foot_height=None,
              foot_lock=False, foot_lock_stretch=None, foot_lock_blend=None, gltf=None, gltf_fps=None):
    """The arguments of `optimize_sequences` / `optimize_recordings` behind the sequences themselves, as one object; `outputs`: the
    files asked for (`report.Outputs`, checked here).  The clip arguments, `upright` / `foot_height`, `foot_lock` with its two
    options and `gltf` / `gltf_fps` go by keyword only.
    (`gmm_weight` and `merge` are accepted and unused, as in the reference: SURVEY D4.)"""
    if foot_height is not None and not np.isfinite(foot_height):
        raise ValueError("foot_height must be a finite number of metres, got %r" % (foot_height,))
    if foot_lock_stretch is not None and not (np.isfinite(foot_lock_stretch) and foot_lock_stretch >= 0):
        raise ValueError("foot_lock_stretch must be a finite number that is not negative, got %r" % (foot_lock_stretch,))
    if foot_lock_blend is not None and not foot_lock_blend >= 1:
        raise ValueError("foot_lock_blend must be at least one frame, got %r" % (foot_lock_blend,))
    if gltf_fps is not None and not (np.isfinite(gltf_fps) and gltf_fps > 0):
        raise ValueError("gltf_fps must be a finite positive number, got %r" % (gltf_fps,))
    outputs = Outputs(mesh_root if save else None, render, render_camera, bvh, bvh_fps, video, video_camera, video_fps, video_quality,
                      upright=upright if upright else None, upright_foot_height=foot_height if upright else None,
                      **(dict(foot_lock=True, foot_lock_stretch=foot_lock_stretch, foot_lock_blend=foot_lock_blend) if foot_lock else {}),
                      **(dict(gltf=gltf, gltf_fps=gltf_fps) if gltf is not None else {}))
    outputs.check()
    if not ground_truth and not device_metrics:
        raise ValueError("ground_truth=False: the report without ground truth is computed on the device only (device_metrics=True)")
    return SimpleNamespace(**locals())


class _Pipeline:
    """The private driver behind `optimize_sequences` and `optimize_recordings`: `groups[g]` are the chunk sources (_Source) of
    sequence g.  It holds one call's batches and what their stages share: the settings, the optimiser, the device's buffers
    (`slots`: one per batch in flight, see `_heat_pool`), the reader pools, every future handed to a pool, and the ChunkReports filed per
    sequence.

    Per batch: `start` (its files start moving), `prepare` (everything that needs neither the heat-maps nor the device's
    attention), `fire` (gathers + the optimiser's call enqueued), `finish` (results read back and reported).  `run` interleaves
    them so that the device never waits for the host."""

    def __init__(self, groups, cfg, lap):
        self.cfg, self.lap, self.opt = cfg, lap, cfg.optimizer
        n = cfg.chunks_per_batch
        spans = groups if cfg.per_sequence else [[s for g in groups for s in g]]          # a batch does not cross these
        lists = [g[i:i + (n or len(g))] for g in spans for i in range(0, len(g), n or len(g))]
        self.batches = [_Batch(i, l) for i, l in enumerate(lists)]
        self.reports = [[] for _ in groups]
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.parse_pool, self.read_pool = reader_pool("parse", 8), reader_pool("read", 8, cpus_near(self.device))
        self.noise_pool = reader_pool("noise", 1)
        self.slots = _heat_pool.setdefault(self.device, [SimpleNamespace(frames=None, arena=None, scratch=Scratch(self.device)) for _ in range(N_BUFFERS)])
        self.submitted = []                          # every future handed to a pool (drained on the way out, whatever happens)

    def slot(self, b):
        return self.slots[b.index % N_BUFFERS]

    def start(self, b):
        """Batch b's files start moving: read tasks (they need the files' sizes only) and, beside them, the parse tasks.  A
        Recording's chunks are on the device already: nothing is read or parsed."""
        if b.reading is not None:
            return
        if not isinstance(b.sources[0].what, str):
            b.reading, b.images, b.chunks = [], [], [_resident_chunk(s.what, self.cfg.ground_truth) for s in b.sources]
            return
        files = [os.path.join(s.what, "test_data.pkl") for s in b.sources]
        sizes = [os.path.getsize(f) for f in files]          # (FileNotFoundError here, like the reference's open())
        at, room, total = side_by_side(sizes, _PAD)
        slot = self.slot(b)
        if slot.arena is None or slot.arena.numel() < total:
            slot.arena = None
            slot.arena = torch.empty(total, dtype=torch.uint8, device=self.device)
        b.images = [slot.arena[o:o + r] for o, r in zip(at.tolist(), room.tolist())]
        b.reading = [self.read_pool.submit(read_file, f, self.device, img, sz) for f, img, sz in zip(files, b.images, sizes)]
        b.parsing = [self.parse_pool.submit(parse_chunk, s.what, True, self.cfg.ground_truth) for s in b.sources]
        self.submitted.extend(b.reading + b.parsing)

    def prepare(self, b):
        """Everything of batch b that needs neither its heat-maps nor the device's attention: parses awaited, window tables, the
        small arrays on their way to the device, the noise being drawn, the report's result-independent half."""
        cfg, lap = self.cfg, self.lap
        self.start(b)
        if b.parsing is not None:
            b.chunks = [f.result() for f in b.parsing]            # (KeyError etc. surface here)
        lap("wait for the parses")
        starts, chunk_of, bounds, f_off = [], [], [], 0
        for ci, (c, src) in enumerate(zip(b.chunks, b.sources)):
            if cfg.verbose:
                print("running data: {}".format(src.name))
            s = window_starts(len(c["est_local"]), cfg.seq_len, cfg.overlap)
            c["starts"] = s
            starts.append(s + f_off)
            chunk_of.append(np.full(len(s), ci, dtype=np.int64))
            bounds.append((f_off, f_off + len(c["est_local"])))
            f_off += len(c["est_local"])
        n_win = int(sum(len(s) for s in starts))
        if self.opt is None:
            self.opt = SequenceOptimizer(cfg.camera_model_path, cfg.global_vae_path, cfg.local_vae_path, max_windows=max(n_win, 1),
                                         seq_len=cfg.seq_len)
        if n_win > self.opt.engine.max_windows:
            raise ValueError("%d windows in one batch exceed the engine's max_windows=%d: pass chunks_per_batch" %
                             (n_win, self.opt.engine.max_windows))
        b.noise = self.noise_pool.submit(_draw_noise, [2 * len(c["starts"]) for c in b.chunks], self.opt.engine.D, b.index % N_BUFFERS)
        self.submitted.append(b.noise)
        b.listed = [(i, self.read_pool.submit(stage_list, c, self.device)) for i, c in enumerate(b.chunks) if c["heat_via"] == LISTED]
        self.submitted.extend(f for _, f in b.listed)      # (files the library's reader declined: stacked on the host)
        b.weights = self.opt.stage_weights(cfg.vae_weight, cfg.smoothness_weight, cfg.bone_length_weight, cfg.weight_3d, cfg.reproj_weight)
        est_cat = np.concatenate([c["est_local"] for c in b.chunks])
        cams_cat = np.concatenate([c["cams"] for c in b.chunks])
        b.counts = [len(c["starts"]) for c in b.chunks]
        b.frame_lo = np.array([lo for lo, _ in bounds], dtype=np.int64)
        lap("window tables")
        slot = self.slot(b)
        slot.scratch.reset(len(est_cat) * (45 * 4 + 16 * 8 + 8 + 3 * 45 * 8) + 16 * n_win + 8192)
        b.prep = self.opt.prepare(est_cat, cams_cat, np.concatenate(starts), np.concatenate(chunk_of), bounds, timings=cfg.timings,
                                  upload=slot.scratch.upload)
        # the batch's frame buffer (one shape of heat-map: the chunks' frames side by side)
        frames = sum(c["n"] for c in b.chunks)
        shapes = {tuple(c["heat_shape"]) for c in b.chunks}
        b.heat, b.dests = None, [None] * len(b.chunks)
        if len(shapes) == 1 and frames:
            hs = next(iter(shapes))
            if slot.frames is None or slot.frames.shape[0] < frames or tuple(slot.frames.shape[1:]) != hs:
                slot.frames = None
                slot.frames = torch.empty((frames,) + hs, dtype=torch.float32, device=self.device)
            b.heat = slot.frames[:frames]
            b.dests = [b.heat[lo:hi] for lo, hi in bounds]
        # (where every heat-map's raw data lie in the ARENA of file images: the file's place in the arena + the array's place in the file)
        located = [c["heat_offsets"] + (b.images[i].data_ptr() - slot.arena.data_ptr()) for i, c in enumerate(b.chunks) if c["heat_via"] == LOCATED]
        b.offsets = slot.scratch.upload(np.concatenate(located), torch.int64) if located else None
        lap("small uploads")
        b.report = None
        if cfg.device_metrics and b.counts and min(b.counts) == max(b.counts) and b.counts[0] > 0:
            b.report = report_inputs(b.chunks, starts, est_cat, cams_cat, cfg.seq_len, cfg.overlap, slot.scratch.upload, cfg.ground_truth)
        lap("report preparation")

    def fire(self, b):
        """Batch b goes to the device: its files' last copies awaited (issued, not finished), the heat-maps gathered into the frame
        buffer by the way they travel, the optimiser's call enqueued behind them.  Nothing waits for the device."""
        lap, timings = self.lap, self.cfg.timings
        eps = b.noise.result()
        lap("wait for the noise")
        cur = torch.cuda.current_stream()
        at, parts = 0, [None] * len(b.chunks)
        located = [i for i, c in enumerate(b.chunks) if c["heat_via"] == LOCATED]
        for i in located:
            ev, _ = b.reading[i].result()             # (the file's last copy has been issued: its event is recorded)
            cur.wait_event(ev)
        arena = self.slot(b).arena
        kinds = {(b.chunks[i]["heat_dtype"], b.chunks[i]["heat_fortran"], tuple(b.chunks[i]["heat_shape"])) for i in located}
        if b.heat is not None and len(located) == len(b.chunks) and len(kinds) == 1 and len(b.heat) <= 65535:
            # every chunk's file image lies in ONE arena and their frames side by side in the batch's frame buffer: one launch picks all
            # heat-maps out (b.offsets was built relative to the arena in prepare())
            dtype, fortran, shape = next(iter(kinds))
            gather_heat(arena, arena.numel(), b.offsets, len(b.heat), shape, dtype, fortran, b.heat, cur)
        else:
            for i in located:
                c = b.chunks[i]
                parts[i] = b.dests[i] if b.dests[i] is not None else torch.empty((c["n"],) + tuple(c["heat_shape"]), dtype=torch.float32, device=self.device)
                base = b.images[i].data_ptr() - arena.data_ptr()
                gather_heat(arena, base + c["file_bytes"], b.offsets[at:at + c["n"]], c["n"], c["heat_shape"], c["heat_dtype"], c["heat_fortran"],
                            parts[i], cur)
                at += c["n"]
        for i, f in b.listed:
            t, ev = f.result()
            cur.wait_event(ev)
            t.record_stream(cur)
            parts[i] = b.dests[i].copy_(t) if b.dests[i] is not None else t
        for i, c in enumerate(b.chunks):
            if c["heat_via"] == RESIDENT:             # device to device
                parts[i] = b.dests[i].copy_(c["heat"]) if b.dests[i] is not None else c["heat"]
        lap("wait for the readers")
        if b.index + 1 < len(self.batches):          # the next batch's files start moving behind this batch's last copy: they arrive
            self.start(self.batches[b.index + 1])    # while this batch is on the device
        if timings is not None and timings.get("_synchronise"):          # developer timing only: separates the PCIe tail from the optimiser's time
            cur.synchronize()
            lap("h2d tail (timing runs only: synchronised)")
        heat_d = b.heat if b.heat is not None else (parts[0] if len(parts) == 1 else torch.cat(parts))
        b.heat_d = heat_d
        b.pending = self.opt.fire(b.prep, heat_d, b.weights[0], b.weights[1], eps=eps, timings=timings)
        b.done = torch.cuda.Event()
        b.done.record(cur)
        lap("enqueue")

    def finish(self, b):
        """Batch b's results: waits for the device, merges / smooths / scores on it, writes the files asked for and files the chunks'
        reports per sequence."""
        # on a stream of its own, behind the batch's LAST kernel only: on the optimiser's stream the read-back would queue up
        # behind the next batch's whole device call, which is already enqueued there
        cfg, lap, e = self.cfg, self.lap, self.opt.engine
        rs = report_stream(self.device)
        rs.wait_event(b.done)
        for t in b.pending:
            if t is not None:
                t.record_stream(rs)
        with torch.cuda.stream(rs):
            mid_local, opt_global, _ = self.opt.collect(b.pending, keep_device=True)
            b.pending = None
            lap("wait for the device + stats")
            mid_np = mid_local.cpu().numpy()
            lap("report: stage-one poses to the host")
            frames = None
            if not cfg.ground_truth:
                # the report without ground truth reads the batch's frame buffers (its slot's, which batch k+3 fills again): its rows
                # are read back here, like the error rows
                heat_d, mb = b.heat_d.contiguous(), b.prep["mean_bone_chunks"].contiguous()
                frames = (b.prep["cams"], heat_d, torch.from_numpy(b.frame_lo).to(self.device), mb)
                for t in (heat_d, mb):
                    t.record_stream(rs)
            if b.report is not None:
                reports = batch_reports(e, b.report, mid_np, opt_global, len(b.chunks), cfg.overlap, bool(cfg.final_smooth),
                                        upload=self.slot(b).scratch.upload, lap=lap, frames=frames, want_mid=cfg.save_pose is not None)
            else:
                reports = chunk_reports(e, b.chunks, mid_np, opt_global, cfg.seq_len, cfg.overlap, bool(cfg.final_smooth), cfg.device_metrics,
                                        frames)
            view_heat, view_cams = None, None
            if cfg.outputs.needs_frames:
                # the camera's view reads the batch's frame buffers too; its files are complete (the device has read the frames) before
                # this returns, three batches before the slot's frame buffer is filled again
                view_heat, view_cams = b.heat_d.contiguous(), b.prep["cams"]
                for t in (view_heat, view_cams):
                    t.record_stream(rs)
            b.heat_d = None
            for ci, (src, r) in enumerate(zip(b.sources, reports)):
                if r is not None:
                    name = os.path.normpath(src.name)
                    lock = cfg.outputs.lock(e, r.sequences()[1])          # (--foot_lock: None without it)
                    found = cfg.outputs.write(e, name, r.sequences(), view_cams, view_heat, int(b.frame_lo[ci]), **({} if lock is None else {"locked": lock}))
                    if lock is not None:          # (the chunk's foot-lock record, beside its errors)
                        r.result["foot_lock"] = lock.as_dict()
                        if cfg.verbose:
                            print("{}: {}".format(src.name, lock.line()))
                    if found is not None:          # (--upright: the chunk's ground record, beside its errors)
                        r.result["ground"] = found.as_dict()
                        if cfg.verbose:
                            print("{}: {}".format(src.name, found.line()))
                    r.drop_views()          # (they alias this batch's slot, which batch k+3 fills again)
                    self.reports[src.group].append(r)
                    if cfg.save_pose is not None:
                        _save_pose(os.path.join(cfg.save_pose, os.path.basename(name)), r, bool(cfg.final_smooth),
                                   **({} if lock is None else {"locked": lock.sequence.cpu().numpy()}))
                    if cfg.ground_truth and cfg.verbose and \
                            r.result["bone_length_aligned_optimized_mpjpe"] > r.result["bone_length_aligned_mid_optimized_mpjpe"]:
                        print(r.result)
            lap("report: result dicts" if b.report is not None else "sequences + reports")

    def run(self, titles):
        """Every batch through its stages.  -> one `optimize_directory` result per sequence (`titles[g]`: sequence g's name in the
        printed summary)."""
        self.lap("plan")
        try:
            prev = None
            for b in self.batches:
                self.prepare(b)               # while batch k-1 is on the device and batch k's files are arriving ...
                self.fire(b)                  # ... batch k is enqueued behind it as soon as its last file has been sent ...
                if prev is not None:
                    self.finish(prev)         # ... and only then batch k-1's report is read back: the device never waits for the host
                    prev.chunks = prev.reading = prev.parsing = prev.images = prev.report = prev.prep = None
                prev = b
            self.finish(prev)
        finally:
            drain(self.submitted)
            if any(b.pending is not None for b in self.batches):
                torch.cuda.synchronize()      # (an exception left device work behind that reads this call's buffers)
        self.lap("readers drained")
        out = [sequence_result(reports, title if len(titles) > 1 else None, self.cfg.verbose) for reports, title in zip(self.reports, titles)]
        self.lap("summaries")
        return out


def optimize_sequences(data_dirs, camera_model_path, *args, **kwargs):
    """Several sequences through the device: the chunks of every directory of `data_dirs`, `chunks_per_batch` per device call
    (default: all of them in ONE call -- BASELINE configs[2]: all test sequences concurrently on one GPU; per_sequence=True: one
    call per directory), the reports per sequence.  Returns a list of (summary, per-chunk error dicts, estimated_pose,
    optimized_pose, gt_pose), one per directory, each exactly what `optimize_directory` returns; the noise is drawn sequence by
    sequence, chunk by chunk.

    The files cross PCIe as they are (`read_file`: file -> pinned memory -> an image of the file in HBM, on 8 reader threads,
    nothing of it passing through Python) WHILE the library interprets the pickles on other threads (`parse_chunk`), the noise
    is drawn on a thread of its own (same generator, same order: D5) and the main thread uploads the small arrays; one kernel
    per chunk then picks the heat-maps out of the images (`gather_heat`).  Batches are pipelined: batch k+1's files are read
    behind batch k's, so they arrive while batch k is on the device, and batch k+1 is enqueued before batch k's report is read
    back.  The frame buffers, file-image arenas, noise blocks and reader threads this module keeps between calls (about 1 GB
    of HBM and 0.4 GB of pinned host memory per 2000-frame batch in flight, at most three) are shared by all calls of the
    process without locking -- one call at a time -- and are given back by `release_pools()`.

    Further arguments, positional or by keyword, in this order (defaults: `_settings`): vae_weight, gmm_weight, smoothness_weight,
    bone_length_weight, weight_3d, reproj_weight, final_smooth, merge, global_vae_path, local_vae_path, chunks_per_batch, optimizer,
    device_metrics, verbose, seq_len, overlap, timings, per_sequence, ground_truth, save_pose, save, mesh_root, render, render_camera,
    bvh, bvh_fps; and by keyword only: video, video_camera, video_fps, video_quality, upright, foot_height, foot_lock,
    foot_lock_stretch, foot_lock_blend, gltf, gltf_fps.

    ground_truth=False: the chunks carry no ground truth (`prepare` with a scale).  Their pickles are not asked for
    `gt_global_skeleton`, every chunk's report is the seven entries of QUALITY_KEYS (`WindowEngine.sequence_quality` on the estimated
    and on the optimised sequence, device only), the summary their mean over the chunks, and `gt_pose` is None.
    save_pose=DIR: `DIR/<chunk name>/result_pose.pkl` per chunk with the reference's keys and containers (optimizer.py:469-483):
    estimated_pose, optimized_pose, mid_optimized_pose and, where there is one, gt_pose.
    save=True: every chunk's skeleton meshes (optimizer.py:485-504) as `<mesh_root>/<dataset>/<chunk>/{optimized_global_aligned,
    input_global_aligned,gt_global_aligned}/out_%04d.ply`, one file per merged frame, the first two sequences aligned to the third
    over the chunk (`meshes.write_meshes`; mesh_root defaults to the reference's `out` under the working directory).  With
    ground_truth=False: `optimized_global` and `input_global`, unaligned.  Results and reports do not depend on it.
    render=DIR: every chunk's frames as `DIR/<dataset>/<chunk>/frame_%04d.png`, the estimated (red), the optimised (blue) and the
    ground-truth sequence (green) overlaid, the first two aligned to the third, and one `overview_<name>.png` per sequence with all
    its frames (`render.write_result_frames`, rendered on the device).  With ground_truth=False: two sequences, unaligned.  Results
    and reports do not depend on it.
    render_camera=DIR: every chunk as its camera saw it, `DIR/<dataset>/<chunk>/camera_%04d.png`: the frame's heat-maps under the
    estimated (red), the optimised (blue) and the ground-truth sequence (green, moved onto the optimised one by one similarity: it
    lives in the studio's frame), projected with the reprojection term's arithmetic (`render.write_result_camera_frames`, from the
    batch's frame buffers on the device).  DIR may be `render`'s DIR.  Results and reports do not depend on it.
    bvh=DIR: every chunk as animation, `DIR/<dataset>/<chunk>/{estimated,optimized,gt}.bvh` at `bvh_fps` frames per second (default
    25): a 19-node skeleton with the chunk's mean bone lengths and every frame keyed, the first two sequences aligned to the third
    (`bvh.write_result_bvh`, made on the device).  With ground_truth=False: two files, unaligned.  Results and reports do not
    depend on it.
    video=DIR: every chunk's frames -- the view and overlay of `render`, without the overviews -- as one Motion-JPEG clip,
    `DIR/<dataset>/<chunk>/frames.avi`; video_camera=DIR: the images of `render_camera` as `.../camera.avi`.  Neither needs the PNG
    option: without it no PNG file is written.  Both play at `video_fps` frames per second (default 25) and are encoded on the device
    at JPEG quality `video_quality` (default 90; `report.Outputs`).  Results and reports do not depend on them.
    upright=True: the meshes, frames, clip and BVH files of every chunk stand upright on the ground estimated from the chunk's foot
    contacts -- Y up, the floor at 0, the wearer at the origin facing +Z in the first frame -- (`ground.estimate_ground`, DESIGN.md
    section 6m; foot_height: metres a standing foot point lies above the floor, default 0).  Every chunk's report dict then has the
    entry `ground` (`GroundEstimate.as_dict`), and one line per chunk is printed; the summary does not change.
    foot_lock=True: the meshes, frames, clip and BVH files show the optimised sequence with its standing feet pinned to the floor and
    the legs re-solved by two-bone inverse kinematics (`foot_lock.lock_feet`; foot_lock_stretch: how much longer
    a straight leg may become to hold its pin, default 0.05; foot_lock_blend: frames over which a correction is eased in and out,
    default 0.12 s at `bvh_fps`); the estimated sequence stays as it is.  Every chunk's report dict then has the entry `foot_lock`
    (`FootLock.as_dict`), one line per chunk is printed, and result_pose.pkl holds `foot_locked_pose`.  The returned poses, the
    errors and the report are those of the optimiser's own sequence.
    gltf=DIR: every chunk as ONE glTF binary file, `DIR/<dataset>/<chunk>/result.glb`: the estimated (red), the optimised (blue) and the
    ground-truth sequence (green) as skinned meshes on the BVH files' skeleton, the first two aligned to the third, all driven by one
    animation keyed at every frame at `gltf_fps` keys per second (default 25; `gltf.write_result_gltf`, made on the device, DESIGN.md
    section 6p).  With ground_truth=False: two skeletons, unaligned.  `upright` and `foot_lock` apply to it as to the BVH files.
    Results and reports do not depend on it."""
    cfg = _settings(camera_model_path, *args, **kwargs)
    lap = Laps(cfg.timings, log=True)          # developer timing (tools/whole_sequence_timing.py): wall time of the main thread's phases
    groups = []
    for gi, d in enumerate(data_dirs):
        groups.append([_Source(gi, q, q) for q in list_chunks(d)])
        if not groups[-1]:
            raise FileNotFoundError("no chunk directories under %s" % d)
    return _Pipeline(groups, cfg, lap).run(data_dirs)


def optimize_directory(data_dir, camera_model_path, *args, **kwargs):
    """One sequence = the reference's `optimize_whole_sequence.py`.  Returns (summary OrderedDict, per-chunk error
    dicts, estimated_pose, optimized_pose, gt_pose) -- the three pose sequences are the concatenations
    `optimize_whole_sequence.py:65-67` builds, as arrays [frames,15,3].  Arguments as `optimize_sequences`."""
    return optimize_sequences([data_dir], camera_model_path, *args, **kwargs)[0]


def optimize_recordings(recordings, camera_model_path, *args, **kwargs):
    """`optimize_sequences` for recordings that `prepare.prepare_sequence` left on the device: same keyword arguments, return
    value and printed summary, one entry per `Recording`; no pickle is written or read.  The optimiser is handed the same
    float32 heat-maps, float64 skeletons and cameras that `Recording.write_chunks` + `optimize_sequences` would hand it, so
    the results are bitwise those."""
    cfg = _settings(camera_model_path, *args, **kwargs)
    lap = Laps(cfg.timings, log=True)
    titles = ["recording_%d" % gi for gi in range(len(recordings))]
    groups = []
    for gi, r in enumerate(recordings):
        if not len(r):
            raise FileNotFoundError("a recording without chunks")
        groups.append([_Source(gi, c, os.path.join(titles[gi], c.name)) for c in r.chunks])
    return _Pipeline(groups, cfg, lap).run(titles)


def optimize_recording(recording, camera_model_path, *args, continuous=False, stride=None, **kwargs):
    """One `prepare.Recording` = `optimize_directory` on the chunks it would write.  Arguments and result as there.  continuous=True (by
    keyword, with `stride`): the recording as ONE motion instead, every frame optimised in one world (`continuous.optimize_continuous`,
    DESIGN.md section 6s)."""
    if continuous:
        from .continuous import optimize_continuous
        return optimize_continuous(recording, camera_model_path, *args, **({} if stride is None else {"stride": stride}), **kwargs)
    if stride is not None:
        raise ValueError("stride belongs to continuous=True")
    return optimize_recordings([recording], camera_model_path, *args, **kwargs)[0]


def release_pools():
    """Give back what this module keeps between calls: the per-device frame buffers the readers fill, the pinned noise
    blocks and the mesh and frame writers' buffers, then (`staging.release`) the streams and the reader threads with their pinned staging buffers and device images.
    Not to be called while another call is in flight."""
    from . import bvh, gltf, meshes, render, video
    _heat_pool.clear()
    _noise_pool.clear()
    meshes.release()
    render.release()
    bvh.release()
    gltf.release()
    video.release()
    staging.release()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _truthy(x):
    """The reference's own flag parser."""
    return str(x).lower() == "true"


def _parser():
    import argparse
    from .camera import DEFAULT_CALIBRATION
    p = argparse.ArgumentParser(description="Data directory number")
    p.add_argument("--data_path", required=True, type=str)
    p.add_argument("--camera", type=str, default=DEFAULT_CALIBRATION)
    add_weight_options(p)
    add_output_options(p)
    p.add_argument("--final_smooth", default=True, type=_truthy)
    p.add_argument("--merge", default=True, type=_truthy)
    p.add_argument("--chunks_per_batch", type=int, default=None, help="chunks optimised per device call (default: all)")
    p.add_argument("--ground_truth", default=True, type=_truthy, help="false: chunks without gt_global_skeleton, the report without ground truth")
    p.add_argument("--save_pose", default=None, metavar="DIR", help="write DIR/<chunk name>/result_pose.pkl per chunk")
    return p


def add_weight_options(p):
    """The energy weights of a command line that optimises (`whole_sequence`, `continuous`), the reference's flags."""
    p.add_argument("--vae", type=float, default=0.00)
    p.add_argument("--gmm", type=float, default=0.00)
    p.add_argument("--smooth", type=float, default=0.001)
    p.add_argument("--bone_length", type=float, default=0.01)
    p.add_argument("--weight_3d", type=float, default=0.01)
    p.add_argument("--reproj_weight", type=float, default=0.01)


def add_output_options(p):
    """The files a command line that optimises may write, and how: the options of `report.Outputs` (`check_output_options`,
    `output_arguments`)."""
    p.add_argument("--save", default=False, type=_truthy, help="true: write every chunk's skeleton meshes (PLY) under --mesh_root")
    p.add_argument("--mesh_root", default="out", metavar="DIR", help="where --save true writes <dataset>/<chunk>/<folder>/out_%%04d.ply")
    p.add_argument("--render", default=None, metavar="DIR", help="write every chunk's frames as DIR/<dataset>/<chunk>/frame_%%04d.png")
    p.add_argument("--render_camera", default=None, metavar="DIR",
                   help="write every chunk as its camera saw it, DIR/<dataset>/<chunk>/camera_%%04d.png: heat-maps under the reprojected skeletons")
    p.add_argument("--bvh", default=None, metavar="DIR", help="write every chunk as animation, DIR/<dataset>/<chunk>/{estimated,optimized,gt}.bvh")
    p.add_argument("--bvh_fps", default=None, type=float, metavar="F", help="frames per second of the --bvh files (default 25)")
    p.add_argument("--gltf", default=None, metavar="DIR",
                   help="write every chunk as one glTF binary file of skinned, animated skeletons, DIR/<dataset>/<chunk>/result.glb")
    p.add_argument("--gltf_fps", default=None, type=float, metavar="F", help="keys per second of the --gltf files (default 25)")
    p.add_argument("--video", default=None, metavar="DIR", help="write every chunk's frames as one Motion-JPEG clip, DIR/<dataset>/<chunk>/frames.avi")
    p.add_argument("--video_camera", default=None, metavar="DIR", help="write every chunk as its camera saw it as one clip, DIR/<dataset>/<chunk>/camera.avi")
    p.add_argument("--video_fps", default=None, type=float, metavar="F", help="frames per second of the clips (default 25)")
    p.add_argument("--video_quality", default=None, type=int, metavar="Q", help="JPEG quality of the clips, 1 .. 100 (default 90)")
    p.add_argument("--upright", default=False, type=_truthy,
                   help="true: the meshes, frames, clip and BVH files stand upright on the ground estimated from every chunk's foot contacts")
    p.add_argument("--foot_height", default=None, type=float, metavar="M", help="with --upright true: metres a standing foot point lies above the floor (default 0)")
    p.add_argument("--foot_lock", default=False, type=_truthy,
                   help="true: the meshes, frames, clip and BVH files show the optimised sequence with its standing feet pinned and the legs re-solved")
    p.add_argument("--foot_lock_stretch", default=None, type=float, metavar="S",
                   help="with --foot_lock true: how much longer a straight leg may become to hold its pin (default 0.05)")
    p.add_argument("--foot_lock_blend", default=None, type=int, metavar="FRAMES",
                   help="with --foot_lock true: frames over which a correction is eased in and out (default: 0.12 s)")


def check_output_options(p, a):
    """The rules of `add_output_options`, as parser errors."""
    if a.video_fps is not None and not a.video_fps > 0:
        p.error("argument --video_fps: must be positive")
    if a.video_quality is not None and not 1 <= a.video_quality <= 100:
        p.error("argument --video_quality: a whole number 1 .. 100")
    if a.gltf_fps is not None and not (np.isfinite(a.gltf_fps) and a.gltf_fps > 0):
        p.error("argument --gltf_fps: must be positive")


def output_arguments(a):
    """The parsed options of `add_output_options` as keyword arguments of `optimize_sequences`."""
    return dict(save=a.save, mesh_root=a.mesh_root, render=a.render, render_camera=a.render_camera, bvh=a.bvh, bvh_fps=a.bvh_fps, video=a.video,
                video_camera=a.video_camera, video_fps=a.video_fps, video_quality=a.video_quality,
                **(dict(upright=True, foot_height=a.foot_height) if a.upright else {}),
                **(dict(foot_lock=True, foot_lock_stretch=a.foot_lock_stretch, foot_lock_blend=a.foot_lock_blend) if a.foot_lock else {}),
                **(dict(gltf=a.gltf, gltf_fps=a.gltf_fps) if a.gltf is not None else {}))


def _cli(argv=None):
    p = _parser()
    a = p.parse_args(argv)
    check_output_options(p, a)
    optimize_directory(a.data_path, a.camera, a.vae, a.gmm, a.smooth, a.bone_length, a.weight_3d, a.reproj_weight,
                       final_smooth=a.final_smooth, merge=a.merge, chunks_per_batch=a.chunks_per_batch, ground_truth=a.ground_truth,
                       save_pose=a.save_pose, **output_arguments(a))


if __name__ == "__main__":
    _cli()
