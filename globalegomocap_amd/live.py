"""Live mode: a stream optimised window by window as its frames arrive.

A `LiveOptimizer` takes frames as they come, optimises each 10-frame window the moment its tenth frame is there -- both stages of
`WindowEngine.optimize_windows` with B = 1, one captured-graph replay per window -- and hands back finished global poses eight
frames at a time:

    live = LiveOptimizer(camera_json, global_vae, local_vae, scale=1.0)
    for frame in rig:                                   # a head-mounted rig calls push itself
        got = live.push(heat=frame.heat, depth=frame.depth, rows=frame.trajectory_row)
        use(got["frames"], got["optimized"])            # 8 frames whenever a window completed, else none
    tail = live.flush()                                 # the two frames still held, and how many frames were left over

Frames are numbered n = 0, 1, 2, ... in arrival order and the session's frame is the first frame's camera.  Window w covers the
frames [8w, 8w + 10) (`sequence.SEQ_LEN`, `sequence.OVERLAP`: the reference's `main()` values) and makes the frames [8w, 8w + 8)
final: its first two are averaged with the last two of window w - 1 by `sequence.merge_batches`' expression, its last two are held
for window w + 1.  Two sequences come out: `optimized`, and `estimated` = cams[n] . est_local[n] in float64.  The mid (local-stage)
sequence is not produced in live mode.  The offline Gaussian `final_smooth` needs four frames of look-ahead and has no place
here; `one_euro=(min_cutoff, beta, d_cutoff)` runs the causal One-Euro filter of the reference's `utils/one_euro_filter.py` over
`optimized` instead (off by default, as the reference's `main()` never calls it: with the filter off a session reproduces the
engine's own window results bit for bit).

`LiveOptimizer(..., stride=k, now=True)` is the dense session (section 6h, "Dense live mode"): a window every k <= 8 frames, a second
stream `now` that hands every frame back with no look-ahead (at k = 1 in the push that brought it), and `optimized` the mean of all
windows that cover a frame.  stride=8, now=False is the session described above, untouched.

`replay` / `python -m globalegomocap_amd.live` push the frames of a prepared recording one at a time: a replay of a recording, for
looking at live mode's results and step times.
"""
import os
import pickle
import time

import numpy as np
import torch

from . import _capi
from .camera import FisheyeCamera
from .engine import WindowEngine, stats_to_numpy, raise_if_degenerate, LOCAL_STAGE, GLOBAL_STAGE
from .optimizer import SequenceOptimizer, GLOBAL_VAE_PATH, LOCAL_VAE_PATH, _as_state_dict
from .sequence import SEQ_LEN, OVERLAP
from .skeleton import N_JOINTS
from .vae import infer_shape

STRIDE = SEQ_LEN - OVERLAP
# the defaults of whole_sequence._settings, as SequenceOptimizer.stage_weights takes them
DEFAULT_WEIGHTS = dict(vae_weight=0.0, smoothness_weight=0.001, bone_length_weight=0.01, weight_3d=0.01, reproj_weight=0.01)


def check_stride(stride):
    """The stride of a session, an int in 1 .. 8; ValueError otherwise."""
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or not 1 <= stride <= STRIDE:
        raise ValueError("stride is a whole number of frames between 1 and %d, got %r" % (STRIDE, stride))
    return int(stride)


def dropped_frames(n_pushed, stride=STRIDE):
    """How many of `n_pushed` frames belong to no complete window (the reference's range(0, len - 10 + 1, 8) drops them; `stride`: the
    8 of that range): (n - 10) mod stride from ten frames on, all of them below."""
    n_windows = (n_pushed - SEQ_LEN) // stride + 1 if n_pushed >= SEQ_LEN else 0
    return n_pushed - ((n_windows - 1) * stride + SEQ_LEN if n_windows else 0)


def _pieces(n_pushed, k, stride=STRIDE):
    """A push of k frames behind n_pushed, cut into pieces of at most 8 frames none of which goes past the frame that completes a
    window: the window is optimised -- and its mean bone length taken -- before the frames behind it arrive.  With windows every
    `stride` frames the completing frames are stride * w + 9."""
    out, at = [], 0
    while at < k:
        n = n_pushed + at
        completing = SEQ_LEN - 1 if n < SEQ_LEN else n + (SEQ_LEN - 1 - n) % stride          # the next frame stride * w + 9 at or behind n
        step = min(k - at, _capi.LIVE_PUSH_MAX, completing - n + 1)
        out.append((at, at + step))
        at += step
    return out


def check_push(n_pushed_times, heat, depth, est_local, rows, cams, times, heat_size=(64, 64), keypoints=None):
    """The host-side checks of `LiveOptimizer.push`, before anything is enqueued: exactly one of heat / keypoints, of depth / est_local
    and of rows / cams + times, shapes that agree on k >= 1 frames, timestamps that increase strictly (also past `n_pushed_times`, the
    last timestamp of the pushes before; None on the first).  -> (k, timestamps as a float64 array, the five other arguments as arrays or tensors).  ValueError otherwise.
    depth may be the string "bones" together with heat= (the depths are solved from the bone lengths at the maps' peaks, DESIGN.md
    section 6r): it is handed back as it is; with est_local= or keypoints= it is refused."""
    from_bones = isinstance(depth, str)
    if from_bones:
        if depth != "bones":
            raise ValueError('push: depth is an array [k,%d] or "bones", got %r' % (N_JOINTS, depth))
        if est_local is not None:
            raise ValueError("push: give exactly one of depth= (lifted here) and est_local= (already lifted)")
        if keypoints is not None or heat is None:
            raise ValueError('push: depth="bones" goes with heat= (the depths of keypoints= come from `bone_depths`)')
        depth = None
    if heat is None and keypoints is None:
        raise ValueError("push: heat= is needed")
    if heat is not None and keypoints is not None:
        raise ValueError("push: give exactly one of heat= (the pose network's maps) and keypoints= (2-D detections, splatted here)")
    heat, depth, est_local, rows, cams, times = (x if x is None or torch.is_tensor(x) else np.asarray(x) for x in (heat, depth, est_local, rows, cams, times))
    if not from_bones and (depth is None) == (est_local is None):
        raise ValueError("push: give exactly one of depth= (lifted here) and est_local= (already lifted)")
    if (rows is None) == (cams is None):
        raise ValueError("push: give exactly one of rows= (trajectory rows) and cams= with times=")
    if (cams is None) != (times is None):
        raise ValueError("push: cams= and times= come together (rows= carry their own timestamps)")
    if keypoints is not None:
        shape = tuple(keypoints.shape) if torch.is_tensor(keypoints) else np.shape(keypoints)
        k = int(shape[0]) if len(shape) == 3 else -1
        if k < 1 or shape[1] != N_JOINTS or shape[2] not in (2, 3):
            raise ValueError("push: keypoints must be [k,%d,2] or [k,%d,3] (u, v[, confidence]) with k >= 1, got %s" % (N_JOINTS, N_JOINTS, shape))
    else:
        k = int(heat.shape[0]) if len(heat.shape) == 4 else -1
        want = (k,) + tuple(heat_size) + (N_JOINTS,)
        if k < 1 or tuple(heat.shape) != want:
            raise ValueError("push: heat must be [k,%d,%d,%d] with k >= 1, got %s" % (tuple(heat_size) + (N_JOINTS, tuple(heat.shape))))
    for name, x, shape in (("depth", depth, (k, N_JOINTS)), ("est_local", est_local, (k, N_JOINTS, 3)), ("rows", rows, (k, 8)),
                           ("cams", cams, (k, 4, 4)), ("times", times, (k,))):
        if x is not None and tuple(x.shape) != shape:
            raise ValueError("push: %s must be %s for these %d frames, got %s" % (name, list(shape), k, tuple(x.shape)))
    t = rows[:, 0] if rows is not None else times
    t = np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64)
    chain = t if n_pushed_times is None else np.concatenate([[n_pushed_times], t])
    if not np.isfinite(t).all() or not (np.diff(chain) > 0).all():
        raise ValueError("push: timestamps must be finite and increase strictly")
    return k, t, (heat, "bones" if from_bones else depth, est_local, rows, cams)


class LiveOptimizer:
    """One live session on the current device.

    weights: the arguments of `SequenceOptimizer.stage_weights` (default: DEFAULT_WEIGHTS, the defaults of `whole_sequence`).
    bone: "running" -- every window is given the mean, over all frames pushed up to and including its last one, of the float32 lifted
      skeleton's bone lengths (the reference takes the chunk's mean, optimizer.py:42-43; a stream has no chunk) -- or an array [15]: a
      calibrated value.
    one_euro: None, or (min_cutoff, beta, d_cutoff): the causal filter over the 45 coordinates of `optimized`, after the merge, with
      the frames' own timestamps; its state is carried across windows and across `flush()`.
    eps: None -- torch.randn(2, D) per window (local stage, then global) from a generator seeded by `seed` -- or callable(w) -> [2,D].
    graphs: replay one captured `optimize_windows` call for every window (the window's inputs lie in buffers of fixed address).
    scale: the SLAM scale applied to the translations of `rows=`.
    sigma: the width, in heat-map pixels, of the Gaussians that `push(keypoints=)` splats.
    bones_for_depth, neck_depth: the wearer's 15 bone lengths in metres (entry 0 equal to 0; default: the mean skeleton's) and the neck's
      distance from the camera, for `bone_depths` (`bone_depth.options`).
    min_peak: with `push(heat=, depth="bones")`, a joint whose map peaks below it is treated as not detected.
    stride, now: a window every `stride` frames (1..8) and a second stream `now` with no look-ahead.  stride=8, now=False is the session
      described above.  Anything else is the dense session ("Dense live mode"): window w covers the frames
      [stride w, stride w + 10) and runs when frame stride w + 9 arrives; `push` also returns "now" -- all 10 frames of window 0, then the
      newest `stride` frames of every window as that window left them, every frame once, at stride 1 in the push that brought it;
      `optimized` is the settled stream: the frames [stride w, stride w + stride), which no later window covers, each the mean of all
      windows that covered it (oldest first, in float64); `flush` emits the 10 - stride frames still held.  `one_euro` then filters
      `now`, the stream without look-ahead, and `optimized` is never filtered.
    """

    def __init__(self, camera_model_path, global_vae=GLOBAL_VAE_PATH, local_vae=LOCAL_VAE_PATH, *, scale=1.0, weights=None, bone="running",
                 one_euro=None, eps=None, seed=0, graphs=True, lr=2, max_iter=25, heat_size=(64, 64), sigma=1.5, bones_for_depth=None,
                 neck_depth=None, min_peak=0.0, stride=STRIDE, now=False):
        from . import bone_depth
        self.stride, self.now = check_stride(stride), bool(now)          # (refused before a device is touched)
        self.dense = self.stride != STRIDE or self.now
        self._depth_opts = bone_depth.options(bones_for_depth, neck_depth=neck_depth)          # (refused before a device is touched)
        self.min_peak = float(min_peak)
        if not (np.isfinite(self.min_peak) and self.min_peak >= 0):
            raise ValueError("min_peak must be a finite number >= 0, got %r" % (min_peak,))
        sd_g, sd_l = _as_state_dict(global_vae), _as_state_dict(local_vae)
        shape = infer_shape(sd_l, seq_len=SEQ_LEN)
        if infer_shape(sd_g, seq_len=SEQ_LEN) != shape:
            raise RuntimeError("local and global VAE checkpoints have different architectures")
        if one_euro is not None:
            one_euro = tuple(float(v) for v in one_euro)
            if len(one_euro) == 2:
                one_euro += (1.0,)
            if len(one_euro) != 3 or not all(np.isfinite(v) and v >= 0 for v in one_euro) or one_euro[0] <= 0 or one_euro[2] <= 0:
                raise ValueError("one_euro is (min_cutoff > 0, beta >= 0, d_cutoff > 0), got %r" % (one_euro,))
        self.one_euro, self.scale, self.sigma = one_euro, float(scale), float(sigma)
        if not (np.isfinite(self.sigma) and self.sigma > 0):
            raise ValueError("sigma must be a positive number, got %r" % (sigma,))
        self.engine = e = WindowEngine(shape, FisheyeCamera.from_json(camera_model_path), max_windows=1, heat_size=heat_size)
        e.load_vae(LOCAL_STAGE, sd_l)
        e.load_vae(GLOBAL_STAGE, sd_g)
        if graphs:
            e.enable_graphs(True)
        self.opts = _capi.default_lbfgs_opts(lr, max_iter)
        self.w_local, self.w_global = SequenceOptimizer.stage_weights(None, **dict(DEFAULT_WEIGHTS, **(weights or {})))          # (the method reads no attribute)
        dev, H, W = e.device, e.heat_size[0], e.heat_size[1]
        self._bone_fixed = None
        if not (isinstance(bone, str) and bone == "running"):
            b = np.asarray(bone, dtype=np.float32)
            if b.shape != (N_JOINTS,):
                raise ValueError('bone is "running" or an array of %d bone lengths' % N_JOINTS)
            self._bone_fixed = torch.from_numpy(b.copy()).to(dev)
        self._eps, self._gen = eps, torch.Generator().manual_seed(int(seed))
        # the session's device memory: rings + state, the window buffers of fixed address, the call's small inputs, the output block
        self._bufs = e.live_buffers()
        self._win_pose = torch.zeros(SEQ_LEN, N_JOINTS, 3, device=dev, dtype=torch.float32)
        self._win_cams = torch.zeros(SEQ_LEN, 4, 4, device=dev, dtype=torch.float64)
        self._win_heat = torch.zeros(SEQ_LEN, H, W, N_JOINTS, device=dev, dtype=torch.float32)
        self._frame0 = torch.zeros(1, device=dev, dtype=torch.int32)
        self._mean_bone = torch.zeros(1, N_JOINTS, device=dev, dtype=torch.float32)
        self._eps_l, self._eps_g = (torch.zeros(1, e.D, device=dev, dtype=torch.float32) for _ in range(2))
        self._out = torch.zeros(2, STRIDE, N_JOINTS, 3, device=dev, dtype=torch.float64)
        self._kp_prev = torch.zeros(N_JOINTS, 3, device=dev, dtype=torch.float64)          # push(keypoints=, depth=): the last usable lift of every joint
        # the dense session's own: the sums / counts / filter block and its output block (settled, estimated, now)
        self._dense_state = e.live_dense_state() if self.dense else None
        self._out_dense = torch.zeros(3, SEQ_LEN, N_JOINTS, 3, device=dev, dtype=torch.float64) if self.dense else None
        self.n_pushed = self.n_windows = self.n_emitted = self.n_now = 0
        self._last_time, self._row0, self._flushed = None, None, False
        self.window_log, self._optimized, self._estimated, self._now = [], [], [], []

    # ------------------------------------------------------------------ state
    def close(self):
        """Releases the engine and the session's device memory; `push` and `flush` raise GemError afterwards."""
        if self.engine is not None:
            torch.cuda.synchronize(self.engine.device)
            self.engine.close()
        self.engine = self._bufs = self._win_pose = self._win_cams = self._win_heat = self._out = None
        self._mean_bone = self._eps_l = self._eps_g = self._frame0 = self._bone_fixed = self._kp_prev = None
        self._dense_state = self._out_dense = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def graph_stats(self):
        return self._engine().graph_stats()

    def _engine(self):
        if self.engine is None:
            raise _capi.GemError("this live session has been closed")
        return self.engine

    def result(self):
        """Everything emitted so far: {"frames": 0, "optimized", "estimated"} with numpy f64 arrays [n_emitted,15,3]; a dense session
        adds "now_frames": 0 and "now" [n_now,15,3]."""
        cat = lambda parts: np.concatenate(parts) if parts else np.empty((0, N_JOINTS, 3))          # noqa: E731
        r = {"frames": 0, "optimized": cat(self._optimized), "estimated": cat(self._estimated)}
        return dict(r, now_frames=0, now=cat(self._now)) if self.dense else r

    def save_pose(self, out_dir):
        """`<out_dir>/result_pose.pkl` with `estimated_pose` and `optimized_pose` (lists of [15,3] frames): the schema of the
        no-ground-truth `--save_pose`, minus the mid sequence that live mode does not produce; `render` and `meshes` read it."""
        os.makedirs(out_dir, exist_ok=True)
        r = self.result()
        path = os.path.join(out_dir, "result_pose.pkl")
        with open(path, "wb") as f:
            pickle.dump({"estimated_pose": list(r["estimated"]), "optimized_pose": list(r["optimized"])}, f)
        return path

    # ------------------------------------------------------------------ frames in
    def _device(self, x, dtype):
        t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        return t.to(device=self.engine.device, dtype=dtype).contiguous()

    def _cameras(self, rows):
        """Trajectory rows -> cameras in the session's frame: `slam.scaled_trajectory` of (the session's first row, these rows)."""
        from . import slam
        rows = np.ascontiguousarray(rows.detach().cpu().numpy() if torch.is_tensor(rows) else rows, dtype=np.float64)
        if self._row0 is None:
            self._row0 = rows[:1].copy()
        both = np.concatenate([self._row0, rows])
        return slam.scaled_trajectory(both[:, 1:4], both[:, 4:8], self.scale)[1:]

    def bone_depths(self, keypoints):
        """The depths of detections [k,15,2|3] that have none, for the frames about to be pushed: -> (depth [k,15] f64, solved [k,15]
        u8, keypoints [k,15,3] f64 with the confidence of every unsolved joint set to 0), device tensors (`WindowEngine.bone_depths`
        with the session's `bones_for_depth` and `neck_depth`).  Pushed as `push(keypoints=<the third>, depth=<the first>, ...)`, an
        unsolved joint is a lost detection: its map is blank and it holds its last usable lift.  Every frame is solved on its own: the
        depths do not depend on how the stream is cut into pushes.  No synchronisation."""
        e = self._engine()
        kp_d = e._keypoints("bone_depths", keypoints)
        depth, solved, _ = e.bone_depths(kp_d, opts=self._depth_opts)
        masked = kp_d.clone()
        masked[..., 2] = torch.where(solved.bool(), kp_d[..., 2], torch.zeros_like(kp_d[..., 2]))
        return depth, solved, masked

    def push(self, *, heat=None, depth=None, est_local=None, rows=None, cams=None, times=None, keypoints=None):
        """k >= 1 new frames: heat [k,H,W,15], or in its place keypoints [k,15,2|3] -- 2-D detections (u, v[, confidence]) in pixels of the
        fisheye image, splatted into the maps on the device (`WindowEngine.keypoint_heatmaps`; with depth= they are lifted at the
        detection itself, `lift_keypoints`, a joint without a usable detection holding its last usable lift: the session's first frame
        must have every joint); either depth [k,15] (lifted with `WindowEngine.lift_skeleton`) or est_local [k,15,3]
        (already lifted), or with heat= the string depth="bones" for a pose network without a depth head: the maps' sub-pixel peaks
        (`heatmap_peaks`, the session's `min_peak`) are given depths by `bone_depths` with the session's skeleton and lifted at the
        peak, a joint the solve did not reach holding its last lift (the session's first frame must have every joint solved: one
        15-byte read-back on the first push); the maps pushed are the caller's own;
        either rows [k,8] trajectory rows `time tx ty tz qx qy qz qw` (made cameras by `slam`'s functions, relative
        to the session's first frame, translations times `scale`) or cams [k,4,4] with times [k].  Host or device arrays.  Every window
        these frames complete is optimised at once; the call blocks until they are done, reads their statistics and raises the
        reference's Exception("norm is zero!") for a degenerate one.  -> {"frames": index of the first returned frame, "optimized",
        "estimated"}: numpy f64 [m,15,3], m = 8 x the windows completed (possibly 0); a dense session (`stride`, `now`): m = stride x the
        windows completed, plus "now_frames", the index of the first `now` frame returned, and "now" [m',15,3] f64.  ValueError (before
        anything is enqueued) for timestamps that do not increase strictly, wrong shapes, or contradictory arguments."""
        e = self._engine()
        if self._flushed:
            raise _capi.GemError("this live session has been flushed: its held frames are out, a new stream needs a new session")
        k, t, (heat, depth, est_local, rows, cams) = check_push(self._last_time, heat, depth, est_local, rows, cams, times, e.heat_size, keypoints)
        if keypoints is not None:
            if depth is not None and self.n_pushed == 0:
                from .detections import usable
                kp0 = np.asarray(keypoints[0].detach().cpu().numpy() if torch.is_tensor(keypoints) else np.asarray(keypoints)[0], dtype=np.float64)
                lost = np.nonzero(~(usable(kp0) if kp0.shape[1] == 3 else np.isfinite(kp0).all(axis=1)))[0]
                if len(lost):
                    raise ValueError("push: joints %s of the session's first frame have no usable detection: nothing to hold" % lost.tolist())
            kp_d = e._keypoints("push", keypoints)
            heat_d = e.keypoint_heatmaps(kp_d, self.sigma)
            pose_d = self._device(est_local, torch.float32) if est_local is not None else e.lift_keypoints(kp_d, depth, prev=self._kp_prev, want_f64=False)[1]
        elif isinstance(depth, str):
            heat_d = self._device(heat, torch.float32)
            kp_d, _ = e.heatmap_peaks(heat_d, min_peak=self.min_peak)
            depth_d, solved, _ = e.bone_depths(kp_d, opts=self._depth_opts)
            if self.n_pushed == 0:
                lost = np.nonzero(solved[0].cpu().numpy() == 0)[0]
                if len(lost):
                    raise ValueError("push: joints %s of the session's first frame have no usable detection: nothing to hold" % lost.tolist())
            kp_d[..., 2] = torch.where(solved.bool(), kp_d[..., 2], torch.zeros_like(kp_d[..., 2]))
            pose_d = e.lift_keypoints(kp_d, depth_d, prev=self._kp_prev, want_f64=False)[1]
        else:
            heat_d = self._device(heat, torch.float32)
            pose_d = self._device(est_local, torch.float32) if est_local is not None else e.lift_skeleton(heat_d, depth, want_f64=False)[1]
        cams_d = self._device(self._cameras(rows) if rows is not None else cams, torch.float64)
        times_d = self._device(t, torch.float64)
        self._last_time = float(t[-1])
        first, first_now, done = self.n_emitted, self.n_now, []
        for a, b in _pieces(self.n_pushed, k, self.stride):
            t0 = time.perf_counter()
            e.live_push(self._bufs, self.n_pushed, self.n_windows * self.stride, heat_d[a:b], pose_d[a:b], cams_d[a:b], times_d[a:b])
            self.n_pushed += b - a
            if self.n_pushed == self.n_windows * self.stride + SEQ_LEN:
                done.append(self._window(t0))
        return self._emitted(first, done, self.stride, first_now)

    def _window(self, t0):
        """Window self.n_windows is complete: gather, optimise (both stages, B = 1), emit; blocks on the statistics."""
        e, w = self.engine, self.n_windows
        if self.dense:
            e.live_window_at(self._bufs, w * self.stride, self.n_pushed, self._win_pose, self._win_cams, self._win_heat, self._mean_bone, self._bone_fixed)
        else:
            e.live_window(self._bufs, w, self.n_pushed, self._win_pose, self._win_cams, self._win_heat, self._mean_bone, self._bone_fixed)
        eps = self._eps(w) if self._eps is not None else torch.randn(2, e.D, generator=self._gen)
        eps = torch.as_tensor(np.asarray(eps) if not torch.is_tensor(eps) else eps, dtype=torch.float32).reshape(2, e.D)
        self._eps_l.copy_(eps[0:1])
        self._eps_g.copy_(eps[1:2])
        _, glob, stats = e.optimize_windows(self._win_pose, self._win_cams, self._win_heat, self._frame0, self._mean_bone, self._eps_l,
                                            self._eps_g, self.w_local, self.w_global, self.opts)
        if self.dense:
            e.live_emit_dense(self._bufs, self._dense_state, self.stride, w, self._out_dense, glob, self._win_pose, self._win_cams, one_euro=self.one_euro)
            out = self._out_dense.cpu().numpy()
        else:
            e.live_emit(self._bufs, w, self._out, glob, self._win_pose, self._win_cams, one_euro=self.one_euro)
            out = self._out.cpu().numpy()                               # (behind the emit kernel: the window is done)
        st = stats_to_numpy(stats)
        self.window_log.append({"window": w, "stride": self.stride, "local": st[0].copy(), "global": st[1].copy(),
                                "mean_bone": self._mean_bone[0].cpu().numpy(), "step_ms": (time.perf_counter() - t0) * 1e3})
        self.n_windows += 1
        raise_if_degenerate(st)
        return out

    def _emitted(self, first, done, n, first_now=0, final=False):
        """The output blocks of the windows `done` (n settled frames each) as push's dict; a dense session's blocks carry the `now`
        frames too: all 10 of window 0, the newest `stride` of every other window, none at the flush."""
        opt = np.concatenate([o[0, :n] for o in done]) if done else np.empty((0, N_JOINTS, 3))
        est = np.concatenate([o[1, :n] for o in done]) if done else np.empty((0, N_JOINTS, 3))
        if done:
            self._optimized.append(opt)
            self._estimated.append(est)
            self.n_emitted += len(opt)
        got = {"frames": first, "optimized": opt, "estimated": est}
        if self.dense:
            w0 = self.n_windows - len(done)          # the first of these windows
            parts = [] if final else [o[2, :SEQ_LEN if w0 + i == 0 else self.stride] for i, o in enumerate(done)]
            now = np.concatenate(parts) if parts else np.empty((0, N_JOINTS, 3))
            if len(now):
                self._now.append(now)
                self.n_now += len(now)
            got.update(now_frames=first_now, now=now)
        return got

    def flush(self):
        """The end of the stream: emits the two frames still held, as they are (`merge_batches`' last window; filtered when the filter
        is on), and reports as "dropped" how many pushed frames belonged to no complete window.  -> push's dict plus "dropped".  A
        dense session emits the 10 - stride frames still held, each the mean of the windows that covered it, and no `now` frame."""
        e = self._engine()
        first, done = self.n_emitted, []
        if self.n_windows and not self._flushed:
            if self.dense:
                e.live_emit_dense(self._bufs, self._dense_state, self.stride, self.n_windows, self._out_dense, final=True, one_euro=self.one_euro)
                done.append(self._out_dense.cpu().numpy())
            else:
                e.live_emit(self._bufs, self.n_windows, self._out, final=True, one_euro=self.one_euro)
                done.append(self._out.cpu().numpy())
        self._flushed = True
        return dict(self._emitted(first, done, SEQ_LEN - self.stride, self.n_now, final=True), dropped=dropped_frames(self.n_pushed, self.stride))


# ---------------------------------------------------------------------------------------------------------------------- replay
def step_summary(window_log):
    """Median / 99th percentile / maximum of the per-window step times (ms) and the L-BFGS counts of a session's `window_log`."""
    if not window_log:
        return {"windows": 0}
    ms = np.array([r["step_ms"] for r in window_log])
    out = {"windows": len(ms), "step_ms_median": float(np.median(ms)), "step_ms_p99": float(np.percentile(ms, 99)), "step_ms_max": float(ms.max())}
    for stage in ("local", "global"):
        out[stage + "_iters_mean"] = float(np.mean([r[stage]["n_iter"] for r in window_log]))
        out[stage + "_evals_mean"] = float(np.mean([r[stage]["func_evals"] for r in window_log]))
    return out


def replay(slam_result_path, heatmap_dir, depth_dir, start_frame, end_frame, camera_model_path, fps=25, pace="max", save_pose=None,
           verbose=True, keypoints=None, first_id=0, depth_from=None, **session):
    """A prepared recording pushed through a `LiveOptimizer` one frame at a time: the frames [start_frame, end_frame) of the listings
    come to the device with `prepare`'s reader, the trajectory's rows of those frame ids are the cameras.  pace "realtime" sleeps to
    the timestamps, "max" does not.  `session`: the keyword arguments of `LiveOptimizer`.  -> (result dict with "dropped", the
    session's window_log).  A replay of a recording: a rig calls `push` itself.  `keypoints` (with `heatmap_dir` None): a detections
    file (`detections.read_detections`; `first_id`: the frame id of its first row) pushed with `keypoints=` instead of heat-maps, the
    depths from the file or from `depth_dir`, or with depth_from="bones" solved per push from the bone lengths
    (`LiveOptimizer.bone_depths`; the session's `bones_for_depth=` and `neck_depth=`).  depth_from="bones" with `heatmap_dir` and no
    depth directory: no depth file is read, every frame is pushed as `push(heat=, depth="bones")` (the session's `min_peak=`)."""
    from . import prepare, slam
    if pace not in ("max", "realtime"):
        raise ValueError('pace is "max" or "realtime"')
    with open(slam_result_path) as f:
        rows = slam.trajectory_rows(f.read())
    prepare.check_trajectory(rows, start_frame, end_frame, fps)
    ids = slam.frame_ids(rows, fps)
    rows = rows[(ids >= start_frame) & (ids < end_frame)]
    if (keypoints is None) == (heatmap_dir is None):
        raise ValueError("replay: give exactly one of the heat-map directory and keypoints=")
    if depth_from not in (None, "bones"):
        raise ValueError('replay: depth_from is None or "bones"')
    if depth_from is not None and depth_dir is not None:
        raise ValueError('replay: depth_from="bones" goes without a depth directory')
    if keypoints is not None:
        from . import detections
        det = detections.read_detections(keypoints, first_id)
        pick = detections.span_rows(det["frame_ids"], [(start_frame, end_frame)])[0]
        if det["depth"] is None and depth_dir is None and depth_from is None:
            raise ValueError("replay: the joints' depths are needed: `depth` in the detections file, or the depth directory")
        kp = det["keypoints"][pick]
        if depth_from is not None:
            depth = None
        else:
            depth = det["depth"][pick] if det["depth"] is not None else detections.depths_from_mat_dir(depth_dir, det["frame_ids"][pick])
        heat, live = None, LiveOptimizer(camera_model_path, **session)
    else:
        if depth_dir is None and depth_from is None:
            raise ValueError('replay: the joints\' depths are needed: the depth directory, or depth_from="bones"')
        heat_paths = prepare.list_frames(heatmap_dir, start_frame, end_frame)
        depth_paths = prepare.list_frames(depth_dir, start_frame, end_frame) if depth_from is None else None
        if len(heat_paths) != end_frame - start_frame or (depth_paths is not None and len(depth_paths) != end_frame - start_frame):
            raise ValueError("frames [%d, %d) of the listings are asked for, but there are %d heat-map and %d depth files"
                             % (start_frame, end_frame, len(heat_paths), -1 if depth_paths is None else len(depth_paths)))
        heat, depth, _ = prepare.frames_to_device(heat_paths, depth_paths)
        live = LiveOptimizer(camera_model_path, heat_size=tuple(heat.shape[1:3]), **session)
    try:
        wall0 = time.perf_counter()
        for i in range(len(rows)):
            if pace == "realtime":
                wait = (rows[i, 0] - rows[0, 0]) - (time.perf_counter() - wall0)
                if wait > 0:
                    time.sleep(wait)
            if heat is None and depth is None:
                d, _, masked = live.bone_depths(kp[i:i + 1])
                live.push(keypoints=masked, depth=d, rows=rows[i:i + 1])
            elif heat is None:
                live.push(keypoints=kp[i:i + 1], depth=depth[i:i + 1], rows=rows[i:i + 1])
            elif depth is None:
                live.push(heat=heat[i:i + 1], depth="bones", rows=rows[i:i + 1])
            else:
                live.push(heat=heat[i:i + 1], depth=depth[i:i + 1], rows=rows[i:i + 1])
        tail = live.flush()
        res = dict(live.result(), dropped=tail["dropped"])
        if save_pose is not None:
            live.save_pose(save_pose)
        if verbose:
            s = step_summary(live.window_log)
            print("live: {} frames pushed, {} emitted, {} dropped, {} windows".format(live.n_pushed, live.n_emitted, tail["dropped"], s["windows"]))
            if s["windows"]:
                print("step time per window (ms): median {:.3f}, 99th percentile {:.3f}, max {:.3f}; budget {:.1f} ms at {:g} fps".format(
                    s["step_ms_median"], s["step_ms_p99"], s["step_ms_max"], 1e3 * live.stride / fps, fps))
                print("L-BFGS per window: local {:.1f} iterations / {:.1f} evaluations, global {:.1f} / {:.1f}".format(
                    s["local_iters_mean"], s["local_evals_mean"], s["global_iters_mean"], s["global_evals_mean"]))
        return res, live.window_log
    finally:
        live.close()


def _one_euro_arg(text):
    v = tuple(float(x) for x in text.split(","))
    if len(v) not in (2, 3):
        raise ValueError("--one_euro takes MIN,BETA[,DCUT]")
    return v if len(v) == 3 else v + (1.0,)


def _bone_arg(text):
    return text if text == "running" else np.load(text)


def _parser():
    import argparse
    from .camera import DEFAULT_CALIBRATION
    p = argparse.ArgumentParser(description="Replay a prepared recording through live mode, one frame at a time. This replays a "
                                            "recording; a head-mounted rig calls LiveOptimizer.push itself.")
    p.add_argument("--slam", required=True, metavar="TRAJ", help="the trajectory: lines `time tx ty tz qx qy qz qw`")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--heatmaps", default=None, metavar="DIR")
    src.add_argument("--keypoints", default=None, metavar="FILE", help="2-D detections in place of heat-maps: .npy [N,15,2|3] or .npz with "
                                                                       "keypoints[, depth, frame_ids]; u, v in pixels of the fisheye image")
    p.add_argument("--depths", default=None, metavar="DIR", help="needed with --heatmaps, and with --keypoints unless the file carries `depth`")
    p.add_argument("--depth_from", default=None, choices=("bones",), help="bones: no depths at all -- they are solved from the bone "
                                                                         "lengths, at the detections of --keypoints or at the sub-pixel "
                                                                         "peaks of --heatmaps (DESIGN.md sections 6q, 6r)")
    from .bone_depth import add_bone_depth_options
    add_bone_depth_options(p)
    p.add_argument("--min_peak", type=float, default=None, metavar="P", help="with --heatmaps --depth_from bones: a joint whose map peaks "
                                                                             "below P is treated as not detected (default 0)")
    p.add_argument("--first_id", type=int, default=0, help="frame id of the first row of --keypoints (without frame_ids)")
    p.add_argument("--sigma", type=float, default=1.5, help="the width of the Gaussians splatted from --keypoints, in heat-map pixels")
    p.add_argument("--scale", type=float, default=1.0, help="the SLAM scale applied to the trajectory's translations")
    p.add_argument("--start", type=int, required=True, metavar="A")
    p.add_argument("--end", type=int, required=True, metavar="B")
    p.add_argument("--fps", type=float, default=25)
    p.add_argument("--pace", choices=("max", "realtime"), default="max", help="realtime: sleep to the frames' timestamps")
    p.add_argument("--one_euro", type=_one_euro_arg, default=None, metavar="MIN,BETA[,DCUT]", help="the causal One-Euro filter over the optimised poses (default: off)")
    p.add_argument("--bone", type=_bone_arg, default="running", metavar="running|FILE.npy", help="mean bone lengths: the running mean, or 15 calibrated values")
    p.add_argument("--save_pose", default=None, metavar="DIR", help="write DIR/result_pose.pkl (estimated_pose, optimized_pose)")
    p.add_argument("--camera", type=str, default=DEFAULT_CALIBRATION)
    p.add_argument("--global_vae", type=str, default=GLOBAL_VAE_PATH)
    p.add_argument("--local_vae", type=str, default=LOCAL_VAE_PATH)
    p.add_argument("--vae", type=float, default=DEFAULT_WEIGHTS["vae_weight"])
    p.add_argument("--smooth", type=float, default=DEFAULT_WEIGHTS["smoothness_weight"])
    p.add_argument("--bone_length", type=float, default=DEFAULT_WEIGHTS["bone_length_weight"])
    p.add_argument("--weight_3d", type=float, default=DEFAULT_WEIGHTS["weight_3d"])
    p.add_argument("--reproj_weight", type=float, default=DEFAULT_WEIGHTS["reproj_weight"])
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--stride", type=int, default=STRIDE, metavar="K", help="a window every K frames, 1..8 (default 8); below 8 every frame "
                                                                           "is the mean of all windows that cover it")
    p.add_argument("--now", action="store_true", help="also keep the stream without look-ahead: every window's newest K frames, as it left them")
    return p


def _cli(argv=None):
    p = _parser()
    a = p.parse_args(argv)
    if a.heatmaps is not None and a.depths is None and a.depth_from is None:
        p.error("--heatmaps needs --depths or --depth_from bones")
    if a.depth_from is not None and a.depths is not None:
        p.error("--depth_from bones excludes --depths")
    if a.depth_from is None and (a.bones is not None or a.neck_depth is not None or a.min_peak is not None):
        p.error("--bones, --neck_depth and --min_peak belong to --depth_from bones")
    if a.min_peak is not None and a.heatmaps is None:
        p.error("--min_peak goes with --heatmaps: detections carry their own confidence")
    if a.min_peak is not None and not (np.isfinite(a.min_peak) and a.min_peak >= 0):
        p.error("--min_peak must be a finite number >= 0")
    if not 1 <= a.stride <= STRIDE:
        p.error("--stride is between 1 and %d" % STRIDE)
    from .bone_depth import bones_from_args
    weights = dict(vae_weight=a.vae, smoothness_weight=a.smooth, bone_length_weight=a.bone_length, weight_3d=a.weight_3d,
                   reproj_weight=a.reproj_weight)
    replay(a.slam, a.heatmaps, a.depths, a.start, a.end, a.camera, fps=a.fps, pace=a.pace, save_pose=a.save_pose, global_vae=a.global_vae,
           local_vae=a.local_vae, scale=a.scale, weights=weights, bone=a.bone, one_euro=a.one_euro, seed=a.seed, keypoints=a.keypoints,
           first_id=a.first_id, sigma=a.sigma, depth_from=a.depth_from, bones_for_depth=bones_from_args(a), neck_depth=a.neck_depth,
           min_peak=0.0 if a.min_peak is None else a.min_peak, stride=a.stride, now=a.now)


if __name__ == "__main__":
    _cli()
