"""The report half of a run: what one chunk's report is (`ChunkReport`), how a batch's reports are computed on the device
(`batch_reports`, or chunk by chunk: `chunk_reports`), how a sequence's return value and printed summary follow from them
(`sequence_result`), and the files a chunk's result may be written to (`Outputs`, `result_pose_dict`).  Shared by the
batch pipeline (`whole_sequence`) and the one-chunk `optimizer.main`; it imports neither."""
import os
from collections import OrderedDict
from dataclasses import FrozenInstanceError, dataclass

import numpy as np
import torch

from . import bvh as animation, gltf as scenes, meshes, render as rendering, video as clips          # (`bvh`, `render` and `video` are also fields' names here)
from .errors import calculate_errors
from .sequence import cut_windows, merge_batches, merge_chunks, final_smooth, relative_global_numpy, to_global_numpy

SUMMARY_LINES = (          # (label printed by the reference, key) in print order, None = separator
    ("Average original global pose mpjpe", "original_global_mpjpe"), ("Average mid global pose mpjpe", "mid_global_mpjpe"),
    ("Average optimized global pose mpjpe", "optimized_global_mpjpe"), None,
    ("Average original cam pose error", "original_camera_pos_error"), ("Average optimized cam pose error", "optimized_camera_pos_error"), None,
    ("Average original aligned cam pose error", "original_aligned_camera_pos_error"),
    ("Average optimized aligned cam pose error", "optimized_aligned_camera_pos_error"), None,
    ("Average original_aligned_global_mpjpe", "original_aligned_global_mpjpe"), ("Average aligned_mid_seq_mpjpe", "aligned_mid_seq_mpjpe"),
    ("Average optimized_aligned_global_mpjpe", "optimized_aligned_global_mpjpe"), None,
    ("Average aligned original global pose mpjpe", "aligned_original_mpjpe"),
    ("Average aligned mid local pose mpjpe", "aligned_mid_optimized_mpjpe"),
    ("Average aligned optimized global pose mpjpe", "aligned_optimized_mpjpe"), None,
    ("Average bone length aligned original global pose mpjpe", "bone_length_aligned_original_mpjpe"),
    ("Average bone length aligned mid local pose mpjpe", "bone_length_aligned_mid_optimized_mpjpe"),
    ("Average bone length aligned optimized global pose mpjpe", "bone_length_aligned_optimized_mpjpe"), None,
)

QUALITY_LINES = (          # the report without ground truth, in the order of its keys: (label, key), None = separator
    ("Average estimated heatmap response", "estimated_heatmap_response"), ("Average optimized heatmap response", "optimized_heatmap_response"), None,
    ("Average estimated bone length rms", "estimated_bone_length_rms"), ("Average optimized bone length rms", "optimized_bone_length_rms"), None,
    ("Average estimated acceleration", "estimated_acceleration"), ("Average optimized acceleration", "optimized_acceleration"), None,
    ("Average optimized displacement", "optimized_displacement"), None,
)
QUALITY_KEYS = tuple(line[1] for line in QUALITY_LINES if line is not None)


@dataclass
class ChunkReport:
    """One chunk's report.  `result`: the 18 errors, or without ground truth the seven entries of QUALITY_KEYS; `est` / `opt` / `gt`:
    the estimated, optimised and ground-truth merged sequences on the host (`gt` None: the chunk has no ground truth); `mid`: stage
    one's sequence (None where nobody asked for it); `raw`: the chunk's row of the device report (None: the report was computed
    chunk by chunk against a ground truth); `views`: (est, opt, gt) where the batched report left them on the device, else None."""
    __slots__ = ("result", "est", "opt", "gt", "mid", "raw", "views")
    result: dict
    est: np.ndarray
    opt: np.ndarray
    gt: object
    mid: object
    raw: object
    views: object

    def sequences(self):
        """(estimated, optimised, ground truth or None) for the output writers: on the device where the report left them there, so
        that no sequence goes up again, else the host arrays."""
        return self.views if self.views is not None else (self.est, self.opt, self.gt)

    def drop_views(self):
        """The device views alias the batch's scratch uploads and frame buffers, which the pipeline hands to the batch three further
        on: a report that outlives its batch must not keep them."""
        self.views = None


# ------------------------------------------------------------------------------------------------------------------ the device reports
def report_inputs(chunks, starts, est_cat, cams_cat, seq_len, overlap, upload, ground_truth=True):
    """The report's half that does not depend on the optimiser's result (equal chunks -- the reference's 100-frame chunks: the
    sequences main() returns besides the optimised one, for ALL windows of the batch at once, the overlap merges vectorised over
    the chunks), computed and uploaded while the files are still arriving.  ground_truth=False: no "gt_m" / "gt_d"."""
    idx = np.concatenate(starts)[:, None] + np.arange(seq_len)[None]
    cam_w = cams_cat[idx]
    est_m = merge_chunks(to_global_numpy(relative_global_numpy(est_cat[idx], cam_w), cam_w), len(chunks), overlap)
    gt_m = merge_chunks(np.concatenate([c["gt"] for c in chunks])[idx], len(chunks), overlap) if ground_truth else None
    # (stage one's global sequence: C0 (C0^-1 C_t) X as ONE transform per frame, composed here in the reference's order --
    # utils/utils.py:99-112 then optimizer.py:302-308 -- so that the result-dependent half is a multiply-add)
    A = np.matmul(cam_w[:, :1], np.matmul(np.linalg.inv(cam_w[:, 0])[:, None], cam_w))
    rep = {"mid_A": np.ascontiguousarray(np.moveaxis(A[..., :3, :], (-2, -1), (0, 1))[..., None]), "est_m": est_m,      # mid_A [3,4,W,T,1]
           "est_d": upload(est_m.reshape(-1, 15, 3), torch.float64)}
    if ground_truth:
        rep.update(gt_m=gt_m, gt_d=upload(gt_m.reshape(-1, 15, 3), torch.float64))
    return rep


def _mid_sequences(inputs, mid_np, n_chunks, overlap):
    """Stage one's merged global sequences [n_chunks,fpc,J,3] (host float64) from its local poses and `inputs["mid_A"]`."""
    A, X = inputs["mid_A"], np.ascontiguousarray(np.moveaxis(mid_np.astype(np.float64), -1, 0))          # X [3,W,T,J]
    mid_g = np.empty(mid_np.shape, dtype=np.float64)
    for d in range(3):
        mid_g[..., d] = A[d, 0] * X[0] + A[d, 1] * X[1] + A[d, 2] * X[2] + A[d, 3]
    return merge_chunks(mid_g, n_chunks, overlap)


def _quality_rows(engine, est_d, opt_d, frames, n_chunks):
    """`sequence_quality` of the estimated sequences and of the optimised ones (those also against the estimated ones), enqueued on the
    current stream: a device tensor [n_chunks,7] in the order of QUALITY_KEYS.  `frames`: (cams, heat, frame0, mean_bone) of the
    batch, see `WindowEngine.sequence_quality`."""
    q_est = engine.sequence_quality(est_d, *frames, n_chunks)
    q_opt = engine.sequence_quality(opt_d, *frames, n_chunks, ref=est_d)
    return torch.stack([q_est[:, 0], q_opt[:, 0], q_est[:, 1], q_opt[:, 1], q_est[:, 2], q_opt[:, 2], q_opt[:, 3]], dim=1)


def _result_dict(engine, raw, ground_truth):
    """One chunk's report dict from its raw row: the 17 scalar errors and `joints_error`, or the seven entries of QUALITY_KEYS."""
    if not ground_truth:
        return OrderedDict(zip(QUALITY_KEYS, raw.tolist()))
    res = OrderedDict(zip(engine.ERROR_KEYS, raw[:17].tolist()))
    res["joints_error"] = raw[17:].copy()
    return res


def batch_reports(engine, inputs, mid_np, opt_global, n_chunks, overlap, smooth, *, upload, lap, frames=None, want_mid=True):
    """The reports of all chunks of a batch (`inputs`: what `report_inputs` prepared): ONE merge and ONE scoring call on the device,
    read back with ONE synchronisation.  With ground truth the scoring call is `calculate_errors_chunks`; with `frames` -- (cams,
    heat, first frame of every chunk, mean_bone of the batch) -- the chunks have none and it is two `sequence_quality` calls, and stage
    one's sequences are made only when `want_mid`.  -> one ChunkReport per chunk, its sequences also as views of the device's."""
    ground_truth = frames is None
    fpc = inputs["est_m"].shape[1]
    mid_m = _mid_sequences(inputs, mid_np, n_chunks, overlap) if ground_truth or want_mid else None
    if ground_truth:
        lap("report: stage-one sequences (host float64)")
    opt_d = engine.merge_windows(opt_global, n_chunks, overlap=overlap, smooth=smooth)          # [n_chunks*fpc,15,3] f64, device
    if ground_truth:
        mid_d = upload(mid_m.reshape(n_chunks * fpc, 15, 3), torch.float64)
        raw = engine.calculate_errors_chunks(inputs["est_d"], mid_d, opt_d, inputs["gt_d"], n_chunks)
        lap("report: merge + error kernels enqueued")
    else:
        raw = _quality_rows(engine, inputs["est_d"], opt_d, frames, n_chunks)
        lap("report: merge + quality kernels enqueued")
    raw = raw.cpu().numpy()
    opt_m = opt_d.cpu().numpy().reshape(n_chunks, fpc, 15, 3)
    lap("report: read-back")
    reports = []
    for k in range(n_chunks):
        on_device = slice(k * fpc, (k + 1) * fpc)
        reports.append(ChunkReport(result=_result_dict(engine, raw[k], ground_truth), est=inputs["est_m"][k], opt=opt_m[k],
                                   gt=inputs["gt_m"][k] if ground_truth else None, mid=None if mid_m is None else mid_m[k], raw=raw[k],
                                   views=(inputs["est_d"][on_device], opt_d[on_device], inputs["gt_d"][on_device] if ground_truth else None)))
    return reports


def chunk_reports(engine, chunks, mid_np, opt_global, seq_len, overlap, smooth, device_metrics, frames=None):
    """The reports chunk by chunk: the only route for chunks of different lengths and for device_metrics=False.  -> per chunk a
    ChunkReport without device views, or None for a chunk too short for a window.  `frames` as in `batch_reports`: the chunks have no
    ground truth, and each chunk's row is read back before the next is enqueued."""
    reports, w0 = [], 0
    for ci, c in enumerate(chunks):
        nw = len(c["starts"])
        sl = slice(w0, w0 + nw)
        w0 += nw
        if nw == 0:
            reports.append(None)
            continue
        loc_w, cam_w = cut_windows(c["est_local"], c["starts"], seq_len), cut_windows(c["cams"], c["starts"], seq_len)
        est_seq = merge_batches(to_global_numpy(relative_global_numpy(loc_w, cam_w), cam_w), overlap)
        mid_seq = merge_batches(to_global_numpy(relative_global_numpy(mid_np[sl], cam_w), cam_w), overlap)
        gt_seq = raw = None
        if frames is None:
            gt_seq = np.asarray(merge_batches(cut_windows(c["gt"], c["starts"], seq_len), overlap))
        else:
            est_d = engine._f64(np.asarray(est_seq))
        if device_metrics:
            opt_seq_d = engine.merge_windows(opt_global[sl], 1, overlap=overlap, smooth=smooth)
            if frames is None:
                res = engine.calculate_errors(est_seq, mid_seq, opt_seq_d, gt_seq)
            else:
                raw = _quality_rows(engine, est_d, opt_seq_d, (frames[0], frames[1], frames[2][ci:ci + 1], frames[3][ci:ci + 1]), 1).cpu().numpy()[0]
                res = _result_dict(engine, raw, False)
            opt_seq = opt_seq_d.cpu().numpy()
        else:          # (with ground truth only: `_settings` refuses the other combination)
            opt_seq = merge_batches(opt_global[sl].cpu().numpy(), overlap)
            if smooth:
                opt_seq = final_smooth(opt_seq)
            res = calculate_errors(est_seq, mid_seq, opt_seq, gt_seq)
        reports.append(ChunkReport(result=res, est=np.asarray(est_seq), opt=np.asarray(opt_seq), gt=gt_seq, mid=np.asarray(mid_seq), raw=raw,
                                   views=None))
    return reports


def sequence_result(reports, title, verbose):
    """One sequence's return value from its chunks' reports: (summary, per-chunk report dicts, estimated_pose, optimized_pose,
    gt_pose), the summary printed as the reference prints it (under `title` when there is one).  Without ground truth the summary is
    the mean of the seven report entries and `gt_pose` is None."""
    results, raw = [r.result for r in reports], [r.raw for r in reports]
    ground_truth = not reports or reports[0].gt is not None
    summary = OrderedDict()
    # (`ground`, `foot_lock`: a chunk's ground record with --upright and its foot-lock record with --foot_lock; no numbers to average)
    keys = [k for k in results[0] if k not in ("ground", "foot_lock")] if reports else []
    if reports and all(x is not None for x in raw):          # (every chunk of the sequence came as a row of the device report: one mean)
        mean = np.mean(np.stack(raw), axis=0)
        for i, k in enumerate(keys):
            summary[k] = mean[17:].copy() if k == "joints_error" else float(mean[i])
    elif reports:
        for k in keys:
            summary[k] = (np.mean([r[k] for r in results], axis=0) if k == "joints_error"
                          else float(np.average([r[k] for r in results])))
    if verbose and reports:
        if title is not None:
            print("sequence: {}".format(title))
        for line in SUMMARY_LINES if ground_truth else QUALITY_LINES:
            print("-----------------------------------------" if line is None else "{}: {}".format(line[0], summary[line[1]]))
        if ground_truth:
            print("joints error is: {}".format(summary["joints_error"]))
        print("-------------------------------------------------------------")
    # the pose sequences as arrays [frames,15,3] (iterating them yields the [15,3] frames the reference's lists hold)
    cat = lambda seqs: np.concatenate(seqs) if seqs else np.empty((0, 15, 3))          # noqa: E731
    return (summary, results, cat([r.est for r in reports]), cat([r.opt for r in reports]),
            cat([r.gt for r in reports]) if ground_truth else None)


# ------------------------------------------------------------------------------------------------------------------ the output files
def result_dir(root, data_id):
    """Where one chunk's files go: <root>/<dataset>/<chunk>, the last two components of `data_id` as at optimizer.py:486-498 (split as
    it stands: a caller whose names may end in a separator normalises them first)."""
    dataset_dir, seq_name = os.path.split(data_id)
    return os.path.join(root, os.path.split(dataset_dir)[1], seq_name)


@dataclass(frozen=True)
class _OutputFields:
    """The dataclass fields of `Outputs`, in their order."""
    mesh_root: object = None
    render: object = None
    render_camera: object = None
    bvh: object = None
    bvh_fps: object = None
    video: object = None
    video_camera: object = None
    video_fps: object = None
    video_quality: object = None
    foot_lock: object = None
    foot_lock_stretch: object = None
    foot_lock_blend: object = None
    upright: object = None
    upright_foot_height: object = None
    upright_lag: object = None


class Outputs(_OutputFields):
    """Which files a chunk's result is written to, and how: a root directory per kind (None: not asked for), each chunk's files
    under `result_dir` of that root.
      mesh_root      the skeleton meshes, <chunk>/{optimized,input,gt}_global_aligned/out_%04d.ply (`meshes.write_result_meshes`);
      render         the frames, <chunk>/frame_%04d.png and overview_*.png (`render.write_result_frames`);
      render_camera  the chunk as its camera saw it, <chunk>/camera_%04d.png (`render.write_result_camera_frames`);
      bvh            the sequences as animation, <chunk>/{estimated,optimized,gt}.bvh at `bvh_fps` frames per second (default 25;
                     `bvh.write_result_bvh`);
      video          the frames `render` draws -- the same view and overlay, without the overviews -- as one Motion-JPEG clip,
                     <chunk>/frames.avi; no PNG file is written for it, and it does not need `render`;
      video_camera   the images `render_camera` draws as <chunk>/camera.avi, likewise.
    Both clips play at `video_fps` frames per second (default 25) and are encoded at JPEG quality `video_quality` (default 90).
      upright        True, or a `ground.GroundEstimate`: the meshes, frames, clip and BVH files of a chunk stand in ONE upright frame -- Y up,
                     the floor at 0, the wearer at the origin facing +Z in the first frame -- of the ground estimated once per chunk from
                     its foot contacts: from the ground truth where there is one (the other sequences are
                     aligned to it), else from the optimised sequence; `upright_foot_height`: metres a standing foot point lies above
                     the floor (default 0), `upright_lag`: frames between the two frames of a still pair (default 0.2 s at `bvh_fps`).
                     The camera's views are the camera's own images and take no part.
      foot_lock      True: the optimised sequence is replaced by its foot-locked version (`foot_lock.lock_feet`, DESIGN.md section 6n:
                     standing feet pinned to the floor, the legs by two-bone inverse kinematics) for the meshes, frames, clip and BVH
                     files; the estimated sequence stays as it is, the "before".  `foot_lock_stretch`: how much longer a straight leg may
                     become to hold its pin (default 0.05); `foot_lock_blend`: frames over which a correction is eased in and out (default
                     0.12 s at `bvh_fps`); the contact rule's lag is `upright_lag`.  Ground truth, alignment and `upright` work as before,
                     on the locked sequence.
      gltf           the sequences as ONE file of skinned, animated skeletons, <chunk>/result.glb at `gltf_fps` keys per second (default
                     25; `gltf.write_result_gltf`); `upright` and `foot_lock` apply to it as to the BVH files.
    `gltf` and `gltf_fps` go by keyword only; the positional order, and with it the list of dataclass fields, is closed."""

    def __init__(self, *args, gltf=None, gltf_fps=None, **kwargs):
        super().__init__(*args, **kwargs)
        object.__setattr__(self, "gltf", gltf)          # (the record is frozen: like the fields, set once, here)
        object.__setattr__(self, "gltf_fps", gltf_fps)

    def __setattr__(self, name, value):
        raise FrozenInstanceError("cannot assign to field %r" % name)

    def __delattr__(self, name):
        raise FrozenInstanceError("cannot delete field %r" % name)

    def _key(self):
        return tuple(getattr(self, f) for f in self.__dataclass_fields__) + (self.gltf, self.gltf_fps)

    def __eq__(self, other):
        return self._key() == other._key() if other.__class__ is self.__class__ else NotImplemented

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "Outputs(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f in list(self.__dataclass_fields__) + ["gltf", "gltf_fps"])

    def _posed(self):
        """The roots of the files that show the sequences in space: what `upright` and `foot_lock` apply to."""
        return (self.mesh_root, self.render, self.bvh, self.video, self.gltf)

    def __bool__(self):
        return any(root is not None for root in (self.mesh_root, self.render, self.render_camera, self.bvh, self.video, self.video_camera, self.gltf))

    @property
    def needs_frames(self):
        """Whether `write` reads the chunk's cameras and heat-maps."""
        return self.render_camera is not None or self.video_camera is not None

    def _rates(self):
        """(bvh_fps, video_fps, video_quality) with the defaults where None was given."""
        return (animation.DEFAULT_FPS if self.bvh_fps is None else self.bvh_fps, clips.DEFAULT_FPS if self.video_fps is None else self.video_fps,
                clips.DEFAULT_QUALITY if self.video_quality is None else self.video_quality)

    def check(self):
        """ValueError for clip options no clip can be written with, before anything runs."""
        if self.video is not None or self.video_camera is not None:
            clips.check_options(*self._rates()[1:])

    def lock(self, engine, optimized):
        """The chunk's `foot_lock.FootLock` of its optimised sequence with this record's options, or None without `foot_lock`."""
        if not self.foot_lock:
            return None
        from . import foot_lock
        return foot_lock.lock_feet(engine, optimized, fps=self._rates()[0], lag=self.upright_lag, blend=self.foot_lock_blend,
                                   stretch=foot_lock.STRETCH if self.foot_lock_stretch is None else self.foot_lock_stretch)

    def write(self, engine, data_id, sequences, cams=None, heat=None, first_frame=0, locked=None):
        """One chunk's output files from `sequences` = (estimated, optimised, ground truth or None), host arrays or device tensors.
        `cams` / `heat` (`needs_frames`) hold the chunk's frames from `first_frame` on; merged frame f is the chunk's frame f.  With
        a ground truth the estimated and the optimised sequence are aligned to it and all three are written, as in the reference;
        without, nothing is aligned and there is no third sequence.  With `foot_lock` the optimised sequence is replaced by its locked
        version for every file but the camera's views (`locked`: the chunk's FootLock where the caller has made it with `lock`, else
        it is made here, once).  -> the chunk's `ground.GroundEstimate` with `upright`, else None."""
        est, opt, gt = sequences
        bvh_fps, video_fps, video_quality = self._rates()
        shown = opt          # (the camera's views show the optimiser's own result)
        if self.foot_lock and any(r is not None for r in self._posed()):
            opt = (self.lock(engine, opt) if locked is None else locked).sequence
        clip = dict(video_fps=video_fps, video_quality=video_quality, frames=False)
        frames = slice(first_frame, first_frame + len(est))
        found, extra = None, {}
        if self.upright is not None and self.upright is not False and any(r is not None for r in self._posed()):
            from . import ground
            options = {} if self.upright is not True else dict(fps=bvh_fps, lag=self.upright_lag,
                                                                foot_height=0.0 if self.upright_foot_height is None else self.upright_foot_height)
            found = ground.resolve(engine, self.upright, gt if gt is not None else opt, **options)
            extra = {"upright": found}          # (ONE estimate per chunk: its files share one frame)
        if self.mesh_root is not None:
            meshes.write_result_meshes(engine, result_dir(self.mesh_root, data_id), est, opt, gt, **extra)
        if self.render is not None:
            rendering.write_result_frames(engine, result_dir(self.render, data_id), est, opt, gt, **extra)
        if self.render_camera is not None:
            rendering.write_result_camera_frames(engine, result_dir(self.render_camera, data_id), est, shown, cams[frames], heat[frames], gt)
        if self.bvh is not None:
            animation.write_result_bvh(engine, result_dir(self.bvh, data_id), est, opt, gt, fps=bvh_fps, **extra)
        if self.gltf is not None:
            scenes.write_result_gltf(engine, result_dir(self.gltf, data_id), est, opt, gt,
                                     fps=scenes.DEFAULT_FPS if self.gltf_fps is None else self.gltf_fps, **extra)
        if self.video is not None:
            rendering.write_result_frames(engine, None, est, opt, gt, video=os.path.join(result_dir(self.video, data_id), "frames.avi"), **clip,
                                          **extra)
        if self.video_camera is not None:
            rendering.write_result_camera_frames(engine, None, est, shown, cams[frames], heat[frames], gt,
                                                 video=os.path.join(result_dir(self.video_camera, data_id), "camera.avi"), **clip)
        return found


def result_pose_dict(est, opt, mid, gt, smooth, locked=None):
    """What `result_pose.pkl` holds, in the reference's keys and containers (optimizer.py:469-483): merge_batches' lists of [15,3]
    frames; the optimised sequence an ndarray after the final smoothing (`smooth`); `gt_pose` only where there is a ground truth;
    `foot_locked_pose`, in the container of `optimized_pose`, only with `locked` (--foot_lock)."""
    d = {"estimated_pose": list(est), "optimized_pose": np.asarray(opt) if smooth else list(np.asarray(opt)), "mid_optimized_pose": list(mid)}
    if gt is not None:
        d["gt_pose"] = list(gt)
    if locked is not None:
        d["foot_locked_pose"] = np.asarray(locked) if smooth else list(np.asarray(locked))
    return d
