"""The SLAM scale of a recording without ground truth, estimated from foot contacts (no counterpart in the
reference, whose `SLAMReader.read_trajectory(path, start, end, scale=1)` takes the number as an argument).

A monocular SLAM picks an arbitrary scale on every run.  The recording itself holds the missing number: the pose network's depth
makes `estimated_local_skeleton` metric, SLAM gives the camera's rotation and its translation up to the factor s, and a foot that
stands does not move in the world -- so R_t x_t,foot + s c_t is constant over a stance phase.  `gem_slam_scale` turns that into a
robust one-parameter fit on the device, over the lifted poses where they lie; one small record comes back.

    python -m globalegomocap_amd.slam_scale --slam traj.txt (--heatmaps DIR --depths DIR | --keypoints det.npz [--depths DIR | --depth FILE.npy]) \\
        [--depth_from bones [--bones FILE.npy] [--neck_depth M] [--min_peak P] in place of the depths] --start A --end B --fps 25 [--lag K] [--tau M] [--min_pairs P] [--test_size 100] [--json FILE] [--gt gt.pkl]

`prepare --scale auto` and `detections --scale auto` (`scale="auto"`) call `estimate_scale` on the lifted poses and go on as if the
number had been given.  "The wearer did not walk enough to fix the scale" is an answer: a ValueError naming the counts.
"""
import ctypes as C
import os

import numpy as np

from . import _capi
from .ground import default_lag
from .skeleton import JOINT_NAMES

FEET = tuple(JOINT_NAMES.index(k) for k in ("Right_ankle", "Right_foot", "Left_ankle", "Left_foot"))


class ScaleEstimate:
    """`scale` (metric = scale * SLAM), `s0` the best of the 513 candidates and `g0` its index, `s_ref`, the counts `pairs`, `inliers`,
    `informative` (inliers during which the camera moved more than tau), `residual_rms` of the inliers and `path_length`, metres,
    `stance_share` (right, left), `per_chunk` [n_chunks] the scale each chunk's inliers give on their own (NaN: none; their spread
    shows a drifting SLAM scale) with `per_chunk_sums` [n_chunks,2] the numerators and denominators, the call's `lag`, `tau`,
    `min_pairs`, and `costs`: the 513 candidate costs as a device tensor."""

    def __init__(self, report, costs=None):
        r = np.asarray(report, dtype=np.float64)
        head = _capi.GemScaleReport.from_buffer_copy(r[:_capi.SCALE_REPORT_DOUBLES].tobytes())
        self.scale, self.s0, self.s_ref, self.g0 = head.scale, head.s0, head.s_ref, int(head.g0)
        self.pairs, self.inliers, self.informative = int(head.pairs), int(head.inliers), int(head.informative)
        self.residual_rms, self.path_length = head.residual_rms, head.path_length
        self.stance_share = (head.stance_right, head.stance_left)
        self.status, self.lag, self.tau, self.min_pairs = int(head.status), int(head.lag), head.tau, int(head.min_pairs)
        rest = r[_capi.SCALE_REPORT_DOUBLES:].reshape(-1, 3)
        self.per_chunk_sums, self.per_chunk = rest[:, :2].copy(), rest[:, 2].copy()
        self.costs = costs
        self.report = r

    def as_dict(self):
        """Plain numbers and lists (JSON)."""
        return {"scale": self.scale, "s0": self.s0, "s_ref": self.s_ref, "pairs": self.pairs, "inliers": self.inliers,
                "informative": self.informative, "residual_rms": self.residual_rms, "path_length": self.path_length,
                "stance_share": list(self.stance_share), "per_chunk": [float(v) for v in self.per_chunk], "lag": self.lag, "tau": self.tau,
                "min_pairs": self.min_pairs}

    def line(self):
        return ("SLAM scale estimate: %.9g (%d pairs %d frames apart, %d inliers, %d informative, residual RMS %.4f m, path %.2f m, "
                "stance right / left %.2f / %.2f)" % ((self.scale, self.pairs, self.lag, self.inliers, self.informative, self.residual_rms,
                                                       self.path_length) + self.stance_share))


def selected_poses(rows_or_text, spans, fps):
    """The trajectory lines of the spans' frame ids, in span order -> (R [N,3,3], c [N,3], ids [N] int64): `slam.relative_poses` of
    them all together, so relative to the recording's first frame, unscaled."""
    from . import slam
    rows = rows_or_text if isinstance(rows_or_text, np.ndarray) else slam.trajectory_rows(rows_or_text)
    ids = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in spans]) if len(spans) else np.empty(0, dtype=np.int64)
    if not len(ids):
        return np.empty((0, 3, 3)), np.empty((0, 3)), ids
    # one pass for all spans (a recording of 100 000 frames has a thousand of them): every wanted id must have exactly one line
    line_ids = slam.frame_ids(rows, fps)
    order = np.argsort(line_ids, kind="stable")
    first, behind = np.searchsorted(line_ids[order], ids, side="left"), np.searchsorted(line_ids[order], ids, side="right")
    if (behind - first != 1).any():
        missing, several = ids[behind == first], ids[behind - first > 1]
        raise ValueError("at %g fps the trajectory has %s" % (fps, " and ".join(
            what % v.tolist() for what, v in (("no line for frame ids %s", missing), ("several lines for frame ids %s", several)) if len(v))))
    picked = rows[order[first]]
    rt, rq = slam.relative_poses(picked[:, 1:4], picked[:, 4:8])
    return slam.pose_matrix(rt, rq)[:, :3, :3], rt, ids


def scale_call(chunks, R, c, ids, lag, tau=0.10, min_pairs=50, feet=None, stream=None, read_back=True):
    """gem_slam_scale.  chunks: device tensors [n_k,J,3] f64, each its own allocation or not; R [N,3,3], c [N,3], ids [N] (host).
    -> (return code, report as numpy [16 + 3 n_chunks] or the device tensor when not read_back, costs device tensor [513], message)."""
    import torch
    lib = _capi.load_library()
    chunks = list(chunks)
    for x in chunks:
        if not (x.is_cuda and x.dtype == torch.float64 and x.dim() == 3 and x.shape[2] == 3 and x.is_contiguous()):
            raise ValueError("estimate_scale: the poses must be contiguous float64 device tensors [n,J,3]")
    J = int(chunks[0].shape[1])
    if any(int(x.shape[1]) != J for x in chunks):
        raise ValueError("estimate_scale: the chunks differ in their number of joints")
    device = chunks[0].device
    starts = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
    N, nc = int(starts[-1]), len(chunks)
    R, c = np.ascontiguousarray(R, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    if R.shape != (N, 3, 3) or c.shape != (N, 3) or ids.shape != (N,):
        raise ValueError("estimate_scale: %d frames of poses, but SLAM poses %s %s and frame ids %s" % (N, R.shape, c.shape, ids.shape))
    if not (np.isfinite(R).all() and np.isfinite(c).all()):
        raise ValueError("estimate_scale: the SLAM poses hold values that are not finite")
    feet = FEET if feet is None else tuple(int(j) for j in feet)
    if len(feet) != 4:
        raise ValueError("estimate_scale: feet = (right ankle, right foot, left ankle, left foot)")
    table = np.concatenate([np.array([x.data_ptr() if len(x) else 0 for x in chunks], dtype=np.int64), starts])
    need = int(lib.gem_slam_scale_work(max(N, 1), int(lag), nc))
    if need < 0:          # (sizes out of range: gem_slam_scale itself refuses them, with its own text)
        need = 8
    with torch.cuda.device(device):
        st = torch.cuda.current_stream() if stream is None else stream
        with torch.cuda.stream(st):
            # ONE upload: the chunk table, the frame ids and the SLAM poses
            up = torch.from_numpy(np.concatenate([table, ids, R.reshape(-1).view(np.int64), c.reshape(-1).view(np.int64)])).to(device)
            d_chunks, d_ids = up[:len(table)], up[len(table):len(table) + N]
            d_rot, d_trans = up[len(table) + N:len(table) + 10 * N], up[len(table) + 10 * N:]
            work = torch.empty(need // 8 + 1, dtype=torch.float64, device=device)
            n_rep = _capi.SCALE_REPORT_DOUBLES + 3 * nc
            report = torch.zeros(n_rep, dtype=torch.float64, device=device)
            costs = torch.zeros(_capi.SCALE_CANDIDATES, dtype=torch.float64, device=device)
            host = np.zeros(n_rep, dtype=np.float64)
            rc = lib.gem_slam_scale(C.c_void_p(table.ctypes.data), C.c_void_p(d_chunks.data_ptr()), nc, J, (C.c_int * 4)(*feet),
                                    C.c_void_p(d_rot.data_ptr()), C.c_void_p(d_trans.data_ptr()), C.c_void_p(d_ids.data_ptr()), N, int(lag),
                                    float(tau), int(min_pairs), C.c_void_p(work.data_ptr()), need, C.c_void_p(report.data_ptr()),
                                    C.c_void_p(costs.data_ptr()), C.c_void_p(host.ctypes.data if read_back else 0), C.c_void_p(st.cuda_stream))
            for t in (up, work):
                t.record_stream(st)
    msg = (lib.gem_last_error() or b"").decode() if rc else ""
    return rc, (host if read_back else report), costs, msg


def tracked_poses(est_local, rows, spans, fps):
    """The estimator's inputs for a recording with lost frames: the tracked frames of the spans (which follow one another) alone.
    `est_local`: ONE device tensor holding the spans' poses in order; `rows`: `slam.trajectory_rows`.
    -> ([the tracked frames' poses per span], R, c, ids) as `selected_poses` gives them for a whole trajectory."""
    import torch
    from . import slam
    from .slam_bridge import contiguous_span, tracked_mask, tracked_rows
    A, B = contiguous_span(spans)
    picked, ids = tracked_rows(rows, A, B, fps)
    mask = tracked_mask(ids, A, B)
    rt, rq = slam.relative_poses(picked[:, 1:4], picked[:, 4:8])
    R = slam.pose_matrix(rt, rq)[:, :3, :3]
    keep = torch.from_numpy(np.flatnonzero(mask)).to(est_local.device)
    kept = est_local.index_select(0, keep).contiguous()
    cuts = np.concatenate([[0], np.cumsum([int(mask[a - A:b - A].sum()) for a, b in spans])])
    return [kept[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])], R, rt, ids


def estimate_scale(est_local, rows_or_text, spans, fps, *, lag=None, tau=0.10, min_pairs=50, feet=None, stream=None, tracked=False):
    """The SLAM scale of the recording whose lifted poses are `est_local` -- one device tensor [n,15,3] float64 per span of `spans`
    [(start_frame, end_frame)], or ONE tensor holding them all in order -- and whose trajectory is `rows_or_text`
    (`slam.trajectory_rows`, or the file's text).  On the detection route these are the poses after `gem_fill_missing`.
    `tracked`: the trajectory lacks lines (`slam_bridge`); only the tracked rows and their poses are passed (`tracked_poses`), and
    since the estimator pairs rows where their frame ids lie `lag` apart, no pair reaches across a gap.
    -> ScaleEstimate; ValueError naming the counts when the recording does not fix the scale."""
    import torch
    spans = [(int(a), int(b)) for a, b in spans]
    if tracked:
        est_local, R, c, ids = tracked_poses(est_local, rows_or_text, spans, fps)
    else:
        if torch.is_tensor(est_local):
            cuts = np.concatenate([[0], np.cumsum([b - a for a, b in spans])])
            if int(cuts[-1]) != len(est_local):
                raise ValueError("estimate_scale: %d frames of poses for spans of %d frames" % (len(est_local), int(cuts[-1])))
            est_local = [est_local[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
        est_local = list(est_local)
        if len(est_local) != len(spans) or any(len(x) != b - a for x, (a, b) in zip(est_local, spans)):
            raise ValueError("estimate_scale: one tensor of end - start frames per span is needed")
        if not spans:
            raise ValueError("estimate_scale: no frames, so no pairs (0 pairs, 0 inliers, 0 informative)")
        R, c, ids = selected_poses(rows_or_text, spans, fps)
    lag = default_lag(fps) if lag is None else int(lag)
    rc, report, costs, msg = scale_call(est_local, R, c, ids, lag, tau, min_pairs, feet, stream)
    if rc in (_capi.SCALE_NO_PAIRS, _capi.SCALE_TOO_FEW, _capi.SCALE_BAD_SCALE):
        raise ValueError(msg.replace("gem_slam_scale: ", "the SLAM scale cannot be estimated: "))
    if rc:
        raise _capi.GemError(msg or "gem_slam_scale failed")
    return ScaleEstimate(report, costs)


# ------------------------------------------------------------------------------------------------------------------ command line
def scale_arg(text):
    """argparse type of `--scale`: a positive number (-> float, as before) or the word `auto`."""
    import argparse
    if text == "auto":
        return "auto"
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("a positive number or `auto` is needed, got %r" % text)
    if not (np.isfinite(v) and v > 0):
        raise argparse.ArgumentTypeError("the SLAM scale must be a positive number, got %r" % text)
    return v


def full_spans(start, end, test_size):
    """[start, end) cut into chunks of test_size frames, the last one shorter: the partition of the per-chunk scales."""
    return [(i, min(i + test_size, end)) for i in range(start, end, test_size)]


def umeyama_scales(rows, rec, gt_path, fps, gt_start):
    """Per chunk of `rec` the scale `slam.camera_pose_list_from_heads` fits against the ground truth's head track."""
    from . import prepare, slam
    from .errors import umeyama
    pose_gt = prepare.read_gt(gt_path)
    out = []
    for ch in rec.chunks:
        a, b = ch.start_frame, ch.end_frame
        gt_head = np.asarray(prepare.gt_clip(pose_gt, a, b, gt_start), dtype=np.float64)[:, 0]
        rt, rq = slam.relative_poses(*slam.parse_trajectory(rows, a, b, fps))
        slam_head = np.einsum("nij,nj->ni", slam.pose_matrix(rt, rq)[:, :3, :3], ch.est_local[:, 0].cpu().numpy()) + rt
        out.append(float(umeyama(slam_head, gt_head)[0]))
    return out


def _parser():
    import argparse
    from .camera import DEFAULT_CALIBRATION
    p = argparse.ArgumentParser(description="estimate the SLAM scale of a recording from its foot contacts")
    p.add_argument("--slam", required=True, help="SLAM trajectory: lines `time tx ty tz qx qy qz qw`")
    p.add_argument("--heatmaps", default=None, metavar="DIR", help="directory of per-frame heatmap .mat files (with --depths)")
    p.add_argument("--keypoints", default=None, metavar="FILE", help=".npy / .npz of 2-D detections (`detections`)")
    p.add_argument("--depths", default=None, metavar="DIR", help="directory of per-frame depth .mat files")
    p.add_argument("--depth", default=None, metavar="FILE.npy", help="the joints' depths [N,15], row for row with the detections")
    p.add_argument("--depth_from", default=None, choices=("bones",), help="bones: no depths at all -- they are solved from the bone lengths "
                                                                         "(DESIGN.md sections 6q, 6r); excludes --depths and --depth")
    from .bone_depth import add_bone_depth_options
    add_bone_depth_options(p)
    p.add_argument("--min_peak", type=float, default=None, metavar="P", help="with --heatmaps --depth_from bones: a joint whose map peaks "
                                                                             "below P is treated as not detected (default 0)")
    p.add_argument("--start", required=True, type=int)
    p.add_argument("--end", required=True, type=int)
    p.add_argument("--fps", type=float, default=25)
    p.add_argument("--lag", type=int, default=None, help="frames between the two frames of a pair (default: 0.2 s)")
    p.add_argument("--tau", type=float, default=0.10, help="metres a standing foot may seem to move")
    p.add_argument("--min_pairs", type=int, default=50)
    p.add_argument("--test_size", type=int, default=100, help="frames per chunk of the per-chunk scales")
    p.add_argument("--first_id", type=int, default=0, help="frame id of the detections' first row (without frame_ids)")
    p.add_argument("--json", default=None, metavar="FILE", help="write the report there too")
    p.add_argument("--gt", default=None, help="ground-truth pickle: print the per-chunk Umeyama scale beside the estimate")
    p.add_argument("--mat_start", type=int, default=None, help="frame id of the GT pickle's first entry (default: --start)")
    p.add_argument("--camera", default=DEFAULT_CALIBRATION)
    return p


def _cli(argv=None):
    import json
    from . import detections, prepare, slam
    p = _parser()
    a = p.parse_args(argv)
    if (a.heatmaps is None) == (a.keypoints is None):
        p.error("give --heatmaps DIR --depths DIR, or --keypoints FILE")
    if a.depth_from is not None and (a.depths is not None or a.depth is not None):
        p.error("--depth_from bones excludes --depths and --depth")
    if a.heatmaps is not None and ((a.depths is None and a.depth_from is None) or a.depth is not None):
        p.error("--heatmaps needs --depths DIR or --depth_from bones")
    if a.depth_from is None and (a.bones is not None or a.neck_depth is not None or a.min_peak is not None):
        p.error("--bones, --neck_depth and --min_peak belong to --depth_from bones")
    if a.min_peak is not None and a.heatmaps is None:
        p.error("--min_peak goes with --heatmaps: detections carry their own confidence")
    from .bone_depth import bones_from_args
    spans = full_spans(a.start, a.end, a.test_size)
    options = dict(lag=a.lag, tau=a.tau, min_pairs=a.min_pairs)
    if a.depth_from is not None:
        options.update(depth=a.depth_from, bones=bones_from_args(a), neck_depth=a.neck_depth)
    if a.heatmaps is not None:
        rec = prepare.prepare_spans(a.slam, a.heatmaps, a.depths, None, spans, a.fps, a.start, a.camera, scale="auto", min_peak=a.min_peak, **options)
    else:
        rec = detections.recording_from_detections(a.slam, detections.detections_from_args(a), None, "auto", spans, a.fps,
                                                   camera_model_path=a.camera, **options)
    est = rec.scale_report
    print(est.line())
    out = est.as_dict()
    umeyama_per_chunk = None
    if a.gt is not None:
        with open(a.slam) as f:
            rows = slam.trajectory_rows(f.read())
        umeyama_per_chunk = umeyama_scales(rows, rec, a.gt, a.fps, a.start if a.mat_start is None else a.mat_start)
        out["umeyama_per_chunk"] = umeyama_per_chunk
    for k, ((s, e), v) in enumerate(zip(spans, est.per_chunk)):
        print("chunk %d [%d, %d): scale %.9g%s" % (k, s, e, v, "" if umeyama_per_chunk is None else "   Umeyama against the ground truth %.9g" % umeyama_per_chunk[k]))
    if a.json is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return est


if __name__ == "__main__":
    _cli()
