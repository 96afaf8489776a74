"""The SLAM scale of a recording without ground truth, estimated from foot contacts (no counterpart in the
reference, whose `SLAMReader.read_trajectory(path, start, end, scale=1)` takes the number as an argument).

A monocular SLAM picks an arbitrary scale on every run.  The recording itself holds the missing number: the pose network's depth
makes `estimated_local_skeleton` metric, SLAM gives the camera's rotation and its translation up to the factor s, and a foot that
stands does not move in the world -- so R_t x_t,foot + s c_t is constant over a stance phase.  `gem_slam_scale` turns that into a
robust one-parameter fit on the device, over the lifted poses where they lie; one small record comes back.

    python -m globalegomocap_amd.slam_scale --slam traj.txt (--heatmaps DIR --depths DIR | --keypoints det.npz [--depths DIR | --depth FILE.npy]) \\
        [--depth_from bones [--bones FILE.npy] [--neck_depth M] [--min_peak P] in place of the depths] --start A --end B --fps 25 [--scale auto|drift [--knot S] [--stiffness W]] [--lag K] [--tau M] [--min_pairs P] [--test_size 100] [--json FILE] [--gt gt.pkl]

`prepare --scale auto` and `detections --scale auto` (`scale="auto"`) call `estimate_scale` on the lifted poses and go on as if the
number had been given.  `--scale drift [--knot SECONDS] [--stiffness W]` (`scale="drift"`) is for a SLAM whose
scale creeps over the recording: `estimate_drift` fits a piecewise-linear scale curve to the same stance pairs with `gem_slam_drift`,
rebuilds the camera track in metres, and the routes go on with that track as a metric SLAM's at scale 1.  "The wearer did not walk enough to fix the scale" is an answer: a ValueError naming
the counts.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._binding import _ptr, check_tensor, staged_call
from .ground import default_lag, write_json
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


def _call_inputs(chunks, R, c, ids, feet, who):
    """What a device call checks of its inputs and lays out for its one upload -> (chunks, J, device, N, n_chunks, R, c, ids, feet,
    table: the chunks' addresses and first rows)."""
    import torch
    chunks = list(chunks)
    for x in chunks:
        check_tensor(x, torch.float64, (None, None, 3), error=ValueError("%s: the poses must be contiguous float64 device tensors [n,J,3]" % who))
    J = int(chunks[0].shape[1])
    if any(int(x.shape[1]) != J for x in chunks):
        raise ValueError("%s: the chunks differ in their number of joints" % who)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
    N, nc = int(starts[-1]), len(chunks)
    R, c = np.ascontiguousarray(R, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    if R.shape != (N, 3, 3) or c.shape != (N, 3) or ids.shape != (N,):
        raise ValueError("%s: %d frames of poses, but SLAM poses %s %s and frame ids %s" % (who, N, R.shape, c.shape, ids.shape))
    if not (np.isfinite(R).all() and np.isfinite(c).all()):
        raise ValueError("%s: the SLAM poses hold values that are not finite" % who)
    feet = FEET if feet is None else tuple(int(j) for j in feet)
    if len(feet) != 4:
        raise ValueError("%s: feet = (right ankle, right foot, left ankle, left foot)" % who)
    table = np.concatenate([np.array([x.data_ptr() if len(x) else 0 for x in chunks], dtype=np.int64), starts])
    return chunks, J, chunks[0].device, N, nc, R, c, ids, feet, table


def scale_call(chunks, R, c, ids, lag, tau=0.10, min_pairs=50, feet=None, stream=None, read_back=True):
    """gem_slam_scale.  chunks: device tensors [n_k,J,3] f64, each its own allocation or not; R [N,3,3], c [N,3], ids [N] (host).
    -> (return code, report as numpy [16 + 3 n_chunks] or the device tensor when not read_back, costs device tensor [513], message)."""
    import torch
    lib = _capi.load_library()
    chunks, J, device, N, nc, R, c, ids, feet, table = _call_inputs(chunks, R, c, ids, feet, "estimate_scale")
    need = int(lib.gem_slam_scale_work(max(N, 1), int(lag), nc))
    if need < 0:          # (sizes out of range: gem_slam_scale itself refuses them, with its own text)
        need = 8
    with staged_call(lib, device, stream) as call:
        d_chunks, d_ids, d_rot, d_trans = call.upload(table, ids, R, c)          # (ONE upload: the chunk table, the frame ids, the SLAM poses)
        n_rep = _capi.SCALE_REPORT_DOUBLES + 3 * nc
        report = torch.zeros(n_rep, dtype=torch.float64, device=device)
        costs = torch.zeros(_capi.SCALE_CANDIDATES, dtype=torch.float64, device=device)
        host = np.zeros(n_rep, dtype=np.float64)
        rc, msg = call.run(lib.gem_slam_scale, C.c_void_p(table.ctypes.data), _ptr(d_chunks), nc, J, (C.c_int * 4)(*feet), _ptr(d_rot), _ptr(d_trans),
                           _ptr(d_ids), N, int(lag), float(tau), int(min_pairs), _ptr(call.work(need)), need, _ptr(report), _ptr(costs),
                           C.c_void_p(host.ctypes.data if read_back else 0))
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


def _recording_inputs(est_local, rows_or_text, spans, fps, tracked, who):
    """The estimators' inputs from a recording's lifted poses and trajectory -> ([poses per span], R, c, ids)."""
    import torch
    spans = [(int(a), int(b)) for a, b in spans]
    if tracked:
        return tracked_poses(est_local, rows_or_text, spans, fps)
    if torch.is_tensor(est_local):
        cuts = np.concatenate([[0], np.cumsum([b - a for a, b in spans])])
        if int(cuts[-1]) != len(est_local):
            raise ValueError("%s: %d frames of poses for spans of %d frames" % (who, len(est_local), int(cuts[-1])))
        est_local = [est_local[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
    est_local = list(est_local)
    if len(est_local) != len(spans) or any(len(x) != b - a for x, (a, b) in zip(est_local, spans)):
        raise ValueError("%s: one tensor of end - start frames per span is needed" % who)
    if not spans:
        raise ValueError("%s: no frames, so no pairs (0 pairs, 0 inliers, 0 informative)" % who)
    return (est_local,) + tuple(selected_poses(rows_or_text, spans, fps))


def estimate_scale(est_local, rows_or_text, spans, fps, *, lag=None, tau=0.10, min_pairs=50, feet=None, stream=None, tracked=False):
    """The SLAM scale of the recording whose lifted poses are `est_local` -- one device tensor [n,15,3] float64 per span of `spans`
    [(start_frame, end_frame)], or ONE tensor holding them all in order -- and whose trajectory is `rows_or_text`
    (`slam.trajectory_rows`, or the file's text).  On the detection route these are the poses after `gem_fill_missing`.
    `tracked`: the trajectory lacks lines (`slam_bridge`); only the tracked rows and their poses are passed (`tracked_poses`), and
    since the estimator pairs rows where their frame ids lie `lag` apart, no pair reaches across a gap.
    -> ScaleEstimate; ValueError naming the counts when the recording does not fix the scale."""
    est_local, R, c, ids = _recording_inputs(est_local, rows_or_text, spans, fps, tracked, "estimate_scale")
    lag = default_lag(fps) if lag is None else int(lag)
    rc, report, costs, msg = scale_call(est_local, R, c, ids, lag, tau, min_pairs, feet, stream)
    if rc in (_capi.SCALE_NO_PAIRS, _capi.SCALE_TOO_FEW, _capi.SCALE_BAD_SCALE):
        raise ValueError(msg.replace("gem_slam_scale: ", "the SLAM scale cannot be estimated: "))
    if rc:
        raise _capi.GemError(msg or "gem_slam_scale failed")
    return ScaleEstimate(report, costs)


# ------------------------------------------------------------------------------------- a scale that drifts
def default_knot(fps):
    """Frames between two knots of the scale curve: 10 s."""
    return max(1, int(round(10.0 * fps)))


class DriftEstimate:
    """A scale that drifts within the recording, as a piecewise-linear curve: `global_estimate` (the `ScaleEstimate` it started from),
    `knot_ids` [K] frame ids and `knot_scale` [K] the curve there, `interval_count` / `interval_bb` [K-1] the inlier pairs between two
    knots and their sum <b,b> (0: the curve is interpolated there), the record's `inliers`, `informative`, `residual_rms`, `scale_min`,
    `scale_max`, `scale_mean` (metric path length / SLAM path length: the one number a reader may quote), `metric_length`,
    `slam_length`, `lam`, the call's `knot`, `stiffness`, `lag`, `tau`; `frame_ids` [N] and `metric` [N,3] the camera track in metres
    relative to the first frame, with `quats` [N,4] the relative rotations, which the curve leaves alone."""

    def __init__(self, report, knots, metric, global_estimate, frame_ids, fps, quats):
        self.report = np.asarray(report, dtype=np.float64)
        head = _capi.GemDriftReport.from_buffer_copy(self.report[:_capi.DRIFT_REPORT_DOUBLES].tobytes())
        self.status, self.n_knots, self.knot, self.stiffness = int(head.status), int(head.n_knots), int(head.knot), head.stiffness
        self.inliers, self.informative, self.residual_rms = int(head.inliers), int(head.informative), head.residual_rms
        self.scale_min, self.scale_max, self.scale_mean = head.scale_min, head.scale_max, head.scale_mean
        self.metric_length, self.slam_length, self.lam = head.metric_length, head.slam_length, head.lam
        knots = np.asarray(knots, dtype=np.float64).reshape(-1, 4)
        self.knot_ids = int(head.first_id) + self.knot * np.arange(len(knots), dtype=np.int64)
        self.knot_scale = knots[:, 0].copy()
        self.interval_count, self.interval_bb = knots[:-1, 1].astype(np.int64), knots[:-1, 2].copy()
        self.metric = np.asarray(metric, dtype=np.float64)
        self.global_estimate = global_estimate
        self.frame_ids, self.fps, self.quats = np.asarray(frame_ids, dtype=np.int64), fps, np.asarray(quats, dtype=np.float64)
        self.lag, self.tau, self.min_pairs = global_estimate.lag, global_estimate.tau, global_estimate.min_pairs
        self.per_chunk = global_estimate.per_chunk
        self.scale = self.scale_mean

    def metric_rows(self):
        """Trajectory rows `time tx ty tz qx qy qz qw` of the frames the estimate covers: the metric track and the relative rotations.
        The first row is the identity pose, so `slam.relative_poses` of these rows gives the metric track back as it is, and a recording
        prepared from them with scale 1 is the one this estimate describes."""
        quats = self.quats.copy()
        quats[0] = (0.0, 0.0, 0.0, 1.0)          # (exactly: the first frame relative to itself)
        return np.concatenate([(self.frame_ids / self.fps)[:, None], self.metric, quats], axis=1)

    def as_dict(self):
        """Plain numbers and lists (JSON)."""
        d = self.global_estimate.as_dict()
        d.update({"global_scale": self.global_estimate.scale, "scale": self.scale_mean, "scale_mean": self.scale_mean, "scale_min": self.scale_min,
                  "scale_max": self.scale_max, "knot": self.knot, "stiffness": self.stiffness, "knot_ids": self.knot_ids.tolist(),
                  "knot_scale": [float(v) for v in self.knot_scale], "interval_count": self.interval_count.tolist(),
                  "interval_bb": [float(v) for v in self.interval_bb], "inliers": self.inliers, "informative": self.informative,
                  "residual_rms": self.residual_rms, "metric_length": self.metric_length, "slam_length": self.slam_length})
        return d

    def knot_lines(self):
        """One line per knot: where, the curve there, and what informed the interval to its right."""
        out = []
        for k, (i, s) in enumerate(zip(self.knot_ids, self.knot_scale)):
            right = "" if k == self.n_knots - 1 else ("   %d inlier pairs to its right" % self.interval_count[k] if self.interval_count[k]
                                                       else "   interpolated: no inlier pairs to its right")
            out.append("knot %d at frame %d: scale %.9g%s" % (k, i, s, right))
        return out

    def line(self):
        return ("SLAM scale drift: %.9g .. %.9g over %d knots %d frames apart (mean %.9g, one scale for all: %.9g; %d inliers, %d informative, "
                "residual RMS %.4f m, path %.2f m)" % (self.scale_min, self.scale_max, self.n_knots, self.knot, self.scale_mean,
                                                       self.global_estimate.scale, self.inliers, self.informative, self.residual_rms, self.metric_length))


def drift_call(chunks, R, c, ids, lag, knot, stiffness=1.0, tau=0.10, min_pairs=50, feet=None, stream=None, read_back=True, work_bytes=None,
               outputs=None):
    """gem_slam_drift.  The inputs as `scale_call` takes them; knot: frames between knots.  outputs: (scale report, knots, metric,
    report) device tensors to write into (default: zeros).  -> (return code, {"scale_report", "costs", "knots", "metric", "report"}:
    numpy arrays, or the device tensors when not read_back, message)."""
    import torch
    lib = _capi.load_library()
    chunks, J, device, N, nc, R, c, ids, feet, table = _call_inputs(chunks, R, c, ids, feet, "estimate_drift")
    if N < 1 or (np.diff(ids) <= 0).any():
        raise ValueError("estimate_drift: at least one frame is needed, and the frame ids must rise")
    knot = int(knot)
    K = max(2, -(-int(ids[-1] - ids[0]) // knot) + 1) if knot >= 1 else 2
    K_alloc = min(K, _capi.DRIFT_MAX_KNOTS)
    need = int(lib.gem_slam_drift_work(N, int(lag), K_alloc))
    if need < 0:          # (sizes out of range: the call itself refuses them, with its own text)
        need = 8
    need = need if work_bytes is None else int(work_bytes)
    n_rep = _capi.SCALE_REPORT_DOUBLES + 3 * nc
    with staged_call(lib, device, stream) as call:
        d_chunks, d_ids, d_rot, d_trans = call.upload(table, ids, R, c)          # (ONE upload, as in `scale_call`)
        costs = torch.zeros(_capi.SCALE_CANDIDATES, dtype=torch.float64, device=device)
        if outputs is None:
            outputs = (torch.zeros(n_rep, dtype=torch.float64, device=device), torch.zeros(K_alloc, 4, dtype=torch.float64, device=device),
                       torch.zeros(N, 3, dtype=torch.float64, device=device), torch.zeros(_capi.DRIFT_REPORT_DOUBLES, dtype=torch.float64, device=device))
        host = [np.zeros(tuple(t.shape), dtype=np.float64) if t is not None else None for t in outputs]
        hp = [C.c_void_p(h.ctypes.data if (read_back and h is not None) else 0) for h in host]
        dp = [_ptr(t) for t in outputs]
        rc, msg = call.run(lib.gem_slam_drift, C.c_void_p(table.ctypes.data), _ptr(d_chunks), nc, J, (C.c_int * 4)(*feet), _ptr(d_rot), _ptr(d_trans),
                           _ptr(d_ids), N, int(ids[0]), int(ids[-1]), int(lag), float(tau), int(min_pairs), knot, float(stiffness),
                           _ptr(call.work(need)), need, dp[0], _ptr(costs), dp[1], dp[2], dp[3], hp[0], hp[1], hp[2], hp[3])
    got = host if read_back else list(outputs)
    return rc, {"scale_report": got[0], "costs": costs, "knots": got[1], "metric": got[2], "report": got[3]}, msg


def estimate_drift(est_local, rows_or_text, spans, fps, *, knot=None, stiffness=1.0, lag=None, tau=0.10, min_pairs=50, feet=None, stream=None,
                   tracked=False):
    """`estimate_scale` for a SLAM whose scale creeps over the recording: the same inputs, `knot` frames between
    the knots of the curve (default 10 s) and `stiffness` of its second differences.  -> DriftEstimate, whose `metric_rows()` are the
    trajectory in metres; ValueError when the recording does not fix one scale (`estimate_scale`'s refusals, with their counts) or
    does not fix the curve (the knot intervals without inlier pairs are named)."""
    from . import slam
    rows = rows_or_text if isinstance(rows_or_text, np.ndarray) else slam.trajectory_rows(rows_or_text)
    est_local, R, c, ids = _recording_inputs(est_local, rows, spans, fps, tracked, "estimate_drift")
    lag = default_lag(fps) if lag is None else int(lag)
    knot = default_knot(fps) if knot is None else int(knot)
    if not (np.isfinite(stiffness) and stiffness >= 0):
        raise ValueError("estimate_drift: stiffness must be a finite number >= 0, got %r" % (stiffness,))
    if knot < lag + 1:
        raise ValueError("estimate_drift: knots %d frames apart, but a pair alone is %d frames long" % (knot, lag))
    rc, out, msg = drift_call(est_local, R, c, ids, lag, knot, stiffness, tau, min_pairs, feet, stream)
    if rc in (_capi.SCALE_NO_PAIRS, _capi.SCALE_TOO_FEW, _capi.SCALE_BAD_SCALE):
        raise ValueError(msg.replace("gem_slam_scale: ", "the SLAM scale cannot be estimated: "))
    if rc == _capi.DRIFT_NOT_SOLVED:
        counts = out["knots"][:-1, 1]
        empty = ", ".join("%d-%d" % (k, k + 1) for k in np.flatnonzero(counts == 0)) or "none"
        raise ValueError(msg.replace("gem_slam_drift: ", "the SLAM scale's drift cannot be estimated: ") + "; no inlier pairs between knots " + empty)
    if rc:
        raise _capi.GemError(msg or "gem_slam_drift failed")
    # the relative rotations of the frames the estimate covers, as quaternions: what `slam.relative_poses` makes of their lines
    line_ids = slam.frame_ids(rows, fps)
    order = np.argsort(line_ids, kind="stable")
    picked = rows[order[np.searchsorted(line_ids[order], ids, side="left")]]
    _, rq = slam.relative_poses(picked[:, 1:4], picked[:, 4:8])
    return DriftEstimate(out["report"], out["knots"], out["metric"], ScaleEstimate(out["scale_report"], out["costs"]), ids, fps, rq)


# ------------------------------------------------------------------------------------------------------------------ command line
def scale_arg(text):
    """argparse type of `--scale`: a positive number (-> float, as before), the word `auto`, or the word `drift`."""
    import argparse
    if text in ("auto", "drift"):
        return text
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("a positive number, `auto` or `drift` is needed, got %r" % text)
    if not (np.isfinite(v) and v > 0):
        raise argparse.ArgumentTypeError("the SLAM scale must be a positive number, got %r" % text)
    return v


def add_drift_options(p):
    """`--knot` and `--stiffness` of `--scale drift` (`prepare`, `detections`, `continuous`, `slam_scale`)."""
    p.add_argument("--knot", type=float, default=None, metavar="SECONDS", help="with --scale drift: seconds between two knots of the scale "
                                                                               "curve (default 10)")
    p.add_argument("--stiffness", type=float, default=None, help="with --scale drift: weight of the curve's second differences (default 1)")


def drift_options(p, a):
    """The rules of `add_drift_options`, as parser errors -> {knot: frames or None, stiffness}."""
    if (a.knot is not None or a.stiffness is not None) and a.scale != "drift":
        p.error("--knot and --stiffness belong to --scale drift")
    if a.knot is not None and not (np.isfinite(a.knot) and a.knot > 0):
        p.error("--knot must be a positive number of seconds")
    if a.stiffness is not None and not (np.isfinite(a.stiffness) and a.stiffness >= 0):
        p.error("--stiffness must be a finite number >= 0")
    return {"knot": None if a.knot is None else max(1, int(round(a.knot * a.fps))), "stiffness": 1.0 if a.stiffness is None else a.stiffness}


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
    from .prepare import add_depth_route_options
    p = argparse.ArgumentParser(description="estimate the SLAM scale of a recording from its foot contacts")
    p.add_argument("--slam", required=True, help="SLAM trajectory: lines `time tx ty tz qx qy qz qw`")
    p.add_argument("--heatmaps", default=None, metavar="DIR", help="directory of per-frame heatmap .mat files (with --depths)")
    p.add_argument("--keypoints", default=None, metavar="FILE", help=".npy / .npz of 2-D detections (`detections`)")
    add_depth_route_options(p, depth_file="the joints' depths [N,15], row for row with the detections", peaks=False,
                            depth_from="bones: no depths at all -- they are solved from the bone lengths (DESIGN.md sections 6q, 6r); excludes "
                                       "--depths and --depth",
                            min_peak="with --heatmaps --depth_from bones: a joint whose map peaks below P is treated as not detected (default 0)")
    p.add_argument("--start", required=True, type=int)
    p.add_argument("--end", required=True, type=int)
    p.add_argument("--fps", type=float, default=25)
    p.add_argument("--lag", type=int, default=None, help="frames between the two frames of a pair (default: 0.2 s)")
    p.add_argument("--tau", type=float, default=0.10, help="metres a standing foot may seem to move")
    p.add_argument("--min_pairs", type=int, default=50)
    p.add_argument("--scale", default="auto", choices=("auto", "drift"), help="auto: one scale for the recording; drift: a curve over it "
                                                                              "(DESIGN.md section 6t)")
    add_drift_options(p)
    p.add_argument("--test_size", type=int, default=100, help="frames per chunk of the per-chunk scales")
    p.add_argument("--first_id", type=int, default=0, help="frame id of the detections' first row (without frame_ids)")
    p.add_argument("--json", default=None, metavar="FILE", help="write the report there too")
    p.add_argument("--gt", default=None, help="ground-truth pickle: print the per-chunk Umeyama scale beside the estimate")
    p.add_argument("--mat_start", type=int, default=None, help="frame id of the GT pickle's first entry (default: --start)")
    p.add_argument("--camera", default=DEFAULT_CALIBRATION)
    return p


def _cli(argv=None):
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
    spans = full_spans(a.start, a.end, a.test_size)
    track = dict(prepare.track_arguments(p, a), gt_path=None)          # (--gt is only compared with here: it never fixes the scale)
    if a.heatmaps is not None:
        rec = prepare.prepare_spans(a.slam, a.heatmaps, a.depths, spans=spans, fps=a.fps, mat_start_frame=a.start, camera_model_path=a.camera,
                                    **track, **prepare.depth_route_arguments(a))
    else:
        rec = detections.recording_from_detections(a.slam, detections.detections_from_args(a), spans=spans, fps=a.fps, camera_model_path=a.camera,
                                                   **track, **prepare.depth_route_arguments(a, maps=False))
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
    if a.scale == "drift":
        print("\n".join(est.knot_lines()))
    write_json(a.json, out)
    return est


if __name__ == "__main__":
    _cli()
