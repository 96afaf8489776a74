"""Recordings given as 2-D joint detections instead of heat-maps.

Many 2-D pose estimators hand back one `(u, v, confidence)` per joint and no map: regression heads, soft-argmax heads, a keypoint
detector run on the fisheye image.  A detection is 360 bytes per frame where the heat-maps are 245 KB, so here the detections of a
whole recording go up in one copy and everything the optimiser reads is made on the device: `gem_lift_keypoints` un-projects the
sub-pixel detections (the reference's `camera2world`), `gem_fill_missing` interpolates joints the detector lost, and
`gem_keypoint_heatmaps` splats the maps the reprojection term samples.  The result is the `prepare.Recording` that
`prepare.prepare_spans` builds from .mat files: `whole_sequence.optimize_recording` and `Recording.write_chunks` take it unchanged.

u, v are pixels of the fisheye image the calibration describes (1280 x 1024).  A detection is usable when its confidence is > 0
and u, v are finite; a joint that is unusable in a frame gets a blank heat-map there and the pose interpolated in time from its
usable neighbours inside the chunk.  A joint with no usable detection in a whole chunk is a ValueError.

    python -m globalegomocap_amd.detections --slam traj.txt --keypoints det.npz --scale 1.0|auto|drift --start 0 --end 2001 --fps 25 \\
        [--depths DIR | --depth FILE.npy | --depth_from bones [--bones FILE.npy] [--neck_depth M]] [--sigma 1.5] [--first_id 0] [--test_size 100] [--out DIR] [--optimize] [--camera JSON]
"""
import os

import numpy as np

from .skeleton import N_JOINTS


# ------------------------------------------------------------------------------------------------------------------ host-side logic
def _keypoint_array(kp, what):
    kp = np.asarray(kp)
    if kp.dtype == object or not (np.issubdtype(kp.dtype, np.floating) or np.issubdtype(kp.dtype, np.integer)):
        raise ValueError("%s: the detections must be a numeric array, got dtype %s" % (what, kp.dtype))
    if kp.ndim != 3 or kp.shape[1] != N_JOINTS or kp.shape[2] not in (2, 3):
        raise ValueError("%s: the detections must be [N,%d,2] or [N,%d,3] (u, v[, confidence]), got %s" % (what, N_JOINTS, N_JOINTS, kp.shape))
    kp = kp.astype(np.float64)
    if kp.shape[2] == 2:
        kp = np.concatenate([kp, np.ones(kp.shape[:2] + (1,))], axis=2)
    return np.ascontiguousarray(kp)


def _depth_array(depth, n, what):
    depth = np.asarray(depth)
    if depth.dtype == object or not (np.issubdtype(depth.dtype, np.floating) or np.issubdtype(depth.dtype, np.integer)):
        raise ValueError("%s: depth must be a numeric array, got dtype %s" % (what, depth.dtype))
    if depth.shape != (n, N_JOINTS):
        raise ValueError("%s: depth must be [%d,%d] for these detections, got %s" % (what, n, N_JOINTS, depth.shape))
    return np.ascontiguousarray(depth, dtype=np.float64)


def _frame_id_array(ids, n, what):
    ids = np.asarray(ids)
    if ids.shape != (n,) or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError("%s: frame_ids must be %d integers, got %s %s" % (what, n, ids.dtype, ids.shape))
    ids = ids.astype(np.int64)
    u, c = np.unique(ids, return_counts=True)
    if (c > 1).any():
        raise ValueError("%s: frame ids %s appear more than once" % (what, u[c > 1].tolist()))
    return ids


def as_detections(kp, depth=None, frame_ids=None, first_id=0, what="detections"):
    """-> {"keypoints": [N,15,3] f64 (a missing third column: every confidence 1), "depth": [N,15] f64 or None, "frame_ids": [N]
    int64 (default: first_id + row)}.  ValueError for anything else."""
    kp = _keypoint_array(kp, what)
    n = len(kp)
    return {"keypoints": kp, "depth": None if depth is None else _depth_array(depth, n, what),
            "frame_ids": np.arange(n, dtype=np.int64) + int(first_id) if frame_ids is None else _frame_id_array(frame_ids, n, what)}


def read_detections(path, first_id=0):
    """A `.npy` of [N,15,2|3], or an `.npz` with `keypoints` [N,15,2|3], optionally `depth` [N,15] and `frame_ids` [N]; loaded with
    allow_pickle=False (an object array is a ValueError).  -> `as_detections`' dict."""
    what = str(path)
    loaded = np.load(path, allow_pickle=False)
    if isinstance(loaded, np.ndarray):
        return as_detections(loaded, first_id=first_id, what=what)
    with loaded as f:
        if "keypoints" not in f.files:
            raise ValueError("%s: no array `keypoints` (it holds %s)" % (what, sorted(f.files)))
        return as_detections(f["keypoints"], f["depth"] if "depth" in f.files else None, f["frame_ids"] if "frame_ids" in f.files else None,
                             first_id, what=what)


def span_rows(frame_ids, spans):
    """The row of every frame id of every [a, b) of `spans`, in order: [int64 array per span].  ValueError naming the frame ids the
    detections have no row for (a gap inside a span)."""
    row_of = {int(i): r for r, i in enumerate(np.asarray(frame_ids, dtype=np.int64))}
    out = []
    for a, b in spans:
        missing = [i for i in range(a, b) if i not in row_of]
        if missing:
            raise ValueError("the detections have no row for frame ids %s of [%d, %d)" % (missing, a, b))
        out.append(np.array([row_of[i] for i in range(a, b)], dtype=np.int64))
    return out


def usable(kp):
    """[...,3] detections -> bool [...]: confidence > 0 (NaN is not) and u, v finite -- the device's rule."""
    kp = np.asarray(kp, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (kp[..., 2] > 0) & np.isfinite(kp[..., 0]) & np.isfinite(kp[..., 1])


def check_chunks_have_every_joint(kp, bounds, spans):
    """ValueError when a joint has no usable detection in a whole chunk (rows bounds[k] = (lo, hi) of `kp`): nothing to interpolate from."""
    ok = usable(kp)
    for (lo, hi), (a, b) in zip(bounds, spans):
        lost = np.nonzero(~ok[lo:hi].any(axis=0))[0]
        if len(lost):
            raise ValueError("joints %s have no usable detection in the chunk [%d, %d): nothing to interpolate them from" % (lost.tolist(), a, b))


def depths_from_mat_dir(directory, frame_ids):
    """The depth .mat directory of the pose network (`prepare`'s --depths): frame id i is entry i of the naturally sorted LISTING, as
    there; `loadmat(...)['depth'][0]` of each.  -> [N,15] f64."""
    from .prepare import DEPTH_NAME, read_mat_array
    from .staging import natural_key
    names = sorted(os.listdir(directory), key=natural_key)
    bad = [int(i) for i in frame_ids if not 0 <= i < len(names)]
    if bad:
        raise ValueError("%s holds %d files: no entry for frame ids %s" % (directory, len(names), bad))
    return np.stack([np.asarray(read_mat_array(os.path.join(directory, names[int(i)]), DEPTH_NAME)[0], dtype=np.float64)[0] for i in frame_ids])


def detections_from_args(a):
    """The detections dict of a command line's parsed `--keypoints`, `--first_id` and `--depth` or `--depths`."""
    det = read_detections(a.keypoints, a.first_id)
    if a.depth is not None:
        det["depth"] = _depth_array(np.load(a.depth, allow_pickle=False), len(det["keypoints"]), a.depth)
    elif a.depths is not None:
        det["depth"] = depths_from_mat_dir(a.depths, det["frame_ids"])
    return det


# ------------------------------------------------------------------------------------------------------------------ the device path
def recording_from_detections(slam_result_path, detections, gt_path=None, scale=None, spans=(), fps=25, depth=None, sigma=1.5, first_id=0,
                              camera_model_path=None, device=None, gt_start_frame=None, lag=None, tau=0.10, min_pairs=50, bridge=None,
                              bones=None, neck_depth=None, knot=None, stiffness=1.0):
    """Every (start_frame, end_frame) of `spans` as one chunk of a `prepare.Recording`, from 2-D detections: `detections` is a file
    (`read_detections`), an array [N,15,2|3] or `as_detections`' dict; `depth` [N,15] unless the file carries it, or "bones": the
    depths are solved on the device from the bone lengths (`WindowEngine.bone_depths` with `bone_depth.options(bones,
    neck_depth=neck_depth)`), a joint the solve could not reach is a lost detection from there on, and the
    Recording carries the solve's `depth_report`.  Exactly one of
    `gt_path` (the ground truth fixes the SLAM scale per chunk, as `prepare` does; entry i - gt_start_frame of the pickle is frame id
    i, gt_start_frame defaulting to the first span's start) and `scale`: a number, or "auto" to estimate it from the foot contacts of
    the filled poses (`slam_scale.estimate_scale` with `lag`, `tau`, `min_pairs`), or "drift" to follow a scale that creeps
    over the recording (`knot` frames between the curve's knots, `stiffness`).  One upload, then on the device:
    lift -> fill -> heat-maps -> cameras -> gem_prepare_global; from the filled poses on this is `prepare.RecordingStage`.  `bridge`:
    None, or the seconds of lost SLAM tracking whose cameras are invented (`slam_bridge`), without ground truth
    only."""
    from . import prepare
    stage = prepare.RecordingStage(prepare.CameraRoute(gt_path, scale, bridge, lag, tau, min_pairs, knot, stiffness), spans, fps)
    import torch
    from .camera import DEFAULT_CALIBRATION
    if isinstance(detections, (str, os.PathLike)):
        det = read_detections(detections, first_id)
    elif isinstance(detections, dict):
        det = as_detections(detections["keypoints"], detections.get("depth"), detections.get("frame_ids"), first_id)
    else:
        det = as_detections(detections, first_id=first_id)
    from_bones = isinstance(depth, str)
    if from_bones:
        from . import bone_depth
        if depth != "bones":
            raise ValueError('recording_from_detections: depth is an array [N,%d] or "bones", got %r' % (N_JOINTS, depth))
        bone_opts = bone_depth.options(bones, neck_depth=neck_depth)
    elif bones is not None or neck_depth is not None:
        raise ValueError('recording_from_detections: bones= and neck_depth= belong to depth="bones"')
    elif depth is not None:
        det["depth"] = _depth_array(depth, len(det["keypoints"]), "recording_from_detections")
    if det["depth"] is None and not from_bones:
        raise ValueError("recording_from_detections: the joints' depths are needed (depth=, or `depth` in the .npz)")
    spans = stage.spans
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    stage.read_trajectory(slam_result_path)
    stage.check_trajectory()
    rows = span_rows(det["frame_ids"], spans)
    if not spans:
        return stage.empty()
    bounds = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    stage.bounds = bounds = [(int(lo), int(hi)) for lo, hi in zip(bounds[:-1], bounds[1:])]
    pick = np.concatenate(rows)
    kp = det["keypoints"][pick]
    if from_bones:          # (what the solve will report unsolved counts as lost)
        kp = np.concatenate([kp[..., :2], np.where(bone_depth.solved_mask(kp), kp[..., 2], 0.0)[..., None]], axis=2)
    check_chunks_have_every_joint(kp, bounds, spans)
    pose_gt = stage.read_gt()
    if pose_gt is not None:
        g0 = spans[0][0] if gt_start_frame is None else int(gt_start_frame)
        stage.gts = [prepare.gt_clip(pose_gt, a, b, g0) for a, b in spans]
    # [n,15,4]: ONE copy carries detections and depths; with depth="bones" the detections alone go up
    packed = np.ascontiguousarray(kp) if from_bones else np.concatenate([kp, det["depth"][pick][..., None]], axis=2)
    depth_report = None
    with torch.cuda.device(device):
        engine = prepare._lift_engine(camera_model_path or DEFAULT_CALIBRATION, device.index)
        packed_d = torch.from_numpy(packed).to(device)
        if from_bones:
            kp_d = packed_d
            depth_d, _, depth_report = prepare.solve_bone_depths(engine, kp_d, bone_opts)
        else:
            kp_d, depth_d = packed_d[..., :3].contiguous(), packed_d[..., 3].contiguous()
        est_local, _, valid = engine.lift_keypoints(kp_d, depth_d)
        prepare.fill_chunks(engine, est_local, valid, bounds)
        stage.fix_scale(engine, est_local)          # (a recording that does not fix the scale is refused before the heat-maps are made)
        heat = engine.keypoint_heatmaps(kp_d, sigma)          # (enqueued ahead of the host's camera work and its blocking upload)
        rec = stage.recording(est_local, heat)
        rec.depth_report = depth_report
        return rec


def continuous_from_detections(slam_result_path, detections, gt_path=None, scale=None, start_frame=0, end_frame=0, fps=25, **options):
    """`recording_from_detections` for a recording that is optimised as one motion (`continuous.optimize_continuous`, DESIGN.md section
    6s): the ONE span [start_frame, end_frame) as one chunk; `options`: its other keywords, handed on as they are.  -> a Recording that
    is continuous already."""
    return recording_from_detections(slam_result_path, detections, gt_path, scale, [(int(start_frame), int(end_frame))], fps, **options)


def _parser():
    import argparse
    from . import prepare
    p = argparse.ArgumentParser(description="recording (2-D joint detections) -> chunks for the optimiser")
    p.add_argument("--keypoints", required=True, metavar="FILE", help=".npy [N,15,2|3] or .npz with keypoints[, depth, frame_ids]: u, v in "
                                                                       "pixels of the fisheye image[, confidence]")
    dep = p.add_mutually_exclusive_group()
    dep.add_argument("--depths", default=None, metavar="DIR", help="directory of per-frame depth .mat files")
    dep.add_argument("--depth", default=None, metavar="FILE.npy", help="the joints' depths [N,15], row for row with the detections")
    dep.add_argument("--depth_from", default=None, choices=("bones",), help="bones: no depths at all -- they are solved from the bone "
                                                                           "lengths (DESIGN.md section 6q)")
    from .bone_depth import add_bone_depth_options
    add_bone_depth_options(p)
    p.add_argument("--sigma", type=float, default=1.5, help="the splatted Gaussians' width in heat-map pixels")
    p.add_argument("--first_id", type=int, default=0, help="frame id of the detections' first row (without frame_ids)")
    prepare.add_recording_options(p)
    return p


def _cli(argv=None):
    from . import prepare
    p = _parser()
    a = prepare.parse_recording_options(p, argv)
    if a.depth_from is None and (a.bones is not None or a.neck_depth is not None):
        p.error("--bones and --neck_depth belong to --depth_from bones")
    rec = recording_from_detections(a.slam, detections_from_args(a), spans=prepare.chunk_spans(a.start, a.end, a.test_size), fps=a.fps, sigma=a.sigma,
                                    camera_model_path=a.camera, gt_start_frame=a.mat_start, **prepare.track_arguments(p, a),
                                    **prepare.depth_route_arguments(a, maps=False))
    prepare.print_report(rec)
    if a.out is not None:
        rec.write_chunks(a.out)
    if a.optimize:
        from .whole_sequence import optimize_recording
        optimize_recording(rec, a.camera, ground_truth=a.scale is None)


if __name__ == "__main__":
    _cli()
