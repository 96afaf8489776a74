"""A recording optimised as ONE continuous motion: every frame, one world.

The chunked routes (`whole_sequence`) follow the reference's evaluation protocol: 100-frame chunks, each in its own frame, the last two
frames of a chunk never optimised, the smoothing reflected at every chunk edge, one floor and one set of files per chunk.  A recording
without ground truth has one world already (`Recording.origins`); this module optimises it in that world.  The windows are
`sequence.cover_starts`' -- every `stride` frames, the last one anchored to the recording's end, so that every frame lies in a window
-- they all read ONE frame buffer, `WindowEngine.merge_cover` averages them wherever they overlap, however they are spaced, and the
result is one sequence: one report, one BVH / glTF / clip, one floor, stances that cross the former chunk boundaries.  The merge also
tells how far the windows that cover a frame disagree about it (`window_disagreement`), the only per-frame signal of trouble a
recording without ground truth has.

    python -m globalegomocap_amd.continuous --slam traj.txt --heatmaps DIR --depth_from bones --scale auto --bridge \\
        --start 551 --end 3300 --bvh out --gltf out --upright true --foot_lock true

    python -m globalegomocap_amd.continuous --slam traj.txt --keypoints det.npz --depth_from bones --scale auto --start 0 --end 2000 --save_pose out
"""
import os
import pickle

import numpy as np
import torch

from .report import ChunkReport, _quality_rows, _result_dict, result_pose_dict, sequence_result
from .optimizer import SequenceOptimizer
from .sequence import OVERLAP, cover_starts
from .whole_sequence import KEYS, _K_GT, _settings


def _device_f64(x, device):
    return torch.as_tensor(x).to(device=device, dtype=torch.float64).contiguous()


def optimize_continuous(recording, camera_model_path, *args, stride=8, **kwargs):
    """`recording` (a `prepare.Recording` without ground truth of chunks that follow one another, or any Recording of one chunk) as one
    motion.  The arguments behind `camera_model_path` are `whole_sequence.optimize_recording`'s and mean what they mean there;
    `chunks_per_batch`, `per_sequence`, an `overlap` other than the default and device_metrics=False belong to the chunked route and are
    a ValueError.  stride (by keyword): frames between two windows, 1 .. 8; below 8 more windows cover every frame.

    -> (summary, [report], estimated_pose, optimized_pose, gt_pose or None) as `optimize_recording` returns them, the poses [N,15,3]
    for ALL N frames of the recording, in the recording's frame.  The report is the seven entries of QUALITY_KEYS (ground_truth=False) or
    the 18 errors, with two more: `windows_per_frame` (fewest, most windows over a frame) and `window_disagreement` = {"mean", "max",
    "frame"}: per frame the largest distance, in metres, between a covering window's joint and the merged joint (before the final
    smoothing), its mean and maximum over the frames and the frame of the maximum.  With `save_pose`, result_pose.pkl holds the
    per-frame array as `window_disagreement`.  The files of every output option are written ONCE, under
    `recording_0/data_start_A_end_B`: with `upright` one floor for the whole recording, with `foot_lock` stances of any length.

    The noise is ONE torch.randn(2 * B, D) from the global generator for the B windows, laid out [B, 2, D] (what `SequenceOptimizer.fire`
    draws); a recording of more windows than the optimiser's `max_windows` runs in consecutive calls over the same frame buffers, each
    with its slice of that block: the results do not depend on how the windows are split."""
    cfg = _settings(camera_model_path, *args, **kwargs)
    for name, refused in (("chunks_per_batch", cfg.chunks_per_batch is not None), ("per_sequence", bool(cfg.per_sequence)),
                          ("overlap", cfg.overlap != OVERLAP), ("device_metrics=False", not cfg.device_metrics)):
        if refused:
            raise ValueError("optimize_continuous: %s belongs to the chunked route (one recording is one sequence here; stride= spaces the windows)" % name)
    rec = recording.continuous()
    if not len(rec):
        raise FileNotFoundError("a recording without chunks")
    c = rec.chunks[0]
    if cfg.ground_truth and c.gt is None:
        raise KeyError(KEYS[_K_GT])          # (what the chunked route raises)
    name = os.path.join("recording_0", c.name)
    if cfg.verbose:
        print("running data: {}".format(name))
    device = torch.device("cuda", torch.cuda.current_device())
    host = lambda t: np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64)      # noqa: E731
    est_local, cams = host(c.est_local), host(c.cams)
    N = len(est_local)
    starts = cover_starts(N, cfg.seq_len, stride)
    B = len(starts)
    opt = cfg.optimizer or SequenceOptimizer(cfg.camera_model_path, cfg.global_vae_path, cfg.local_vae_path, max_windows=B, seq_len=cfg.seq_len)
    e = opt.engine
    heat_d = torch.as_tensor(c.heat).to(device=device, dtype=torch.float32).contiguous()
    # one skeleton for the whole recording: the mean bone lengths are those of all its frames
    prep = opt.prepare(est_local, cams, starts, np.zeros(B, dtype=np.int64), [(0, N)], timings=cfg.timings)
    w_local, w_global = opt.stage_weights(cfg.vae_weight, cfg.smoothness_weight, cfg.bone_length_weight, cfg.weight_3d, cfg.reproj_weight)
    eps = torch.randn(2 * B, e.D).reshape(B, 2, e.D)
    per_call = max(1, min(B, e.max_windows))
    mids, globs = [], []
    for lo in range(0, B, per_call):
        hi = min(B, lo + per_call)
        part = dict(prep, mean_bone=prep["mean_bone"][lo:hi].contiguous(), frame0=prep["frame0"][lo:hi].contiguous(), B=hi - lo)
        mid, glob, _ = opt.collect(opt.fire(part, heat_d, w_local, w_global, eps=eps[lo:hi], timings=cfg.timings), keep_device=True)
        several = B > per_call          # (with graphs on, the next call writes the same output buffers)
        mids.append(mid.clone() if several else mid)
        globs.append(glob.clone() if several else glob)
    mid_local, opt_global = (torch.cat(x) if len(x) > 1 else x[0] for x in (mids, globs))
    smooth = bool(cfg.final_smooth)
    merged, smoothed, count, spread = e.merge_cover(opt_global, starts, smooth=smooth, want_spread=True)
    opt_d = smoothed if smooth else merged
    est_d = _device_f64(c.est_global, device)
    gt_d = _device_f64(c.gt, device) if cfg.ground_truth else None
    mid_d = None
    if cfg.ground_truth or cfg.save_pose is not None:
        # stage one's sequence: every window's local poses through their frames' cameras, merged like the optimised ones
        idx = torch.from_numpy(starts.astype(np.int64)[:, None] + np.arange(cfg.seq_len)[None]).to(device)
        M = prep["cams"][idx]                                                                # [B,T,4,4]
        mid_g = torch.matmul(mid_local.to(torch.float64), M[..., :3, :3].transpose(-1, -2)) + M[..., None, :3, 3]
        mid_d = e.merge_cover(mid_g, starts)[0]
    raw = None
    if cfg.ground_truth:
        result = e.calculate_errors(est_d, mid_d, opt_d, gt_d)
    else:
        frames = (prep["cams"], heat_d, torch.zeros(1, dtype=torch.int64, device=device), prep["mean_bone_chunks"].contiguous())
        raw = _quality_rows(e, est_d, opt_d, frames, 1).cpu().numpy()[0]
        result = _result_dict(e, raw, False)
    count_np, spread_np = count.cpu().numpy(), spread.cpu().numpy()
    report = ChunkReport(result=result, est=est_d.cpu().numpy(), opt=opt_d.cpu().numpy(), gt=None if gt_d is None else gt_d.cpu().numpy(),
                         mid=None if mid_d is None else mid_d.cpu().numpy(), raw=raw, views=(est_d, opt_d, gt_d))
    out = sequence_result([report], None, cfg.verbose)
    worst = int(np.argmax(spread_np))
    extra = {"windows_per_frame": (int(count_np.min()), int(count_np.max())),
             "window_disagreement": {"mean": float(spread_np.mean()), "max": float(spread_np[worst]), "frame": worst}}
    if cfg.verbose:
        print("{}: {} windows at stride {} over {} frames, {} to {} per frame; they disagree by {:.4f} m on average, at most {:.4f} m (frame {})".format(
            name, B, int(stride), N, *extra["windows_per_frame"], extra["window_disagreement"]["mean"], extra["window_disagreement"]["max"], worst))
    # the files, as the chunked route's `finish` writes a chunk's: once, for the whole recording
    lock = cfg.outputs.lock(e, opt_d)          # (--foot_lock: None without it)
    found = cfg.outputs.write(e, os.path.normpath(name), report.sequences(), prep["cams"], heat_d, 0, **({} if lock is None else {"locked": lock}))
    if lock is not None:
        extra["foot_lock"] = lock.as_dict()
        if cfg.verbose:
            print("{}: {}".format(name, lock.line()))
    if found is not None:
        extra["ground"] = found.as_dict()
        if cfg.verbose:
            print("{}: {}".format(name, found.line()))
    report.drop_views()
    for d in (result, out[0]):
        d.update(extra)
    if cfg.save_pose is not None:
        pose_dir = os.path.join(cfg.save_pose, c.name)
        os.makedirs(pose_dir, exist_ok=True)
        poses = result_pose_dict(report.est, report.opt, report.mid, report.gt, smooth, **({} if lock is None else {"locked": lock.sequence.cpu().numpy()}))
        poses["window_disagreement"] = spread_np
        with open(os.path.join(pose_dir, "result_pose.pkl"), "wb") as f:
            pickle.dump(poses, f)
    return out


# ------------------------------------------------------------------------------------------------------------------ the command line
def _stride_arg(text):
    import argparse
    k = int(text)
    if not 1 <= k <= 8:
        raise argparse.ArgumentTypeError("a whole number 1 .. 8")
    return k


def _parser():
    import argparse
    from . import prepare, whole_sequence as ws
    p = argparse.ArgumentParser(description="recording -> ONE optimised motion: every frame, one world, one set of files")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--heatmaps", default=None, metavar="DIR", help="directory of per-frame heatmap .mat files (`prepare`'s route)")
    src.add_argument("--keypoints", default=None, metavar="FILE", help=".npy [N,15,2|3] or .npz with keypoints[, depth, frame_ids] (`detections`' route)")
    prepare.add_depth_route_options(p)
    p.add_argument("--depth", default=None, metavar="FILE.npy", help="with --keypoints: the joints' depths [N,15], row for row with the detections")
    p.add_argument("--sigma", type=float, default=None, help="with --keypoints: the splatted Gaussians' width in heat-map pixels (default 1.5)")
    p.add_argument("--first_id", type=int, default=None, help="with --keypoints: frame id of the detections' first row (default 0)")
    prepare.add_track_options(p, gt_help="ground-truth pickle: ONE scale is fitted over the whole span, and the 18 errors are reported")
    p.add_argument("--stride", type=_stride_arg, default=8, metavar="K", help="frames between two windows, 1 .. 8 (default 8)")
    ws.add_weight_options(p)
    ws.add_output_options(p)
    p.add_argument("--final_smooth", default=True, type=ws._truthy)
    p.add_argument("--save_pose", default=None, metavar="DIR", help="write DIR/data_start_A_end_B/result_pose.pkl")
    return p


def parse_args(argv=None):
    """The command line's arguments, checked."""
    from . import prepare, whole_sequence as ws
    p = _parser()
    a = p.parse_args(argv)
    if a.bridge is not None and a.gt is not None:
        p.error("--bridge needs --scale: with --gt there is no common world to bridge in")
    if a.end - a.start < 10:
        p.error("--start / --end: a recording has at least the 10 frames of one window")
    if a.heatmaps is not None:
        if a.depth is not None or a.sigma is not None or a.first_id is not None:
            p.error("--depth, --sigma and --first_id belong to --keypoints")
        prepare.check_depth_route_options(p, a)
    else:
        if a.min_peak is not None or a.peaks is not None:
            p.error("--min_peak and --peaks belong to --heatmaps")
        if sum(x is not None for x in (a.depths, a.depth, a.depth_from)) > 1:
            p.error("give at most one of --depths DIR, --depth FILE.npy and --depth_from bones")
        if a.depth_from is None and (a.bones is not None or a.neck_depth is not None):
            p.error("--bones and --neck_depth belong to --depth_from bones")
    ws.check_output_options(p, a)
    a.track = prepare.track_arguments(p, a)          # (the rules of --scale drift are checked here)
    a.drift = {k: a.track[k] for k in ("knot", "stiffness")}
    return a


def _cli(argv=None):
    from . import detections, prepare, whole_sequence as ws
    a = parse_args(argv)
    if a.heatmaps is not None:
        rec = prepare.prepare_continuous(a.slam, a.heatmaps, a.depths, total_start_frame=a.start, total_end_frame=a.end, fps=a.fps,
                                         mat_start_frame=a.mat_start, camera_model_path=a.camera, **a.track, **prepare.depth_route_arguments(a))
    else:
        a.first_id = 0 if a.first_id is None else a.first_id
        rec = detections.continuous_from_detections(a.slam, detections.detections_from_args(a), start_frame=a.start, end_frame=a.end, fps=a.fps,
                                                    sigma=1.5 if a.sigma is None else a.sigma, camera_model_path=a.camera, gt_start_frame=a.mat_start,
                                                    **a.track, **prepare.depth_route_arguments(a, maps=False))
        prepare.print_report(rec)
    optimize_continuous(rec, a.camera, a.vae, a.gmm, a.smooth, a.bone_length, a.weight_3d, a.reproj_weight, final_smooth=a.final_smooth,
                        ground_truth=a.scale is None, save_pose=a.save_pose, stride=a.stride, **ws.output_arguments(a))


if __name__ == "__main__":
    _cli()
