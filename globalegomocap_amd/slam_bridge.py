"""Bridging the frames on which SLAM lost tracking (`--bridge MAX_GAP_SECONDS` of `prepare` and `detections`).

OpenVSLAM / ORB-SLAM write no trajectory line for a frame on which tracking was lost.  Without this option such a span is refused
(`prepare.check_trajectory`); with it, on the route without ground truth, the missing cameras are invented kinematically and marked:
the rotation by slerp between the two tracked neighbours, the translation by the minimum-acceleration curve through the tracked
neighbours (`gem_slam_bridge`, specified by tests/bridge_twin.py).  The poses are not looked at.  What was invented is recorded:
`Recording.bridged` marks the frames, `Recording.bridge_report` holds the counts and the largest bridged distances.

    python -m globalegomocap_amd.slam_bridge --slam traj.txt --start A --end B --fps 25 [--max_gap S] [--json FILE]

prints the gaps of a trajectory without touching a device.
"""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._binding import _ptr, staged_call

MAX_GAP = _capi.BRIDGE_MAX_GAP
DEFAULT_MAX_GAP_SECONDS = 1.0


def gap_seconds(value):
    """The longest gap to bridge as a float; ValueError unless it is a positive finite number."""
    seconds = float(value)
    if not (math.isfinite(seconds) and seconds > 0):
        raise ValueError("bridge: the longest gap to bridge must be a positive number of seconds, got %r" % (value,))
    return seconds


def max_gap_frames(seconds, fps):
    """floor(seconds * fps + 0.5); ValueError unless seconds is a positive finite number."""
    return int(math.floor(gap_seconds(float(seconds)) * float(fps) + 0.5))


def bridge_arg(bridge, gt_path=None):
    """The `bridge=` argument of the preparing functions -> None (off) or seconds.  True stands for the default of 1 s.  ValueError with
    `gt_path`: the per-chunk Umeyama scale leaves no common world to bridge in."""
    if bridge is None or bridge is False:
        return None
    if gt_path is not None:
        raise ValueError("bridge applies to a recording without ground truth (scale=): with gt_path every chunk has its own Umeyama scale "
                         "and there is no common world to bridge in")
    return DEFAULT_MAX_GAP_SECONDS if bridge is True else gap_seconds(bridge)


def tracked_mask(frame_ids, start_frame, end_frame):
    """[end - start] bool: whether the trajectory has a line for the frame id.  ValueError for an id that appears twice."""
    ids = np.asarray(frame_ids, dtype=np.int64)
    ids = ids[(ids >= start_frame) & (ids < end_frame)]
    u, c = np.unique(ids, return_counts=True)
    if (c > 1).any():
        raise ValueError("the trajectory has several lines for frame ids %s" % u[c > 1].tolist())
    mask = np.zeros(max(int(end_frame) - int(start_frame), 0), dtype=bool)
    mask[u - int(start_frame)] = True
    return mask


def gap_list(mask):
    """[(index of the first lost frame, lost frames)] of the maximal runs of False in `mask`."""
    m = np.asarray(mask, dtype=bool)
    edge = np.diff(np.concatenate([[1], m.astype(np.int8), [1]]))
    first, behind = np.flatnonzero(edge == -1), np.flatnonzero(edge == 1)
    return [(int(a), int(b - a)) for a, b in zip(first, behind)]


def find_gaps(frame_ids, start_frame, end_frame, max_gap_frames):
    """The systems of the span [start_frame, end_frame) of a trajectory whose lines have `frame_ids`: [(frame id of the first lost
    frame, frames up to and including the last lost one)], gaps separated by fewer than two tracked frames being one system.  ValueError
    for an id that appears twice, a first or last id that is not tracked (naming the first and last tracked id), gaps longer than
    min(max_gap_frames, 64) (naming each with its ids) and a system of more than 64 lost frames."""
    A, B = int(start_frame), int(end_frame)
    if B <= A:
        raise ValueError("an empty span [%d, %d)" % (A, B))
    mask = tracked_mask(frame_ids, A, B)
    if not mask.any():
        raise ValueError("the trajectory has no line for any frame id of [%d, %d)" % (A, B))
    if not (mask[0] and mask[-1]):
        where = np.flatnonzero(mask)
        raise ValueError("the first and the last frame id of [%d, %d) must be tracked for the bridge: the first tracked id is %d, the last %d "
                         "(re-run with --start %d --end %d)" % (A, B, A + where[0], A + where[-1], A + where[0], A + where[-1] + 1))
    gaps = gap_list(mask)
    most = min(int(max_gap_frames), MAX_GAP)
    long = [(a, m) for a, m in gaps if m > most]
    if long:
        raise ValueError("gaps too long to bridge (at most %d lost frames; the hard cap is %d): %s"
                         % (most, MAX_GAP, ", ".join("ids [%d, %d): %d frames" % (A + a, A + a + m, m) for a, m in long)))
    systems = []
    for a, m in gaps:
        if systems and a - (systems[-1][0] + systems[-1][1]) < 2:
            systems[-1] = (systems[-1][0], a + m - systems[-1][0])
        else:
            systems.append((a, m))
    for a, length in systems:
        unknowns = int((~mask[a:a + length]).sum())
        if unknowns > MAX_GAP:
            raise ValueError("ids [%d, %d) hold %d lost frames in gaps less than two tracked frames apart: one system of more than %d unknowns"
                             % (A + a, A + a + length, unknowns, MAX_GAP))
    return [(A + a, length) for a, length in systems]


def tracked_rows(rows, start_frame, end_frame, fps):
    """The trajectory rows (`slam.trajectory_rows`) of the tracked frame ids of [start_frame, end_frame), in id order, and their ids."""
    from . import slam
    ids = slam.frame_ids(rows, fps)
    keep = np.flatnonzero((ids >= start_frame) & (ids < end_frame))
    keep = keep[np.argsort(ids[keep], kind="stable")]
    return rows[keep], ids[keep]


def relative_rows(rows, start_frame, end_frame, fps, scale):
    """-> (poses [n,7], mask [n]): the tracked frames' poses relative to frame `start_frame`, translation times `scale`, as
    `slam.scaled_trajectory` makes them (t xyz, q xyzw); rows of lost frames are zero."""
    from . import slam
    picked, ids = tracked_rows(rows, start_frame, end_frame, fps)
    mask = tracked_mask(ids, start_frame, end_frame)
    if not mask[0]:
        raise ValueError("frame id %d, the span's first, is not tracked" % start_frame)
    rt, rq = slam.relative_poses(picked[:, 1:4], picked[:, 4:8])
    poses = np.zeros((len(mask), 7))
    poses[mask] = np.concatenate([rt * float(scale), rq], axis=1)
    return poses, mask


class BridgeReport:
    """What `gem_slam_bridge` invented: `frames`, `lost`, `gaps`, `systems`, `longest_gap` (frames), `offset_max` (the largest distance
    of a bridged camera from the straight line between its gap's neighbours, metres), `angle_max` (the largest rotation bridged across
    one gap, radians) and `translation_max` (the largest distance bridged across one gap, metres); `gap_ids` [(first lost id, lost
    frames)], `bridged` [frames] bool, the call's `fps` and `max_gap` (seconds)."""

    def __init__(self, record, bridged, gap_ids, fps, max_gap):
        r = np.asarray(record, dtype=np.float64)
        head = _capi.GemBridgeRecord.from_buffer_copy(r[:_capi.BRIDGE_RECORD_DOUBLES].tobytes())
        self.status = int(head.status)
        self.frames, self.lost, self.gaps, self.systems, self.longest_gap = (int(head.frames), int(head.lost), int(head.gaps), int(head.systems),
                                                                             int(head.longest_gap))
        self.offset_max, self.angle_max, self.translation_max = head.offset_max, head.angle_max, head.translation_max
        self.bridged = np.asarray(bridged, dtype=bool)
        self.gap_ids = [(int(a), int(m)) for a, m in gap_ids]
        self.fps, self.max_gap = float(fps), float(max_gap)
        self.record = r

    def as_dict(self):
        """Plain numbers and lists (JSON)."""
        return {"frames": self.frames, "lost": self.lost, "gaps": self.gaps, "systems": self.systems, "longest_gap": self.longest_gap,
                "offset_max": self.offset_max, "angle_max": self.angle_max, "translation_max": self.translation_max,
                "gap_ids": [list(g) for g in self.gap_ids], "fps": self.fps, "max_gap": self.max_gap}

    def line(self):
        return ("SLAM bridge: %d of %d frames invented in %d gaps (%d systems, longest %d frames = %.2f s); largest bridged rotation %.2f "
                "degrees, distance %.3f m, offset from the straight line %.3f m"
                % (self.lost, self.frames, self.gaps, self.systems, self.longest_gap, self.longest_gap / self.fps, math.degrees(self.angle_max),
                   self.translation_max, self.offset_max))


def bridge_call(device, poses, mask, systems, chunk_starts, stream=None, outputs=None, check=True):
    """gem_slam_bridge.  poses [n,7] float64 and mask [n] (host), systems [(first frame index, length)], chunk_starts [n_chunks]
    (indices).  `outputs`: None, or (G [n,4,4], cams [n,4,4], origins [n_chunks,4,4] float64, bridged [n] uint8, record [16] float64)
    device tensors to write into.  -> (G, cams, origins, bridged, record) on the device; with check=False (return code, message) come
    in front and nothing is raised."""
    import torch
    lib = _capi.load_library()
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    mask8 = np.ascontiguousarray(np.asarray(mask, dtype=bool).astype(np.uint8))
    n = len(mask8)
    if poses.shape != (n, 7):
        raise ValueError("bridge_call: %d frames in the mask, poses %s" % (n, poses.shape))
    sys32 = np.ascontiguousarray(np.asarray(systems, dtype=np.int32).reshape(-1, 2))
    starts32 = np.ascontiguousarray(chunk_starts, dtype=np.int32)
    ns, nc = len(sys32), len(starts32)
    need = int(lib.gem_slam_bridge_work(max(n, 1)))
    if need < 0:          # (n out of range: gem_slam_bridge itself refuses it, with its own text)
        need = 8
    device = torch.device(device)
    with staged_call(lib, device, stream) as call:
        d_poses, d_sys, d_starts, d_mask = call.upload(poses, sys32, starts32, mask8)          # (ONE upload, the 8-byte items first)
        if outputs is None:
            outputs = (torch.empty((n, 4, 4), dtype=torch.float64, device=device), torch.empty((n, 4, 4), dtype=torch.float64, device=device),
                       torch.empty((nc, 4, 4), dtype=torch.float64, device=device), torch.empty(n, dtype=torch.uint8, device=device),
                       torch.empty(_capi.BRIDGE_RECORD_DOUBLES, dtype=torch.float64, device=device))
        G, cams, origins, bridged, record = outputs
        if tuple(G.shape) != (n, 4, 4) or tuple(cams.shape) != (n, 4, 4) or tuple(origins.shape) != (nc, 4, 4) or tuple(bridged.shape) != (n,) \
                or record.numel() != _capi.BRIDGE_RECORD_DOUBLES or not all(t.is_contiguous() for t in outputs):
            raise ValueError("bridge_call: the outputs do not have the shapes of %d frames in %d chunks" % (n, nc))
        rc, msg = call.run(lib.gem_slam_bridge, _ptr(d_poses), C.c_void_p(mask8.ctypes.data), _ptr(d_mask),
                           C.c_void_p(sys32.ctypes.data if ns else 0), _ptr(d_sys if ns else None), ns,
                           C.c_void_p(starts32.ctypes.data if nc else 0), _ptr(d_starts if nc else None), nc, n,
                           _ptr(G), _ptr(cams), _ptr(origins), _ptr(bridged), _ptr(call.work(need)), need, _ptr(record))
    if not check:
        return rc, msg, G, cams, origins, bridged, record
    if rc:
        raise _capi.GemError(msg or "gem_slam_bridge failed")
    return G, cams, origins, bridged, record


def contiguous_span(spans):
    """(A, B) of chunks that follow one another without a hole; ValueError otherwise."""
    spans = [(int(a), int(b)) for a, b in spans]
    if not spans:
        raise ValueError("bridge: no chunks")
    for (a, b), (a2, _) in zip(spans, spans[1:] + [(spans[-1][1], None)]):
        if b <= a or a2 != b:
            raise ValueError("bridge: the chunks must follow one another without a hole, got %s" % spans)
    return spans[0][0], spans[-1][1]


def bridge_cameras(engine, rows, spans, fps, scale, max_gap=DEFAULT_MAX_GAP_SECONDS, stream=None, systems=None):
    """The cameras of a recording without ground truth whose trajectory (`slam.trajectory_rows`) lacks lines: the span from the first
    chunk's start to the last chunk's end is bridged as a whole (`find_gaps`, or its result for this span as `systems`;
    `gem_slam_bridge`) and cut into the chunks of `spans` on the device.
    -> ([cams [n_k,4,4] per chunk: device tensors, views of one block], origins [n_chunks,4,4] numpy, BridgeReport).
    With no lost frame the cameras are those of `prepare.scaled_cameras`, to rounding.  `engine`: anything with a `.device`."""
    from . import slam
    A, B = contiguous_span(spans)
    if systems is None:
        systems = find_gaps(slam.frame_ids(rows, fps), A, B, max_gap_frames(max_gap, fps))
    poses, mask = relative_rows(rows, A, B, fps, scale)
    device = getattr(engine, "device", engine)
    starts = [a - A for a, _ in spans]
    G, cams, origins, bridged, record = bridge_call(device, poses, mask, [(f - A, length) for f, length in systems], starts, stream)
    report = BridgeReport(record.cpu().numpy(), ~mask, [(A + a, m) for a, m in gap_list(mask)], fps, max_gap)
    if report.status != 0:
        raise ValueError("the bridge's equations could not be solved: the tracked poses around a gap are not finite")
    return [cams[a - A:b - A] for a, b in spans], origins.cpu().numpy(), report


# ------------------------------------------------------------------------------------------------------------------ command line
def _parser():
    import argparse
    p = argparse.ArgumentParser(description="the frames of a SLAM trajectory on which tracking was lost, and what --bridge would need")
    p.add_argument("--slam", required=True, help="SLAM trajectory: lines `time tx ty tz qx qy qz qw`")
    p.add_argument("--start", required=True, type=int)
    p.add_argument("--end", required=True, type=int)
    p.add_argument("--fps", type=float, default=25)
    p.add_argument("--max_gap", type=float, default=None, metavar="S", help="also say whether --bridge S would accept the span")
    p.add_argument("--json", default=None, metavar="FILE", help="write the gaps there too")
    return p


def _cli(argv=None):
    from . import slam
    from .ground import write_json
    a = _parser().parse_args(argv)
    with open(a.slam) as f:
        ids = slam.frame_ids(slam.trajectory_rows(f.read()), a.fps)
    mask = tracked_mask(ids, a.start, a.end)
    gaps = [(a.start + g, m) for g, m in gap_list(mask)]
    where = np.flatnonzero(mask)
    out = {"start": a.start, "end": a.end, "fps": a.fps, "frames": len(mask), "lost": int((~mask).sum()), "gaps": [list(g) for g in gaps],
           "first_tracked": int(a.start + where[0]) if len(where) else None, "last_tracked": int(a.start + where[-1]) if len(where) else None,
           "longest_gap": max([m for _, m in gaps], default=0)}
    print("[%d, %d) at %g fps: %d of %d frame ids have no line, in %d gaps" % (a.start, a.end, a.fps, out["lost"], out["frames"], len(gaps)))
    for g, m in gaps:
        print("  ids [%d, %d): %d frames = %.2f s" % (g, g + m, m, m / a.fps))
    if len(where):
        print("first tracked id %d, last tracked id %d; the longest gap needs --bridge %.2f or more%s"
              % (out["first_tracked"], out["last_tracked"], out["longest_gap"] / a.fps,
                 "" if out["longest_gap"] <= MAX_GAP else " and exceeds the hard cap of %d frames" % MAX_GAP))
    if a.max_gap is not None:
        try:
            systems = find_gaps(ids, a.start, a.end, max_gap_frames(a.max_gap, a.fps))
            out["accepted"], out["systems"] = True, [list(s) for s in systems]
            print("--bridge %g accepts the span: %d systems" % (a.max_gap, len(systems)))
        except ValueError as e:
            out["accepted"], out["refusal"] = False, str(e)
            print("--bridge %g refuses the span: %s" % (a.max_gap, e))
    write_json(a.json, out)
    return out


if __name__ == "__main__":
    _cli()
