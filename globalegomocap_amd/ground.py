"""The ground plane of a pose sequence from its foot contacts, and the upright frame it defines (no counterpart
in the reference, whose files lie in the frame of the chunk's first camera: a fisheye on the forehead that looks down).

A foot that stands does not move, and the places where the feet stand lie on the floor.  `gem_ground_plane` finds the still foot
points of a sequence, fits the plane through them and derives the rigid transform into an upright frame -- Y up, the floor at height
0, the wearer at the origin and facing +Z in the first frame -- in the 13-double (c, R, t) form of `WindowEngine.sequence_align`,
which every writer applies (`move=`, `upright=`).  The same pass reports what a user without ground truth wants to know about a
result's feet: how much they slide while they stand, and how far they sink into the floor.

    python -m globalegomocap_amd.ground result_pose.pkl [--fps 25] [--lag K] [--tau_v M] [--tau_h M] [--foot_height M] [--json FILE]

prints the report for the estimated and the optimised sequence side by side (and for gt_pose where the pickle has one), and the
angle between their normals: whether the optimiser reduced foot skating.
"""
import ctypes as C
import os

import numpy as np

from . import _capi
from ._binding import _ptr, _stream, check_tensor, staged_call

TAU_V, TAU_H, MIN_SPREAD, MIN_POINTS = 0.10, 0.05, 0.05, 8
DEFAULT_FPS = 25.0


def default_lag(fps):
    """0.2 s in frames, at least one."""
    return max(1, int(round(0.2 * fps)))


class GroundEstimate:
    """`normal` [3] and `offset` of the plane normal . p = offset; `source`: "plane", "body_normal" (the contacts span no plane: the
    body's direction, the contacts' height) or "body" (too few contacts: the lowest foot point); `body_up` and `tilt_deg`, the angle
    between the two; the counts `points` (contact candidates) and `inliers` with their residual `rms`; `spread` and `extent`, metres:
    the square roots of the middle and the largest eigenvalue of the contacts' scatter; `contact_share` (right, left): the share of
    frames in contact; `skate`, metres per second a foot in contact slides along the floor (`skate_pairs`: over how many pairs of
    frames); `penetration` and `lift_max`, metres below and above the plane; `frames`, `lag`, `fps`; `crt`: the upright transform as
    a device tensor [13] (None where the estimate was made from a host record alone)."""

    def __init__(self, record, fps=DEFAULT_FPS, crt=None):
        r = _capi.GemGroundRecord.from_buffer_copy(np.ascontiguousarray(record, dtype=np.float64).tobytes())
        self.status, self.source = int(r.status), _capi.GROUND_SOURCES[int(r.source)]
        self.normal, self.offset, self.body_up = np.array(r.n), r.d, np.array(r.u0)
        self.tilt_deg = float(np.degrees(np.arctan2(np.linalg.norm(np.cross(self.normal, self.body_up)), r.tilt_cos)))
        self.points, self.inliers, self.rms, self.spread, self.extent = int(r.points), int(r.inliers), r.rms, r.spread, r.extent
        self.frames, self.lag, self.fps = int(r.frames), int(r.lag), float(fps)
        self.contact_frames = (int(r.contact_right), int(r.contact_left))
        self.contact_share = tuple(c / max(self.frames, 1) for c in self.contact_frames)
        self.skate, self.skate_pairs = r.skate * self.fps, int(r.skate_pairs)
        self.penetration, self.lift_max = r.penetration, r.lift_max
        self.crt_host = np.array(r.crt)
        self.crt = crt
        self.record = np.array(record, dtype=np.float64)

    def as_dict(self):
        """Plain numbers and lists (JSON)."""
        return {"normal": self.normal.tolist(), "offset": self.offset, "source": self.source, "tilt_deg": self.tilt_deg, "points": self.points,
                "inliers": self.inliers, "rms": self.rms, "spread": self.spread, "extent": self.extent,
                "contact_share": list(self.contact_share), "skate": self.skate, "skate_pairs": self.skate_pairs, "penetration": self.penetration,
                "lift_max": self.lift_max, "frames": self.frames, "lag": self.lag, "fps": self.fps, "crt": self.crt_host.tolist()}

    def line(self):
        return ("ground: %s, tilt against the body %.2f deg, %d contact points (%d inliers, rms %.4f m, spread %.3f m), contact right / left "
                "%.2f / %.2f, skate %.4f m/s, penetration %.4f m" % ((self.source, self.tilt_deg, self.points, self.inliers, self.rms, self.spread)
                                                                     + self.contact_share + (self.skate, self.penetration)))


def _transform(engine, t, what):
    import torch
    wrong = TypeError("%s must be a contiguous float64 device tensor [13] or [n,13]" % what)
    check_tensor(t, torch.float64, at_least=1, error=wrong)
    if t.shape[-1] != 13:
        raise wrong
    return t


def check_sequences(who, sequences):
    """What `ground_call` and `foot_lock.lock_call` ask of every sequence: a contiguous float64 device tensor [F,15,3], any F."""
    import torch
    for x in sequences:
        check_tensor(x, torch.float64, (None, 15, 3), error=ValueError("%s: a sequence must be a contiguous float64 device tensor [F,15,3]" % who))


def sequence_table(lib, work_fn, sequences):
    """The head of the tables of `gem_ground_plane` and `gem_foot_lock` -> (the sequences' addresses, their frames, their offsets in
    the work buffer, its bytes as `work_fn` fixes them); GemError with the library's text where it refuses the sizes."""
    n = len(sequences)
    frames = np.array([len(x) for x in sequences], dtype=np.int64)
    offsets = np.full(max(n, 1), -1, dtype=np.int64)
    need = int(work_fn(C.c_void_p(frames.ctypes.data), n, C.c_void_p(offsets.ctypes.data))) if n else 0
    if need < 0:
        raise _capi.GemError((lib.gem_last_error() or b"").decode())
    return np.array([x.data_ptr() if len(x) else 0 for x in sequences], dtype=np.int64), frames, offsets[:n], need


def compose(engine, a, b):
    """The similarity `a`, then `b` (gem_similarity_compose): device tensors [13] or [n,13] of (c, R row-major, t), as
    `WindowEngine.sequence_align` and `GroundEstimate.crt` give them -> one of the same shape.  No synchronisation."""
    import torch
    a, b = _transform(engine, a, "compose: a"), _transform(engine, b, "compose: b")
    if a.shape != b.shape:
        raise ValueError("compose: a and b must have one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    out = torch.empty_like(a)
    _capi.check(engine.lib.gem_similarity_compose(_ptr(a), _ptr(b), _ptr(out), a.numel() // 13, _stream()), engine.lib)
    return out


def ground_call(engine, sequences, lag, tau_v=TAU_V, tau_h=TAU_H, min_spread=MIN_SPREAD, min_points=MIN_POINTS, foot_height=0.0, moved_by=None,
                stream=None):
    """gem_ground_plane on device tensors [F,15,3] f64 (contiguous, each its own allocation or not); moved_by: per sequence a [13] device
    tensor that is applied to its joints first, or None -> the records, a device tensor [n, 48].  ONE upload (the table), no
    synchronisation."""
    import torch
    lib, n = engine.lib, len(sequences)
    moved_by = [None] * n if moved_by is None else list(moved_by)
    if len(moved_by) != n:
        raise ValueError("estimate_ground: %d transforms for %d sequences" % (len(moved_by), n))
    check_sequences("estimate_ground", sequences)
    for m in moved_by:
        if m is not None and _transform(engine, m, "estimate_ground: moved_by").numel() != 13:
            raise TypeError("estimate_ground: moved_by holds one [13] transform per sequence")
    addresses, frames, offsets, need = sequence_table(lib, lib.gem_ground_plane_work, sequences)
    table = np.concatenate([addresses, frames, np.array([0 if m is None else m.data_ptr() for m in moved_by], dtype=np.int64), offsets])
    with staged_call(lib, engine.device, stream) as call:
        d_table, = call.upload(table)
        records = torch.empty(max(n, 1), _capi.GROUND_RECORD_DOUBLES, dtype=torch.float64, device=engine.device)
        rc, _ = call.run(lib.gem_ground_plane, C.c_void_p(table.ctypes.data), _ptr(d_table), n, int(lag), float(tau_v), float(tau_h),
                         float(min_spread), int(min_points), float(foot_height), _ptr(call.work(need)), need, _ptr(records))
    _capi.check(rc, lib)
    return records[:n]


def estimate_ground(engine, sequences, fps=DEFAULT_FPS, lag=None, tau_v=TAU_V, tau_h=TAU_H, min_spread=MIN_SPREAD, min_points=MIN_POINTS,
                    foot_height=0.0, moved_by=None, stream=None):
    """The ground plane, the foot figures and the upright transform of `sequences`: one global sequence [F,15,3] in metres (array or
    tensor) -> a GroundEstimate, or a list of sequences -> a list of them, all in ONE launch.  lag: frames between the two frames of a
    still pair (default 0.2 s at `fps`); tau_v: metres a standing foot may seem to move over the lag; tau_h: metres a contact may lie
    off the plane; min_spread, min_points: what a plane needs; foot_height: how far above the floor a standing foot point lies, so
    that the upright frame's y = 0 is the floor.  moved_by: a [13] device tensor (or one or None per sequence) that is applied to the
    joints first: the alignment the writers apply, behind which the upright transform then goes.  One upload of the table and one
    small record back; ValueError naming the sequence that has no body direction (a NaN joint, or neck and feet in one place)."""
    import torch
    from .meshes import _sequence
    one = not isinstance(sequences, (list, tuple))
    seqs = [_sequence(engine, s) for s in ([sequences] if one else sequences)]
    if not seqs:
        raise ValueError("estimate_ground: no sequence")
    if one or torch.is_tensor(moved_by):
        moved_by = [moved_by] * len(seqs)
    if not fps > 0:
        raise ValueError("fps must be positive, got %r" % (fps,))
    lag = default_lag(fps) if lag is None else int(lag)
    records = ground_call(engine, seqs, lag, tau_v, tau_h, min_spread, min_points, foot_height, moved_by, stream)
    host = records.cpu().numpy()
    out = []
    for i, row in enumerate(host):
        status = int(row[0])
        if status == _capi.GROUND_NO_BODY:
            raise ValueError("estimate_ground: sequence %d (%d frames) has no body direction: a joint that is not a number, or neck and feet in "
                             "one place" % (i, len(seqs[i])))
        if status:
            raise ValueError("estimate_ground: sequence %d cannot be used (%d frames; at least one is needed)" % (i, len(seqs[i])))
        out.append(GroundEstimate(row, fps, records[i, 23:36]))
    return out[0] if one else out


def upright_sequence(engine, seq, estimate):
    """`seq` [F,15,3] moved into the estimate's upright frame -> a float64 device tensor [F,15,3]: c * (p . R) + t."""
    from .meshes import _sequence
    x, k = _sequence(engine, seq), estimate.crt if estimate.crt is not None else engine._f64(estimate.crt_host)
    return k[0] * (x @ k[1:10].reshape(3, 3)) + k[10:13]


def resolve(engine, upright, reference, **options):
    """What the writers make of their `upright` argument: None / False -> None; True -> the estimate of `reference`; a GroundEstimate ->
    that one."""
    if upright is None or upright is False:
        return None
    if upright is True:
        return estimate_ground(engine, reference, **options)
    if not isinstance(upright, GroundEstimate):
        raise TypeError("upright must be None, a bool or a GroundEstimate, got %r" % (upright,))
    if upright.crt is None:
        upright.crt = engine._f64(upright.crt_host)
    return upright


# ------------------------------------------------------------------------------------------------------------------ command line
def add_contact_arguments(p):
    """`--fps`, `--lag`, `--tau_v` and `--tau_h`: the contact rule, as this module's and `foot_lock`'s command lines take it."""
    p.add_argument("--fps", type=float, default=DEFAULT_FPS, help="frames per second of the sequences (default 25)")
    p.add_argument("--lag", type=int, default=None, help="frames between the two frames of a still pair (default: 0.2 s)")
    p.add_argument("--tau_v", type=float, default=TAU_V, help="metres a standing foot may seem to move over the lag")
    p.add_argument("--tau_h", type=float, default=TAU_H, help="metres a contact may lie off the plane")


def contact_arguments(p, a, frame_counts=("lag",)):
    """The rules of `add_contact_arguments`, as parser errors -> the contact rule as keyword arguments.  frame_counts: the options
    that count frames, --lag and the caller's own."""
    if not a.fps > 0:
        p.error("argument --fps: must be positive")
    for name in frame_counts:
        if getattr(a, name) is not None and getattr(a, name) < 1:
            p.error("argument --%s: at least one frame" % name)
    for name in ("tau_v", "tau_h"):
        if not (np.isfinite(getattr(a, name)) and getattr(a, name) > 0):
            p.error("argument --%s: a positive number of metres" % name)
    return dict(fps=a.fps, lag=a.lag, tau_v=a.tau_v, tau_h=a.tau_h)


def cli_inputs(p, path, keys, no_device):
    """What a command line on a pose pickle starts from -> (the pickle at `path`, which must hold every one of `keys`: a parser error
    names the one it lacks; an engine that needs no VAE, on the current device: GemError(`no_device`) where there is none)."""
    import pickle
    import torch
    with open(path, "rb") as f:
        d = pickle.load(f)
    for key in keys:
        if key not in d:
            p.error("%s has no %s" % (path, key))
    if not torch.cuda.is_available():
        raise _capi.GemError(no_device)
    from .camera import DEFAULT_CALIBRATION
    from .prepare import _lift_engine
    return d, _lift_engine(DEFAULT_CALIBRATION, torch.cuda.current_device())


def write_json(path, data):
    """`data` as JSON into `path` (its directory is made), unless `path` is None."""
    import json
    if path is not None:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(data, f, indent=1)


def _parser():
    import argparse
    p = argparse.ArgumentParser(description="the ground plane and the foot-contact figures of a saved result_pose.pkl")
    p.add_argument("pose_pickle", help="result_pose.pkl as --save_pose writes it: estimated_pose, optimized_pose and, optionally, gt_pose")
    add_contact_arguments(p)
    p.add_argument("--foot_height", type=float, default=0.0, help="metres a standing foot point lies above the floor")
    p.add_argument("--json", default=None, metavar="FILE", help="write the reports there too")
    return p


REPORT_ROWS = (("source", "source", "%s"), ("tilt against the body (deg)", "tilt_deg", "%.3f"), ("contact points", "points", "%d"),
               ("inliers", "inliers", "%d"), ("residual rms (m)", "rms", "%.4f"), ("spread (m)", "spread", "%.3f"),
               ("contact share right", "contact_right", "%.3f"), ("contact share left", "contact_left", "%.3f"), ("skate (m/s)", "skate", "%.4f"),
               ("penetration (m)", "penetration", "%.4f"))


def report_text(estimates):
    """The side-by-side report of {name: GroundEstimate} as text."""
    names = list(estimates)
    lines = ["%-30s" % "" + "".join("%16s" % n for n in names)]
    for label, key, fmt in REPORT_ROWS:
        cells = []
        for n in names:
            e = estimates[n]
            v = e.contact_share[0] if key == "contact_right" else e.contact_share[1] if key == "contact_left" else getattr(e, key)
            cells.append("%16s" % (fmt % v))
        lines.append("%-30s" % label + "".join(cells))
    return "\n".join(lines)


def normal_angle(a, b):
    """Degrees between the normals of two estimates."""
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(a.normal, b.normal)), float(a.normal @ b.normal))))


def _cli(argv=None):
    p = _parser()
    a = p.parse_args(argv)
    rule = contact_arguments(p, a)
    d, engine = cli_inputs(p, a.pose_pickle, ("estimated_pose", "optimized_pose"), "no HIP device visible: the ground plane is estimated on the device")
    names = ["estimated", "optimized"] + (["gt"] if d.get("gt_pose") is not None else [])
    seqs = [np.asarray(d[k + "_pose"], dtype=np.float64) for k in names]
    found = estimate_ground(engine, seqs, foot_height=a.foot_height, **rule)
    estimates = dict(zip(names, found))
    print(report_text(estimates))
    angle = normal_angle(estimates["estimated"], estimates["optimized"])
    print("angle between the normals of the estimated and the optimised sequence: %.3f deg" % angle)
    write_json(a.json, dict({k: e.as_dict() for k, e in estimates.items()}, normal_angle_deg=angle))
    return estimates


if __name__ == "__main__":
    _cli()
