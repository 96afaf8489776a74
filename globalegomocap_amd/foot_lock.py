"""Foot-skate clean-up of a pose sequence (no counterpart in the reference): every stance of a foot is held at
one place on the floor, and the leg follows by two-bone inverse kinematics from the unmoved hip.

A foot that stands does not move.  `ground.estimate_ground` measures how far a result is from that (`skate`); `gem_foot_lock` removes
it: with the contact rule and the plane of the ground estimate, every run of at least `min_run` contact frames of a foot is pinned to
the mean of its foot point, put onto the floor (`snap`); the correction is eased in and out over `blend` frames around the run; knee,
ankle and foot of that leg are re-solved with the frame's own bone lengths.  A target the leg cannot reach makes it straight and up
to `stretch` longer; beyond that the pin is missed and the frame is counted.  Only joints 8, 9, 10, 12, 13, 14 change.

    python -m globalegomocap_amd.foot_lock result_pose.pkl --out locked.pkl [--sequence optimized|estimated|both] [--fps 25] [--lag K]
           [--tau_v M] [--tau_h M] [--min_run FRAMES] [--blend FRAMES] [--stretch S] [--no_snap] [--json FILE]

writes the pose pickle with the chosen sequences replaced by their locked versions and prints, before and after side by side, the
slide inside the pinned stances and the ground report's `skate` and `penetration`.
"""
import ctypes as C
import os

import numpy as np

from . import _capi, ground as grounds
from ._binding import _ptr, call_stream, check_tensor, staged_call
from .ground import DEFAULT_FPS, TAU_H, TAU_V, default_lag

MIN_RUN, STRETCH = 3, 0.05
STATUS = {0: "ok", _capi.FOOT_LOCK_NO_CONTACT: "no_contact"}


def default_blend(fps):
    """0.12 s in frames, at least one."""
    return max(1, int(round(0.12 * fps)))


class FootLock:
    """`sequence`: the cleaned sequence, a float64 device tensor [F,15,3] (None where the record was made from a host record alone);
    `status`: "ok" or "no_contact" (no stance was found: the sequence is a copy); `runs` and `pinned` (right, left): stances and the
    frames inside them; `changed`: frames with a leg that moved; `lengthened`: legs (frame and side) made straight and longer;
    `unreachable`: legs whose target was missed; `delta_max`, `delta_mean`: metres a pinned foot point was moved; `knee_max`: the
    largest displacement of a knee; `stretch_max`: the largest lengthening factor; `slide_before`, `slide_after`: metres per frame a
    foot point moves along the floor between consecutive frames of one stance (`slide_pairs` of them), `slide_before_speed` and
    `slide_after_speed` the same in metres per second; `frames`, `fps`; `ground`: the GroundEstimate that was used."""

    def __init__(self, record, fps=DEFAULT_FPS, sequence=None, ground=None):
        r = _capi.GemFootLockRecord.from_buffer_copy(np.ascontiguousarray(record, dtype=np.float64).tobytes())
        self.status = STATUS[int(r.status)]
        self.runs, self.pinned = (int(r.runs_right), int(r.runs_left)), (int(r.pinned_right), int(r.pinned_left))
        self.changed, self.lengthened, self.unreachable = int(r.changed), int(r.lengthened), int(r.unreachable)
        self.delta_max, self.delta_mean, self.knee_max, self.stretch_max = r.delta_max, r.delta_mean, r.knee_max, r.stretch_max
        self.slide_before, self.slide_after, self.slide_pairs = r.slide_before, r.slide_after, int(r.slide_pairs)
        self.frames, self.fps = int(r.frames), float(fps)
        self.slide_before_speed, self.slide_after_speed = r.slide_before * self.fps, r.slide_after * self.fps
        self.sequence, self.ground = sequence, ground
        self.record = np.array(record, dtype=np.float64)

    def as_dict(self):
        """Plain numbers and lists (JSON)."""
        return {"status": self.status, "runs": list(self.runs), "pinned": list(self.pinned), "changed": self.changed, "lengthened": self.lengthened,
                "unreachable": self.unreachable, "delta_max": self.delta_max, "delta_mean": self.delta_mean, "knee_max": self.knee_max,
                "stretch_max": self.stretch_max, "slide_before": self.slide_before_speed, "slide_after": self.slide_after_speed,
                "slide_pairs": self.slide_pairs, "frames": self.frames, "fps": self.fps}

    def line(self):
        if self.status != "ok":
            return "foot lock: no stance found in %d frames, nothing changed" % self.frames
        return ("foot lock: %d + %d stances, %d + %d pinned frames of %d, slide %.4f -> %.4f m/s, moved %.4f m on average (%.4f m at most), "
                "%d legs lengthened (%.3f at most), %d unreachable" % (self.runs + self.pinned + (self.frames, self.slide_before_speed, self.slide_after_speed,
                                                                                                  self.delta_mean, self.delta_max, self.lengthened,
                                                                                                  self.stretch_max, self.unreachable)))


def lock_call(engine, sequences, ground_records, lag, tau_v=TAU_V, tau_h=TAU_H, min_run=MIN_RUN, blend=3, snap=True, stretch=STRETCH, stream=None,
              outputs=None):
    """gem_foot_lock on device tensors [F,15,3] f64 (contiguous) and their ground records, a device tensor [n,48] as `ground.ground_call`
    gives it -> (the cleaned sequences, tensors of their own; the records, a device tensor [n,24]).  outputs: the tensors to write
    to.  ONE upload (the table), no synchronisation."""
    import torch
    lib, n = engine.lib, len(sequences)
    grounds.check_sequences("lock_feet", sequences)
    check_tensor(ground_records, torch.float64, (n, _capi.GROUND_RECORD_DOUBLES),
                 error=ValueError("lock_feet: the ground records must be a contiguous float64 device tensor [%d,%d]" % (n, _capi.GROUND_RECORD_DOUBLES)))
    addresses, frames, offsets, need = grounds.sequence_table(lib, lib.gem_foot_lock_work, sequences)
    with staged_call(lib, engine.device, stream) as call:
        outs = [torch.empty_like(x) for x in sequences] if outputs is None else list(outputs)
        table = np.concatenate([addresses, frames, np.array([y.data_ptr() if len(y) else 0 for y in outs], dtype=np.int64), offsets])
        d_table, = call.upload(table)
        records = torch.empty(max(n, 1), _capi.FOOT_LOCK_RECORD_DOUBLES, dtype=torch.float64, device=engine.device)
        rc, _ = call.run(lib.gem_foot_lock, C.c_void_p(table.ctypes.data), _ptr(d_table), n, _ptr(ground_records), int(lag), float(tau_v),
                         float(tau_h), int(min_run), int(blend), 1 if snap else 0, float(stretch), _ptr(call.work(need)), need, _ptr(records))
    _capi.check(rc, lib)
    return outs, records[:n]


def lock_feet(engine, sequences, fps=DEFAULT_FPS, lag=None, tau_v=TAU_V, tau_h=TAU_H, min_run=MIN_RUN, blend=None, snap=True, stretch=STRETCH,
              ground=None, stream=None):
    """`sequences` with their standing feet pinned: one global sequence [F,15,3] in metres (array or tensor) -> a FootLock, or a list of
    sequences -> a list of them, all in ONE ground launch plus ONE lock launch and one small read-back.  lag, tau_v, tau_h: the
    contact rule of `ground.estimate_ground`; min_run: the fewest consecutive contact frames that make a stance; blend: frames over
    which the correction is eased in and out (default 0.12 s at `fps`); snap: the pin is put onto the floor; stretch: how much longer
    than its bones a straight leg may become to hold its pin.  ground: a GroundEstimate (or a list, one per sequence) made elsewhere
    with the same lag, tau_v and tau_h, instead of the estimate made here.  ValueError naming the sequence whose ground cannot be
    estimated; a sequence without a stance comes back as a copy with status "no_contact"."""
    import torch
    from .meshes import _sequence
    one = not isinstance(sequences, (list, tuple))
    seqs = [_sequence(engine, s) for s in ([sequences] if one else sequences)]
    if not seqs:
        raise ValueError("lock_feet: no sequence")
    if not fps > 0:
        raise ValueError("fps must be positive, got %r" % (fps,))
    lag = default_lag(fps) if lag is None else int(lag)
    blend = default_blend(fps) if blend is None else int(blend)
    given = None
    if ground is not None:
        given = [ground] * len(seqs) if isinstance(ground, grounds.GroundEstimate) else list(ground)
        if len(given) != len(seqs) or not all(isinstance(g, grounds.GroundEstimate) for g in given):
            raise TypeError("lock_feet: ground must be a GroundEstimate or a list of one per sequence")
        g_records = engine._f64(np.stack([g.record for g in given]))
    else:
        g_records = grounds.ground_call(engine, seqs, lag, tau_v, tau_h, stream=stream)
    outs, records = lock_call(engine, seqs, g_records, lag, tau_v, tau_h, min_run, blend, snap, stretch, stream)
    with torch.cuda.device(engine.device), torch.cuda.stream(call_stream(engine.device, stream)):
        host = torch.cat([g_records.reshape(-1), records.reshape(-1)]).cpu().numpy()          # (the one read-back)
    n = len(seqs)
    g_host, l_host = host[:n * _capi.GROUND_RECORD_DOUBLES].reshape(n, -1), host[n * _capi.GROUND_RECORD_DOUBLES:].reshape(n, -1)
    found = []
    for i in range(n):
        status = int(l_host[i, 0])
        if status == _capi.FOOT_LOCK_BAD_GROUND:
            raise ValueError("lock_feet: sequence %d (%d frames): its ground cannot be estimated (ground status %d: a joint that is not a "
                             "number, or neck and feet in one place)" % (i, len(seqs[i]), int(g_host[i, 0])))
        if status not in STATUS:
            raise ValueError("lock_feet: sequence %d cannot be used (%d frames; at least one is needed)" % (i, len(seqs[i])))
        estimate = given[i] if given is not None else grounds.GroundEstimate(g_host[i], fps, g_records[i, 23:36])
        found.append(FootLock(l_host[i], fps, outs[i], estimate))
    return found[0] if one else found


# ------------------------------------------------------------------------------------------------------------------ command line
def _parser():
    import argparse
    p = argparse.ArgumentParser(description="pin the standing feet of the sequences of a saved result_pose.pkl and re-solve the legs")
    p.add_argument("pose_pickle", help="result_pose.pkl as --save_pose writes it: estimated_pose and optimized_pose")
    p.add_argument("--out", required=True, metavar="FILE", help="the pose pickle to write, the chosen sequences replaced by their locked versions")
    p.add_argument("--sequence", default="optimized", choices=("optimized", "estimated", "both"), help="which sequence to lock (default optimized)")
    grounds.add_contact_arguments(p)
    p.add_argument("--min_run", type=int, default=MIN_RUN, help="the fewest consecutive contact frames that make a stance (default 3)")
    p.add_argument("--blend", type=int, default=None, help="frames over which the correction is eased in and out (default: 0.12 s)")
    p.add_argument("--stretch", type=float, default=STRETCH, help="how much longer a straight leg may become to hold its pin (default 0.05)")
    p.add_argument("--no_snap", action="store_true", help="pin a stance where its foot point was on average, not on the floor")
    p.add_argument("--json", default=None, metavar="FILE", help="write the reports there too")
    return p


def report_text(names, locks, before, after):
    """Before and after side by side: per sequence the slide inside the stances, and the ground report's skate and penetration."""
    lines = ["%-30s" % "" + "".join("%16s%16s" % (n, "locked") for n in names)]
    rows = (("slide (m/s)", [(l.slide_before_speed, l.slide_after_speed) for l in locks], "%.4f"),
            ("skate (m/s)", [(b.skate, a.skate) for b, a in zip(before, after)], "%.4f"),
            ("penetration (m)", [(b.penetration, a.penetration) for b, a in zip(before, after)], "%.4f"))
    for label, cells, fmt in rows:
        lines.append("%-30s" % label + "".join("%16s%16s" % (fmt % c[0], fmt % c[1]) for c in cells))
    return "\n".join(lines)


def _cli(argv=None):
    import pickle
    p = _parser()
    a = p.parse_args(argv)
    rule = grounds.contact_arguments(p, a, frame_counts=("lag", "blend"))
    if a.min_run < 1:
        p.error("argument --min_run: at least one frame")
    if not (np.isfinite(a.stretch) and a.stretch >= 0):
        p.error("argument --stretch: a number that is not negative")
    names = ["optimized", "estimated"] if a.sequence == "both" else [a.sequence]
    d, engine = grounds.cli_inputs(p, a.pose_pickle, [k + "_pose" for k in names], "no HIP device visible: the feet are locked on the device")
    locks = lock_feet(engine, [np.asarray(d[k + "_pose"], dtype=np.float64) for k in names], min_run=a.min_run, blend=a.blend, snap=not a.no_snap,
                      stretch=a.stretch, **rule)
    after = grounds.estimate_ground(engine, [l.sequence for l in locks], **rule)
    print(report_text(names, locks, [l.ground for l in locks], after))
    for name, l in zip(names, locks):
        print("%s: %s" % (name, l.line()))
    out = dict(d)
    for name, l in zip(names, locks):
        seq = l.sequence.cpu().numpy()
        out[name + "_pose"] = seq if isinstance(d[name + "_pose"], np.ndarray) else list(seq)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "wb") as f:
        pickle.dump(out, f)
    grounds.write_json(a.json, {name: dict(l.as_dict(), ground_before=l.ground.as_dict(), ground_after=g.as_dict())
                                for name, l, g in zip(names, locks, after)})
    return dict(zip(names, locks))


if __name__ == "__main__":
    _cli()
