"""Skeleton sequences as BVH animation files: motion that Blender, Maya, Unity or MotionBuilder load and retarget.

A file holds a 19-node skeleton on the 15 joints -- Hips on the midpoint of the hip joints, a Spine and two collar helpers with zero
offsets, rest directions along the axes (Y up, Z forward, +X the character's left), the rest lengths the sequence's mean bone
lengths -- and per frame 60 channels: the root's position and (Z, X, Y) Euler angles of every node's local rotation.  The library makes
all of it on the device: the rest lengths (gem_bvh_rest), the channels by position-only inverse kinematics (gem_bvh_channels) and the
motion block's text, "%15.6f" per channel, correctly rounded (gem_format_fields).  `write_bvh` moves the text device -> pinned memory
-> file in slices of frames through two alternating pinned buffers; Python formats the HIERARCHY block only.  `read_bvh`,
`joint_positions` and `skeleton_from_nodes` read such a file back into joint positions.

    python -m globalegomocap_amd.bvh out/<dataset>/<chunk>/result_pose.pkl --out DIR [--fps F] [--align true] [--unit_scale S]
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

from . import _capi
from ._binding import _ptr, _stream, check_tensor
from .meshes import _alignment, _sequence, _upright, result_poses

Layout = namedtuple("Layout", "nodes channels field_bytes frame_bytes")
Tables = namedtuple("Tables", "parents joint_of_node rest_dirs")
Parsed = namedtuple("Parsed", "names parents offsets channels frame_time motion")
NODE_NAMES = ("Hips", "Spine", "Neck", "Right_collar", "Right_shoulder", "Right_elbow", "Right_wrist", "Left_collar", "Left_shoulder",
              "Left_elbow", "Left_wrist", "Right_hip", "Right_knee", "Right_ankle", "Right_foot", "Left_hip", "Left_knee", "Left_ankle",
              "Left_foot")
ROOT_CHANNELS = ("Xposition", "Yposition", "Zposition", "Zrotation", "Xrotation", "Yrotation")
DEFAULT_FPS = 25                 # frames per second of a file wherever a caller gives none
PINNED_BYTES = 16 << 20          # each of the two pinned buffers the text crosses PCIe through (17 476 frames), whatever the sequence's length
FILE_NAMES = ("estimated.bvh", "optimized.bvh", "gt.bvh")

_layout = None
_tables = None


def layout():
    """Nodes, channels per frame, bytes per field and per frame of the motion block (gem_bvh_layout); needs no GPU."""
    global _layout
    if _layout is None:
        lib = _capi.load_library()
        out = (C.c_int64 * 4)()
        _capi.check(lib.gem_bvh_layout(out), lib)
        _layout = Layout(*[int(v) for v in out])
    return _layout


def tables():
    """The tree (gem_bvh_tables): parents [19] (-1: the root), joint_of_node [19] (-1: Hips and the helpers), rest_dirs [19,3]; needs no GPU."""
    global _tables
    if _tables is None:
        lib, n = _capi.load_library(), layout().nodes
        parents, joints, rest = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_double * (3 * n))()
        _capi.check(lib.gem_bvh_tables(parents, joints, rest), lib)
        _tables = Tables(np.array(parents, dtype=np.int32), np.array(joints, dtype=np.int32), np.array(rest, dtype=np.float64).reshape(n, 3))
        for t in _tables:
            t.setflags(write=False)
    return _tables


def rest_lengths(engine, seq_d, crt=None):
    """The rest length of every node's bone (gem_bvh_rest): the mean of |pos(node) - pos(parent)| over the frames of `seq_d` [F,15,3]
    (contiguous float64 device tensor, F >= 1), the joints moved by `crt` ([13] from `engine.sequence_align`) first when given ->
    [19] f64 on the device, 0 for the root and the helpers.  No synchronisation; the same bits on every call."""
    import torch
    out = torch.empty(layout().nodes, device=seq_d.device, dtype=torch.float64)
    _capi.check(engine.lib.gem_bvh_rest(_ptr(seq_d), seq_d.shape[0], _ptr(crt), _ptr(out), _stream()), engine.lib)
    return out


def channels(engine, seq_d, crt, rest, unit_scale=100.0):
    """The channels of every frame (gem_bvh_channels) -> [F,60] f64 on the device: the root's position times `unit_scale`, then the
    19 nodes' (Z, X, Y) Euler angles in degrees.  Arguments as `rest_lengths`; `rest` is its result.  No synchronisation."""
    import torch
    out = torch.empty(seq_d.shape[0], layout().channels, device=seq_d.device, dtype=torch.float64)
    _capi.check(engine.lib.gem_bvh_channels(_ptr(seq_d), seq_d.shape[0], _ptr(crt), _ptr(rest), C.c_double(float(unit_scale)), _ptr(out), _stream()),
                engine.lib)
    return out


def new_counter(device):
    """The device-side counter `format_fields` raises: int64 [2] = (fields that are not numbers of the field's width, the first line with one
    or -1)."""
    import torch
    return torch.tensor([0, -1], dtype=torch.int64, device=device)


def format_fields(engine, values, values_per_line, bad, out=None):
    """`values` (contiguous float64 device tensor) as text (gem_format_fields): 16 bytes per value, "%15.6f" and a space, a newline
    after every `values_per_line`-th -> uint8 device tensor [values.numel() * 16], `out` when given (16-byte aligned).  nan, inf and
    values beyond +-9999999.999999 raise `bad` (`new_counter`).  No synchronisation."""
    import torch
    check_tensor(values, torch.float64, error=TypeError("format_fields wants a contiguous float64 device tensor"))
    n, fb = values.numel(), layout().field_bytes
    if out is None:
        out = torch.empty(n * fb, device=values.device, dtype=torch.uint8)
    check_tensor(out, torch.uint8, at_least=n * fb,
                 error=ValueError("format_fields: out must be a contiguous uint8 device tensor of at least %d bytes" % (n * fb)))
    check_tensor(bad, torch.int64, numel=2, error=TypeError("format_fields: bad must be an int64 device tensor of 2 values (new_counter)"))
    _capi.check(engine.lib.gem_format_fields(_ptr(values), n, int(values_per_line), _ptr(out), _ptr(bad), _stream()), engine.lib)
    return out[:n * fb]


def hierarchy_text(rest, unit_scale=100.0):
    """The HIERARCHY block for the rest lengths `rest` [19] (metres): every node's OFFSET is its rest direction times its rest length
    times `unit_scale`; the wrists and feet end in an `End Site` of offset 0."""
    tab, rest = tables(), np.asarray(rest, dtype=np.float64)
    kids = [[c for c in range(len(NODE_NAMES)) if tab.parents[c] == n] for n in range(len(NODE_NAMES))]
    lines = ["HIERARCHY"]

    def node(n, depth):
        pad = "  " * depth
        off = tab.rest_dirs[n] * rest[n] * unit_scale + 0.0          # (+ 0.0: no "-0.000000" for the zero components)
        lines.append("%s%s %s" % (pad, "ROOT" if n == 0 else "JOINT", NODE_NAMES[n]))
        lines.append(pad + "{")
        lines.append("%s  OFFSET %.6f %.6f %.6f" % ((pad,) + tuple(off)))
        names = ROOT_CHANNELS if n == 0 else ROOT_CHANNELS[3:]
        lines.append("%s  CHANNELS %d %s" % (pad, len(names), " ".join(names)))
        for c in kids[n]:
            node(c, depth + 1)
        if not kids[n]:
            lines.extend([pad + "  End Site", pad + "  {", pad + "    OFFSET 0.000000 0.000000 0.000000", pad + "  }"])
        lines.append(pad + "}")
    node(0, 0)
    return "\n".join(lines) + "\n"


def write_bvh(engine, seq, path, fps=DEFAULT_FPS, align_to=None, unit_scale=100.0, move=None):
    """`seq` [F,15,3] (array or tensor, metres, F >= 1) as the BVH file `path`, one keyed frame per frame at `fps`; positions and
    offsets are metres times `unit_scale` (100: centimetres, what most importers assume).  align_to [F,15,3]: the sequence is first
    moved by the one similarity transform that takes it onto `align_to` (`errors.align_sequence`).  move: a [13] device tensor
    (c, R, t), for instance `GroundEstimate.crt`, applied behind the alignment.  Rest lengths, channels and the
    motion block's text are made on the device; the text crosses PCIe in slices of at most PINNED_BYTES through two alternating
    pinned buffers and is appended in order while the next slice is formatted and copied.  A frame with a channel that is no
    number or does not fit its field (a NaN joint, a position beyond +-9999999.999999 units) deletes the partial file and raises
    ValueError naming the frame.  Runs on the current stream; the file is complete and closed on return.  Returns F."""
    import torch
    from .staging import STOP, reader_pool, stream_out
    seq_d = _sequence(engine, seq)
    F, lay = seq_d.shape[0], layout()
    if F < 1:
        raise ValueError("a BVH file needs at least one frame")
    if not fps > 0:
        raise ValueError("fps must be positive, got %r" % (fps,))
    crt = _alignment(engine, seq_d, align_to, move)
    rest = rest_lengths(engine, seq_d, crt)
    chan = channels(engine, seq_d, crt, rest, unit_scale)
    per = max(1, PINNED_BYTES // lay.frame_bytes)
    header = hierarchy_text(rest.cpu().numpy(), unit_scale) + "MOTION\nFrames: %d\nFrame Time: %.6f\n" % (F, 1.0 / fps)
    pool = reader_pool("bvh", 1)          # one writer: the slices are appended in order
    counters = new_counter(engine.device).repeat((F + per - 1) // per, 1)          # one per slice: its first bad line counts from the slice's start
    failed = []

    def produce(k, out):
        n = min(per, F - k * per)
        format_fields(engine, chan[k * per:k * per + n], lay.channels, counters[k], out=out)
        return n * lay.frame_bytes, counters[k]

    def consume(k, data, side):
        count, first = side.view(torch.int64).tolist()
        if count:
            failed.append(k * per + first)
            return STOP
        return [pool.submit(f.write, data.numpy())]

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        stream_out(engine.device, "bvh", per * lay.frame_bytes, len(counters), produce, consume, side_bytes=16)
    if failed:
        os.remove(path)
        raise ValueError("%s: frame %d has a channel that is not a number of at most 7 digits before the point (a NaN joint, or a position "
                         "beyond the field at unit_scale %g): no file written" % (path, failed[0], unit_scale))
    return F


def release():
    """Give back the pinned and device buffers `write_bvh` keeps between calls."""
    from .staging import release_kept
    release_kept("bvh")


# ------------------------------------------------------------------------------------------------------------------ reading back
def read_bvh(path):
    """A BVH file as `write_bvh` writes it -> Parsed(names, parents [N] (-1: the root), offsets [N,3], channels (per node the tuple of
    its channel names), frame_time, motion [frames, C]).  Understands ROOT / JOINT / End Site / OFFSET / CHANNELS with the six channel
    names in any order; an End Site is no node.  It is for round trips: ValueError for anything else."""
    with open(path, "r") as f:
        tokens = f.read().split()
    names, parents, offsets, chans, stack, at = [], [], [], [], [], 0
    allowed = set(ROOT_CHANNELS)

    def need(word):
        nonlocal at
        if at >= len(tokens) or tokens[at] != word:
            raise ValueError("%s: expected %s, found %s" % (path, word, tokens[at] if at < len(tokens) else "the end of the file"))
        at += 1

    def floats(n):
        nonlocal at
        try:
            v = [float(t) for t in tokens[at:at + n]]
        except ValueError:
            v = []
        if len(v) != n:
            raise ValueError("%s: expected %d numbers at token %d" % (path, n, at))
        at += n
        return v

    need("HIERARCHY")
    while at < len(tokens) and tokens[at] != "MOTION":
        t = tokens[at]
        if t in ("ROOT", "JOINT"):
            if (t == "ROOT") != (not names) or at + 1 >= len(tokens):
                raise ValueError("%s: one ROOT, first, then JOINTs" % path)
            names.append(tokens[at + 1])
            parents.append(stack[-1] if stack else -1)
            offsets.append(None)
            chans.append(())
            at += 2
            need("{")
            stack.append(len(names) - 1)
        elif t == "End":
            at += 1
            need("Site")
            need("{")
            need("OFFSET")
            floats(3)
            need("}")
        elif t == "OFFSET" and stack:
            at += 1
            offsets[stack[-1]] = floats(3)
        elif t == "CHANNELS" and stack:
            n = int(tokens[at + 1]) if at + 1 < len(tokens) and tokens[at + 1].isdigit() else -1
            c = tuple(tokens[at + 2:at + 2 + max(n, 0)])
            if n < 0 or len(c) != n or not set(c) <= allowed or len(set(c)) != n:
                raise ValueError("%s: CHANNELS of %s" % (path, names[stack[-1]]))
            chans[stack[-1]] = c
            at += 2 + n
        elif t == "}" and stack:
            stack.pop()
            at += 1
        else:
            raise ValueError("%s: unexpected %s in the HIERARCHY" % (path, t))
    if stack or not names or any(o is None for o in offsets):
        raise ValueError("%s: the HIERARCHY is incomplete" % path)
    need("MOTION")
    need("Frames:")
    if at >= len(tokens) or not tokens[at].isdigit():
        raise ValueError("%s: Frames: wants a count" % path)
    n_frames = int(tokens[at])
    at += 1
    need("Frame")
    need("Time:")
    frame_time = floats(1)[0]
    width = sum(len(c) for c in chans)
    try:
        motion = np.array(tokens[at:], dtype=np.float64)
    except ValueError:
        raise ValueError("%s: the motion block holds something that is no number" % path)
    if motion.size != n_frames * width:
        raise ValueError("%s: %d numbers in the motion block, but %d frames of %d channels" % (path, motion.size, n_frames, width))
    return Parsed(tuple(names), np.array(parents, dtype=np.int32), np.array(offsets, dtype=np.float64).reshape(-1, 3), tuple(chans),
                  frame_time, motion.reshape(n_frames, width))


def _axis_rotation(axis, deg):
    a = np.radians(deg)
    c, s, o, z = np.cos(a), np.sin(a), np.ones_like(a), np.zeros_like(a)
    m = {"X": [[o, z, z], [z, c, -s], [z, s, c]], "Y": [[c, z, s], [z, o, z], [-s, z, c]], "Z": [[c, -s, z], [s, c, z], [z, z, o]]}[axis]
    return np.stack([np.stack(r, axis=-1) for r in m], axis=-2)


def joint_positions(parsed):
    """Forward kinematics of a `read_bvh` result on the host -> [frames, nodes, 3] in the file's units: a node's local transform is its
    OFFSET plus its position channels, then its rotation channels as matrices multiplied in the order of the channels."""
    n, N = parsed.motion.shape[0], len(parsed.names)
    pos, G, at = np.zeros((n, N, 3)), np.zeros((n, N, 3, 3)), 0
    for k in range(N):
        t = np.tile(parsed.offsets[k], (n, 1))
        R = np.tile(np.eye(3), (n, 1, 1))
        for name in parsed.channels[k]:
            v = parsed.motion[:, at]
            at += 1
            if name.endswith("position"):
                t[:, "XYZ".index(name[0])] += v
            else:
                R = R @ _axis_rotation(name[0], v)
        p = parsed.parents[k]
        if p < 0:
            pos[:, k], G[:, k] = t, R
        else:
            if p >= k:
                raise ValueError("a node before its parent")
            pos[:, k] = pos[:, p] + np.einsum("nij,nj->ni", G[:, p], t)
            G[:, k] = G[:, p] @ R
    return pos


def skeleton_from_nodes(positions):
    """Node positions [frames, 19, 3] (`joint_positions`) -> the 15 joints [frames, 15, 3]: every joint from the node that sits on it."""
    tab = tables()
    positions = np.asarray(positions)
    out = np.empty(positions.shape[:-2] + (15, 3), dtype=positions.dtype)
    for node, j in enumerate(tab.joint_of_node):
        if j >= 0:
            out[..., j, :] = positions[..., node, :]
    return out


# ------------------------------------------------------------------------------------------------------------------ a result's files
def write_result_bvh(engine, out_dir, estimated, optimized, gt=None, fps=DEFAULT_FPS, align=None, unit_scale=100.0, upright=None):
    """`estimated.bvh`, `optimized.bvh` and, with a ground truth, `gt.bvh` under `out_dir` from the merged sequences, by the convention of
    `report.Outputs`: with a ground truth the first two are aligned to it (`align`, default: whenever there is one).  upright: True or
    a `ground.GroundEstimate`: the files stand in the upright frame of the ground estimated from the foot contacts -- Y up, the floor at
    0, the wearer at the origin facing +Z in the first frame (`meshes._upright`).  Returns the number of files."""
    align = gt is not None if align is None else align
    if align and gt is None:
        raise ValueError("aligned BVH files need a ground-truth sequence to align to")
    to = gt if align else None
    move, move_gt = _upright(engine, upright, align, optimized, gt)
    extra, extra_gt = ({} if move is None else {"move": move}), ({} if move_gt is None else {"move": move_gt})
    os.makedirs(out_dir, exist_ok=True)
    write_bvh(engine, estimated, os.path.join(out_dir, FILE_NAMES[0]), fps=fps, align_to=to, unit_scale=unit_scale, **extra)
    write_bvh(engine, optimized, os.path.join(out_dir, FILE_NAMES[1]), fps=fps, align_to=to, unit_scale=unit_scale, **extra)
    if gt is not None:
        write_bvh(engine, gt, os.path.join(out_dir, FILE_NAMES[2]), fps=fps, unit_scale=unit_scale, **extra_gt)
    return 2 if gt is None else 3


def main(argv=None):
    import argparse
    truthy = lambda x: str(x).lower() == "true"          # noqa: E731  (the reference's own flag parser)
    p = argparse.ArgumentParser(description="BVH animation files from a saved result_pose.pkl")
    p.add_argument("pose_pickle", help="result_pose.pkl as --save_pose writes it: estimated_pose, optimized_pose and, optionally, gt_pose")
    p.add_argument("--out", required=True, metavar="DIR")
    p.add_argument("--fps", default=float(DEFAULT_FPS), type=float, help="frames per second of the files (Frame Time = 1 / fps)")
    p.add_argument("--align", default=False, type=truthy, help="true: align both sequences to gt_pose first")
    p.add_argument("--unit_scale", default=100.0, type=float, help="file units per metre (100: centimetres)")
    p.add_argument("--upright", action="store_true", help="stand the files upright on the ground estimated from the foot contacts: Y up, the floor at 0")
    p.add_argument("--foot_lock", action="store_true", help="pin the standing feet of the optimised sequence and re-solve its legs first")
    a = p.parse_args(argv)
    if not a.fps > 0:
        p.error("--fps must be positive")
    if not a.unit_scale > 0:
        p.error("--unit_scale must be positive")
    n = write_result_bvh(*result_poses(p, a, "the BVH files are made on the device"), fps=a.fps, align=a.align, unit_scale=a.unit_scale,
                         upright=a.upright or None)
    print("{} BVH files written under {}".format(n, a.out))


if __name__ == "__main__":
    main()
