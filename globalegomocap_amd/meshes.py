"""Skeleton meshes as PLY files: what the reference's `--save` writes (optimizer.py:485-504 -> save_mesh -> Skeleton.joints_2_mesh).

One file per frame -- 15 spheres of radius 0.02 m on the joints, 15 cylinders of radius 0.005 m along `skeleton.MESH_LINES`, binary
little-endian PLY as open3d's writer lays it out.  A file is 685 kB and only its vertex block depends on the
pose: the library builds header and face block once on the host (`constant`), a kernel builds the vertex blocks of all frames as
the bytes the files hold (`vertex_blocks`: gem_skeleton_mesh, optionally behind the similarity alignment of the whole sequence,
gem_sequence_align), and `write_meshes` moves them device -> pinned memory -> files with a pool of writer threads; Python touches
a frame once, to name its file.  `read_ply` reads such a file back.

    python -m globalegomocap_amd.meshes out/<dataset>/<chunk>/result_pose.pkl --out DIR [--align true]
"""
import ctypes as C
import os
import pickle
import re
from collections import namedtuple

import numpy as np

from . import _capi
from .skeleton import N_JOINTS

Layout = namedtuple("Layout", "vertices triangles header_bytes vertex_bytes face_bytes file_bytes")
PINNED_BYTES = 64 << 20          # each of the two pinned buffers the vertex blocks cross PCIe through (191 frames), whatever the sequence's length
MAX_WRITERS = 16
ALIGNED_DIRS = ("optimized_global_aligned", "input_global_aligned", "gt_global_aligned")          # optimizer.py:490-496
PLAIN_DIRS = ("optimized_global", "input_global", "gt_global")

_layout = None
_constant = None


def layout():
    """Counts and byte sizes of one mesh file (gem_skeleton_mesh_layout); needs no GPU."""
    global _layout
    if _layout is None:
        lib = _capi.load_library()
        out = (C.c_int64 * 6)()
        _capi.check(lib.gem_skeleton_mesh_layout(out), lib)
        _layout = Layout(*[int(v) for v in out])
    return _layout


def constant():
    """(header, face block) of every mesh file as bytes (gem_skeleton_mesh_constant); needs no GPU."""
    global _constant
    if _constant is None:
        lib, lay = _capi.load_library(), layout()
        header, faces = C.create_string_buffer(lay.header_bytes), C.create_string_buffer(lay.face_bytes)
        _capi.check(lib.gem_skeleton_mesh_constant(header, faces), lib)
        _constant = (header.raw, faces.raw)
    return _constant


def _sequence(engine, seq):
    import torch
    t = seq if torch.is_tensor(seq) else torch.from_numpy(np.array(seq, dtype=np.float64))          # (a copy: 360 bytes per frame)
    t = t.to(device=engine.device, dtype=torch.float64).contiguous()
    if t.dim() != 3 or tuple(t.shape[1:]) != (N_JOINTS, 3):
        raise ValueError("a pose sequence must be [F,%d,3], got %s" % (N_JOINTS, tuple(t.shape)))
    return t


def _alignment(engine, seq_d, align_to, move=None):
    """The (c, R, t) [13] on the device that the kernels apply to the joints, or None: the similarity onto `align_to`, then `move`
    (composed on the device, `ground.compose`)."""
    crt = None
    if align_to is not None:
        to_d = _sequence(engine, align_to)
        if to_d.shape != seq_d.shape:
            raise ValueError("align_to must have the sequence's shape %s, got %s" % (tuple(seq_d.shape), tuple(to_d.shape)))
        crt = engine.sequence_align(seq_d, to_d)
    if move is None:
        return crt
    import torch
    from ._binding import check_tensor
    from .ground import compose
    check_tensor(move, torch.float64, (13,), error=TypeError("move must be a contiguous float64 device tensor of 13 values (c, R, t)"))
    return move if crt is None else compose(engine, crt, move)


def _upright(engine, upright, aligned, optimized, gt):
    """The `move` of a `write_result_*` for its `upright` argument -> (for the estimated and the optimised sequence, for the ground
    truth).  True: ONE estimate for all sequences written -- of the ground truth where the other two are aligned to it, else of the
    optimised sequence; a ground truth the others are not aligned to lives in a frame of its own and is stood upright by its own."""
    if upright is None or upright is False:
        return None, None
    from .ground import resolve
    g = resolve(engine, upright, gt if aligned else optimized)
    if gt is None or aligned or upright is not True:
        return g.crt, g.crt
    return g.crt, resolve(engine, True, gt).crt


def vertex_blocks(engine, seq, align_to=None, move=None):
    """The vertex blocks of the meshes of `seq` [F,15,3] (array or tensor) as the files hold them: a uint8 device tensor
    [F, vertex_bytes].  align_to [F,15,3]: the sequence is first moved by the one similarity transform that takes it onto
    `align_to` (`errors.align_sequence`, the reference's global_align_skeleton_seq).  move: a [13] device tensor (c, R, t), for
    instance `GroundEstimate.crt`, applied behind the alignment.  Nothing synchronises."""
    seq_d = _sequence(engine, seq)
    return engine.skeleton_mesh(seq_d, _alignment(engine, seq_d, align_to, move))


def _write_file(path, parts):
    """One file from its parts (bytes-like), written with as few system calls as the kernel allows, closed when this returns."""
    parts = [memoryview(p).cast("B") for p in parts]
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
    try:
        while parts:
            n = os.writev(fd, parts)
            while parts and n >= len(parts[0]):
                n -= len(parts.pop(0))
            if parts and n:
                parts[0] = parts[0][n:]
    finally:
        os.close(fd)


def write_meshes(engine, seq, out_dir, align_to=None, pattern="out_%04d.ply", move=None):
    """`out_dir/pattern % f` for every frame f of `seq` [F,15,3] (the reference's save_mesh), `align_to` and `move` as in `vertex_blocks`.
    The vertex blocks are made on the device, at most PINNED_BYTES of them at a time, and go through `staging.stream_out` to the
    writer threads (at most MAX_WRITERS, on the CPUs near the device).  Runs on the current stream.  Every file is complete and closed when this
    returns; returns the number of files."""
    from .staging import cpus_near, reader_pool, stream_out
    seq_d = _sequence(engine, seq)
    crt = _alignment(engine, seq_d, align_to, move)
    os.makedirs(out_dir, exist_ok=True)
    F, lay = seq_d.shape[0], layout()
    if F == 0:
        return 0
    header, faces = constant()
    per = max(1, PINNED_BYTES // lay.vertex_bytes)
    pool = reader_pool("mesh", min(MAX_WRITERS, os.cpu_count() or 1), cpus_near(engine.device))

    def produce(k, out):
        n = min(per, F - k * per)
        engine.skeleton_mesh(seq_d[k * per:k * per + n], crt, out=out.view(per, lay.vertex_bytes)[:n])
        return n * lay.vertex_bytes

    def consume(k, data, side):
        rows = data.numpy().reshape(-1, lay.vertex_bytes)
        return (pool.submit(_write_file, os.path.join(out_dir, pattern % (k * per + i)), (header, rows[i], faces)) for i in range(len(rows)))

    stream_out(engine.device, "meshes", per * lay.vertex_bytes, (F + per - 1) // per, produce, consume)
    return F


def release():
    """Give back the pinned and device buffers `write_meshes` keeps between calls."""
    from .staging import release_kept
    release_kept("meshes")


_HEADER_RE = re.compile(rb"ply\nformat binary_little_endian 1\.0\ncomment [^\n]*\nelement vertex (\d+)\nproperty double x\nproperty double y\n"
                        rb"property double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face (\d+)\n"
                        rb"property list uchar uint vertex_indices\nend_header\n")


def read_ply(path):
    """A mesh file of this module's layout -> (vertices f64 [V,3], colours u8 [V,3], triangles u32 [T,3]).  Strict: binary
    little-endian PLY with exactly the properties `write_meshes` writes, in their order; the file must be as long as its header
    says, every face a triangle with indices below the vertex count.  ValueError otherwise."""
    with open(path, "rb") as f:
        data = f.read()
    m = _HEADER_RE.match(data)
    if m is None:
        raise ValueError("%s: not a binary little-endian PLY with the skeleton-mesh header (double x y z, uchar red green blue, "
                         "list uchar uint vertex_indices)" % path)
    V, T = int(m.group(1)), int(m.group(2))
    want = m.end() + 27 * V + 13 * T
    if len(data) != want:
        raise ValueError("%s: %d bytes, but its header announces %d vertices and %d faces = %d bytes" % (path, len(data), V, T, want))
    vert = np.frombuffer(data, dtype=np.dtype([("p", "<f8", 3), ("c", "u1", 3)]), count=V, offset=m.end())
    face = np.frombuffer(data, dtype=np.dtype([("n", "u1"), ("i", "<u4", 3)]), count=T, offset=m.end() + 27 * V)
    if T and (face["n"] != 3).any():
        raise ValueError("%s: a face that is no triangle" % path)
    if T and face["i"].max() >= V:
        raise ValueError("%s: a face names vertex %d of %d" % (path, int(face["i"].max()), V))
    return vert["p"].copy(), vert["c"].copy(), face["i"].astype(np.uint32)


def write_result_meshes(engine, out_dir, estimated, optimized, gt=None, align=None, upright=None):
    """The reference's three folders under `out_dir` (optimizer.py:486-504) from the merged sequences: the optimised and the
    estimated one aligned to the ground truth (`align`, default: whenever there is one), and the ground truth itself.  Without
    alignment the folders are called optimized_global / input_global (/ gt_global).  upright: True or a `ground.GroundEstimate`: all
    meshes stand in the upright frame of the ground estimated from the foot contacts (`_upright`)."""
    align = gt is not None if align is None else align
    if align and gt is None:
        raise ValueError("aligned meshes need a ground-truth sequence to align to")
    names = ALIGNED_DIRS if align else PLAIN_DIRS
    to = gt if align else None
    move, move_gt = _upright(engine, upright, align, optimized, gt)
    extra, extra_gt = ({} if move is None else {"move": move}), ({} if move_gt is None else {"move": move_gt})
    n = write_meshes(engine, optimized, os.path.join(out_dir, names[0]), align_to=to, **extra)
    n += write_meshes(engine, estimated, os.path.join(out_dir, names[1]), align_to=to, **extra)
    if gt is not None:
        n += write_meshes(engine, gt, os.path.join(out_dir, names[2]), **extra_gt)
    return n


def result_poses(p, a, why_a_device):
    """What the command lines of `meshes`, `render` and `bvh` do behind their parser `p`: `a.pose_pickle` loaded and checked (with
    `a.align`: it has a gt_pose), a device found and an engine made -> (engine, a.out, estimated, optimised, ground truth or None),
    the leading arguments of a `write_result_*`.  With `a.foot_lock` the optimised sequence is its foot-locked version
    (`foot_lock.lock_feet` at its defaults; the estimate's frame rate is `a.fps` where the parser has one)."""
    with open(a.pose_pickle, "rb") as f:
        d = pickle.load(f)
    for key in ("estimated_pose", "optimized_pose"):
        if key not in d:
            p.error("%s has no %s" % (a.pose_pickle, key))
    gt = d.get("gt_pose")
    if a.align and gt is None:
        p.error("--align true needs a gt_pose in %s" % a.pose_pickle)
    from .camera import DEFAULT_CALIBRATION
    from .prepare import _lift_engine
    import torch
    if not torch.cuda.is_available():
        raise _capi.GemError("no HIP device visible: " + why_a_device)
    engine, optimized = _lift_engine(DEFAULT_CALIBRATION, torch.cuda.current_device()), np.asarray(d["optimized_pose"])
    if getattr(a, "foot_lock", False):
        from . import foot_lock
        lock = foot_lock.lock_feet(engine, optimized, **({"fps": a.fps} if getattr(a, "fps", None) else {}))
        print(lock.line())
        optimized = lock.sequence
    return engine, a.out, np.asarray(d["estimated_pose"]), optimized, None if gt is None else np.asarray(gt)


def main(argv=None):
    import argparse
    truthy = lambda x: str(x).lower() == "true"          # noqa: E731  (the reference's own flag parser)
    p = argparse.ArgumentParser(description="Skeleton meshes (PLY, one per frame) from a saved result_pose.pkl")
    p.add_argument("pose_pickle", help="result_pose.pkl as --save_pose writes it: estimated_pose, optimized_pose and, optionally, gt_pose")
    p.add_argument("--out", required=True, metavar="DIR")
    p.add_argument("--align", default=False, type=truthy, help="true: align both sequences to gt_pose first (the reference's --save)")
    p.add_argument("--upright", action="store_true", help="stand the meshes upright on the ground estimated from the foot contacts")
    p.add_argument("--foot_lock", action="store_true", help="pin the standing feet of the optimised sequence and re-solve its legs first")
    a = p.parse_args(argv)
    n = write_result_meshes(*result_poses(p, a, "the meshes are built on the device"), align=a.align, upright=a.upright or None)
    print("{} meshes written under {}".format(n, a.out))


if __name__ == "__main__":
    main()
