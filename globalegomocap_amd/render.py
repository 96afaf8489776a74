"""Skeleton sequences as PNG frames, rendered on the device: something to look at without a mesh viewer.

A skeleton frame is 30 capsules -- the 15 joints as spheres of radius 0.02 m, the 15 lines of `skeleton.MESH_LINES` with radius
0.005 m, the meshes' figure -- drawn through one orthographic camera (`fit_view`: one view per call, shared by all frames and all
overlaid sequences, so the figure does not jump).  A kernel rasterises every image into the bytes a PNG holds before deflate
(`scanlines`: gem_skeleton_capsules + gem_render_capsules), and `write_frames` moves them device -> pinned memory -> files with the
writer threads `meshes.write_meshes` uses; the host only deflates (zlib, level 1) and frames them.  `write_frames` writes one
`frame_%04d.png` per frame with all given sequences overlaid and one `overview_<name>.png` per sequence with all its frames in one
scene -- what the reference's viewer shows first (optimizer.py:452-467).  `read_png` reads such a file back.

    python -m globalegomocap_amd.render out/<dataset>/<chunk>/result_pose.pkl --out DIR [--align true] [--size WxH] [--view side|front|top]

The camera's view is the picture from where the evidence lives: the frame's heat-maps, tinted, with the
sequences projected through the frame's camera by the reprojection term's own arithmetic and drawn flat on top (`camera_scanlines`:
gem_project_sequence + gem_render_camera; `write_camera_frames` writes one `camera_%04d.png` per frame by the same route).

    python -m globalegomocap_amd.render out/<dataset>/<chunk>/result_pose.pkl --out DIR --camera <chunk directory> [--size N]

Either set of frames can also become one clip that plays: `video=PATH` hands the same images to
`video.write_video`, which encodes them on the device as Motion-JPEG.

    python -m globalegomocap_amd.render result_pose.pkl --out DIR --video [--video_fps F] [--video_quality Q] [--no_frames]
"""
import ctypes as C
import os
import struct
import zlib
from collections import namedtuple

import numpy as np

from . import _capi
from .meshes import _alignment, _sequence, result_poses
from .skeleton import N_JOINTS
from .video import DEFAULT_FPS, DEFAULT_QUALITY

Layout = namedtuple("Layout", "row_bytes image_bytes stride")
PINNED_BYTES = 64 << 20          # each of the two pinned buffers the scanlines cross PCIe through (69 images of 640 x 480)
MAX_WRITERS = 16
VIEWS = ("side", "front", "top")
PALETTE = {"estimated": (214, 39, 40), "optimized": (31, 119, 180), "gt": (44, 160, 44)}
DEFAULT_SIZE = (640, 480)        # (width, height) wherever a caller gives none
CAMERA_SIZE = 512                # pixels each way of a camera view wherever a caller gives none
HEAT_COLOUR = (148, 103, 189)    # the background's colour where the heat-maps say 1
MARGIN = 0.1                     # metres around the joints' bounding box
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def layout(width, height):
    """Row bytes, image bytes and image stride of a width x height image (gem_render_layout); needs no GPU."""
    lib = _capi.load_library()
    out = (C.c_int64 * 3)()
    _capi.check(lib.gem_render_layout(int(width), int(height), out), lib)
    return Layout(*[int(v) for v in out])


def _host(seq):
    a = seq.detach().cpu().numpy() if hasattr(seq, "detach") else np.asarray(seq)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 3 or a.shape[1:] != (N_JOINTS, 3):
        raise ValueError("a pose sequence must be [F,%d,3], got %s" % (N_JOINTS, a.shape))
    return a


def fit_view(sequences, width, height, view="side"):
    """The orthographic camera (`_capi.GemView`) that shows every joint of `sequences` (arrays [F,15,3]) in a width x height image.
    `up` is the normalised mean over all frames of neck - (right foot + left foot) / 2 -- (0,-1,0) when that is shorter than
    1e-6 -- and `down` = -up.  "side" looks along the world axis that is most nearly level (smallest |e . up|, the lowest index
    on ties), made orthogonal to up; "front" along that vector turned by 90 degrees about up; "top" looks along `down`, with the
    side vector as the image's down.  right = down x forward.  The centre is the middle of the joints' bounding box in view
    coordinates; half_width the larger of its half extent in x and its half extent in y times W / H, plus 0.1 m.  numpy, no GPU."""
    if view not in VIEWS:
        raise ValueError("view must be one of %s, got %r" % (", ".join(VIEWS), view))
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("an image needs at least one pixel each way, got %d x %d" % (width, height))
    pts = np.concatenate([_host(s) for s in sequences], axis=0)
    if pts.shape[0] == 0:
        raise ValueError("no frame to fit a view to")
    up = (pts[:, 0] - 0.5 * (pts[:, 10] + pts[:, 14])).mean(axis=0)
    n = np.linalg.norm(up)
    up = up / n if n >= 1e-6 else np.array([0.0, -1.0, 0.0])
    e = np.eye(3)[int(np.argmin(np.abs(up)))]          # (argmin: the lowest index on ties)
    side = e - (e @ up) * up
    side /= np.linalg.norm(side)
    if view == "side":
        down, forward = -up, side
    elif view == "front":
        down, forward = -up, np.cross(up, side)
    else:
        down, forward = side, -up
    right = np.cross(down, forward)
    axes = np.stack([right, down, forward])
    q = pts.reshape(-1, 3) @ axes.T
    lo, hi = q.min(axis=0), q.max(axis=0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    v = _capi.GemView()
    for name, vec in (("right", right), ("down", down), ("forward", forward), ("centre", mid @ axes)):
        for i in range(3):
            getattr(v, name)[i] = float(vec[i])
    v.half_width = float(max(half[0], half[1] * width / height) + MARGIN)
    v.width, v.height = width, height
    return v


def _prepare(engine, sequences, align_to, move=None):
    """The sequences on the device and, per sequence, the similarity (`WindowEngine.sequence_align`, [13] on the device) onto its
    entry of `align_to`: None, one sequence for all, or a list with a sequence or None for each.  move: None, one [13] device tensor
    for all or a list with one or None for each, applied behind the alignment."""
    seqs = [_sequence(engine, s) for s in sequences]
    if not seqs:
        raise ValueError("no sequence to draw")
    if any(s.shape != seqs[0].shape for s in seqs):
        raise ValueError("overlaid sequences must have the same number of frames, got %s" % [tuple(s.shape) for s in seqs])
    targets = list(align_to) if isinstance(align_to, (list, tuple)) else [align_to] * len(seqs)
    if len(targets) != len(seqs):
        raise ValueError("align_to lists %d targets for %d sequences" % (len(targets), len(seqs)))
    if move is None:
        return seqs, [_alignment(engine, s, to) for s, to in zip(seqs, targets)]
    moves = list(move) if isinstance(move, (list, tuple)) else [move] * len(seqs)
    if len(moves) != len(seqs):
        raise ValueError("move lists %d transforms for %d sequences" % (len(moves), len(seqs)))
    return seqs, [_alignment(engine, s, to, m) for s, to, m in zip(seqs, targets, moves)]


def frames_view(engine, sequences, align_to=None, size=None, view="side"):
    """The view `write_frames` draws these sequences through: `fit_view` of the sequences as drawn, that is behind their alignment."""
    seqs, crts = _prepare(engine, sequences, align_to)
    return _view_of(seqs, crts, size, view)


def _view_of(seqs, crts, size, view):
    size = DEFAULT_SIZE if size is None else size
    drawn = []
    for s, crt in zip(seqs, crts):
        p = s.cpu().numpy()
        if crt is not None:          # c * (p . R) + t, as the kernel moves the joints
            k = crt.cpu().numpy()
            p = k[0] * (p @ k[1:10].reshape(3, 3)) + k[10:13]
        drawn.append(p)
    return fit_view(drawn, size[0], size[1], view)


def _rgb_word(c):
    r, g, b = (int(x) for x in c)
    if not all(0 <= x <= 255 for x in (r, g, b)):
        raise ValueError("a colour is three integers 0 .. 255, got %r" % (c,))
    return r | (g << 8) | (b << 16)


def _scene(engine, seqs, crts, colours, overview):
    """(geometry, colours, first) of the images: per frame the capsules of all sequences, or per sequence those of all its frames."""
    import torch
    if len(colours) != len(seqs):
        raise ValueError("%d colours for %d sequences" % (len(colours), len(seqs)))
    S, F = len(seqs), seqs[0].shape[0]
    parts = [engine.skeleton_capsules(s, crt, _rgb_word(c), _rgb_word(c)) for s, crt, c in zip(seqs, crts, colours)]
    geom = torch.stack([p[0].view(F, 30, 7) for p in parts])          # [S,F,30,7]
    rgb = torch.stack([p[1].view(F, 30) for p in parts])
    if overview:
        n, per = S, F * 30
    else:
        geom, rgb = geom.permute(1, 0, 2, 3), rgb.permute(1, 0, 2)
        n, per = F, S * 30
    first = torch.arange(n + 1, dtype=torch.int32) * per
    return geom.reshape(-1, 7).contiguous(), rgb.reshape(-1).contiguous(), first.to(engine.device)


def scanlines(engine, sequences, view, colours, overview=False, align_to=None):
    """The images of `sequences` (each [F,15,3], array or tensor; one RGB colour each) through `view`, as the bytes their PNG files
    hold before deflate: a uint8 device tensor [n, stride], an image's bytes first in its row (`layout`).  One image per frame with
    all sequences overlaid, or (overview=True) one per sequence with all its frames.  align_to: see `write_frames`."""
    seqs, crts = _prepare(engine, sequences, align_to)
    geom, rgb, first = _scene(engine, seqs, crts, colours, overview)
    return engine.render_capsules(geom, rgb, first, view)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, scanline_bytes, width, height):
    """An 8-bit RGB, non-interlaced PNG from its scanline stream (height rows of filter byte 0 + 3 * width bytes): IHDR, one IDAT
    (zlib level 1), IEND.  Standard library only; zlib releases the GIL while it deflates."""
    data = memoryview(scanline_bytes).cast("B")
    if len(data) != height * (1 + 3 * width):
        raise ValueError("%d x %d pixels are %d scanline bytes, got %d" % (width, height, height * (1 + 3 * width), len(data)))
    body = PNG_SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)) + \
        _chunk(b"IDAT", zlib.compress(data, 1)) + _chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(body)


def read_png(path):
    """A PNG of this module's making -> uint8 [H,W,3].  Strict: the signature, then exactly IHDR, one IDAT and IEND with good CRCs
    and nothing behind them; 8-bit RGB, not interlaced; the inflated stream as long as the header says, every filter byte 0.
    ValueError otherwise."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != PNG_SIGNATURE:
        raise ValueError("%s: no PNG signature" % path)
    at, chunks = 8, []
    while at < len(data):
        if at + 12 > len(data):
            raise ValueError("%s: truncated inside a chunk header" % path)
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        if at + 12 + n > len(data):
            raise ValueError("%s: truncated inside its %s chunk" % (path, kind.decode("latin-1")))
        body = data[at + 8:at + 8 + n]
        if struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != zlib.crc32(kind + body) & 0xFFFFFFFF:
            raise ValueError("%s: bad CRC in its %s chunk" % (path, kind.decode("latin-1")))
        chunks.append((kind, body))
        at += 12 + n
    if [k for k, _ in chunks] != [b"IHDR", b"IDAT", b"IEND"] or len(chunks[0][1]) != 13 or chunks[2][1]:
        raise ValueError("%s: not exactly IHDR, one IDAT, IEND (got %s)" % (path, b" ".join(k for k, _ in chunks).decode("latin-1")))
    W, H, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    if (depth, colour, compression, filt, interlace) != (8, 2, 0, 0, 0) or W < 1 or H < 1:
        raise ValueError("%s: not an 8-bit RGB, non-interlaced image (bit depth %d, colour type %d, interlace %d)" % (path, depth, colour, interlace))
    try:
        raw = zlib.decompress(chunks[1][1])
    except zlib.error as e:
        raise ValueError("%s: its IDAT does not inflate: %s" % (path, e))
    if len(raw) != H * (1 + 3 * W):
        raise ValueError("%s: %d scanline bytes for %d x %d pixels" % (path, len(raw), W, H))
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + 3 * W)
    if rows[:, 0].any():
        raise ValueError("%s: a scanline with a filter other than 0" % path)
    return rows[:, 1:].reshape(H, W, 3).copy()


def _write_images(engine, geom, rgb, first, view, paths):
    """Image i of the scene -> paths[i] (`_write_scanlines`)."""
    _write_scanlines(engine, lambda lo, n, out: engine.render_capsules(geom, rgb, first[lo:lo + n + 1], view, out=out), view.width, view.height, paths)


def _write_scanlines(engine, draw, W, H, paths):
    """Image i -> paths[i], W x H pixels each; `draw(lo, n, out)` renders the images lo .. lo + n into the rows of `out`.  The
    scanlines are made on the device, at most PINNED_BYTES of them at a time, and go through `staging.stream_out` to the meshes'
    writer threads, which deflate and write them.  Every file is complete and closed when this returns."""
    from .staging import cpus_near, reader_pool, stream_out
    n_images = len(paths)
    if n_images == 0:
        return
    lay = layout(W, H)
    per = max(1, PINNED_BYTES // lay.stride)
    pool = reader_pool("mesh", min(MAX_WRITERS, os.cpu_count() or 1), cpus_near(engine.device))          # (the meshes' writer threads)

    def produce(k, out):
        n = min(per, n_images - k * per)
        draw(k * per, n, out.view(per, lay.stride)[:n])
        return n * lay.stride

    def consume(k, data, side):
        rows = data.numpy().reshape(-1, lay.stride)
        return (pool.submit(write_png, paths[k * per + i], rows[i, :lay.image_bytes], W, H) for i in range(len(rows)))

    stream_out(engine.device, "render", per * lay.stride, (n_images + per - 1) // per, produce, consume)


def _video_arguments(video, video_fps, video_quality, frames):
    """What `write_frames` / `write_camera_frames` refuse before they draw anything."""
    if video is None:
        if not frames:
            raise ValueError("frames=False leaves nothing to write: it needs video=PATH")
        return
    from .video import check_options
    check_options(video_fps, video_quality)


def write_frames(engine, sequences, out_dir, colours=None, align_to=None, size=None, view="side", overview=True, names=None, video=None,
                 video_fps=DEFAULT_FPS, video_quality=DEFAULT_QUALITY, frames=True, move=None):
    """`out_dir/frame_%04d.png` for every frame, all `sequences` (each [F,15,3]) overlaid in their `colours` (default: the palette's
    order estimated, optimised, ground truth), and -- overview=True -- `out_dir/overview_<name>.png` per sequence with all its
    frames in one scene (`names`, default: the palette's names).  align_to: None, one sequence [F,15,3] for all, or a list with one
    target or None per sequence; a sequence with a target is first moved by the one similarity transform that takes it onto the
    target (`errors.align_sequence`).  size = (width, height), default DEFAULT_SIZE; `view` as in `fit_view`, fitted once to everything that is drawn.
    video=PATH additionally writes the per-frame images -- not the overviews -- as one Motion-JPEG clip to PATH at `video_fps` frames
    per second and JPEG quality `video_quality` (`video.write_video`: encoded on the device); with
    frames=False no PNG file is written, and `out_dir` is not touched.  move: a [13] device tensor (c, R, t), for instance
    `GroundEstimate.crt`, or a list with one or None per sequence, applied behind the alignment.
    Runs on the current stream; every file is complete and closed on return; returns the number of files."""
    _video_arguments(video, video_fps, video_quality, frames)
    seqs, crts = _prepare(engine, sequences, align_to, move)
    S, F = len(seqs), seqs[0].shape[0]
    default = list(PALETTE)
    if colours is None:
        if S > len(default):
            raise ValueError("more than %d sequences need their colours given" % len(default))
        colours = [PALETTE[k] for k in default[:S]]
    if names is None:
        names = default[:S] if S <= len(default) else ["%d" % i for i in range(S)]
    if len(names) != S:
        raise ValueError("%d names for %d sequences" % (len(names), S))
    if frames:
        os.makedirs(out_dir, exist_ok=True)
    if F == 0:
        return 0
    v = _view_of(seqs, crts, size, view)
    geom, rgb, first = _scene(engine, seqs, crts, colours, False)
    if video is not None:
        from .video import write_video
        write_video(engine, lambda lo, n, out: engine.render_capsules(geom, rgb, first[lo:lo + n + 1], v, out=out), v.width, v.height, F,
                    video, video_fps, video_quality)
        if not frames:
            return 1
    _write_images(engine, geom, rgb, first, v, [os.path.join(out_dir, "frame_%04d.png" % f) for f in range(F)])
    if not overview:
        return F + (video is not None)
    geom, rgb, first = _scene(engine, seqs, crts, colours, True)
    _write_images(engine, geom, rgb, first, v, [os.path.join(out_dir, "overview_%s.png" % n) for n in names])
    return F + S + (video is not None)


def write_result_frames(engine, out_dir, estimated, optimized, gt=None, align=None, size=None, view="side", video=None, video_fps=DEFAULT_FPS,
                        video_quality=DEFAULT_QUALITY, frames=True, upright=None):
    """One result's frames under `out_dir`: the estimated, the optimised and, where there is one, the ground-truth sequence overlaid
    (red, blue, green), the first two aligned to the third (`align`, default: whenever there is one) as `meshes.write_result_meshes`
    aligns the meshes.  video, video_fps, video_quality, frames: see `write_frames`.  upright: True or a `ground.GroundEstimate`: the
    sequences are drawn in the upright frame of the ground estimated from the foot contacts (`meshes._upright`)."""
    align = gt is not None if align is None else align
    if align and gt is None:
        raise ValueError("aligned frames need a ground-truth sequence to align to")
    sequences = [estimated, optimized] + ([gt] if gt is not None else [])
    to = [gt if align else None] * 2 + ([None] if gt is not None else [])
    from .meshes import _upright
    move, move_gt = _upright(engine, upright, align, optimized, gt)
    extra = {} if move is None else {"move": [move, move] + ([move_gt] if gt is not None else [])}
    return write_frames(engine, sequences, out_dir, align_to=to, size=size, view=view, video=video, video_fps=video_fps,
                        video_quality=video_quality, frames=frames, **extra)


# ------------------------------------------------------------------------------------------------------------------ the camera's view
def camera_view(size=None, joint_radius=8.0, line_radius=3.0, heat_joints=None, heat_colour=HEAT_COLOUR):
    """The `_capi.GemCameraView` of size x size pixels (default CAMERA_SIZE) over the 1024 x 1024 crop the heat-maps cover: radii in
    pixels of the 1280 x 1024 image, `heat_joints` the joints whose heat-maps make the background (default: all), tinted
    `heat_colour`.  Needs no GPU."""
    size = CAMERA_SIZE if size is None else int(size)
    if not 1 <= size <= 1024:
        raise ValueError("a camera view is 1 .. 1024 pixels each way, got %d" % size)
    joints = range(N_JOINTS) if heat_joints is None else [int(j) for j in heat_joints]
    if not all(0 <= j < N_JOINTS for j in joints):
        raise ValueError("heat_joints are joint indices 0 .. %d, got %r" % (N_JOINTS - 1, list(joints)))
    for r in (joint_radius, line_radius):
        if not (np.isfinite(r) and r >= 0):
            raise ValueError("a radius is a finite number of pixels, not negative; got %r" % (r,))
    v = _capi.GemCameraView()
    v.size, v.joint_mask, v.rgb_heat, v.reserved = size, sum({1 << j for j in joints}), _rgb_word(heat_colour), 0
    v.joint_radius, v.line_radius = float(joint_radius), float(line_radius)
    return v


def _camera_scene(engine, sequences, cams, heat, colours, align_to):
    """What `gem_render_camera` reads, on the device: the heat-maps [F,H,W,15] (or None), the image points [S,F,15,2] of the
    global-frame sequences seen through `cams` [F,4,4], and the sequences' colour words."""
    import torch
    seqs, crts = _prepare(engine, sequences, align_to)
    if len(colours) != len(seqs):
        raise ValueError("%d colours for %d sequences" % (len(colours), len(seqs)))
    F = seqs[0].shape[0]
    cams_d = (cams if torch.is_tensor(cams) else torch.from_numpy(np.array(cams, dtype=np.float64))).to(device=engine.device, dtype=torch.float64).contiguous()
    if tuple(cams_d.shape) != (F, 4, 4):
        raise ValueError("the cameras must be [%d,4,4], one per frame, got %s" % (F, tuple(cams_d.shape)))
    if heat is not None:
        heat = (heat if torch.is_tensor(heat) else torch.from_numpy(np.array(heat, dtype=np.float32))).to(device=engine.device, dtype=torch.float32).contiguous()
        if heat.dim() != 4 or heat.shape[0] != F:
            raise ValueError("the heat-maps must be [%d,H,W,%d], one set per frame, got %s" % (F, N_JOINTS, tuple(heat.shape)))
    uv = torch.stack([engine.project_sequence(s, cams_d, crt) for s, crt in zip(seqs, crts)])
    rgb = torch.tensor([_rgb_word(c) for c in colours], dtype=torch.int32).to(engine.device)
    return heat, uv, rgb


def camera_scanlines(engine, sequences, cams, heat, colours, size=None, joint_radius=8.0, line_radius=3.0, heat_joints=None, align_to=None):
    """The camera's view of every frame: `heat` [F,H,W,15] (or None: white) tinted under the `sequences` (each
    [F,15,3] in the frame the cameras `cams` [F,4,4] live in; one RGB colour each, a later sequence over an earlier one), projected
    with the reprojection term's arithmetic, as the bytes their PNG files hold before deflate: a uint8 device tensor [F, stride]
    (`layout(size, size)`).  Further arguments: `camera_view`; align_to: see `write_frames`."""
    heat, uv, rgb = _camera_scene(engine, sequences, cams, heat, colours, align_to)
    return engine.render_camera(heat, uv, rgb, camera_view(size, joint_radius, line_radius, heat_joints))


def write_camera_frames(engine, sequences, cams, heat, out_dir, colours=None, size=None, joint_radius=8.0, line_radius=3.0, heat_joints=None,
                        align_to=None, video=None, video_fps=DEFAULT_FPS, video_quality=DEFAULT_QUALITY, frames=True):
    """`out_dir/camera_%04d.png` for every frame: `camera_scanlines` (colours default: the palette's order) through `write_frames`'
    pinned buffers and writer threads.  video, video_fps, video_quality, frames: as in `write_frames`, the same images as one clip.
    Runs on the current stream; every file is complete and closed on return; returns the number of files."""
    _video_arguments(video, video_fps, video_quality, frames)
    default = list(PALETTE)
    if colours is None:
        if len(sequences) > len(default):
            raise ValueError("more than %d sequences need their colours given" % len(default))
        colours = [PALETTE[k] for k in default[:len(sequences)]]
    heat, uv, rgb = _camera_scene(engine, sequences, cams, heat, colours, align_to)
    view = camera_view(size, joint_radius, line_radius, heat_joints)
    if frames:
        os.makedirs(out_dir, exist_ok=True)
    F = uv.shape[1]

    def draw(lo, n, out):
        engine.render_camera(None if heat is None else heat[lo:lo + n], uv[:, lo:lo + n].contiguous(), rgb, view, out=out)
    if video is not None and F:
        from .video import write_video
        write_video(engine, draw, view.size, view.size, F, video, video_fps, video_quality)
        if not frames:
            return 1
    _write_scanlines(engine, draw, view.size, view.size, [os.path.join(out_dir, "camera_%04d.png" % f) for f in range(F)])
    return F + (video is not None and F > 0)


def write_result_camera_frames(engine, out_dir, estimated, optimized, cams, heat, gt=None, size=None, video=None, video_fps=DEFAULT_FPS,
                               video_quality=DEFAULT_QUALITY, frames=True):
    """One result as the camera saw it, `out_dir/camera_%04d.png`: the estimated (red), the optimised (blue) and, where there is one,
    the ground-truth sequence (green) over the frames' heat-maps.  The ground truth lives in the studio's frame, not in the
    cameras': it is first moved by the one similarity that takes it onto the optimised sequence.  video, video_fps, video_quality,
    frames: see `write_frames`."""
    sequences = [estimated, optimized] + ([gt] if gt is not None else [])
    to = [None, None] + ([optimized] if gt is not None else [])
    return write_camera_frames(engine, sequences, cams, heat, out_dir, align_to=to, size=size, video=video, video_fps=video_fps,
                               video_quality=video_quality, frames=frames)


def release():
    """Give back the pinned and device buffers `write_frames` keeps between calls."""
    from .staging import release_kept
    release_kept("render")


def _size(text):
    try:
        w, h = (int(x) for x in str(text).lower().split("x"))
    except ValueError:
        w = h = 0
    if w < 1 or h < 1:
        import argparse
        raise argparse.ArgumentTypeError("a size is WIDTHxHEIGHT, for instance 640x480; got %r" % text)
    return w, h


def _size_or_side(text):
    """`--size`: WIDTHxHEIGHT (a pair) or, for `--camera`, one number of pixels (an int)."""
    try:
        n = int(str(text))
    except ValueError:
        return _size(text)
    if n < 1:
        import argparse
        raise argparse.ArgumentTypeError("a size is WIDTHxHEIGHT, for instance 640x480, or with --camera one number 1 .. 1024; got %r" % text)
    return n


def main(argv=None):
    import argparse
    truthy = lambda x: str(x).lower() == "true"          # noqa: E731  (the reference's own flag parser)
    p = argparse.ArgumentParser(description="Skeleton frames (PNG, one per frame, and one overview per sequence) from a saved result_pose.pkl")
    p.add_argument("pose_pickle", help="result_pose.pkl as --save_pose writes it: estimated_pose, optimized_pose and, optionally, gt_pose")
    p.add_argument("--out", required=True, metavar="DIR")
    p.add_argument("--align", default=False, type=truthy, help="true: align both sequences to gt_pose first")
    p.add_argument("--size", default=None, type=_size_or_side, metavar="WxH", help="default 640x480; with --camera one number N (default 512)")
    p.add_argument("--view", default="side", choices=VIEWS)
    p.add_argument("--camera", default=None, metavar="CHUNK_DIR",
                   help="draw the camera's view instead (camera_%%04d.png): the directory whose test_data.pkl holds the cameras and "
                        "heat-maps the poses belong to (merged frame f is the chunk's frame f); gt_pose is aligned onto optimized_pose")
    p.add_argument("--video", action="store_true", help="also write the frames as one Motion-JPEG clip, DIR/frames.avi (with --camera: DIR/camera.avi)")
    p.add_argument("--video_fps", default=float(DEFAULT_FPS), type=float, metavar="F", help="frames per second of the clip (default 25)")
    p.add_argument("--video_quality", default=DEFAULT_QUALITY, type=int, metavar="Q", help="JPEG quality of the clip, 1 .. 100 (default 90)")
    p.add_argument("--no_frames", action="store_true", help="with --video: the clip only, no PNG files")
    p.add_argument("--upright", action="store_true", help="draw the sequences upright on the ground estimated from the foot contacts (not with --camera)")
    p.add_argument("--foot_lock", action="store_true", help="pin the standing feet of the optimised sequence and re-solve its legs first (not with --camera)")
    a = p.parse_args(argv)
    if not a.video_fps > 0:
        p.error("argument --video_fps: must be positive")
    if not 1 <= a.video_quality <= 100:
        p.error("argument --video_quality: a whole number 1 .. 100")
    if a.no_frames and not a.video:
        p.error("--no_frames needs --video")
    clip = dict(video=os.path.join(a.out, "camera.avi" if a.camera is not None else "frames.avi") if a.video else None,
                video_fps=a.video_fps, video_quality=a.video_quality, frames=not a.no_frames)
    if a.camera is None and isinstance(a.size, int):
        p.error("argument --size: a size is WIDTHxHEIGHT, for instance 640x480; got %r" % str(a.size))
    if a.camera is not None and a.upright:
        p.error("--upright: the camera's view is the camera's own image and is not stood upright")
    if a.camera is not None and a.foot_lock:
        p.error("--foot_lock: the camera's view shows the optimiser's own result")
    if a.camera is not None:
        if isinstance(a.size, tuple) or (a.size is not None and a.size > 1024):
            p.error("argument --size: with --camera a size is one number of pixels 1 .. 1024")
        if not os.path.isfile(os.path.join(a.camera, "test_data.pkl")):
            p.error("--camera %s: no test_data.pkl in that directory" % a.camera)
    engine, out, est, opt, gt = result_poses(p, a, "the frames are rendered on the device")
    if a.camera is not None:
        from .whole_sequence import parse_chunk
        c = parse_chunk(a.camera, native=False, ground_truth=False)
        F = len(est)
        if c["n"] < F or len(c["cams"]) < F:
            p.error("--camera %s holds %d frames, the poses %d" % (a.camera, min(c["n"], len(c["cams"])), F))
        heat = np.asarray(c["heat_list"][:F], dtype=np.float32).reshape((F,) + tuple(c["heat_shape"]))
        n = write_result_camera_frames(engine, out, est, opt, c["cams"][:F], heat, gt, size=a.size, **clip)
    else:
        n = write_result_frames(engine, out, est, opt, gt, align=a.align, size=DEFAULT_SIZE if a.size is None else a.size, view=a.view,
                                upright=a.upright or None, **clip)
    print("{} {} written under {}".format(n, "files" if a.video else "images", a.out))


if __name__ == "__main__":
    main()
