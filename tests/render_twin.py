"""numpy float64 twin of the capsule rasteriser, written from the definition there: a loop over the capsules
of an image, every step of "Hit" and "Shade" spelt out with vectors (cross products against the unit axis, the line starting at
the depth of the capsule's first end), the pixels of an image side by side in arrays.  Besides id, depth and colour it reports,
per pixel, how close the pixel is to a decision that float64 rounding could turn: `near_silhouette`, `near_tie`, `near_round`.
And a PNG reader of its own (any filter type, any number of IDAT chunks)."""
import struct
import zlib
from types import SimpleNamespace

import numpy as np

LINES = [(0, 1), (0, 4), (1, 2), (2, 3), (4, 5), (5, 6), (1, 7), (4, 11), (7, 8), (8, 9), (9, 10), (11, 12), (12, 13), (13, 14), (7, 11)]
JOINT_R, LINE_R = 0.02, 0.005
CLOSE = 1e-7            # metres: silhouettes and ties nearer than this are not compared
ROUND_CLOSE = 1e-6      # levels: c * L + 0.5 nearer than this to an integer may round either way
PARALLEL = 1e-24        # sin^2 of the angle between axis and forward at which the axis counts as parallel


def view_of(v):
    """A gem_view (the ctypes mirror) as plain numpy."""
    return SimpleNamespace(right=np.array(list(v.right)), down=np.array(list(v.down)), forward=np.array(list(v.forward)),
                           centre=np.array(list(v.centre)), half_width=float(v.half_width), width=int(v.width), height=int(v.height))


def frame_capsules(pose, colour, crt=None):
    """The 30 capsules (a, b, r, colour) of one frame [15,3]: the joints, then the lines.  crt = (c, R, t): p -> c * (p @ R) + t."""
    pose = np.asarray(pose, dtype=np.float64)
    if crt is not None:
        pose = crt[0] * (pose @ crt[1]) + crt[2]
    caps = [(pose[j], pose[j], JOINT_R, tuple(colour)) for j in range(15)]
    caps += [(pose[a], pose[b], LINE_R, tuple(colour)) for a, b in LINES]
    return caps


def pixel_grid(view):
    W, H = view.width, view.height
    s = 2.0 * view.half_width / W
    u = (np.arange(W) + 0.5 - W / 2) * s
    v = (np.arange(H) + 0.5 - H / 2) * s
    return np.broadcast_to(u[None, :], (H, W)).copy(), np.broadcast_to(v[:, None], (H, W)).copy()


def _sphere(u, v, c, r):
    """Entry of the lines (u, v, .) into the sphere about c: (hit, t, n)."""
    px, py = u - c[0], v - c[1]
    h2 = r * r - (px * px + py * py)
    hit = h2 >= 0
    h = np.sqrt(np.where(hit, h2, 0.0))
    n = np.stack([px, py, -h], axis=-1)
    return hit, c[2] - h, n


def capsule_hit(u, v, a, b, r):
    """Per pixel: (hit, t, n) of the capsule a-b, r in view coordinates; n from the closest point of the segment to the hit."""
    f = np.array([0.0, 0.0, 1.0])
    d = b - a
    length = np.sqrt(d @ d)
    if length == 0.0:
        return _sphere(u, v, a, r)
    dh = d / length
    fxd = np.cross(f, dh)
    A = fxd @ fxd
    if A <= PARALLEL:
        return _sphere(u, v, a if a[2] <= b[2] else b, r)
    # the line o + t' f with o = (u, v, a_z): w = o - a
    w = np.stack([u - a[0], v - a[1], np.zeros_like(u)], axis=-1)
    wxd = np.cross(w, dh)
    B = wxd @ fxd
    C = (wxd * wxd).sum(-1) - r * r
    disc = B * B - A * C
    inside_cyl = disc >= 0
    tp = (-B - np.sqrt(np.where(inside_cyl, disc, 0.0))) / A
    p = w + tp[..., None] * f
    s = (p @ dh) / length
    body = inside_cyl & (s > 0) & (s < 1)
    n_body = p - (s * length)[..., None] * dh
    hit_a, t_a, n_a = _sphere(u, v, a, r)
    hit_b, t_b, n_b = _sphere(u, v, b, r)
    at_a, at_b = inside_cyl & (s <= 0), inside_cyl & (s >= 1)
    hit = body | (at_a & hit_a) | (at_b & hit_b)
    t = np.where(body, a[2] + tp, np.where(at_a, t_a, t_b))
    n = np.where(body[..., None], n_body, np.where(at_a[..., None], n_a, n_b))
    return hit, t, n


def clearance(u, v, a, b, r):
    """Distance of the lines (u, v, .) to the segment a-b, minus r."""
    d = b[:2] - a[:2]
    dd = d @ d
    px, py = u - a[0], v - a[1]
    s = np.clip((px * d[0] + py * d[1]) / dd, 0.0, 1.0) if dd > 0 else np.zeros_like(u)
    return np.hypot(px - s * d[0], py - s * d[1]) - r


def render(caps, view):
    """One image of the capsules `caps` (a, b, r, colour in world coordinates): a namespace of [H,W] arrays ids (-1: background),
    depth (inf), rgb [H,W,3] uint8, and the flags near_silhouette, near_tie, near_round."""
    W, H = view.width, view.height
    u, v = pixel_grid(view)
    axes = np.stack([view.right, view.down, view.forward])
    ids = np.full((H, W), -1, dtype=np.int32)
    depth = np.full((H, W), np.inf)
    second = np.full((H, W), np.inf)
    normal = np.zeros((H, W, 3))
    colour = np.zeros((H, W, 3))
    near_silhouette = np.zeros((H, W), dtype=bool)
    for k, (a, b, r, c) in enumerate(caps):
        av, bv = axes @ (np.asarray(a) - view.centre), axes @ (np.asarray(b) - view.centre)
        near_silhouette |= np.abs(clearance(u, v, av, bv, r)) < CLOSE
        hit, t, n = capsule_hit(u, v, av, bv, r)
        t = np.where(hit, t, np.inf)
        better = t < depth          # (strictly: on equal t the lower index stays)
        second = np.where(better, depth, np.minimum(second, t))
        ids[better] = k
        depth = np.where(better, t, depth)
        normal[better] = n[better]
        colour[better] = c
    covered = ids >= 0
    length = np.sqrt((normal * normal).sum(-1))
    L = 0.3 + 0.7 * np.maximum(0.0, -normal[..., 2] / np.where(covered, length, 1.0))
    x = colour * L[..., None] + 0.5
    rgb = np.where(covered[..., None], np.floor(x), 255.0).astype(np.uint8)
    near_round = covered & (np.abs(x - np.round(x)) < ROUND_CLOSE).any(-1)
    near_tie = covered & (np.where(covered, second, np.inf) - np.where(covered, depth, 0.0) < CLOSE)
    return SimpleNamespace(ids=ids, depth=depth, rgb=rgb, covered=covered, near_silhouette=near_silhouette, near_tie=near_tie,
                           near_round=near_round)


def scanline_bytes(rgb):
    """[H,W,3] uint8 -> the PNG scanline stream [H, 1 + 3 W] with filter bytes 0."""
    H, W, _ = rgb.shape
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)
    rows[:, 1:] = rgb.reshape(H, 3 * W)
    return rows


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def read_png(path):
    """An 8-bit RGB or RGBA, non-interlaced PNG -> uint8 [H,W,channels], by the PNG specification: any chunk order it allows, the
    IDAT chunks concatenated, every CRC checked, all five filter types."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "signature"
    at, idat, header, ended = 8, b"", None, False
    while at < len(data):
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        assert len(body) == n and struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        elif kind == b"IEND":
            ended = True
        at += 12 + n
    assert header is not None and ended
    W, H, bits, colour, _, _, interlace = header
    assert bits == 8 and colour in (2, 6) and interlace == 0, header
    ch = 3 if colour == 2 else 4
    raw = zlib.decompress(idat)
    assert len(raw) == H * (1 + ch * W)
    out = np.zeros((H, ch * W), dtype=np.int64)
    for y in range(H):
        ft, line = raw[y * (1 + ch * W)], raw[y * (1 + ch * W) + 1:(y + 1) * (1 + ch * W)]
        up = out[y - 1] if y else np.zeros(ch * W, dtype=np.int64)
        for i, x in enumerate(line):
            left = out[y, i - ch] if i >= ch else 0
            upleft = up[i - ch] if i >= ch else 0
            pred = (0, left, up[i], (left + up[i]) // 2, _paeth(int(left), int(up[i]), int(upleft)))[ft]
            out[y, i] = (x + pred) & 255
    return out.astype(np.uint8).reshape(H, W, ch)
