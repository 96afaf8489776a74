"""The numpy twin of gem_render_camera (the camera's view): the background from the oracle's fp32 heat-map
coordinates and bilinear sample, the overlay in plain float64 numpy on the widened fp32 image points."""
from collections import namedtuple

import numpy as np

from globalegomocap_amd.skeleton import MESH_LINES
from oracle import np_oracle as O

F32 = np.float32
N_PRIMS = 30
EDGE = 1e-6          # image pixels: a pixel centre this near a primitive's rim may fall either way
ROUND = 1e-4         # of a byte: a background value this near a rounding step may fall either way

Image = namedtuple("Image", "ids response rgb near_edge near_round")


def places(N):
    """The pixels' places in the 1280 x 1024 image: (u, v) in fp32 for the background and in float64 for the overlay, each [N]."""
    k32, k64 = np.arange(N, dtype=F32), np.arange(N, dtype=np.float64)
    s32, s64 = F32(1024) / F32(N), 1024.0 / N
    return (F32(128) + (k32 + F32(0.5)) * s32, (k32 + F32(0.5)) * s32), (128.0 + (k64 + 0.5) * s64, (k64 + 0.5) * s64)


def response(heat, N, joint_mask):
    """heat [H,W,J] f32 or None -> m [N,N] f32: the largest bilinear sample over the joints of `joint_mask`, clamped to [0, 1]."""
    m = np.zeros((N, N), dtype=F32)
    if heat is None or not joint_mask:
        return m
    heat = np.asarray(heat, dtype=F32)
    H, W, J = heat.shape
    (u, v), _ = places(N)
    uv = np.stack([np.tile(u, N), np.repeat(v, N)], axis=1).astype(F32)
    ix, iy = O.heat_coords(uv, H, W)
    for j in range(J):
        if (joint_mask >> j) & 1:
            val = O.bilinear_sample(np.broadcast_to(heat[:, :, j], (N * N, H, W)), ix, iy)[0]
            m = np.maximum(m, val.reshape(N, N))
    return np.minimum(m, F32(1)).astype(F32)


def distances(a, b, u, v):
    """The distance of every pixel centre (u [N] across, v [N] down) from the segment a-b (a == b: a point) -> [N,N] float64."""
    U, V = np.meshgrid(u, v)
    wx, wy = U - a[0], V - a[1]
    dx, dy = b[0] - a[0], b[1] - a[1]
    dd = dx * dx + dy * dy
    t = np.clip((wx * dx + wy * dy) / dd, 0.0, 1.0) if dd > 0.0 else 0.0
    ex, ey = wx - t * dx, wy - t * dy
    return np.sqrt(ex * ex + ey * ey), ex * ex + ey * ey


def render(heat, uv, colours, N, joint_mask=0x7FFF, heat_colour=(148, 103, 189), joint_radius=8.0, line_radius=3.0):
    """One image.  heat [H,W,J] f32 or None; uv [S,15,2] f32 (the image points as the device holds them); colours S RGB triples."""
    uv = np.asarray(uv, dtype=F32).astype(np.float64).reshape(-1, 15, 2)
    _, (u, v) = places(N)
    m = response(heat, N, joint_mask)
    value = 255.0 + (np.asarray(heat_colour, dtype=np.float64)[None, None, :] - 255.0) * m.astype(np.float64)[:, :, None] + 0.5
    rgb = np.floor(value).astype(np.uint8)
    frac = value - np.floor(value)
    near_round = ((frac < ROUND) | (frac > 1.0 - ROUND)).any(axis=-1)
    ids = np.full((N, N), -1, dtype=np.int32)
    near_edge = np.zeros((N, N), dtype=bool)
    for s in range(uv.shape[0]):          # painted over: the higher sequence, then the joint, then the lower index stays on top
        for c in range(N_PRIMS - 1, -1, -1):
            ja, jb = (c, c) if c < 15 else MESH_LINES[c - 15]
            a, b = uv[s, ja], uv[s, jb]
            if not (np.isfinite(a).all() and np.isfinite(b).all()):
                continue
            r = joint_radius if c < 15 else line_radius
            d, d2 = distances(a, b, u, v)
            covered = d2 <= r * r
            near_edge |= np.abs(d - r) <= EDGE
            ids[covered] = s * N_PRIMS + c
            rgb[covered] = np.asarray(colours[s], dtype=np.uint8)
    return Image(ids, m, rgb, near_edge, near_round)
