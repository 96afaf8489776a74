"""A synthetic walker seen from its own head-mounted camera, from parameters (tests, tools/slam_scale_bench.py).

The wearer walks along a gently curving path on alternating feet: the foot that stands is EXACTLY stationary in the world -- its
frames hold the same three doubles -- while the other one swings to its next landing point.  The camera sits in front of the head,
looks down, and turns (yaw, pitch) with time on top of the path's heading.  The SLAM trajectory is the true camera track under a
similarity: rotated by an arbitrary `world_rotation`, shifted by `world_offset` and DIVIDED by `scale`, so that `scale` is the
number `slam_scale.estimate_scale` has to find (metric = scale * SLAM).

Everything is a function of the parameters alone, built from IEEE basic operations, sqrt and sin / cos; the noise is numpy's
Generator(PCG64) normal with the given seed.
"""
import numpy as np

from .skeleton import MEAN3D_MM, N_JOINTS

CAMERA_HEIGHT = 1.45          # metres above the ground: the rest skeleton's feet are 1.39 .. 1.41 m below the camera
FOOT_HEIGHT = 0.05            # the foot point (midpoint of ankle and foot joint) above the ground while standing
HALF_STANCE_WIDTH = 0.10
FOOT_HALF = np.array([0.07, 0.0, -0.04])      # foot joint - foot point (forward, left, up); the ankle is the mirror image


def _rot_z(a):
    c, s, z, o = np.cos(a), np.sin(a), np.zeros_like(a), np.ones_like(a)
    return np.stack([np.stack([c, -s, z], -1), np.stack([s, c, z], -1), np.stack([z, z, o], -1)], -2)


def _rot_y(a):
    c, s, z, o = np.cos(a), np.sin(a), np.zeros_like(a), np.ones_like(a)
    return np.stack([np.stack([c, z, s], -1), np.stack([z, o, z], -1), np.stack([-s, z, c], -1)], -2)


def _rotvec_matrix(v):
    """Rodrigues: the rotation about v by |v| radians."""
    v = np.asarray(v, dtype=np.float64)
    th = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if th == 0.0:
        return np.eye(3)
    k = v / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def _quat_xyzw(R):
    """Rotation matrices [n,3,3] -> unit quaternions [n,4] (x, y, z, w), w >= 0 where it is the largest component."""
    from scipy.spatial.transform import Rotation
    return Rotation.from_matrix(R).as_quat()


# camera axes (right, back, down) in the body frame (forward, left, up) at heading 0 and no pitch: the columns of B0
_B0 = np.array([[0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, -1.0]]).T


def walk(n_frames, scale=1.0, fps=25.0, stance=14, step=10, speed=1.2, stand=(), noise=0.0, seed=0, world_rotation=(0.3, -0.5, 0.8),
         world_offset=(2.0, -1.0, 0.5), first_id=0):
    """-> dict:
      feet [n,2,3]    the world foot points (right, left): the midpoint of ankle and foot joint
      head [n,3]      the camera centre in the world, metres;  cams [n,4,4] the true camera-to-world matrices
      local [n,15,3]  the poses in the camera's frame (+ noise): what the pose network's lift estimates
      depth [n,15]    |local|, the joints' distances from the camera
      rows [n,8]      the SLAM trajectory `time tx ty tz qx qy qz qw` (time = frame id / fps), frame_ids [n]
      standing [n,2]  whether the foot stands (is stationary) in that frame
      world [n,15,3]  the joints in the world, without noise: a standing foot's joints hold the same doubles frame after frame
    step: a foot lands every `step` frames, the right one at the even multiples; stance: it then stands for frames
    [m step, m step + stance], both ends included (step <= stance < 2 step: both feet stand for stance - step frames in between),
    so that of any two frames no more than stance - step + 1 apart one foot stands in both; speed: metres per second, a number or one
    per frame; stand: [(a, b)] frame ranges [a, b) with speed 0 -- the wearer keeps stepping on the spot; noise: sigma in metres on
    every coordinate of `local`; scale: a number, or one per frame for a SLAM whose scale drifts -- the
    trajectory is then the running sum of the head's steps, each divided by the mean of its two frames' scales."""
    S, P, n = int(stance), int(step), int(n_frames)
    if n < 1 or P < 1 or not P <= S < 2 * P:
        raise ValueError("walk: need at least one frame and 1 <= step <= stance < 2 step")
    ext = n + 4 * P + 1                                  # landing points look a stride ahead
    v = np.broadcast_to(np.asarray(speed, dtype=np.float64), (n,)) if np.ndim(speed) else np.full(n, float(speed))
    v = np.concatenate([v, np.full(ext - n, v[-1])])
    for a, b in stand:
        v[int(a):int(b)] = 0.0
    d = np.concatenate([[0.0], np.cumsum(v[:-1] / fps)])                 # distance walked at every frame
    t = np.arange(ext, dtype=np.float64) / fps
    path = np.stack([d, 0.3 * np.sin(0.4 * d), np.zeros(ext)], 1)
    slope = 0.12 * np.cos(0.4 * d)                                       # the path's dy / dx
    fwd = np.stack([np.ones(ext), slope, np.zeros(ext)], 1) / np.sqrt(1.0 + slope * slope)[:, None]
    left = np.stack([-fwd[:, 1], fwd[:, 0], np.zeros(ext)], 1)
    up = np.array([0.0, 0.0, 1.0])
    head = path + up * CAMERA_HEIGHT + up[None] * (0.02 * np.sin(2.0 * np.pi * d / 0.7))[:, None] + 0.10 * fwd
    # landing points: stance m (frames [m step, m step + stance]) stands where the body is in the middle of it
    n_st = ext // P + 3
    ms = np.arange(-2, n_st)                                             # index m + 2 holds stance m
    at = np.clip(ms * P + S // 2, 0, ext - 1)
    lateral = np.where(ms % 2 == 0, -HALF_STANCE_WIDTH, HALF_STANCE_WIDTH)[:, None]          # even m: the right foot
    land = path[at] + lateral * left[at] + up * FOOT_HEIGHT
    land_fwd = fwd[at]
    feet = np.empty((ext, 2, 3))
    foot_fwd = np.empty((ext, 2, 3))
    standing = np.zeros((ext, 2), dtype=bool)
    for f in range(ext):
        for side in range(2):
            m = (f // P - side) // 2 * 2 + side                          # the side's latest stance that has begun
            since = f - m * P
            if since <= S:
                feet[f, side], foot_fwd[f, side], standing[f, side] = land[m + 2], land_fwd[m + 2], True
            else:
                u = (since - S) / (2 * P - S)
                w = u * u * (3.0 - 2.0 * u)
                stride = land[m + 4] - land[m + 2]
                lift = 0.15 * np.sqrt(stride[0] * stride[0] + stride[1] * stride[1]) * 4.0 * u * (1.0 - u)
                feet[f, side] = land[m + 2] + w * stride + up * lift
                foot_fwd[f, side] = land_fwd[m + 2] + w * (land_fwd[m + 4] - land_fwd[m + 2])
    # the camera: heading plus a yaw and a pitch that swing with time
    yaw = 0.15 * np.sin(2.0 * np.pi * 0.7 * t)
    pitch = 0.10 * np.sin(2.0 * np.pi * 0.45 * t + 0.5)
    body = np.stack([fwd, left, np.broadcast_to(up, (ext, 3))], -1)      # columns: forward, left, up
    R = body @ _rot_z(yaw) @ _rot_y(pitch) @ _B0
    # the body: upper body and hips ride with the head at constant offsets, the legs hang between hips and feet
    rest = MEAN3D_MM.T / 1000.0                          # camera frame: x right, y back, z down
    world = np.empty((ext, N_JOINTS, 3))
    for j in (0, 1, 2, 3, 4, 5, 6, 7, 11):
        world[:, j] = head - rest[j, 0] * left - rest[j, 1] * fwd - rest[j, 2] * up
    for side, (hip, knee, ankle, foot) in enumerate(((7, 8, 9, 10), (11, 12, 13, 14))):
        off = FOOT_HALF[0] * foot_fwd[:, side] + FOOT_HALF[2] * up
        world[:, ankle] = feet[:, side] - off
        world[:, foot] = feet[:, side] + off
        world[:, knee] = 0.5 * (world[:, hip] + world[:, ankle]) + 0.05 * fwd
    rel = world - head[:, None, :]
    local = np.stack([rel[..., 0] * R[:, None, 0, c] + rel[..., 1] * R[:, None, 1, c] + rel[..., 2] * R[:, None, 2, c] for c in range(3)], -1)
    cut = slice(0, n)
    local = local[cut]
    if noise > 0:
        local = local + np.random.default_rng(seed).normal(0.0, noise, local.shape)
    cams = np.tile(np.eye(4), (n, 1, 1))
    cams[:, :3, :3], cams[:, :3, 3] = R[cut], head[cut]
    Q = _rotvec_matrix(world_rotation)
    ids = np.arange(n, dtype=np.int64) + int(first_id)
    if np.ndim(scale):                                   # a drifting scale: every step of the head at the mean of its two frames' scales
        scale = np.asarray(scale, dtype=np.float64)
        if scale.shape != (n,):
            raise ValueError("walk: scale is a number or one per frame")
        moved = head[cut] @ Q.T
        first = moved[:1] / scale[0]
        track = np.concatenate([first, first + np.cumsum((moved[1:] - moved[:-1]) / (0.5 * (scale[1:] + scale[:-1]))[:, None], axis=0)])
    else:
        track = head[cut] @ Q.T / scale
    rows = np.concatenate([(ids / fps)[:, None], track + np.asarray(world_offset, dtype=np.float64), _quat_xyzw(Q @ R[cut])], 1)
    return {"feet": feet[cut], "head": head[cut], "cams": cams, "local": local, "depth": np.sqrt((local * local).sum(-1)), "rows": rows,
            "frame_ids": ids, "standing": standing[cut], "world": world[cut], "scale": scale if np.ndim(scale) else float(scale), "fps": float(fps),
            "stance": S, "step": P}


def slam_inputs(w, lo=0, hi=None):
    """(R [n,3,3], c [n,3]) of frames [lo, hi) of a walker: `slam.relative_poses` of its trajectory rows, as the estimator takes them."""
    from . import slam
    rows = w["rows"][lo:hi]
    rt, rq = slam.relative_poses(rows[:, 1:4], rows[:, 4:8])
    return slam.pose_matrix(rt, rq)[:, :3, :3], rt
