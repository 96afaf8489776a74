"""The five energy terms of one window and dE_k/dX of each, in float64, written from the formulas -- TEST INFRASTRUCTURE.

Reference (paths relative to the reference tree): optimizer.py:139-149 (heat-map sample), 172-177 (bone length), 202-213
(smoothness, 3-D), 226-240 (the sum); utils/fisheye/FishEyeCalibrated.py:96-129 (projection).  Nothing here follows the fp32
staging of oracle/np_oracle.py or of the device code: every quantity is float64 from the widened inputs on, the gradient of a
term is the derivative of the expression that stands above it, and the skeleton is an argument.  tests/test_energy_f64_cpu.py
holds it to the oracle and to its own central differences; tests/test_energy_terms_gpu.py holds every device form of the
energy code to it, evaluated at the pose the device itself decoded."""
import numpy as np

TERMS = ("3d", "smooth", "bone", "vae", "reproj")


def project(cam, P):
    """Camera-frame points P [n,3] -> image points (u, v) and d(u,v)/dP [n,2,3] (FishEyeCalibrated.py:96-129:
    rho(theta) = sum_i poly[i] theta^i with theta = atan(-z / |(x,y)|), (u, v) = rho * (x,y)/|(x,y)| + (cx, cy))."""
    poly = np.asarray(cam.poly, dtype=np.float64)
    xy, z = P[:, :2], P[:, 2]
    n = np.sqrt(np.sum(xy * xy, axis=1))
    if not (n != 0).all():
        raise ValueError("a point on the optical axis has no projection")
    theta = np.arctan2(-z, n)
    k = np.arange(len(poly))
    rho = np.sum(poly * theta[:, None] ** k, axis=1)
    drho = np.sum(poly[1:] * k[1:] * theta[:, None] ** (k[1:] - 1), axis=1)
    c = xy / n[:, None]                                             # unit direction in the image plane
    uv = c * rho[:, None] + np.array([cam.cx, cam.cy], dtype=np.float64)
    r2 = n * n + z * z
    dth_dn, dth_dz = z / r2, -n / r2                                # theta = atan2(-z, n)
    J = np.empty((P.shape[0], 2, 3))
    # d(c)/d(xy) = (I - c c^T) / n;  d(rho)/d(xy) = rho' * dtheta/dn * c
    J[:, :, :2] = rho[:, None, None] * (np.eye(2) - c[:, :, None] * c[:, None, :]) / n[:, None, None] \
        + c[:, :, None] * (drho * dth_dn)[:, None, None] * c[:, None, :]
    J[:, :, 2] = c * (drho * dth_dz)[:, None]
    return uv, J


def heat_coords(uv, H, W):
    """Image point -> heat-map texel coordinates (optimizer.py:143-147, then grid_sample's align_corners=True un-normalisation):
    the 1024-wide image between the 128-pixel side bands maps onto texels 0 .. W-1."""
    ix = (((uv[:, 0] - 128.0) - 512.0) / 512.0 + 1.0) / 2.0 * (W - 1)
    iy = ((uv[:, 1] - 512.0) / 512.0 + 1.0) / 2.0 * (H - 1)
    return ix, iy


def bilinear(heat, ix, iy):
    """heat [T,H,W,J]; ix, iy [T*J]: pair (t, j) samples the map heat[t, :, :, j] -> (value, d/dix, d/diy); texels outside the
    map are zero (grid_sample, padding 'zeros')."""
    T, H, W, J = heat.shape
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    fx, fy = ix - x0, iy - y0
    t, j = np.repeat(np.arange(T), J), np.tile(np.arange(J), T)

    def texel(y, x):
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(inside, heat[t, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1), j].astype(np.float64), 0.0)

    nw, ne, sw, se = texel(y0, x0), texel(y0, x0 + 1), texel(y0 + 1, x0), texel(y0 + 1, x0 + 1)
    top, bottom = nw + (ne - nw) * fx, sw + (se - sw) * fx
    val = top + (bottom - top) * fy
    dix = (ne - nw) * (1.0 - fy) + (se - sw) * fy
    diy = bottom - top
    return val, dix, diy


def terms64(X, X0, mean_bone, heat, cam, parents):
    """X, X0 [T,J,3]; mean_bone [J]; heat [T,H,W,J] (or None: no reprojection term); cam: poly / cx / cy; parents [J].

    Returns (parts [5] = E_3d, E_smooth, E_bone, E_vae, E_reproj; grads [5,T,J,3] = dE_k/dX; (ix, iy) [T,J] each: where every
    (frame, joint) pair falls in its heat-map, NaN without heat-maps).  The total energy is weights . parts, its gradient
    sum_k weights[k] * grads[k]."""
    X = np.asarray(X, dtype=np.float64)                             # (float32 input is widened exactly)
    X0 = np.asarray(X0, dtype=np.float64)
    mb = np.asarray(mean_bone, dtype=np.float64)
    parents = np.asarray(parents, dtype=np.int64)
    T, J, _ = X.shape
    parts, grads = np.zeros(5), np.zeros((5, T, J, 3))

    d = X - X0                                                      # 3-D term: sum |X - X0|^2
    parts[0] = np.sum(d * d)
    grads[0] = 2.0 * d

    acc = X[:-2] - 2.0 * X[1:-1] + X[2:]                            # smoothness: sum_t |X[t-1] - 2 X[t] + X[t+1]|^2
    parts[1] = np.sum(acc * acc)
    grads[1, :-2] += 2.0 * acc
    grads[1, 1:-1] -= 4.0 * acc
    grads[1, 2:] += 2.0 * acc

    bone = X - X[:, parents]                                        # bone length: sum (|X_j - X_parent(j)| - mean_bone_j)^2
    length = np.sqrt(np.sum(bone * bone, axis=-1))
    diff = length - mb[None]
    parts[2] = np.sum(diff * diff)
    unit = np.divide(bone, length[..., None], out=np.zeros_like(bone), where=length[..., None] > 0)    # d|v|/dv := 0 at v = 0
    gb = 2.0 * diff[..., None] * unit
    grads[2] += gb
    np.subtract.at(grads[2], (slice(None), parents), gb)

    parts[3] = np.sum(X * X)                                        # "vae" term: sum X^2 (on the pose)
    grads[3] = 2.0 * X

    ix = iy = np.full((T, J), np.nan)
    if heat is not None:                                            # reprojection: -sum heat[t,:,:,j](projection of X[t,j])
        H, W = heat.shape[1], heat.shape[2]
        uv, Juv = project(cam, X.reshape(-1, 3))
        ix, iy = heat_coords(uv, H, W)
        val, dix, diy = bilinear(np.asarray(heat), ix, iy)
        parts[4] = -np.sum(val)
        du, dv = dix * (W - 1) / 1024.0, diy * (H - 1) / 1024.0    # d(ix)/du, d(iy)/dv
        grads[4] = -(du[:, None] * Juv[:, 0] + dv[:, None] * Juv[:, 1]).reshape(T, J, 3)
        ix, iy = ix.reshape(T, J), iy.reshape(T, J)
    return parts, grads, (ix, iy)


def texel_line_distance(ix, iy):
    """Distance (texels) of every pair to the nearest texel line in x or y: across a line the sample's derivative jumps, and an
    fp32 floor may fall on the other side than the float64 one."""
    return np.minimum(np.abs(ix - np.round(ix)), np.abs(iy - np.round(iy)))
