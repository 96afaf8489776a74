"""What the end-to-end tests of `save`, `render` and `render_camera` share (tests/test_meshes_gpu.py, test_render_gpu.py,
test_camera_view_gpu.py): the tiny recording their chunks are cut from, the bit-for-bit comparison of two results, and the checkers
of a chunk's mesh folders, frame files and camera views against the sequences a call returned."""
import os

import numpy as np

import mesh_twin

SIZE = 26                  # frames per chunk: three windows
IMG = (64, 48)             # `render.DEFAULT_SIZE` under `small_images`
CAMERA_N = 48              # `render.CAMERA_SIZE` under `small_images`


def write_recording(root, n, seed):
    from globalegomocap_amd import synth_recording as S
    par = S.random_parameters(n, seed=seed)
    heat64 = S.paraboloid_heatmaps(par["centres"], par["radii"])
    names = ["f_%d.mat" % k for k in range(n)]
    return S.write_recording(str(root), heat64, par["depth"], names, np.arange(n) % 7 == 3, np.arange(n) % 5 == 1, par["rows"], par["gt"])


def same_bits(x, y):
    assert list(x[0]) == list(y[0]) and len(x[1]) == len(y[1])
    for rx, ry in zip([x[0]] + x[1], [y[0]] + y[1]):
        for k in rx:
            assert np.array_equal(np.asarray(rx[k], dtype=np.float64).view(np.uint64), np.asarray(ry[k], dtype=np.float64).view(np.uint64)), k
    for i in (2, 3, 4):
        assert (x[i] is None and y[i] is None) or np.array_equal(x[i], y[i]), i


def sphere_centres(path):
    assert os.path.getsize(path) == len(mesh_twin.HEADER) + 349920 + 335400, path
    v, c, t = mesh_twin.read_ply(path)
    return v[:15 * 762].reshape(15, 762, 3).mean(axis=1)


def check_folder(folder, want):
    assert sorted(os.listdir(folder)) == ["out_%04d.ply" % f for f in range(len(want))], folder
    for f in range(len(want)):
        np.testing.assert_allclose(sphere_centres(os.path.join(folder, "out_%04d.ply" % f)), want[f], rtol=0, atol=1e-9, err_msg="%s %d" % (folder, f))


def image_of(rows, k, W, H):
    return rows[k, :H * (1 + 3 * W)].reshape(H, 1 + 3 * W)[:, 1:].reshape(H, W, 3)


def check_tree(env, base, est, opt, gt):
    """frame_%04d.png for every frame and one overview per sequence under `base`, 64 x 48 pixels (`small_images`);
    frame 3 and the last overview equal `scanlines` of the sequences, the first two aligned to the ground truth where there is one."""
    from globalegomocap_amd import render as R
    trio = [est, opt] + ([gt] if gt is not None else [])
    names = list(R.PALETTE)[:len(trio)]
    assert sorted(os.listdir(base)) == sorted(["frame_%04d.png" % f for f in range(len(est))] + ["overview_%s.png" % n for n in names])
    to = [gt, gt, None] if gt is not None else None
    view = R.frames_view(env, trio, align_to=to, size=IMG)
    colours = [R.PALETTE[n] for n in names]
    frames = R.scanlines(env, trio, view, colours, align_to=to).cpu().numpy()
    assert np.array_equal(R.read_png(os.path.join(base, "frame_0003.png")), image_of(frames, 3, *IMG))
    assert (image_of(frames, 3, *IMG) != 255).any()
    overviews = R.scanlines(env, trio, view, colours, overview=True, align_to=to).cpu().numpy()
    assert np.array_equal(R.read_png(os.path.join(base, "overview_%s.png" % names[-1])), image_of(overviews, len(trio) - 1, *IMG))


def check_camera_tree(env, base, est, opt, gt, cams, heat, others=()):
    """camera_%04d.png for every frame under `base` (beside `others`), CAMERA_N pixels each way (`small_images`); frame 3 equals
    `camera_scanlines` of the sequences, the ground truth moved onto the optimised sequence where there is one."""
    from globalegomocap_amd import render as R
    n = len(est)
    assert sorted(os.listdir(base)) == sorted(["camera_%04d.png" % f for f in range(n)] + list(others))
    trio = [est, opt] + ([gt] if gt is not None else [])
    colours = [R.PALETTE[k] for k in list(R.PALETTE)[:len(trio)]]
    want = R.camera_scanlines(env, trio, cams[:n], heat[:n], colours, align_to=[None, None, opt][:len(trio)]).cpu().numpy()
    got = R.read_png(os.path.join(base, "camera_0003.png"))
    assert got.shape == (CAMERA_N, CAMERA_N, 3) and np.array_equal(got, image_of(want, 3, CAMERA_N, CAMERA_N))
    assert (got != 255).any()
    return got
