#!/usr/bin/env python3
"""What the camera's view of `--render_camera` costs, for one 98-frame chunk with two sequences over its
heat-maps at 512 x 512 and the default radii, beside the orthographic renderer of `--render` for the same number and size of images
on the same card:

    python tools/camera_view_bench.py [--frames 98] [--size 512x512] [--dir DIR] [--repeats 5]

  kernel_camera   gem_render_camera for the chunk's images (60 primitives each, 15 heat-maps): the kernel's device time from a
                  `rocprofv3 --kernel-trace` run of its own (tools/render_bench.py's route), and the call between two HIP events,
                  best of --repeats; Mpixel/s and the store bandwidth are pixels and scanline bytes / kernel time
  kernel_ortho    gem_render_capsules for as many images of that size with the same two sequences (60 capsules each)
  total_camera    `render.write_camera_frames`, all of it: projection, kernel, copies, deflate and files pipelined
  total_ortho     `render.write_frames` without its overviews, for the same sequences

Prints one JSON line.  The files go to a temporary directory under --dir (default: the system's) and are removed.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np          # noqa: E402

import render_bench as B          # noqa: E402


def chunk(frames):
    """Synthetic frames with rotated cameras: heat-maps, cameras, and two sequences in the cameras' world."""
    from globalegomocap_amd import synth
    s = synth.make_sequence(n_frames=frames, seed=7, cam_jitter=(2.0, 0.01))
    cams = np.asarray(s["camera_pose_list"], dtype=np.float64)
    local = np.asarray(s["estimated_local_skeleton"], dtype=np.float64)
    est = np.einsum("nij,nkj->nki", cams[:, :3, :3], local) + cams[:, None, :3, 3]
    return [est, est + np.random.default_rng(7).normal(0.0, 0.03, est.shape)], cams, np.asarray(s["heatmap_list"], dtype=np.float32)


def scenes(e, frames, N):
    """What the two kernels read: (heat, uv, rgb, view) of the camera's view, (geom, rgb, first, view) of the orthographic frames."""
    from globalegomocap_amd import render as R
    seqs, cams, heat = chunk(frames)
    colours = list(R.PALETTE.values())[:2]
    camera = R._camera_scene(e, seqs, cams, heat, colours, None) + (R.camera_view(N),)
    d_seqs, crts = R._prepare(e, seqs, None)
    ortho = R._scene(e, d_seqs, crts, colours, False) + (R.frames_view(e, seqs, size=(N, N)),)
    return seqs, cams, heat, camera, ortho


def kernels_only(frames, N, repeats):
    """`repeats` + 1 launches of either kernel and nothing else (run under rocprofv3)."""
    import torch
    from globalegomocap_amd import render as R
    e = B.engine()
    _, _, _, camera, ortho = scenes(e, frames, N)
    out = torch.empty(frames, R.layout(N, N).stride, dtype=torch.uint8, device=e.device)
    for _ in range(repeats + 1):
        e.render_camera(*camera, out=out)
    for _ in range(repeats + 1):
        e.render_capsules(*ortho, out=out)
    torch.cuda.synchronize()


def measure(frames, N, work, repeats):
    import torch
    from globalegomocap_amd import render as R
    me = os.path.abspath(__file__)
    lay = R.layout(N, N)
    res = {"frames": frames, "size": "%dx%d" % (N, N), "sequences": 2, "scanline_mb": round(frames * lay.image_bytes / 1e6, 1)}
    kt, why = B.kernel_times(frames, (N, N), repeats, work, script=me, kernels=("render_camera_kernel", "render_capsules_kernel"), groups=1)          # (before this process opens the device)
    if kt is None:
        res["kernel"] = why
    else:
        for name, k in zip(("camera", "ortho"), kt):
            res.update({"kernel_%s_ms" % name: round(k * 1e3, 4), "kernel_%s_mpixel_s" % name: round(frames * N * N / k / 1e6, 1),
                        "kernel_%s_store_gb_s" % name: round(frames * lay.image_bytes / k / 1e9, 1)})
    e = B.engine()
    seqs, cams, heat, camera, ortho = scenes(e, frames, N)
    out = torch.empty(frames, lay.stride, dtype=torch.uint8, device=e.device)
    res["call_camera_ms"] = round(B.timed(lambda: e.render_camera(*camera, out=out), repeats) * 1e3, 4)
    res["camera_bytes_not_white"] = round(float((out[:, :lay.image_bytes] != 255).float().mean()), 4)          # (something was drawn)
    res["call_ortho_ms"] = round(B.timed(lambda: e.render_capsules(*ortho, out=out), repeats) * 1e3, 4)
    res["ortho_bytes_not_white"] = round(float((out[:, :lay.image_bytes] != 255).float().mean()), 4)
    # all of it, pipelined (twice: the first call also allocates the pinned buffers)
    for name, fn in (("camera", lambda d: R.write_camera_frames(e, seqs, cams, heat, d, size=N)),
                     ("ortho", lambda d: R.write_frames(e, seqs, d, size=(N, N), overview=False))):
        totals = []
        for _ in range(2):
            d = tempfile.mkdtemp(prefix="camera_total_", dir=work)
            try:
                torch.cuda.synchronize()
                t = time.perf_counter()
                n = fn(d)
                totals.append(time.perf_counter() - t)
                assert n == frames
            finally:
                shutil.rmtree(d, ignore_errors=True)
        res.update({"write_%s_frames_ms" % name: [round(x * 1e3, 1) for x in totals], "write_%s_images_s" % name: round(frames / min(totals), 1)})
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=98)
    p.add_argument("--size", default="512x512", help="NxN")
    p.add_argument("--dir", default=None, help="where the temporary files go")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernels-only", action="store_true", help="(the run under rocprofv3)")
    a = p.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import render as R
    N, N2 = R._size(a.size)
    if N != N2:
        p.error("the camera's view is square: --size NxN")
    if a.kernels_only:
        kernels_only(a.frames, N, a.repeats)
        return
    print(json.dumps(measure(a.frames, N, a.dir, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
