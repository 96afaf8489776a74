#!/usr/bin/env python3
"""What the two routes into a `Recording` compute, as sha256 sums: for comparing two trees on one card.

    python tools/recording_identity.py --json FILE [--parent FILE_OF_THE_OTHER_TREE]

A 208-frame walker (`synth_walk`, SLAM scale 0.6) as eight 26-frame chunks: once as the pose network's .mat files (heat-maps with one
paraboloid per joint) through `prepare.prepare_sequence` and, for its first chunk, `prepare.main`; once as 2-D detections through
`detections.recording_from_detections` and the `detections` command line.  Both under five settings: ground truth, a number,
"auto", bridge + number and bridge + "auto" -- the bridge on a trajectory without the lines of frame ids 36 .. 40 -- and then with
"drift" and a knot distance, with the depths from the bone lengths (no depth file, no depth array), with the sub-pixel lift of the .mat
route beside depth files, and once as ONE span through `prepare.prepare_continuous` and `detections.continuous_from_detections`.  Every
option is given by keyword, or as the command line spells it.  Hashed: every
chunk's heat, est_local, est_global, cams and gt, the origins, the scale, both reports' as_dict(), what was printed, and the pickles
`write_chunks` / `write_chunk` left.  A refusal is hashed as its type and text.  With --parent the sums are compared with those file
holds and both runs are written to --json (`profiles/recording_identity.json`); the exit status tells whether they are equal.
"""
import argparse
import contextlib
import hashlib
import io
import json
import os
import shutil
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N, SIZE, FPS, SCALE, LOST = 208, 26, 25, 0.6, (36, 41)
SETTINGS = {"ground truth": dict(gt=True), "number": dict(scale=0.6), "auto": dict(scale="auto"),
            "bridge + number": dict(scale=0.6, bridge=1.0, holed=True), "bridge + auto": dict(scale="auto", bridge=1.0, holed=True),
            # `more`: keywords of every route (`more_cli`: as the command line spells them); `mat`: of the .mat route alone
            "drift": dict(scale="drift", more=dict(knot=52), more_cli=["--knot", "2.08"]),
            "bones": dict(scale=0.6, more=dict(depth="bones"), more_cli=["--depth_from", "bones"], no_depth_dir=True),
            "subpixel": dict(scale=0.6, mat=dict(peaks="subpixel")),
            "one span": dict(scale="auto", one_span=True)}


def sha(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        x = str(x.dtype).encode() + str(x.shape).encode() + np.ascontiguousarray(x).tobytes()
    elif not isinstance(x, bytes):
        x = json.dumps(x, sort_keys=True).encode()
    return hashlib.sha256(x).hexdigest()


def recording_sums(rec):
    out = {"chunks": len(rec), "origins": sha(rec.origins), "scale": sha(rec.scale),
           "scale_report": sha(None if rec.scale_report is None else rec.scale_report.as_dict()),
           "bridge_report": sha(None if rec.bridge_report is None else rec.bridge_report.as_dict()),
           "bridged": sha(None if rec.bridged is None else np.concatenate(rec.bridged)),
           "depth_report": sha(None if rec.depth_report is None else rec.depth_report.as_dict()),
           "initial_mpjpe": sha([c.initial_mpjpe for c in rec.chunks])}
    for i, c in enumerate(rec.chunks):
        for k in ("heat", "est_local", "est_global", "cams", "gt"):
            out["chunk %d %s" % (i, k)] = sha(getattr(c, k))
    return out


def pickle_sums(root):
    out = {}
    for dirpath, _, files in sorted(os.walk(root)):
        for f in sorted(files):
            with open(os.path.join(dirpath, f), "rb") as fh:
                out["file " + os.path.relpath(os.path.join(dirpath, f), root)] = sha(fh.read())
    return out


def run(fn, out_root):
    """fn() with its stdout captured -> the sums of what it returned, printed and wrote; a refusal as its type and text."""
    printed = io.StringIO()
    try:
        with contextlib.redirect_stdout(printed):
            rec = fn()
        sums = {} if rec is None else recording_sums(rec)
    except (ValueError, SystemExit) as e:
        sums = {"refused": "%s: %s" % (type(e).__name__, e)}
    sums["stdout"] = sha(printed.getvalue().replace(out_root, "<out>"))
    sums["stdout lines"] = len(printed.getvalue().splitlines())
    sums.update(pickle_sums(out_root))
    return sums


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", required=True, metavar="FILE")
    ap.add_argument("--parent", default=None, metavar="FILE", help="the sums of the other tree's run, to compare with")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from globalegomocap_amd import detections as D, prepare as P, synth, synth_recording as R, synth_walk as W
    from globalegomocap_amd.camera import DEFAULT_CALIBRATION, FisheyeCamera
    w = W.walk(N, scale=SCALE)
    cam = FisheyeCamera.from_json(DEFAULT_CALIBRATION)
    uv = cam.project_numpy(w["local"].reshape(-1, 3)).reshape(N, 15, 2)
    ix, iy = synth.heatmap_coords(uv)
    heat64 = R.paraboloid_heatmaps(np.floor(np.stack([ix, iy], -1)) + np.array([0.3, 0.2]), np.full((N, 15), 5.0))
    gt = np.einsum("nij,nkj->nki", w["cams"][:, :3, :3], w["local"]) + w["cams"][:, None, :3, 3]
    work = tempfile.mkdtemp(prefix="gem_recording_identity_")
    sums = {}
    try:
        hd, dd, traj, gtp = R.write_recording(os.path.join(work, "rec"), heat64, w["depth"], ["f_%d.mat" % k for k in range(N)], None, None,
                                              w["rows"], gt)
        holed = os.path.join(work, "holed.txt")
        with open(traj) as f, open(holed, "w") as g:
            g.write("".join(l for k, l in enumerate(f.read().splitlines(True)) if not LOST[0] <= k < LOST[1]))
        det = os.path.join(work, "det.npz")
        np.savez(det, keypoints=np.concatenate([uv, np.ones((N, 15, 1))], axis=2), depth=w["depth"])
        spans = P.chunk_spans(0, N + 1, SIZE)
        for name, s in SETTINGS.items():
            t = holed if s.get("holed") else traj
            g, scale, bridge = (gtp if s.get("gt") else None), s.get("scale"), s.get("bridge")
            how = (["--gt", gtp] if g else ["--scale", str(scale)]) + (["--bridge", str(bridge)] if bridge else []) + s.get("more_cli", [])
            more = s.get("more", {})
            mat = dict(more, **s.get("mat", {}))
            depths = None if s.get("no_depth_dir") else dd
            routes = {
                "prepare_sequence": lambda o: P.prepare_sequence(t, hd, depths, g, 0, N + 1, fps=FPS, test_size=SIZE, out_root=o, scale=scale,
                                                                 min_pairs=10, bridge=bridge, **mat),
                "prepare.main": lambda o: P.main(t, hd, depths, g, 0, SIZE, o, FPS, scale=scale, min_pairs=5, bridge=bridge, **mat),
                "recording_from_detections": lambda o: D.recording_from_detections(t, det, g, scale, spans, FPS, min_pairs=30, bridge=bridge, **more),
                "detections command line": lambda o: D._cli(["--slam", t, "--keypoints", det, "--start", "0", "--end", str(N + 1), "--fps", str(FPS),
                                                            "--test_size", str(SIZE), "--out", o] + how),
            }
            if s.get("one_span"):
                routes = {
                    "prepare_continuous": lambda o: P.prepare_continuous(t, hd, dd, g, 0, N, fps=FPS, scale=scale, min_pairs=10),
                    "continuous_from_detections": lambda o: D.continuous_from_detections(t, det, g, scale, 0, N, FPS, min_pairs=30),
                }
            for route, fn in routes.items():
                out_root = os.path.join(work, "out")
                sums["%s / %s" % (name, route)] = run(lambda: fn(out_root), out_root)
                shutil.rmtree(out_root, ignore_errors=True)
                torch.cuda.synchronize()
    finally:
        shutil.rmtree(work, ignore_errors=True)
    result = {"what": "sha256 of what the two routes into a Recording compute, print and write from one synthetic 208-frame walker under nine "
                      "settings (tools/recording_identity.py)", "device": torch.cuda.get_device_name(0), "sums": sums}
    same = None
    if a.parent is not None:
        with open(a.parent) as f:
            parent = json.load(f)
        same = parent["sums"] == sums
        result = {"what": result["what"], "device": result["device"], "identical_to_parent": same,
                  "differing": sorted(k for k in set(sums) | set(parent["sums"]) if sums.get(k) != parent["sums"].get(k)),
                  "refusals": {k: v["refused"] for k, v in sums.items() if "refused" in v}, "parent": parent["sums"], "this_tree": sums}
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("%d runs hashed%s" % (len(sums), "" if same is None else "; identical to the parent's: %s" % same))
    return 0 if same in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
