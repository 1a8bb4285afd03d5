#!/usr/bin/env python3
"""Time of StocsEstimator.explain_poses_mesh (stocs_explain_poses_mesh: clear, key render, one depth render and one resolve pass per
chunk, one read-back, one synchronisation per call) for 1, 8 and 64 poses on a 640 x 480 frame, on the level-5 Cm mesh
(synth.make_model_mesh: 25 600 triangles) at synth.gt_pose() and on tools/mesh_time.py's 12-triangle box that fills a third of the frame.
Beside the Cm rows the same poses through explain_poses on the 5 000-point Cm cloud at the default radius: the path the masks took before.
Median of 20 calls after 5 warm-up calls of the host wall clock, with the spread, and the median HIP-event time of the two new kernels
(the key render; the resolve kernel of the call's one chunk) of as many calls with the option device_clock on.  No time is promised.

    python tools/render_mesh_time.py [--out profiles/render_mesh_time.json]

Needs a GPU; no fallback."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from depth_check_time import clock, perturbed  # noqa: E402
from mesh_time import box_mesh_and_pose, frame_from  # noqa: E402
import mesh_time  # noqa: E402

SIZES = (1, 8, 64)
REPS, WARM = 20, 5
F = np.float32


def device_medians(est, call):
    est.set_option("device_clock", 1)
    t = []
    for i in range(WARM + REPS):
        call()
        if i >= WARM:
            t.append(est.render_mesh_last_device_ms())
    est.set_option("device_clock", 0)
    t = np.asarray(t)
    return float(np.median(t[:, 0])), float(np.median(t[:, 1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_mesh_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("render_mesh_time.py needs a GPU: no time is taken without one")
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    mesh_time.K = [float(v) for v in synth.YCB_INTRINSICS]
    m = synth.make_model(5000)
    rng = np.random.default_rng(3); sp = rng.normal(0, 0.05, (64, 3)).astype(F)
    est = StocsEstimator(sp, sp / np.linalg.norm(sp, axis=1, keepdims=True), np.ones(64, F), None, m.pos, m.nrm, build_index=False)
    bv, bt, bP = box_mesh_and_pose()
    rows = []
    for label, v, t, P0, with_points in (("Cm level 5", *synth.make_model_mesh(5), synth.gt_pose(), True), ("box 12 triangles", bv, bt, bP, False)):
        est.set_mesh(v, t)
        share = frame_from(est, P0)
        for n in SIZES:
            poses = perturbed(P0, n, 100 + n)
            mesh = lambda: est.explain_poses_mesh(poses)
            rec = mesh()
            key_ms, resolve_ms = device_medians(est, mesh)
            row = {"workload": label, "triangles": int(len(t)), "frame_share": round(share, 3), "poses": n, "explain_poses_mesh": clock(mesh),
                   "key_render_kernel_ms": key_ms, "resolve_kernel_ms": resolve_ms, "mean_footprint": float(rec["footprint"].mean()),
                   "mean_visible": float(rec["visible"].mean())}
            if with_points:
                pts = est.explain_poses(poses)
                row.update({"explain_poses_5000_points": clock(lambda: est.explain_poses(poses)), "points_mean_footprint": float(pts["footprint"].mean())})
            rows.append(row)
            print(json.dumps(row), flush=True)
    est.close()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "mesh.hip", "render_mesh.hip"], capture_output=True, text=True,
                         stdin=subprocess.DEVNULL)
    out = {"what": "host wall clock of explain_poses_mesh and HIP-event time of its two new kernels, next to explain_poses on the 5 000-point cloud, same poses",
           "device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM, "note": "one visit, one GPU; the host column shares the machine with other work",
           "kernel_resources": res.stdout.strip(), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
