#!/usr/bin/env python3
"""Host wall clock of StocsEstimator.explain_poses (stocs_explain_poses: clear, splat, resolve, one read-back, one synchronisation per
call; records only, and records + label and state images) for n = 1, 6, 16 and 64 poses, on the ycb example fixture (472-point model)
and on a 5 000-point synthetic model against a 640 x 480 frame rendered from it.  Two yardsticks from the same visit: depth_check_poses
of the same poses (the nearest existing call: every pose alone, no image-space output) and the float32 numpy restatement
tests/render_ref.py::explain (the only route to masks and visibility before).  Median of 20 calls after 5 warm-up calls, with the spread
(min, max); the restatement, seconds per pass at the larger sizes, is timed over fewer passes (recorded).  Asserts that the library's
records, labels and states equal the restatement's.  Needs a GPU; no fallback.

    python tools/render_time.py [--out profiles/render_time.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_ref  # noqa: E402
from depth_check_time import _rot, clock, perturbed, render  # noqa: E402

SIZES = (1, 6, 16, 64)
REPS, WARM = 20, 5


def measure(label, est, mpos, mnrm, depth, prob, K, scale, P0):
    rows = []
    for n in SIZES:
        poses = perturbed(P0, n, 100 + n)
        records = clock(lambda: est.explain_poses(poses), REPS, WARM)
        with_labels = clock(lambda: est.explain_poses(poses, labels=True), REPS, WARM)
        depth_check = clock(lambda: est.depth_check_poses(poses), REPS, WARM)
        host_reps = 3 if n <= 6 else 1
        host = clock(lambda: render_ref.explain(poses, mpos, mnrm, depth, prob, K, scale), reps=host_reps, warm=0)
        rec, lab, st = est.explain_poses(poses, labels=True)
        w_rec, w_lab, w_st, _ = render_ref.explain(poses, mpos, mnrm, depth, prob, K, scale)
        assert render_ref.records_equal(rec, w_rec) and np.array_equal(lab, w_lab) and np.array_equal(st, w_st), (label, n)
        rows.append({"workload": label, "n": n, "model_points": int(len(mpos)), "explain_poses": records, "explain_poses_with_labels": with_labels,
                     "depth_check_poses": depth_check, "numpy_restatement": dict(host, reps=host_reps), "equal_to_restatement": True,
                     "footprint_px": int(rec["footprint"].sum()), "visible_px": int(rec["visible"].sum()), "labelled_px": int((lab >= 0).sum())})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("render_time.py needs a GPU: no time is taken without one")
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    rows = []
    gold = os.path.join(ROOT, "tests", "golden")
    d = np.load(os.path.join(gold, "example_ycb_024_bowl.npz")); raw = np.load(os.path.join(gold, "example_ycb_024_bowl_raw.npz"))
    K, scale = [float(x) for x in raw["K"]], float(raw["depth_scale"])
    P0 = np.asarray(json.load(open(os.path.join(gold, "example_summary.json")))["ycb_024_bowl"]["best_pose16"], np.float64).reshape(4, 4).T
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=False)
    est.set_frame(raw["depth"], raw["prob"], K, scale)
    rows += measure("ycb_024_bowl", est, d["model_pos"], d["model_nrm"], raw["depth"], raw["prob"], K, scale, P0)
    est.close()
    m = synth.make_model_asym(5000)
    K, scale, W, H = (600.0, 319.5, 600.0, 239.5), 1e-4, 640, 480
    P0 = np.eye(4); P0[:3, :3] = _rot((1, 2, 3), 40); P0[:3, 3] = (0.03, -0.02, 0.6)
    depth = render(m.pos, m.nrm, P0, K, W, H, scale)
    prob = np.where(depth < 15000, 10000, 0).astype(np.uint16)
    rng = np.random.default_rng(3); sp = rng.normal(0, 0.05, (64, 3)).astype(np.float32)
    est = StocsEstimator(sp, sp / np.linalg.norm(sp, axis=1, keepdims=True), np.ones(64, np.float32), None, m.pos, m.nrm, build_index=False)
    est.set_frame(depth, prob, K, scale)
    rows += measure("synthetic_5000", est, m.pos, m.nrm, depth, prob, K, scale, P0)
    est.close()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "render.hip"], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    out = {"what": "host wall clock of explain_poses (clear, splat, resolve, [labels,] one read-back, one synchronisation) next to depth_check_poses of the "
                   "same poses and to the numpy restatement on the host",
           "device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM, "note": "one visit, one GPU; the host column shares the machine with other work",
           "kernel_resources": res.stdout.strip(), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
