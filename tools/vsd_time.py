#!/usr/bin/env python3
"""Host wall clock of StocsEstimator.pose_errors_vsd (stocs_pose_errors_vsd: surfel renders, one compare pass per pair, one read-back,
one synchronisation per call) for 1, 16, 64 and 256 pairs, with one ground truth for all (n_gt = 1) and one each (n_gt = n), on the ycb
example fixture (472-point model on its own 640 x 480 depth image) and on synth:Cm (5 000 points at synth.gt_pose() on a 640 x 480 frame
rendered from it, wall at 1.5 m).  Next to it the host baseline: the float32 numpy restatement (tests/vsd_ref.py) on ONE pair.  Median
of 20 calls after warm-up, with the spread (min, max), and the HIP-event time of the launches of one more call.  No time is promised.
Needs a GPU; no fallback.

    python tools/vsd_time.py [--out profiles/vsd_time.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from depth_check_time import clock, perturbed  # noqa: E402

SIZES = (1, 16, 64, 256)
REPS, WARM = 20, 5


def device_ms(est):
    """the "device: kernel" entry of the last call's timing (stocs_last_call_timing, which = 7)"""
    labels = (C.c_char_p * 18)(); ms = (C.c_double * 18)(); n = C.c_int(0)
    est.L.stocs_last_call_timing(est.h, 7, labels, ms, 18, C.byref(n))
    for i in range(n.value):
        if labels[i].decode() == "device: kernel":
            return float(ms[i])
    return None


def measure(label, est, mpos, mnrm, depth, K, scale, P0):
    import vsd_ref as ref
    rows = []
    gt = np.asarray(P0, np.float64).T.reshape(16).astype(np.float32)
    dia = np.float32(est.model_diameter())
    taus = [np.float32(0.05 * i) * dia for i in range(1, 11)]
    one = perturbed(P0, 1, 99)
    host = clock(lambda: ref.pose_errors_vsd(one, gt, mpos, mnrm, depth, K, scale, taus), reps=5, warm=1)
    for n in SIZES:
        poses = perturbed(P0, n, 100 + n)
        for n_gt in (1, n):
            G = gt if n_gt == 1 else np.tile(gt, (n, 1))
            gpu = clock(lambda: est.pose_errors_vsd(poses, G, taus))
            est.set_option("device_clock", 1)
            rec = est.pose_errors_vsd(poses, G, taus)
            dev = device_ms(est)
            est.set_option("device_clock", 0)
            rows.append({"workload": label, "pairs": n, "n_gt": n_gt, "model_points": int(len(mpos)), "gpu": gpu, "device_kernels_ms": dev,
                         "host_numpy_restatement_one_pair": dict(host, reps=5), "mean_e_tau_0.20": float(rec["e"][:, 3].mean()),
                         "mean_union_px": float(rec["uni"].mean())})
            print(json.dumps(rows[-1]), flush=True)
            if n == 1:
                break                                      # n_gt = n is the same call
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vsd_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vsd_time.py needs a GPU: no time is taken without one")
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    rows = []
    gold = os.path.join(ROOT, "tests", "golden")
    d = np.load(os.path.join(gold, "example_ycb_024_bowl.npz")); raw = np.load(os.path.join(gold, "example_ycb_024_bowl_raw.npz"))
    K, scale = [float(x) for x in raw["K"]], float(raw["depth_scale"])
    P0 = np.asarray(json.load(open(os.path.join(gold, "example_summary.json")))["ycb_024_bowl"]["best_pose16"], np.float64).reshape(4, 4).T
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=False)
    est.set_frame(raw["depth"], raw["prob"], K, scale)
    rows += measure("ycb_024_bowl", est, d["model_pos"], d["model_nrm"], raw["depth"], K, scale, P0)
    est.close()
    m = synth.make_model(5000)
    K, scale = [float(v) for v in synth.YCB_INTRINSICS], 1e-4
    P0 = synth.gt_pose()
    rng = np.random.default_rng(3); sp = rng.normal(0, 0.05, (64, 3)).astype(np.float32)
    est = StocsEstimator(sp, sp / np.linalg.norm(sp, axis=1, keepdims=True), np.ones(64, np.float32), None, m.pos, m.nrm, build_index=False)
    est.set_frame(np.zeros((480, 640), np.uint16), None, K, scale)     # the camera alone: the renderer reads no depth
    z = est.render_depth(P0.T.reshape(16).astype(np.float32))[0]
    depth = np.rint(np.where(z > 0, z, 1.5) / scale).astype(np.uint16)
    est.set_frame(depth, None, K, scale)
    rows += measure("synth:Cm", est, m.pos, m.nrm, depth, K, scale, P0)
    est.close()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "vsd.hip"], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    out = {"what": "host wall clock of pose_errors_vsd (renders, one compare pass per pair, one read-back, one synchronisation) next to the numpy restatement on one pair",
           "device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM, "note": "one visit, one GPU; the host column shares the machine with other work",
           "kernel_resources": res.stdout.strip(), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
