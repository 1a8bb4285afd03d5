#!/usr/bin/env python3
"""Host wall clock of StocsEstimator.depth_check_poses (stocs_depth_check_poses: one launch, one read-back, one synchronisation per
call) for n = 1, 10, 64 and 700 hypotheses, on the ycb example fixture (472-point model) and on a 5 000-point synthetic model against
a 640 x 480 frame rendered from it; next to it the only route the library had before: tools/pose_check.py::depth_agreement (numpy,
float64) once per hypothesis on the host.  Median of 20 calls after warm-up, with the spread (min, max).  Needs a GPU; no fallback.

    python tools/depth_check_time.py [--out profiles/depth_check_time.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_check import depth_agreement  # noqa: E402

SIZES = (1, 10, 64, 700)
REPS, WARM = 20, 5


def _rot(axis, deg):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def perturbed(P0, n, seed):
    """n hypotheses around the 4x4 pose P0: <= 10 degrees about the object's position, <= 2 cm (what a clustered trial batch looks like)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        T = np.eye(4)
        T[:3, :3] = _rot(rng.normal(size=3), rng.uniform(0, 10))
        c = P0[:3, 3]
        T[:3, 3] = c - T[:3, :3] @ c + rng.uniform(-0.02, 0.02, 3)
        out.append((T @ P0).T.reshape(16))
    return np.asarray(out, np.float32)


def render(pos, nrm, P, K, W, H, scale, r=2):
    p = pos.astype(np.float64) @ P[:3, :3].T + P[:3, 3]
    q = nrm.astype(np.float64) @ P[:3, :3].T
    p = p[((q * p).sum(1) < 0) & (p[:, 2] > 1e-6)]
    col = np.floor(K[0] * p[:, 0] / p[:, 2] + K[1] + 0.5).astype(int); row = np.floor(K[2] * p[:, 1] / p[:, 2] + K[3] + 0.5).astype(int)
    z = np.full((H, W), np.inf)
    for dr in range(-r, r + 1):
        for dc in range(-r, r + 1):
            rr, cc = row + dr, col + dc
            ok = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
            np.minimum.at(z, (rr[ok], cc[ok]), p[ok, 2])
    z[~np.isfinite(z)] = 1.5
    return np.round(z / scale).astype(np.uint16)


def clock(fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))}


def measure(label, est, mpos, mnrm, depth, prob, K, scale, P0):
    rows = []
    for n in SIZES:
        poses = perturbed(P0, n, 100 + n)
        gpu = clock(lambda: est.depth_check_poses(poses))
        host_reps = 20 if n <= 64 else 3        # 700 hypotheses on the host take seconds per pass
        host = clock(lambda: [depth_agreement(p.reshape(4, 4).T, mpos, mnrm, depth, prob, K, scale) for p in poses], reps=host_reps, warm=1)
        rec = est.depth_check_poses(poses)
        rows.append({"workload": label, "n": n, "model_points": int(len(mpos)), "gpu": gpu, "host_depth_agreement": dict(host, reps=host_reps),
                     "mean_score": float(rec["score"].mean()), "mean_violation": float(rec["violation"].mean())})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_check_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("depth_check_time.py needs a GPU: no time is taken without one")
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
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "depth.hip"], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    out = {"what": "host wall clock of depth_check_poses (one launch, one read-back, one synchronisation) next to depth_agreement per hypothesis on the host",
           "device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM, "note": "one visit, one GPU; the host column shares the machine with other work",
           "kernel_resources": res.stdout.strip(), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
