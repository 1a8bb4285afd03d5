"""Cost of the pose errors (stocs_pose_errors) -> profiles/pose_error_time.json.

For 1, 64, 1 024 and 8 192 pairs, on the ycb-size model (the 472 points of the bowl example) and on synthetic Cm (5 000 points):
  wall_ms      host wall clock of one pose_errors call (upload, launch, read-back, one synchronisation), median of --reps after --warmup;
  kernel_ms    HIP-event time of the call's launches (the "device_clock" option; a run of its own, the events cost a few microseconds),
               median of --reps;
  evals_per_s  distance evaluations (pairs x M x M) over kernel_ms, next to the chip's non-FMA fp32 vector rate: 157.3 TFLOP/s counts an
               FMA as two, so 78.6e12 single operations per second, nine per evaluation (3 sub, 3 mul, 2 add, 1 compare-select);
  host_ms      bench.py's method on the same inputs: a kd-tree over the ground-truth points, one query per estimate, float64 products
               (scipy's cKDTree when importable, else brute force in numpy chunks), median of --host-reps (fewer pairs are timed when one
               repetition would take more than --host-budget seconds; the figure is then scaled and marked).
The poses: ground truth the workload's own, estimates the ground truth disturbed by up to 10 degrees and 1 cm (what a trial batch's winners
look like); the kernel's cost does not depend on them.  No GPU: the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from model_matching_amd import synth  # noqa: E402
from model_matching_amd.estimator import StocsEstimator  # noqa: E402

PEAK_NON_FMA_OPS = 157.3e12 / 2
OPS_PER_EVAL = 9


def disturbed(T_gt, n, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 16), np.float32)
    for i in range(n):
        Q = np.array(T_gt, np.float64)
        Q[:3, :3] = Q[:3, :3] @ synth._rot_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0, 10)))
        Q[:3, 3] += rng.normal(0, 0.01 / np.sqrt(3), 3)
        out[i] = Q.T.reshape(16).astype(np.float32)
    return out


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def host_method(model_pos, T_gt):
    """-> fn(est16 (n, 16)) -> (add, adds) in metres, and the name of the nearest-neighbour search used"""
    m = model_pos.astype(np.float64)
    gt_pts = m @ T_gt[:3, :3].T + T_gt[:3, 3]
    try:
        from scipy.spatial import cKDTree
        tree, how = cKDTree(gt_pts), "scipy cKDTree"
        nearest = lambda p: tree.query(p)[0]
    except ImportError:
        how = "numpy brute force in chunks"

        def nearest(p):
            out = np.empty(len(p))
            for a in range(0, len(p), 256):
                out[a:a + 256] = np.sqrt(((p[a:a + 256, None, :] - gt_pts[None, :, :]) ** 2).sum(-1).min(1))
            return out

    def run(est16):
        add, adds = np.empty(len(est16)), np.empty(len(est16))
        for k, P16 in enumerate(est16):
            P = P16.reshape(4, 4).T.astype(np.float64)
            p = m @ P[:3, :3].T + P[:3, 3]
            adds[k] = nearest(p).mean()
            add[k] = np.linalg.norm(p - gt_pts, axis=1).mean()
        return add, adds
    return run, how


def models():
    d = np.load(os.path.join(ROOT, "tests", "golden", "example_ycb_024_bowl.npz"))
    yield "ycb_024_bowl", d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], None
    m, s, _ = synth.workload("Cm")
    yield "Cm", s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, s.T_gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,64,1024,8192")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-budget", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_error_time.json"))
    a = ap.parse_args()
    pairs = [int(x) for x in a.pairs.split(",")]
    rows = []
    for name, sp, sn, spr, spx, mp, mn, T_gt in models():
        est = StocsEstimator(sp, sn, spr, spx, mp, mn, build_index=False)
        M = len(mp)
        if T_gt is None:   # the example frames carry no ground truth: a pose in front of the camera serves (the cost does not depend on it)
            T_gt = np.eye(4); T_gt[:3, :3] = synth._rot_axis_angle(np.array([1.0, 2.0, 3.0]), 0.7); T_gt[:3, 3] = (0.02, -0.03, 0.8)
        gt16 = np.asarray(T_gt, np.float64).T.reshape(16).astype(np.float32)
        host, how = host_method(np.asarray(mp), np.asarray(T_gt, np.float64))
        diameter = float(est.model_diameter())
        for n in pairs:
            E = disturbed(T_gt, n, 100 + n)
            est.set_option("device_clock", 0)
            wall = median_ms(lambda: est.pose_errors(E, gt16), a.warmup, a.reps)
            est.set_option("device_clock", 1)
            kern = []
            for _ in range(a.warmup + a.reps):
                est.pose_errors(E, gt16)
                kern.append(dict(est.last_call_timing(4))["device: kernel"])
            kernel_ms = statistics.median(kern[a.warmup:])
            est.set_option("device_clock", 0)
            got = est.pose_errors(E, gt16)
            # the host method, on as many of the pairs as the budget allows
            t0 = time.perf_counter(); host(E[:1]); one = time.perf_counter() - t0
            n_host = max(1, min(n, int(a.host_budget / max(one, 1e-6) / max(a.host_reps, 1))))
            host_ms = median_ms(lambda: host(E[:n_host]), 1, a.host_reps) * (n / n_host)
            h_add, h_adds = host(E[:min(n, 8)])
            evals = float(n) * M * M
            rows.append({
                "model": name, "model_points": M, "pairs": n, "distance_evaluations": evals,
                "wall_ms": round(wall, 4), "kernel_ms": round(kernel_ms, 4),
                "evals_per_s_kernel": evals / (kernel_ms * 1e-3), "evals_per_s_wall": evals / (wall * 1e-3),
                "share_of_non_fma_fp32_rate": evals * OPS_PER_EVAL / (kernel_ms * 1e-3) / PEAK_NON_FMA_OPS,
                "host_ms": round(host_ms, 3), "host_pairs_timed": n_host, "host_scaled": n_host < n, "host_search": how,
                "host_over_wall": host_ms / wall,
                "max_abs_add_diff_vs_host_m": float(np.abs(got["add"][:len(h_add)] - h_add).max()),
                "max_abs_adds_diff_vs_host_m": float(np.abs(got["adds"][:len(h_adds)] - h_adds).max()),
                "model_diameter_m": diameter})
            print(json.dumps(rows[-1]), flush=True)
        est.close()
    out = {"what": "stocs_pose_errors: host wall clock and HIP-event kernel time per call, medians of %d after %d warm-up calls" % (a.reps, a.warmup),
           "peak_non_fma_fp32_ops_per_s": PEAK_NON_FMA_OPS, "ops_per_distance_evaluation": OPS_PER_EVAL, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
