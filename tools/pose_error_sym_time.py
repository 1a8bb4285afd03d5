"""Cost of the symmetry-aware pose errors (stocs_pose_errors_sym) -> profiles/pose_error_sym_time.json.

For 1, 64, 1 024 and 8 192 pairs, 1, 8 and 72 symmetries, with and without projection, on the ycb-size model (the 472 points of the bowl
example) and on synthetic Cm (5 000 points):
  wall_ms      host wall clock of one pose_errors_sym call (upload, three launches, read-back, one synchronisation), median of --reps
               after --warmup;
  kernel_ms    HIP-event time of the call's launches (the "device_clock" option; a run of its own), median of --reps;
  evals_per_s  point evaluations (pairs x K x M) over kernel_ms, and the share of the chip's non-FMA fp32 vector rate they stand for:
               157.3 TFLOP/s counts an FMA as two, so 78.6e12 single operations per second; 17 per point and symmetry without projection
               (9 of the transform, 8 of the distance), the root, the fixed point and the projection's divisions not counted;
  host_ms      the same inputs through a float64 numpy method (compose, transform, norms, maxima and means per symmetry), median of
               --host-reps; fewer pairs are timed when one repetition would take more than --host-budget seconds, and the figure is then
               scaled and marked.
The symmetry sets are symmetry_set((0, 0, 360), K); the estimates are the ground truth disturbed by up to 10 degrees and 1 cm.  The
kernel's cost does not depend on the poses.  No GPU: the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from model_matching_amd import synth  # noqa: E402
from model_matching_amd.estimator import StocsEstimator, symmetry_set  # noqa: E402
from pose_error_time import disturbed, median_ms, models  # noqa: E402

PEAK_NON_FMA_OPS = 157.3e12 / 2
OPS_PER_EVAL = 17
CAMERA = synth.YCB_INTRINSICS


def host_method(model_pos, T_gt, syms, cam):
    """-> fn(est16 (n, 16)) -> (mssd, add, mspd) per pair in float64"""
    m = model_pos.astype(np.float64)
    G = np.asarray(T_gt, np.float64)
    comp = [G @ np.asarray(S, np.float64).reshape(4, 4).T for S in syms]
    gk = [m @ Cm[:3, :3].T + Cm[:3, 3] for Cm in comp]

    def proj(x):
        return np.stack([cam[0] * x[:, 0] / x[:, 2] + cam[1], cam[2] * x[:, 1] / x[:, 2] + cam[3]], 1)
    gp = [proj(g) for g in gk] if cam is not None else None

    def run(est16):
        out = np.empty((len(est16), 3))
        for i, P16 in enumerate(est16):
            P = P16.reshape(4, 4).T.astype(np.float64)
            p = m @ P[:3, :3].T + P[:3, 3]
            e = [np.linalg.norm(p - g, axis=1) for g in gk]
            out[i, 0] = min(x.max() for x in e)
            out[i, 1] = min(x.mean() for x in e)
            out[i, 2] = np.inf
            if cam is not None:
                pp = proj(p)
                out[i, 2] = min(np.linalg.norm(pp - q, axis=1).max() for q in gp)
        return out
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,64,1024,8192")
    ap.add_argument("--symmetries", default="1,8,72")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-budget", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_error_sym_time.json"))
    a = ap.parse_args()
    rows = []
    for name, sp, sn, spr, spx, mp, mn, T_gt in models():
        est = StocsEstimator(sp, sn, spr, spx, mp, mn, build_index=False)
        M = len(mp)
        if T_gt is None:
            T_gt = np.eye(4); T_gt[:3, :3] = synth._rot_axis_angle(np.array([1.0, 2.0, 3.0]), 0.7); T_gt[:3, 3] = (0.02, -0.03, 0.8)
        gt16 = np.asarray(T_gt, np.float64).T.reshape(16).astype(np.float32)
        for K in [int(x) for x in a.symmetries.split(",")]:
            S = symmetry_set((0, 0, 360), K)
            for cam in (None, CAMERA):
                host = host_method(np.asarray(mp), T_gt, S, cam)
                for n in [int(x) for x in a.pairs.split(",")]:
                    E = disturbed(T_gt, n, 100 + n)
                    call = lambda: est.pose_errors_sym(E, gt16, S, cam)
                    est.set_option("device_clock", 0)
                    wall = median_ms(call, a.warmup, a.reps)
                    est.set_option("device_clock", 1)
                    kern = []
                    for _ in range(a.warmup + a.reps):
                        call()
                        kern.append(dict(est.last_call_timing(5))["device: kernel"])
                    kernel_ms = statistics.median(kern[a.warmup:])
                    est.set_option("device_clock", 0)
                    got = call()
                    t0 = time.perf_counter(); host(E[:1]); one = time.perf_counter() - t0
                    n_host = max(1, min(n, int(a.host_budget / max(one, 1e-6) / max(a.host_reps, 1))))
                    host_ms = median_ms(lambda: host(E[:n_host]), 0, a.host_reps) * (n / n_host)
                    h = host(E[:min(n, 4)])
                    evals = float(n) * K * M
                    rows.append({
                        "model": name, "model_points": M, "pairs": n, "symmetries": K, "projection": cam is not None, "point_evaluations": evals,
                        "wall_ms": round(wall, 4), "kernel_ms": round(kernel_ms, 4),
                        "evals_per_s_kernel": evals / (kernel_ms * 1e-3), "evals_per_s_wall": evals / (wall * 1e-3),
                        "share_of_non_fma_fp32_rate": evals * OPS_PER_EVAL / (kernel_ms * 1e-3) / PEAK_NON_FMA_OPS,
                        "host_ms": round(host_ms, 3), "host_pairs_timed": n_host, "host_scaled": n_host < n, "host_over_wall": host_ms / wall,
                        "max_abs_mssd_diff_vs_host_m": float(np.abs(got["mssd"][:len(h)] - h[:, 0]).max()),
                        "max_abs_add_diff_vs_host_m": float(np.abs(got["add"][:len(h)] - h[:, 1]).max()),
                        "max_abs_mspd_diff_vs_host_px": float(np.abs(got["mspd"][:len(h)] - h[:, 2]).max()) if cam is not None else None})
                    print(json.dumps(rows[-1]), flush=True)
        est.close()
    out = {"what": "stocs_pose_errors_sym: host wall clock and HIP-event kernel time per call, medians of %d after %d warm-up calls" % (a.reps, a.warmup),
           "peak_non_fma_fp32_ops_per_s": PEAK_NON_FMA_OPS, "ops_per_point_evaluation_without_projection": OPS_PER_EVAL, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
