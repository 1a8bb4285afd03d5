"""Cost of the self-distance scoring and of the symmetry search -> profiles/symmetry_time.json.

On the ycb-size model (the 472 points of the bowl example) and on synthetic Cm (5 000 points), medians of --reps after --warmup:
  symmetry_errors at K = 1, 64, 1 024 and the default search's coarse K (n_axes x (max_order - 1)), reach a tenth of the diameter:
    wall_ms      host wall clock of one call (upload, launches, read-back, one synchronisation);
    kernel_ms    HIP-event time of the call's launches (the "device_clock" option; a run of its own);
    brute_*      the yardstick, the capability the library had before: the same transforms through pose_errors(S, I), the brute-force
                 K x M^2 kernel, whose adds / adds_max are the unclamped mean and maximum of the same nearest-neighbour distances;
                 at the coarse K fewer transforms are timed when K x M^2 exceeds --brute-budget pairs, and the figure is scaled and marked;
    ratio_*      brute over grid: above 1 the grid form wins;
    agree        whether, for the transforms with no far point, max equals adds_max bit for bit (the same expressions);
  find_symmetries: the whole call at its defaults, wall clock only (it is several scoring calls and host logic).
The transforms are rotations about the search's own candidate axes through the centroid.  No GPU: the tool fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from model_matching_amd.estimator import StocsEstimator, symmetry_axes, symmetry_rotation, symmetry_search  # noqa: E402
from pose_error_time import median_ms, models  # noqa: E402

IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


def kernel_ms(est, call, which, warmup, reps):
    est.set_option("device_clock", 1)
    ms = []
    for _ in range(warmup + reps):
        call()
        ms.append(dict(est.last_call_timing(which))["device: kernel"])
    est.set_option("device_clock", 0)
    return statistics.median(ms[warmup:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,64,1024")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--brute-budget", type=float, default=3e10, help="largest K x M^2 the brute-force yardstick is timed at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "symmetry_time.json"))
    a = ap.parse_args()
    prm = symmetry_search()
    coarse = prm.n_axes * (prm.max_order - 1)
    dirs = symmetry_axes(prm.n_axes)
    rows, searches = [], []
    for name, sp, sn, spr, spx, mp, mn, _ in models():
        est = StocsEstimator(sp, sn, spr, spx, mp, mn, build_index=False)
        M = len(mp)
        reach = float(np.float32(0.1) * est.model_diameter())
        centre = np.asarray(mp, np.float64).mean(0).astype(np.float32)
        T_all = np.stack([symmetry_rotation(d, 360.0 / n, centre) for d in dirs for n in range(2, prm.max_order + 1)])
        for K in [int(x) for x in a.counts.split(",")] + [coarse]:
            T = T_all[:K]
            call = lambda: est.symmetry_errors(T, reach)
            wall = median_ms(call, a.warmup, a.reps)
            kern = kernel_ms(est, call, 6, a.warmup, a.reps)
            Kb = max(1, min(K, int(a.brute_budget / (float(M) * M))))
            brute = lambda: est.pose_errors(T[:Kb], IDENTITY)
            b_wall = median_ms(brute, a.warmup, a.reps) * (K / Kb)
            b_kern = kernel_ms(est, brute, 4, a.warmup, a.reps) * (K / Kb)
            got, want = call()[:Kb], brute()
            whole = got["n_far"] == 0
            rows.append({"model": name, "model_points": M, "transforms": K, "reach_m": reach, "wall_ms": round(wall, 4), "kernel_ms": round(kern, 4),
                         "brute_wall_ms": round(b_wall, 4), "brute_kernel_ms": round(b_kern, 4), "brute_transforms_timed": Kb, "brute_scaled": Kb < K,
                         "ratio_wall": b_wall / wall, "ratio_kernel": b_kern / kern, "transforms_without_far_points": int(whole.sum()),
                         "agree": bool(np.array_equal(got["max"][whole], want["adds_max"][whole]))})
            print(json.dumps(rows[-1]), flush=True)
        find = lambda: est.find_symmetries()
        wall = median_ms(find, a.warmup, a.reps)
        axes, S, sym3, flags = find()
        searches.append({"model": name, "model_points": M, "find_symmetries_wall_ms": round(wall, 3), "coarse_transforms": coarse,
                         "refine_transforms": int(prm.rounds * prm.n_refine * prm.n_local), "axes": len(axes), "set": len(S), "flags": flags})
        print(json.dumps(searches[-1]), flush=True)
        est.close()
    out = {"what": "stocs_symmetry_errors against the brute-force stocs_pose_errors(S, I) on the same transforms, and stocs_find_symmetries at its "
                   "defaults: medians of %d after %d warm-up calls" % (a.reps, a.warmup), "rows": rows, "find_symmetries": searches}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
