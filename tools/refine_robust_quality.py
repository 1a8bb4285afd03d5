#!/usr/bin/env python3
"""Pose quality of the refinement's forms on the synthetic workloads with a known pose: ADD and ADD-S (stocs_pose_errors, mm) before
and after 5 iterations at 3.5 cm of the plain form, keep 0.7 alone, a 30 degree gate alone, and both -- on Cm_asym and Cm, for the
first two tiers of synth.make_candidates (within 1 mm / 1 degree, within 1 cm / 5 degrees of the truth) and for 64 trial winners (the
best pose of 64 seeded trials).  Measurement only.
usage: python tools/refine_robust_quality.py [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("STOCS_PIN_BLAS", "1")
from model_matching_amd import synth  # noqa: E402
from model_matching_amd.estimator import StocsEstimator  # noqa: E402

FORMS = (("plain", 1.0, None), ("keep_0.7", 0.7, None), ("gate_30deg", 1.0, 30.0), ("keep_0.7_gate_30deg", 0.7, 30.0))
N_TIER = 64


def tiers(Tgt):
    """the first N_TIER candidates of make_candidates' first tier (1 mm, 1 degree) and of its second (1 cm, 5 degrees): the tier draw
    is the generator's first, so it is recomputed here"""
    k = 65536
    H = synth.make_candidates(Tgt, k)
    tier = np.random.Generator(np.random.PCG64(synth.SEED_CAND)).random(k)
    return {"tier_1mm_1deg": H[tier < 0.01][:N_TIER], "tier_1cm_5deg": H[(tier >= 0.01) & (tier < 0.10)][:N_TIER]}


def winners(est, n=64, seed0=100):
    """centred hypotheses of the best pose of n seeded trials"""
    out = []
    for t in range(n):
        est.sample_bases(seed0 + t, 100)
        est.find_congruent_all()
        est.make_transforms(200, seed0 + t)
        best_lcp, best_idx, _ = est.compute_best_transform()
        if best_idx >= 0:
            out.append(est.get_pose_candidates()[0][best_idx])
    return np.array(out, np.float32).reshape(-1, 16)


def stats(v):
    v = np.asarray(v, np.float64) * 1e3
    return {"median_mm": float(np.median(v)), "mean_mm": float(v.mean()), "max_mm": float(v.max())}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "refine_robust_quality.json")
    rec = {"iterations": 5, "distance": 0.035, "workloads": {}}
    for name in ("Cm_asym", "Cm"):
        m, s, _ = synth.workload(name)
        est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
        Tgt = synth.centred_gt(s.T_gt, est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64))
        gt = np.asarray(s.T_gt, np.float64).T.reshape(16).astype(np.float32)
        sets = tiers(Tgt)
        sets["trial_winners"] = winners(est)
        w = {}
        for sname, H in sets.items():
            if len(H) == 0:
                continue
            row = {"n": int(len(H))}
            P0 = est.refine_poses_robust(H, 0)[1]
            e = est.pose_errors(P0, gt)
            row["before"] = {"add": stats(e["add"]), "adds": stats(e["adds"]), "lcp_median": float(np.median(est.score_transforms(H)))}
            for form, keep, deg in FORMS:
                To, Po, lcp, nc, ncand, it = est.refine_poses_robust(H, 5, 0.035, keep, deg)
                e = est.pose_errors(Po, gt)
                row[form] = {"add": stats(e["add"]), "adds": stats(e["adds"]), "lcp_median": float(np.median(lcp)), "kept_median": float(np.median(nc)),
                             "candidates_median": float(np.median(ncand))}
            w[sname] = row
            print(name, sname, len(H), "ADD median mm: before %.2f" % row["before"]["add"]["median_mm"],
                  " ".join("%s %.2f" % (f[0], row[f[0]]["add"]["median_mm"]) for f in FORMS), flush=True)
        rec["workloads"][name] = w
        est.close()
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
