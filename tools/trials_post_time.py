#!/usr/bin/env python3
"""Host wall clock of a 64-trial batch with and without its post-processing, on the ycb, linemod and packed (instance
mode) example frames and on Cm:
  (a) run_trials alone;
  (b) run_trials with the clustering inside the batch (stocs_run_trials_post, refine_iterations 0);
  (c) (b) + 5 refine iterations of the kept hypotheses;
  (d) the route before it: run_trials with keep_details, host stocs_cluster_poses per trial, one stocs_refine_poses on all kept
      hypotheses;
  (e) with --robust keep[,deg]: (c) with the robust refinement inside the batch (stocs_run_trials_post_robust), next to (a) and (c)
      in the same process -- only these three forms are timed then, and the record (default profiles/trials_post_robust_time.json)
      carries trials/s of (c) and (e), their ratio, the groups the batch refined its slots in and the robust workspace's bytes;
plus stocs_refine_poses alone on the hypotheses (c) kept.  Clustering: 0.8, 10, 2 cm, 15 degrees, no symmetry (stocs_single
--cluster 1); refinement: 5 iterations, 3.5 cm.  Medians over reps after a warm-up.  Measurement only.
usage: python tools/trials_post_time.py [out.json] [reps] [--robust keep[,deg]]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("STOCS_PIN_BLAS", "1")
from model_matching_amd import synth  # noqa: E402
from model_matching_amd.estimator import StocsEstimator, cluster_poses, trial_post  # noqa: E402

N_TRIALS, N_ATTEMPTS, MAX_PER_BASE = 64, 100, 200
FRAMES = {"ycb": "ycb_024_bowl", "linemod": "linemod_obj_06", "packed": "packed_dove"}


def estimator(name):
    if name == "Cm":
        m, s, _ = synth.workload("Cm")
        return StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True), 0
    d = np.load(os.path.join(ROOT, "tests", "golden", "example_%s.npz" % FRAMES[name]))
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
    mode = 0
    if "edge_map" in d.files:
        est.set_edge_map(d["edge_map"])
        mode = 1
    return est, mode


def timed(fn, reps):
    for _ in range(2):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(t)), "min": float(np.min(t))}


def robust_option(argv):
    """--robust keep[,deg] taken out of argv -> dict(keep_ratio, max_normal_deg) or None"""
    if "--robust" not in argv:
        return None
    i = argv.index("--robust")
    v = argv[i + 1].split(",")
    del argv[i:i + 2]
    return dict(keep_ratio=float(v[0]), max_normal_deg=float(v[1]) if len(v) > 1 else None)


def main():
    argv = list(sys.argv)
    robust = robust_option(argv)
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "trials_post_robust_time.json" if robust else "trials_post_time.json")
    reps = int(argv[2]) if len(argv) > 2 else 10
    seeds = list(range(1000, 1000 + N_TRIALS))
    cl = dict(acceptable_fraction=0.8, maximum_pose_count=10, min_distance=0.02, min_angle=15.0, sym3=(0.0, 0.0, 0.0), max_correspondence_distance=0.035)
    rec = {"trials": N_TRIALS, "attempts": N_ATTEMPTS, "max_per_base": MAX_PER_BASE, "clustering": cl, "refine_iterations": 5, "reps": reps,
           "workloads": {}}
    for name in ("ycb", "linemod", "packed", "Cm"):
        est, mode = estimator(name)
        run = lambda **kw: est.run_trials(seeds, N_ATTEMPTS, mode=mode, max_per_base=MAX_PER_BASE, **kw)  # noqa: E731
        p_cluster, p_refine = trial_post(refine_iterations=0, **cl), trial_post(refine_iterations=5, **cl)

        def host_route():
            res = run(keep_details=True)
            H = []
            for t in range(N_TRIALS):
                T, P, l, b = est.trial_candidates(t)
                keep = cluster_poses(P, l, 0.8, res[t]["best_lcp"], 10, 0.02, 15.0, np.zeros(3, np.float32))
                H.append(T[keep])
            H = np.concatenate(H)
            if len(H):
                est.refine_poses(H, 5, 0.035)
            return H

        w = {"nS": int(est.nS), "nM": int(est.nM), "mode": "instance" if mode else "class"}
        # (a)-(d) interleaved, after a warm-up of each: the scene's state (its LCP distance field, filled once enough has been scored
        # against it) is then the same for all four
        forms = {"a_run_trials_ms": lambda: run(), "b_with_clustering_ms": lambda: run(post=p_cluster),
                 "c_with_clustering_refine5_ms": lambda: run(post=p_refine), "d_keep_details_host_cluster_refine_ms": host_route}
        if robust:
            forms = {"a_run_trials_ms": forms["a_run_trials_ms"], "c_with_clustering_refine5_ms": forms["c_with_clustering_refine5_ms"],
                     "e_with_clustering_robust_refine5_ms": lambda: run(post=p_refine, robust=robust)}
        for _ in range(3):
            for f in forms.values():
                f()
        times = {k: [] for k in forms}
        for _ in range(reps):
            for k, f in forms.items():
                t0 = time.perf_counter()
                f()
                times[k].append((time.perf_counter() - t0) * 1e3)
        for k, t in times.items():
            w[k] = {"median": float(np.median(t)), "min": float(np.min(t))}
        if robust:
            res = run(post=p_refine, robust=robust)
            H = [est.trials_get_hypotheses(t) for t in range(N_TRIALS)]
            w["robust"] = robust
            w["candidates"] = int(sum(r["n_candidates"] for r in res))
            w["hypotheses"] = int(sum(len(h) for h in H))
            w["hypotheses_moved"] = int(sum(int((h["iterations"] > 0).sum()) for h in H))
            w["hypotheses_refined_lcp_up"] = int(sum(int((h["refined_lcp"] > h["lcp"]).sum()) for h in H))
            w["robust_groups"] = next(v for k, v in est.last_call_timing(3) if k.startswith("robust refinement: groups"))
            w["robust_workspace_bytes"] = est.refine_robust_workspace()[1]
            c_ms, e_ms = w["c_with_clustering_refine5_ms"]["median"], w["e_with_clustering_robust_refine5_ms"]["median"]
            w["plain_trials_per_s"] = N_TRIALS / c_ms * 1e3
            w["robust_trials_per_s"] = N_TRIALS / e_ms * 1e3
            w["robust_over_plain_call"] = e_ms / c_ms
            w["robust_over_plain_refinement_part"] = (e_ms - w["a_run_trials_ms"]["median"]) / (c_ms - w["a_run_trials_ms"]["median"])
            print(name, json.dumps(w), flush=True)
            rec["workloads"][name] = w
            est.close()
            continue
        res = run(post=p_refine)
        H = [est.trials_get_hypotheses(t) for t in range(N_TRIALS)]
        w["candidates"] = int(sum(r["n_candidates"] for r in res))
        w["hypotheses"] = int(sum(len(h) for h in H))
        w["hypotheses_moved"] = int(sum(int((h["iterations"] > 0).sum()) for h in H))
        w["hypotheses_refined_lcp_up"] = int(sum(int((h["refined_lcp"] > h["lcp"]).sum()) for h in H))
        Hd = host_route()
        assert len(Hd) == w["hypotheses"]
        w["refine_poses_alone_ms"] = timed(lambda: est.refine_poses(Hd, 5, 0.035), reps) if len(Hd) else None
        w["b_minus_a_ms"] = w["b_with_clustering_ms"]["median"] - w["a_run_trials_ms"]["median"]
        w["c_minus_a_ms"] = w["c_with_clustering_refine5_ms"]["median"] - w["a_run_trials_ms"]["median"]
        w["d_over_c"] = w["d_keep_details_host_cluster_refine_ms"]["median"] / w["c_with_clustering_refine5_ms"]["median"]
        print(name, json.dumps(w), flush=True)
        rec["workloads"][name] = w
        est.close()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
