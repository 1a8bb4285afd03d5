#!/usr/bin/env python3
"""Host wall clock of stocs_refine_poses (5 iterations, 3.5 cm) for 1, 10, 64 and 256 hypotheses on the ycb example frame and on
Cm, and of the same hypotheses through the stand-alone stocs_icp_point_to_plane one by one (the caller's alternative before
stocs_refine_poses; its source clouds are prepared outside the timing).  Measurement only.
usage: python tools/refine_time.py [out.json] [reps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("STOCS_PIN_BLAS", "1")
from model_matching_amd import synth  # noqa: E402
from model_matching_amd.estimator import StocsEstimator, cluster_poses, icp_point_to_plane  # noqa: E402

SIZES = (1, 10, 64, 256)


def perturb(T16, k, seed, max_t=0.005, max_deg=4.0):
    rng = np.random.default_rng(seed)
    T0 = np.asarray(T16, np.float64).reshape(4, 4).T
    out = np.zeros((k, 16), np.float32)
    for i in range(k):
        dR = synth._rot_axis_angle(rng.normal(size=3), np.radians(max_deg) * rng.uniform(-1, 1))
        d = rng.normal(size=3)
        T = np.eye(4)
        T[:3, :3] = T0[:3, :3] @ dR
        T[:3, 3] = T0[:3, 3] + d / np.linalg.norm(d) * rng.uniform(0, max_t)
        out[i] = T.T.reshape(16)
    return out


def hypotheses(name):
    """(estimator, model positions, model normals, 256 hypotheses): on ycb the clustered hypotheses of a seeded trial first"""
    if name == "ycb":
        d = np.load(os.path.join(ROOT, "tests", "golden", "example_ycb_024_bowl.npz"))
        est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
        est.sample_bases(7, 100)
        est.find_congruent_all()
        est.make_transforms(200, 7)
        best_lcp, best_idx, _ = est.compute_best_transform()
        T, P, l, b = est.get_pose_candidates()
        keep = cluster_poses(P, l, 0.8, best_lcp, 10, 0.02, 15.0, np.zeros(3, np.float32))
        H = np.concatenate([T[keep], perturb(T[best_idx], 256, 1)])[:256]
        return est, d["model_pos"], d["model_nrm"], H, len(keep)
    m, s, _ = synth.workload(name)
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    Tgt = synth.centred_gt(s.T_gt, est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64))
    return est, m.pos, m.nrm, perturb(Tgt.T.reshape(16), 256, 1), 0


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "refine_time.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rec = {"iterations": 5, "distance": 0.035, "reps": reps, "workloads": {}}
    for name in ("ycb", "Cm"):
        est, mpos, mnrm, H, n_clustered = hypotheses(name)
        scene_c = est.get_scene()[0]
        cm = est.get_model_centroid()
        model_c = (np.asarray(mpos, np.float32) - cm).astype(np.float32)
        w = {"nS": int(est.nS), "nM": int(est.nM), "n_clustered": n_clustered, "refine_ms": {}, "icp_one_by_one_ms": {}}
        for n in SIZES:
            h = H[:n]
            for _ in range(3):
                est.refine_poses(h)
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                est.refine_poses(h)
                t.append((time.perf_counter() - t0) * 1e3)
            w["refine_ms"][str(n)] = {"median": float(np.median(t)), "min": float(np.min(t))}
            # the stand-alone call, one hypothesis at a time, on the scene moved into the model frame
            srcs = []
            for k in range(n):
                Ti = np.linalg.inv(h[k].reshape(4, 4).T.astype(np.float64))
                srcs.append(np.ascontiguousarray((Ti[:3, :3] @ scene_c.T.astype(np.float64) + Ti[:3, 3:]).T.astype(np.float32)))
            icp_point_to_plane(srcs[0], model_c, mnrm, 5, 0.035)
            t0 = time.perf_counter()
            for k in range(n):
                icp_point_to_plane(srcs[k], model_c, mnrm, 5, 0.035)
            w["icp_one_by_one_ms"][str(n)] = (time.perf_counter() - t0) * 1e3
            print(name, n, "refine %.3f ms (min %.3f)" % (w["refine_ms"][str(n)]["median"], w["refine_ms"][str(n)]["min"]),
                  "icp one by one %.3f ms" % w["icp_one_by_one_ms"][str(n)], flush=True)
        rec["workloads"][name] = w
        est.close()
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
