#!/usr/bin/env python3
"""Host wall clock of StocsEstimator.select_instances (stocs_select_instances: detail rows, marking, order, walk and records on the
device, one read-back, one synchronisation per call) for n = 10, 64, 256 and 700 hypotheses, on the packed example fixture and on a
synthetic frame of 20 000 scene points holding four copies of a 5 000-point model.  Next to each: (a) score_transforms of the same
hypotheses -- the floor, the call cannot beat its own scoring launch -- and (b) the only route the library had before: lcp_detail once
per hypothesis plus the numpy reference (tests/instances_ref.py) on the host.  Median of 20 calls after 5 warm-ups, with min and max.
The figure to read is the call's time over (a).  Needs a GPU; no fallback.

    python tools/instances_time.py [--out profiles/instances_time.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import instances_cases as cases  # noqa: E402
import instances_ref as ref  # noqa: E402

SIZES = (10, 64, 256, 700)
REPS, WARM = 20, 5
F = np.float32


def clock(fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "reps": reps}


def around(T0, n, seed, max_t=0.005, max_deg=5.0):
    """n centred-frame hypotheses: the given ones first, then perturbations of them in turn (what several trials of one frame return)"""
    from model_matching_amd import synth
    rng = np.random.default_rng(seed)
    out = [t for t in T0[:n]]
    k = 0
    while len(out) < n:
        A = T0[k % len(T0)].astype(np.float64).reshape(4, 4).T
        dR = synth._rot_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0, max_deg)))
        B = np.eye(4); B[:3, :3] = A[:3, :3] @ dR; B[:3, 3] = A[:3, 3] + rng.uniform(-max_t, max_t, 3)
        out.append(B.T.reshape(16))
        k += 1
    return np.ascontiguousarray(np.asarray(out, F))


def host_route(est, T):
    rows = [est.lcp_detail(t) for t in T]
    return ref.select(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), est.score_transforms(T))


def measure(label, est, T0):
    out = []
    for n in SIZES:
        T = around(T0, n, 100 + n)
        call = clock(lambda: est.select_instances(T))
        floor = clock(lambda: est.score_transforms(T))
        host = clock(lambda: host_route(est, T), reps=20 if n <= 64 else 3, warm=1)
        rec, sel = est.select_instances(T)
        want = host_route(est, T)
        assert ref.records_equal(rec, want[0]) and np.array_equal(sel, want[1])   # faster and different is not faster
        out.append({"workload": label, "n": n, "scene_points": est.nS, "model_points": est.nM, "select_instances": call, "score_transforms": floor,
                    "over_scoring": call["median_ms"] / floor["median_ms"], "lcp_detail_per_hypothesis_plus_numpy": host, "selected": int(len(sel)),
                    "mean_own": float(rec["own"].mean())})
        print(json.dumps(out[-1]), flush=True)
    return out


def synthetic_frame(seed=5):
    """20 000 scene points: four copies of make_model(5000) seen from the camera, and a lattice plane behind them"""
    from model_matching_amd import synth
    rng = np.random.default_rng(seed)
    model = synth.make_model(5000)
    pos, nrm, prob, poses = [], [], [], []
    for c in ([-0.30, -0.05, 0.85], [-0.08, 0.06, 0.80], [0.14, -0.04, 0.88], [0.36, 0.03, 0.83]):
        R = synth.random_rotation(rng)
        p = model.pos.astype(np.float64) @ R.T + np.array(c)
        k = model.nrm.astype(np.float64) @ R.T
        f = (k * (-p / np.linalg.norm(p, axis=1, keepdims=True))).sum(1) > 0.1
        pos.append(p[f] + rng.normal(0, 0.0005, p[f].shape)); nrm.append(synth._perturb_normals(rng, k[f], 5.0)); prob.append(np.full(f.sum(), 0.9))
        P = np.eye(4); P[:3, :3] = R; P[:3, 3] = c
        poses.append(P)
    n_cl = 20000 - sum(len(p) for p in pos)
    side = int(np.ceil(np.sqrt(n_cl)))
    ii, jj = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    plane = np.array([-0.5, -0.35, 1.15]) + 0.008 * np.stack([ii.ravel()[:n_cl], jj.ravel()[:n_cl], np.zeros(n_cl)], axis=1)
    pos.append(plane + rng.normal(0, 0.0003, plane.shape)); nrm.append(np.tile([0.0, 0.0, -1.0], (n_cl, 1))); prob.append(np.full(n_cl, 0.2))
    sp = np.concatenate(pos).astype(F)
    return model, sp, np.concatenate(nrm).astype(F), np.concatenate(prob).astype(F), synth._project(sp.astype(np.float64)), poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instances_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("instances_time.py needs a GPU: no time is taken without one")
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator, trial_post
    rows = []
    d = np.load(os.path.join(ROOT, "tests", "golden", "example_packed_dove.npz"))
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
    est.run_trials(list(range(8)), 100, max_per_base=200, post=trial_post())
    P = np.concatenate([est.trials_get_hypotheses(t)["pose16"] for t in range(8)]).astype(F).reshape(-1, 16)
    rows += measure("packed_dove", est, cases.centred_from_camera(P, est.get_scene_centroid(), est.get_model_centroid()))
    est.close()
    model, sp, sn, spr, spx, poses = synthetic_frame()
    est = StocsEstimator(sp, sn, spr, spx, model.pos, model.nrm, build_index=False)
    cs, cm = est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64)
    T0 = np.asarray([synth.centred_gt(Pc, cs, cm).T.reshape(16) for Pc in poses], F)
    rows += measure("synthetic_20000_5000_four_instances", est, T0)
    est.close()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "instances.hip"], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    out = {"what": "host wall clock of select_instances next to score_transforms of the same hypotheses (its floor) and to lcp_detail per hypothesis plus numpy",
           "device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM, "note": "one visit, one GPU; the host column shares the machine with other work",
           "kernel_resources": res.stdout.strip(), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
