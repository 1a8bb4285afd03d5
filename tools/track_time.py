"""Cost and accuracy of pose tracking (stocs_track_poses) -> profiles/track_time.json.

cost: host wall clock of one tracking call on the ycb and linemod example frames and synthetic Cm, with 1 and 8 priors, with and
  without refinement (5 iterations, 3.5 cm), next to one trial and a 64-trial batch (stocs_run_trials) on the same frame; medians of
  --reps calls after --warmup.
sweep: rounds x samples (x shrink) on synthetic motion sequences (synth.motion_sequence: up to 1.5 cm and 8 degrees per frame; the
  tracker starts from frame 0's ground truth, then from its own previous pose): worst translation / rotation error against the ground
  truth, frames within 5 mm and 3 degrees, median wall clock of a call.  The defaults are the cheapest setting that keeps the most frames
  (ideally all) of every sequence within 5 mm and 3 degrees.
also: the lcp of a prior 30 cm behind the object (the driver's fallback threshold), and the ycb check of tests/test_track_gpu.py
  (a 64-trial winner moved by 1 cm and 5 degrees, tracked with the defaults).
--robust keep[,deg]: only the cost of the robust refinement behind the tracker (stocs_track_poses_robust) against the plain one in the
  same process: 1, 10 and 64 priors on ycb and Cm, 5 iterations at 3.5 cm -> profiles/track_robust_time.json (unless --out names another)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from model_matching_amd import synth  # noqa: E402
from model_matching_amd.estimator import StocsEstimator, TRACK_DEFAULTS  # noqa: E402


def pose_err(P16, T):
    P = np.asarray(P16, np.float64).reshape(4, 4).T
    dR = P[:3, :3].T @ np.asarray(T)[:3, :3]
    return float(np.linalg.norm(P[:3, 3] - T[:3, 3])) * 1e3, math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2))))


def perturbed(P16, k, seed, max_t, max_deg, exact=False):
    rng = np.random.default_rng(seed)
    P = np.asarray(P16, np.float64).reshape(4, 4).T
    out = np.zeros((k, 16), np.float32)
    for i in range(k):
        ang = math.radians(max_deg) * (1.0 if exact else rng.uniform(0, 1))
        d = rng.normal(size=3)
        Q = np.eye(4)
        Q[:3, :3] = P[:3, :3] @ synth._rot_axis_angle(rng.normal(size=3), ang)
        Q[:3, 3] = P[:3, 3] + d / np.linalg.norm(d) * (max_t if exact else rng.uniform(0, max_t))
        out[i] = Q.T.reshape(16).astype(np.float32)
    return out


def wall(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4)


def frame(name):
    if name == "Cm":
        m, s, _ = synth.workload("Cm")
        est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
        return est, s.T_gt.T.reshape(16).astype(np.float32)
    d = np.load(os.path.join(ROOT, "tests", "golden", "example_%s.npz" % name))
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
    res = est.run_trials(list(range(100, 164)))
    w = max(res, key=lambda r: r["best_lcp"])
    return est, np.asarray(w["best_pose"], np.float32)


def cost(args):
    rows = []
    for name in ("ycb_024_bowl", "linemod_obj_06", "Cm"):
        est, P0 = frame(name)
        row = dict(frame=name, nS=est.nS, nM=est.nM)
        row["one_trial_ms"] = wall(lambda: est.run_trials([1]), args.warmup, args.reps)
        row["trials64_ms"] = wall(lambda: est.run_trials(list(range(64))), 2, args.reps)
        for npri in (1, 8):
            pri = perturbed(P0, npri, seed=1, max_t=0.01, max_deg=5.0)
            for it in (0, 5):
                row["track_%dpriors_refine%d_ms" % (npri, it)] = wall(lambda: est.track_poses(pri, refine_iterations=it), args.warmup, args.reps)
        rows.append(row)
        print(json.dumps(row), flush=True)
        est.close()
    return rows


def robust_cost(args, keep, deg):
    rows = []
    for name in ("ycb_024_bowl", "Cm"):
        est, P0 = frame(name)
        row = dict(frame=name, nS=est.nS, nM=est.nM, keep_ratio=keep, max_normal_deg=deg)
        for npri in (1, 10, 64):
            pri = perturbed(P0, npri, seed=1, max_t=0.01, max_deg=5.0)
            forms = dict(search=lambda: est.track_poses(pri, refine_iterations=0), plain=lambda: est.track_poses(pri, refine_iterations=5),
                         robust=lambda: est.track_poses(pri, refine_iterations=5, keep_ratio=keep, max_normal_deg=deg))
            for f in forms.values():
                for _ in range(args.warmup):
                    f()
            ts = {k: [] for k in forms}
            for _ in range(args.reps):   # interleaved: the three forms see the same machine
                for k, f in forms.items():
                    t0 = time.perf_counter()
                    f()
                    ts[k].append((time.perf_counter() - t0) * 1e3)
            ms = {k: statistics.median(v) for k, v in ts.items()}
            row["track_%dpriors" % npri] = dict(search_ms=round(ms["search"], 4), plain_refine5_ms=round(ms["plain"], 4), robust_refine5_ms=round(ms["robust"], 4),
                                                robust_over_plain_call=round(ms["robust"] / ms["plain"], 4),
                                                robust_over_plain_refinement_part=round((ms["robust"] - ms["search"]) / max(ms["plain"] - ms["search"], 1e-9), 4))
        row["robust_workspace_bytes"] = est.refine_robust_workspace()[1]
        rows.append(row)
        print(json.dumps(row), flush=True)
        est.close()
    return rows


def sequences(n_seq, n_frames):
    m = synth.make_model_asym(2000)
    out = []
    for q in range(n_seq):
        Ts = synth.motion_sequence(synth.gt_pose(), n_frames, 0.015, 8.0, seed=synth.SEED_POSE + 303 + q)
        out.append((Ts, [synth.make_scene(m, 12000, seed=synth.SEED_SCENE + 500 + 100 * q + k, T_gt=T) for k, T in enumerate(Ts)]))
    return m, out


def run_sequence(est, Ts, scenes, kw):
    prior = Ts[0].T.reshape(1, 16).astype(np.float32)
    errs, ms, lost = [], [], 0
    for k, (T, s) in enumerate(zip(Ts, scenes)):
        est.set_scene(s.pos, s.nrm, s.prob, s.pixel)
        est.track_poses(prior, **kw)   # warm (the first call after a scene change builds nothing of its own, but the scene is new)
        t0 = time.perf_counter()
        r = est.track_poses(prior, **kw)[0]
        ms.append((time.perf_counter() - t0) * 1e3)
        lost += int(r["lcp"] < 0.02)
        errs.append(pose_err(r["pose16"], T))
        prior = np.asarray(r["pose16"], np.float32)[None]
    return errs, ms, lost


def sweep(args):
    m, seqs = sequences(args.sequences, args.frames)
    Ts0, sc0 = seqs[0]
    est = StocsEstimator(sc0[0].pos, sc0[0].nrm, sc0[0].prob, sc0[0].pixel, m.pos, m.nrm, build_index=False)
    rows = []
    # (the first run, profiles/track_time_first_run.json, swept rounds 2-8 x samples 32-512 x shrink 0.5 / 0.7: no setting kept every frame
    # within 3 degrees, the best ones were the widest and slowest-shrinking -- and a round costs the same at 32 and at 512 samples)
    for shrink in (0.5, 0.7, 0.8):
        for rounds in (4, 6, 8, 10):
            for samples in (256, 512, 1024, 2048):
                kw = dict(rounds=rounds, samples=samples, shrink=shrink, refine_iterations=0)
                E, M, L = [], [], 0
                for Ts, sc in seqs:
                    e, ms, lost = run_sequence(est, Ts, sc, kw)
                    E += e; M += ms; L += lost
                ok = sum(1 for dt, da in E if dt <= 5.0 and da <= 3.0)
                row = dict(rounds=rounds, samples=samples, shrink=shrink, frames=len(E), within_5mm_3deg=ok, lost=L,
                           max_mm=round(max(e[0] for e in E), 3), max_deg=round(max(e[1] for e in E), 3),
                           mean_mm=round(float(np.mean([e[0] for e in E])), 3), mean_deg=round(float(np.mean([e[1] for e in E])), 3),
                           median_call_ms=round(statistics.median(M), 4))
                rows.append(row)
                print(json.dumps(row), flush=True)
    best = max(r["within_5mm_3deg"] for r in rows)
    pick = min((r for r in rows if r["within_5mm_3deg"] == best), key=lambda r: r["median_call_ms"])
    # far prior: 30 cm behind the object on frame 0 of the first sequence
    est.set_scene(sc0[0].pos, sc0[0].nrm, sc0[0].prob, sc0[0].pixel)
    far = Ts0[0].copy(); far[2, 3] += 0.30
    far_lcp = float(est.track_poses(far.T.reshape(1, 16).astype(np.float32))[0]["lcp"])
    near_lcp = float(est.track_poses(Ts0[0].T.reshape(1, 16).astype(np.float32))[0]["lcp"])
    est.close()
    return rows, pick, dict(far_prior_lcp=far_lcp, gt_prior_tracked_lcp=near_lcp)


def ycb_check():
    d = np.load(os.path.join(ROOT, "tests", "golden", "example_ycb_024_bowl.npz"))
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
    res = est.run_trials(list(range(100, 164)))
    w = max(res, key=lambda r: r["best_lcp"])
    W = np.asarray(w["best_pose"], np.float32)
    out = est.track_poses(perturbed(W, 4, seed=11, max_t=0.01, max_deg=5.0, exact=True))
    rows = []
    for r in out:
        dt, da = pose_err(r["pose16"], W.reshape(4, 4).T.astype(np.float64))
        rows.append(dict(prior_lcp=float(r["prior_lcp"]), lcp=float(r["lcp"]), lcp_over_W=float(r["lcp"] / w["best_lcp"]), mm_from_W=round(dt, 3),
                         deg_from_W=round(da, 3)))
    est.close()
    return dict(W_lcp=float(w["best_lcp"]), tracked=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--robust", default=None, metavar="keep[,deg]")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sequences", type=int, default=3)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--skip-sweep", action="store_true")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "track_robust_time.json" if args.robust else "track_time.json")
    if args.robust:
        v = args.robust.split(",")
        rec = dict(reps=args.reps, warmup=args.warmup, refine_iterations=5, cost=robust_cost(args, float(v[0]), float(v[1]) if len(v) > 1 else None))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
        return
    rec = dict(defaults=TRACK_DEFAULTS, cost=cost(args), ycb_perturbed_winner=ycb_check())
    if not args.skip_sweep:
        rows, pick, far = sweep(args)
        rec.update(sweep=rows, sweep_pick=pick, **far)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("pick:", json.dumps(rec.get("sweep_pick")))


if __name__ == "__main__":
    main()
