#!/usr/bin/env python3
"""Time of StocsEstimator.refine_poses_visible (stocs_refine_poses_visible: per iteration one triangle-key render, one accumulation and one
solve; one read-back and one synchronisation per call) for 1, 10, 64 and 256 hypotheses x 5 iterations on a 640 x 480 frame: the Cm meshes
of levels 4 and 5 (synth.make_model_mesh) around synth.gt_pose() and tools/mesh_time.py's 12-triangle box that fills a third of the frame.
The frame is the mesh's own depth image at the ground truth.  Median of 20 calls after 5 warm-up calls of the host wall clock, with the
spread, and the median HIP-event time of the three kernels of the last iteration with the option device_clock on.  Beside the Cm rows, as
orientation and not as a bar (another algorithm: a voxel-sampled scene segment against the model cloud), stocs_refine_poses on the same
hypotheses in the centred frames of the Cm workload.  No time is promised.

    python tools/refine_visible_time.py [--out profiles/refine_visible_time.json]

--damped: StocsEstimator.refine_poses_visible_damped (K = 5: six evaluations) against the plain call (five iterations) on the same workloads
at 1, 64 and 256 hypotheses, in one visit and alternating call by call (plain, damped, plain): the host wall clock per evaluation against
the plain form's per iteration, with the A/A spread of the two plain series as the margin; written to
profiles/refine_visible_damped_time.json.  Measurement only, no bar.

--contour: StocsEstimator.refine_poses_visible_contour (K = 5) against the damped call on the same workloads, the frame with the mesh's
own silhouette as its class image, at 1, 64 and 256 hypotheses and pull_radius_px 16 and 64, alternating damped, contour, damped over 30
rounds: the ratio per evaluation with the A/A spread of the two damped series, and the HIP-event time of the contour kernel next to the
accumulation's; written to profiles/refine_visible_contour_time.json.  Measurement only, no bar.

Needs a GPU; no fallback."""
import time
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from depth_check_time import clock  # noqa: E402
from mesh_time import box_mesh_and_pose, frame_from  # noqa: E402
import mesh_time  # noqa: E402

SIZES = (1, 10, 64, 256)
REPS, WARM = 20, 5
ITERATIONS = 5
F = np.float32


def perturbed(P0, n, seed, max_t=0.005, max_deg=3.0):
    """n hypotheses around the 4x4 pose P0 as 4x4 matrices: <= max_deg about the object's position, <= max_t"""
    from model_matching_amd import synth
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        D = np.eye(4)
        D[:3, :3] = synth._rot_axis_angle(rng.normal(size=3), np.radians(max_deg) * rng.uniform(-1, 1))
        d = rng.normal(size=3)
        D[:3, 3] = P0[:3, 3] - D[:3, :3] @ P0[:3, 3] + d / np.linalg.norm(d) * rng.uniform(0, max_t)
        out.append(D @ P0)
    return out


def pose16(T):
    return np.ascontiguousarray(np.asarray(T, np.float64).T.reshape(16), F)


def device_medians(est, call):
    est.set_option("device_clock", 1)
    t = []
    for i in range(WARM + REPS):
        call()
        if i >= WARM:
            t.append(est.refine_visible_last_device_ms())
    est.set_option("device_clock", 0)
    return [float(x) for x in np.median(np.asarray(t), axis=0)]


DAMPED_SIZES = (1, 64, 256)
DAMPED_REPS = 30


def alternating(calls, reps=DAMPED_REPS, warm=WARM):
    """the calls in turn, `reps` rounds after `warm` warm-up rounds -> one list of ms per call"""
    t = [[] for _ in calls]
    for i in range(warm + reps):
        for k, fn in enumerate(calls):
            t0 = time.perf_counter(); fn(); dt = (time.perf_counter() - t0) * 1e3
            if i >= warm:
                t[k].append(dt)
    return t


def stats(t):
    return {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))}


def damped_rows(est, label, v, t, P0):
    """plain (A), damped, plain (A') alternating on one workload"""
    rows = []
    est.set_mesh(v, t)
    share = frame_from(est, np.asarray(P0, np.float64))
    for n in DAMPED_SIZES:
        poses = np.stack([pose16(T) for T in perturbed(np.asarray(P0, np.float64), n, 100 + n)])
        plain = lambda: est.refine_poses_visible(poses, max_iterations=ITERATIONS)
        damped = lambda: est.refine_poses_visible_damped(poses, max_iterations=ITERATIONS)
        out, rec = damped()
        a, d, a2 = alternating([plain, damped, plain])
        per_it = [np.median(a) / ITERATIONS, np.median(a2) / ITERATIONS]
        per_eval = np.median(d) / (ITERATIONS + 1)
        solve_plain = device_medians(est, plain)[2]
        solve_damped = device_medians(est, damped)[2]
        row = {"workload": label, "triangles": int(len(t)), "frame_share": round(share, 3), "hypotheses": n, "iterations": ITERATIONS, "evaluations": ITERATIONS + 1,
               "plain_a": stats(a), "damped": stats(d), "plain_a2": stats(a2), "plain_ms_per_iteration": [float(x) for x in per_it],
               "damped_ms_per_evaluation": float(per_eval), "ratio_per_evaluation_over_per_iteration": float(per_eval / np.mean(per_it)),
               "aa_spread": float(abs(per_it[0] - per_it[1]) / np.mean(per_it)), "ratio_call_over_call": float(np.median(d) / np.mean([np.median(a), np.median(a2)])),
               "expected_call_ratio": (ITERATIONS + 1) / ITERATIONS, "solve_kernel_ms_plain": solve_plain, "solve_kernel_ms_damped": solve_damped,
               "mean_accepted": float(rec["iterations"].mean()), "mean_rejected": float(rec["rejected"].mean()), "frozen": int(rec["frozen"].sum())}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main_damped(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("refine_visible_time.py needs a GPU: no time is taken without one")
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    mesh_time.K = [float(v) for v in synth.YCB_INTRINSICS]
    m, s, _ = synth.workload("Cm")
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    bv, bt, bP = box_mesh_and_pose()
    rows = []
    for label, v, t, P0 in (("Cm level 4", *synth.make_model_mesh(4), s.T_gt), ("Cm level 5", *synth.make_model_mesh(5), s.T_gt), ("box 12 triangles", bv, bt, bP)):
        rows += damped_rows(est, label, v, t, P0)
    est.close()
    out = {"what": "host wall clock of refine_poses_visible_damped (K = 5, six evaluations) per evaluation against refine_poses_visible (five iterations) per iteration, "
                   "alternating plain, damped, plain in one visit; aa_spread is the relative difference of the two plain series, the margin of the ratio; no bar",
           "device": torch.cuda.get_device_name(0), "reps": DAMPED_REPS, "warmup": WARM, "note": "one visit, one GPU; the host column shares the machine with other work",
           "kernel_resources": "profiles/refine_visible_damped.md (tools/kernel_resources.py refine_visible.hip)", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def contour_rows(est, label, v, t, P0, K):
    """damped (A), contour, damped (A') alternating on one workload, per pull radius"""
    from mesh_time import SCALE
    rows = []
    est.set_mesh(v, t)
    est.set_frame(np.zeros((480, 640), np.uint16), None, K, SCALE)
    z = est.render_depth_mesh(pose16(P0))[0]
    est.set_frame(np.rint(np.where(z > 0, z, 1.5) / SCALE).astype(np.uint16), np.where(z > 0, 10000, 0).astype(np.uint16), K, SCALE)
    for n in DAMPED_SIZES:
        poses = np.stack([pose16(T) for T in perturbed(np.asarray(P0, np.float64), n, 100 + n)])
        damped = lambda: est.refine_poses_visible_damped(poses, max_iterations=ITERATIONS)
        for R in (16, 64):
            contour = lambda: est.refine_poses_visible_contour(poses, max_iterations=ITERATIONS, pull_radius_px=R)
            out, rec = contour()
            a, c, a2 = alternating([damped, contour, damped])
            per_a = [np.median(a) / (ITERATIONS + 1), np.median(a2) / (ITERATIONS + 1)]
            per_c = np.median(c) / (ITERATIONS + 1)
            est.set_option("device_clock", 1)
            dev = []
            for i in range(WARM + REPS):
                contour()
                if i >= WARM:
                    dev.append(est.refine_visible_last_device_ms() + (est.refine_visible_contour_last_device_ms(),))
            est.set_option("device_clock", 0)
            render_ms, acc_ms, solve_ms, contour_ms = [float(x) for x in np.median(np.asarray(dev), axis=0)]
            row = {"workload": label, "triangles": int(len(t)), "frame_share": round(float((z > 0).mean()), 3), "hypotheses": n, "evaluations": ITERATIONS + 1,
                   "pull_radius_px": R, "damped_a": stats(a), "contour": stats(c), "damped_a2": stats(a2), "damped_ms_per_evaluation": [float(x) for x in per_a],
                   "contour_ms_per_evaluation": float(per_c), "ratio_contour_over_damped": float(per_c / np.mean(per_a)),
                   "aa_spread": float(abs(per_a[0] - per_a[1]) / np.mean(per_a)), "render_kernel_ms": render_ms, "contour_kernel_ms": contour_ms,
                   "accumulate_kernel_ms": acc_ms, "solve_kernel_ms": solve_ms, "mean_uncovered": float(rec["uncovered"].mean()), "mean_pulled": float(rec["pulled"].mean()),
                   "mean_accepted": float(rec["iterations"].mean()), "mean_rejected": float(rec["rejected"].mean())}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main_contour(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("refine_visible_time.py needs a GPU: no time is taken without one")
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    K = [float(v) for v in synth.YCB_INTRINSICS]
    m, s, _ = synth.workload("Cm")
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    bv, bt, bP = box_mesh_and_pose()
    rows = []
    for label, v, t, P0 in (("Cm level 4", *synth.make_model_mesh(4), s.T_gt), ("Cm level 5", *synth.make_model_mesh(5), s.T_gt), ("box 12 triangles", bv, bt, bP)):
        rows += contour_rows(est, label, v, t, P0, K)
    est.close()
    out = {"what": "host wall clock of refine_poses_visible_contour (K = 5, six evaluations, the library's defaults but the radius) per evaluation against "
                   "refine_poses_visible_damped, alternating damped, contour, damped in one visit; aa_spread is the relative difference of the two damped series, the "
                   "margin of the ratio; kernel columns: median HIP-event time of the last evaluation of a contour call; no bar",
           "device": torch.cuda.get_device_name(0), "reps": DAMPED_REPS, "warmup": WARM, "note": "one visit, one GPU; the host column shares the machine with other work",
           "kernel_resources": "profiles/refine_visible_contour.md (tools/kernel_resources.py refine_visible.hip)", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--damped", action="store_true")
    ap.add_argument("--contour", action="store_true")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "refine_visible_contour_time.json" if args.contour else "refine_visible_damped_time.json" if args.damped
                                else "refine_visible_time.json")
    if args.contour:
        return main_contour(args)
    if args.damped:
        return main_damped(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("refine_visible_time.py needs a GPU: no time is taken without one")
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    mesh_time.K = [float(v) for v in synth.YCB_INTRINSICS]
    m, s, _ = synth.workload("Cm")
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    cs, cm = est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64)
    bv, bt, bP = box_mesh_and_pose()
    rows = []
    for label, v, t, P0, with_points in (("Cm level 4", *synth.make_model_mesh(4), s.T_gt, True), ("Cm level 5", *synth.make_model_mesh(5), s.T_gt, True),
                                          ("box 12 triangles", bv, bt, bP, False)):
        est.set_mesh(v, t)
        share = frame_from(est, np.asarray(P0, np.float64))
        for n in SIZES:
            hyp = perturbed(np.asarray(P0, np.float64), n, 100 + n)
            poses = np.stack([pose16(T) for T in hyp])
            call = lambda: est.refine_poses_visible(poses, max_iterations=ITERATIONS)
            out, rec = call()
            render_ms, acc_ms, solve_ms = device_medians(est, call)
            row = {"workload": label, "triangles": int(len(t)), "frame_share": round(share, 3), "hypotheses": n, "iterations": ITERATIONS,
                   "refine_poses_visible": clock(call), "render_kernel_ms": render_ms, "accumulate_kernel_ms": acc_ms, "solve_kernel_ms": solve_ms,
                   "mean_counted": float(rec["counted"].mean()), "mean_iterations": float(rec["iterations"].mean()), "frozen": int(rec["frozen"].sum())}
            if with_points:
                T16 = np.stack([pose16(synth.centred_gt(T, cs, cm)) for T in hyp])
                row["stocs_refine_poses_same_hypotheses"] = clock(lambda: est.refine_poses(T16, ITERATIONS, 0.035))
            rows.append(row)
            print(json.dumps(row), flush=True)
    est.close()
    out = {"what": "host wall clock of refine_poses_visible and HIP-event time of the three kernels of its last iteration; beside the Cm rows stocs_refine_poses on "
                   "the same hypotheses (orientation: another algorithm, no bar)",
           "device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM, "note": "one visit, one GPU; the host column shares the machine with other work",
           "kernel_resources": "profiles/refine_visible.md (tools/kernel_resources.py refine_visible.hip mesh.hip)", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
