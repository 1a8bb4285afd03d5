"""Recall of StoCS trials against the synthetic ground truth -> profiles/trial_recall.json.

    python tools/trial_recall.py --example synth:Cm_asym --trials 256 [--post]

Runs --trials independent trials as one batch (run_trials, seeds --seed, --seed + 1, ...), scores every trial's winner against the scene's
T_gt with pose_errors (ADD, ADD-S on the GPU) and reports the share of trials whose error is below 0.1 of the model's diameter: of the
trials that returned a pose (pose_recall) and of all trials.  With --post the batch clusters and refines (5 iterations) inside the call and
the best refined hypothesis of every trial (first maximum of the rescored lcp) is scored too.  synth:Cm is an ellipsoid of revolution
with one bump: its ADD says little, its ADD-S is the meaningful one; synth:Cm_asym has no symmetry.  With --sym a,b,c [--sym-steps n] the
winners are also scored under the symmetries that descriptor stands for (symmetry_set, pose_errors_sym): BOP's average recalls of MSSD and
MSPD, the share with the symmetric ADD and with MSSD below 0.1 diameter, and how many records' symmetric ADD equals their plain ADD bit
for bit (all of them under --sym 0,0,0, the identity alone).  A --sym run is a row of its own in the file.  With --vsd the winners are
scored by BOP's third measure too (pose_errors_vsd, the taus 0.05 .. 0.50 diameters): the frame is the ground truth's own surfel depth
image (render_depth) in front of a wall at 1.5 m, rounded to depth units of 0.1 mm -- an ideal sensor; the average recall of VSD is taken
over ALL trials (a trial without a pose counts as wrong).  With --sym as well, `average_recall` is BOP's AR, the mean of the three average
recalls, each taken over all trials.  A --vsd run is a row of its own too.  No GPU: the tool fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from model_matching_amd import cloudio, synth  # noqa: E402
from model_matching_amd.estimator import StocsEstimator, pose_recall, pose_recall_sym, pose_recall_vsd, symmetry_set  # noqa: E402


def summary(err, diameter, n_trials):
    ra, rs, nv = pose_recall(err, diameter, 0.1)
    ok = err["valid"] != 0
    thr = np.float32(0.1) * np.float32(diameter)
    return {"trials": n_trials, "with_pose": nv, "recall_add_of_poses": ra, "recall_adds_of_poses": rs,
            "recall_add_of_trials": float((ok & (err["add"] < thr)).sum()) / n_trials,
            "recall_adds_of_trials": float((ok & (err["adds"] < thr)).sum()) / n_trials,
            "median_add_mm": float(np.median(err["add"][ok]) * 1e3) if nv else None,
            "median_adds_mm": float(np.median(err["adds"][ok]) * 1e3) if nv else None}


def summary_sym(err, plain, diameter, n_trials, image_width):
    ar3, ar2, ra, nv = pose_recall_sym(err, diameter, image_width)
    ok = err["valid"] != 0
    thr = np.float32(0.1) * np.float32(diameter)
    return {"trials": n_trials, "with_pose": nv, "average_recall_mssd_of_poses": ar3, "average_recall_mspd_of_poses": ar2, "recall_sym_add_of_poses": ra,
            "recall_mssd_of_poses": float((err["mssd"][ok] < thr).mean()) if nv else None,
            "recall_sym_add_of_trials": float((ok & (err["add"] < thr)).sum()) / n_trials,
            "recall_mssd_of_trials": float((ok & (err["mssd"] < thr)).sum()) / n_trials,
            "median_sym_add_mm": float(np.median(err["add"][ok]) * 1e3) if nv else None,
            "median_mssd_mm": float(np.median(err["mssd"][ok]) * 1e3) if nv else None,
            "sym_add_equals_add_bitwise": int((err["add_fix"][ok] == plain["add_fix"][ok]).sum())}


def summary_vsd(err, n_trials):
    ar, nv = pose_recall_vsd(err)
    ok = err["valid"] != 0
    return {"trials": n_trials, "with_pose": nv, "average_recall_vsd_of_trials": ar,
            "mean_e_at_tau_0.20_of_poses": float(err["e"][ok, 3].mean()) if nv else None,
            "median_visible_union_px": float(np.median(err["uni"][ok])) if nv else None}


def bop_ar(vsd, sym, n_trials):
    """BOP's AR: the mean of the three average recalls, each over all trials"""
    share = sym["with_pose"] / n_trials
    return float(np.mean([vsd["average_recall_vsd_of_trials"], sym["average_recall_mssd_of_poses"] * share, sym["average_recall_mspd_of_poses"] * share])) if sym["with_pose"] else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--example", default="synth:Cm_asym", choices=["synth:Cm_asym", "synth:Cm"])
    ap.add_argument("--trials", type=int, default=256)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--post", action="store_true")
    ap.add_argument("--robust", default=None, metavar="keep[,deg]", help="with --post: the refinement inside the batch is the robust one")
    ap.add_argument("--sym", default=None, help="a,b,c: the clustering's symmetry descriptor (0, 90, 180 or 360 per axis)")
    ap.add_argument("--sym-steps", type=int, default=72)
    ap.add_argument("--vsd", action="store_true", help="score by visible-surface discrepancy on the ground truth's own rendered depth image too")
    ap.add_argument("--mesh", default=None, metavar="ply|level", help="with --vsd: the model as a triangle mesh (a PLY file on the model's frame, or a level "
                    "of synth.make_model_mesh with synth:Cm), rasterised in place of the surfels")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trial_recall.json"))
    a = ap.parse_args()
    if a.mesh is not None and (not a.vsd or (a.mesh.isdigit() and a.example != "synth:Cm")):
        ap.error("--mesh needs --vsd, and a level needs --example synth:Cm (make_model_mesh is Cm's solid)")
    name = a.example.split(":", 1)[1]
    model, scene, _ = synth.workload(name)
    est = StocsEstimator(scene.pos, scene.nrm, scene.prob, scene.pixel, model.pos, model.nrm, build_index=True)
    gt16 = np.asarray(scene.T_gt, np.float64).T.reshape(16).astype(np.float32)
    seeds = list(range(a.seed, a.seed + a.trials))
    post = dict(refine_iterations=5) if a.post else None
    robust = None
    if a.robust is not None:
        if not a.post:
            ap.error("--robust needs --post")
        v = a.robust.split(",")
        robust = dict(keep_ratio=float(v[0]), max_normal_deg=float(v[1]) if len(v) > 1 else None)
    res = est.run_trials(seeds, post=post, robust=robust)
    diameter = float(est.model_diameter())
    W = np.stack([r["best_pose"] for r in res]).astype(np.float32)
    plain_w = est.pose_errors(W, gt16)
    row = {"example": a.example, "model_points": len(model.pos), "scene_points": len(scene.pos), "first_seed": a.seed, "model_diameter_m": diameter,
           "threshold_m": float(np.float32(0.1) * np.float32(diameter)), "winners": summary(plain_w, diameter, a.trials)}
    if robust is not None:
        row["robust"] = robust
    S = None
    if a.sym is not None:
        sym3 = [float(x) for x in a.sym.split(",")]
        S = symmetry_set(sym3, a.sym_steps)
        row["sym"] = {"descriptor": sym3, "steps": a.sym_steps, "symmetries": len(S)}
        row["winners_sym"] = summary_sym(est.pose_errors_sym(W, gt16, S, synth.YCB_INTRINSICS), plain_w, diameter, a.trials, 640)
    if a.vsd:
        est.set_frame(np.zeros((480, 640), np.uint16), None, synth.YCB_INTRINSICS, 1e-4)     # the camera alone: the renderer reads no depth
        if a.mesh is not None:
            mv, mt = synth.make_model_mesh(int(a.mesh)) if a.mesh.isdigit() else cloudio.read_ply_mesh(a.mesh)
            est.set_mesh(mv, mt)
        vsd_errors = est.pose_errors_vsd if a.mesh is None else est.pose_errors_vsd_mesh
        z = (est.render_depth(gt16) if a.mesh is None else est.render_depth_mesh(gt16))[0]
        est.set_frame(np.rint(np.where(z > 0, z, 1.5) / 1e-4).astype(np.uint16), None, synth.YCB_INTRINSICS, 1e-4)
        row["vsd"] = {"frame": "ground truth rendered, wall at 1.5 m", "delta_m": 0.015, "object_pixels": int((z > 0).sum())}
        row["vsd"].update({"surfel_radius_m": 0.006} if a.mesh is None else {"mesh": a.mesh, "triangles": int(len(mt))})
        row["winners_vsd"] = summary_vsd(vsd_errors(W, gt16), a.trials)
        if S is not None:
            row["winners_average_recall"] = bop_ar(row["winners_vsd"], row["winners_sym"], a.trials)
    if a.post:
        R = np.zeros((a.trials, 16), np.float32)      # all zero: "no pose"
        for t in range(a.trials):
            h = est.trials_get_hypotheses(t)
            if len(h):
                R[t] = h["refined_pose16"][int(np.argmax(h["refined_lcp"]))]
        plain_r = est.pose_errors(R, gt16)
        row["refined_winners"] = summary(plain_r, diameter, a.trials)
        if S is not None:
            row["refined_winners_sym"] = summary_sym(est.pose_errors_sym(R, gt16, S, synth.YCB_INTRINSICS), plain_r, diameter, a.trials, 640)
        if a.vsd:
            row["refined_winners_vsd"] = summary_vsd(vsd_errors(R, gt16), a.trials)
            if S is not None:
                row["refined_winners_average_recall"] = bop_ar(row["refined_winners_vsd"], row["refined_winners_sym"], a.trials)
    est.close()
    print(json.dumps(row), flush=True)
    # one file, one entry per example (and per --post): a second run adds to it
    data = {"what": "share of trials whose winner is within 0.1 diameter of T_gt (ADD, ADD-S); one visit's numbers", "rows": []}
    if os.path.exists(a.out):
        with open(a.out) as f:
            data = json.load(f)
    key = (a.example, a.post, json.dumps(row.get("sym")), json.dumps(row.get("robust")), a.trials, "vsd" in row, row.get("vsd", {}).get("mesh"))
    data["rows"] = [r for r in data["rows"] if (r["example"], "refined_winners" in r, json.dumps(r.get("sym")), json.dumps(r.get("robust")),
                                                r.get("winners", {}).get("trials", a.trials), "vsd" in r, r.get("vsd", {}).get("mesh")) != key] + [row]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
