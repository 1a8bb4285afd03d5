#!/usr/bin/env python3
"""What stocs_refine_poses_visible does to poses that are off by a known amount: ground-truth poses of the Cm solid perturbed over a range of
millimetres and degrees, refined against frames that are ray-cast ANALYTICALLY from the solid (tests/vsd_cases.py::cm_analytic_depth, as
tools/mesh_quality.py does it; the level-5 mesh is the model, so the frame is not the mesh's own image), ADD before and after.  Three
frames: clean, with Gaussian depth noise, and with an occluder in front of a part of the object.  Next to it, on the same hypotheses,
stocs_refine_poses and stocs_refine_poses_robust on the scene ingested from the same frame (stocs_ingest_scene; the class image is the
analytic silhouette): another algorithm, shown for orientation.  The Cm solid is an ellipsoid of revolution but for its bump, so one
rotation is weakly constrained by depth; the last rows therefore repeat the visible refinement on a solid without a near-symmetry,
tools/mesh_time.py's box on its own mesh image (largest corner distance in place of ADD: no model cloud goes with it).  Measurement
only; nothing is promised.

    python tools/refine_visible_quality.py [--out profiles/refine_visible_quality.json] [--samples 16]

--damped: every row also gets stocs_refine_poses_visible_damped on the same hypotheses (the library's defaults about the mean of the mesh's
vertices, K = 5 and K = 10; add_damped_5/10 or corner_error_damped_5/10, accepted and rejected steps), whether the damped median is at or
below the row's error before, and for a row where it is not the trace of its worst hypothesis; written to
profiles/refine_visible_damped_quality.json.

--contour: the 18 Cm rows and the box rows with the analytic (Cm) or the mesh's own (box) silhouette as the class image, plus lateral-offset
rows (the start displaced across the rays by 0.5, 1 and 1.5 object widths, in evenly spaced image directions): the error before, after
stocs_refine_poses_visible_damped and after stocs_refine_poses_visible_contour at contour_weight 0.25, 1 and 4 from the same starts (K = 10,
max_distance 0.02, otherwise the library's defaults), and for the lateral rows also a wide form (pull_radius_px 64, pull_distance two
widths); written to profiles/refine_visible_contour_quality.json.

Needs a GPU; no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_visible_ref as rvref  # noqa: E402
import vsd_cases as vc  # noqa: E402
from mesh_time import box_mesh_and_pose  # noqa: E402
from refine_visible_time import perturbed, pose16  # noqa: E402

F = np.float32
W, H, SCALE = 640, 480, 1.0e-4
LEVELS = [(0.002, 1.0), (0.005, 2.0), (0.010, 4.0), (0.015, 6.0), (0.020, 8.0), (0.030, 12.0)]   # (metres, degrees): the largest perturbation of a level
WALL = 1.2                                                                                   # metres: the background behind the object


def frames(za, rng):
    """clean, noisy (sigma 1 mm on every measured pixel) and occluded (a slab 10 cm in front of the object's left third) raw images"""
    sil = za > 0
    z = np.where(sil, za, WALL)
    out = {"clean": vc.raw_from_depth(z, SCALE)}
    out["noise_1mm"] = vc.raw_from_depth(z + rng.normal(0, 0.001, z.shape), SCALE)
    cols = np.flatnonzero(sil.any(axis=0))
    occ = z.copy()
    c_end = cols[0] + (cols[-1] - cols[0]) // 3
    occ[:, cols[0] - 5: c_end] = np.minimum(occ[:, cols[0] - 5: c_end], za[sil].min() - 0.10)
    out["occluder_third"] = vc.raw_from_depth(occ, SCALE)
    return out, sil


def summary(x):
    x = np.asarray(x, np.float64)
    return {"median_mm": float(np.median(x) * 1e3), "p90_mm": float(np.percentile(x, 90) * 1e3), "max_mm": float(x.max() * 1e3)}


def damped_columns(est, poses, error, key, before):
    """the damped form on the row's hypotheses -> the row's extra columns; error(P) gives one error per pose"""
    cols = {}
    for K in (5, 10):
        P, rec, tr = est.refine_poses_visible_damped(poses, trace=True, max_iterations=K, max_distance=0.02)
        err = np.asarray(error(P), np.float64)
        cols["%s_damped_%d" % (key, K)] = summary(err)
        cols["damped_%d_mean_accepted" % K] = float(rec["iterations"].mean())
        cols["damped_%d_mean_rejected" % K] = float(rec["rejected"].mean())
        cols["damped_%d_frozen" % K] = int(rec["frozen"].sum())
        cols["damped_%d_worse_than_before" % K] = int((err > np.asarray(before, np.float64)).sum())
        ok = bool(np.median(err) <= np.median(before))
        cols["damped_%d_median_at_or_below_before" % K] = ok
        if not ok:
            w = int(np.argmax(err - np.asarray(before, np.float64)))
            cols["damped_%d_worst_trace" % K] = {"hypothesis": w, "error_before_mm": float(before[w]) * 1e3, "error_after_mm": float(err[w]) * 1e3,
                                                "cost": [float(x) for x in tr[w]["cost"]], "lambda": [float(x) for x in tr[w]["lambda"]],
                                                "accepted": [int(x) for x in tr[w]["accepted"]], "state": [int(x) for x in tr[w]["state"]]}
    return cols


CONTOUR_WEIGHTS = (0.25, 1.0, 4.0)
LATERAL = (0.5, 1.0, 1.5)       # object widths across the rays


def contour_columns(est, poses, error, key, wide=None):
    """damped and contour (w = 0.25, 1, 4; with `wide` also pull_radius_px 64 and that pull_distance) from the same starts -> the row's columns"""
    cols = {key + "_before": summary(error(poses))}
    P, rec = est.refine_poses_visible_damped(poses, max_iterations=10, max_distance=0.02)
    cols[key + "_damped"] = summary(error(P))
    cols["damped_frozen"] = int(rec["frozen"].sum())
    forms = [("contour_w%g" % w, dict(contour_weight=w)) for w in CONTOUR_WEIGHTS]
    if wide is not None:
        forms += [("contour_w%g_R64_wide" % w, dict(contour_weight=w, pull_radius_px=64, pull_distance=wide)) for w in CONTOUR_WEIGHTS]
    for name, prm in forms:
        P, rec = est.refine_poses_visible_contour(poses, max_iterations=10, max_distance=0.02, **prm)
        cols["%s_%s" % (key, name)] = summary(error(P))
        cols[name + "_frozen"] = int(rec["frozen"].sum())
        cols[name + "_mean_accepted"] = float(rec["iterations"].mean())
        cols[name + "_mean_pulled"] = float(rec["pulled"].mean())
        cols[name + "_mean_uncovered"] = float(rec["uncovered"].mean())
    return cols


def lateral_starts(T, width_m, factor, n):
    """n starts: T displaced by factor * width_m in the camera's x-y plane, in evenly spaced directions"""
    out = []
    for i in range(n):
        a = 2 * np.pi * (i + 0.5) / n
        S = np.asarray(T, np.float64).copy()
        S[:3, 3] += factor * width_m * np.array([np.cos(a), np.sin(a), 0.0])
        out.append(pose16(S))
    return np.stack(out)


def main_contour(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("refine_visible_quality.py needs a GPU: nothing is measured without one")
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator, ingest_scene
    K = [float(v) for v in synth.YCB_INTRINSICS]
    m = synth.make_model(5000)
    T = synth.gt_pose()
    gt16 = pose16(T)
    za = vc.cm_analytic_depth(T, vc.cm_ellipsoid_centre(m.pos), K, W, H)
    rng = np.random.default_rng(17)
    raws, sil = frames(za, rng)
    prob = np.where(sil, 10000, 0).astype(np.uint16)
    v, t = synth.make_model_mesh(5)
    sp, sn, spr, spx = ingest_scene(raws["clean"], prob, K, SCALE)
    est = StocsEstimator(sp, sn, spr, spx, m.pos, m.nrm, build_index=False)
    est.set_mesh(v, t)
    add = lambda P: est.pose_errors(P, gt16)["add"]
    cols_of = np.flatnonzero(sil.any(axis=0))
    width = float((cols_of[-1] - cols_of[0] + 1) * T[2, 3] / K[0])
    rows = []
    for name, raw in raws.items():
        est.set_frame(raw, prob, K, SCALE)
        for li, (max_t, max_deg) in enumerate(LEVELS):
            poses = np.stack([pose16(x) for x in perturbed(T, args.samples, 1000 + li, max_t=max_t, max_deg=max_deg)])
            row = {"frame": name, "max_translation_mm": max_t * 1e3, "max_rotation_deg": max_deg, "samples": args.samples}
            row.update(contour_columns(est, poses, add, "add"))
            rows.append(row)
            print(json.dumps(row), flush=True)
    est.set_frame(raws["clean"], prob, K, SCALE)
    for f in LATERAL:
        row = {"frame": "clean", "lateral_offset_widths": f, "object_width_mm": width * 1e3, "samples": args.samples}
        row.update(contour_columns(est, lateral_starts(T, width, f, args.samples), add, "add", wide=2 * width))
        rows.append(row)
        print(json.dumps(row), flush=True)
    bv, bt, bP = box_mesh_and_pose()
    est.set_mesh(bv, bt)
    est.set_frame(np.zeros((H, W), np.uint16), None, K, SCALE)
    zb = est.render_depth_mesh(pose16(bP))[0].astype(np.float64)
    bprob = np.where(zb > 0, 10000, 0).astype(np.uint16)
    corner = lambda P: [rvref.vertex_error(p, pose16(bP), bv) for p in P]
    bcols = np.flatnonzero((zb > 0).any(axis=0))
    bwidth = float((bcols[-1] - bcols[0] + 1) * bP[2, 3] / K[0])
    for name, zimg in (("box clean", np.where(zb > 0, zb, WALL)), ("box noise_1mm", np.where(zb > 0, zb, WALL) + rng.normal(0, 0.001, zb.shape))):
        est.set_frame(vc.raw_from_depth(zimg, SCALE), bprob, K, SCALE)
        for li, (max_t, max_deg) in enumerate(LEVELS):
            poses = np.stack([pose16(x) for x in perturbed(bP, args.samples, 2000 + li, max_t=max_t, max_deg=max_deg)])
            row = {"frame": name, "max_translation_mm": max_t * 1e3, "max_rotation_deg": max_deg, "samples": args.samples}
            row.update(contour_columns(est, poses, corner, "corner_error"))
            rows.append(row)
            print(json.dumps(row), flush=True)
        if name == "box clean":
            for f in LATERAL:
                row = {"frame": name, "lateral_offset_widths": f, "object_width_mm": bwidth * 1e3, "samples": args.samples}
                row.update(contour_columns(est, lateral_starts(bP, bwidth, f, args.samples), corner, "corner_error", wide=2 * bwidth))
                rows.append(row)
                print(json.dumps(row), flush=True)
    est.close()
    out = {"what": "ADD (Cm rows) or largest corner distance (box rows) of perturbed and of laterally displaced ground-truth poses before, after "
                   "stocs_refine_poses_visible_damped and after stocs_refine_poses_visible_contour at three weights from the same starts; K = 10, max_distance 0.02, "
                   "the class image is the object's true silhouette; synthetic frames only",
           "device": torch.cuda.get_device_name(0), "frame": [W, H], "depth_unit_mm": SCALE * 1e3, "triangles": int(len(t)), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_visible_quality.json"))
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--damped", action="store_true")
    ap.add_argument("--contour", action="store_true")
    args = ap.parse_args()
    if args.contour:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(ROOT, "profiles", "refine_visible_contour_quality.json")
        return main_contour(args)
    if args.damped and args.out == ap.get_default("out"):
        args.out = os.path.join(ROOT, "profiles", "refine_visible_damped_quality.json")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("refine_visible_quality.py needs a GPU: nothing is measured without one")
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator, ingest_scene
    K = [float(v) for v in synth.YCB_INTRINSICS]
    m = synth.make_model(5000)
    T = synth.gt_pose()
    gt16 = pose16(T)
    za = vc.cm_analytic_depth(T, vc.cm_ellipsoid_centre(m.pos), K, W, H)
    rng = np.random.default_rng(17)
    raws, sil = frames(za, rng)
    prob = np.where(sil, 10000, 0).astype(np.uint16)
    v, t = synth.make_model_mesh(5)
    est = None
    rows = []
    for name, raw in raws.items():
        sp, sn, spr, spx = ingest_scene(raw, prob, K, SCALE)
        if est is None:
            est = StocsEstimator(sp, sn, spr, spx, m.pos, m.nrm, build_index=False)
            est.set_mesh(v, t)
        else:
            est.set_scene(sp, sn, spr, spx)
        est.set_frame(raw, prob, K, SCALE)
        cs, cm = est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64)
        for li, (max_t, max_deg) in enumerate(LEVELS):
            hyp = perturbed(T, args.samples, 1000 + li, max_t=max_t, max_deg=max_deg)
            poses = np.stack([pose16(x) for x in hyp])
            T16 = np.stack([pose16(synth.centred_gt(x, cs, cm)) for x in hyp])
            before = est.pose_errors(poses, gt16)["add"]
            out, rec = est.refine_poses_visible(poses, max_iterations=5, max_distance=0.02)
            out10, rec10 = est.refine_poses_visible(poses, max_iterations=10, max_distance=0.02)
            plain = est.refine_poses(T16, 5, 0.035)[1]
            robust = est.refine_poses_robust(T16, 5, 0.035, 0.7, 30.0)[1]
            row = {"frame": name, "scene_points": int(len(sp)), "max_translation_mm": max_t * 1e3, "max_rotation_deg": max_deg, "samples": args.samples,
                   "add_before": summary(before), "add_visible_5": summary(est.pose_errors(out, gt16)["add"]),
                   "add_visible_10": summary(est.pose_errors(out10, gt16)["add"]), "add_refine_poses_5": summary(est.pose_errors(plain, gt16)["add"]),
                   "add_refine_poses_robust_5": summary(est.pose_errors(robust, gt16)["add"]), "visible_mean_counted": float(rec["counted"].mean()),
                   "visible_frozen": int(rec["frozen"].sum()), "visible_median_rms_mm": float(np.median(rec["rms"]) * 1e3)}
            if args.damped:
                row.update(damped_columns(est, poses, lambda P: est.pose_errors(P, gt16)["add"], "add", before))
            rows.append(row)
            print(json.dumps(row), flush=True)
    # a solid without a near-symmetry: tools/mesh_time.py's box at its pose, the frame its own mesh image in front of the wall; no model
    # cloud goes with it, so the error is the largest distance between the box's corners under the two poses
    bv, bt, bP = box_mesh_and_pose()
    est.set_mesh(bv, bt)
    est.set_frame(np.zeros((H, W), np.uint16), None, K, SCALE)
    zb = est.render_depth_mesh(pose16(bP))[0].astype(np.float64)
    for name, zimg in (("box clean", np.where(zb > 0, zb, WALL)), ("box noise_1mm", np.where(zb > 0, zb, WALL) + rng.normal(0, 0.001, zb.shape))):
        est.set_frame(vc.raw_from_depth(zimg, SCALE), None, K, SCALE)
        for li, (max_t, max_deg) in enumerate(LEVELS):
            poses = np.stack([pose16(x) for x in perturbed(bP, args.samples, 2000 + li, max_t=max_t, max_deg=max_deg)])
            corner = lambda P: [rvref.vertex_error(p, pose16(bP), bv) for p in P]
            out5, rec = est.refine_poses_visible(poses, max_iterations=5, max_distance=0.02)
            out10, _ = est.refine_poses_visible(poses, max_iterations=10, max_distance=0.02)
            row = {"frame": name, "max_translation_mm": max_t * 1e3, "max_rotation_deg": max_deg, "samples": args.samples, "corner_error_before": summary(corner(poses)),
                   "corner_error_visible_5": summary(corner(out5)), "corner_error_visible_10": summary(corner(out10)), "visible_mean_counted": float(rec["counted"].mean()),
                   "visible_frozen": int(rec["frozen"].sum()), "visible_median_rms_mm": float(np.median(rec["rms"]) * 1e3)}
            if args.damped:
                row.update(damped_columns(est, poses, corner, "corner_error", corner(poses)))
            rows.append(row)
            print(json.dumps(row), flush=True)
    est.close()
    out = {"what": "ADD (mean vertex distance of the 5 000-point Cm cloud, stocs_pose_errors) of perturbed ground-truth poses before and after refinement, per frame and "
                   "perturbation level; visible: stocs_refine_poses_visible on the level-5 mesh, max_distance 0.02; refine_poses[_robust]: the scene ingested from "
                   "the same frame, 3.5 cm, keep 0.7, 30 degrees; box rows: the 12-triangle box on its own mesh image, largest corner distance"
                   + ("; damped: stocs_refine_poses_visible_damped with the library's defaults about the mean of the mesh's vertices" if args.damped else ""),
           "device": torch.cuda.get_device_name(0), "frame": [W, H], "depth_unit_mm": SCALE * 1e3, "triangles": int(len(t)), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
