#!/usr/bin/env python3
"""What a model made from a mesh is worth, by the numpy restatement alone (tests/mesh_sample_ref.py; no GPU) -> the "models" rows of
profiles/mesh_sample_quality.json.  The solid is Cm's ellipsoid (0.08, 0.08, 0.03 m; the bump is left out so that the normal is analytic
everywhere) as icosphere(level) for level 3, 4, 5; voxel 10 mm; spacings voxel / 2, / 4, / 8.  Per row: the model's points; the share of
the leaves that a much denser sampling (voxel / 32) occupies which the model occupies too; the angle between a model normal and the
analytic normal at the model point (median, p99, the share beyond 90 degrees); and the same figures for the radius-normal path
(oracle/ingest_oracle.preprocess_model, normal radius 5 mm) on the mesh's vertices.

With --recall (needs the GPU) the closed loop of tests/test_mesh_sample_driver_gpu.py is run as well and its recalls are recorded under
"closed_loop": the share of 16 seeded trials within 0.1 diameter, for the Cm mesh beside the same frame matched with make_model's cloud.

    python tools/mesh_sample_quality.py [--recall] [--out profiles/mesh_sample_quality.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_sample_cases as mc  # noqa: E402
import mesh_sample_ref as ref  # noqa: E402
from model_matching_amd import synth  # noqa: E402
from oracle import ingest_oracle  # noqa: E402

VOXEL, RADIUS = 0.01, 0.005


def leaves(pos, voxel):
    return {tuple(r) for r in np.floor(np.asarray(pos, np.float32).astype(np.float64) * (1.0 / np.float64(np.float32(voxel)))).astype(np.int64)}


def figures(pos, nrm, dense_leaves):
    if len(pos) == 0:
        return {"model_points": 0, "coverage": 0.0}
    ang = np.degrees(np.arccos(np.clip((nrm.astype(np.float64) * mc.ellipsoid_normal(pos)).sum(axis=1), -1, 1)))
    return {"model_points": int(len(pos)), "coverage": len(leaves(pos, VOXEL) & dense_leaves) / len(dense_leaves), "angle_median_deg": float(np.median(ang)),
            "angle_p99_deg": float(np.percentile(ang, 99)), "share_beyond_90_deg": float((ang > 90).mean())}


def model_rows():
    rows = []
    for level in (3, 4, 5):
        v, t = mc.ellipsoid(level)
        dense = leaves(ref.sample(v, t, VOXEL / 32, mc.SEED + 1)[0], VOXEL)
        rpos, rnrm = ingest_oracle.preprocess_model(v, RADIUS, VOXEL, 1.0)
        row = {"level": level, "vertices": int(len(v)), "triangles": int(len(t)), "leaves_of_the_dense_sampling": len(dense),
               "radius_normals_on_the_vertices": figures(rpos, rnrm, dense), "mesh": []}
        for div in (2, 4, 8):
            pos, nrm = ref.preprocess_model_mesh(v, t, VOXEL, VOXEL / div, mc.SEED, 0, 1.0, ingest_oracle.voxel_grid)
            row["mesh"].append(dict(figures(pos, nrm, dense), spacing=VOXEL / div))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def recall_rows():
    from model_matching_amd.estimator import symmetry_set
    out = []
    v, t = synth.make_model_mesh(4)
    m = synth.make_model(5000)
    for name, kw in (("Cm level 4, model from the mesh", dict(verts=v, tris=t)), ("Cm level 4, model make_model(5000)", dict(verts=v, tris=t, model=(m.pos, m.nrm))),
                     ("box, model from the mesh, symmetric ADD", dict(verts=mc.box()[0], tris=mc.box()[1], symmetries=symmetry_set((180, 180, 180))))):
        r = mc.closed_loop(**kw)
        row = {"case": name, "trials": mc.LOOP_TRIALS, "scene_points": r["scene_points"], "model_points": r["model_points"],
               "recall_add_0.1_diameter": float((r["add_over_diameter"] < 0.1).mean()), "best_add_over_diameter": float(r["add_over_diameter"][r["best"]]),
               "best_vsd_at_tau_0.2_diameter": float(r["vsd"]["e"][3]), "highest_score_add_over_diameter": float(r["add_over_diameter"][r["winner"]]),
               "highest_score_vsd_at_tau_0.2_diameter": float(r["vsd_winner"]["e"][3])}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mesh_sample_quality.json")
    data = json.load(open(out_path)) if os.path.exists(out_path) else {}
    data["what"] = ("models from a mesh by the numpy restatement (voxel %g m, normal radius %g m for the vertex path), and, where run, the closed loop's "
                    "recalls on one MI355X" % (VOXEL, RADIUS))
    if "--recall" in sys.argv:
        data["closed_loop"] = recall_rows()
    else:
        data["models"] = model_rows()
    with open(out_path, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
