"""What stocs_find_symmetries reports on a model: its axes, their orders, the largest and the clamped mean self-distance of each axis's
generator, the count of matched points whose normals disagree, the size of the closed set, the clustering descriptor and the flags.

  python tools/find_symmetry.py synth:Cm synth:Cm_asym example:ycb_024_bowl example:linemod_obj_06 example:packed_dove
  python tools/find_symmetry.py model.npz --tol-diameters 0.05,0.1,0.15 --json out.json

A model is synth:<workload of model_matching_amd.synth>, example:<fixture of tests/golden> or an .npz file with model_pos and model_nrm.
The tolerance is given in diameters of the model (stocs_model_diameter).  One line per model and tolerance, then one per axis.  No GPU:
the tool fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from model_matching_amd import capi, synth  # noqa: E402
from model_matching_amd.estimator import StocsEstimator  # noqa: E402


def load_model(spec):
    if spec.startswith("synth:"):
        m, _, _ = synth.workload(spec[6:])
        return np.asarray(m.pos, np.float32), np.asarray(m.nrm, np.float32)
    path = os.path.join(ROOT, "tests", "golden", "example_%s.npz" % spec[8:]) if spec.startswith("example:") else spec
    d = np.load(path)
    return d["model_pos"].astype(np.float32), d["model_nrm"].astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="+")
    ap.add_argument("--tol-diameters", default="0.05,0.1,0.15")
    ap.add_argument("--max-normal-bad", type=float, default=1.0, help="accepted share of points failing the normal gate (1: not used)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    scene = np.array([[0.0, 0.0, 1.0]], np.float32)
    rows = []
    for spec in a.models:
        pos, nrm = load_model(spec)
        est = StocsEstimator(scene, -scene, np.ones(1, np.float32), None, pos, nrm, build_index=False)
        diameter = float(est.model_diameter())
        for t in [float(x) for x in a.tol_diameters.split(",")]:
            tol = float(np.float32(t) * np.float32(diameter))
            axes, S, sym3, flags = est.find_symmetries(tol_max=tol, max_normal_bad=a.max_normal_bad)
            row = {"model": spec, "model_points": len(pos), "diameter_m": diameter, "tol_diameters": t, "tol_m": tol, "K": len(S),
                   "sym3": [float(x) for x in sym3], "descriptor_inexact": bool(flags & capi.SYMMETRY_DESCRIPTOR_INEXACT),
                   "set_truncated": bool(flags & capi.SYMMETRY_SET_TRUNCATED), "nothing_found": bool(flags & capi.SYMMETRY_NOTHING_FOUND),
                   "axes": [{"axis": [round(float(x), 5) for x in ax["axis"]], "order": int(ax["order"]), "max_m": float(ax["max"]), "mean_m": float(ax["mean"]),
                             "n_normal_bad": int(ax["n_normal_bad"])} for ax in axes]}
            rows.append(row)
            print("%s  M=%d  diameter=%.4f  tol=%.2f d (%.4f m)  axes=%d  K=%d  sym3=%s%s%s%s" % (
                spec, len(pos), diameter, t, tol, len(axes), len(S), ",".join("%g" % x for x in sym3), "  descriptor-inexact" if row["descriptor_inexact"] else "",
                "  set-truncated" if row["set_truncated"] else "", "  nothing-found" if row["nothing_found"] else ""), flush=True)
            for ax in row["axes"]:
                print("    axis=(%.4f, %.4f, %.4f)  order=%s  max=%.5f  mean=%.5f  n_normal_bad=%d" % (
                    ax["axis"][0], ax["axis"][1], ax["axis"][2], "continuous" if ax["order"] == 0 else ax["order"], ax["max_m"], ax["mean_m"], ax["n_normal_bad"]))
        est.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
