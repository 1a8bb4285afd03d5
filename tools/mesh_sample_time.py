#!/usr/bin/env python3
"""Times of mesh sampling on the GPU -> profiles/mesh_sample_time.json (run on the GPU box from the repo root).

  calls    mesh_sample and preprocess_model_mesh (the whole call: upload, count, scan, sample, download / voxel grid; a host clock around
           a call that ends in a synchronise; 3 warm-up calls, then the median and the minimum of REPS) on the box and on the Cm meshes of
           level 3, 5 and 7 at spacings of voxel / 2, voxel / 4 and voxel / 8 (voxel 5 mm), beside stocs_preprocess_model on the same
           mesh's vertices: the parent path, with its O(n^2) normals
  forms    the sample kernel alone under each forced form (STOCS_MESH_SAMPLE_FORM), from rocprofv3 --kernel-trace --stats, one child
           process per (case, form): the two regimes the search must serve and two between them
  kernels  tools/kernel_resources.py mesh_sample.hip

    python tools/mesh_sample_time.py [--out profiles/mesh_sample_time.json] [--no-forms]"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from model_matching_amd import synth  # noqa: E402

VOXEL = 0.005
BOX_SIZE = (0.10, 0.06, 0.04)
REPS = 15
# (name, mesh, spacing): what each stands for is in the `forms` rows
FORM_CASES = (("box, spacing 0.1 mm", "box", 0.0001), ("Cm level 5, voxel / 8", "cm5", VOXEL / 8), ("Cm level 7, voxel / 8", "cm7", VOXEL / 8),
              ("Cm level 7, voxel / 2", "cm7", VOXEL / 2))
FORM_NAMES = {"1": "global", "2": "window"}


def mesh_of(key):
    return synth.box_mesh(BOX_SIZE) if key == "box" else synth.make_model_mesh(int(key[2:]))


def timed(fn, reps=REPS, warm=3):
    for _ in range(warm):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "reps": reps}, out


def child(key, spacing):
    """the work of one forms pass: 30 calls of mesh_sample"""
    from model_matching_amd.estimator import mesh_sample
    v, t = mesh_of(key)
    for _ in range(30):
        pos = mesh_sample(v, t, spacing, 1)[0]
    print(len(pos))


def forms_rows(outdir):
    import pmc_all
    rows = []
    for name, key, spacing in FORM_CASES:
        row = {"case": name, "triangles": int(len(mesh_of(key)[1]))}
        for form, label in FORM_NAMES.items():
            os.environ["STOCS_MESH_SAMPLE_FORM"] = form
            st = pmc_all.stats_pass([sys.executable, os.path.abspath(__file__), "--child", key, repr(spacing)], os.path.join(outdir, "%s_%s" % (key, form) + repr(spacing)), 200)
            del os.environ["STOCS_MESH_SAMPLE_FORM"]
            for k, rec in st.items():
                if "mesh_sample_kernel" in k:
                    row[label] = {"avg_us": rec["avg_us"], "calls": rec["calls"]}
                if "mesh_sample_count_kernel" in k:
                    row["count_kernel_avg_us"] = rec["avg_us"]
            digits = [l for l in open(os.path.join(outdir, "%s_%s" % (key, form) + repr(spacing), "log")).read().split("\n") if l.strip().isdigit()]
            if digits:
                row["samples"] = int(digits[-1])
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], float(sys.argv[3]))
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mesh_sample_time.json")
    from model_matching_amd.estimator import mesh_sample, preprocess_model, preprocess_model_mesh
    import kernel_resources
    data = {"what": "mesh sampling on one MI355X: whole calls by a host clock (median and minimum of %d after 3 warm-up calls), the sample kernel per "
                    "forced form by rocprofv3 --kernel-trace --stats (average over 30 calls, one process per row and form); one visit's numbers" % REPS,
            "voxel": VOXEL, "calls": [], "forms": [], "kernels": kernel_resources.kernels_of("mesh_sample.hip")}
    for key in ("box", "cm3", "cm5", "cm7"):
        v, t = mesh_of(key)
        reps = 3 if key == "cm7" else REPS
        old, (opos, _) = timed(lambda: preprocess_model(v, VOXEL, VOXEL, 1.0), reps=reps, warm=1)       # the parent path: normal radius = one voxel
        row = {"mesh": key, "vertices": int(len(v)), "triangles": int(len(t)), "preprocess_model_on_the_vertices": dict(old, model_points=int(len(opos)), normal_radius=VOXEL), "spacings": []}
        for div in (2, 4, 8):
            h = VOXEL / div
            a, (pos, _, _) = timed(lambda: mesh_sample(v, t, h, 1))
            b, (mpos, _) = timed(lambda: preprocess_model_mesh(v, t, VOXEL, spacing=h, seed=1))
            row["spacings"].append({"spacing": h, "samples": int(len(pos)), "mesh_sample": a, "preprocess_model_mesh": dict(b, model_points=int(len(mpos)))})
        data["calls"].append(row)
        print(json.dumps(row), flush=True)
    if "--no-forms" not in sys.argv:
        with tempfile.TemporaryDirectory() as tmp:
            data["forms"] = forms_rows(tmp)
    with open(out_path, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
