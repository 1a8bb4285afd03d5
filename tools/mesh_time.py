#!/usr/bin/env python3
"""Time of StocsEstimator.pose_errors_vsd_mesh (stocs_pose_errors_vsd_mesh: triangle renders, one compare pass per pair, one read-back, one
synchronisation per call) for 1, 16, 64 and 256 pairs, with one ground truth for all (n_gt = 1) and one each (n_gt = n), on the level-3,
level-5 and level-7 Cm meshes (synth.make_model_mesh: 1 600, 25 600 and 409 600 triangles) at synth.gt_pose() and on a 12-triangle box
that fills a third of the frame, all on a 640 x 480 frame rendered from the ground truth, wall at 1.5 m.  Beside the Cm rows the same
poses through stocs_pose_errors_vsd on the 5 000-point Cm cloud (6 mm surfels).  Median of 20 calls after 5 warm-up calls of the host
wall clock, with the spread, and the median HIP-event time of the launches ("device: kernel") of as many calls.  No time is promised.

    python tools/mesh_time.py [--out profiles/mesh_time.json]
    python tools/mesh_time.py --forms [--out profiles/mesh_forms.json]

--forms is the A/B visit that sets STOCS_MESH_SMALL_PX and the read-first rule: the HIP-event time of the launches (median of 7 after 2)
for every mesh at 1 and 64 pairs under each small-box limit (STOCS_MESH_SMALL_PX in the environment; 0: no lane walks its own box) with
the atomics blind and behind a read, and with the largest boxes on the workgroup or on one wavefront.  Every form gives the same bits;
the tool checks that the records of every form are the first form's.  Needs a GPU; no fallback."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from depth_check_time import clock, perturbed  # noqa: E402

SIZES = (1, 16, 64, 256)
REPS, WARM = 20, 5
F = np.float32
K = None
SCALE = 1e-4


def device_median(est, call, reps, warm):
    """the median "device: kernel" entry of `reps` calls after `warm`"""
    est.set_option("device_clock", 1)
    t = []
    for i in range(warm + reps):
        call()
        if i >= warm:
            t.append(dict(est.last_mesh_call_timing() if call.mesh else est.last_call_timing(7))["device: kernel"])
    est.set_option("device_clock", 0)
    return float(np.median(t))


def box_mesh_and_pose():
    """a 0.20 x 0.15 x 0.10 m box at 0.7 m, turned so that three faces show: about a third of 640 x 480"""
    sx, sy, sz = 0.20, 0.15, 0.10
    v = np.array([(x, y, z) for z in (-sz, sz) for y in (-sy, sy) for x in (-sx, sx)], F) * F(0.5)
    q = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = np.array([f for a, b, c, d in q for f in ((a, b, c), (a, c, d))], np.int32)
    a, b = np.deg2rad(25.0), np.deg2rad(-30.0)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    P = np.eye(4); P[:3, :3] = Rx @ Ry; P[:3, 3] = (0.0, 0.0, 0.7)
    return v, t, P


def workloads():
    from model_matching_amd import synth
    P0 = synth.gt_pose()
    out = [("Cm level %d" % lv, *synth.make_model_mesh(lv), P0, True) for lv in (3, 5, 7)]
    v, t, P = box_mesh_and_pose()
    out.append(("box 12 triangles", v, t, P, False))
    return out


def frame_from(est, P0):
    est.set_frame(np.zeros((480, 640), np.uint16), None, K, SCALE)     # the camera alone: the renderer reads no depth
    z = est.render_depth_mesh(P0.T.reshape(16).astype(F))[0]
    est.set_frame(np.rint(np.where(z > 0, z, 1.5) / SCALE).astype(np.uint16), None, K, SCALE)
    return float((z > 0).mean())


def time_table(est, taus):
    rows = []
    for label, v, t, P0, with_surfels in workloads():
        est.set_mesh(v, t)
        share = frame_from(est, P0)
        gt = np.asarray(P0, np.float64).T.reshape(16).astype(F)
        for n in SIZES:
            poses = perturbed(P0, n, 100 + n)
            for n_gt in (1, n):
                G = gt if n_gt == 1 else np.tile(gt, (n, 1))
                mesh = lambda: est.pose_errors_vsd_mesh(poses, G, taus)
                mesh.mesh = True
                row = {"workload": label, "triangles": int(len(t)), "frame_share": round(share, 3), "pairs": n, "n_gt": n_gt, "mesh": clock(mesh),
                       "mesh_device_kernels_ms": device_median(est, mesh, REPS, WARM)}
                if with_surfels:
                    surf = lambda: est.pose_errors_vsd(poses, G, taus)
                    surf.mesh = False
                    row.update({"surfels_5000_points": clock(surf), "surfels_device_kernels_ms": device_median(est, surf, REPS, WARM)})
                rows.append(row)
                print(json.dumps(row), flush=True)
                if n == 1:
                    break                                      # n_gt = n is the same call
    return rows


def forms_table(est, taus):
    rows = []
    for label, v, t, P0, _ in workloads():
        est.set_mesh(v, t)
        frame_from(est, P0)
        gt = np.asarray(P0, np.float64).T.reshape(16).astype(F)
        for n in (1, 64):
            poses = perturbed(P0, n, 100 + n)
            first = None
            for small in (0, 36, 64, 100, 144, 256, 1024):
                for form, name in ((8, "blind"), (4, "read first"), (8 | 16, "blind, no workgroup boxes")):
                    if form & 16 and (small != 64 or len(t) > 100):
                        continue                               # the workgroup's boxes matter on the box alone
                    os.environ["STOCS_MESH_SMALL_PX"] = str(small)
                    os.environ["STOCS_MESH_FORM"] = str(form)
                    call = lambda: est.pose_errors_vsd_mesh(poses, gt, taus)
                    call.mesh = True
                    rec = call()
                    first = rec if first is None else first
                    if rec.tobytes() != first.tobytes():
                        raise SystemExit("form %d, small %d on %s: the records differ from the first form's" % (form, small, label))
                    rows.append({"workload": label, "triangles": int(len(t)), "pairs": n, "n_gt": 1, "small_px": small, "atomics": name,
                                 "device_kernels_ms": device_median(est, call, 7, 2)})
                    print(json.dumps(rows[-1]), flush=True)
    os.environ.pop("STOCS_MESH_SMALL_PX", None); os.environ.pop("STOCS_MESH_FORM", None)
    return rows


def main():
    global K
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", action="store_true", help="the A/B of the kernel's forms, not the time table")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", "mesh_forms.json" if args.forms else "mesh_time.json")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_time.py needs a GPU: no time is taken without one")
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    K = [float(v) for v in synth.YCB_INTRINSICS]
    m = synth.make_model(5000)
    rng = np.random.default_rng(3); sp = rng.normal(0, 0.05, (64, 3)).astype(F)
    est = StocsEstimator(sp, sp / np.linalg.norm(sp, axis=1, keepdims=True), np.ones(64, F), None, m.pos, m.nrm, build_index=False)
    dia = F(est.model_diameter())
    taus = [F(0.05 * i) * dia for i in range(1, 11)]
    rows = forms_table(est, taus) if args.forms else time_table(est, taus)
    est.close()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "mesh.hip"], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    what = ("HIP-event time of the launches of pose_errors_vsd_mesh under each forced form (STOCS_MESH_SMALL_PX, STOCS_MESH_FORM)" if args.forms else
            "host wall clock and HIP-event time of pose_errors_vsd_mesh next to pose_errors_vsd on the 5 000-point cloud, same poses")
    out = {"what": what, "device": torch.cuda.get_device_name(0), "reps": 7 if args.forms else REPS, "warmup": 2 if args.forms else WARM,
           "note": "one visit, one GPU; the host column shares the machine with other work", "kernel_resources": res.stdout.strip(), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
