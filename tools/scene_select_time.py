#!/usr/bin/env python3
"""Host wall clock of select_scene (footprints of every object's hypotheses into one pool of pixel rows, then the walk: one
stocs_scene_footprints call per object and one stocs_scene_select call) for pools of 6, 64 and 512 hypotheses of 2, 4 and 6 objects on a
640 x 480 frame rendered from the objects' true poses.  The yardstick, from the same visit, is the only route to this result before: one
explain_poses(labels=True) call per hypothesis (its record, and its agree pixels from the state image) plus the numpy walk of
tests/scene_ref.py.  Median of 20 calls after 5 warm-up calls, with the spread (min, max); the yardstick is timed over fewer passes
(recorded).  Asserts, before anything is timed, that the footprints equal the per-hypothesis records and that the selection equals the
restatement's walk on the per-hypothesis masks.  Needs a GPU; no fallback.

    python tools/scene_select_time.py [--out profiles/scene_select_time.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_ref  # noqa: E402
from depth_check_time import _rot, clock, perturbed, render  # noqa: E402

POOLS = ((6, 2), (64, 4), (512, 6))     # (hypotheses, objects)
REPS, WARM = 20, 5
K, SCALE, W, H = (600.0, 319.5, 600.0, 239.5), 1e-4, 640, 480


def build(n_obj, per_obj, seed):
    """-> (estimators, pools, true depth): n_obj copies of the asymmetric model at n_obj places of the frame, each with its own class image"""
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m = synth.make_model_asym(3000)
    rng = np.random.default_rng(seed)
    true, zs = [], []
    for k in range(n_obj):
        P = np.eye(4)
        P[:3, :3] = _rot(rng.normal(size=3), rng.uniform(0, 180))
        P[:3, 3] = (-0.25 + 0.25 * (k % 3), -0.1 + 0.2 * (k // 3), 0.7 + 0.05 * k)
        true.append(P)
        zs.append(render(m.pos, m.nrm, P, K, W, H, SCALE))
    depth = np.minimum.reduce(zs)
    sp = rng.normal(0, 0.05, (64, 3)).astype(np.float32)
    ests, pools = [], []
    for k in range(n_obj):
        prob = np.where(zs[k] < 15000, 10000, 0).astype(np.uint16)
        est = StocsEstimator(sp, sp / np.linalg.norm(sp, axis=1, keepdims=True), np.ones(64, np.float32), None, m.pos, m.nrm, build_index=False)
        est.set_frame(depth, prob, K, SCALE)
        ests.append(est)
        P = perturbed(true[k], per_obj, seed + 10 * k)
        P[0] = true[k].T.reshape(16)
        pools.append(P.astype(np.float32))
    return ests, pools


def old_route(ests, pools):
    """one explain_poses(labels=True) per hypothesis, then the numpy walk"""
    foot, masks, group = [], [], []
    for k, (est, P) in enumerate(zip(ests, pools)):
        for h in range(len(P)):
            rec, lab, st = est.explain_poses(P[h:h + 1], labels=True)
            m = ((st & 15) == 2).reshape(-1)
            foot.append((rec["footprint"][0], rec["no_depth"][0], rec["agree"][0], rec["in_front"][0], rec["behind"][0], rec["on_mask"][0], int(m.sum())))
            masks.append(m); group.append(k)
    foot = np.array(foot, scene_ref.RECORD_DTYPE)
    rec, sel = scene_ref.select(np.stack(masks), scene_ref.default_score(foot), np.array(group, np.int32), foot, len(ests))
    return foot, rec, sel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_select_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scene_select_time.py needs a GPU: no time is taken without one")
    from model_matching_amd.estimator import select_scene
    rows = []
    for n, n_obj in POOLS:
        ests, pools = build(n_obj, n // n_obj + (1 if n % n_obj else 0), 7 + n)
        pools[-1] = pools[-1][:n - sum(len(p) for p in pools[:-1])]
        got = select_scene(ests, pools)
        foot, rec, sel = old_route(ests, pools)
        assert scene_ref.records_equal(got["footprints"], foot) and scene_ref.records_equal(got["records"], rec) and np.array_equal(got["selected"], sel), n
        new = clock(lambda: select_scene(ests, pools), REPS, WARM)
        with_labels = clock(lambda: select_scene(ests, pools, labels=True), REPS, WARM)
        old_reps = 3 if n <= 64 else 1
        old = clock(lambda: old_route(ests, pools), reps=old_reps, warm=0)
        rows.append({"hypotheses": n, "objects": n_obj, "model_points": int(ests[0].nM), "select_scene": new, "select_scene_with_labels": with_labels,
                     "explain_per_hypothesis_plus_numpy_walk": dict(old, reps=old_reps), "equal_to_restatement": True, "selected": int(len(sel)),
                     "claimed_px": int(foot["claimed"].sum()), "reasons": np.bincount(rec["reason"], minlength=5).tolist()})
        print(json.dumps(rows[-1]), flush=True)
        for e in ests:
            e.close()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "scene.hip"], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    out = {"what": "host wall clock of select_scene (one stocs_scene_footprints call per object, one stocs_scene_select call; pool allocated and freed inside) next "
                   "to the route there was before: explain_poses(labels=True) once per hypothesis plus the numpy walk on the host",
           "device": torch.cuda.get_device_name(0), "frame": [W, H], "reps": REPS, "warmup": WARM,
           "note": "one visit, one GPU; the host column shares the machine with other work", "kernel_resources": res.stdout.strip(), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
