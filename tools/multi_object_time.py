#!/usr/bin/env python3
"""Several objects of one frame on the ycb example frame, K in {1, 2, 4, 8} class-probability maps (the frame's own map, then maps
derived from it by shifting it):
  (a) ingest: K calls of stocs_ingest_scene against one stocs_ingest_scene_multi;
  (b) depth image -> K poses: the sequential single-object path (per object: ingest_scene, set_scene, one trial of 100 base attempts)
      against one ingest_scene_multi plus the K objects' set_scene + trial on concurrent contexts (at most 4 host threads).
Every timed window ends in a synchronisation (the calls return host arrays); warm-up first, then the median of the repetitions, the
two forms interleaved.  The models cycle through the three example models; every context (model + PPF index) exists before the clock
starts, as for a stream of frames.  (b) checks that both forms give the same poses.
usage: python tools/multi_object_time.py [repetitions] [out.json]"""
import json
import os
import sys
import time

for _v in ("OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "NUMEXPR_NUM_THREADS"):
    os.environ.setdefault(_v, "1")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("STOCS_PIN_BLAS", "1")
from model_matching_amd.estimator import StocsEstimator, ingest_scene, ingest_scene_multi, preprocess_model  # noqa: E402

NAMES = ("ycb_024_bowl", "linemod_obj_06", "packed_dove")


def derived_maps(prob, k):
    shifts = [(0, 0), (0, 37), (-60, 0), (0, -90), (40, 40), (-30, 120), (80, -50), (0, 200)]
    return [np.ascontiguousarray(np.roll(np.roll(prob, dr, axis=0), dc, axis=1)) for dr, dc in shifts[:k]]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    from concurrent.futures import ThreadPoolExecutor
    raw = np.load(os.path.join(ROOT, "tests", "golden", "example_ycb_024_bowl_raw.npz"))
    K, ds = [float(x) for x in raw["K"]], float(raw["depth_scale"])
    depth, prob = np.ascontiguousarray(raw["depth"]), np.ascontiguousarray(raw["prob"])
    models = []
    for name in NAMES:
        r = np.load(os.path.join(ROOT, "tests", "golden", "example_%s_raw.npz" % name))
        models.append(preprocess_model(r["model_raw"], float(r["normal_radius"]), float(r["model_voxel"]), float(r["model_scale"])))
    rows = {}
    for k in (1, 2, 4, 8):
        maps = derived_maps(prob, k)
        # (a) ingest only
        for _ in range(5):
            [ingest_scene(depth, m, K, ds) for m in maps]; ingest_scene_multi(depth, maps, K, ds)
        ta, tb = [], []
        for _ in range(reps):
            t0 = time.perf_counter(); [ingest_scene(depth, m, K, ds) for m in maps]; t1 = time.perf_counter()
            ingest_scene_multi(depth, maps, K, ds); t2 = time.perf_counter()
            ta.append((t1 - t0) * 1e3); tb.append((t2 - t1) * 1e3)
        scenes = ingest_scene_multi(depth, maps, K, ds)
        # (b) depth -> K poses; one context per object, built before the clock
        ests = [StocsEstimator(*scenes[j], *models[j % 3], build_index=True) for j in range(k)]
        pool = ThreadPoolExecutor(min(4, k))

        def trial(j, sc, seed):
            est = ests[j]
            est.set_scene(*sc)
            est.sample_bases(seed, 100, mode=0, dispersion=0.9)
            est.find_congruent_all(); est.make_transforms(200, seed)
            lcp, idx, pose = est.compute_best_transform()
            return float(lcp), int(idx), pose.tobytes()

        def sequential(seed):
            return [trial(j, ingest_scene(depth, maps[j], K, ds), seed) for j in range(k)]

        def concurrent(seed):
            sc = ingest_scene_multi(depth, maps, K, ds)
            return list(pool.map(lambda j: trial(j, sc[j], seed), range(k)))

        for w in range(3):
            sequential(100 + w); concurrent(100 + w)
        ts, tc, same = [], [], True
        for r in range(reps):
            t0 = time.perf_counter(); a = sequential(200 + r); t1 = time.perf_counter()
            b = concurrent(200 + r); t2 = time.perf_counter()
            ts.append((t1 - t0) * 1e3); tc.append((t2 - t1) * 1e3)
            same = same and a == b
        pool.shutdown()
        for e in ests:
            e.close()
        med = lambda v: float(np.median(v))
        rows[str(k)] = {
            "points_per_object": [int(len(s[0])) for s in scenes],
            "ingest_ms": {"k_single_calls": med(ta), "one_multi_call": med(tb), "single_call_x1": med(ta) / k,
                          "multi_over_one_single_call": med(tb) / (med(ta) / k), "spread_multi_p10_p90": [float(np.percentile(tb, 10)), float(np.percentile(tb, 90))]},
            "frame_to_k_poses_ms": {"sequential_single_object": med(ts), "multi_ingest_concurrent_contexts": med(tc), "speedup": med(ts) / med(tc),
                                    "spread_concurrent_p10_p90": [float(np.percentile(tc, 10)), float(np.percentile(tc, 90))]},
            "same_poses_both_forms": bool(same)}
        print(k, json.dumps(rows[str(k)]), flush=True)
    rec = {"frame": "ycb_024_bowl (640x480)", "repetitions": reps, "warmup": "5 ingest pairs, 3 frame pairs", "by_objects": rows}
    print(json.dumps(rec, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
