#!/usr/bin/env python3
"""bench.py -- candidate poses verified / second on the metric configuration "Cm"
(synthetic 20 000-point scene vs 5 000-point model, 65 536 candidate transforms per step per GPU).

A step = one pass of the verification hot path over one batch that is already resident in HBM:
the batched weighted-LCP kernel over all candidates (reference src/stocs.cpp:1006-1041 per
candidate), the arg-max of compute_best_transform (stocs.cpp:982-1004) and, for N > 1, the RCCL
max all-reduce of the packed (score, candidate id) key over xGMI.  Every rank verifies its own
independent batch (weak scaling: StoCS trials shard one-per-GPU, no data-path collective).

Contract: python bench.py --gpus N --steps K --warmup W ; rank 0 prints ONE JSON line.

A plain run does only what that line's headline needs: set up, warm up, time the K steps, write --dump-outputs, print.  Everything
else it can measure or check -- the hit census and kernel roofline (live counters, the C5 leg), the untimed whole-path reports, the
CPU baselines and the oracle comparison of the whole batch -- comes with --full (the --no-* switches then skip parts of it).
"""
import argparse
import json
import os
import sys
import time

# The host-side bookkeeping around the trials is a few tiny numpy calls: keep the BLAS / OpenMP pools to one thread.  On the GPU boxes
# the process sees 256 CPUs but its cgroup has a quota of 16; OpenBLAS sizes its pool by the former, its spinning workers exhaust the
# latter, and the kernel then freezes the whole process for the rest of a 100 ms period -- the sporadic 65-80 ms "stall" of rounds
# 1-3 (profiles/r03_stall_root_cause.json).  Must happen before numpy is imported.
for _v in ("OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "NUMEXPR_NUM_THREADS"):
    os.environ.setdefault(_v, "1")
os.environ.setdefault("STOCS_PIN_BLAS", "1")   # harness side (importing the library itself has no side effects)

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


PEAK_HBM_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E ~8 TB/s
NEEDED_BYTES_PER_HIT = 28      # one nearest scene record: position 12 + normal 12 + class probability 4


def kernel_record(est, dT, kcand, dL, reps, workload, candidates_arg, run_pmc, groups=None, prefix="", count_hits=True, hits_counted=None):
    """Flat, scalar-only description of the dominant kernel for one workload -- everything a reader needs to recompute it:
    * contract figure: ALGORITHMIC bytes (68 + 52 |M| per pose) / kernel time / HBM peak.  Not a ceiling on
      cache-resident workloads: it charges a scene record to every model point and the model to every pose.
    * needed bytes: what a pose cannot do without -- 64-byte transform in, 4-byte score out, and ONE 28-byte scene record per
      model point that really has a neighbour within epsilon (hits counted by the kernel's own per-point detail form over the
      whole batch, stocs_lcp_hit_count).  needed_frac = needed bytes / kernel time / HBM peak is <= 1 by construction and can be
      recomputed from the kernel's average duration in profiles/r04_*_kernel_stats.csv.
    * counters of THIS command (child rocprofv3 --pmc passes, tools/pmc.py): L2 memory-side bytes (FETCH_SIZE x2 + WRITE_SIZE; the
      guide: Infinity-Cache hits are counted, so this is NOT pure HBM), L2 -> L1 bytes, unit utilisations, and the binding unit."""
    b_pose = 68 + 52 * est.nM
    k_ms = est.time_score_kernel(dT, kcand, dL, reps)
    hits, counted = hits_counted if hits_counted is not None else (est.lcp_hit_count(dT, kcand) if count_hits else (0, 0))
    needed = float(hits) * NEEDED_BYTES_PER_HIT + 68.0 * kcand
    sec = k_ms * 1e-3
    rec = {
        "kernel_ms": k_ms, "kernel_timed_launches": reps, "kernel_poses_per_s": kcand / sec,
        "nn_queries_per_s": kcand * float(est.nM) / sec,
        "algorithmic_bytes_per_launch": float(b_pose) * kcand,
        "contract_frac": float(b_pose) * kcand / sec / 1e9 / PEAK_HBM_GBS,
        "hits_per_pose": hits / float(kcand), "hit_fraction_of_queries": hits / (float(kcand) * est.nM),
        "counted_per_pose": counted / float(kcand),
        "needed_bytes_per_launch": needed, "needed_frac": needed / sec / 1e9 / PEAK_HBM_GBS,
        "memory_side_bytes_per_launch": None, "memory_side_frac": None, "traffic_over_needed": None, "traffic_over_algorithmic": None,
        "l2_to_l1_bytes_per_launch_64B": None, "l2_to_l1_bytes_per_launch_128B": None, "l2_to_l1_frac_64B": None, "l2_to_l1_frac_128B": None,
        "l2_hit_rate": None, "ta_busy_frac": None, "valu_issue_frac": None, "wave_wait_frac": None, "waves_per_simd_avg": None,
        "binding_unit": None, "binding_frac": None,
    }
    nested = {"pmc": None, "binding": None}
    if run_pmc:
        add_counters(rec, nested, workload, candidates_arg, groups)
    if prefix:
        rec = {prefix + k: v for k, v in rec.items()}
    return rec, nested


def add_counters(rec, nested, workload, candidates_arg, groups=None):
    """Counters of the command that produced `rec` (un-prefixed keys): child rocprofv3 --pmc passes of this script (tools/pmc.py)."""
    import os, shutil, sys, tempfile
    k_ms, needed, algorithmic = rec["kernel_ms"], rec["needed_bytes_per_launch"], rec["algorithmic_bytes_per_launch"]
    sec = k_ms * 1e-3
    try:
        root = os.path.dirname(os.path.abspath(__file__))
        sys.path.insert(0, os.path.join(root, "tools"))
        import pmc as pmc_tool
        if shutil.which("rocprofv3"):
            pdir = tempfile.mkdtemp(prefix="stocs_pmc_")
            child = ["python3", os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1",     # a plain run: the timed steps alone
                     "--details", os.devnull, "--workload", workload] + (["--candidates", str(candidates_arg)] if candidates_arg else [])
            grp = pmc_tool.GROUPS if not groups else type(pmc_tool.GROUPS)((g, pmc_tool.GROUPS[g]) for g in groups if g in pmc_tool.GROUPS)
            raw = pmc_tool.collect("lcp_coopq_kernel<false", child, pdir, groups=grp)   # the scoring kernel, not its per-point detail form (<true, ...>)
            der = pmc_tool.derive(raw, k_ms)
            shutil.rmtree(pdir, ignore_errors=True)
            mem = der.get("hbm_bytes_per_launch")
            if mem is not None:
                rec["memory_side_bytes_per_launch"] = mem
                rec["memory_side_frac"] = mem / sec / 1e9 / PEAK_HBM_GBS
                rec["traffic_over_needed"] = mem / needed
                rec["traffic_over_algorithmic"] = mem / algorithmic
            l2b = der.get("l2_bytes_per_launch_64B_128B")
            if l2b:
                rec["l2_to_l1_bytes_per_launch_64B"], rec["l2_to_l1_bytes_per_launch_128B"] = l2b
                rec["l2_to_l1_frac_64B"], rec["l2_to_l1_frac_128B"] = der["l2_bw_frac_64B_128B"]
            for k in ("l2_hit_rate", "ta_busy_frac", "valu_issue_frac", "wave_wait_frac", "waves_per_simd_avg"):
                rec[k] = der.get(k)
            b = der.get("binding")
            if b:
                # the memory-side figure is named for what it is (the guide: FETCH_SIZE counts the L2's fabric requests, Infinity-Cache hits included)
                name = {"hbm_fabric": "l2_memory_side"}.get(b["bound"], b["bound"])
                rec["binding_unit"], rec["binding_frac"] = name, b["frac"]
                nested["binding"] = dict(b, bound=name, all={{"hbm_fabric": "l2_memory_side"}.get(k, k): v for k, v in b["all"].items()})
            nested["pmc"] = {"kernel": raw["kernel"], "passes": raw["passes"], "counters_per_launch": {k: v["per_launch_mean"] for k, v in raw["counters"].items()},
                             "source": "rocprofv3 --pmc child runs of this command (tools/pmc.py), launched by this bench process"}
        else:
            nested["pmc"] = {"error": "rocprofv3 not found"}
    except Exception as e:   # the bench line must not depend on the profiler
        nested["pmc"] = {"error": repr(e)}


def c5_leg(device, run_pmc, groups, launches=8, oracle_candidates=256):
    """The one configuration whose lists do not stay in any cache (SURVEY 8d "C5": 200 000-point scene, 50 000-point model, 16 384
    candidates): a few timed launches with the same record as Cm, and an oracle check of the first candidates."""
    import numpy as np
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    model, scene, kcand = synth.workload("C5")
    est = StocsEstimator(scene.pos, scene.nrm, scene.prob, scene.pixel, model.pos, model.nrm, build_index=False, device=device)
    cs = est.get_scene_centroid().astype(np.float64); cm = est.get_model_centroid().astype(np.float64)
    T = synth.make_candidates(synth.centred_gt(scene.T_gt, cs, cm), kcand, seed=synth.SEED_CAND)
    dT = est.dev_alloc(T.nbytes); dL = est.dev_alloc(kcand * 4)
    est.dev_upload(dT, T)
    lcp = np.zeros(kcand, np.float32)
    for _ in range(3):      # warm: the patch test's distance field is filled once the scene has seen 1e9 point queries
        est.score_device(dT, kcand, dL)
    est.sync()
    rec, nested = kernel_record(est, dT, kcand, dL, launches, "C5", 0, run_pmc, groups, prefix="c5_")
    est.score_device(dT, kcand, dL)
    est.dev_download(dL, lcp)
    rec["c5_workload"] = "C5: synthetic %d-pt scene vs %d-pt model, %d candidate transforms per launch, eps=5mm" % (est.nS, est.nM, kcand)
    try:
        from oracle import pyoracle
        pyoracle.build()
        orc = pyoracle.Oracle(scene.pos, scene.nrm, scene.prob, scene.pixel, model.pos, model.nrm, build_index=False)
        nth = max(1, min(16, len(os.sched_getaffinity(0))))
        ref = orc.lcp_batch(T[:oracle_candidates], nthreads=nth)
        d = np.abs(ref - lcp[:oracle_candidates])
        rec["c5_oracle_candidates_compared"] = int(oracle_candidates)
        rec["c5_oracle_max_abs_lcp_diff"] = float(d.max())
        rec["c5_oracle_candidates_over_1e-5"] = int((d > 1e-5).sum())   # only exact-distance ties of the lattice-sampled scene (Q11) get here
    except Exception as e:
        rec["c5_oracle_error"] = repr(e)
    est.dev_free(dT); est.dev_free(dL)
    est.close()
    return rec, nested


def pipeline_report(model, scene, device, n_runs=8, batch_trials=16):
    """The whole hot path outside the timed region: index build, then StoCS trials of 100 base attempts through the four entry points
    (sample -> congruent sets -> <= 200 transforms per base -> verification), host wall clock; the winners against the synthetic
    ground truth; and the same trials as ONE batch through stocs_run_trials (every trial of the batch in one set of launches)."""
    import numpy as np
    from model_matching_amd.estimator import StocsEstimator
    # secondary, outside the timed region: the whole hot path once (index build, phases 1-4)
    t = time.perf_counter()
    pe = StocsEstimator(scene.pos, scene.nrm, scene.prob, scene.pixel, model.pos, model.nrm, build_index=True, device=device)
    pe.sync()
    t_idx = time.perf_counter() - t
    runs = []
    from scipy.spatial import cKDTree
    gt_pts = model.pos.astype(np.float64) @ np.asarray(scene.T_gt, np.float64)[:3, :3].T + np.asarray(scene.T_gt, np.float64)[:3, 3]
    gt_tree = cKDTree(gt_pts)
    # the trials run back to back, as a trial stream does; the comparison of each winner with the synthetic ground truth (a
    # kd-tree query and float64 products on the host, milliseconds during which the GPU would idle and clock down) comes after
    raw = []
    for r in range(n_runs):
        pe.L.stocs_clear_bases(pe.h)
        n_alloc0 = int(pe.L.stocs_device_alloc_count())
        t0 = time.perf_counter(); valid, _, _ = pe.sample_bases(1234 + r, 100)
        t1 = time.perf_counter(); nq = pe.find_congruent_all()
        t2 = time.perf_counter(); nc = pe.make_transforms(200, 1234 + r)
        t3 = time.perf_counter(); bl, bi, P = pe.compute_best_transform()
        t4 = time.perf_counter()
        raw.append((r, int(valid.sum()), int(nq), int(nc), float(bl), P.copy(), (t0, t1, t2, t3, t4), int(pe.L.stocs_device_alloc_count()) - n_alloc0,
                    # host wall clock of the steps inside the three calls (always recorded by the library): a stalled run names its step
                    {name: [[lab, round(ms, 4)] for lab, ms in pe.last_call_timing(w)]
                     for w, name in ((0, "find_congruent_all"), (1, "make_transforms"), (2, "verify_all"))}))
    for r, n_valid, nq, nc, bl, P, (t0, t1, t2, t3, t4), n_alloc, steps in raw:
        # winner vs the synthetic ground truth (camera frame, SURVEY.md 8(d): <= 1 mm / 1 deg is the oracle-vs-GPU
        # bar; against the noisy scene the estimate itself is limited by eps = 5 mm)
        Pm = P.reshape(4, 4).T.astype(np.float64)
        dR = Pm[:3, :3] @ np.asarray(scene.T_gt, np.float64)[:3, :3].T
        rot_err = float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))))
        c0 = model.pos.astype(np.float64).mean(0)
        tr_err = float(np.linalg.norm((Pm[:3, :3] @ c0 + Pm[:3, 3]) - (np.asarray(scene.T_gt)[:3, :3] @ c0 + np.asarray(scene.T_gt)[:3, 3])) * 1e3)
        est_pts = model.pos.astype(np.float64) @ Pm[:3, :3].T + Pm[:3, 3]
        add_s = float(gt_tree.query(est_pts)[0].mean() * 1e3)   # symmetry-aware: mean closest-point distance (ADD-S)
        add = float(np.linalg.norm(est_pts - gt_pts, axis=1).mean() * 1e3)   # point-to-same-point distance (ADD): meaningful on a model without symmetry
        runs.append({"warmup": r < 2, "bases": n_valid, "congruent_quads": nq, "candidates": nc, "best_lcp": bl,
                     "winner_rot_err_deg_vs_gt": rot_err, "winner_centroid_err_mm_vs_gt": tr_err, "winner_add_s_mm_vs_gt": add_s, "winner_add_mm_vs_gt": add,
                     "sample_ms": (t1 - t0) * 1e3, "congruent_ms": (t2 - t1) * 1e3, "transforms_ms": (t3 - t2) * 1e3,
                     "verify_ms": (t4 - t3) * 1e3, "poses_per_s_phases_2_4": nc / max(t4 - t1, 1e-9),
                     "device_allocations_during_trial": n_alloc, "steps_ms": steps})
    # per-frame cost of a new scene against the same model: scene upload + GPU grid build (the index is kept)
    t_set = []
    for r in range(4):
        t0 = time.perf_counter()
        pe.set_scene(scene.pos, scene.nrm, scene.prob, scene.pixel)
        pe.sync()
        t_set.append((time.perf_counter() - t0) * 1e3)
    rep = {"note": "StoCS trial streams of 100 base attempts, <=200 quads per base, host wall clock incl. launches "
                               "and copies; the first two runs grow the context's arenas (one-time hipMalloc, counted in device_allocations_during_trial) and are marked warmup. "
                               "On the metric model -- a near-symmetric ellipsoid of revolution (SURVEY 8d) -- the rotation about its "
                               "axis is barely observable, so the rotation error is reported next to the symmetry-aware ADD-S; "
                               "pipeline_asymmetric_model repeats the report on a model without symmetry", "context_plus_index_build_s": t_idx, "set_scene_ms": float(np.median(t_set)), "runs": runs,
                       "steady_state_poses_per_s_phases_2_4": float(np.mean([x["poses_per_s_phases_2_4"] for x in runs if not x["warmup"]])),
                       # the median next to the mean: on the shared GPU hosts a runtime call now and then stalls for tens of
                       # milliseconds (seen in about one trial of 300 in round 2, with zero device allocations in the stalled
                       # trial); such a run is listed with the others and flagged here
                       "steady_state_median_poses_per_s_phases_2_4": float(np.median([x["poses_per_s_phases_2_4"] for x in runs if not x["warmup"]])),
                       "runs_with_a_phase_over_10x_its_median": [i for i, x in enumerate(runs) if not x["warmup"] and any(
                           x[k] > 10.0 * float(np.median([y[k] for y in runs if not y["warmup"]])) for k in ("sample_ms", "congruent_ms", "transforms_ms", "verify_ms"))]}
    pe.close()
    # the same kind of trials as ONE batch (stocs_run_trials): every launch shared by all of them
    pe2 = StocsEstimator(scene.pos, scene.nrm, scene.prob, scene.pixel, model.pos, model.nrm, build_index=True, device=device)
    seeds = [5000 + i for i in range(batch_trials)]
    pe2.run_trials(seeds, 100)                                   # sizes the arenas of the batched form
    tb = time.perf_counter()
    res = pe2.run_trials(seeds, 100)
    dtb = time.perf_counter() - tb
    best = max(res, key=lambda x: x["best_lcp"])
    Pm = best["best_pose"].reshape(4, 4).T.astype(np.float64)
    Tg = np.asarray(scene.T_gt, np.float64)
    dR = Pm[:3, :3] @ Tg[:3, :3].T
    est_pts = model.pos.astype(np.float64) @ Pm[:3, :3].T + Pm[:3, 3]
    rep["batched_trials"] = {"trials": batch_trials, "seconds": dtb, "trials_per_s": batch_trials / dtb,
                             "candidates_verified": int(sum(x["n_candidates"] for x in res)),
                             "poses_per_s_all_phases": float(sum(x["n_candidates"] for x in res)) / dtb,
                             "best_lcp_of_the_batch": best["best_lcp"],
                             "best_rot_err_deg_vs_gt": float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))),
                             "best_add_mm_vs_gt": float(np.linalg.norm(est_pts - gt_pts, axis=1).mean() * 1e3),
                             "best_add_s_mm_vs_gt": float(gt_tree.query(est_pts)[0].mean() * 1e3),
                             "phases_ms": [[lab, round(ms, 4)] for lab, ms in pe2.last_call_timing(3)]}
    pe2.close()
    return rep



def _sig(x, n=6):
    """Floats to n significant digits (the contract line must stay small); everything else unchanged."""
    if isinstance(x, bool) or x is None:
        return x
    if isinstance(x, float):
        if x != x or x in (float("inf"), float("-inf")):
            return None
        return float("%.*g" % (n, x))
    if isinstance(x, (list, tuple)):
        return [_sig(v, n) for v in x]
    if isinstance(x, dict):
        return {k: _sig(v, n) for k, v in x.items()}
    if isinstance(x, (np.floating,)):
        return _sig(float(x), n)
    if isinstance(x, (np.integer,)):
        return int(x)
    return x


ROOFLINE_KEYS = ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel_ms", "contract_frac", "needed_frac", "memory_side_frac",
                 "traffic_over_needed", "binding_unit", "binding_frac", "hits_per_pose", "ta_busy_frac", "valu_issue_frac", "l2_to_l1_frac_128B",
                 "c5_kernel_ms", "c5_kernel_poses_per_s", "c5_contract_frac", "c5_needed_frac", "c5_memory_side_bytes_per_launch", "c5_memory_side_frac",
                 "c5_traffic_over_needed", "c5_binding_unit", "c5_binding_frac", "c5_hits_per_pose", "c5_oracle_max_abs_lcp_diff")
COMPACT_LIMIT = 4096


def compact_line(full):
    """The contract line: ONE small JSON object (< 4 KB) with scalars only -- the contract keys, a flat roofline, the CPU baselines, the
    oracle check and the medians of the whole-path sections.  Everything else (per-run tables, step records, counter nests, notes) lives
    in bench_details.json next to this script.  Round 4's line had grown to 34 KB and the driver could not parse it."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    out = {k: full.get(k) for k in keep}
    cfg = full.get("config", {})
    out["config"] = {k: cfg.get(k) for k in ("workload", "candidates_per_step_per_gpu", "scene_points", "model_points", "parallelism")}
    out["final_lcp_percent"] = full.get("final_lcp_percent")
    if full.get("rehearsal"):
        out["rehearsal"] = True                                 # (ranks sharing one GPU over gloo: never a measurement)
    di = full.get("distributed")
    if di:
        out["distributed"] = {"world_size": di.get("world_size"), "backend": di.get("backend"), "ranks_reporting": [r.get("rank") for r in di.get("ranks", [])][:8]}
    rf = full.get("roofline")
    if rf:                                                      # (--full only)
        out["roofline"] = {k: rf.get(k) for k in ROOFLINE_KEYS if k in rf}
    cb = full.get("cpu_baseline")
    if cb:
        out["cpu_baseline"] = {k: cb.get(k) for k in ("value", "unit", "cores", "kind", "sample")}
    ca = full.get("cpu_baseline_all_cores")
    if ca:
        out["cpu_baseline_all_cores"] = {"value": ca.get("value"), "cores": ca.get("cores")}
    oc = full.get("oracle_check")
    if oc:
        out["oracle_check"] = {k: oc.get(k) for k in ("candidates_compared", "max_abs_lcp_diff_vs_gpu", "within_tolerance")}
    pl = full.get("pipeline")
    if pl:
        runs = [r for r in pl.get("runs", []) if not r.get("warmup")]
        if runs:
            out["pipeline_poses_per_s_phases_2_4"] = float(np.median([r["poses_per_s_phases_2_4"] for r in runs]))
            out["pipeline_ms"] = [float(np.median([r[k] for r in runs])) for k in ("sample_ms", "congruent_ms", "transforms_ms", "verify_ms")]
            out["pipeline_candidates_per_trial"] = float(np.median([r["candidates"] for r in runs]))
        bt = pl.get("batched_trials")
        if bt:
            out["batched_trials_per_s"] = bt.get("trials_per_s")
            out["batched_poses_per_s_all_phases"] = bt.get("poses_per_s_all_phases")
    pa = full.get("pipeline_asymmetric_model")
    if pa:
        runs = [r for r in pa.get("runs", []) if not r.get("warmup")]
        if runs:
            out["winner_single_trial_rot_err_deg"] = float(np.median([r["winner_rot_err_deg_vs_gt"] for r in runs]))
            out["winner_single_trial_add_mm"] = float(np.median([r["winner_add_mm_vs_gt"] for r in runs]))
        bt = pa.get("batched_trials")
        if bt:
            out["winner_best_of_batch_rot_err_deg"] = bt.get("best_rot_err_deg_vs_gt")
            out["winner_best_of_batch_add_mm"] = bt.get("best_add_mm_vs_gt")
    cp = full.get("cpu_baseline_pipeline")
    if cp:
        for k in ("cpu_pipeline_ms", "cpu_pipeline_poses_per_s_phases_2_4", "cpu_pipeline_attempts", "cpu_pipeline_cores",
                  "ycb_cpu_trial_ms", "ycb_cpu_trials_per_s", "ycb_gpu_trial_ms", "ycb_gpu_trials_per_s_single", "ycb_gpu_trials_per_s_batch64"):
            if k in cp:
                out[k] = cp[k]
    out["details"] = full.get("details_file")
    out = _sig(out)
    # never over the limit: drop the optional tail first, the contract keys never
    for victim in ("winner_best_of_batch_add_mm", "winner_best_of_batch_rot_err_deg", "winner_single_trial_add_mm", "winner_single_trial_rot_err_deg",
                   "pipeline_candidates_per_trial", "ycb_gpu_trial_ms", "ycb_cpu_trial_ms", "pipeline_ms", "cpu_pipeline_ms", "oracle_check", "cpu_baseline_all_cores"):
        if len(json.dumps(out)) < COMPACT_LIMIT:
            break
        out.pop(victim, None)
    return out


DUMP_MAX_SCORES = 4 << 20      # 16 MB of float32 scores; a larger batch is dumped as a fixed sample (+ its float64 indices)


def dump_outputs(out_dir, lcp, best_lcp, best_gid):
    """--dump-outputs: what a caller of the timed path receives from its last step -- every candidate's LCP score and the
    arg-max key unpacked (score, global candidate id) -- as .npy files.  The inputs are seeded (synth), so two builds run
    with the same arguments can be compared file for file."""
    os.makedirs(out_dir, exist_ok=True)
    scores = np.ascontiguousarray(lcp, np.float32)
    if len(scores) > DUMP_MAX_SCORES:
        idx = np.sort(np.random.Generator(np.random.PCG64(0x5EED00D0)).choice(len(scores), DUMP_MAX_SCORES, replace=False))
        np.save(os.path.join(out_dir, "lcp_scores_sample_index.npy"), idx.astype(np.float64))
        scores = scores[idx]
    np.save(os.path.join(out_dir, "lcp_scores.npy"), scores)
    np.save(os.path.join(out_dir, "best_lcp.npy"), np.array([best_lcp], np.float32))
    np.save(os.path.join(out_dir, "best_candidate_id.npy"), np.array([best_gid], np.float64))


def cpu_pipeline_baseline(model, scene, device, threads, cm_attempts=8):
    """The reference's CPU path over the WHOLE path, beside the GPU's whole-path numbers: the oracle's restated run_stocs_estimation
    (oracle/stocs_oracle.cpp orc_run_mode, one thread like the reference) reports the same three spans the reference's driver prints --
    base sampling / congruent sets + transforms / verification (src/stocs_match_one_object.cpp:80-105,110-151,156-163).
    * Cm: `cm_attempts` of the 100 base attempts (a Cm trial takes the CPU about a minute: 45-190 M congruent sets are materialised),
      spans scaled to 100 attempts; candidate poses / s over phases 2-4 = candidates / (congruent + verify span).
    * the ycb 024_bowl frame (BASELINE configs 1/2; tests/golden fixture): one whole trial, 100 attempts, <= 200 per base, next to the
      same trial on the GPU -- through the four calls, and 64 of them as one batch."""
    from oracle import pyoracle
    from model_matching_amd.estimator import StocsEstimator
    pyoracle.build()
    pyoracle.set_index_build_threads(threads)
    rec = {"cpu_pipeline_cores": 1, "cpu_pipeline_attempts": cm_attempts, "kind": "port",
           "what": "oracle run_stocs_estimation, one core; index build (offline in the reference) not in any span"}
    t = time.perf_counter()
    orc = pyoracle.Oracle(scene.pos, scene.nrm, scene.prob, scene.pixel, model.pos, model.nrm, build_index=True)
    rec["cm_cpu_index_build_s"] = time.perf_counter() - t
    rec["cm_cpu_index_build_threads"] = threads
    r = orc.run(1234, cm_attempts, 200)
    sc = 100.0 / max(cm_attempts, 1)
    rec["cm_cpu_spans_s"] = [r.t_sample_s, r.t_congruent_s, r.t_verify_s]
    rec["cm_cpu_bases_quads_candidates"] = [int(r.n_bases), int(r.n_quads_total), int(r.n_candidates)]
    rec["cpu_pipeline_ms"] = [r.t_sample_s * sc * 1e3, r.t_congruent_s * sc * 1e3, r.t_verify_s * sc * 1e3]
    rec["cpu_pipeline_poses_per_s_phases_2_4"] = r.n_candidates / max(r.t_congruent_s + r.t_verify_s, 1e-9)
    del orc
    gold = os.path.join(ROOT, "tests", "golden", "example_ycb_024_bowl.npz")
    if os.path.exists(gold):
        d = np.load(gold)
        orc = pyoracle.Oracle(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
        t = time.perf_counter()
        r = orc.run(1234, 100, 200)
        dt = time.perf_counter() - t
        rec["ycb_cpu_trial_ms"] = [r.t_sample_s * 1e3, r.t_congruent_s * 1e3, r.t_verify_s * 1e3]
        rec["ycb_cpu_trials_per_s"] = 1.0 / max(dt, 1e-9)
        rec["ycb_cpu_bases_quads_candidates_lcp"] = [int(r.n_bases), int(r.n_quads_total), int(r.n_candidates), float(r.best_lcp)]
        del orc
        est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True, device=device)
        spans = []
        for k in range(6):
            est.reset_trial()
            t0 = time.perf_counter(); est.sample_bases(1234 + k, 100)
            t1 = time.perf_counter(); est.find_congruent_all()
            t2 = time.perf_counter(); est.make_transforms(200, 1234 + k)
            t3 = time.perf_counter(); bl, bi, P = est.compute_best_transform()
            t4 = time.perf_counter()
            spans.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3))
            if k == 0:
                rec["ycb_gpu_same_seed_bases_quads_candidates_lcp"] = [int(est.L.stocs_num_bases(est.h)), None, None, float(bl)]
        med = [float(np.median([s_[i] for s_ in spans[2:]])) for i in range(4)]
        rec["ycb_gpu_trial_ms"] = med
        rec["ycb_gpu_trials_per_s_single"] = 1e3 / max(sum(med), 1e-9)
        seeds = [7000 + i for i in range(64)]
        est.run_trials(seeds, 100)
        t0 = time.perf_counter(); est.run_trials(seeds, 100); dtb = time.perf_counter() - t0
        rec["ycb_gpu_trials_per_s_batch64"] = 64.0 / dtb
        est.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)     # ~0.65 s of timed region at Cm: long enough for rocm-smi to see it
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="Cm", choices=["Cm", "C5", "small", "tiny"])
    ap.add_argument("--candidates", type=int, default=0, help="override candidates per step per GPU")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check, outside the timed steps, everything beyond the headline: hit census and kernel roofline (live counters, "
                         "C5 leg), the untimed whole-path reports, the CPU baselines and the oracle comparison of the whole batch")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true", help="skip the untimed phases 1-4 report")
    ap.add_argument("--cpu-seconds", type=float, default=8.0)
    ap.add_argument("--no-pmc", action="store_true", help="skip the live rocprofv3 counter passes (roofline.traffic / binding become null)")
    ap.add_argument("--no-c5", action="store_true", help="skip the C5 leg of the roofline record (200 000-point scene, 50 000-point model: the HBM-bound configuration)")
    ap.add_argument("--no-prewarm", action="store_true", help="skip the 120 ms of untimed scoring launches that bring an idle chip to its sustained clocks")
    ap.add_argument("--no-hits", action="store_true", help="skip the hit census behind needed_bytes (its per-point detail launches, ~30 ms of device work in front of the warm-up)")
    ap.add_argument("--no-cpu-pipeline", action="store_true", help="skip the CPU whole-path baseline (oracle run_stocs_estimation at Cm and on the ycb frame)")
    ap.add_argument("--details", default="", help="where the full record goes (default: bench_details.json next to this script, and gpurun_out/ when it exists)")
    ap.add_argument("--pmc-groups", default="", help="comma-separated counter groups of tools/pmc.py for the live passes (default: all)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step computed (rank 0's scores, the arg-max over all ranks) to DIR/<name>.npy, to compare two builds")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # --gpus N > 1 without a launcher around it: this process becomes the launcher of N rank children (before torch or the
    # GPU runtime is loaded) and relays rank 0's JSON line; it never runs one rank under an N-GPU label
    from model_matching_amd import dist as sdist
    sdist.launch_ranks_if_needed(args.gpus, os.path.abspath(__file__), sys.argv[1:])
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE=%d does not match --gpus %d" % (world, args.gpus))

    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback)")
    # STOCS_BENCH_REHEARSAL=1: every rank shares GPU 0 and the collective runs over gloo -- only to
    # rehearse the N > 1 code path on a one-GPU box; never a measurement
    rehearsal = os.environ.get("STOCS_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator

    model, scene, kcand = synth.workload(args.workload)
    if args.candidates:
        kcand = args.candidates
    est = StocsEstimator(scene.pos, scene.nrm, scene.prob, scene.pixel, model.pos, model.nrm,
                         build_index=False, device=local_rank)
    cs = est.get_scene_centroid().astype(np.float64)
    cm = est.get_model_centroid().astype(np.float64)
    Tgt = synth.centred_gt(scene.T_gt, cs, cm)
    # every rank verifies its own independent batch (different seed) -- weak scaling
    T = synth.make_candidates(Tgt, kcand, seed=synth.SEED_CAND + rank)
    dT = est.dev_alloc(T.nbytes)
    dL = est.dev_alloc(kcand * 4)
    est.dev_upload(dT, T)
    lcp = np.zeros(kcand, np.float32)

    # All work of a step is enqueued on PyTorch's current HIP stream: LCP kernel with the device arg-max in its epilogue into an
    # 8-byte torch tensor -- no host round trip per step.  With N > 1 the RCCL max all-reduce of that key (8 bytes over xGMI,
    # latency-bound) runs on a SIDE stream behind an event, on the buffer of step k, while the compute stream already scores step
    # k + 1 into the other buffer: the collective is off the critical path (round 3 enqueued it on the compute stream: ~30 us per
    # 1.1 ms step).  A buffer is rewritten at step k + 2 only behind the event that closes its all-reduce.
    est.set_stream(torch.cuda.current_stream().cuda_stream)
    keys = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2)]
    overlap = world > 1 and not rehearsal
    comm_stream = torch.cuda.Stream() if overlap else None
    scored = [torch.cuda.Event() for _ in range(2)] if overlap else None
    reduced = [torch.cuda.Event() for _ in range(2)] if overlap else None
    state = {"k": 0}

    def step():
        i = state["k"] & 1
        state["k"] += 1
        key = keys[i]
        compute = torch.cuda.current_stream()
        if overlap and state["k"] > 2:
            compute.wait_event(reduced[i])                                    # the all-reduce of step k - 2 has read and written this buffer
        # the metric kernel; its epilogue takes compute_best_transform's arg-max (first maximum wins, stocs.cpp:994) into `key`
        est.score_best_device_async(dT, kcand, dL, rank * kcand, key.data_ptr())
        if overlap:
            scored[i].record(compute)
            with torch.cuda.stream(comm_stream):
                comm_stream.wait_event(scored[i])
                dist.all_reduce(key, op=dist.ReduceOp.MAX)                    # 8 bytes over xGMI, next to the next step's kernel
                reduced[i].record(comm_stream)
        elif world > 1:                                                       # rehearsal: gloo on the host, synchronous
            k = key.cpu()
            dist.all_reduce(k, op=dist.ReduceOp.MAX)
            key.copy_(k)

    # The hit census behind needed_bytes (the per-point detail form of the kernel over the whole batch, ~30 ms of device work) comes
    # first: it is a measurement of the same batch, and taking it in front leaves the chip at its working clocks for the W warm-up steps
    # and the K timed ones (a 20-step timed region is 24 ms: after 5 warm-up steps from idle it ran 7 % below the 400-step rate in
    # round 3).  The timed region below is unchanged: W untimed steps, then exactly K; the kernel's own clock is taken after it.
    # (--full only: a plain run has the pre-warm below in front of its warm-up steps)
    hits_counted = est.lcp_hit_count(dT, kcand) if args.full and not args.no_hits else (0, 0)
    # An idle MI355X needs ~60-100 ms of load to reach its sustained clocks (kernel trace of this command: the same launch takes 1.39, 1.17, 1.13,
    # ... 0.98 ms over the first 25 launches and 0.95 from the 35th on), longer than the driver's whole 5 + 20-step run.  So the chip is brought
    # to its working state first -- the same scoring launch, untimed, for a fixed 120 ms -- and then the contract runs as written: W untimed
    # steps, exactly K timed ones.  Nothing is skipped inside the timed region; `pre_warm_ms` in the details file says how long this took.
    t_pw = time.perf_counter()
    if not args.no_prewarm:
        while time.perf_counter() - t_pw < 0.12:
            for _ in range(8):
                est.score_device(dT, kcand, dL)
            est.sync()
    pre_warm_ms = (time.perf_counter() - t_pw) * 1e3
    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    dt_local = dt
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device="cpu" if rehearsal else "cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    poses = float(kcand) * args.steps * world
    value = poses / dt

    key = keys[(state["k"] - 1) & 1]                      # the last step's buffer (torch.cuda.synchronize above covers the side stream)
    final_key = int(key.item())
    final_lcp, final_gid = sdist.unpack_best(final_key) if final_key else (0.0, -1)
    if args.full or (rank == 0 and args.dump_outputs):
        est.dev_download(dL, lcp)                         # every candidate's score of the last step
        if world == 1:
            i_chk = int(np.argmax(lcp))
            assert final_gid == i_chk and final_lcp == float(lcp[i_chk]), (final_gid, i_chk)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, lcp, final_lcp, final_gid)
    run_pmc = args.full and rank == 0 and world == 1 and not args.no_pmc
    groups = [g for g in args.pmc_groups.split(",") if g] or None

    out = {
        "metric": "candidate poses verified/sec",
        "value": value,
        "unit": "poses/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "%s: synthetic %d-pt scene vs %d-pt model, %d candidate transforms per step per GPU, "
                               "eps=5mm" % (args.workload, est.nS, est.nM, kcand),
                   "candidates_per_step_per_gpu": kcand, "scene_points": est.nS, "model_points": est.nM,
                   "parallelism": "independent trial batches, one per GPU; 8-byte RCCL max all-reduce per step, on a side stream next to the following step"},
        "rehearsal": rehearsal,
        "pre_warm_ms": pre_warm_ms,
        "final_lcp_percent": float(final_lcp) * 100.0,
        "best_global_candidate_id": int(final_gid),
    }
    if args.full:
        # roofline of the dominant kernel: HIP events on the context's stream, resident inputs
        b_pose = 68 + 52 * est.nM                      # algorithmic bytes per pose
        reps = max(5, min(args.steps, 400))
        krec, knest = kernel_record(est, dT, kcand, dL, reps, args.workload, args.candidates, False, hits_counted=hits_counted)   # (counters: after the pipeline section, below)
        k_ms = krec["kernel_ms"]
        achieved = b_pose * kcand / (k_ms * 1e-3) / 1e9   # GB/s
        peak = PEAK_HBM_GBS
        out["roofline"] = dict({"bound": "hbm", "achieved": achieved, "peak": peak, "unit": "GB/s", "frac": achieved / peak,
                                "frac_is_a_ceiling": False, "traffic": None,
                                "note": "achieved / frac: the SURVEY 8(d) contract figure -- ALGORITHMIC bytes (68 + 52 |M| per pose) over the kernel time against the "
                                        "HBM peak; it charges a 28-byte scene record to every model point and the model to every pose, so on a cache-resident "
                                        "workload it is not bounded by 1.  The physical numbers are the flat keys next to it: needed_* (transform + score + one "
                                        "28-byte record per model point that has a neighbour; needed_frac <= 1, recomputable from the kernel's average duration), "
                                        "memory_side_* (FETCH_SIZE x2 + WRITE_SIZE of this run: the L2's memory-side requests, Infinity-Cache hits included), "
                                        "l2_to_l1_*, the unit utilisations and binding_unit / binding_frac = the busiest unit.  `bound` names that unit once the "
                                        "counters are in (else the contract's \"hbm\"); c5_* is the same record for the one workload whose lists leave the caches",
                                "kernel": "lcp_coopq_kernel behind stocs_score_transforms_device (kernel_ms includes the ~50 us candidate ordering in front of it where the library orders: scenes with >= 12 MB of lists, i.e. C5, not Cm)"},
                               **krec)

    # what the collective saw: every rank reports itself through the same backend (evidence that RCCL ran with N ranks)
    me = {"rank": rank, "local_rank": local_rank, "device": torch.cuda.get_device_name(local_rank), "candidates_per_step": int(kcand),
          "seconds": dt_local}
    ranks = [me]
    if world > 1:
        ranks = [None] * world
        dist.all_gather_object(ranks, me)
    out["distributed"] = {"world_size": world, "backend": (dist.get_backend() if world > 1 else None), "ranks": ranks,
                          "collective_per_step": "all_reduce(int64 MAX) of the packed (score, candidate id) key, 8 bytes" if world > 1 else None}

    if args.full and rank == 0 and world == 1 and not args.no_pipeline and est.nM <= 8192:
        out["pipeline"] = pipeline_report(model, scene, local_rank)
        if args.workload == "Cm":
            # the same sizes with a model WITHOUT symmetry: the metric model is an ellipsoid of revolution with one bump, on
            # which a rotation about the axis is barely observable; on this one the rotation error of a winner means something
            am, asc, _ = synth.workload("Cm_asym")
            out["pipeline_asymmetric_model"] = pipeline_report(am, asc, local_rank, n_runs=5, batch_trials=16)
            out["pipeline_asymmetric_model"]["model"] = "tri-axial ellipsoid (0.08, 0.055, 0.03) m + two bumps off every symmetry plane, 5 000 points (synth.make_model_asym)"
    # Counters of THIS run: the same command is re-run under rocprofv3 (child processes, one --pmc pass per counter group,
    # a few steps each) and the LCP kernel's per-launch means come back: memory-side traffic as the guide prescribes (FETCH_SIZE x2 +
    # WRITE_SIZE on gfx950) and the utilisation of the units that can actually bound a cache-resident kernel.
    if run_pmc:
        add_counters(krec, knest, args.workload, args.candidates, groups)
        out["roofline"].update(krec)
        out["roofline"]["traffic"] = krec["memory_side_bytes_per_launch"]
        # `bound` keeps the contract's vocabulary ("hbm" | "mfma": this path is byte work, never MFMA); the unit the counters
        # show busiest is `binding_unit` / `binding_frac` next to it
        out["roofline"]["binding"] = knest["binding"]
        out["roofline"]["pmc"] = knest["pmc"]
    # the same record on C5 (the configuration where the memory side IS the bound): flat c5_* keys in the same object
    if args.full and rank == 0 and world == 1 and not args.no_c5 and args.workload == "Cm":
        try:
            c5rec, c5nest = c5_leg(local_rank, run_pmc, groups or ["fetch", "write", "mem"])
            out["roofline"].update(c5rec)
            out["roofline"]["c5_binding"] = c5nest["binding"]
            out["roofline"]["c5_pmc"] = c5nest["pmc"]
        except Exception as e:   # the Cm line must not depend on the second workload
            out["roofline"]["c5_error"] = repr(e)

    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        # CPU baseline: the oracle (single-threaded restatement of the reference's kd-tree LCP) on a
        # bounded sample of the SAME candidate batch.  Reported, never the target.
        from oracle import pyoracle
        pyoracle.build()
        orc = pyoracle.Oracle(scene.pos, scene.nrm, scene.prob, scene.pixel, model.pos, model.nrm, build_index=False)
        n0 = 32
        t = time.perf_counter()
        ref0 = orc.lcp_batch(T[:n0])
        per = (time.perf_counter() - t) / n0
        ns = int(max(n0, min(kcand, args.cpu_seconds / max(per, 1e-9))))
        t = time.perf_counter()
        ref = orc.lcp_batch(T[:ns])
        cpu_dt = time.perf_counter() - t
        err = float(np.abs(ref - lcp[:ns]).max())
        out["cpu_baseline"] = {"value": ns / cpu_dt, "unit": "poses/s", "cores": 1, "kind": "port",
                               "sample": "first %d of the %d candidates of rank 0's batch, oracle kd-tree LCP "
                                         "(oracle/stocs_oracle.cpp), %.1f s" % (ns, kcand, cpu_dt),
                               "max_abs_lcp_diff_vs_gpu": err,
                               "host_cpus": os.cpu_count()}
        # all host cores (OpenMP over candidates, one kd-tree stack per thread) over the WHOLE batch: the generous baseline,
        # and the oracle comparison of every candidate the GPU scored in the timed steps
        try:
            ncore = len(os.sched_getaffinity(0))
        except AttributeError:
            ncore = os.cpu_count() or 1
        # The cores this process may actually use: its cgroup's CPU quota, when there is one (the GPU boxes show 256 CPUs and
        # grant 16 -- cpu.max "1600000 100000"; more runnable threads than that get the whole process frozen for the rest of each
        # 100 ms period, profiles/r03_stall_root_cause.json; rounds 1-2 quoted "64 / 128 threads" that ran on 16 CPUs' worth of time)
        host_cpus = ncore
        quota_cpus = None
        try:
            q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
            if q != "max":
                quota_cpus = float(q) / float(per)
        except Exception:
            try:
                q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    quota_cpus = q / per
            except Exception:
                pass
        # without a quota: one thread per physical core (the kd-tree walk is latency bound and SMT siblings slow it down)
        ncore = max(1, min(ncore // 2 if ncore >= 64 else ncore, 128))
        if quota_cpus is not None:
            ncore = max(1, min(ncore, int(quota_cpus)))
        t = time.perf_counter()
        ref_all, exact_all = orc.lcp_batch_exact(T, nthreads=ncore)   # the reference's running float sum, and the same matches summed in double
        all_dt = time.perf_counter() - t
        diff = np.abs(ref_all - lcp)
        diff_exact = np.abs(lcp.astype(np.float64) - exact_all)
        out["cpu_baseline_all_cores"] = {"value": kcand / all_dt, "unit": "poses/s", "cores": ncore, "kind": "port",
                                         "host_cpus_available": host_cpus, "cgroup_cpu_quota": quota_cpus,
                                         "sample": "all %d candidates of rank 0's batch, OpenMP over candidates, %.1f s" % (kcand, all_dt),
                                         "max_abs_lcp_diff_vs_gpu": float(diff.max()), "candidates_compared": int(kcand),
                                         "argmax_oracle": int(np.argmax(ref_all)), "argmax_gpu": int(np.argmax(lcp)),
                                         "mean_abs_lcp_diff_vs_gpu": float(diff.mean())}
        # candidates beyond 1e-5: explained only by exact-distance ties of the nearest-neighbour query (Q11: the kd-tree's
        # visiting order decides those in the reference; one flipped point moves a score by weight / |M|)
        over = np.nonzero(diff > 1e-5)[0]
        ties_only = True
        spos = orc.scene_centred().astype(np.float64)
        for cnd in over[:16]:
            hg, cg = est.lcp_detail(T[cnd])
            ho, co = orc.lcp_detail(T[cnd])
            Tm = T[cnd].reshape(4, 4).T.astype(np.float64)
            mp = (model.pos.astype(np.float64) - cm)
            for i in np.nonzero(hg != ho)[0]:
                if hg[i] < 0 or ho[i] < 0:
                    ties_only = False
                    continue
                q = Tm[:3, :3] @ mp[i] + Tm[:3, 3]
                if abs(np.linalg.norm(q - spos[hg[i]]) - np.linalg.norm(q - spos[ho[i]])) > 1e-7:
                    ties_only = False
            same = hg == ho
            if not np.array_equal(cg[same], co[same]):
                ties_only = False
        out["oracle_check"] = {"candidates_compared": int(kcand), "max_abs_lcp_diff_vs_gpu": float(diff.max()), "tolerance": 1e-5,
                               "candidates_over_tolerance": int(len(over)),
                               "over_tolerance_explained_by_exact_distance_ties_only": bool(ties_only) if len(over) else None,
                               "within_tolerance": bool(diff.max() <= 1e-5 or ties_only),
                               "max_abs_diff_vs_exact_double_sum_of_the_same_matches": float(diff_exact.max()),
                               "oracle_float_sum_vs_its_own_exact_sum": float(np.abs(ref_all - exact_all).max()),
                               "note": "the GPU adds the weights as integers and returns the exact mean; the reference's running float sum drifts "
                                       "from the exact mean by the last figure; a flipped exact-distance tie (Q11) moves a score by weight / |M|"}
        if not args.no_cpu_pipeline and not args.no_pipeline and est.nM <= 8192:
            try:
                out["cpu_baseline_pipeline"] = cpu_pipeline_baseline(model, scene, local_rank, ncore)
            except Exception as e:   # the contract line must not depend on it
                out["cpu_baseline_pipeline"] = {"error": repr(e)}
    est.dev_free(dT)
    est.dev_free(dL)
    if rank == 0:
        # the full record goes to a file; stdout carries ONE small contract line, last
        paths = [args.details] if args.details else [os.path.join(ROOT, "bench_details.json")]
        if not args.details and os.path.isdir(os.path.join(ROOT, "gpurun_out")):
            paths.append(os.path.join(ROOT, "gpurun_out", "bench_details.json"))
        written = None
        for pth in paths:
            try:
                with open(pth, "w") as f:
                    json.dump(out, f)
                written = written or os.path.relpath(pth, ROOT)
            except Exception:
                pass
        out["details_file"] = written
        line = json.dumps(compact_line(out))
        assert len(line) < COMPACT_LIMIT, len(line)
        print(line, flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
