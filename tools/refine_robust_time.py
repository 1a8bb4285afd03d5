#!/usr/bin/env python3
"""Host wall clock of the robust refinement next to the plain one (5 iterations, 3.5 cm) for 1, 10, 64 and 256 hypotheses on the ycb
example frame and on Cm, four forms in one process: stocs_refine_poses, stocs_refine_poses_robust with keep 0.7 and a 30 degree gate,
with keep 1 and the gate off (the plain form's accumulation, one launch per iteration) and with keep 1 and the 30 degree gate (the
accumulation's gate-on form, one launch per iteration).  Method as tools/refine_time.py: median of
20 after 5 warm-ups.  The yardstick is the plain call; the record holds the ratio per row.  A kernel trace of ONE call per robust form
(Cm, 64 hypotheses) is taken in child processes before this process opens the GPU.  Measurement only.
usage: python tools/refine_robust_time.py [out.json] [reps]        (--one-call WORKLOAD N FORM: the traced child)"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("STOCS_PIN_BLAS", "1")

SIZES = (1, 10, 64, 256)
FORMS = {"plain": None, "robust_0.7_30deg": (0.7, 30.0), "robust_keep1_nogate": (1.0, None), "robust_keep1_30deg": (1.0, 30.0)}


def call(est, form, h):
    if FORMS[form] is None:
        return est.refine_poses(h)
    keep, deg = FORMS[form]
    return est.refine_poses_robust(h, 5, 0.035, keep, deg)


def one_call(name, n, form):
    import refine_time
    est, mpos, mnrm, H, _ = refine_time.hypotheses(name)
    est.refine_poses(H[:n])          # the grid and the plain workspace exist; the traced kernels of the robust form run once
    call(est, form, H[:n])
    est.close()


def trace(name, n, form):
    """kernel trace of one call in a child process -> {kernel: {calls, total_ms, avg_us}} (None when the profiler is not there)"""
    import pmc_all
    with tempfile.TemporaryDirectory() as d:
        st = pmc_all.stats_pass([sys.executable, os.path.abspath(__file__), "--one-call", name, str(n), form], d, timeout=240)
    return {pmc_all.short(k): {"calls": v["calls"], "total_ms": v["total_ms"], "avg_us": v["avg_us"]} for k, v in st.items()
            if "refine" in k or "robust" in k or "lcp" in k.lower()} or None


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one-call":
        return one_call(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "refine_robust_time.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rec = {"iterations": 5, "distance": 0.035, "reps": reps, "warmups": 5, "forms": {k: v for k, v in FORMS.items()}, "workloads": {}}
    rec["kernel_trace_Cm_64"] = {form: trace("Cm", 64, form) for form in FORMS}
    import refine_time
    for name in ("ycb", "Cm"):
        est, mpos, mnrm, H, n_clustered = refine_time.hypotheses(name)
        w = {"nS": int(est.nS), "nM": int(est.nM), "rows": {}}
        for n in SIZES:
            h = H[:n]
            row = {}
            for form in FORMS:
                for _ in range(5):
                    call(est, form, h)
                t = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    call(est, form, h)
                    t.append((time.perf_counter() - t0) * 1e3)
                row[form] = {"median_ms": float(np.median(t)), "min_ms": float(np.min(t))}
            for form in FORMS:
                row[form]["ratio_to_plain"] = row[form]["median_ms"] / row["plain"]["median_ms"]
            w["rows"][str(n)] = row
            print(name, n, " ".join("%s %.3f ms (x%.2f)" % (f, row[f]["median_ms"], row[f]["ratio_to_plain"]) for f in FORMS), flush=True)
        rec["workloads"][name] = w
        est.close()
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec["workloads"]))


if __name__ == "__main__":
    main()
