"""Child process of the tests that need a switch the library reads ONCE per process (STOCS_SORT, STOCS_GATHER_WGS, STOCS_SORT_SHAPE,
STOCS_SORT_HIST_SUB are cached in static variables): the parent starts this script with the switch in its environment, one process per
setting, and checks what it returns.  Not a test module.

    fresh_process_child.py congruent <bases.npz>    bases (ids, inv) on the `tiny` workload -> one JSON line on stdout: total, per-base
                                                    quads, the first ranks of every base's walk order, the host steps of the call
    fresh_process_child.py sort <in.npz> <out.npz>  the library's own sort of a segmented and an unsegmented list -> sorted pairs in out.npz
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("STOCS_PIN_BLAS", "1")

import numpy as np  # noqa: E402

WALK_RANKS = 300


def congruent(path):
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    z = np.load(path)
    m, s, _ = synth.workload("tiny")
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    try:
        est.set_bases(z["ids"], z["inv"])
        total = est.find_congruent_all()
        labels = [lab for lab, _ in est.last_call_timing(0)]
        quads, walk = [], []
        for k in range(len(z["ids"])):
            q = est.get_quads(k)
            quads.append(q.reshape(-1).tolist())
            walk.append(est.get_quads_at(k, np.arange(min(len(q), WALK_RANKS))).reshape(-1).tolist())
    finally:
        est.close()
    print(json.dumps({"total": total, "labels": labels, "quads": quads, "walk": walk}))


def sort(path_in, path_out):
    from model_matching_amd import capi
    L = capi.load()
    z = np.load(path_in)
    u32p = C.POINTER(C.c_uint32)
    out = {}
    for name in ("seg", "flat"):
        k = np.ascontiguousarray(z[name + "_keys"], np.uint32)
        v = np.ascontiguousarray(z[name + "_vals"], np.uint32)
        so = np.ascontiguousarray(z[name + "_off"], np.uint32) if name + "_off" in z else None
        ko = np.zeros_like(k); vo = np.zeros_like(v)
        ms = C.c_float(0)
        capi.check(L.stocs_debug_sort_pairs(-1, k.ctypes.data_as(u32p), v.ctypes.data_as(u32p), len(k), int(z[name + "_end_bit"]), 1, 1,
                                            ko.ctypes.data_as(u32p), vo.ctypes.data_as(u32p), C.byref(ms),
                                            None if so is None else so.ctypes.data_as(u32p), 0 if so is None else len(so) - 1))
        out[name + "_keys"] = ko; out[name + "_vals"] = vo
    np.savez(path_out, **out)


if __name__ == "__main__":
    if sys.argv[1] == "congruent":
        congruent(sys.argv[2])
    elif sys.argv[1] == "sort":
        sort(sys.argv[2], sys.argv[3])
    else:
        sys.exit("unknown mode %r" % sys.argv[1])
