"""The device pose clustering (trial_cluster_kernel, csrc/cluster.hip) at its edges, through its own entry point
stocs_cluster_trials_device on the cases of oracle/cluster_oracle.py.

The contract: per trial, index list and count equal stocs_cluster_poses (host function, the kernel's float twin) bit for bit, on every
case; on the cases whose every pair decision is clear or exact they equal the float64 reference too.  The reported survivor count of
the first pass says which of the kernel's paths the later rounds took (at most 2048: the list in LDS; above: the flags in global
memory)."""
import ctypes as C

import numpy as np
import pytest

from oracle import cluster_oracle as co

pytestmark = pytest.mark.gpu
_CTX = {}


def _est():
    """one context for the module, on the tiny workload (scene and model play no part in the clustering)"""
    if "est" not in _CTX:
        from model_matching_amd import synth
        from model_matching_amd.estimator import StocsEstimator
        m, s, _ = synth.workload("tiny")
        _CTX["est"] = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    return _CTX["est"]


def _run(c):
    return _est().cluster_trials_device(c.poses, c.lcp, c.off, c.best, c.fraction, c.count, c.min_distance, c.min_angle, c.sym)


def _host(c, t):
    from model_matching_amd.estimator import cluster_poses
    key = (c.name, t)
    if key not in _CTX:
        P, l = c.trial(t)
        _CTX[key] = cluster_poses(P, l, c.fraction, float(c.best[t]), c.count, c.min_distance, c.min_angle, np.asarray(c.sym, np.float32))
    return _CTX[key]


def _check(c):
    """every property of one case; -> the per-trial lists and the survivor counts"""
    est = _est()
    off, cnt, idx, surv = _run(c)
    a0 = est.L.stocs_device_alloc_count()
    off2, cnt2, idx2, surv2 = _run(c)
    assert est.L.stocs_device_alloc_count() == a0, c.name                   # the second call allocates nothing
    for a, b in ((off, off2), (cnt, cnt2), (idx, idx2), (surv, surv2)):
        assert a.tobytes() == b.tobytes(), c.name                           # and gives the same bytes
    kept, ref_surv, classes, _ = co.reference(c)
    n = np.diff(c.off)
    assert off[0] == 0 and np.array_equal(np.diff(off), np.minimum(c.count + 1, n)), c.name
    lists = []
    for t in range(c.n_trials):
        key = (c.name, t)
        slots = idx[off[t]:off[t + 1]]
        assert 0 <= cnt[t] <= len(slots), key
        assert (slots[cnt[t]:] == -1).all(), key                            # the unused slots keep their fill
        got = slots[:cnt[t]]
        assert got.tolist() == _host(c, t).tolist(), key                    # bit for bit the host function
        if not classes[co.AMBIGUOUS]:
            assert got.tolist() == kept[t].tolist(), key                    # and the float64 reference
        if n[t] == 0:
            assert cnt[t] == 0 and surv[t] == 0, key
        assert surv[t] == ref_surv[t], key
        lists.append(got.tolist())
    return lists, surv


@pytest.mark.parametrize("family", [f for f in co.FAMILIES if f not in ("lds", "batch")])
def test_family(family):
    kept_total = 0
    for c in co.cases(family):
        lists, surv = _check(c)
        assert (surv <= co.LDS_SURVIVORS).all()
        kept_total += sum(len(x) for x in lists)
    assert kept_total > 0


def test_lds_boundary_takes_both_paths():
    seen = set()
    for c in co.cases("lds"):
        _, surv = _check(c)
        assert surv[0] == c.note["survivors"], c.name
        seen.add(int(surv[0]))
    assert seen == {co.LDS_SURVIVORS - 1, co.LDS_SURVIVORS, co.LDS_SURVIVORS + 1}     # <= 2048: the LDS list; 2049: the flags


def test_batch_and_its_reverse():
    f, r = co.cases("batch")
    lf, sf = _check(f)
    lr, sr = _check(r)
    assert (sf > co.LDS_SURVIVORS).any() and ((sf > 0) & (sf <= co.LDS_SURVIVORS)).any() and (sf == 0).any()     # both paths and empty trials in one launch
    assert lf == lr[::-1] and sf.tolist() == sr.tolist()[::-1]             # a trial's list does not depend on its place in the batch
    assert lf[0] == [] and lf[3] == [] and lf[1] == [0]


def test_the_pipeline_runs_this_kernel():
    """one batch with post-processing on the tiny workload: its own candidates through the entry point give its hypotheses"""
    from model_matching_amd.estimator import trial_post
    est = _est()
    n_trials = 8
    post = trial_post(acceptable_fraction=0.5, maximum_pose_count=10, min_distance=0.02, min_angle=15.0, sym3=(0, 0, 180), refine_iterations=0,
                      max_correspondence_distance=0.035)
    res = est.run_trials(list(range(100, 100 + n_trials)), 40, mode=0, max_per_base=50, keep_details=True, post=post)
    Ps, ls, hyp = [], [], []
    for t in range(n_trials):
        _, P, l, _ = est.trial_candidates(t)
        Ps.append(np.asarray(P, np.float32).reshape(-1, 16)); ls.append(np.asarray(l, np.float32))
        hyp.append(est.trials_get_hypotheses(t)["candidate_index"].tolist())
    off = np.concatenate([[0], np.cumsum([len(l) for l in ls])]).astype(np.int32)
    best = np.asarray([res[t]["best_lcp"] for t in range(n_trials)], np.float32)
    o, cnt, idx, _ = est.cluster_trials_device(np.concatenate(Ps), np.concatenate(ls), off, best, 0.5, 10, 0.02, 15.0, (0, 0, 180))
    assert sum(len(h) for h in hyp) > 0
    for t in range(n_trials):
        assert idx[o[t]:o[t] + cnt[t]].tolist() == hyp[t], t


def test_errors():
    from model_matching_amd import capi
    est = _est()
    L = est.L
    P = np.stack(co._far_line(3)).astype(np.float32); l = np.asarray([0.5, 0.4375, 0.375], np.float32)    # all above 0.5 * best, 0.5 apart
    off = np.asarray([0, 3], np.int32); best = np.asarray([0.5], np.float32); sym = np.zeros(3, np.float32)
    o_off = np.zeros(2, np.int32); o_cnt = np.zeros(1, np.int32); o_idx = np.zeros(3, np.int32)
    fp, ip = capi._fp, capi._ip

    def call(P=P, l=l, off=off, best=best, nT=1, fraction=0.5, count=2, min_d=0.02, min_a=15.0, sym=sym, o_off=o_off, o_cnt=o_cnt, o_idx=o_idx, cap=3, h=est.h):
        p = lambda a, ty: None if a is None else a.ctypes.data_as(ty)
        return L.stocs_cluster_trials_device(h, p(P, fp), p(l, fp), p(off, ip), p(best, fp), nT, fraction, count, min_d, min_a, p(sym, fp), p(o_off, ip),
                                             p(o_cnt, ip), p(o_idx, ip), cap, None)

    assert call() == capi.STOCS_OK and o_cnt[0] == 3 and o_idx.tolist() == [0, 1, 2]
    assert call(nT=0) == capi.STOCS_OK
    bad = [dict(l=np.asarray([0.5, -0.25, 0.125], np.float32)), dict(l=np.asarray([0.5, -0.0, 0.125], np.float32)), dict(fraction=float("nan")),
           dict(min_d=0.0), dict(min_d=float("inf")), dict(min_d=float("nan")), dict(min_a=-1.0), dict(min_a=float("inf")), dict(count=-1),
           dict(off=np.asarray([0, 3, 2], np.int32), nT=2, best=np.asarray([0.5, 0.5], np.float32), o_off=np.zeros(3, np.int32), o_cnt=np.zeros(2, np.int32)),
           dict(off=np.asarray([1, 3], np.int32)), dict(nT=-1), dict(P=None), dict(l=None), dict(off=None), dict(best=None), dict(sym=None),
           dict(o_off=None), dict(o_cnt=None), dict(o_idx=None), dict(h=None)]
    for kw in bad:
        assert call(**kw) == capi.ERR_INVALID, kw
        assert len(L.stocs_last_error()) > 0, kw
    assert call(cap=2) == capi.ERR_CAPACITY
    assert call() == capi.STOCS_OK                                          # the context is none the worse for it
