"""The robust refinement's candidate rule, select and kept sums at their edges (csrc/refine_robust.h through stocs_refine_robust_detail
and stocs_refine_poses_robust): oracle/refine_oracle.py's families at several keep ratios, the built cut cases of
tests/refine_robust_cases.py (every rank word known bit for bit) and the normal gate at equality and against float64.

The kept set is always compared with the k smallest of the kernel's OWN (rank word, position) by an integer sort on the host."""
import os
import sys

import numpy as np
import pytest

from oracle import refine_oracle as ro

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import refine_robust_cases as rc  # noqa: E402
import refine_robust_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
NOT = rr.NOT_CANDIDATE
RO_CASES = [c for c in ro.all_cases() if c.family in ("lattice_ties", "duplicates", "n_src") or c.family.startswith("random_")]
CUT_CASES = rc.cut_cases()


def _ids(cs):
    return [c.id for c in cs]


def _est(case):
    from model_matching_amd import capi
    from model_matching_amd.estimator import StocsEstimator
    prm = capi.default_params()
    prm.distance_threshold = 0.005 * case.unit
    sp, sn, spr, spx, mp, mn = case.estimator_inputs()
    return StocsEstimator(sp, sn, spr, spx, mp, mn, params=prm, build_index=False)


def _prm(dist, keep=1.0, min_cos=-2.0, iters=1):
    from model_matching_amd import capi
    return capi.RefineRobustParams(iters, dist, keep, min_cos)


def _held(case, est):
    sc, mc, src = case.held()
    assert np.array_equal(est.get_scene()[0].view(np.uint32), sc.view(np.uint32))
    return sc, mc, src


def _bits(v):
    return np.asarray(v, F).view(np.uint32)


def _check_common(case, d, src, mc, grid, cl, keep):
    """what holds for every detail result: flags, counts, and the kept set by integer sort of the kernel's own words"""
    n = len(src)
    assert len(d["match"]) == n
    assert np.array_equal(d["candidate"], (d["rank"] != NOT).astype(np.uint8))
    assert d["n_cand"] == int(d["candidate"].sum())
    assert d["k"] == rr.keep_count(rr.device_ratio(keep), d["n_cand"])
    kept, k, n_cand = rr.kept_by_sort(d["rank"], rr.device_ratio(keep))
    assert np.array_equal(d["kept"], kept), np.nonzero(d["kept"] != kept)[0][:8]
    assert int(d["kept"].sum()) == d["k"] and d["sums28"][27] == d["k"]
    if n:
        bad = ro.check_detail(src, mc, case.dist, grid, d["match"], d["candidate"], case.exact, cl)
        assert not bad, (len(bad), bad[:8])


def _check_sums(case, d, src, mc, nrm):
    want, bound = ro.exact_sums(src, mc, nrm, d["match"], d["kept"])
    err = np.abs(d["sums28"] - want)
    assert want[27] == d["k"]
    assert (err[:27] <= bound[:27]).all(), (err[:27] / np.maximum(bound[:27], 1e-300)).max()


def _check_pose(case, est, d, src, mc, nrm, keep, min_cos=-2.0):
    """the shipping path against the detail path: counts, freeze at k < 6, and -- on the families whose systems are regular -- the
    one-iteration pose from the kept pairs.  Kept pairs that repeat one lattice point give a system the longdouble reference itself
    cannot solve (cond 2^-50 > 1e-3 or not finite): no pose to compare there; test_five_kept_freeze_six_update pins k = 6 on a
    regular system."""
    To, Po, lcp, nc, ncand, it = est.refine_poses_robust(case.T16[None, :], src_idx=case.src_idx, params=_prm(case.dist, keep, min_cos, 1))
    assert nc[0] == d["k"] and ncand[0] == d["n_cand"], (nc, ncand, d["k"], d["n_cand"])
    if d["k"] < 6:
        assert it[0] == 0 and np.array_equal(To[0].view(np.uint32), case.T16.view(np.uint32))
        return
    if case.family not in ro.POSE_FAMILIES:
        return
    Tl, cond = ro.one_iteration(case.T16, src, mc, nrm, d["match"], d["kept"], np.longdouble)
    if not np.isfinite(cond) or cond * 2.0 ** -50 > 1e-3:
        return   # no bound that says anything (the freeze and the counts above still hold)
    tol = ro.pose_tolerance(Tl, cond)
    G = np.asarray(To[0], F).reshape(4, 4).T.astype(np.float64)
    dev = np.abs(G[:3, :] - Tl.astype(np.float64)[:3, :])
    print("POSE %s keep %.4f k %d cond %.3g max dev/tol %.3g" % (case.id, keep, d["k"], cond, (dev / tol).max()))
    assert it[0] == 1 and (dev <= tol).all(), ((dev / tol).max(), cond)


@pytest.mark.parametrize("case", RO_CASES, ids=_ids(RO_CASES))
def test_select_bit_for_bit_on_the_oracle_families(case):
    est = _est(case)
    sc, mc, src = _held(case, est)
    grid = ro.predict_grid(mc, case.dist)
    cl = ro.classify(src, mc) if len(src) else None
    nrm = case.unit_normals()
    d1 = est.refine_robust_detail(case.T16, src_idx=case.src_idx, params=_prm(case.dist, 1.0))
    n_cand = d1["n_cand"]
    # the plain form's own first evaluation: same matches, candidates = counted
    pm, pc, ps = est.refine_detail(case.T16, case.dist, src_idx=case.src_idx)
    assert np.array_equal(pm, d1["match"]) and np.array_equal(pc, d1["candidate"])
    assert np.array_equal(ps.view(np.uint64), d1["sums28"].view(np.uint64))   # everything kept, the plain order: bitwise
    # the rank word against the float64 squared distance of its pair
    ci = np.nonzero(d1["candidate"])[0]
    if len(ci):
        d2 = ro.dist2(src[ci], mc, d1["match"][ci])
        w = d1["rank"][ci].view(F).astype(np.float64)
        if case.exact:
            assert np.array_equal(d1["rank"][ci], _bits(d2.astype(F)))
        else:
            assert (np.abs(w - d2) <= d2 * 2.0 ** -22).all(), (np.abs(w - d2) / np.maximum(d2, 1e-300)).max()
    keeps = [1.0, 0.75, 0.5] + [rr.ratio_for_k(k, n_cand) for k in (6, 5) if 1 <= k <= n_cand]
    for keep in keeps:
        d = d1 if keep == 1.0 else est.refine_robust_detail(case.T16, src_idx=case.src_idx, params=_prm(case.dist, keep))
        assert np.array_equal(d["rank"], d1["rank"]) and np.array_equal(d["match"], d1["match"])
        _check_common(case, d, src, mc, grid, cl, keep)
        _check_sums(case, d, src, mc, nrm)
        _check_pose(case, est, d, src, mc, nrm, keep)
    if n_cand >= 6:
        assert est.refine_robust_detail(case.T16, src_idx=case.src_idx, params=_prm(case.dist, rr.ratio_for_k(6, n_cand)))["k"] == 6
    est.close()


@pytest.mark.parametrize("case", CUT_CASES, ids=_ids(CUT_CASES))
def test_built_cut_cases(case):
    est = _est(case)
    sc, mc, src = _held(case, est)
    assert np.array_equal(est.get_scene_centroid(), np.zeros(3, F)) and np.array_equal(est.get_model_centroid(), np.zeros(3, F))
    grid = ro.predict_grid(mc, case.dist)
    cl = ro.classify(src, mc)
    nrm = case.unit_normals()
    words = case.source_words()
    n_cand = int((words != NOT).sum())
    ks = rc.ks_for(case)
    keeps = [rr.ratio_for_k(k, n_cand) for k in ks] if ks else [1.0, 0.5]
    seen = set()
    for keep in keeps:
        d = est.refine_robust_detail(case.T16, src_idx=case.src_idx, params=_prm(case.dist, keep))
        assert np.array_equal(d["rank"], words), np.nonzero(d["rank"] != words)[0][:8]   # bit for bit, by construction
        assert d["n_cand"] == n_cand
        _check_common(case, d, src, mc, grid, cl, keep)
        _check_sums(case, d, src, mc, nrm)
        _check_pose(case, est, d, src, mc, nrm, keep)
        seen.add(d["k"])
        if hasattr(case, "twice") and case.twice[0] < d["k"] <= case.twice[1]:
            a, b = case.twice   # one level: the first k positions are kept, so the earlier naming of the point is in, the later one out
            assert d["kept"][a] == 1 and d["kept"][b] == 0 and d["rank"][a] == d["rank"][b]
    assert seen == (set(ks) if ks else {0})
    if n_cand == 0:
        assert not d["kept"].any() and not d["sums28"].any()
    est.close()


def test_five_kept_freeze_six_update():
    """eight distinct candidates off the lattice points (a residual to correct): trimmed to five the hypothesis freezes, to six it updates"""
    case = next(c for c in RO_CASES if c.family == "lattice_ties")
    est = _est(case)
    sc, mc, src = _held(case, est)
    nrm = case.unit_normals()
    m, counted, _ = est.refine_detail(case.T16, case.dist)
    off = [i for i in np.nonzero(counted)[0] if ro.dist2(src[i:i + 1], mc, m[i:i + 1])[0] > 0]
    idx8 = np.array(off[:8], np.int32)[::-1].copy()
    for k, updates in ((5, False), (6, True)):
        keep = rr.ratio_for_k(k, 8)
        d = est.refine_robust_detail(case.T16, src_idx=idx8, params=_prm(case.dist, keep))
        assert d["n_cand"] == 8 and d["k"] == k
        To, Po, lcp, nc, ncand, it = est.refine_poses_robust(case.T16[None, :], src_idx=idx8, params=_prm(case.dist, keep, -2.0, 5 if not updates else 1))
        assert nc[0] == k and ncand[0] == 8
        if not updates:
            assert it[0] == 0 and np.array_equal(To[0].view(np.uint32), case.T16.view(np.uint32))
            continue
        Tl, cond = ro.one_iteration(case.T16, src[idx8], mc, nrm, d["match"], d["kept"], np.longdouble)
        G = np.asarray(To[0], F).reshape(4, 4).T.astype(np.float64)
        dev = np.abs(G[:3, :] - Tl.astype(np.float64)[:3, :])
        print("POSE six_kept cond %.3g max dev %.3g" % (cond, dev.max()))
        assert it[0] == 1 and np.isfinite(cond) and (dev <= ro.pose_tolerance(Tl, cond)).all(), (dev.max(), cond)
    est.close()


@pytest.mark.parametrize("min_cos", list(rc.GATE_MIN_COS) + [-2.0])
def test_gate_at_equality(min_cos):
    """c is exactly -1, 0 or 1: the flag is pinned at >= bit for bit; below -1 the gate is off"""
    case = rc.gate_exact()
    est = _est(case)
    sc, mc, src = _held(case, est)
    ns = est.get_scene()[1]
    assert np.array_equal(ns, case.scene_nrm)                       # axis vectors stay what they are
    d = est.refine_robust_detail(case.T16, params=_prm(case.dist, 1.0, min_cos))
    near = case.words != NOT
    assert np.array_equal(d["match"][near] >= 0, np.ones(int(near.sum()), bool))
    c = rr.gate_c(rr.hyp_inverse(case.T16), np.eye(4)[:3, :], ns, case.unit_normals()[np.maximum(d["match"], 0)])
    assert set(np.unique(c[near]).tolist()) == {-1.0, 0.0, 1.0}
    want = near & ((c >= min_cos) if min_cos >= -1.0 else True)
    assert np.array_equal(d["candidate"], want.astype(np.uint8))
    assert np.array_equal(d["rank"], np.where(want, case.words, NOT).astype(np.uint32))
    assert d["n_cand"] == int(want.sum()) == d["k"] and 0 < d["n_cand"]
    if min_cos == 1.0:
        assert d["n_cand"] < int(near.sum()) // 2
    # the shipping path with keep_ratio == 1 is the fused launch: same counts
    To, Po, lcp, nc, ncand, it = est.refine_poses_robust(case.T16[None, :], params=_prm(case.dist, 1.0, min_cos, 1))
    assert nc[0] == ncand[0] == d["n_cand"]
    est.close()


def test_gate_against_float64_on_a_random_cloud():
    case = rc.gate_random()
    est = _est(case)
    sc, mc, src = _held(case, est)
    ns = est.get_scene()[1]
    assert np.array_equal(ns.view(np.uint32), rr.unit_normals(case.scene_nrm).view(np.uint32))
    mcos = rr.min_cos_of_degrees(30.0)
    off = est.refine_robust_detail(case.T16, params=_prm(case.dist, 1.0, -2.0))
    on = est.refine_robust_detail(case.T16, params=_prm(case.dist, 1.0, mcos))
    assert np.array_equal(off["match"], on["match"])
    near = off["candidate"] != 0
    c = rr.gate_c(rr.hyp_inverse(case.T16), np.eye(4)[:3, :], ns, case.unit_normals()[np.maximum(on["match"], 0)])
    want = near & (c >= mcos)
    differ = want != (on["candidate"] != 0)
    band = near & (np.abs(c - mcos) <= rr.GATE_BAND)
    print("GATE near %d pass %d band %d differ %d" % (near.sum(), want.sum(), band.sum(), differ.sum()))
    assert not (differ & ~band).any()
    assert band.sum() <= 0.01 * near.sum() and 0 < want.sum() < 0.5 * near.sum()
    # trimmed as well: the kept set of the gated candidates
    d = est.refine_robust_detail(case.T16, params=_prm(case.dist, 0.7, mcos))
    kept, k, n_cand = rr.kept_by_sort(d["rank"], rr.device_ratio(0.7))
    assert np.array_equal(d["kept"], kept) and d["k"] == k and d["n_cand"] == n_cand == on["n_cand"]
    _check_sums(case, d, src, mc, case.unit_normals())
    est.close()
