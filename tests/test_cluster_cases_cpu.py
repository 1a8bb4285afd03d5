"""The clustering cases of oracle/cluster_oracle.py held to themselves and to the float twins, without a GPU: the float64 reference
equals stocs_cluster_poses (host function of the library) and the oracle's greedy_clustering on every case that is not ambiguous, each
generator produces what its name says, and the derived float32 error bound holds against the host twin's pose_diff on every pair the
cases meet."""
import os

import numpy as np
import pytest

from oracle import cluster_oracle as co


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    from model_matching_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        g.build()
    from model_matching_amd.estimator import cluster_poses
    return cluster_poses


def _args(c, t):
    return c.fraction, float(c.best[t]), c.count, c.min_distance, c.min_angle, np.asarray(c.sym, np.float32)


@pytest.mark.parametrize("family", list(co.FAMILIES))
def test_reference_equals_both_twins(family, host, oracle_lib):
    for c in co.cases(family):
        kept, _, classes, _ = co.reference(c)
        for t in range(c.n_trials):
            P, l = c.trial(t)
            a = host(P, l, *_args(c, t))
            b = oracle_lib.greedy_clustering(P, l, *_args(c, t))
            assert np.array_equal(a, b), (c.name, t)                       # the twins agree on every case, ambiguous or not
            if not classes[co.AMBIGUOUS]:
                assert np.array_equal(kept[t], a), (c.name, t, kept[t][:8], a[:8])


def test_few_cases_are_left_out():
    amb_random = 0
    for c in co.cases():
        amb = co.reference(c)[2][co.AMBIGUOUS] > 0
        if c.family == "random":
            amb_random += amb
        else:
            assert amb == c.built_ambiguous, c.name          # of the directed families only the two near-gimbal cases are ambiguous
    assert [c.name for c in co.cases() if c.built_ambiguous] == ["gimbal_near_-1e-03", "gimbal_near_+1e-03"]
    assert amb_random * 20 <= len(co.cases("random")) == 64


def test_expected_results_of_the_directed_cases():
    for c in co.cases():
        if c.built_ambiguous:
            continue
        kept = co.reference(c)[0]
        if "kept" in c.note:
            assert len(kept[0]) == c.note["kept"], c.name
        if "kept_list" in c.note:
            assert kept[0].tolist() == c.note["kept_list"], c.name


def test_size_and_survivor_counts():
    assert [int(c.off[-1]) for c in co.cases("sizes")] == [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 1280]
    seen = set()
    for c in co.cases("lds"):
        surv = co.reference(c)[1]
        assert surv == [c.note["survivors"]], c.name
        seen.add((surv[0], int(c.off[-1])))
        assert c.count <= 48 and len(co.reference(c)[0][0]) <= 48
    assert seen == {(s, n) for s in (2047, 2048, 2049) for n in (s, 4608)}
    top = [c for c in co.cases("lds") if c.name.endswith("top_last")][0]
    order = np.argsort(-top.lcp, kind="stable")[:64]
    assert order.min() >= len(top.lcp) - 64                 # the 64 best survivors are the last 64 candidates
    for c in co.cases("batch"):
        assert sorted(np.diff(c.off).tolist()) == sorted([0, 1, 300, 0, 2600, 2048, 5])
        surv = co.reference(c)[1]
        assert max(surv) > co.LDS_SURVIVORS and co.LDS_SURVIVORS in surv and 0 in surv
    f, r = co.cases("batch")
    assert np.diff(f.off).tolist() == np.diff(r.off).tolist()[::-1]


def test_ties_are_ties():
    a, b, c = co.cases("ties")
    assert len(set(a.lcp.tolist())) == 1
    assert len(set(b.lcp.tolist())) == 7 and (np.diff(b.lcp[:16]) == 0).all()
    assert c.lcp[0] < c.fraction * c.best[0] < c.lcp[1] == c.lcp[2] == c.lcp.max() and co.reference(c)[0][0][0] == 1
    assert co.reference(a)[0][0][0] == 0


def test_threshold_cases_are_exact_in_float32():
    for c in co.cases("thresholds"):
        if "distance" not in c.name:
            continue
        d = c.poses[1, 12:15].astype(np.float64) - c.poses[0, 12:15].astype(np.float64)
        assert co._exact_distance(d)
        dist = np.float32(np.sqrt((d * d).sum()))
        if "equal" in c.name:
            assert np.float32(c.min_distance) == dist
        else:
            assert np.float32(c.min_distance) == np.nextafter(dist, np.float32(1))
        assert co.reference(c)[2][co.EXACT] == 1
    c = [c for c in co.cases("thresholds") if c.name == "thr_lcp_equal_and_above"][0]
    thr = np.float32(c.fraction) * c.best[0]
    assert c.lcp[1] == thr and c.lcp[2] == np.nextafter(thr, np.float32(1)) and co.reference(c)[1] == [2]


def test_argument_order_pairs_really_differ(oracle_lib):
    for c in co.cases("order"):
        a, b = c.poses
        sym = np.zeros(3, np.float32)
        r_ab, _ = oracle_lib.pose_diff(a, b, sym)
        r_ba, _ = oracle_lib.pose_diff(b, a, sym)
        assert r_ab < c.min_angle - 0.9 and r_ba > c.min_angle + 0.9, (c.name, r_ab, r_ba)


def test_quaternion_cases_take_their_branch():
    seen = set()
    for c in co.cases("quaternion"):
        tr, i = co.diff_trace32(c.poses[1], c.poses[0])      # (test = the lower score, base = the kept one)
        assert tr <= 0 and i == c.note["branch"], (c.name, tr, i)
        if "trace" in c.note:
            assert tr == 0.0
        seen.add(i)
    assert seen == {0, 1, 2}


def test_bound_holds_against_the_host_twin(oracle_lib, capsys):
    """|float32 twin - float64| <= the derived bound on every distinct pose pair the cases meet (pairs whose rotation error is NaN or
    undefined in the reference: the twin's must be NaN, or is not looked at)."""
    worst_r = worst_t = 0.0
    n_pairs = 0
    for c in co.cases():
        sym = np.asarray(c.sym, np.float32)
        seen = set()
        for (t, i, j, te, re, bt, br, lower_only) in co.reference(c)[3]:
            P, _ = c.trial(t)
            key = (P[i].tobytes(), P[j].tobytes())
            if key in seen:
                continue
            seen.add(key)
            n_pairs += 1
            r32, t32 = oracle_lib.pose_diff(P[i], P[j], sym)
            if np.isfinite(te):
                assert abs(t32 - te) <= bt + 1e-45, (c.name, i, j, t32, te, bt)
                if bt > 0:
                    worst_t = max(worst_t, abs(t32 - te) / bt)
            else:
                assert not np.isfinite(t32)
            if not np.isfinite(re) or not np.isfinite(br):
                continue
            if lower_only:
                assert r32 >= re - br, (c.name, i, j, r32, re, br)
                continue
            assert abs(r32 - re) <= br, (c.name, i, j, r32, re, br)
            if br > 0:
                worst_r = max(worst_r, abs(r32 - re) / br)
    with capsys.disabled():
        print("\ncluster bound: %d distinct pairs, largest |twin - float64| / bound: rotation %.3f, translation %.3f" % (n_pairs, worst_r, worst_t))
    assert n_pairs > 10000


def test_nan_rule_matches_the_twin(oracle_lib):
    """where the reference applies its rule (NaN rotation error: never <), the float routine gives NaN too"""
    n = 0
    for c in co.cases("degenerate"):
        P, _ = c.trial(0)
        prep = co._Prep(P)
        for j in range(len(P)):
            ev = co.pair_eval(prep, np.arange(len(P)), j, c.min_distance, c.min_angle, c.sym)
            for i in np.flatnonzero(ev["nan_rule"]):
                r32, _ = oracle_lib.pose_diff(P[i], P[j], np.asarray(c.sym, np.float32))
                assert r32 != r32, (c.name, i, j, r32)
                n += 1
    assert n > 0
