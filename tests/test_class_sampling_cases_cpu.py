"""The cases of tests/class_sampling_cases.py checked with the CPU oracle alone: every condition the GPU tests of
tests/test_class_sampling_edges_gpu.py rely on, so that a case cannot go vacuous unnoticed.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import class_sampling_cases as cs


def _oracle(oracle_lib, pos, nrm, prob, pix):
    m = cs.model()
    return oracle_lib.Oracle(pos, nrm, prob, pix, m.pos, m.nrm)


@pytest.mark.parametrize("S", cs.SIZES)
def test_every_size_has_its_point_count_and_enough_valid_attempts(oracle_lib, S):
    sc = cs.scene(S)
    assert len(sc.pos) == len(sc.nrm) == len(sc.prob) == S
    orc = _oracle(oracle_lib, sc.pos, sc.nrm, sc.prob, sc.pixel)
    for n_attempts in (cs.n_attempts_few(S), cs.n_attempts_many(S)):
        att = cs.compared_attempts(n_attempts, S)
        assert att[0] == 0 and att[-1] == n_attempts - 1
        n_valid = sum(orc.sample_class_base(cs.SEED, a)[0] for a in att)
        print("S=%d attempts=%d compared=%d valid=%d" % (S, n_attempts, len(att), n_valid))
        assert n_valid >= 10, (S, n_attempts, n_valid)
    # no attempt of the "many" call outgrows the smallest list its size gets: the GPU test asserts that nothing is redone
    cap = cs.expected_form(S)["cap"]
    if cap:
        _, counts = cs.survivor_counts(oracle_lib, orc, sc.prob, cs.SEED, cs.n_attempts_many(S))
        assert counts.max() <= cap, (S, int(counts.max()), cap)


@pytest.mark.parametrize("S", cs.PRIOR_SIZES)
@pytest.mark.parametrize("kind", cs.PRIORS)
def test_degenerate_priors_validate_what_the_gpu_tests_expect(oracle_lib, S, kind):
    sc = cs.scene(S)
    assert sc.n_object == 185 and len(sc.pos) == S
    pos, nrm, prob, pix = cs.with_prior(sc, kind)
    assert len(prob) == S and prob.dtype == np.float32
    W = cs.fixed_weights(prob)
    assert (sum(W) == 0) == (kind in cs.ZERO_TOTAL)
    if kind in ("all_below_resolution", "clutter_below_resolution"):
        assert np.count_nonzero(prob) == S and sum(1 for v in W if v) == (0 if kind == "all_below_resolution" else 185)
    if kind == "object_at_end":
        assert np.array_equal(pos[S - 185:], sc.pos[:185]) and not prob[:S - 185].any() and prob[S - 185:].all()
    orc = _oracle(oracle_lib, pos, nrm, prob, pix)
    n_valid = sum(orc.sample_class_base(cs.SEED_PRIOR, a)[0] for a in range(cs.FIRST))
    print("S=%d prior=%s valid=%d of %d" % (S, kind, n_valid, cs.FIRST))
    if kind in cs.NO_VALID:
        assert n_valid == 0
    else:
        assert n_valid >= 10


@pytest.mark.parametrize("S", cs.PRIOR_SIZES)
def test_the_overflow_edge_has_an_attempt_on_either_side_of_its_cap(oracle_lib, S):
    sc = cs.scene(S)
    orc = _oracle(oracle_lib, sc.pos, sc.nrm, sc.prob, sc.pixel)
    first, counts = cs.survivor_counts(oracle_lib, orc, sc.prob, cs.SEED, 257)
    cap = cs.expected_form(S)["cap"]
    a, k = cs.pick_overflow_attempt(counts, cap)
    print("S=%d default cap=%d attempt=%d k=%d survivors min/median/max=%d/%d/%d" % (S, cap, a, k, counts.min(), np.median(counts), counts.max()))
    assert (first >= 0).all()
    assert counts[a] == k and not counts[a] > k and counts[a] > k - 2
    for c in (k, k - 2, 2):
        n_over = int((counts > c).sum())
        assert 0 < n_over <= 257                                          # every cap of the GPU test redoes something
    assert int((counts > k).sum()) < int((counts > 2).sum())              # and the three caps do not all redo the same attempts
    assert int((counts > cap).sum()) == 0                                 # the default list holds every attempt of these scenes


@pytest.mark.parametrize("S", cs.POINT1_SIZES)
def test_point1_words_sit_on_the_prefix_boundaries(oracle_lib, S):
    L = oracle_lib.lib()
    sc = cs.scene(S)
    for kind in ("own",) + cs.PRIORS:
        prob = cs.with_prior(sc, kind)[2]
        words = cs.point1_words(prob)
        W = cs.fixed_weights(prob)
        total = sum(W)
        if kind in cs.ZERO_TOTAL:
            assert total == 0 and len(words) == 205
            assert L.orc_draw(prob.ctypes.data_as(C.POINTER(C.c_float)), S, words[7]) == -1
            continue
        assert 0 < total < 1 << 64 and all(0 <= r < 1 << 64 for r in words)
        bw = words[205:]
        assert len(bw) >= 2
        # a boundary word's draw is the first index whose prefix exceeds its target: the word below it draws an earlier or the same index
        pre = np.cumsum(np.array(W, dtype=object))
        for r in bw[:: max(1, len(bw) // 16)]:
            t = cs.mulhi64(r, total)
            want = int(np.searchsorted(np.array(pre, dtype=np.float64), float(t), side="right")) if total < 1 << 52 else None
            got = L.orc_draw(prob.ctypes.data_as(C.POINTER(C.c_float)), S, r)
            assert pre[got] > t and (got == 0 or pre[got - 1] <= t)
            if want is not None:
                assert got == want
    assert len(cs.boundary_indices(S)) == min(S, 64) and cs.boundary_indices(S)[0] == 0 and cs.boundary_indices(S)[-1] == S - 1


def test_the_form_rule_at_its_thresholds():
    f = cs.expected_form
    assert f(63)["kernel"] == "full_lds" and f(64)["kernel"] == "lean" and f(26000)["kernel"] == "lean" and f(26001)["kernel"] == "full_device_memory"
    assert [f(S)["threads"] for S in (64, 8000, 8001, 24000, 24001, 26000)] == [256, 256, 512, 512, 1024, 1024]
    assert f(8000, n_attempts=256)["kernel"] == "full_lds" and f(8000, n_attempts=40, prefix_sums_current=True)["kernel"] == "lean"
    assert f(64)["lds_bytes"] == 400 and f(64)["cap"] == 64 and f(8000)["lds_bytes"] == 16384 and f(8001)["lds_bytes"] == 36864
    assert f(26000)["lds_bytes"] == 76800 and f(26000)["cap"] == 12798
    assert f(26001, n_attempts=5200, batch=True)["launches"] == 2 and f(26001, n_attempts=5162, batch=True)["launches"] == 1
    ids = [c[0] for c in cs.form_cases()]
    assert len(ids) == len(set(ids))
