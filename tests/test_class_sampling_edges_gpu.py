"""Class-mode base sampling (sample.hip; reference sample_class_base, src/stocs.cpp:363-519) in every kernel form at the scene sizes where
the form, or the trip count of one of its chunked loops, changes -- each against the CPU oracle, bit for bit: `valid`, the four ids and the
two invariants of Oracle.sample_class_base(seed, attempt), failed attempts by their valid == 0.  Every test first asserts through
stocs_last_sampling_form that the call ran the form it is named for, with the threads, LDS bytes and list capacity the header documents
(tests/class_sampling_cases.py restates that rule; tests/test_class_sampling_cases_cpu.py checks the cases with the oracle alone)."""
import ctypes as C

import numpy as np
import pytest

import class_sampling_cases as cs

pytestmark = pytest.mark.gpu

_ORACLES, _RESULTS, _ESTS = {}, {}, {}


def _estimator(pos, nrm, prob, pix):
    from model_matching_amd.estimator import StocsEstimator
    m = cs.model()
    return StocsEstimator(pos, nrm, prob, pix, m.pos, m.nrm, build_index=True)


def _oracle(oracle_lib, key, pos, nrm, prob, pix):
    """one oracle object per (scene, prior), and one result per (oracle, seed, attempt), for the whole module"""
    if key not in _ORACLES:
        m = cs.model()
        _ORACLES[key] = oracle_lib.Oracle(pos, nrm, prob, pix, m.pos, m.nrm)
    return _ORACLES[key]


def _ref(oracle_lib, key, data, seed, attempt):
    k = (key, seed, attempt)
    if k not in _RESULTS:
        ok, ids, inv = _oracle(oracle_lib, key, *data).sample_class_base(seed, attempt)
        _RESULTS[k] = (ok, ids.copy(), inv.copy())
    return _RESULTS[k]


def _assert_equal_oracle(oracle_lib, key, data, seed, attempts, got, first_attempt=0, what=""):
    """got = (valid, ids, inv) of attempts first_attempt ..; -> number of valid attempts compared"""
    valid, ids, inv = got
    n_ok = 0
    for a in attempts:
        ok, oi, ov = _ref(oracle_lib, key, data, seed, a)
        j = a - first_attempt
        assert ok == bool(valid[j]), (what, a)
        if ok:
            assert np.array_equal(oi, ids[j]), (what, a, oi, ids[j])
            assert np.array_equal(ov.view(np.uint32), inv[j].view(np.uint32)), (what, a)
            n_ok += 1
    return n_ok


def _assert_form(est, want, what=""):
    got = est.last_sampling_form()
    for k, v in want.items():
        assert got[k] == v, (what, k, got, want)
    return got


def _size_est(S):
    if S not in _ESTS:
        sc = cs.scene(S)
        _ESTS[S] = _estimator(sc.pos, sc.nrm, sc.prob, sc.pixel)
    return _ESTS[S]


@pytest.fixture(scope="module", autouse=True)
def _close_estimators():
    yield
    for e in _ESTS.values():
        e.close()
    _ESTS.clear(); _ORACLES.clear(); _RESULTS.clear()


@pytest.mark.parametrize("case", cs.form_cases(), ids=[c[0] for c in cs.form_cases()])
def test_every_size_in_every_form_equals_the_oracle(oracle_lib, case, monkeypatch):
    name, S, env, n_attempts, fresh = case
    sc = cs.scene(S)
    data = (sc.pos, sc.nrm, sc.prob, sc.pixel)
    for e in env:
        monkeypatch.setenv(e, "1")
    if fresh:
        est = _estimator(*data)                                 # no prefix sums yet: at most 256 attempts take the full-size kernel
    else:
        est = _size_est(S)
        est.reset_trial()
    try:
        got = est.sample_bases(cs.SEED, n_attempts)
        want = cs.expected_form(S, env, n_attempts)
        form = _assert_form(est, want, name)
        assert form["redone"] == 0, form                         # the default list holds every attempt of these scenes
        if "lean" in name or (name.endswith("many") and cs.LEAN_MIN_S <= S <= cs.LDS_MAX_S):
            assert form["kernel"] == "lean"
        if name.endswith("few") or name.endswith("full") or S in (63, 26001):
            assert form["kernel"] != "lean"                      # the lean kernel must not be taken
        n_ok = _assert_equal_oracle(oracle_lib, ("size", S), data, cs.SEED, cs.compared_attempts(n_attempts, S), got, what=name)
        assert n_ok >= 10, (name, n_ok)
    finally:
        if fresh:
            est.close()


@pytest.mark.parametrize("S", cs.PRIOR_SIZES)
@pytest.mark.parametrize("kind", cs.PRIORS)
def test_degenerate_priors_equal_the_oracle_in_the_lean_and_the_full_kernel(oracle_lib, S, kind):
    """Zeros, ones and weights below the draw's 2^-32 resolution: non-zero as floats (the full-size kernel keeps them as survivors), zero
    for every draw.  The lean kernel (257 attempts) and the full-size one (40 attempts after a reset) against the oracle of that prior."""
    data = cs.with_prior(cs.scene(S), kind)
    est = _size_est(S)
    est.set_scene(*data)
    try:
        for n_attempts, kernel in ((257, "lean"), (40, "full_lds")):
            est.reset_trial()
            got = est.sample_bases(cs.SEED_PRIOR, n_attempts)
            _assert_form(est, cs.expected_form(S, (), n_attempts), (kind, n_attempts))
            assert est.last_sampling_form()["kernel"] == kernel
            n_ok = _assert_equal_oracle(oracle_lib, ("prior", S, kind), data, cs.SEED_PRIOR, cs.compared_attempts(n_attempts, S), got, what=(kind, n_attempts))
            if kind in cs.NO_VALID:
                assert n_ok == 0 and not got[0].any()
            else:
                assert n_ok >= 10
    finally:
        sc = cs.scene(S)
        est.set_scene(sc.pos, sc.nrm, sc.prob, sc.pixel)


@pytest.mark.parametrize("S", cs.PRIOR_SIZES)
def test_the_overflow_edge_redoes_exactly_the_attempts_beyond_the_cap(oracle_lib, S, monkeypatch):
    """n_surv == cap stays in the lean kernel, n_surv == cap + 1 (and anything beyond) is redone by the full-size kernel: the number of
    redone attempts equals the number of attempts whose pass-1 survivors, counted with the oracle, exceed the cap -- at the survivor count
    k of one attempt (not redone), at k - 2 (redone) and at 2 -- and every attempt equals the oracle each time."""
    sc = cs.scene(S)
    data = (sc.pos, sc.nrm, sc.prob, sc.pixel)
    orc = _oracle(oracle_lib, ("size", S), *data)
    first, counts = cs.survivor_counts(oracle_lib, orc, sc.prob, cs.SEED, 257)
    a, k = cs.pick_overflow_attempt(counts, cs.expected_form(S)["cap"])
    est = _size_est(S)
    redone = {}
    for cap in (k, k - 2, 2):
        monkeypatch.setenv("STOCS_CLASS_LEAN_CAP", str(cap))
        est.reset_trial()
        got = est.sample_bases(cs.SEED, 257)
        form = _assert_form(est, cs.expected_form(S, (), 257, cap_env=cap), cap)
        assert form["kernel"] == "lean" and form["cap"] == cap
        redone[cap] = form["redone"]
        print("S=%d cap=%d redone=%d of 257 (oracle: %d)" % (S, cap, form["redone"], int((counts > cap).sum())))
        assert form["redone"] == int((counts > cap).sum()), (cap, form)
        assert _assert_equal_oracle(oracle_lib, ("size", S), data, cs.SEED, range(257), got, what=cap) >= 200
    monkeypatch.delenv("STOCS_CLASS_LEAN_CAP")
    # the chosen attempt has exactly k survivors: inside the list at k, beyond it at k - 2
    assert redone[k - 2] - redone[k] == int(((counts == k) | (counts == k - 1)).sum()) >= 1
    assert redone[2] > redone[k - 2] > 0


@pytest.mark.parametrize("S", cs.POINT1_SIZES)
def test_point_1_search_equals_the_oracle_draw(oracle_lib, S):
    """The lean kernel's 64-ary wavefront search of the prior's prefix sums, on its own (stocs_debug_draw_point1): the extreme words, 200
    random ones, and the smallest word on either side of 64 prefix boundaries, for the scene's own prior and the degenerate ones."""
    L = oracle_lib.lib()
    sc = cs.scene(S)
    est = _size_est(S)
    try:
        for kind in ("own",) + cs.PRIORS:
            data = cs.with_prior(sc, kind)
            prob = data[2]
            est.set_scene(*data)
            words = cs.point1_words(prob)
            got = est.debug_draw_point1(words)
            pw = prob.ctypes.data_as(C.POINTER(C.c_float))
            want = np.array([L.orc_draw(pw, S, r) for r in words], np.int32)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (kind, [(hex(words[i]), int(got[i]), int(want[i])) for i in bad[:5]])
            if kind in cs.ZERO_TOTAL:
                assert (got == -1).all()
            else:
                n_nonzero = sum(1 for v in cs.fixed_weights(prob) if v)
                assert (got >= 0).all() and len(words) > 205 and len(set(got.tolist())) >= min(50, n_nonzero)
    finally:
        est.set_scene(sc.pos, sc.nrm, sc.prob, sc.pixel)


def test_point_1_entry_refuses_scenes_the_lean_kernel_does_not_take():
    from model_matching_amd import capi
    for S in (63,):
        with pytest.raises(capi.StocsError) as e:
            _size_est(S).debug_draw_point1([0, 1])
        assert e.value.code == capi.ERR_INVALID and "64 to 32768" in str(e.value)


def test_the_prior_cache_follows_the_prior(oracle_lib):
    """The prefix sums the lean kernel draws point 1 from are cached per context (cdf_epoch / cdf_n): a stocs_ctx_set_scene that keeps the
    point count and the positions and changes the prior, a stocs_reset_trial, and a scene of another size and back must each leave the
    lean kernel (257 attempts) and the full-size one (40 attempts) on the oracle of the prior in force."""
    S = 1500
    sc = cs.scene(S)
    a = cs.with_prior(sc, "object_at_end_own")
    b = cs.with_prior(sc, "object_at_end")
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[2], b[2])
    other = cs.scene(2049)
    est = _estimator(*a)
    try:
        def check(kind, data, step):
            for n_attempts, kernel in ((257, "lean"), (40, "full_lds")):
                if kernel == "full_lds":
                    est.reset_trial()                            # (prefix sums that are current would send 40 attempts to the lean kernel too)
                got = est.sample_bases(cs.SEED_PRIOR, n_attempts)
                assert est.last_sampling_form()["kernel"] == kernel, (step, kernel)
                assert _assert_equal_oracle(oracle_lib, ("prior", S, kind), data, cs.SEED_PRIOR, cs.compared_attempts(n_attempts, S), got, what=(step, kernel)) >= 10
            got = est.sample_bases(cs.SEED_PRIOR, 40)            # prefix sums current again? then lean, else full: either way the oracle's
            _assert_equal_oracle(oracle_lib, ("prior", S, kind), data, cs.SEED_PRIOR, range(40), got, what=(step, "after"))
        check("object_at_end_own", a, "created")
        for step in ("set_scene", "reset_trial"):
            est.set_scene(*b)
            check("object_at_end", b, step + " b")
            if step == "reset_trial":
                est.reset_trial()
                check("object_at_end", b, "reset b")
            est.set_scene(*a)
            check("object_at_end_own", a, step + " a")
        est.set_scene(other.pos, other.nrm, other.prob, other.pixel)
        got = est.sample_bases(cs.SEED, 257)
        assert est.last_sampling_form()["kernel"] == "lean"
        _assert_equal_oracle(oracle_lib, ("size", 2049), (other.pos, other.nrm, other.prob, other.pixel), cs.SEED, cs.compared_attempts(257, 2049), got, what="other size")
        est.set_scene(*b)
        check("object_at_end", b, "back")
    finally:
        est.close()


@pytest.mark.parametrize("S,n_trials,kernel,launches", [(8001, 6, "lean", 1), (26001, 52, "full_device_memory", 2)])
def test_trial_batches_equal_the_oracle(oracle_lib, S, n_trials, kernel, launches):
    """Class-mode trial batches (stocs_run_trials): the lean kernel in one launch, and the device-memory form cut into launches of at most
    1 GiB of working set (2^30 / (26001 * 8) = 5162 attempts) with wg_offset: the first trial, the last one, the one the cut falls into
    and one more (against stocs_sample_bases on a fresh context)."""
    sc = cs.scene(S)
    data = (sc.pos, sc.nrm, sc.prob, sc.pixel)
    seeds = [9100 + 13 * t for t in range(n_trials)]
    nA = 100
    est = _size_est(S)
    est.run_trials(seeds, nA, max_per_base=1, keep_details=True)
    want = cs.expected_form(S, (), n_trials * nA, batch=True)
    form = _assert_form(est, want, S)
    assert form["kernel"] == kernel and form["launches"] == launches and form["redone"] == 0
    per_launch = max(1, min(n_trials * nA, (1 << 30) // (8 * S)))
    cut = min(per_launch, n_trials * nA - 1) // nA
    further = n_trials // 2
    bases = {t: est.trial_bases(t) for t in sorted({0, n_trials - 1, cut, further})}
    for t in sorted({0, n_trials - 1, cut}):
        assert len(bases[t][0]) == nA
        assert _assert_equal_oracle(oracle_lib, ("size", S), data, seeds[t], range(nA), bases[t], what=("trial", t)) >= 50
    fresh = _estimator(*data)
    try:
        v, i, f = fresh.sample_bases(seeds[further], nA)
    finally:
        fresh.close()
    gv, gi, gf = bases[further]
    assert np.array_equal(v, gv) and np.array_equal(i[v], gi[gv]) and np.array_equal(f[v].view(np.uint32), gf[gv].view(np.uint32))
    assert int(v.sum()) >= 50
