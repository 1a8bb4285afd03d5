"""Instance-mode base sampling (instance_attempts_kernel<WLDS>, sample.hip; reference sample_instance_base, src/stocs.cpp:559-751) with the
attempt's working set in LDS and in device memory, at the scene sizes, run counts and image positions where a loop takes another trip or the
kernel another form -- each against the CPU oracle, bit for bit: `valid`, the ordered base and its invariants of EVERY attempt, `segment`
and the decayed class probabilities after the last one; the scores of eight poses within the suite's 1e-5, because the LCP adds the decayed
prior.  Every case also asserts through stocs_last_sampling_form which form ran, and the per-attempt records of
stocs_last_instance_attempts prove over the whole table that every path of the mask was taken (tests/instance_sampling_cases.py holds the
table and restates the form rule; tests/test_instance_sampling_cases_cpu.py checks the cases with the oracle alone)."""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import instance_sampling_cases as ic

pytestmark = pytest.mark.gpu

LCP_TOL = 1e-5
_REF, _RUNS = {}, {}


@contextlib.contextmanager
def _env(names):
    """the STOCS_* switches of a case (read with getenv at every launch), for the duration of the block"""
    old = {k: os.environ.get(k) for k in names}
    os.environ.update({k: "1" for k in names})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _estimator(S, kind):
    """a fresh context on scene(S) under the map `kind`"""
    from model_matching_amd import capi
    from model_matching_amd.estimator import StocsEstimator
    sc, m = ic.scene(S), ic.model()
    H, W = ic.image_size(kind)
    edge, pix = ic.case_input(S, kind)
    est = StocsEstimator(sc.pos, sc.nrm, sc.prob, pix, m.pos, m.nrm, params=capi.default_params(image_height=H, image_width=W), build_index=True)
    est.set_edge_map(edge)
    return est


def _poses(est, S):
    from model_matching_amd import synth
    c_s, c_m = est.get_scene_centroid(), est.get_model_centroid()
    return synth.make_candidates(synth.centred_gt(ic.scene(S).T_gt, c_s.astype(np.float64), c_m.astype(np.float64)), ic.N_POSES)


def _run_calls(est, calls, disp):
    valid, ids, inv, recs, forms = [], [], [], [], []
    for first, n in calls:
        v, i, f = est.sample_bases(ic.SEED, n, first_attempt=first, mode=1, dispersion=disp)
        valid.append(v); ids.append(i); inv.append(f)
        forms.append(est.last_sampling_form())
        rec = est.last_instance_attempts()
        assert rec.shape == (n, 4)
        recs.append(rec)
    return dict(valid=np.concatenate(valid), ids=np.concatenate(ids), inv=np.concatenate(inv), recs=np.concatenate(recs), forms=forms,
                segment=est.get_segment().copy(), prob=est.get_scene()[2].copy())


def _gpu(case):
    """The case on the device, once for the whole module: one fresh context, the case's calls, then stocs_reset_trial and the same calls
    again -> (first run, run after the reset); the first run also holds the poses and their scores under the decayed prior."""
    name, S, kind, size, disp, calls, env = case
    if name not in _RUNS:
        with _env(env):
            est = _estimator(S, kind)
            try:
                run = _run_calls(est, calls, disp)
                run["poses"] = _poses(est, S)
                run["lcp"] = est.score_transforms(run["poses"])
                est.reset_trial()
                assert np.array_equal(est.get_scene()[2], ic.scene(S).prob.astype(np.float32)) and len(est.get_segment()) == 0
                again = _run_calls(est, calls, disp)
            finally:
                est.close()
        _RUNS[name] = (run, again)
    return _RUNS[name]


def _ref(oracle_lib, case):
    k = ic.reference_key(case)
    if k not in _REF:
        _REF[k] = ic.run_oracle(oracle_lib, case)
    return _REF[k]


def _assert_bases_equal(want, got, what):
    """valid of every attempt, ids and invariants of every valid one -> number of valid attempts"""
    assert len(want["valid"]) == len(got["valid"]), what
    assert np.array_equal(want["valid"], got["valid"]), (what, np.nonzero(want["valid"] != got["valid"])[0][:8])
    v = want["valid"]
    bad = np.nonzero((want["ids"][v] != got["ids"][v]).any(axis=1))[0]
    assert len(bad) == 0, (what, np.nonzero(v)[0][bad][:8], want["ids"][v][bad][:2], got["ids"][v][bad][:2])
    assert np.array_equal(want["inv"][v].view(np.uint32), got["inv"][v].view(np.uint32)), what
    return int(v.sum())


@pytest.fixture(scope="module", autouse=True)
def _drop_module_state():
    yield
    _REF.clear(); _RUNS.clear()


CASES = ic.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_case_equals_the_oracle(oracle_lib, case):
    name, S, kind, size, disp, calls, env = case
    run, again = _gpu(case)
    want = _ref(oracle_lib, case)
    counts = ic.path_counts(run["recs"])
    print("%s: %s valid=%d of %d paths=%s" % (name, run["forms"][-1]["kernel"], int(run["valid"].sum()), len(run["valid"]), counts))
    # the form the calls ran (stocs_last_sampling_form) is the documented one -- at 16 000 points 161 568 bytes of dynamic LDS, launched
    form = ic.expected_form(S, env)
    for got_form in run["forms"] + again["forms"]:
        assert got_form == form, (name, got_form, form)
    if S == 16000 and not env:
        assert form["kernel"] == "instance_lds" and form["lds_bytes"] == 161568
    # bases of every attempt, `segment` and the decayed prior after the last call: the oracle's, bit for bit
    assert _assert_bases_equal(want, run, name) >= 3
    assert np.array_equal(run["segment"], want["segment"]), name
    assert np.array_equal(run["prob"].view(np.uint32), want["prob"].view(np.uint32)), (name, int((run["prob"] != want["prob"]).sum()))
    # the LCP adds the decayed prior (Q8)
    assert np.array_equal(run["poses"], want["poses"])
    print("%s: largest score difference %.3g" % (name, np.abs(run["lcp"] - want["lcp"]).max()))
    assert np.abs(run["lcp"] - want["lcp"]).max() <= LCP_TOL, name
    # the records agree with the results: an attempt that failed at its first draw has no base, one that reached its mask has point 1
    for a, rec in enumerate(run["recs"]):
        path = ic.path_of(rec)
        assert (path == "failed_first_draw") == (a in want["failed_first"]), (name, a, rec)
        assert rec[0] == want["seg_sizes"][a] or path == "failed_first_draw", (name, a, rec)
        if run["valid"][a]:
            assert rec[1] in run["ids"][a] and rec[0] >= 3, (name, a, rec)
    # state carried across calls: stocs_reset_trial and the same calls give the same results
    for k in ("valid", "ids", "inv", "recs", "segment", "prob"):
        assert np.array_equal(run[k], again[k]), (name, k)


@pytest.mark.parametrize("env", [(), (ic.NO_LDS,)], ids=["lds", "no_lds"])
def test_attempts_cut_into_two_calls_equal_one_call(env):
    tag = "-no_lds" if env else ""
    single, _ = _gpu(ic.case_by_id("4097-box_and_lines%s-single254" % tag))
    split, _ = _gpu(ic.case_by_id("4097-box_and_lines%s-split254" % tag))
    assert len(single["valid"]) == len(split["valid"]) == 254 and int(single["valid"].sum()) >= 100
    for k in ("valid", "ids", "inv", "recs", "segment", "prob", "lcp"):
        assert np.array_equal(single[k], split[k]), k


def test_the_table_takes_every_path_in_both_forms():
    """Over the whole table, per working-set form: a new flood fill with its parents in LDS, one with its parents in device memory, a
    reused mask, a failed first draw; and the 64-row maps put a disc on either side of INST_MAX_NODES."""
    per_form = {"instance_lds": ic.path_counts([]), "instance_device_memory": ic.path_counts([])}
    for case in CASES:
        run, _ = _gpu(case)
        assert run["forms"][0]["kernel"] == ic.working_set_form(case)
        for k, v in ic.path_counts(run["recs"]).items():
            per_form[ic.working_set_form(case)][k] += v
        nodes = run["recs"][:, 3]
        if case[2] == "rows64_16384":
            assert (nodes == ic.INST_MAX_NODES).any() and nodes.max() == ic.INST_MAX_NODES, (case[0], nodes.max())
        if case[2] == "rows64_16385":
            assert (nodes == ic.INST_MAX_NODES + 1).any(), (case[0], nodes.max())
    for form, counts in per_form.items():
        print(form, counts)
    for form, counts in per_form.items():
        for path in ic.PATHS:
            assert counts[path] >= 1, (form, path, counts)


def test_the_attempt_limit_refuses_and_leaves_the_context_usable(oracle_lib):
    from model_matching_amd import capi
    case = ic.case_by_id("65-box_and_lines")
    assert case[5] == ((0, 254),)                                  # 254 attempts are accepted (and equal the oracle: the table's test)
    want = _ref(oracle_lib, case)
    est = _estimator(65, "box_and_lines")
    try:
        for first, n in ((0, 255), (200, 55)):
            with pytest.raises(capi.StocsError) as e:
                est.sample_bases(ic.SEED, n, first_attempt=first, mode=1, dispersion=0.9)
            assert e.value.code == capi.ERR_INVALID
            with pytest.raises(capi.StocsError) as e:              # nothing ran: no record, no form
                est.last_instance_attempts()
            assert e.value.code == capi.ERR_STATE
            with pytest.raises(capi.StocsError):
                est.last_sampling_form()
        got = _run_calls(est, ((0, 254),), 0.9)
        assert _assert_bases_equal(want, got, "after the refusals") >= 3
        assert np.array_equal(got["segment"], want["segment"]) and np.array_equal(got["prob"].view(np.uint32), want["prob"].view(np.uint32))
        with pytest.raises(capi.StocsError):                       # the trial is used up: attempt 254 does not exist
            est.sample_bases(ic.SEED, 1, first_attempt=254, mode=1, dispersion=0.9)
        assert len(est.last_instance_attempts()) == 254            # (a refused call leaves the records of the last one that ran)
    finally:
        est.close()


@functools.lru_cache(maxsize=None)
def _n_cu():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked once per module in a child process: torch brings a HIP runtime of
    its own, which finds no device in a process where the library's runtime has opened it first (as every earlier test of a run has)"""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


@pytest.mark.parametrize("S,env", [(S, ()) for S in ic.BATCH_SIZES] + [(ic.BATCH_SIZES[0], (ic.NO_LDS,))],
                         ids=["%d" % S for S in ic.BATCH_SIZES] + ["%d-no_lds" % ic.BATCH_SIZES[0]])
def test_a_trial_batch_equals_its_trials_alone_and_the_oracle(oracle_lib, S, env):
    """Three trials in one launch, working set in LDS and in device memory (where every trial needs weights and survivor lists of its own:
    a batch of several trials there used to share those of its first trial)."""
    kind, n, seeds = "box_and_lines", ic.BATCH_ATTEMPTS, list(ic.BATCH_SEEDS)
    with _env(env):
        est = _estimator(S, kind)
        try:
            est.run_trials(seeds, n, mode=1, dispersion=0.9, max_per_base=1, keep_details=True)
            assert est.last_sampling_form() == ic.expected_form(S, env, n_trials=len(seeds), n_cu=_n_cu())
            bases = [est.trial_bases(t) for t in range(len(seeds))]
        finally:
            est.close()
    orc = ic.make_oracle(oracle_lib, S, kind)
    for t, seed in enumerate(seeds):
        got = dict(valid=bases[t][0], ids=bases[t][1], inv=bases[t][2])
        orc.restart_trial()
        want = ic.oracle_trial(oracle_lib, orc, S, kind, seed, n, 0.9, with_lcp=False)
        assert _assert_bases_equal(want, got, ("oracle", S, t)) >= 3
        alone = _estimator(S, kind)
        try:
            v, i, f = alone.sample_bases(seed, n, mode=1, dispersion=0.9)
        finally:
            alone.close()
        _assert_bases_equal(dict(valid=v, ids=i, inv=f), got, ("alone", S, t))


def test_a_trial_batch_cut_into_two_launches_equals_the_oracle(oracle_lib):
    """sample_trials launches at most n_cu / 2 trials at a time and moves fifteen pointers on for the next piece: one trial more than a launch
    holds, every trial against the oracle."""
    S, kind, n = ic.MANY_S, "box_and_lines", ic.MANY_ATTEMPTS
    per_launch = max(1, _n_cu() // 2)
    seeds = [7000 + 3 * t for t in range(per_launch + 1)]
    est = _estimator(S, kind)
    try:
        est.run_trials(seeds, n, mode=1, dispersion=0.9, max_per_base=1, keep_details=True)
        form = est.last_sampling_form()
        assert form == ic.expected_form(S, (), n_trials=len(seeds), n_cu=_n_cu()) and form["launches"] == 2
        bases = [est.trial_bases(t) for t in range(len(seeds))]
    finally:
        est.close()
    orc = ic.make_oracle(oracle_lib, S, kind)
    n_valid = 0
    for t, seed in enumerate(seeds):
        orc.restart_trial()
        want = ic.oracle_trial(oracle_lib, orc, S, kind, seed, n, 0.9, with_lcp=False)
        got = dict(valid=bases[t][0], ids=bases[t][1], inv=bases[t][2])
        last_of_first, second = bases[per_launch - 1], bases[per_launch]
        n_valid += _assert_bases_equal(want, got, ("trial %d of %d" % (t, len(seeds)), "last trial of the first launch:", last_of_first[1][last_of_first[0]].tolist(),
                                                    "the trial of the second launch:", second[1][second[0]].tolist()))
    assert n_valid >= 3 * len(seeds)
    assert bases[per_launch][0].sum() >= 3 and not np.array_equal(bases[per_launch][1], bases[per_launch - 1][1])
