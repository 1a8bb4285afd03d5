"""The pick draw of stocs_make_transforms at its edges: a base with strictly fewer quads than the per-base maximum is used whole, in
set order (stocs_match_one_object.cpp:126); a base AT the maximum, or above it, gets the seeded draw.  Per-base maxima around the
quad count of one base and around the largest count of the trial -- every base drawn, every base whole, and the two sides of the
threshold -- with the picks drawn on the device, drawn on the host (STOCS_TRANSFORMS_HOST_PICKS=1) and by the oracle's own
restatement of the draw: candidate count, T, pose and base index bit for bit equal among the three.  And a trial batch whose bases
draw with the seed and slot of THEIR trial, in both forms, against the same trials run alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED, ATTEMPTS = 4321, 60


@pytest.fixture(scope="module")
def setup(oracle_lib):
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, k = synth.workload("tiny")
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    orc = oracle_lib.Oracle(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    return est, orc


@pytest.fixture(scope="module")
def counts(setup):
    """quad count of every base of the trial (SEED, ATTEMPTS), read once through get_quads"""
    est, orc = setup
    est.L.stocs_clear_bases(est.h)
    valid, ids, inv = est.sample_bases(SEED, ATTEMPTS)
    est.find_congruent_all()
    return np.array([len(est.get_quads(k)) for k in range(int(valid.sum()))], np.int64)


def _maxima(counts):
    """-> {label: max_per_base}: nq* = the count of the first base with at least two quads, nmax = the largest count"""
    big = counts[counts >= 2]
    assert len(big), counts
    nq, nmax = int(big[0]), int(counts.max())
    return {"one": 1, "two": 2, "nq-1": nq - 1, "nq": nq, "nq+1": nq + 1, "nmax+1": nmax + 1}


@pytest.mark.parametrize("case", ["one", "two", "nq-1", "nq", "nq+1", "nmax+1"])
def test_device_draw_host_draw_and_oracle_agree_around_the_threshold(setup, counts, case, monkeypatch):
    est, orc = setup
    mpb = _maxima(counts)[case]
    n_whole, n_drawn = int(((counts > 0) & (counts < mpb)).sum()), int((counts >= mpb).sum())
    if case == "one":
        assert n_whole == 0 and n_drawn > 0           # every base large
    if case == "nmax+1":
        assert n_drawn == 0 and n_whole > 0           # every base small
    if case == "nq":
        assert (counts == mpb).any()                  # a base at exactly the maximum: drawn, not taken whole
    if case == "nq+1":
        assert (counts == mpb - 1).any()              # one below the maximum: taken whole, in set order
    est.L.stocs_clear_bases(est.h)
    est.sample_bases(SEED, ATTEMPTS)
    est.find_congruent_all()
    monkeypatch.delenv("STOCS_TRANSFORMS_HOST_PICKS", raising=False)
    n_dev = est.make_transforms(mpb, SEED)
    dev = est.get_pose_candidates()
    monkeypatch.setenv("STOCS_TRANSFORMS_HOST_PICKS", "1")
    n_host = est.make_transforms(mpb, SEED)
    host = est.get_pose_candidates()
    r = orc.run(SEED, ATTEMPTS, mpb)
    To, Po, bo = orc.candidates()
    print("max_per_base %d: %d bases whole, %d drawn; candidates device %d host %d oracle %d" % (mpb, n_whole, n_drawn, n_dev, n_host, r.n_candidates))
    assert n_dev == n_host == r.n_candidates == len(To) and n_dev > 0
    assert np.array_equal(dev[0], To) and np.array_equal(dev[1], Po) and np.array_equal(dev[3], bo)
    assert np.array_equal(host[0], To) and np.array_equal(host[1], Po) and np.array_equal(host[3], bo)
    assert np.array_equal(dev[0].view(np.uint32), host[0].view(np.uint32)) and np.array_equal(dev[1].view(np.uint32), host[1].view(np.uint32))


@pytest.mark.parametrize("host_picks", [False, True])
def test_batch_draws_with_the_seed_and_slot_of_each_trial(setup, host_picks, monkeypatch):
    est, orc = setup
    seeds = [11, 12, 13]
    if host_picks:
        monkeypatch.setenv("STOCS_TRANSFORMS_HOST_PICKS", "1")
    else:
        monkeypatch.delenv("STOCS_TRANSFORMS_HOST_PICKS", raising=False)
    res = est.run_trials(seeds, 24, max_per_base=2, keep_details=True)
    got = [est.trial_candidates(t) for t in range(len(seeds))]
    total = 0
    for t, seed in enumerate(seeds):
        est.reset_trial()
        est.sample_bases(seed, 24)
        est.find_congruent_all()
        n = est.make_transforms(2, seed)
        T, P, l, b = est.get_pose_candidates()
        assert res[t]["n_candidates"] == n == len(got[t][0]), t
        assert np.array_equal(got[t][0].view(np.uint32), T.view(np.uint32)) and np.array_equal(got[t][1].view(np.uint32), P.view(np.uint32)), t
        assert np.array_equal(got[t][3], b), t
        total += n
    assert total > 0
