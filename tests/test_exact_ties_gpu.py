"""The opt-in exact_ties mode (stocs_set_option "exact_ties" = 1): every (candidate, model point) query returns the scene index the
reference's kd-tree returns, exact float32 distance ties included (divergence Q11).  No tie escape anywhere here.

The fixture is a lattice scene (spacing 2^-9, symmetric about the origin: its float centroid is exactly zero, so centring keeps every
tie exact) and a symmetric model whose points sit on edge, face and body midpoints of the lattice cells.  Candidates are signed axis
permutations with half-spacing translations, so the transformed model points land on tie positions again."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
H = 2.0 ** -9
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _lattice_scene(seed, kx=24, kz=2):
    rng = np.random.default_rng(seed)
    rx = np.arange(-kx, kx + 1, dtype=np.float32) * np.float32(H)
    rz = np.arange(-kz, kz + 1, dtype=np.float32) * np.float32(H)
    g = np.stack(np.meshgrid(rx, rx, rz, indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))]
    nrm = _unit(np.concatenate([rng.normal(0, 0.45, (len(g), 2)), np.ones((len(g), 1))], 1))
    prob = (rng.integers(52, 513, len(g)) / 512.0).astype(np.float32)          # multiples of 2^-9 in [0.1, 1]
    return g.astype(np.float32), nrm, prob


def _lattice_model(seed, n_half=300, k=14):
    rng = np.random.default_rng(seed)
    c = rng.integers(-k, k, size=(n_half, 3)).astype(np.float32)
    c[:, 2] = rng.integers(-1, 1, n_half)
    off = rng.integers(0, 2, size=(n_half, 3)).astype(np.float32)
    off[off.sum(1) < 2, 0] = 1                                                   # at least two half offsets: 4- or 8-way ties (or 2 on an edge)
    p = (c + off * 0.5) * np.float32(H)
    p = np.concatenate([p, -p]).astype(np.float32)                               # symmetric: the model centroid is exactly zero
    nrm = _unit(np.concatenate([rng.normal(0, 0.3, (len(p), 2)), np.ones((len(p), 1))], 1))
    return p, nrm


def _candidates(seed, n):
    rng = np.random.default_rng(seed)
    perms = [(0, 1, 2), (1, 0, 2), (0, 1, 2), (1, 0, 2)]
    out = []
    for i in range(n):
        R = np.zeros((3, 3))
        pm = perms[rng.integers(0, len(perms))]
        for r, col in enumerate(pm):
            R[r, col] = 1.0
        R[0] *= rng.choice([-1.0, 1.0]); R[1] *= rng.choice([-1.0, 1.0])
        if np.linalg.det(R) < 0:
            R[2] *= -1.0
        M = np.eye(4); M[:3, :3] = R
        M[:3, 3] = rng.integers(-8, 9, 3) * (H / 2.0)
        M[2, 3] = rng.integers(-1, 2) * (H / 2.0)
        if i == 0:
            M = np.eye(4)
        out.append(M.T.reshape(16))
    return np.array(out, np.float32)


def _make(oracle_lib, scene_seed, dense, monkeypatch, build_index=False):
    from model_matching_amd.estimator import StocsEstimator
    sp, sn, sprob = _lattice_scene(scene_seed)
    mp, mn = _lattice_model(5)
    if dense:
        monkeypatch.setenv("STOCS_GRID_DENSE", "1")                              # centre-sorted lists (variant 39 / 31 territory)
    est = StocsEstimator(sp, sn, sprob, None, mp, mn, build_index=build_index)
    monkeypatch.delenv("STOCS_GRID_DENSE", raising=False)
    orc = oracle_lib.Oracle(sp, sn, sprob, None, mp, mn, build_index=False)
    assert np.array_equal(orc.scene_centred(), sp) and np.array_equal(orc.model_centred(), mp)
    return est, orc


@pytest.fixture(params=[False, True], ids=["sparse", "dense"])
def lattice(request, oracle_lib, monkeypatch):
    est, orc = _make(oracle_lib, 3, request.param, monkeypatch)
    yield est, orc, _candidates(7, 96)
    est.close()


def _parity(est, orc, T):
    for c in range(len(T)):
        hg, cg = est.lcp_detail(T[c])
        ho, co = orc.lcp_detail(T[c])
        assert np.array_equal(hg, ho), (c, np.nonzero(hg != ho)[0][:8])
        assert np.array_equal(cg, co), c


def test_fixture_exercises_q11_in_default_mode(lattice):
    est, orc, T = lattice
    differs = 0
    for c in range(16):
        differs += int((est.lcp_detail(T[c])[0] != orc.lcp_detail(T[c])[0]).sum())
    assert differs > 0
    assert est.last_tie_counts() == (0, 0)


# the kernel forms of test_per_point_parity_every_form (tests/test_ref_accel_gpu.py walks the same list), and the settings that undo one
FORMS = ({"lcp_variant": 0}, {"lcp_variant": 31}, {"lcp_variant": 39}, {"lcp_variant": 24},
         {"lcp_split": 0, "lcp_flat": 0}, {"lcp_split": 1, "lcp_flat": 1, "lcp_cull": 2}, {"lcp_cull": 0, "lcp_order": 2})
FORM_DEFAULTS = (("lcp_variant", 99), ("lcp_split", 1), ("lcp_flat", 1), ("lcp_cull", 1), ("lcp_order", 1))


def test_per_point_parity_every_form(lattice):
    est, orc, T = lattice
    est.set_option("exact_ties", 1)
    _parity(est, orc, T[:64])
    for opts in FORMS:
        for k, v in opts.items():
            est.set_option(k, v)
        _parity(est, orc, T[:16])
        for k, v in FORM_DEFAULTS:
            est.set_option(k, v)


def test_scores_hit_counts_and_counters(lattice):
    est, orc, T = lattice
    est.set_option("exact_ties", 1)
    got = est.score_transforms(T)
    f, ch = est.last_tie_counts()
    assert f > 0 and ch > 0 and ch <= f
    ref, ex = orc.lcp_batch_exact(T)
    assert np.abs(got.astype(np.float64) - ex).max() <= 1e-7
    assert np.abs(got - ref).max() <= 1e-5
    # lcp_hit_count: the same matches as the oracle's per-point rows
    dT = est.dev_alloc(T.nbytes)
    try:
        est.dev_upload(dT, T)
        hits, counted = est.lcp_hit_count(dT, len(T))
    finally:
        est.dev_free(dT)
    h_ref = c_ref = 0
    for c in range(len(T)):
        ho, co = orc.lcp_detail(T[c])
        h_ref += int((ho >= 0).sum()); c_ref += int(co.sum())
    assert (hits, counted) == (h_ref, c_ref)
    # off again: default rule, counters 0 / 0
    est.set_option("exact_ties", 0)
    est.score_transforms(T)
    assert est.last_tie_counts() == (0, 0)


def _argmax_batch(est, orc, T):
    """two candidates whose order under the largest-index rule differs from the reference's: the batch [j, i], where i wins"""
    est.set_option("exact_ties", 0)
    dflt = est.score_transforms(T)
    _, ex = orc.lcp_batch_exact(T)
    for i in range(len(T)):
        for j in range(len(T)):
            if i != j and ex[i] > ex[j] + 1e-9 and dflt[j] >= dflt[i]:
                return T[[j, i]]
    return None


def test_argmax_key_is_the_references_first_maximum(lattice, oracle_lib):
    est, orc, T = lattice
    B = _argmax_batch(est, orc, T)
    assert B is not None
    ref = orc.lcp_batch(B)
    want = 1
    assert oracle_lib.best(ref)[0] == want
    dT = est.dev_alloc(B.nbytes); dL = est.dev_alloc(4 * len(B)); dK = est.dev_alloc(8)
    try:
        est.dev_upload(dT, B)
        _, idx_default = est.score_best_device(dT, len(B), dL)
        assert idx_default != want                                              # the largest-index rule picks the other one
        est.set_option("exact_ties", 1)
        s, idx = est.score_best_device(dT, len(B), dL)
        assert idx == want and abs(s - ref[want]) <= 1e-5
        est.score_best_device_async(dT, len(B), dL, 0, dK.value)
        key = np.zeros(1, np.uint64)
        est.sync()
        est.dev_download(dK, key)
        assert 0xFFFFFFFF - (int(key[0]) & 0xFFFFFFFF) == want
        scores = np.zeros(len(B), np.float32)
        est.dev_download(dL, scores)
        assert np.array_equal(scores, est.score_transforms(B))
    finally:
        for p in (dT, dL, dK):
            est.dev_free(p)


def test_toggle_across_scenes_and_no_warm_allocations(oracle_lib, monkeypatch):
    from model_matching_amd import capi
    est, orc = _make(oracle_lib, 3, False, monkeypatch)
    T = _candidates(9, 24)
    est.set_option("exact_ties", 1)
    _parity(est, orc, T[:8])
    est.set_option("exact_ties", 0)
    # a second scene: the same lattice in another index order (the tree and the tie answers change with it)
    sp2, sn2, sprob2 = _lattice_scene(4)
    est.set_scene(sp2, sn2, sprob2)
    mp, mn = _lattice_model(5)
    orc2 = oracle_lib.Oracle(sp2, sn2, sprob2, None, mp, mn, build_index=False)
    est.set_option("exact_ties", 1)
    _parity(est, orc2, T[:8])
    est.score_transforms(T)
    assert est.last_tie_counts()[1] > 0
    # option on at stocs_ctx_set_scene: the tree is built there, for the new scene
    est.set_scene(*_lattice_scene(3))
    _parity(est, orc, T[:8])
    L = capi.load()
    est.score_transforms(T)
    a0 = L.stocs_device_alloc_count()
    for _ in range(3):
        est.score_transforms(T)
        est.lcp_detail(T[0])
    assert L.stocs_device_alloc_count() == a0
    est.close()


def test_option_values(lattice):
    from model_matching_amd import capi
    est, orc, T = lattice
    for v in (-1, 2, 7):
        with pytest.raises(capi.StocsError):
            est.set_option("exact_ties", v)
    est.set_option("exact_ties", 1)
    est.set_option("exact_ties", 0)


@pytest.mark.parametrize("name", ["tiny", "small", "dense"])
def test_synth_workloads_per_point_parity(name, oracle_lib):
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, k = synth.workload(name)
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    orc = oracle_lib.Oracle(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    cs, cm = orc.centroids()
    T = synth.make_candidates(synth.centred_gt(s.T_gt, cs.astype(np.float64), cm.astype(np.float64)), k)
    est.set_option("exact_ties", 1)
    got = est.score_transforms(T)
    assert np.abs(got - orc.lcp_batch(T, nthreads=4)).max() <= 1e-5
    _parity(est, orc, T[list(range(12)) + [int(np.argmax(got))]])
    est.close()


def _single(est, seed, n_attempts, mode, max_per_base):
    est.reset_trial()
    est.sample_bases(seed, n_attempts, mode=mode, dispersion=0.9)
    est.find_congruent_all()
    est.make_transforms(max_per_base, seed)
    lcp, idx, pose = est.compute_best_transform()
    T, P, l, b = est.get_pose_candidates()
    return dict(best_lcp=lcp, best_index=idx, best_pose=pose.copy(), lcp=l)


def test_trial_batches(oracle_lib, monkeypatch):
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, k = synth.workload("tiny")
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    est.set_option("exact_ties", 1)
    # class mode against the restated run_stocs_estimation
    orc = oracle_lib.Oracle(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    seeds = [1234, 7, 99]
    res = est.run_trials(seeds, 40, max_per_base=50)
    for t, seed in enumerate(seeds):
        r = orc.run(seed, 40, 50)
        assert res[t]["n_candidates"] == r.n_candidates and res[t]["best_index"] == r.best_index, t
        assert abs(res[t]["best_lcp"] - r.best_lcp) <= 1e-5, t
    # several pieces == one piece
    monkeypatch.setenv("STOCS_TRIALS_PER_PIECE", "1")
    cut = est.run_trials(seeds, 40, max_per_base=50)
    monkeypatch.delenv("STOCS_TRIALS_PER_PIECE")
    for a, b in zip(res, cut):
        assert a["best_lcp"] == b["best_lcp"] and a["best_index"] == b["best_index"] and np.array_equal(a["best_pose"], b["best_pose"])
    est.close()
    # instance mode: each trial of the batch equals the single-trial sequence run alone with the option on
    d = np.load(os.path.join(GOLD, "example_packed_dove.npz"))
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
    est.set_edge_map(d["edge_map"])
    est.set_option("exact_ties", 1)
    seeds = [1, 2, 3]
    res = est.run_trials(seeds, 24, mode=1, max_per_base=200, keep_details=True)
    lcps = [est.trial_candidates(t)[2] for t in range(len(seeds))]
    for t, seed in enumerate(seeds):
        ref = _single(est, seed, 24, 1, 200)
        assert np.array_equal(lcps[t].view(np.uint32), ref["lcp"].view(np.uint32)), t
        assert res[t]["best_index"] == ref["best_index"] and res[t]["best_lcp"] == ref["best_lcp"], t
        assert np.array_equal(res[t]["best_pose"].view(np.uint32), ref["best_pose"].view(np.uint32)), t
    est.close()
