"""GPU parity of the batched LCP verification kernel (the metric kernel) against the CPU oracle.
Calls go through the C ABI (libstocs_hip.so).  Integer results (matched scene index, counted flag)
must be bit-exact; the score is a float sum accumulated in a different (tree) order than the
reference's sequential loop, tolerance 1e-5 absolute on a value in [0, 1]."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LCP_TOL = 1e-5


def _setup(name, oracle_lib):
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, k = synth.workload(name)
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    orc = oracle_lib.Oracle(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    cs, cm = orc.centroids()
    Tgt = synth.centred_gt(s.T_gt, cs.astype(np.float64), cm.astype(np.float64))
    return m, s, k, est, orc, Tgt


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_scores_and_matches_equal_oracle(name, oracle_lib):
    from model_matching_amd import synth
    m, s, k, est, orc, Tgt = _setup(name, oracle_lib)
    assert np.array_equal(est.get_scene_centroid(), orc.centroids()[0])      # centroid_shift parity
    assert np.array_equal(est.get_model_centroid(), orc.centroids()[1])
    T = synth.make_candidates(Tgt, k)
    got = est.score_transforms(T)
    ref = orc.lcp_batch(T, nthreads=4)
    assert np.abs(got - ref).max() <= LCP_TOL
    assert got.max() > 0.05 and (got == 0).sum() < len(got)
    # arg-max parity (first maximum wins)
    assert int(np.argmax(got)) == oracle_lib.best(ref)[0] or abs(got.max() - ref.max()) <= LCP_TOL
    # per-point parity: matched scene index and counted flag, bit-exact
    pos = orc.scene_centred()
    checked = 0
    for c in list(range(12)) + [int(np.argmax(got))]:
        hg, cg = est.lcp_detail(T[c])
        ho, co = orc.lcp_detail(T[c])
        if not np.array_equal(hg, ho):
            # only exact-distance ties may differ (kd-tree visiting order, Q11)
            for i in np.nonzero(hg != ho)[0]:
                assert hg[i] >= 0 and ho[i] >= 0
            continue
        assert np.array_equal(cg, co)
        checked += 1
    assert checked >= 10


def test_edge_cases(oracle_lib):
    from model_matching_amd import synth
    m, s, k, est, orc, Tgt = _setup("tiny", oracle_lib)
    # empty batch
    assert len(est.score_transforms(np.zeros((0, 16), np.float32))) == 0
    # model thrown far outside the scene grid: nothing matches
    far = np.eye(4); far[:3, 3] = [50.0, -40.0, 30.0]
    Tfar = far.T.reshape(1, 16).astype(np.float32)
    assert est.score_transforms(Tfar)[0] == 0.0 and orc.lcp(Tfar[0]) == 0.0
    # ragged batch sizes (not a multiple of the 4 candidates per workgroup)
    T = synth.make_candidates(Tgt, 7)
    assert np.abs(est.score_transforms(T) - orc.lcp_batch(T)).max() <= LCP_TOL
    # exact ground truth scores high; flipped (mirrored-normal) transform scores ~0
    Tg = Tgt.T.reshape(1, 16).astype(np.float32)
    g = est.score_transforms(Tg)[0]
    assert abs(g - orc.lcp(Tg[0])) <= LCP_TOL and g > 0.2
    # NaN transform: no match, score 0 on both sides
    Tn = Tg.copy(); Tn[0, 12] = np.nan
    assert est.score_transforms(Tn)[0] == 0.0 and orc.lcp(Tn[0]) == 0.0


def test_identity_on_self_reproduces_q7(oracle_lib):
    """Scene == model, T = I: points whose |n|^2 rounds above 1 are NOT counted (acos -> NaN)."""
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m = synth.make_model(300, seed=5)
    prob = np.linspace(0.2, 1.0, 300).astype(np.float32)
    est = StocsEstimator(m.pos, m.nrm, prob, None, m.pos, m.nrm, build_index=False)
    orc = oracle_lib.Oracle(m.pos, m.nrm, prob, None, m.pos, m.nrm, build_index=False)
    T = np.eye(4, dtype=np.float32).reshape(16)
    hg, cg = est.lcp_detail(T)
    ho, co = orc.lcp_detail(T)
    assert np.array_equal(hg, ho) and np.array_equal(cg, co) and (hg == np.arange(300)).all()
    assert 150 < cg.sum() < 300
    assert abs(est.compute_alignment_score_for_rigid_transform(T) - orc.lcp(T)) <= LCP_TOL


def test_full_size_properties(oracle_lib):
    """Cm size (20k scene, 5k model): size-independent properties + a sampled oracle comparison."""
    from model_matching_amd import synth
    m, s, k, est, orc, Tgt = _setup("Cm", oracle_lib)
    T = synth.make_candidates(Tgt, 4096)
    got = est.score_transforms(T)
    assert got.min() >= 0.0 and got.max() <= 1.0
    # batch invariance: a candidate's score does not depend on its batch or position in it
    perm = np.random.default_rng(0).permutation(len(T))
    assert np.array_equal(est.score_transforms(T[perm]), got[perm])
    assert np.array_equal(est.score_transforms(T[:1000]), got[:1000])
    # run-to-run determinism
    assert np.array_equal(est.score_transforms(T), got)
    # the tight tier (<= 1 mm / 1 deg from ground truth) outscores the loose tier on average
    ref, exact = orc.lcp_batch_exact(T[:2048], nthreads=16)      # bench.py compares all 65 536 of its batch (oracle_check in the bench line)
    assert np.abs(got[:2048] - ref).max() <= LCP_TOL
    # the kernel adds the weights as integers: against the double sum of the oracle's matches only the final rounding to float
    # is left (the 1e-6 against `ref` is the drift of the reference's running float sum)
    assert np.abs(got[:2048].astype(np.float64) - exact).max() <= 1e-7
    # every kernel option leaves the scores bit for bit (integer accumulation): flat cell table, four wavefronts per candidate
    for opt in ("lcp_flat", "lcp_split"):
        est.set_option(opt, 0)
        assert np.array_equal(est.score_transforms(T), got), opt
        est.set_option(opt, 1)
    gt = est.score_transforms(Tgt.T.reshape(1, 16).astype(np.float32))[0]
    assert gt > np.percentile(got, 90)


def test_metric_batch_all_65536_candidates_equal_oracle(oracle_lib):
    """The metric configuration at its full size: EVERY one of the 65 536 candidates of bench.py's Cm batch (same seed)
    against the oracle's kd-tree LCP (stocs.cpp:1006-1041, kdtree.h:394-459), so that parity at the size the headline number
    is quoted on does not depend on bench.py's epilogue.  Tolerance 1e-5 absolute on a score in [0, 1] (the reference's
    running float sum drifts from the exact mean in the last figure); against the double sum of the oracle's own matches
    only the final rounding to float is left (1e-7); the arg-max (first maximum) must be the same candidate."""
    import os
    from model_matching_amd import synth
    m, s, k, est, orc, Tgt = _setup("Cm", oracle_lib)
    assert (est.nS, est.nM, k) == (20000, 5000, 65536)
    T = synth.make_candidates(Tgt, k, seed=synth.SEED_CAND)
    got = est.score_transforms(T)
    nthreads = max(1, min(16, len(os.sched_getaffinity(0))))
    ref, exact = orc.lcp_batch_exact(T, nthreads=nthreads)
    assert len(ref) == k
    assert np.abs(got - ref).max() <= LCP_TOL
    assert np.abs(got.astype(np.float64) - exact).max() <= 1e-7
    assert int(np.argmax(got)) == int(np.argmax(ref))
    dT, dL = est.dev_alloc(T.nbytes), est.dev_alloc(k * 4)
    est.dev_upload(dT, T)
    est.score_device(dT, k, dL)
    bl, bi, key_two_kernels = est.best_device(dL, k, 0)
    assert bi == int(np.argmax(got)) and bl == float(got[bi])
    # the arg-max taken in the scoring kernel's epilogue (what bench.py times per step): the same key, the same scores
    dK = est.dev_alloc(8)
    est.score_best_device_async(dT, k, dL, 0, dK.value)
    kb = np.zeros(1, np.uint64); again = np.zeros(k, np.float32)
    est.dev_download(dK, kb); est.dev_download(dL, again)
    assert int(kb[0]) == key_two_kernels and np.array_equal(again, got)
    est.score_best_device_async(dT, k, dL, 7 * k, dK.value)          # global ids of rank 7 of a sharded run
    est.dev_download(dK, kb)
    from model_matching_amd import dist as sd
    assert sd.unpack_best(int(kb[0])) == (float(got[bi]), 7 * k + bi)
    est.dev_free(dT); est.dev_free(dL); est.dev_free(dK)


def test_config5_200k_scene_50k_model(oracle_lib):
    """BASELINE config 5 (synthetic 200k-point scene vs 50k-point model, 16 384 candidates; no PPF index at this size,
    SURVEY 8d): the verify path of stocs.cpp:1006-1041 / kdtree.h:394-459 at its full size against the oracle --
    256 candidates' scores, per-point matches of 3 candidates, and size-independent properties on the whole batch."""
    from model_matching_amd import synth
    m, s, k, est, orc, Tgt = _setup("C5", oracle_lib)
    assert (est.nS, est.nM, k) == (200000, 50000, 16384)
    assert np.array_equal(est.get_scene_centroid(), orc.centroids()[0]) and np.array_equal(est.get_model_centroid(), orc.centroids()[1])
    T = synth.make_candidates(Tgt, k)
    got = est.score_transforms(T)
    assert got.min() >= 0.0 and got.max() <= 1.0 and got.max() > 0.2
    n_ref = 256
    ref = orc.lcp_batch(T[:n_ref], nthreads=16)
    assert np.abs(got[:n_ref] - ref).max() <= LCP_TOL
    # per-point parity on the best, the median and a poor candidate of the checked block: matched scene index and counted
    # flag bit-exact; only exact-distance ties may pick another point (kd-tree visiting order, Q11)
    order = np.argsort(ref)
    for c in (int(order[-1]), int(order[n_ref // 2]), int(order[3])):
        hg, cg = est.lcp_detail(T[c])
        ho, co = orc.lcp_detail(T[c])
        diff = np.nonzero(hg != ho)[0]
        assert len(diff) <= 2 and all(hg[i] >= 0 and ho[i] >= 0 for i in diff)
        same = hg == ho
        assert np.array_equal(cg[same], co[same]) and (hg >= 0).sum() > 0
    # determinism and batch invariance over all 16 384 candidates
    assert np.array_equal(est.score_transforms(T), got)
    perm = np.random.default_rng(1).permutation(k)
    assert np.array_equal(est.score_transforms(T[perm]), got[perm])
    assert np.array_equal(est.score_transforms(T[5000:5100]), got[5000:5100])
    # a ragged batch on the automatic ordered path: XCD runs of 128 slots, 15 whole rounds of 8 x 128 workgroups and a tail of 1 021
    ragged = 16381
    assert np.array_equal(est.score_transforms(T[:ragged]).view(np.uint32), got[:ragged].view(np.uint32))
    dT, dL = est.dev_alloc(T.nbytes), est.dev_alloc(k * 4)
    est.dev_upload(dT, T)
    # the same into a buffer that holds -1 everywhere (scores are >= 0): a slot the placement skipped would keep it, while the scratch
    # block of score_transforms still holds the right score from the call before
    est.dev_upload(dL, np.full(ragged, -1.0, np.float32))
    est.score_device(dT, ragged, dL)
    again = np.zeros(ragged, np.float32)
    est.dev_download(dL, again)
    assert not (again == -1.0).any() and np.array_equal(again.view(np.uint32), got[:ragged].view(np.uint32))
    # the device arg-max picks the first maximum of those scores
    est.score_device(dT, k, dL)
    sc, gid, key = est.best_device(dL, k)
    assert gid == int(np.argmax(got)) and sc == float(got.max())
    est.dev_free(dT); est.dev_free(dL)
    gt = est.score_transforms(Tgt.T.reshape(1, 16).astype(np.float32))[0]
    assert gt > np.percentile(got, 90)
    est.close()


def test_device_argmax_matches_reference_rule(oracle_lib):
    """stocs_best_device == compute_best_transform's arg-max (stocs.cpp:982-1004): first maximum, none if all zero."""
    from model_matching_amd import synth
    m, s, k, est, orc, Tgt = _setup("tiny", oracle_lib)
    T = synth.make_candidates(Tgt, 777)
    T[500] = T[100]                      # an exact tie: the lower id must win
    got = est.score_transforms(T)
    dT, dL = est.dev_alloc(T.nbytes), est.dev_alloc(len(T) * 4)
    est.dev_upload(dT, T)
    est.score_device(dT, len(T), dL)
    sc, gid, key = est.best_device(dL, len(T), 1000)
    i, ref = oracle_lib.best(got)
    assert gid == 1000 + i and sc == ref
    got2 = got.copy(); got2[:] = 0.0
    est.dev_upload(dL, got2)
    assert est.best_device(dL, len(T))[:2] == (0.0, -1)
    got2[100] = got2[500] = 0.25
    est.dev_upload(dL, got2)
    assert est.best_device(dL, len(T))[:2] == (0.25, 100)
    est.dev_free(dT); est.dev_free(dL)


def test_all_scan_variants_on_sparse_scene(oracle_lib):
    """Every scan kernel selectable through stocs_set_option agrees with the oracle on a 5 mm scene."""
    from model_matching_amd import synth
    m, s, k, est, orc, Tgt = _setup("small", oracle_lib)
    T = synth.make_candidates(Tgt, 600)
    ref = orc.lcp_batch(T, nthreads=8)
    best = int(np.argmax(ref))
    ho, co = orc.lcp_detail(T[best])
    for v in (0, 24, 31):                       # (31 is a dense-scene kernel: on this grid it maps to 24)
        est.set_option("lcp_variant", v)
        assert np.abs(est.score_transforms(T) - ref).max() <= LCP_TOL, v
        hg, cg = est.lcp_detail(T[best])
        assert np.array_equal(hg, ho) and np.array_equal(cg, co), v
    est.set_option("lcp_variant", 99)
    # measurement-only kernels (and the timing ablations of round 1) are not part of the product library
    from model_matching_amd import capi
    for v in (1, 9, 10, 11, 12, 13, 14, 15, 16, 20, 28, 98, -1):
        with pytest.raises(capi.StocsError):
            est.set_option("lcp_variant", v)


def test_dense_scene_and_all_scan_variants(oracle_lib):
    """Dense scene (~1.6 mm spacing): long candidate lists -> epsilon/2 grid + unrolled cooperative scan.
    Every scan variant must agree with the oracle (per-point matches bit-exact) and with each other."""
    from model_matching_amd import synth
    m, s, k, est, orc, Tgt = _setup("dense", oracle_lib)
    T = synth.make_candidates(Tgt, k)
    ref = orc.lcp_batch(T, nthreads=8)
    got = est.score_transforms(T)                      # automatic choice
    assert np.abs(got - ref).max() <= LCP_TOL and got.max() > 0.05
    best = int(np.argmax(ref))
    ho, co = orc.lcp_detail(T[best])
    for v in (0, 31, 39, 24):     # 39: queue-fed scan with early exit (the default here); on a dense (centre-sorted) grid 24 maps to it
        est.set_option("lcp_variant", v)
        gv = est.score_transforms(T)
        assert np.abs(gv - ref).max() <= LCP_TOL, v
        hg, cg = est.lcp_detail(T[best])
        same = hg == ho
        assert same.mean() > 0.999, v                  # only exact-distance ties may differ (Q11)
        assert np.array_equal(cg[same], co[same]), v
    est.set_option("lcp_variant", 99)


def test_processing_order_does_not_change_scores(oracle_lib):
    """Big batches are processed in a spatial order of the candidates (and optionally in XCD-contiguous blocks):
    every score must be bitwise identical to the plain batch order, and the device arg-max must pick the same
    first maximum."""
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, k = synth.workload("small")
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    cs, cm = est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64)
    n = 160000                                  # x 1000 model points: above the ordering threshold of launch_lcp
    T = synth.make_candidates(synth.centred_gt(s.T_gt, cs, cm), n)
    T[123, 12:15] = np.nan                      # a NaN translation sorts somewhere and still scores like in batch order
    T[7] = T[5]                                 # duplicate candidates: equal scores, the lower index wins the arg-max
    outs = []
    for mode in (0, 1, 2):
        est.set_option("lcp_order", mode)
        outs.append(est.score_transforms(T))
    assert np.array_equal(outs[0], outs[1], equal_nan=True) and np.array_equal(outs[0], outs[2], equal_nan=True)
    assert outs[0][5] == outs[0][7]
    est.close()
