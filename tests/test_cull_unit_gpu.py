"""The unit of the patch test (stocs_set_option "lcp_cull_unit"): 16-point sub-patches, the live ones packed four to a step of
the wavefront, against whole 64-point steps and against no test at all.  A culled point has no scene point within epsilon, and
scores are integer sums, so every result must be the same BITWISE in all three: scores, arg-max keys, per-point rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = [("off", 0, 64), ("unit64", 2, 64), ("unit16", 2, 16)]


def _setup(name):
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, k = synth.workload(name)
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    cs = est.get_scene_centroid().astype(np.float64); cm = est.get_model_centroid().astype(np.float64)
    return m, s, k, est, synth.centred_gt(s.T_gt, cs, cm)


def _mode(est, cull, unit):
    est.set_option("lcp_cull", cull)
    est.set_option("lcp_cull_unit", unit)


def _odd_transforms(near, rng):
    """the transforms of test_cull_gpu.py the sphere bound has to hold for: scaled, sheared, mirrored, flattened, not finite"""
    odd = near[:64].reshape(64, 4, 4).copy()
    for i in range(64):
        A = odd[i, :3, :3].T.astype(np.float64)
        kind = i % 4
        if kind == 0: A = A * rng.uniform(0.3, 2.5)
        elif kind == 1: A = A @ (np.eye(3) + rng.uniform(-0.6, 0.6, (3, 3)))
        elif kind == 2: A = A @ np.diag([1.0, -1.0, 1.0])
        else: A = A @ np.diag([1.0, 1.0, 1e-3])
        odd[i, :3, :3] = A.T.astype(np.float32)
    bad = near[:8].copy()
    bad[0, 12] = np.nan; bad[1, 0] = np.inf; bad[2, 13] = -np.inf; bad[3, 14] = 3e38; bad[4, 5] = 1e30; bad[5, :] = 0.0; bad[6, 12:15] = [1e6, -1e6, 1e6]
    return np.concatenate([odd.reshape(64, 16), bad])


def _scores_and_key(est, T):
    k = len(T)
    dT, dL, dK = est.dev_alloc(T.nbytes), est.dev_alloc(k * 4), est.dev_alloc(8)
    est.dev_upload(dT, T)
    est.score_best_device_async(dT, k, dL, 0, dK.value)
    key = np.zeros(1, np.uint64); out = np.zeros(k, np.float32)
    est.dev_download(dK, key); est.dev_download(dL, out)
    for p in (dT, dL, dK):
        est.dev_free(p)
    return out, int(key[0])


@pytest.mark.parametrize("name", ["tiny", "small", "dense", "Cm"])
def test_units_bitwise_equal(name):
    from model_matching_amd import synth
    m, s, k, est, Tgt = _setup(name)
    rng = np.random.default_rng(17)
    near = synth.make_candidates(Tgt, min(k, 8192))
    T = np.concatenate([near, _odd_transforms(near, rng)])
    res = {}
    for label, cull, unit in MODES:
        _mode(est, cull, unit)
        res[label] = _scores_and_key(est, T)
        # per-point rows of a few candidates: near, odd, not finite
        res[label] += (tuple(est.lcp_detail(T[c]) for c in (0, 5, len(near), len(near) + 1, len(near) + 2, len(T) - 8, len(T) - 5)),)
    base_s, base_key, base_rows = res["off"]
    assert base_s.max() > 0.05 and base_key != 0
    for label in ("unit64", "unit16"):
        s_, key, rows = res[label]
        assert np.array_equal(s_.view(np.uint32), base_s.view(np.uint32)), label
        assert key == base_key, label
        for (h0, c0), (h1, c1) in zip(base_rows, rows):
            assert np.array_equal(h0, h1) and np.array_equal(c0, c1), label


def test_units_on_a_scene_change_and_one_wavefront_per_candidate():
    """a new scene on the same context (the field is rebuilt, the model's spheres stay), and lcp_split 0 (one wavefront walks all
    the steps: more than one ballot window of sub-patches per wavefront)"""
    from model_matching_amd import synth
    m, s, k, est, Tgt = _setup("Cm")
    T = synth.make_candidates(Tgt, 4096)
    est.set_scene(s.pos + np.array([0.011, -0.006, 0.017], np.float32), s.nrm, s.prob, s.pixel)
    for split in (1, 0):
        est.set_option("lcp_split", split)
        outs = {}
        for label, cull, unit in MODES:
            _mode(est, cull, unit)
            outs[label] = est.score_transforms(T)
        assert outs["off"].max() > 0.05
        for label in ("unit64", "unit16"):
            assert np.array_equal(outs[label].view(np.uint32), outs["off"].view(np.uint32)), (split, label)


def test_units_on_trial_winners():
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, _ = synth.workload("tiny")
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    seeds = list(range(300, 316))
    res = {}
    for label, cull, unit in MODES:
        _mode(est, cull, unit)
        res[label] = est.run_trials(seeds, 40, max_per_base=40)
    assert any(r["best_lcp"] > 0 for r in res["off"])
    for label in ("unit64", "unit16"):
        for a, b in zip(res["off"], res[label]):
            assert a["best_index"] == b["best_index"] and a["best_lcp"] == b["best_lcp"] and a["n_candidates"] == b["n_candidates"], label
            assert np.array_equal(np.asarray(a["best_pose"]).view(np.uint32), np.asarray(b["best_pose"]).view(np.uint32)), label


def test_option_values():
    from model_matching_amd import capi
    m, s, k, est, Tgt = _setup("tiny")
    for bad in (0, 8, 32, 128, -16):
        with pytest.raises(capi.StocsError):
            est.set_option("lcp_cull_unit", bad)
    est.set_option("lcp_cull_unit", 64)
    est.set_option("lcp_cull_unit", 16)
