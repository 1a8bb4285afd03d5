"""Post-processing inside trial batches (stocs_run_trials_post): every trial's candidates clustered on the device
(clustering::greedy_clustering, reference src/pose_clustering.cpp:79-121) and the kept hypotheses refined
(clustering::point_to_plane_icp, :123-140), per piece of the batch.

The contract: trial t's hypotheses are, bit for bit, what the host route gives on the same context -- stocs_cluster_poses (and the
oracle's greedy_clustering) on that trial's candidates with best_score = its best_lcp, then stocs_refine_poses on the kept
candidates' centred T16 right after the trial has been run alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
APP = os.path.join(ROOT, "model_matching_amd", "apps", "stocs_single")

SYMS = [(0, 0, 0), (0, 0, 180), (90, 0, 0), (0, 0, 360)]
# (sym, count, fraction) on the frames: every sym, count and fraction at least once (the whole product on the tiny workload; fraction 0
# with an unbounded count makes the host loop quadratic in the candidates of a frame, so the frames take it with bounded counts)
COMBOS = [(SYMS[0], 10, 0.8), (SYMS[1], 100000, 0.8), (SYMS[2], 1, 0.0), (SYMS[3], 0, 1.0), (SYMS[1], 10, 0.0), (SYMS[2], 100000, 0.8),
          (SYMS[3], 10, 0.8), (SYMS[0], 100000, 1.0)]
_CACHE = {}


def _workload(name):
    """(estimator, mode, n_attempts, max_per_base) of a workload, one context per module"""
    if name in _CACHE:
        return _CACHE[name]
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    mode, nA, mpb = 0, 100, 200
    if name in ("tiny", "Cm"):
        m, s, _ = synth.workload(name)
        est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
        if name == "tiny":
            nA, mpb = 40, 50
    else:
        d = np.load(os.path.join(GOLD, "example_%s.npz" % {"ycb": "ycb_024_bowl", "linemod": "linemod_obj_06", "packed": "packed_dove"}[name]))
        est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
        if "edge_map" in d.files:
            est.set_edge_map(d["edge_map"])
            mode, nA = 1, 24
    _CACHE[name] = (est, mode, nA, mpb)
    return _CACHE[name]


def _post(sym=(0, 0, 0), count=10, fraction=0.8, iters=0, dist=0.035):
    from model_matching_amd.estimator import trial_post
    return trial_post(acceptable_fraction=fraction, maximum_pose_count=count, min_distance=0.02, min_angle=15.0, sym3=sym, refine_iterations=iters,
                      max_correspondence_distance=dist)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name,n_trials", [("tiny", 16), ("ycb", 8), ("linemod", 8), ("packed", 8), ("Cm", 8)])
def test_clustering_equals_host_and_oracle(name, n_trials, oracle_lib):
    from model_matching_amd.estimator import cluster_poses
    est, mode, nA, mpb = _workload(name)
    seeds = list(range(100, 100 + n_trials))
    combos = [(s, c, f) for s in SYMS for c in (0, 1, 10, 100000) for f in (0.0, 0.8, 1.0)] if name == "tiny" else COMBOS
    kept_total = 0
    for sym, count, fraction in combos:
        res = est.run_trials(seeds, nA, mode=mode, max_per_base=mpb, keep_details=True, post=_post(sym, count, fraction))
        sym32 = np.array(sym, np.float32)
        for t in range(n_trials):
            T, P, l, b = est.trial_candidates(t)
            h = est.trials_get_hypotheses(t)
            ref = cluster_poses(P, l, fraction, res[t]["best_lcp"], count, 0.02, 15.0, sym32)
            orc = oracle_lib.greedy_clustering(P, l, fraction, res[t]["best_lcp"], count, 0.02, 15.0, sym32)
            key = (name, sym, count, fraction, t)
            assert h["candidate_index"].tolist() == ref.tolist() == list(orc), key
            if res[t]["best_index"] < 0:
                assert len(h) == 0, key
            if fraction == 1.0:
                assert len(h) == 0, key                        # lcp > best keeps nothing
            assert len(h) <= count + 1, key
            idx = h["candidate_index"]
            assert np.array_equal(h["base_index"], b[idx]) and np.array_equal(_bits(h["lcp"]), _bits(l[idx])), key
            assert np.array_equal(_bits(h["pose16"]), _bits(P[idx])), key
            # without refinement the refined fields are the candidate's
            assert np.array_equal(_bits(h["refined_pose16"]), _bits(P[idx])) and np.array_equal(_bits(h["refined_lcp"]), _bits(l[idx])), key
            assert not h["n_correspondences"].any() and not h["iterations"].any(), key
            kept_total += len(h)
    assert kept_total > 0


def _single_refined(est, seed, mode, nA, mpb, count, iters, dist):
    """the host route of one trial on the same context: run alone, host clustering, stocs_refine_poses on the kept centred T16"""
    from model_matching_amd.estimator import cluster_poses
    est.reset_trial()
    est.sample_bases(seed, nA, mode=mode, dispersion=0.9)
    est.find_congruent_all()
    est.make_transforms(mpb, seed)
    best_lcp, _, _ = est.compute_best_transform()
    T, P, l, b = est.get_pose_candidates()
    keep = cluster_poses(P, l, 0.8, best_lcp, count, 0.02, 15.0, np.zeros(3, np.float32))
    if len(keep) == 0:
        return keep, None
    return keep, est.refine_poses(T[keep], iters, dist)


@pytest.mark.parametrize("name", ["ycb", "Cm", "packed"])
def test_refinement_equals_the_host_route(name):
    est, mode, nA, mpb = _workload(name)
    seeds = [7, 8, 9, 10]
    res = est.run_trials(seeds, nA, mode=mode, max_per_base=mpb, post=_post(count=10, iters=5))
    hyps = [est.trials_get_hypotheses(t) for t in range(len(seeds))]
    n_ref = 0
    for t, seed in enumerate(seeds):
        keep, out = _single_refined(est, seed, mode, nA, mpb, 10, 5, 0.035)
        h = hyps[t]
        assert h["candidate_index"].tolist() == keep.tolist(), (name, t)
        if out is None:
            continue
        To, Po, lcp, nc, it = out
        assert np.array_equal(_bits(h["refined_pose16"]), _bits(Po)), (name, t)
        assert np.array_equal(_bits(h["refined_lcp"]), _bits(lcp)), (name, t)
        assert np.array_equal(h["n_correspondences"], nc) and np.array_equal(h["iterations"], it), (name, t)
        n_ref += int((it > 0).sum())
        assert res[t]["best_index"] >= 0
    assert n_ref > 0                                           # some hypotheses actually moved


def test_pieces_give_the_same_hypotheses(monkeypatch):
    est, mode, nA, mpb = _workload("tiny")
    seeds = [11, 12, 13, 14, 15]
    post = _post(count=10, fraction=0.5, iters=3)
    est.run_trials(seeds, nA, max_per_base=mpb, post=post)
    assert est.last_call_timing(3)[-1][1] == 1.0
    whole = [est.trials_get_hypotheses(t) for t in range(len(seeds))]
    assert sum(len(h) for h in whole) > len(seeds)
    for knob, value in (("STOCS_TRIALS_PER_PIECE", "2"), ("STOCS_TRIALS_MAX_MB", "1")):
        monkeypatch.setenv(knob, value)
        est.run_trials(seeds, nA, max_per_base=mpb, post=post)
        monkeypatch.delenv(knob)
        assert est.last_call_timing(3)[-1][1] >= 3.0, knob
        for t in range(len(seeds)):
            assert est.trials_get_hypotheses(t).tobytes() == whole[t].tobytes(), (knob, t)


def test_no_change_without_post_and_no_allocation():
    from model_matching_amd import capi
    est, mode, nA, mpb = _workload("tiny")
    L = capi.load()
    seeds = (C.c_uint64 * 6)(*[21, 22, 23, 24, 25, 26])
    a = (capi.TrialResult * 6)()
    b = (capi.TrialResult * 6)()
    capi.check(L.stocs_run_trials(est.h, 0, 6, seeds, nA, 0.9, mpb, 0, a))
    capi.check(L.stocs_run_trials_post(est.h, 0, 6, seeds, nA, 0.9, mpb, 0, None, b))
    assert bytes(a) == bytes(b)
    n = C.c_int(0)
    assert L.stocs_trials_get_hypotheses(est.h, 0, None, 0, C.byref(n)) == -5        # a batch without post has no hypotheses
    post = _post(count=10, fraction=0.5, iters=5)
    est.run_trials(list(seeds), nA, max_per_base=mpb, post=post)
    first = [est.trials_get_hypotheses(t).tobytes() for t in range(6)]
    a0 = L.stocs_device_alloc_count()
    est.run_trials(list(seeds), nA, max_per_base=mpb, post=post)
    assert L.stocs_device_alloc_count() == a0
    assert [est.trials_get_hypotheses(t).tobytes() for t in range(6)] == first
    # and the plain batch after it is still the plain batch
    c = (capi.TrialResult * 6)()
    capi.check(L.stocs_run_trials(est.h, 0, 6, seeds, nA, 0.9, mpb, 0, c))
    assert bytes(a) == bytes(c)


def test_errors():
    from model_matching_amd import capi
    est, mode, nA, mpb = _workload("tiny")
    L = capi.load()
    seeds = (C.c_uint64 * 2)(3, 4)
    bad = [dict(count=-1), dict(iters=-1), dict(fraction=float("nan")), dict(dist=0.0), dict(dist=-1.0), dict(dist=float("inf"))]
    for kw in bad:
        p = _post(**kw)
        assert L.stocs_run_trials_post(est.h, 0, 2, seeds, nA, 0.9, mpb, 0, C.byref(p), None) == capi.ERR_INVALID, kw
    for field, value in (("min_distance", 0.0), ("min_distance", -0.02), ("min_distance", float("nan")), ("min_angle", 0.0), ("min_angle", float("inf"))):
        p = _post()
        setattr(p, field, value)
        assert L.stocs_run_trials_post(est.h, 0, 2, seeds, nA, 0.9, mpb, 0, C.byref(p), None) == capi.ERR_INVALID, field
    # n_trials = 0: nothing to do, no trial to ask about
    p = _post()
    assert L.stocs_run_trials_post(est.h, 0, 0, seeds, nA, 0.9, mpb, 0, C.byref(p), None) == 0
    assert est.run_trials([], nA, post=_post()) == []
    n = C.c_int(0)
    assert L.stocs_trials_get_hypotheses(est.h, 0, None, 0, C.byref(n)) == -5
    # capacity: a short buffer is STOCS_ERR_CAPACITY with the count reported
    est.run_trials(list(range(30, 38)), nA, max_per_base=mpb, post=_post(count=100000, fraction=0.0))
    t = max(range(8), key=lambda k: len(est.trials_get_hypotheses(k)))
    full = est.trials_get_hypotheses(t)
    assert len(full) >= 2
    buf = (capi.TrialHypothesis * 1)()
    assert L.stocs_trials_get_hypotheses(est.h, t, buf, 1, C.byref(n)) == capi.ERR_CAPACITY and n.value == len(full)
    assert buf[0].candidate_index == full[0]["candidate_index"]
    assert L.stocs_trials_get_hypotheses(est.h, 8, buf, 1, C.byref(n)) == -5            # trial out of range
    assert L.stocs_trials_get_hypotheses(est.h, t, buf, 1, None) == capi.ERR_INVALID


def _driver_lines(stdout):
    return [ln for ln in stdout.splitlines() if not ln.startswith("|M|")]


def test_driver_trials_cluster_refine(tmp_path):
    from model_matching_amd import cloudio, synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, _ = synth.workload("tiny")
    cloudio.write_stcl(tmp_path / "scene.stcl", s.pos, s.nrm, s.prob, s.pixel)
    cloudio.write_stcl(tmp_path / "model.stcl", m.pos, m.nrm)
    seed = 5
    base = [APP, "--clouds", str(tmp_path / "scene.stcl"), str(tmp_path / "model.stcl"), "--seed", str(seed), "--trials", "4"]
    r0 = subprocess.run(base + ["--out", str(tmp_path / "a.txt")], capture_output=True, text=True, timeout=300)
    r1 = subprocess.run(base + ["--out", str(tmp_path / "b.txt"), "--cluster", "1", "--refine", "5"], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes()
    assert not (tmp_path / "a.txt.refined").exists() and (tmp_path / "b.txt.refined").exists()
    # without --cluster: the lines of today (trial lines, pose, summary); with it, the same plus the per-trial blocks
    timing = re.compile(r"total_microseconds=\d+")
    plain = [timing.sub("", ln) for ln in _driver_lines(r0.stdout)]
    post_lines = [timing.sub("", ln) for ln in _driver_lines(r1.stdout)]
    extra = re.compile(r"^(trial \d+ clustered hypotheses: \d+|  cluster \d+: .*|  refined \d+: .*|refined pose:.*)$")
    assert [ln for ln in post_lines if not extra.match(ln)] == plain
    assert not any(extra.match(ln) for ln in plain) and any(ln.startswith("trials: n=4") for ln in plain)
    # the Python hypotheses of the same batch
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    res = est.run_trials([seed + t for t in range(4)], 100, max_per_base=200, post=_post(count=10, fraction=0.8, iters=5))
    blocks = {}
    for ln in r1.stdout.splitlines():
        mt = re.match(r"^trial (\d+) clustered hypotheses: (\d+)$", ln)
        if mt:
            cur = int(mt.group(1)); blocks[cur] = dict(n=int(mt.group(2)), cluster=[], refined=[])
        mc = re.match(r"^  cluster (\d+): base (-?\d+) lcp (\S+)$", ln)
        if mc:
            blocks[cur]["cluster"].append((int(mc.group(2)), float(mc.group(3))))
        mr = re.match(r"^  refined (\d+): base (-?\d+) lcp (\S+) -> (\S+)$", ln)
        if mr:
            blocks[cur]["refined"].append((int(mr.group(2)), float(mr.group(4))))
    assert sorted(blocks) == [0, 1, 2, 3]
    total = 0
    for t in range(4):
        h = est.trials_get_hypotheses(t)
        assert blocks[t]["n"] == len(h) == len(blocks[t]["cluster"]) == len(blocks[t]["refined"]), t
        for k in range(len(h)):
            assert blocks[t]["cluster"][k][0] == h["base_index"][k] and abs(blocks[t]["cluster"][k][1] - h["lcp"][k]) <= 1e-5 * max(1.0, h["lcp"][k])
            assert blocks[t]["refined"][k][0] == h["base_index"][k] and abs(blocks[t]["refined"][k][1] - h["refined_lcp"][k]) <= 1e-5 * max(1.0, h["refined_lcp"][k])
        total += len(h)
    assert total > 0
    # .refined: the best trial's best refined hypothesis (first maximum), in the 3x4 row-major format
    best = max(range(4), key=lambda t: (res[t]["best_index"] >= 0, res[t]["best_lcp"], -t))
    h = est.trials_get_hypotheses(best)
    k = int(np.argmax(h["refined_lcp"]))
    want = h["refined_pose16"][k].reshape(4, 4).T[:3, :].reshape(12)
    got = np.array([ln for ln in r1.stdout.splitlines() if ln.startswith("refined pose:")][-1].split()[2:], np.float64).astype(np.float32)
    assert np.array_equal(got, want)
    assert np.allclose(np.array((tmp_path / "b.txt.refined").read_text().split(), np.float64), got, rtol=1e-5, atol=1e-6)
