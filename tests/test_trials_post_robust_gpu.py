"""The robust refinement inside trial batches (stocs_run_trials_post_robust): trial t's hypotheses are, bit for bit, what the host
route gives on the same context -- the trial run alone, stocs_cluster_poses, then stocs_refine_poses_robust on the kept candidates'
centred T16; with everything kept and the gate off the batch is stocs_run_trials_post's, byte for byte; dead slots and frozen
hypotheses; pieces and groups change no byte; a repeated call allocates nothing; the argument checks; the driver's --robust."""
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
ROBUST = dict(keep_ratio=0.7, max_normal_deg=30.0)
ALL_KEPT = dict(keep_ratio=1.0, max_normal_deg=None)
_CACHE = {}


def _workload(name):
    """(estimator, mode, n_attempts, max_per_base) of a workload, one context per module (tests/test_trials_post_gpu.py's)"""
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
        d = np.load(os.path.join(GOLD, "example_%s.npz" % {"ycb": "ycb_024_bowl", "packed": "packed_dove"}[name]))
        est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
        if "edge_map" in d.files:
            est.set_edge_map(d["edge_map"])
            mode, nA = 1, 24
    _CACHE[name] = (est, mode, nA, mpb)
    return _CACHE[name]


def _post(count=10, fraction=0.8, iters=0, dist=0.035):
    from model_matching_amd.estimator import trial_post
    return trial_post(acceptable_fraction=fraction, maximum_pose_count=count, min_distance=0.02, min_angle=15.0, sym3=(0, 0, 0), refine_iterations=iters,
                      max_correspondence_distance=dist)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _groups(est):
    """the groups the last robust batch refined its slots in (stocs_last_call_timing, next to the pieces)"""
    rows = [v for k, v in est.last_call_timing(3) if k.startswith("robust refinement: groups")]
    assert len(rows) == 1
    return int(rows[0])


def _single_refined(est, seed, mode, nA, mpb, count, iters, dist):
    """the host route of one trial on the same context: run alone, host clustering, stocs_refine_poses_robust on the kept centred T16"""
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
    return keep, est.refine_poses_robust(T[keep], iters, dist, **ROBUST)


@pytest.mark.parametrize("name", ["ycb", "Cm", "packed"])
def test_refinement_equals_the_host_route(name):
    est, mode, nA, mpb = _workload(name)
    seeds = [7, 8, 9, 10]
    res = est.run_trials(seeds, nA, mode=mode, max_per_base=mpb, post=_post(count=10, iters=5), robust=ROBUST)
    hyps = [est.trials_get_hypotheses(t) for t in range(len(seeds))]
    n_moved = 0
    for t, seed in enumerate(seeds):
        keep, out = _single_refined(est, seed, mode, nA, mpb, 10, 5, 0.035)
        h = hyps[t]
        assert h["candidate_index"].tolist() == keep.tolist(), (name, t)
        if out is None:
            continue
        To, Po, lcp, nc, ncand, it = out
        assert np.array_equal(_bits(h["refined_pose16"]), _bits(Po)), (name, t)
        assert np.array_equal(_bits(h["refined_lcp"]), _bits(lcp)), (name, t)
        assert np.array_equal(h["n_correspondences"], nc) and np.array_equal(h["iterations"], it), (name, t)
        assert (nc <= ncand).all()                                # n_correspondences is k, the kept share of the candidates
        n_moved += int((it > 0).sum())
        assert res[t]["best_index"] >= 0
    assert n_moved > 0                                             # some hypotheses actually moved


def test_everything_kept_gate_off_is_the_plain_batch_byte_for_byte():
    est, mode, nA, mpb = _workload("tiny")
    seeds = [11, 12, 13, 14, 15]
    post = _post(count=10, fraction=0.5, iters=5)
    plain_res = est.run_trials(seeds, nA, max_per_base=mpb, post=post)
    plain = [est.trials_get_hypotheses(t).tobytes() for t in range(len(seeds))]
    rob_res = est.run_trials(seeds, nA, max_per_base=mpb, post=post, robust=ALL_KEPT)
    rob = [est.trials_get_hypotheses(t) for t in range(len(seeds))]
    assert [h.tobytes() for h in rob] == plain
    assert sum(int((h["iterations"] > 0).sum()) for h in rob) > 0
    for a, b in zip(plain_res, rob_res):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    # the result records themselves, through the C entry points
    from model_matching_amd import capi
    L = capi.load()
    sd = (C.c_uint64 * 5)(*seeds)
    a = (capi.TrialResult * 5)(); b = (capi.TrialResult * 5)()
    capi.check(L.stocs_run_trials_post(est.h, 0, 5, sd, nA, 0.9, mpb, 0, C.byref(post), a))
    capi.check(L.stocs_run_trials_post_robust(est.h, 0, 5, sd, nA, 0.9, mpb, 0, C.byref(post), 1.0, -2.0, b))
    assert bytes(a) == bytes(b)


def test_dead_slots_and_freezes():
    est, mode, nA, mpb = _workload("tiny")
    seeds = [11, 12, 13, 14, 15]
    run = lambda post, robust=ROBUST, s=seeds, **kw: est.run_trials(s, nA, max_per_base=mpb, post=post, robust=robust, **kw)
    # fraction 1: lcp > best keeps nothing -- every slot of every trial is dead
    res = run(_post(count=10, fraction=1.0, iters=5))
    assert all(len(est.trials_get_hypotheses(t)) == 0 for t in range(len(seeds))) and any(r["best_index"] >= 0 for r in res)
    assert [r["best_lcp"] for r in res] == [r["best_lcp"] for r in est.run_trials(seeds, nA, max_per_base=mpb)]
    # count 0: one slot per trial; the live ones equal the plain call's clustering and the stand-alone robust refinement
    run(_post(count=0, fraction=0.5, iters=5), keep_details=True)
    one = [est.trials_get_hypotheses(t) for t in range(len(seeds))]
    cands = [est.trial_candidates(t) for t in range(len(seeds))]
    assert all(len(h) <= 1 for h in one) and sum(len(h) for h in one) > 0
    for t, h in enumerate(one):
        if len(h):
            To, Po, lcp, nc, ncand, it = est.refine_poses_robust(cands[t][0][h["candidate_index"]], 5, 0.035, **ROBUST)
            assert np.array_equal(_bits(h["refined_pose16"]), _bits(Po)) and np.array_equal(_bits(h["refined_lcp"]), _bits(lcp)), t
            assert np.array_equal(h["n_correspondences"], nc) and np.array_equal(h["iterations"], it), t
    # trials that find no pose (no attempt: no base, no candidate, no slot)
    res = est.run_trials(seeds, 0, max_per_base=mpb, post=_post(iters=5), robust=ROBUST)
    assert all(r["best_index"] < 0 for r in res) and all(len(est.trials_get_hypotheses(t)) == 0 for t in range(len(seeds)))
    # keep_ratio 1e-6: k = 0 at the first evaluation, frozen at once -- the refined fields are the inputs as scored (the lcp of the
    # candidate, its camera pose as the refinement forms it from the unchanged centred T16: stocs_refine_poses_robust with 0 iterations), counts 0
    run(_post(count=10, fraction=0.5, iters=5), robust=dict(keep_ratio=1e-6, max_normal_deg=30.0), keep_details=True)
    frozen = [est.trials_get_hypotheses(t) for t in range(len(seeds))]
    cands = [est.trial_candidates(t) for t in range(len(seeds))]
    assert sum(len(h) for h in frozen) > len(seeds)
    for t, h in enumerate(frozen):
        assert np.array_equal(_bits(h["refined_lcp"]), _bits(h["lcp"])), t
        assert not h["n_correspondences"].any() and not h["iterations"].any(), t
        if len(h):
            To, Po, lcp, nc, ncand, it = est.refine_poses_robust(cands[t][0][h["candidate_index"]], 0)
            assert np.array_equal(_bits(h["refined_pose16"]), _bits(Po)) and np.array_equal(_bits(h["refined_lcp"]), _bits(lcp)), t
            assert np.abs(h["refined_pose16"] - h["pose16"]).max() <= 1e-6, t


def test_pieces_and_groups_give_the_same_hypotheses(monkeypatch):
    est, mode, nA, mpb = _workload("tiny")
    seeds = [11, 12, 13, 14, 15]
    post = _post(count=10, fraction=0.5, iters=3)
    est.run_trials(seeds, nA, max_per_base=mpb, post=post, robust=ROBUST)
    assert est.last_call_timing(3)[-1][1] == 1.0 and _groups(est) == 1
    whole = [est.trials_get_hypotheses(t) for t in range(len(seeds))]
    n_hyp = sum(len(h) for h in whole)
    assert n_hyp > len(seeds) and sum(int((h["iterations"] > 0).sum()) for h in whole) > 0
    res = est.run_trials(seeds, nA, max_per_base=mpb)
    slots = [min(11, r["n_candidates"]) for r in res]              # min(count + 1, candidates) per trial
    offs = set(np.cumsum([0] + slots).tolist())
    assert any(b not in offs for b in range(0, sum(slots), 3)) and sum(slots) % 3 != 0   # a three-slot boundary inside a trial, a partial last group
    slot = est.nS * 8                                              # one slot's workspace demand
    settings = [({"STOCS_TRIALS_PER_PIECE": "2"}, 3, 3), ({"STOCS_REFINE_ROBUST_GROUP_BYTES": str(slot)}, 1, None),
                ({"STOCS_REFINE_ROBUST_GROUP_BYTES": str(3 * slot)}, 1, None),
                ({"STOCS_TRIALS_PER_PIECE": "2", "STOCS_REFINE_ROBUST_GROUP_BYTES": str(3 * slot)}, 3, None)]
    for env, pieces, groups in settings:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        est.run_trials(seeds, nA, max_per_base=mpb, post=post, robust=ROBUST)
        for k in env:
            monkeypatch.delenv(k)
        assert est.last_call_timing(3)[-1][1] == float(pieces), env
        g = _groups(est)
        if groups is not None:
            assert 1 <= g <= groups, env                           # at most one group per piece without the knob
        else:
            assert g > pieces and g >= n_hyp // (int(env["STOCS_REFINE_ROBUST_GROUP_BYTES"]) // slot), env   # (the slots bound the hypotheses)
        for t in range(len(seeds)):
            assert est.trials_get_hypotheses(t).tobytes() == whole[t].tobytes(), (env, t)


def test_repeated_call_allocates_nothing():
    from model_matching_amd import capi
    est, mode, nA, mpb = _workload("tiny")
    L = capi.load()
    seeds = [21, 22, 23, 24, 25, 26]
    post = _post(count=10, fraction=0.5, iters=5)
    est.run_trials(seeds, nA, max_per_base=mpb, post=post, robust=ROBUST)
    first = [est.trials_get_hypotheses(t).tobytes() for t in range(6)]
    ws, allocs = est.refine_robust_workspace(), L.stocs_device_alloc_count()
    assert ws[0] != 0 and ws[1] > 0
    est.run_trials(seeds, nA, max_per_base=mpb, post=post, robust=ROBUST)
    assert est.refine_robust_workspace() == ws and L.stocs_device_alloc_count() == allocs
    assert [est.trials_get_hypotheses(t).tobytes() for t in range(6)] == first
    # the plain batch after it is still the plain batch
    est.run_trials(seeds, nA, max_per_base=mpb, post=post)
    plain = [est.trials_get_hypotheses(t).tobytes() for t in range(6)]
    est.run_trials(seeds, nA, max_per_base=mpb, post=post, robust=ALL_KEPT)
    assert [est.trials_get_hypotheses(t).tobytes() for t in range(6)] == plain and plain != first


def test_errors():
    from model_matching_amd import capi
    est, mode, nA, mpb = _workload("tiny")
    L = capi.load()
    seeds = (C.c_uint64 * 2)(3, 4)
    good = _post(iters=5)

    def call(post=good, keep=0.7, mc=0.5, h=est.h, n=2, sd=seeds, mode=0, mpb_=mpb):
        return L.stocs_run_trials_post_robust(h, mode, n, sd, nA, 0.9, mpb_, 0, None if post is None else C.byref(post), keep, mc, None)

    assert call() == 0
    assert call(post=None) == capi.ERR_INVALID and b"post" in L.stocs_last_error()
    for keep, mc in ((1.0, 0.5), (0.7, 1.0), (0.7, -1.0), (0.7, -2.0), (0.7, float("-inf")), (1e-6, 0.5)):
        assert call(keep=keep, mc=mc) == 0, (keep, mc)
    nan, inf = float("nan"), float("inf")
    # tests/test_refine_robust_gpu.py's list of invalid settings
    for keep, mc in ((0.0, 0.5), (-0.1, 0.5), (1.0000001, 0.5), (nan, 0.5), (inf, 0.5), (0.7, 1.0000001), (0.7, nan), (0.7, inf)):
        assert call(keep=keep, mc=mc) == capi.ERR_INVALID, (keep, mc)
        assert len(L.stocs_last_error()) > 0
    # the plain entry point's own errors, unchanged
    for kw in (dict(count=-1), dict(iters=-1), dict(fraction=nan), dict(dist=0.0), dict(dist=-1.0), dict(dist=inf)):
        assert call(post=_post(**kw)) == capi.ERR_INVALID, kw
    for field, value in (("min_distance", 0.0), ("min_distance", nan), ("min_angle", 0.0), ("min_angle", inf)):
        p = _post()
        setattr(p, field, value)
        assert call(post=p) == capi.ERR_INVALID, field
    for kw in (dict(h=None), dict(n=-1), dict(sd=None), dict(mode=2), dict(mpb_=0)):
        assert call(**kw) == capi.ERR_INVALID, kw
    assert call(n=0) == 0
    assert est.run_trials([], nA, post=_post(iters=5), robust=ROBUST) == []
    n = C.c_int(0)
    assert L.stocs_trials_get_hypotheses(est.h, 0, None, 0, C.byref(n)) == -5


def _driver_lines(stdout):
    return [ln for ln in stdout.splitlines() if not ln.startswith("|M|")]


def _blocks(stdout):
    """trial -> [(base index, refined lcp)] of the driver's per-trial "refined" lines"""
    blocks, cur = {}, None
    for ln in stdout.splitlines():
        mt = re.match(r"^trial (\d+) clustered hypotheses: (\d+)$", ln)
        if mt:
            cur = int(mt.group(1)); blocks[cur] = []
        mr = re.match(r"^  refined (\d+): base (-?\d+) lcp (\S+) -> (\S+)$", ln)
        if mr:
            blocks[cur].append((int(mr.group(2)), float(mr.group(4))))
    return blocks


def _refined_pose(stdout):
    return np.array([ln for ln in stdout.splitlines() if ln.startswith("refined pose:")][-1].split()[2:], np.float64).astype(np.float32)


def test_driver_robust(tmp_path):
    from model_matching_amd import cloudio, synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, _ = synth.workload("tiny")
    cloudio.write_stcl(tmp_path / "scene.stcl", s.pos, s.nrm, s.prob, s.pixel)
    cloudio.write_stcl(tmp_path / "model.stcl", m.pos, m.nrm)
    seed = 5
    base = [APP, "--clouds", str(tmp_path / "scene.stcl"), str(tmp_path / "model.stcl"), "--seed", str(seed)]
    batch = ["--trials", "4", "--cluster", "1", "--refine", "5"]
    run = lambda tag, extra: subprocess.run(base + ["--out", str(tmp_path / (tag + ".txt"))] + extra, capture_output=True, text=True, timeout=300)
    timing = re.compile(r"(total_microseconds|track_microseconds)=\d+")
    lines = lambda r: [timing.sub("", ln) for ln in _driver_lines(r.stdout)]
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    res = est.run_trials([seed + t for t in range(4)], 100, max_per_base=200, post=_post(count=10, fraction=0.8, iters=5), robust=ROBUST)
    hyps = [est.trials_get_hypotheses(t) for t in range(4)]
    best = max(range(4), key=lambda t: (res[t]["best_index"] >= 0, res[t]["best_lcp"], -t))
    want_pose = hyps[best]["refined_pose16"][int(np.argmax(hyps[best]["refined_lcp"]))].reshape(4, 4).T[:3, :].reshape(12)
    est.close()
    assert sum(int((h["iterations"] > 0).sum()) for h in hyps) > 0
    # a prior 30 cm behind the object: the tracked lcp stays below the threshold and the run falls back to the detection, which refines
    far = np.asarray(s.T_gt, np.float64)[:3, :].copy()
    far[2, 3] += 0.30
    (tmp_path / "prior.txt").write_text(" ".join("%.9g" % x for x in far.ravel()) + "\n")
    track = ["--track", str(tmp_path / "prior.txt")]
    for tag, front in (("b", []), ("t", track)):
        plain, kept, robust = run(tag + "0", front + batch), run(tag + "1", front + batch + ["--robust", "1"]), run(tag + "2", front + batch + ["--robust", "0.7,30"])
        assert plain.returncode == 0 and kept.returncode == 0 and robust.returncode == 0, plain.stderr + kept.stderr + robust.stderr
        if front:
            assert any(ln.startswith("track: route=detection") for ln in robust.stdout.splitlines())
        # --robust 1: what the command prints without it
        assert lines(kept) == lines(plain) and any(ln.startswith("refined pose:") for ln in lines(plain))
        assert (tmp_path / (tag + "0.txt.refined")).read_bytes() == (tmp_path / (tag + "1.txt.refined")).read_bytes()
        # --robust 0.7,30: the library's refined hypotheses for the same seeds
        blocks = _blocks(robust.stdout)
        assert sorted(blocks) == [0, 1, 2, 3]
        for t in range(4):
            h = hyps[t]
            assert len(blocks[t]) == len(h), (tag, t)
            for k in range(len(h)):
                assert blocks[t][k][0] == h["base_index"][k] and abs(blocks[t][k][1] - h["refined_lcp"][k]) <= 1e-5 * max(1.0, h["refined_lcp"][k]), (tag, t, k)
        assert np.array_equal(_refined_pose(robust.stdout), want_pose), tag
        assert (tmp_path / (tag + "0.txt")).read_bytes() == (tmp_path / (tag + "2.txt")).read_bytes()      # the search itself is untouched
    for bad in (batch + ["--robust", "0"], batch + ["--robust", "1.5"], batch + ["--robust", "0.7,-1"], ["--trials", "4", "--cluster", "1", "--robust", "0.7,30"],
                ["--trials", "4", "--robust", "0.7"], track + ["--robust", "0.7,30"]):
        r = run("d", bad)
        assert r.returncode != 0 and "--robust" in r.stderr, bad
