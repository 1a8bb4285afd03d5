"""The robust refinement as a whole (stocs_refine_poses_robust): bitwise the plain form with everything kept and the gate off, batch
independence and a workspace that does not move, parity with the float64 restatement tests/refine_robust_ref.py and the pose quality
it exists for, and the argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import refine_robust_cases as rc  # noqa: E402
import refine_robust_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
ROT_TOL, TRANS_TOL = 1e-5, 2e-5   # tests/test_refine_gpu.py's


def _workload(name):
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, _ = synth.workload(name)
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    Tgt = synth.centred_gt(s.T_gt, est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64))
    return m, s, est, Tgt


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_keep_everything_gate_off_is_the_plain_form_bitwise(name):
    from model_matching_amd import synth
    m, s, est, Tgt = _workload(name)
    H = synth.make_candidates(Tgt, 16, seed=synth.SEED_CAND + 17)
    plain = est.refine_poses(H, 5, 0.035)
    To, Po, lcp, nc, ncand, it = est.refine_poses_robust(H, 5, 0.035, keep_ratio=1.0, max_normal_deg=None)
    for a, b in zip(plain, (To, Po, lcp, nc, it)):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(ncand, nc) and (it > 0).any()
    est.close()


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_keep_everything_gate_on_against_the_restatement(name):
    """keep 1 with the 30 degree gate runs the accumulation's gate-on form: the six table hypotheses against the float64 restatement, all
    six (tests/test_refine_robust_cases_cpu.py: the restatement is clear for every one of them on both workloads)"""
    m, s, est, Tgt = _workload(name)
    H = rc.table_hypotheses(Tgt)
    scene_c, scene_n = est.get_scene()[0], est.get_scene()[1]
    model_c = (np.asarray(m.pos, F) - est.get_model_centroid()).astype(F)
    model_n = rr.unit_normals(m.nrm)
    To, Po, lcp, nc, ncand, it = est.refine_poses_robust(H, 5, 0.035, 1.0, 30.0)
    for k in range(len(H)):
        ref = rr.robust_loop(H[k], scene_c, scene_n, model_c, model_n, 5, 0.035, 1.0, rr.min_cos_of_degrees(30.0))
        G = To[k].reshape(4, 4).T.astype(np.float64)
        dr, dt = np.abs(G[:3, :3] - ref["T"][:3, :3]).max(), np.abs(G[:3, 3] - ref["T"][:3, 3]).max()
        print("GATE1 %s %d clear %s k %d/%d n_cand %d it %d/%d dR %.3g dt %.3g" % (name, k, ref["clear"], nc[k], ref["k"], ncand[k], it[k], ref["iterations"], dr, dt))
        assert nc[k] == ref["k"] and ncand[k] == nc[k] and it[k] == ref["iterations"], k
        assert dr <= ROT_TOL and dt <= TRANS_TOL, (k, dr, dt)
    est.close()


def test_the_index_list_of_every_point_is_no_index_list_and_a_subset_is_batch_independent():
    """tiny, 16 hypotheses, the plain and the robust (0.7, 30 degrees) entry point, which share one call frame and one driver:
    src_idx = 0 .. nS - 1 gives every output bitwise as the call without an index list, and on a 300-point subset a hypothesis refined
    alone gives bitwise what it gives in the batch"""
    from model_matching_amd import synth
    m, s, est, Tgt = _workload("tiny")
    H = np.concatenate([rc.table_hypotheses(Tgt, 8, seed=11), synth.make_candidates(Tgt, 8, seed=synth.SEED_CAND + 29)])
    every = np.arange(len(s.pos), dtype=np.int32)
    subset = np.sort(np.random.default_rng(7).choice(len(s.pos), 300, replace=False)).astype(np.int32)
    same = lambda a, b: a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for call in (lambda h, idx: est.refine_poses(h, 5, 0.035, src_idx=idx), lambda h, idx: est.refine_poses_robust(h, 5, 0.035, 0.7, 30.0, src_idx=idx)):
        whole = call(H, None)
        assert (whole[-1] > 0).any()
        assert all(same(a, b) for a, b in zip(whole, call(H, every)))
        batch = call(H, subset)
        assert (batch[-1] > 0).any() and not all(same(a, b) for a, b in zip(whole, batch))
        for k in range(len(H)):
            assert all(same(a[k:k + 1], b) for a, b in zip(batch, call(H[k:k + 1], subset))), k
    est.close()


def test_batch_independence_and_a_workspace_that_stays():
    from model_matching_amd import capi, synth
    L = capi.load()
    m, s, est, Tgt = _workload("tiny")
    H = np.concatenate([rc.table_hypotheses(Tgt, 16, seed=9), synth.make_candidates(Tgt, 48, seed=synth.SEED_CAND + 23)])
    whole = est.refine_poses_robust(H, 5, 0.035, 0.7, 30.0)
    ws, allocs = est.refine_robust_workspace(), L.stocs_device_alloc_count()
    assert ws[0] != 0 and ws[1] >= 64 * len(s.pos) * 8
    again = est.refine_poses_robust(H, 5, 0.035, 0.7, 30.0)
    assert est.refine_robust_workspace() == ws and L.stocs_device_alloc_count() == allocs
    rev = est.refine_poses_robust(H[::-1].copy(), 5, 0.035, 0.7, 30.0)
    assert (whole[5] == 5).any() and (whole[3] < whole[4]).any()
    for a, b in zip(whole, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for k in range(64):
        alone = est.refine_poses_robust(H[k:k + 1], 5, 0.035, 0.7, 30.0)
        for a, b, r in zip(whole, alone, rev):
            assert np.array_equal(a[k].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[k].view(np.uint32), r[63 - k].view(np.uint32)), k
    assert est.refine_robust_workspace() == ws and L.stocs_device_alloc_count() == allocs
    est.close()


def test_end_to_end_parity_and_quality_on_small():
    """The six hypotheses of DESIGN.md 7.11's table (2 degrees, 4 mm off the truth), 5 iterations, keep 0.7, gate 30 degrees.  Parity
    where the restatement is clear at every iteration (tests/test_refine_robust_cases_cpu.py: at least four of the six are); quality for
    all six: the robust form at least halves ADD, the plain form makes it worse."""
    m, s, est, Tgt = _workload("small")
    H = rc.table_hypotheses(Tgt)
    scene_c, scene_n = est.get_scene()[0], est.get_scene()[1]
    model_c = (np.asarray(m.pos, F) - est.get_model_centroid()).astype(F)
    model_n = rr.unit_normals(m.nrm)
    mcos = rr.min_cos_of_degrees(30.0)
    To, Po, lcp, nc, ncand, it = est.refine_poses_robust(H, 5, 0.035, 0.7, 30.0)
    held = 0
    for k in range(len(H)):
        ref = rr.robust_loop(H[k], scene_c, scene_n, model_c, model_n, 5, 0.035, rr.device_ratio(0.7), mcos)
        G = To[k].reshape(4, 4).T.astype(np.float64)
        dr, dt = np.abs(G[:3, :3] - ref["T"][:3, :3]).max(), np.abs(G[:3, 3] - ref["T"][:3, 3]).max()
        print("E2E %d clear %s k %d/%d n_cand %d/%d it %d/%d dR %.3g dt %.3g" % (k, ref["clear"], nc[k], ref["k"], ncand[k], ref["n_cand"], it[k], ref["iterations"], dr, dt))
        if ref["clear"]:
            held += 1
            assert nc[k] == ref["k"] and ncand[k] == ref["n_cand"] and it[k] == ref["iterations"], k
            assert dr <= ROT_TOL and dt <= TRANS_TOL, (k, dr, dt)
    assert held >= 4
    gt = np.asarray(s.T_gt, np.float64).T.reshape(16).astype(F)
    P0 = est.refine_poses_robust(H, 0)[1]                     # the camera form of the inputs
    Pp = est.refine_poses(H, 5, 0.035)[1]
    before, robust, plain = (est.pose_errors(P, gt)["add"].astype(np.float64) for P in (P0, Po, Pp))
    print("ADD mm before %s robust %s plain %s" % (np.round(before * 1e3, 3), np.round(robust * 1e3, 3), np.round(plain * 1e3, 3)))
    assert (robust < 0.5 * before).all()
    assert (plain > before).all()
    est.close()


def test_arguments():
    from model_matching_amd import capi
    L = capi.load()
    m, s, est, Tgt = _workload("tiny")
    T = Tgt.T.reshape(1, 16).astype(F)
    out = np.zeros((1, 16), F)
    fp = lambda a: a.ctypes.data_as(capi._fp)
    ok_idx = np.arange(4, dtype=np.int32)

    def prm(iters=5, dist=0.035, keep=0.7, mc=0.5):
        return capi.RefineRobustParams(iters, dist, keep, mc)

    def call(h=est.h, T16=T, n=1, idx=None, n_src=0, p=prm()):
        return L.stocs_refine_poses_robust(h, None if T16 is None else fp(T16), n, None if idx is None else idx.ctypes.data_as(capi._ip), n_src,
                                           None if p is None else C.byref(p), fp(out), None, None, None, None, None)

    def detail(p, T16=T):
        n = len(s.pos)
        a = np.zeros(n, np.int32); b = np.zeros(n, np.uint8); c = np.zeros(n, np.uint8); r = np.zeros(n, np.uint32)
        return L.stocs_refine_robust_detail(est.h, None if T16 is None else fp(T16), None, 0, None if p is None else C.byref(p), a.ctypes.data_as(capi._ip),
                                            b.ctypes.data_as(capi._u8p), c.ctypes.data_as(capi._u8p), r.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, None)

    assert call() == 0 and call(idx=ok_idx, n_src=4) == 0 and detail(prm()) == 0
    for good in (prm(keep=1.0), prm(mc=1.0), prm(mc=-1.0), prm(mc=-2.0), prm(mc=float("-inf")), prm(keep=1e-6)):
        assert call(p=good) == 0, (good.keep_ratio, good.min_normal_cos)
    nan, inf = float("nan"), float("inf")
    bad_params = [None, prm(keep=0.0), prm(keep=-0.1), prm(keep=1.0000001), prm(keep=nan), prm(keep=inf), prm(mc=1.0000001), prm(mc=nan), prm(mc=inf),
                  prm(iters=-1), prm(dist=0.0), prm(dist=-0.01), prm(dist=nan), prm(dist=inf)]
    for p in bad_params:
        for rc_ in (call(p=p), detail(p)):
            assert rc_ == capi.ERR_INVALID, (None if p is None else (p.max_iterations, p.max_correspondence_distance, p.keep_ratio, p.min_normal_cos))
            assert len(L.stocs_last_error()) > 0
    for kw in (dict(h=None), dict(n=-1), dict(T16=None), dict(idx=ok_idx, n_src=-1), dict(idx=np.array([0, len(s.pos)], np.int32), n_src=2),
               dict(idx=np.array([-1], np.int32), n_src=1)):
        assert call(**kw) == capi.ERR_INVALID, kw
        assert len(L.stocs_last_error()) > 0
    assert detail(prm(), T16=None) == capi.ERR_INVALID
    # the workspace demand n * n_src * 8 against the header's limit, just below and just above
    limit = 1 << 30
    n_over = limit // (len(s.pos) * 8) + 1
    big = np.tile(T, (n_over, 1))
    big_out = np.zeros((n_over, 16), F)
    assert L.stocs_refine_poses_robust(est.h, fp(big), n_over, None, 0, C.byref(prm()), fp(big_out), None, None, None, None, None) == capi.ERR_INVALID
    assert b"limit" in L.stocs_last_error()
    # n == 0: a no-op; max_iterations == 0: the inputs, scored
    assert call(n=0) == 0
    To, Po, lcp, nc, ncand, it = est.refine_poses_robust(np.zeros((0, 16), F))
    assert To.shape == (0, 16) and lcp.shape == (0,)
    H = rc.table_hypotheses(Tgt, 5, seed=3)
    To, Po, lcp, nc, ncand, it = est.refine_poses_robust(H, 0)
    assert np.array_equal(To.view(np.uint32), H.view(np.uint32)) and not nc.any() and not ncand.any() and not it.any()
    assert np.array_equal(lcp.view(np.uint32), est.score_transforms(H).view(np.uint32))
    est.close()


def _facade_centred(P16, cs, cm):
    """include/stocs.hpp refine_pose_candidates_robust: camera -> centred, t = (t_camera - c_scene) + R c_model in double, rounded once"""
    T = np.array(P16, F).copy()
    for r in range(3):
        R = [float(T[r]), float(T[4 + r]), float(T[8 + r])]
        T[12 + r] = F((float(T[12 + r]) - float(cs[r])) + ((R[0] * float(cm[0]) + R[1] * float(cm[1])) + R[2] * float(cm[2])))
    return T


def test_driver_trim_and_normal_gate(tmp_path):
    import subprocess
    from model_matching_amd import cloudio, synth
    from model_matching_amd.estimator import StocsEstimator, cluster_poses
    app = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "model_matching_amd", "apps", "stocs_single")
    m, s, _ = synth.workload("tiny")
    cloudio.write_stcl(tmp_path / "scene.stcl", s.pos, s.nrm, s.prob, s.pixel)
    cloudio.write_stcl(tmp_path / "model.stcl", m.pos, m.nrm)
    seed = 3
    base = [app, "--clouds", str(tmp_path / "scene.stcl"), str(tmp_path / "model.stcl"), "--seed", str(seed), "--cluster", "1", "--refine", "5"]
    run = lambda tag, extra: subprocess.run(base + ["--out", str(tmp_path / (tag + ".txt"))] + extra, capture_output=True, text=True, timeout=300)
    refined = lambda r: [l for l in r.stdout.splitlines() if l.startswith("refined pose:")][-1]
    plain, all_kept, robust = run("a", []), run("b", ["--trim", "1"]), run("c", ["--trim", "0.7", "--normal-gate", "30"])
    assert plain.returncode == 0 and all_kept.returncode == 0 and robust.returncode == 0, plain.stderr + all_kept.stderr + robust.stderr
    # everything kept, no gate: the plain form's results, byte for byte (the lines that carry no clock reading)
    results = lambda r: [l for l in r.stdout.splitlines() if l.startswith(("pose:", "clustered", "  cluster", "  refined", "refined pose:"))]
    assert results(all_kept) == results(plain) and len(results(plain)) >= 5
    assert (tmp_path / "a.txt.refined").read_bytes() == (tmp_path / "b.txt.refined").read_bytes()
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "c.txt").read_bytes()          # the search itself is untouched
    # the library's robust refinement of the same clustered hypotheses, through the façade's frame conversion and its float cosine
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    est.sample_bases(seed, 100)
    est.find_congruent_all()
    est.make_transforms(200, seed)
    best_lcp, best_idx, _ = est.compute_best_transform()
    T, P, l, b = est.get_pose_candidates()
    keep = cluster_poses(P, l, 0.8, best_lcp, 10, 0.02, 15.0, np.zeros(3, F))
    cs, cm = est.get_scene_centroid(), est.get_model_centroid()
    H = np.stack([_facade_centred(P[k], cs, cm) for k in keep])
    To, Po, lcp, nc, ncand, it = est.refine_poses_robust(H, 5, 0.035, 0.7, 30.0)
    got = np.array(refined(robust).split()[2:], np.float64).astype(F)
    best = int(np.argmax(lcp))
    assert np.array_equal(Po[best].reshape(4, 4).T[:3, :].reshape(12), got)
    est.close()
    for bad in (["--trim", "0"], ["--trim", "1.5"], ["--normal-gate", "30"], ["--trim", "0.7", "--normal-gate", "-1"], ["--trim", "0.7", "--trials", "4"]):
        r = run("d", bad)
        assert r.returncode != 0 and "--trim" in r.stderr, bad
