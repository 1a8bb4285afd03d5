"""Batched point-to-plane refinement of pose hypotheses on the context (stocs_refine_poses): parity with the numpy restatement
oracle/ingest_oracle.py::icp applied per hypothesis (the reference's clustering::point_to_plane_icp, pose_clustering.cpp:123-140;
parity with PCL itself is unpinned), convergence, batch independence, rescoring, degenerate inputs, errors, state, driver."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
APP = os.path.join(ROOT, "model_matching_amd", "apps", "stocs_single")
ROT_TOL, TRANS_TOL, EDGE_TOL = 1e-5, 2e-5, 1e-6


def _est(scene_pos, scene_nrm, scene_prob, scene_pixel, model_pos, model_nrm, build_index=False):
    from model_matching_amd.estimator import StocsEstimator
    return StocsEstimator(scene_pos, scene_nrm, scene_prob, scene_pixel, model_pos, model_nrm, build_index=build_index)


def _unit(n):
    n = np.asarray(n, np.float32)
    z = n[:, 0] * n[:, 0] + (n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    return (n / np.sqrt(z)[:, None]).astype(np.float32)


def _target(est, model_pos, model_nrm):
    cm = est.get_model_centroid()
    return (np.asarray(model_pos, np.float32) - cm).astype(np.float32), _unit(model_nrm)


def _perturb(T16, k, seed, max_t, max_deg, exact=False):
    """k perturbations of one centred hypothesis (column-major 16) about the model origin: rotations up to max_deg about seeded
    axes, translations up to max_t (exactly those magnitudes with exact=True)."""
    from model_matching_amd.synth import _rot_axis_angle
    rng = np.random.default_rng(seed)
    T0 = np.asarray(T16, np.float64).reshape(4, 4).T
    out = np.zeros((k, 16), np.float32)
    for i in range(k):
        ang = math.radians(max_deg) * (1.0 if exact else rng.uniform(-1, 1))
        dR = _rot_axis_angle(rng.normal(size=3), ang)
        d = rng.normal(size=3)
        dt = d / np.linalg.norm(d) * (max_t if exact else rng.uniform(0, max_t))
        T = np.eye(4)
        T[:3, :3] = T0[:3, :3] @ dR
        T[:3, 3] = T0[:3, 3] + dt
        out[i] = T.T.reshape(16).astype(np.float32)
    return out


def _oracle(T16, scene_c, model_c, model_n, iters, dist, src_idx=None):
    """T_ref = T inv(U) with U from oracle icp on the centred scene moved into the model frame; also returns the source"""
    from oracle import ingest_oracle
    T = np.asarray(T16, np.float32).reshape(4, 4).T.astype(np.float64)
    x = scene_c if src_idx is None else scene_c[src_idx]
    Ti = np.linalg.inv(T)
    src = (Ti[:3, :3] @ x.T.astype(np.float64) + Ti[:3, 3:]).T
    U, nc = ingest_oracle.icp(src, model_c, model_n, iters, dist)
    return T @ np.linalg.inv(U), nc, src


def _edge_points(src, model_c, model_n, iters_done, max_iterations, dist):
    """points of the oracle's last evaluated iteration that lie within EDGE_TOL of the correspondence distance"""
    from oracle import ingest_oracle
    last = min(iters_done, max_iterations - 1)
    U, _ = ingest_oracle.icp(src, model_c, model_n, last, dist) if last > 0 else (np.eye(4), 0)
    s = np.asarray(src, np.float32).astype(np.float64) @ U[:3, :3].T + U[:3, 3]
    d, _ = cKDTree(model_c.astype(np.float64)).query(s)
    return int((np.abs(d - float(np.float32(dist))) <= EDGE_TOL).sum())


def _check_parity(est, hyps, scene_c, model_c, model_n, iters, dist, src_idx=None):
    To, Po, lcp, nc, it = est.refine_poses(hyps, iters, dist, src_idx=src_idx)
    for k in range(len(hyps)):
        T_ref, nc_ref, src = _oracle(hyps[k], scene_c, model_c, model_n, iters, dist, src_idx)
        G = To[k].reshape(4, 4).T.astype(np.float64)
        assert np.abs(G[:3, :3] - T_ref[:3, :3]).max() <= ROT_TOL, (k, np.abs(G[:3, :3] - T_ref[:3, :3]).max())
        assert np.abs(G[:3, 3] - T_ref[:3, 3]).max() <= TRANS_TOL, (k, np.abs(G[:3, 3] - T_ref[:3, 3]).max())
        if nc[k] != nc_ref:
            assert abs(int(nc[k]) - nc_ref) <= _edge_points(src, model_c, model_n, int(it[k]), iters, dist), (k, nc[k], nc_ref)
    return To, Po, lcp, nc, it


def _ycb():
    d = np.load(os.path.join(GOLD, "example_ycb_024_bowl.npz"), allow_pickle=False)
    return {k: d[k] for k in d.files}


def _clustered(est, seed):
    """a seeded trial's candidates and the clustered hypotheses of stocs_single --cluster 1 (0.8, best, 10, 2 cm, 15 deg)"""
    from model_matching_amd.estimator import cluster_poses
    est.sample_bases(seed, 100)
    est.find_congruent_all()
    est.make_transforms(200, seed)
    best_lcp, best_idx, _ = est.compute_best_transform()
    T, P, l, b = est.get_pose_candidates()
    keep = cluster_poses(P, l, 0.8, best_lcp, 10, 0.02, 15.0, np.zeros(3, np.float32))
    return T, P, l, best_lcp, best_idx, keep


@pytest.fixture(scope="module")
def ycb():
    d = _ycb()
    est = _est(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
    T, P, l, best_lcp, best_idx, keep = _clustered(est, 7)
    assert best_idx >= 0 and len(keep) >= 1
    hyps = np.concatenate([T[keep], _perturb(T[best_idx], 32, 11, 0.005, 4.0)])
    return d, est, hyps


def test_oracle_parity_on_ycb(ycb):
    d, est, hyps = ycb
    scene_c = est.get_scene()[0]
    model_c, model_n = _target(est, d["model_pos"], d["model_nrm"])
    To, Po, lcp, nc, it = _check_parity(est, hyps, scene_c, model_c, model_n, 5, 0.035)
    assert (it == 5).all() and (nc >= 6).all()
    # the camera form as stocs_get_candidates builds it: same linear part, tc = (t + c_scene) - R c_model
    cs, cm = est.get_scene_centroid(), est.get_model_centroid()
    for k in range(len(hyps)):
        G = To[k].reshape(4, 4).T
        Pc = Po[k].reshape(4, 4).T
        assert np.array_equal(G[:3, :3], Pc[:3, :3])
        assert np.abs(Pc[:3, 3] - (G[:3, 3] + cs - G[:3, :3].astype(np.float64) @ cm)).max() <= 1e-6


def test_parity_on_tiny_subset_two_distances():
    from model_matching_amd import synth
    m, s, _ = synth.workload("tiny")
    est = _est(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm)
    scene_c = est.get_scene()[0]
    model_c, model_n = _target(est, m.pos, m.nrm)
    Tgt = synth.centred_gt(s.T_gt, est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64))
    hyps = _perturb(Tgt.T.reshape(16), 12, 5, 0.006, 5.0)
    src_idx = np.sort(np.random.default_rng(3).choice(len(s.pos), len(s.pos) // 2, replace=False)).astype(np.int32)
    r1 = _check_parity(est, hyps, scene_c, model_c, model_n, 5, 0.01, src_idx)
    r2 = _check_parity(est, hyps, scene_c, model_c, model_n, 5, 0.035, src_idx)   # a different distance rebuilds the grid
    assert (r1[3] < r2[3]).any()
    r3 = est.refine_poses(hyps, 5, 0.01, src_idx=src_idx)                          # and back
    for a, b in zip(r1, r3):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n_model,scale", [(2000, 0.5), (5000, 1.0)])
def test_parity_on_dense_models(n_model, scale):
    """models with many points per 3.5 cm cell: the walk tests the octants of a cell one by one; the 2 000-point model is walked
    from LDS, the 5 000-point one from global memory"""
    from model_matching_amd import synth
    m = synth.make_model(n_model, seed=synth.SEED_MODEL + 3, scale=scale)
    s = synth.make_scene(m, 3000, seed=synth.SEED_SCENE + 3)
    est = _est(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm)
    scene_c = est.get_scene()[0]
    model_c, model_n = _target(est, m.pos, m.nrm)
    Tgt = synth.centred_gt(s.T_gt, est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64))
    _check_parity(est, _perturb(Tgt.T.reshape(16), 8, 13, 0.005, 4.0), scene_c, model_c, model_n, 5, 0.035)


def _convergence_errors():
    """16 starts 4 mm / 3 deg off the centred ground truth (seeded axes), refined on the object's own points of a synthetic scene
    whose model has no symmetry (every rotation observable): (translation mm, rotation deg) of each result against the truth"""
    from model_matching_amd import synth
    m = synth.make_model_asym(1000)
    s = synth.make_scene(m, 5000, seed=synth.SEED_SCENE + 31)
    est = _est(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm)
    Tgt = synth.centred_gt(s.T_gt, est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64))
    hyps = _perturb(Tgt.T.reshape(16), 16, 21, 0.004, 3.0, exact=True)
    To, Po, lcp, nc, it = est.refine_poses(hyps, 5, 0.035, src_idx=np.arange(s.n_object, dtype=np.int32))
    err = []
    for k in range(16):
        G = To[k].reshape(4, 4).T.astype(np.float64)
        dR = G[:3, :3].T @ Tgt[:3, :3]
        err.append((np.linalg.norm(G[:3, 3] - Tgt[:3, 3]) * 1e3, math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2))))))
    return np.array(err)


def test_convergence_on_known_pose():
    """Thresholds 1 mm / 0.5 deg are the first guess, kept after the first run: every start came to rest at 0.51 mm / 0.40 deg from
    the truth (the same fixed point for all 16: the scene's noise, not the starts, sets it).  Results are bitwise reproducible."""
    err = _convergence_errors()
    assert (err[:, 0] <= 1.0).all() and (err[:, 1] <= 0.5).all(), np.round(err, 4).tolist()


def test_batch_independence(ycb):
    d, est, hyps = ycb
    H = np.concatenate([hyps, _perturb(hyps[0], 64, 99, 0.005, 4.0)])[:64]
    whole = est.refine_poses(H)
    rev = est.refine_poses(H[::-1].copy())
    for k in range(64):
        alone = est.refine_poses(H[k:k + 1])
        for a, b, r in zip(whole, alone, rev):
            assert np.array_equal(a[k], b[0]) and np.array_equal(a[k], r[63 - k]), k


@pytest.mark.parametrize("exact", [0, 1])
def test_rescoring_is_score_transforms(ycb, exact):
    d, est, hyps = ycb
    est.set_option("exact_ties", exact)
    try:
        To, Po, lcp, nc, it = est.refine_poses(hyps)
        assert np.array_equal(lcp.view(np.uint32), est.score_transforms(To).view(np.uint32))
    finally:
        est.set_option("exact_ties", 0)


def test_degenerate_cases(ycb):
    d, est, hyps = ycb
    far = hyps[:2].copy()
    far[:, 12] += 5.0
    To, Po, lcp, nc, it = est.refine_poses(far)
    assert np.array_equal(To.view(np.uint32), far.view(np.uint32)) and (nc == 0).all() and (it == 0).all()
    To, Po, lcp, nc, it = est.refine_poses(hyps, max_iterations=0)
    assert np.array_equal(To.view(np.uint32), hyps.view(np.uint32)) and (it == 0).all() and (nc == 0).all()
    assert np.array_equal(lcp, est.score_transforms(hyps))
    To, Po, lcp, nc, it = est.refine_poses(np.zeros((0, 16), np.float32))
    assert To.shape == (0, 16) and lcp.shape == (0,)


def test_errors():
    from model_matching_amd import capi, synth
    L = capi.load()
    m, s, _ = synth.workload("tiny")
    est = _est(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm)
    T = np.eye(4, dtype=np.float32).reshape(1, 16)
    out = np.zeros((1, 16), np.float32)
    fp = lambda a: a.ctypes.data_as(capi._fp)
    ok_idx = np.arange(4, dtype=np.int32)

    def call(h=est.h, T16=T, n=1, idx=None, n_src=0, iters=5, dist=0.035):
        return L.stocs_refine_poses(h, None if T16 is None else fp(T16), n, None if idx is None else idx.ctypes.data_as(capi._ip), n_src, iters, dist,
                                    fp(out), None, None, None, None)

    assert call() == 0 and call(idx=ok_idx, n_src=4) == 0
    cases = [dict(h=None), dict(n=-1), dict(T16=None), dict(idx=ok_idx, n_src=-1), dict(iters=-1), dict(dist=0.0), dict(dist=-0.01),
             dict(dist=float("nan")), dict(dist=float("inf")), dict(idx=np.array([0, len(s.pos)], np.int32), n_src=2),
             dict(idx=np.array([-1], np.int32), n_src=1)]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert len(L.stocs_last_error()) > 0
    # a scene the grid refuses leaves the context scene-less: STATE
    bad = np.array([[0, 0, 0], [1000, 1000, 1000]], np.float32)
    with pytest.raises(capi.StocsError):
        est.set_scene(bad, np.array([[0, 0, 1], [0, 0, 1]], np.float32), np.ones(2, np.float32))
    assert call() == -5 and b"no scene" in L.stocs_last_error()


def test_state_no_allocation_and_new_scene():
    from model_matching_amd import capi, synth
    L = capi.load()
    m, s, _ = synth.workload("tiny")
    est = _est(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm)
    Tgt = synth.centred_gt(s.T_gt, est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64))
    hyps = _perturb(Tgt.T.reshape(16), 10, 8, 0.005, 4.0)
    est.refine_poses(hyps)
    a0 = L.stocs_device_alloc_count()
    est.refine_poses(hyps)
    est.refine_poses(hyps[:4], src_idx=np.arange(100, dtype=np.int32))
    assert L.stocs_device_alloc_count() == a0
    # another frame on the same context: the model grid stays, the source is the new scene
    s2 = synth.make_scene(m, 1200, seed=4242)
    est.set_scene(s2.pos, s2.nrm, s2.prob, s2.pixel)
    scene_c = est.get_scene()[0]
    model_c, model_n = _target(est, m.pos, m.nrm)
    Tgt2 = synth.centred_gt(s2.T_gt, est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64))
    _check_parity(est, _perturb(Tgt2.T.reshape(16), 8, 9, 0.005, 4.0), scene_c, model_c, model_n, 5, 0.035)


def _facade_centred(P16, cs, cm):
    """include/stocs.hpp refine_pose_candidates: camera -> centred, t = (t_camera - c_scene) + R c_model in double, rounded once"""
    T = np.array(P16, np.float32).copy()
    for r in range(3):
        R = [float(T[r]), float(T[4 + r]), float(T[8 + r])]
        T[12 + r] = np.float32((float(T[12 + r]) - float(cs[r])) + ((R[0] * float(cm[0]) + R[1] * float(cm[1])) + R[2] * float(cm[2])))
    return T


def test_driver_refine(tmp_path):
    from model_matching_amd import cloudio, synth
    m, s, _ = synth.workload("tiny")
    cloudio.write_stcl(tmp_path / "scene.stcl", s.pos, s.nrm, s.prob, s.pixel)
    cloudio.write_stcl(tmp_path / "model.stcl", m.pos, m.nrm)
    seed = 3
    base = [APP, "--clouds", str(tmp_path / "scene.stcl"), str(tmp_path / "model.stcl"), "--seed", str(seed), "--cluster", "1"]
    r0 = subprocess.run(base + ["--out", str(tmp_path / "a.txt")], capture_output=True, text=True, timeout=300)
    r1 = subprocess.run(base + ["--out", str(tmp_path / "b.txt"), "--refine", "5"], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes()
    assert not (tmp_path / "a.txt.refined").exists()
    assert "refined 0: base" in r1.stdout
    got = np.array([l for l in r1.stdout.splitlines() if l.startswith("refined pose:")][-1].split()[2:], np.float64).astype(np.float32)
    assert np.allclose(np.array((tmp_path / "b.txt.refined").read_text().split(), np.float64), got, rtol=1e-5, atol=1e-6)
    # the library's refinement of the same clustered hypotheses, through the façade's frame conversion
    est = _est(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    T, P, l, best_lcp, best_idx, keep = _clustered(est, seed)
    cs, cm = est.get_scene_centroid(), est.get_model_centroid()
    H = np.stack([_facade_centred(P[k], cs, cm) for k in keep])
    To, Po, lcp, nc, it = est.refine_poses(H, 5, 0.035)
    b = int(np.argmax(lcp))   # first maximum
    assert np.array_equal(Po[b].reshape(4, 4).T[:3, :].reshape(12), got)
