"""The normal-cone gate of the queue kernel (stocs_set_option "lcp_normal_gate", csrc/normal_cone.h): a query whose cell's cone of
scene normals cannot pass the 30-degree test never joins the queue.  A dropped query is one the ungated kernel would not count, and
scores are integer sums, so every score must be the same BITWISE with the gate on, with it off, and from the plain kernel
(lcp_variant 0) -- on the synthetic workloads in every form the option reaches, and on hand-built scenes made to break it.
stocs_lcp_gate_count runs the kernel's own gate function over every query and reports how many it rules out and how many of those
the per-point detail form counts: never one."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DOT_LO = np.float32(np.cos(np.deg2rad(30.0)))


def _estimator(spos, snrm, mpos, mnrm, prob=None, **prm):
    from model_matching_amd import capi
    from model_matching_amd.estimator import StocsEstimator
    prob = np.full(len(spos), 0.5, np.float32) if prob is None else prob
    params = capi.default_params(**prm) if prm else None
    return StocsEstimator(spos.astype(np.float32), snrm.astype(np.float32), prob, np.zeros((len(spos), 2), np.int32), mpos.astype(np.float32),
                          mnrm.astype(np.float32), params=params, build_index=False)


def _workload(name, scale=1.0, **prm):
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    from model_matching_amd import capi
    m, s, k = synth.workload(name)
    est = StocsEstimator(s.pos * np.float32(scale), s.nrm, s.prob, s.pixel, m.pos * np.float32(scale), m.nrm,
                         params=capi.default_params(**prm) if prm else None, build_index=False)
    cs = est.get_scene_centroid().astype(np.float64); cm = est.get_model_centroid().astype(np.float64)
    Tgt = synth.centred_gt(s.T_gt, cs / scale, cm / scale)
    T = synth.make_candidates(Tgt, min(k, 1024))
    T[:, 12:15] *= np.float32(scale)
    return est, T


def _odd(near, rng):
    """matrices the gate's bound has to hold for: scaled by 2 and by less than 1, sheared, mirrored, with NaN and infinite entries"""
    odd = near[:48].reshape(48, 4, 4).copy()
    for i in range(48):
        A = odd[i, :3, :3].T.astype(np.float64)
        kind = i % 4
        if kind == 0: A = A * 2.0
        elif kind == 1: A = A @ (np.eye(3) + rng.uniform(-0.6, 0.6, (3, 3)))
        elif kind == 2: A = A @ np.diag([1.0, -1.0, 1.0])
        else: A = A * rng.uniform(0.3, 0.95)
        odd[i, :3, :3] = A.T.astype(np.float32)
    bad = near[:8].copy()
    bad[0, 0] = np.nan; bad[1, 5] = np.nan; bad[2, 10] = np.inf; bad[3, 9] = -np.inf; bad[4, 12] = np.nan; bad[5, :] = 0.0; bad[6, 0:3] = 3e38; bad[7, 8:11] = np.nan
    return np.concatenate([odd.reshape(48, 16), bad])


def _three_ways(est, T):
    """scores with the gate off, on, and from the plain kernel; asserts they are bitwise equal and returns them"""
    est.set_option("lcp_variant", 99)
    est.set_option("lcp_normal_gate", 0); off = est.score_transforms(T)
    est.set_option("lcp_normal_gate", 1); on = est.score_transforms(T)
    est.set_option("lcp_variant", 0); plain = est.score_transforms(T)
    est.set_option("lcp_variant", 99)
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
    assert np.array_equal(on.view(np.uint32), plain.view(np.uint32))
    return on


def _gate_count(est, T):
    dT = est.dev_alloc(T.nbytes)
    est.dev_upload(dT, T)
    out = est.lcp_gate_count(dT, len(T))
    est.dev_free(dT)
    return out


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_gate_bitwise_equal_in_every_form(name):
    est, near = _workload(name)
    T = np.concatenate([near, _odd(near, np.random.default_rng(5))])
    base = None
    for split in (1, 0):
        for flat in (1, 0):
            for cull, unit in ((2, 16), (2, 64), (0, 64)):
                est.set_option("lcp_split", split); est.set_option("lcp_flat", flat); est.set_option("lcp_cull", cull); est.set_option("lcp_cull_unit", unit)
                s = _three_ways(est, T)
                base = s if base is None else base
                assert np.array_equal(s.view(np.uint32), base.view(np.uint32)), (split, flat, cull, unit)
    assert base[: len(near)].max() > 0.05
    q, ruled, wrong = _gate_count(est, T)
    assert wrong == 0 and 0 < ruled < q
    if name == "small":
        # the CPU census (tools/gate_census.py) rules out 39 % of the mask survivors here: a quarter only keeps a dead gate from passing
        qn, rn, wn = _gate_count(est, near)
        assert wn == 0 and rn >= 0.25 * qn, (qn, rn)


def test_gate_on_a_grid_with_distance_bounds():
    """`dense`: lists long enough for the epsilon/2 grid, whose cell words carry a distance bound in place of the mask (has_nearest)"""
    est, near = _workload("dense")
    T = np.concatenate([near[:512], _odd(near, np.random.default_rng(6))])
    for split in (1, 0):
        est.set_option("lcp_split", split)
        s = _three_ways(est, T)
    assert s[:512].max() > 0.05
    q, ruled, wrong = _gate_count(est, T)
    assert wrong == 0 and ruled > 0


def test_gate_on_unpruned_lists(monkeypatch):
    """STOCS_GRID_PRUNE=0: the lists hold every scene point within epsilon of the cell, and the cones cover all of them"""
    est0, near = _workload("small")
    ref = _three_ways(est0, near)
    monkeypatch.setenv("STOCS_GRID_PRUNE", "0")
    est, _ = _workload("small")
    s = _three_ways(est, near)
    assert np.array_equal(s.view(np.uint32), ref.view(np.uint32))
    q, ruled, wrong = _gate_count(est, near)
    assert wrong == 0 and ruled >= 0.25 * q


def test_gate_in_millimetres():
    est_m, Tm = _workload("small")
    ref = _three_ways(est_m, Tm)
    est, T = _workload("small", scale=1000.0, distance_threshold=5.0)
    s = _three_ways(est, T)
    assert s.max() > 0.05 and abs(float(s.max()) - float(ref.max())) < 0.05
    q, ruled, wrong = _gate_count(est, T)
    assert wrong == 0 and ruled >= 0.25 * q


# ---- hand-built scenes --------------------------------------------------------------------------------------------------
def _plane(n=25, step=0.002):
    g = (np.arange(n) - (n - 1) / 2.0) * step
    x, y = np.meshgrid(g, g)
    return np.stack([x.ravel(), y.ravel(), np.zeros(n * n)], 1)


def _line(n=121, step=0.0003):
    x = (np.arange(n) - (n - 1) / 2.0) * step
    return np.stack([x, np.zeros(n), np.zeros(n)], 1)


def _rot_x(c, s, ty=0.0):
    """column-major centred transform: rotation about x with the given cosine and sine (float32 as given), translation along y"""
    T = np.zeros((4, 4), np.float32)
    T[0, 0] = 1; T[1, 1] = c; T[1, 2] = -s; T[2, 1] = s; T[2, 2] = c; T[1, 3] = ty; T[3, 3] = 1
    return T.T.reshape(16)


def _poses_about_the_threshold():
    """the model normal (0, 0, 1) of a line of points on the rotation axis, turned so that its dot product with the plane's normal
    is cos 30 degrees +- 0..8 ulps (the rotated normal's z IS the matrix entry), and well past it, at three offsets across cells"""
    T = []
    for ty in (0.0, 0.0013, -0.0101):
        for k in range(-8, 9):
            c = DOT_LO
            for _ in range(abs(k)):
                c = np.nextafter(c, np.float32(2.0 if k > 0 else 0.0), dtype=np.float32)
            T.append(_rot_x(c, np.float32(np.sqrt(1.0 - float(c) ** 2)), ty))
        for deg in (0.0, 25.0, 29.9, 30.1, 33.0, 34.0, 35.0, 40.0, 60.0, 90.0, 120.0, 150.0, 180.0, -35.0, -90.0):
            T.append(_rot_x(np.float32(np.cos(np.deg2rad(deg))), np.float32(np.sin(np.deg2rad(deg))), ty))
    return np.stack(T)


def test_plane_with_identical_normals_about_the_threshold():
    spos = _plane(); snrm = np.tile([0.0, 0.0, 1.0], (len(spos), 1))
    mpos = _line(); mnrm = np.tile([0.0, 0.0, 1.0], (len(mpos), 1))
    est = _estimator(spos, snrm, mpos, mnrm)
    T = _poses_about_the_threshold()
    for split in (1, 0):
        est.set_option("lcp_split", split)
        s = _three_ways(est, T)
    # the threshold is straddled: 8 ulps above counts every point, 8 ulps below none
    assert s[16] > 0.4 and s[0] == 0.0 and s[17] > 0.4 and s[17 + 5] == 0.0
    q, ruled, wrong = _gate_count(est, T)
    assert wrong == 0 and ruled > 0      # the poses well past 30 degrees are ruled out, the ones about it are not counted wrongly


def test_cells_with_opposite_and_broken_normals():
    """a plane whose normals alternate between +z and -z (no cone can hold them), then one with zero, NaN, half-length and
    double-length normals sprinkled in (the loader normalises what it can; a cell with a normal that is not unit has no cone)"""
    spos = _plane()
    mpos = _line(); mnrm = np.tile([0.0, 0.0, 1.0], (len(mpos), 1))
    T = _poses_about_the_threshold()
    flip = np.where((np.arange(len(spos)) % 2 == 0)[:, None], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0])
    est = _estimator(spos, flip, mpos, mnrm)
    s = _three_ways(est, T)
    assert s.max() > 0.0
    assert _gate_count(est, T)[2] == 0
    broken = np.tile([0.0, 0.0, 1.0], (len(spos), 1))
    broken[3::17] = 0.0; broken[5::19] = np.nan; broken[7::23] *= 0.5; broken[11::29] *= 2.0; broken[13::31] = [0.0, 0.6, 0.8]
    est = _estimator(spos, broken, mpos, mnrm)
    s = _three_ways(est, T)
    assert s.max() > 0.0
    assert _gate_count(est, T)[2] == 0


def test_instance_mode_batch_with_per_trial_weights():
    """every trial of an instance-mode batch scores against its own copy of the scene normals and weights: the same normals the
    cones were built from, so those launches stay gated -- and return what the ungated ones return"""
    from model_matching_amd.estimator import StocsEstimator
    d = np.load(os.path.join(GOLD, "example_packed_dove.npz"))
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
    est.set_edge_map(d["edge_map"])
    res = {}
    for g in (0, 1):
        est.set_option("lcp_normal_gate", g)
        res[g] = est.run_trials([1, 2, 3], 24, mode=1)
    assert any(r["best_lcp"] > 0 for r in res[0])
    for a, b in zip(res[0], res[1]):
        assert a["best_index"] == b["best_index"] and a["best_lcp"] == b["best_lcp"] and a["n_candidates"] == b["n_candidates"]


def test_option_values():
    from model_matching_amd import capi
    est, _ = _workload("tiny")
    for bad in (2, -1, 16):
        with pytest.raises(capi.StocsError):
            est.set_option("lcp_normal_gate", bad)
    est.set_option("lcp_normal_gate", 0)
    est.set_option("lcp_normal_gate", 1)
