"""stocs_symmetry_errors / stocs_symmetry_errors_detail / stocs_find_symmetries on the GPU.  Records and detail against the float32
restatement of their contract (tests/symmetry_ref.py): bit equality on every field, on the smallest shapes at which the kernel can go wrong
(tests/symmetry_cases.py).  The search against the restated search on float64 scores: the same axes within the angle derived from its
parameters, the same orders, set size, descriptor and flags.  The scene plays no part (a handful of points serves)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pose_error_cases as pc  # noqa: E402
import symmetry_cases as cases  # noqa: E402
import symmetry_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
KERNEL = cases.kernel_cases()
SEARCH = sorted(cases.SEARCH_CASES)


def _est(model, normals):
    from model_matching_amd.estimator import StocsEstimator
    rng = np.random.default_rng(1)
    sp = rng.normal(0, 0.05, (32, 3)).astype(F)
    sn = sp / np.linalg.norm(sp, axis=1, keepdims=True)
    return StocsEstimator(sp, sn, np.ones(32, F), None, np.asarray(model, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3), build_index=False)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = [i for i in range(len(got)) if not ref.records_equal(got[i], want[i])]
    assert not bad, (bad[:5], got[bad[:5]], want[bad[:5]])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (a, b)


@pytest.mark.parametrize("name", sorted(KERNEL))
def test_records_and_detail_equal_the_restatement(name):
    c = KERNEL[name]
    est = _est(c["model"], c["normals"])
    got = est.symmetry_errors(c["transforms"], c["reach"], c["cos_normal"])
    _same(got, ref.records(c["transforms"], c["model"], c["normals"], c["reach"], c["cos_normal"]))
    boundary = name.startswith("lattice") and not name.endswith("wide")
    for T in c["transforms"]:
        s, nn, dot = est.symmetry_errors_detail(T, c["reach"], c["cos_normal"])
        ws, wnn, wdot, matched, _ = ref.detail(T, c["model"], c["normals"], c["reach"], c["cos_normal"])
        _same_bits(s, ws); _same_bits(nn, wnn); _same_bits(dot, wdot)
        if not boundary:   # the library's own brute-force kernel: the same expressions wherever a point is matched
            _, ls, lnn = est.pose_errors_detail(T, ref.IDENTITY)
            _same_bits(s[matched], ls[matched]); _same_bits(nn[matched], lnn[matched])
    est.close()


@pytest.fixture(scope="module")
def shared():
    """one 257-point model, its context and a batch of 300 transforms with their restated records"""
    c = cases.random_case(257, 300, 11, unit=False)
    est = _est(c["model"], c["normals"])
    want = ref.records(c["transforms"], c["model"], c["normals"], c["reach"], c["cos_normal"])
    yield dict(c, est=est, want=want)
    est.close()


def test_a_record_does_not_depend_on_its_batch(shared):
    est, T, reach = shared["est"], shared["transforms"], shared["reach"]
    _same(est.symmetry_errors(T, reach), shared["want"])
    for k in (7, 150, 299):
        one = T[k]
        for at in (0, 150, 299):   # first, in the middle, last of 300
            B = T.copy(); B[at] = one
            _same(est.symmetry_errors(B, reach)[at:at + 1], shared["want"][k:k + 1])
        _same(est.symmetry_errors(one, reach), shared["want"][k:k + 1])
    assert len(est.symmetry_errors(np.zeros((0, 16), F), reach)) == 0


def test_a_repeat_call_allocates_nothing(shared):
    from model_matching_amd import capi
    est, T, reach = shared["est"], shared["transforms"], shared["reach"]
    est.symmetry_errors(T, reach)
    est.symmetry_errors_detail(T[0], reach)
    n0 = capi.load().stocs_device_alloc_count()
    _same(est.symmetry_errors(T, reach), shared["want"])
    _same(est.symmetry_errors(T[:17], reach), shared["want"][:17])
    est.symmetry_errors_detail(T[3], reach)
    assert capi.load().stocs_device_alloc_count() == n0
    steps = dict(est.last_call_timing(6))
    assert {"stage and enqueue", "wait for the device", "records"} <= set(steps)


def test_another_reach_rebuilds_the_grid_and_going_back_restores_it(shared):
    est, T = shared["est"], shared["transforms"][:12]
    second = F(0.0031)
    _same(est.symmetry_errors(T, shared["reach"]), shared["want"][:12])
    _same(est.symmetry_errors(T, second), ref.records(T, shared["model"], shared["normals"], second))
    _same(est.symmetry_errors(T, shared["reach"]), shared["want"][:12])
    s, nn, dot = est.symmetry_errors_detail(T[5], second)
    ws, wnn, wdot, _, _ = ref.detail(T[5], shared["model"], shared["normals"], second)
    _same_bits(s, ws); _same_bits(nn, wnn); _same_bits(dot, wdot)


@pytest.mark.parametrize("K", cases.launch_counts())
def test_transform_counts_about_the_launch_limit(K):
    """three distinct transforms tiled: every record of a call of several launches is the restated one of its transform"""
    c = cases.random_case(3, 3, 12)
    est = _est(c["model"], c["normals"])
    want = ref.records(c["transforms"], c["model"], c["normals"], c["reach"])
    idx = np.arange(K) % 3
    idx[-1] = 1
    _same(est.symmetry_errors(c["transforms"][idx], c["reach"]), want[idx])
    est.close()


def test_argument_checks_on_a_live_context(shared):
    from model_matching_amd import capi
    est, T = shared["est"], shared["transforms"]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(capi.StocsError):
            est.symmetry_errors(T[:2], bad)
        with pytest.raises(capi.StocsError):
            est.symmetry_errors_detail(T[0], bad)
    B = T[:3].copy(); B[1, 13] = np.inf
    with pytest.raises(capi.StocsError):
        est.symmetry_errors(B, shared["reach"])
    B = T[:3].copy(); B[1, 3] = np.nan   # not among the twelve
    _same(est.symmetry_errors(B, shared["reach"]), shared["want"][:3])
    _same(est.symmetry_errors(T[:3], shared["reach"]), shared["want"][:3])   # a refused call leaves the state usable
    with pytest.raises(capi.StocsError):
        est.symmetry_errors(T[:2], 1e-20)   # a reach whose square is not a normal float
    with pytest.raises(capi.StocsError):
        est.symmetry_errors_detail(T[0], 1e-20)
    # the checks in the header's order, straight at the C ABI: K < 0, K == 0 before any pointer, NULL pointers, the workspace limit
    L = capi.load()
    prm = capi.SymmetryParams(float(shared["reach"]), 0.5, (C.c_int32 * 2)(0, 0))
    out = (capi.SymmetryError * 3)()
    Tp = np.ascontiguousarray(T[:3]).ctypes.data_as(capi._fp)
    assert L.stocs_symmetry_errors(est.h, Tp, -1, C.byref(prm), out) == -1
    assert L.stocs_symmetry_errors(est.h, None, 0, None, None) == 0
    assert L.stocs_symmetry_errors(est.h, None, 3, C.byref(prm), out) == -1
    assert L.stocs_symmetry_errors(est.h, Tp, 3, None, out) == -1
    assert L.stocs_symmetry_errors(est.h, Tp, 3, C.byref(prm), None) == -1
    assert L.stocs_symmetry_errors_detail(est.h, None, C.byref(prm), None, None, None) == -1
    assert L.stocs_symmetry_errors_detail(est.h, Tp, None, None, None, None) == -1
    assert L.stocs_symmetry_errors_detail(est.h, Tp, C.byref(prm), None, None, None) == 0   # every output may be NULL
    too_many = (1 << 30) // 96 + 1000            # 96 bytes of workspace per transform against the 1 GiB limit
    big = np.zeros((too_many, 16), F)            # untouched zero pages: finite entries, nothing is copied
    n0 = L.stocs_device_alloc_count()
    assert L.stocs_symmetry_errors(est.h, big.ctypes.data_as(capi._fp), too_many, C.byref(prm), out) == -1
    assert b"workspace" in L.stocs_last_error() and L.stocs_device_alloc_count() == n0
    del big
    assert L.stocs_symmetry_errors(est.h, Tp, 3, C.byref(prm), out) == 0
    _same(np.frombuffer(out, dtype=ref.DTYPE, count=3), ref.records(T[:3], shared["model"], shared["normals"], shared["reach"], 0.5))
    with pytest.raises(capi.StocsError):
        est.find_symmetries(n_axes=2)
    with pytest.raises(capi.StocsError):
        est.find_symmetries(same_deg=0.0)


# ---- the search ----
@pytest.fixture(scope="module")
def found():
    """name -> (case, estimator, what find_symmetries returned); one context per search case"""
    out = {}
    for name in SEARCH:
        c = cases.search_case(name)
        est = _est(c["model"], c["normals"])
        out[name] = (c, est, est.find_symmetries(tol_max=float(c["tol_resolved"])))
    yield out
    for _, est, _ in out.values():
        est.close()


@pytest.mark.parametrize("name", SEARCH)
def test_find_symmetries_returns_the_restated_search(found, name):
    c, est, (axes, S, sym3, flags) = found[name]
    waxes, wS, wsym3, wflags = cases.search_restated(name)
    assert len(axes) == len(waxes) == len(c["expect"]) and flags == wflags == c["flags"]
    assert len(S) == len(wS) == c["K"] and np.array_equal(sym3, wsym3)
    bound = cases.axis_bound_deg()
    left = list(range(len(waxes)))
    for a in axes:
        k = min(left, key=lambda j: cases.angle_deg(a["axis"], waxes[j]["axis"]))
        assert cases.angle_deg(a["axis"], waxes[k]["axis"]) <= bound and a["order"] == waxes[k]["order"], (a, waxes[k])
        left.remove(k)
    assert np.array_equal(S[0], ref.IDENTITY)
    if len(axes) > 1:
        assert np.all(np.diff(axes["mean"]) >= 0)   # best first


@pytest.mark.parametrize("name", SEARCH)
def test_every_transform_of_the_found_set_passes(found, name):
    c, est, (axes, S, sym3, flags) = found[name]
    tol = c["tol_resolved"]
    rec = est.symmetry_errors(S, tol)
    assert np.all(rec["n_far"] == 0) and np.all(rec["max"] <= tol)
    assert rec[0]["sum_fix"] == 0 and rec[0]["max"] == 0
    if len(axes):   # the axes' records are those of their generators
        from model_matching_amd.estimator import symmetry_rotation
        gens = np.stack([symmetry_rotation(a["axis"], 360.0 / (int(a["order"]) or 6), c["center"]) for a in axes])
        again = est.symmetry_errors(gens, tol)
        assert np.array_equal(again["mean"], axes["mean"]) and np.array_equal(again["max"], axes["max"])
        assert np.array_equal(again["n_normal_bad"], axes["n_normal_bad"])


def test_the_blob_returns_the_identity_alone(found):
    c, est, (axes, S, sym3, flags) = found["blob"]
    assert len(axes) == 0 and flags == ref.NOTHING and S.shape == (1, 16) and np.array_equal(S[0], ref.IDENTITY) and not sym3.any()


def test_the_default_tolerance_is_a_tenth_of_the_diameter(found):
    c, est, _ = found["d2"]
    a = est.find_symmetries()
    b = est.find_symmetries(tol_max=float(F(0.1) * est.model_diameter()))
    for x, y in zip(a[:3], b[:3]):
        _same_bits(x, y)
    assert a[3] == b[3]


def test_found_set_closes_the_loop_with_the_symmetric_pose_errors(found):
    """estimates gt o S_k of the C4 case: under the found set the MSSD is within the tolerance, under the identity alone it is not"""
    c, est, (axes, S, sym3, flags) = found["c4_z"]
    tol = c["tol_resolved"]
    gt = pc.pose(pc.rot((0.2, -0.4, 0.9), 37.0), (0.03, -0.02, 0.8))
    G = gt.reshape(4, 4).T.astype(np.float64)
    ests = np.stack([(G @ s.reshape(4, 4).T.astype(np.float64)).T.reshape(16).astype(F) for s in S])
    with_set = est.pose_errors_sym(ests, gt, S)
    alone = est.pose_errors_sym(ests, gt, ref.IDENTITY)
    assert np.all(with_set["valid"] == 1) and np.all(with_set["mssd"] <= tol)
    assert np.all(alone["mssd"][1:] > tol) and alone["mssd"][0] <= tol
    assert sorted(with_set["k_mssd"]) == list(range(len(S)))
