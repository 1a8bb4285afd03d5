"""stocs_pose_errors_sym / stocs_pose_errors_sym_detail on the GPU against the float32 restatement of their contract
(tests/pose_error_sym_ref.py): every comparison is bit equality on every field.  The shapes are the smallest at which the kernel can go
wrong: the issue's model sizes plus one below, at and one above every constant include/stocs_hip.h names for the kernel, symmetry counts
around the symmetry block, a few pairs.  The scene plays no part (a handful of points serves)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pose_error_cases as pc  # noqa: E402
import pose_error_ref as base  # noqa: E402
import pose_error_sym_cases as cases  # noqa: E402
import pose_error_sym_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
KB = cases.kernel_sizes()["BLOCK"]
KMAX = cases.kernel_sizes()["MAX"]


def _est(model_pos):
    from model_matching_amd.estimator import StocsEstimator
    m = np.asarray(model_pos, F).reshape(-1, 3)
    rng = np.random.default_rng(1)
    sp = rng.normal(0, 0.05, (32, 3)).astype(F)
    sn = sp / np.linalg.norm(sp, axis=1, keepdims=True)
    nrm = np.tile(np.array([0, 0, 1], F), (len(m), 1))
    return StocsEstimator(sp, sn, np.ones(32, F), None, m, nrm, build_index=False)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = [i for i in range(len(got)) if not ref.records_equal(got[i], want[i])]
    assert not bad, (bad[:5], got[bad[:5]], want[bad[:5]])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (a, b)


def _check(est, c, detail_of=0):
    """the records, and for one pair the detail, against the restatement; the records' minima against the index-ordered minima of the
    library's own detail -> the records"""
    e, g = np.asarray(c["est"], F).reshape(-1, 16), np.asarray(c["gt"], F).reshape(-1, 16)
    got = est.pose_errors_sym(e, g, c["syms"], c.get("cam"))
    _same(got, ref.records(e, g, c["syms"], c["model"], c.get("cam")))
    gk = g[0 if len(g) == 1 else detail_of]
    af, m3, m2 = est.pose_errors_sym_detail(e[detail_of], gk, c["syms"], c.get("cam"))
    waf, wm3, wm2 = ref.per_symmetry(e[detail_of], gk, c["syms"], c["model"], c.get("cam"))
    _same_bits(af, waf); _same_bits(m3, wm3); _same_bits(m2, wm2)
    r = got[detail_of]
    if r["valid"]:
        assert r["add_fix"] == af.min() and r["k_add"] == int(np.argmin(af))
        assert r["mssd"] == m3.min() and r["k_mssd"] == (int(np.argmin(m3)) if np.isfinite(m3.min()) else -1)
        assert r["mspd"] == m2.min() and r["k_mspd"] == (int(np.argmin(m2)) if np.isfinite(m2.min()) else -1)
    return got


@pytest.mark.parametrize("M", cases.model_sizes())
def test_every_model_size(M):
    est = _est(pc.random_model(M))
    _check(est, cases.random_case(M, KB + 1, 3, M, cam=cases.CAM), detail_of=2)
    _check(est, cases.random_case(M, 3, 2, M + 7, n_gt=1))
    est.close()


@pytest.fixture(scope="module")
def shared():
    """one 65-point model and its context for the tests that need nothing else"""
    model = pc.random_model(65)
    est = _est(model)
    yield dict(model=model, est=est)
    est.close()


@pytest.mark.parametrize("K", cases.sym_counts())
@pytest.mark.parametrize("cam", [None, cases.CAM, cases.CAM_OFF], ids=["nocam", "cam", "offcentre"])
def test_every_symmetry_count(shared, K, cam):
    c = cases.random_case(65, K, 3, 40 + K, cam=cam)
    _check(shared["est"], c, detail_of=1)
    c = cases.random_case(65, K, 3, 41 + K, n_gt=1, cam=cam)
    _check(shared["est"], c)


def test_the_largest_symmetry_count(shared):
    c = cases.random_case(65, KMAX, 1, 5, cam=cases.CAM)
    got = _check(shared["est"], c)
    assert got["valid"][0] == 1 and 0 <= got["k_mssd"][0] < KMAX


@pytest.mark.parametrize("n", [1, 3, 257])
def test_batches_with_one_and_with_n_ground_truths(shared, n):
    _check(shared["est"], cases.random_case(65, KB + 1, n, 90 + n, cam=cases.CAM), detail_of=n - 1)
    _check(shared["est"], cases.random_case(65, 2, n, 91 + n, n_gt=1), detail_of=n // 2)


def test_identity_set_equals_the_plain_records(shared):
    """K = 1 and the identity: add_fix and add equal stocs_pose_errors's and mssd its add_max, bit for bit, library against library"""
    e, g = pc.random_pairs(40, 17)
    e[20:], g[20:] = pc.random_pairs(20, 18, near=True)
    plain = shared["est"].pose_errors(e, g)
    sym = shared["est"].pose_errors_sym(e, g, ref.IDENTITY)
    assert np.all(sym["valid"] == 1)
    _same_bits(sym["add_fix"], plain["add_fix"]); _same_bits(sym["add"], plain["add"]); _same_bits(sym["mssd"], plain["add_max"])
    assert np.all(sym["k_add"] == 0) and np.all(sym["k_mssd"] == 0) and np.all(sym["k_mspd"] == -1) and np.all(np.isposinf(sym["mspd"]))


@pytest.mark.parametrize("j", [0, 1, 2, 3])
def test_exact_hit_names_its_symmetry(j):
    c = cases.exact_hit(j)
    est = _est(c["model"])
    r = _check(est, c)[0]
    assert r["mssd"] == 0 and r["add_fix"] == 0 and r["add"] == 0 and r["mspd"] == 0 and r["k_mssd"] == j and r["k_add"] == j and r["k_mspd"] == j
    est.close()


def test_exact_ties_go_to_the_lowest_index():
    c = cases.exact_listed_twice()
    est = _est(c["model"])
    r = _check(est, c)[0]
    assert r["mssd"] == 0 and r["k_mssd"] == 1 and r["k_add"] == 1 and r["k_mspd"] == 1
    est.close()
    c = cases.exact_invariant_model()
    est = _est(c["model"])
    r = _check(est, c, detail_of=1)
    assert np.all(r["k_mssd"] == 0) and np.all(r["k_add"] == 0) and np.all(r["k_mspd"] == 0) and r["mssd"][0] == 0 and r["mssd"][1] == c["shift"]
    # the same tie across symmetry blocks and across the min kernel's lanes: the four quarter turns again and again, 2 KB + 1 and 130 entries
    for K in (2 * KB + 1, 130):
        c2 = dict(c, syms=np.tile(c["syms"], (K // 4 + 1, 1))[:K])
        r = _check(est, c2, detail_of=1)
        assert np.all(r["k_mssd"] == 0) and np.all(r["k_add"] == 0) and np.all(r["k_mspd"] == 0)
    est.close()
    c = cases.exact_none_right()
    est = _est(c["model"])
    r = _check(est, c)[0]
    assert r["mssd"] == c["mssd"] and r["k_mssd"] == 0 and r["k_add"] == 0 and r["add_fix"] > 0
    est.close()


def test_a_late_symmetry_wins_from_any_lane_and_block():
    """130 symmetries of which exactly one is right, at an index in the last block and in the min kernel's third round"""
    c = cases.exact_hit(1)
    q = c["syms"]
    est = _est(c["model"])
    for at in (0, 63, 64, 129):
        syms = np.tile(q[3], (130, 1)); syms[at] = q[1]
        r = _check(est, dict(c, syms=syms))[0]
        assert r["mssd"] == 0 and r["k_mssd"] == at and r["k_add"] == at and r["k_mspd"] == at
    est.close()


def test_projection_edges():
    c = cases.depth_edge_ground_truth()
    est = _est(c["model"])
    _check(est, c)
    _, _, m2 = est.pose_errors_sym_detail(c["est"][0], c["gt"][0], c["syms"], c["cam"])
    assert [k for k in range(4) if np.isposinf(m2[k])] == c["inf_k"] and np.all(np.isfinite(np.delete(m2, c["inf_k"])))
    c = cases.depth_edge_estimate()
    r = _check(est, c)
    assert np.isposinf(r["mspd"][0]) and r["k_mspd"][0] == -1 and np.isfinite(r["mspd"][1]) and r["k_mspd"][1] >= 0 and np.all(np.isfinite(r["mssd"]))
    est.close()
    c = cases.behind_camera()
    est = _est(c["model"])
    r = _check(est, c)[0]
    assert np.isposinf(r["mspd"]) and r["k_mspd"] == -1 and np.isfinite(r["mssd"]) and r["k_mssd"] >= 0 and r["valid"] == 1
    est.close()
    c = cases.optical_axis()
    est = _est(c["model"])
    r = _check(est, c)[0]
    assert r["mspd"] == 0 and r["k_mspd"] == 0 and r["mssd"] == F(0.25)
    est.close()


def test_saturation_and_validity():
    c = cases.far_apart()
    est = _est(c["model"])
    r = _check(est, c)[0]
    assert r["add_fix"] == len(c["model"]) * (1 << 47) and r["add"] == F(32768) and r["mssd"] > 0.9e5 and r["valid"] == 1
    c = cases.invalid_poses()
    got = _check(est, c)
    assert np.array_equal(got["valid"], c["valid"])
    bad = got[c["valid"] == 0]
    assert np.all(bad["add_fix"] == 0) and all(np.all(np.isposinf(bad[k])) for k in ("add", "mssd", "mspd"))
    assert all(np.all(bad[k] == -1) for k in ("k_add", "k_mssd", "k_mspd"))
    keep = [0, 2, 4, 6]
    _same(got[keep], est.pose_errors_sym(c["est"][keep], c["gt"][keep], c["syms"], c["cam"]))     # the invalid neighbours changed nothing
    g = c["gt"][3:4]                                                                             # ONE ground truth that is itself invalid
    got = est.pose_errors_sym(c["est"], g, c["syms"], c["cam"])
    _same(got, ref.records(c["est"], g, c["syms"], c["model"], c["cam"]))
    assert np.all(got["valid"] == 0)
    est.close()


def test_a_record_does_not_depend_on_its_batch(shared):
    c = cases.random_case(65, KB + 1, 300, 23, cam=cases.CAM)
    est = shared["est"]
    whole = est.pose_errors_sym(c["est"], c["gt"], c["syms"], c["cam"])
    for k in (0, 150, 299):
        alone = est.pose_errors_sym(c["est"][k], c["gt"][k], c["syms"], c["cam"])
        _same(alone, whole[k:k + 1])
        _same(alone, ref.records(c["est"][k], c["gt"][k], c["syms"], c["model"], c["cam"]))
    rev = est.pose_errors_sym(c["est"][::-1], c["gt"][::-1], c["syms"], c["cam"])
    _same(rev[::-1].copy(), whole)


def test_second_call_gives_the_same_bytes_and_allocates_nothing(shared):
    from model_matching_amd import capi
    L = capi.load()
    est = shared["est"]
    c = cases.random_case(65, 2 * KB + 1, 40, 31, cam=cases.CAM)
    first = est.pose_errors_sym(c["est"], c["gt"], c["syms"], c["cam"])
    est.pose_errors_sym_detail(c["est"][0], c["gt"][0], c["syms"], c["cam"])
    before = L.stocs_device_alloc_count()
    second = est.pose_errors_sym(c["est"], c["gt"], c["syms"], c["cam"])
    est.pose_errors_sym(c["est"][:7], c["gt"][:1], c["syms"][:3])
    est.pose_errors_sym_detail(c["est"][1], c["gt"][1], c["syms"], c["cam"])
    assert L.stocs_device_alloc_count() == before
    assert first.tobytes() == second.tobytes()


def test_call_timing_names_the_steps_and_the_kernel(shared):
    est = shared["est"]
    c = cases.random_case(65, 3, 5, 37)
    steps = ["stage and enqueue", "wait for the device", "records"]
    est.set_option("device_clock", 0)
    want = est.pose_errors_sym(c["est"], c["gt"], c["syms"])
    t = est.last_call_timing(5)
    assert [k for k, _ in t] == steps and all(ms >= 0 for _, ms in t)
    est.set_option("device_clock", 1)
    got = est.pose_errors_sym(c["est"], c["gt"], c["syms"])
    t = est.last_call_timing(5)
    est.set_option("device_clock", 0)
    assert [k for k, _ in t] == steps + ["device: kernel"] and dict(t)["device: kernel"] > 0
    _same(got, want)


def test_refusals(shared):
    from model_matching_amd import capi
    L = capi.load()
    h = shared["est"].h
    c = cases.random_case(65, 3, 4, 3, cam=cases.CAM)
    P, G, S = np.ascontiguousarray(c["est"]), np.ascontiguousarray(c["gt"]), np.ascontiguousarray(c["syms"])
    pP, pG, pS = P.ctypes.data_as(capi._fp), G.ctypes.data_as(capi._fp), S.ctypes.data_as(capi._fp)
    out = (capi.PoseErrorSym * 4)()
    cam = capi.Camera(600.0, 320.0, 600.0, 240.0, 1.0, 0, 0, 0)
    f = L.stocs_pose_errors_sym
    assert f(h, pP, 4, pG, 4, pS, 3, C.byref(cam), out) == 0 and f(h, pP, 4, pG, 1, pS, 3, None, out) == 0
    assert f(None, pP, 4, pG, 4, pS, 3, None, out) == -1 and f(None, pP, 0, pG, 4, pS, 3, None, out) == -1
    assert f(h, pP, -1, pG, 1, pS, 3, None, out) == -1
    assert f(h, None, 0, None, 7, None, 0, None, None) == 0                       # n == 0: a no-op that looks at nothing else
    for K in (0, -1, KMAX + 1):
        assert f(h, pP, 4, pG, 4, pS, K, None, out) == -1, K
    assert f(h, None, 4, pG, 4, pS, 3, None, out) == -1 and f(h, pP, 4, None, 4, pS, 3, None, out) == -1
    assert f(h, pP, 4, pG, 4, None, 3, None, out) == -1 and f(h, pP, 4, pG, 4, pS, 3, None, None) == -1
    for n_gt in (0, 2, 3, 5, -1):
        assert f(h, pP, 4, pG, n_gt, pS, 3, None, out) == -1, n_gt
    for at, v in ((0, np.nan), (16 + 13, np.inf), (32 + 10, -np.inf)):
        S2 = S.copy(); S2.reshape(-1)[at] = v
        assert f(h, pP, 4, pG, 4, S2.ctypes.data_as(capi._fp), 3, None, out) == -1, at
    S2 = S.copy(); S2.reshape(-1)[[3, 7, 11, 15]] = np.nan                        # not among the twelve used entries
    assert f(h, pP, 4, pG, 4, S2.ctypes.data_as(capi._fp), 3, None, out) == 0
    for name in ("fx", "fy", "cx", "cy"):
        bad = capi.Camera(600.0, 320.0, 600.0, 240.0, 1.0, 0, 0, 0); setattr(bad, name, float("nan"))
        assert f(h, pP, 4, pG, 4, pS, 3, C.byref(bad), out) == -1, name
    # a workspace above 1 GiB: 4 096 pairs with their own ground truths x 4 096 symmetries (80 bytes per pair and symmetry); nothing is allocated
    n = 4096
    bigP, bigS = np.tile(P[:1], (n, 1)), np.tile(S[:1], (KMAX, 1))
    bigout = (capi.PoseErrorSym * n)()
    before = L.stocs_device_alloc_count()
    assert f(h, bigP.ctypes.data_as(capi._fp), n, bigP.ctypes.data_as(capi._fp), n, bigS.ctypes.data_as(capi._fp), KMAX, None, bigout) == -1
    assert L.stocs_device_alloc_count() == before and b"workspace" in L.stocs_last_error()
    d = L.stocs_pose_errors_sym_detail
    assert d(h, pP, pG, pS, 3, None, None, None, None) == 0                        # every output may be NULL
    assert d(None, pP, pG, pS, 3, None, None, None, None) == -1 and d(h, None, pG, pS, 3, None, None, None, None) == -1
    assert d(h, pP, None, pS, 3, None, None, None, None) == -1 and d(h, pP, pG, None, 3, None, None, None, None) == -1
    assert d(h, pP, pG, pS, 0, None, None, None, None) == -1 and d(h, pP, pG, pS, KMAX + 1, None, None, None, None) == -1


def test_a_turned_pose_on_the_symmetric_model():
    """synth's Cm (an ellipsoid of revolution with one bump) under symmetry_set((0, 0, 360), 72): the estimate is the ground truth turned by
    137 degrees about the model's z and moved 2 mm.  Plain ADD is above 0.1 diameter, MSSD below it, and the winning step is the one
    nearest to 137 degrees (27: 135 degrees).  Both expectations come from the float64 brute force, not from the library."""
    from model_matching_amd import synth
    from model_matching_amd.estimator import symmetry_set
    model = synth.make_model().pos
    gt = synth.gt_pose().T.reshape(16).astype(F)
    D = np.eye(4); D[:3, :3] = pc.rot((0, 0, 1), 137.0); D[:3, 3] = (0.002, 0.0, 0.0)
    e = cases.compose64(gt, D.T.reshape(16))
    S = symmetry_set((0, 0, 360), 72)
    d64 = base.diameter64(model)
    w = ref.measures64(e, gt, S, model, cases.CAM)
    plain64 = ref.measures64(e, gt, ref.IDENTITY[None], model)
    assert plain64["add"] > 0.1 * d64 and w["mssd"] < 0.1 * d64 and w["k_mssd"] == 27      # what the test expects, settled in float64
    est = _est(model)
    got = _check(est, dict(model=model, est=e[None], gt=gt[None], syms=S, cam=cases.CAM))[0]
    plain = est.pose_errors(e, gt)[0]
    d = est.model_diameter()
    assert plain["add"] > 0.1 * d and got["mssd"] < 0.1 * d and got["k_mssd"] == 27 and got["k_mssd"] == w["k_mssd"]
    assert abs(float(got["mssd"]) - w["mssd"]) < 5e-6 and abs(float(got["add"]) - w["add"]) < 5e-6 and got["k_add"] == w["k_add"]      # T = sqrt(3) (g4 + g7) A with A < 2 m
    assert abs(float(got["mspd"]) - w["mspd"]) < 1e-2 and got["k_mspd"] == w["k_mspd"]
    est.close()
