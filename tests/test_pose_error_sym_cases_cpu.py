"""The symmetry-aware restatement (tests/pose_error_sym_ref.py) against a float64 brute force, the seeded cases
(tests/pose_error_sym_cases.py) against what each is named for, stocs_symmetry_set through ctypes, and pose_recall_sym.  No GPU.

The bound.  u = 2^-24, g_n = n u / (1 - n u).  tests/test_pose_error_cases_cpu.py derives |e32 - e64| <= T + 6u e with
T = 2 sqrt(3) g4 A, where g4 A bounds the error of one coordinate of a transformed point (three products and three sums: four rounding
levels) and the factor 2 counts the two points of a difference.  Here the ground-truth point is transformed by the COMPOSED pose, itself
rounded.  Follow one term of g_a = (C_a0 m_x + (C_a1 m_y + C_a2 m_z)) + u_a from the inputs: C_ab = G_a0 S_0b + (G_a1 S_1b + G_a2 S_2b)
passes through at most three roundings (product, inner sum, outer sum), then C_ab m_b through at most four more (product, two sums, + u_a):
seven levels; a term of u_a = (G_a0 s_0 + (G_a1 s_1 + G_a2 s_2)) + t_a passes through at most four, then one more in + u_a: five.  So
|g_a - exact| <= g7 A' with A' >= sum_bc |G_ac| |S_cb| |m_b| + sum_c |G_ac| |s_c| + |t_a| (the standard (1 + u)^n - 1 <= g_n argument
over the expanded sum; no cancellation is assumed).  The estimate's point carries g4 A_P as before.  With A >= A_P and A >= A' for
every point, row, pair and symmetry of the case: the difference d = p - g carries (g4 + g7) A + u |d_a| per coordinate, the vector at
most T = sqrt(3) (g4 + g7) A in length; squares, sums and root add less than 4u relatively as there.  Hence
    |e32 - e64| <= T + 6u e,   T = sqrt(3) (g4 + g7) A     (one extra rounding level of the composed pose: g4 + g4 became g4 + g7).
A maximum and a minimum move by no more than their candidates: max3_k, mssd within T + 6u x; the mean adds 2^-32 (the fixed point's
floor) and one rounding to float.
The projection.  With delta the coordinate error above (g4 A for the estimate, g7 A for the ground truth) and z = x_2 > delta, the
quotient fx x_0 / x_2 moves by at most fx delta (1 + |x_0| / z) / (z - delta), and the three operations (product, quotient, + cx) add
3u (|fx x_0 / z| + |cx|).  A difference of two such adds u |da|, the two squares, their sum and the root less than 4u relatively; so
per point |q32 - q64| <= sqrt(2) (E_p + E_g) + 6u q with E the larger of the a and b bounds of that point.  Checked only where every
point of both poses is in front of the camera (z > 1e-3)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import pose_error_cases as pc  # noqa: E402
import pose_error_ref as base  # noqa: E402
import pose_error_sym_cases as cases  # noqa: E402
import pose_error_sym_ref as ref  # noqa: E402

F = np.float32
U = 2.0 ** -24
G4 = 4 * U / (1 - 4 * U)
G7 = 7 * U / (1 - 7 * U)


def _abs_rows(M, m):
    """per point and row: sum_b |M_ab| |m_b| + |t_a|"""
    return m @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3])


def _A(model, est, gt, syms):
    m = np.abs(np.asarray(model, np.float64)).reshape(-1, 3)
    mat = lambda p: np.asarray(p, np.float64).reshape(4, 4).T
    a = max(float(_abs_rows(mat(P), m).max()) for P in est)
    for G in gt:
        for S in syms:
            Cm = np.abs(mat(G)) @ np.abs(mat(S))      # |G| |S|, the translation column included: sum_c |G_ac| |s_c| + |t_a|
            a = max(a, float(_abs_rows(Cm, m).max()))
    return a


def _proj_bound(cam, x, delta):
    """per point: the larger of the a and b error bounds of step 4 for float64 points x whose coordinates are known to delta"""
    fx, cx, fy, cy = [abs(float(F(v))) for v in cam]
    z = x[:, 2]
    ea = fx * delta * (1 + np.abs(x[:, 0]) / z) / (z - delta) + 3 * U * (fx * np.abs(x[:, 0]) / z + cx)
    eb = fy * delta * (1 + np.abs(x[:, 1]) / z) / (z - delta) + 3 * U * (fy * np.abs(x[:, 1]) / z + cy)
    return np.maximum(ea, eb)


def _check_against_float64(c):
    model, syms, cam = c["model"], np.asarray(c["syms"], F).reshape(-1, 16), c.get("cam")
    est, gt = np.asarray(c["est"], F).reshape(-1, 16), np.asarray(c["gt"], F).reshape(-1, 16)
    A = _A(model, est, gt, syms)
    T = np.sqrt(3.0) * (G4 + G7) * A
    rec = ref.records(est, gt, syms, model, cam)
    M = len(model)
    for n in range(len(est)):
        g = gt[0 if len(gt) == 1 else n]
        af, m3, m2 = ref.per_symmetry(est[n], g, syms, model, cam)
        e64, q64 = ref.per_symmetry64(est[n], g, syms, model, cam)
        x3 = e64.max(1)
        assert np.all(np.abs(m3 - x3) <= T + 6 * U * x3), np.abs(m3 - x3).max()
        mean32 = af.astype(np.float64) / 4294967296.0 / M
        assert np.all(np.abs(mean32 - e64.mean(1)) <= T + 6 * U * x3 + 2.0 ** -32), np.abs(mean32 - e64.mean(1)).max()
        r = rec[n]
        assert r["valid"] == 1 and r["k_add"] >= 0 and r["k_mssd"] >= 0
        assert abs(float(r["mssd"]) - x3.min()) <= T + 6 * U * x3.min()
        assert abs(float(r["add"]) - e64.mean(1).min()) <= T + 6 * U * x3.max() + 2.0 ** -32 + U * e64.mean(1).min()
        assert r["mssd"] == m3.min() and r["k_mssd"] == int(np.argmin(m3)) and r["add_fix"] == af.min() and r["k_add"] == int(np.argmin(af))
        if cam is None:
            assert np.all(np.isposinf(m2)) and np.isposinf(r["mspd"]) and r["k_mspd"] == -1
            continue
        Pm, Gm = np.asarray(est[n], np.float64).reshape(4, 4).T, np.asarray(g, np.float64).reshape(4, 4).T
        m64 = np.asarray(model, np.float64)
        p = m64 @ Pm[:3, :3].T + Pm[:3, 3]
        for k, S in enumerate(syms):
            Cm = Gm @ np.asarray(S, np.float64).reshape(4, 4).T
            gk = m64 @ Cm[:3, :3].T + Cm[:3, 3]
            if p[:, 2].min() <= 1e-3 or gk[:, 2].min() <= 1e-3:
                continue
            tol = np.sqrt(2.0) * (_proj_bound(cam, p, G4 * A) + _proj_bound(cam, gk, G7 * A)) + 6 * U * q64[k]
            assert abs(float(m2[k]) - q64[k].max()) <= tol.max(), (k, m2[k], q64[k].max(), tol.max())
        assert r["mspd"] == m2.min() and r["k_mspd"] == int(np.argmin(m2))
    return rec


@pytest.mark.parametrize("M", [1, 2, 65, 257, 1025])
def test_restatement_agrees_with_float64_on_random_pairs(M):
    _check_against_float64(cases.random_case(M, 9, 3, M, cam=cases.CAM))
    _check_against_float64(cases.random_case(M, 5, 3, M + 1, n_gt=1, cam=cases.CAM_OFF))
    _check_against_float64(cases.random_case(M, 2, 2, M + 2))


def test_restatement_agrees_with_float64_on_the_built_cases():
    for c in (cases.exact_hit(2), cases.exact_listed_twice(), cases.exact_invariant_model(), cases.exact_none_right(), cases.optical_axis()):
        _check_against_float64(c)


@pytest.mark.parametrize("M", [1, 65, 1025])
def test_identity_set_equals_the_plain_records_bit_for_bit(M):
    """K = 1 and the identity: add_fix and add equal stocs_pose_errors's, mssd its add_max, for every valid pair"""
    model = pc.random_model(M)
    e, g = pc.random_pairs(50, 300 + M)
    e[25:], g[25:] = pc.random_pairs(25, 301 + M, near=True)
    e = np.concatenate([e, pc.pose(pc.rot((0, 0, 1), 90), (0.0, -0.0, 0.5))[None]])       # axis-aligned, a -0 translation entry
    g = np.concatenate([g, pc.pose(pc.rot((1, 0, 0), 180), (-0.0, 0.25, 0.5))[None]])
    plain = base.records(e, g, model)
    sym = ref.records(e, g, ref.IDENTITY[None], model)
    assert np.all(plain["valid"] == 1) and np.all(sym["valid"] == 1)
    assert sym["add_fix"].tobytes() == plain["add_fix"].tobytes()
    assert sym["add"].tobytes() == plain["add"].tobytes()
    assert sym["mssd"].tobytes() == plain["add_max"].tobytes()
    assert np.all(sym["k_add"] == 0) and np.all(sym["k_mssd"] == 0) and np.all(sym["k_mspd"] == -1) and np.all(np.isposinf(sym["mspd"]))


@pytest.mark.parametrize("j", [0, 1, 2, 3])
def test_exact_hit_names_its_symmetry(j):
    c = cases.exact_hit(j)
    af, m3, m2 = ref.per_symmetry(c["est"][0], c["gt"][0], c["syms"], c["model"], c["cam"])
    assert [k for k in range(4) if m3[k] == 0] == [j] and [k for k in range(4) if af[k] == 0] == [j] and [k for k in range(4) if m2[k] == 0] == [j]
    r = ref.records(c["est"], c["gt"], c["syms"], c["model"], c["cam"])[0]
    assert r["mssd"] == 0 and r["add_fix"] == 0 and r["add"] == 0 and r["mspd"] == 0 and r["k_mssd"] == j and r["k_add"] == j and r["k_mspd"] == j


def test_exact_ties_go_to_the_lowest_index():
    c = cases.exact_listed_twice()
    af, m3, m2 = ref.per_symmetry(c["est"][0], c["gt"][0], c["syms"], c["model"], c["cam"])
    assert m3[1] == 0 and m3[2] == 0 and m3[0] > 0 and m3[3] > 0 and af[1] == 0 and af[2] == 0
    r = ref.records(c["est"], c["gt"], c["syms"], c["model"], c["cam"])[0]
    assert r["k_mssd"] == 1 and r["k_add"] == 1 and r["k_mspd"] == 1 and r["mssd"] == 0
    c = cases.exact_invariant_model()
    for n, want in ((0, F(0)), (1, c["shift"])):
        af, m3, m2 = ref.per_symmetry(c["est"][n], c["gt"][0], c["syms"], c["model"], c["cam"])
        assert np.all(m3 == want) and np.all(af == af[0]) and np.all(m2 == m2[0])
    r = ref.records(c["est"], c["gt"], c["syms"], c["model"], c["cam"])
    assert np.all(r["k_mssd"] == 0) and np.all(r["k_add"] == 0) and np.all(r["k_mspd"] == 0) and r["mssd"][0] == 0 and r["mssd"][1] == c["shift"]
    c = cases.exact_none_right()
    af, m3, m2 = ref.per_symmetry(c["est"][0], c["gt"][0], c["syms"], c["model"])
    assert m3[0] == c["mssd"] and m3[1] == c["mssd"] and af[0] == af[1] > 0
    r = ref.records(c["est"], c["gt"], c["syms"], c["model"])[0]
    assert r["mssd"] == c["mssd"] and r["k_mssd"] == 0 and r["k_add"] == 0


def test_projection_edges():
    c = cases.depth_edge_ground_truth()
    g = [base.transform(ref.compose(c["gt"][0], S), c["model"])[0, 2] for S in c["syms"]]
    assert g[1] == cases.EPS_Z and g[2] == np.nextafter(cases.EPS_Z, F(1))
    _, _, m2 = ref.per_symmetry(c["est"][0], c["gt"][0], c["syms"], c["model"], c["cam"])
    assert [k for k in range(4) if np.isposinf(m2[k])] == c["inf_k"] and np.all(np.isfinite(np.delete(m2, c["inf_k"])))
    c = cases.depth_edge_estimate()
    assert base.transform(c["est"][0], c["model"])[0, 2] == cases.EPS_Z
    r = ref.records(c["est"], c["gt"], c["syms"], c["model"], c["cam"])
    assert np.isposinf(r["mspd"][0]) and r["k_mspd"][0] == -1 and np.isfinite(r["mspd"][1]) and r["k_mspd"][1] >= 0 and np.all(np.isfinite(r["mssd"]))
    c = cases.behind_camera()
    r = ref.records(c["est"], c["gt"], c["syms"], c["model"], c["cam"])[0]
    assert np.isposinf(r["mspd"]) and r["k_mspd"] == -1 and np.isfinite(r["mssd"]) and r["k_mssd"] >= 0 and r["valid"] == 1
    c = cases.optical_axis()
    _, m3, m2 = ref.per_symmetry(c["est"][0], c["gt"][0], c["syms"], c["model"], c["cam"])
    assert np.all(m2 == 0) and np.all(m3 == F(0.25))
    r = ref.records(c["est"], c["gt"], c["syms"], c["model"], c["cam"])[0]
    assert r["mspd"] == 0 and r["k_mspd"] == 0 and r["mssd"] == F(0.25)


def test_saturation_and_validity():
    c = cases.far_apart()
    r = ref.records(c["est"], c["gt"], c["syms"], c["model"], c["cam"])[0]
    assert r["add_fix"] == len(c["model"]) * (1 << 47) and r["add"] == F(32768) and 0.9e5 < r["mssd"] < 1.1e5 and r["valid"] == 1 and r["k_add"] == 0
    c = cases.invalid_poses()
    r = ref.records(c["est"], c["gt"], c["syms"], c["model"], c["cam"])
    assert np.array_equal(r["valid"], c["valid"])
    bad = r[c["valid"] == 0]
    assert np.all(bad["add_fix"] == 0) and all(np.all(np.isposinf(bad[k])) for k in ("add", "mssd", "mspd"))
    assert all(np.all(bad[k] == -1) for k in ("k_add", "k_mssd", "k_mspd"))
    alone = ref.records(c["est"][[0, 2, 4, 6]], c["gt"][[0, 2, 4, 6]], c["syms"], c["model"], c["cam"])
    assert ref.records_equal(r[c["valid"] == 1], alone)


def test_sizes_cover_the_header_constants():
    k = cases.kernel_sizes()
    assert k["MAX"] == 4096 and k["THREADS"] % 64 == 0
    for v in k.values():
        assert {v - 1, v, v + 1} <= set(cases.model_sizes())
    assert {1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1025, 4097} <= set(cases.model_sizes())
    assert {1, 2, k["BLOCK"] - 1, k["BLOCK"], k["BLOCK"] + 1, 2 * k["BLOCK"] + 1, 72} <= set(cases.sym_counts())


# ---- stocs_symmetry_set (host code of the library: loads without a GPU) ----
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from model_matching_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        g.build()
    return capi.load()


def _mats(S):
    return np.asarray(S, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)


def test_symmetry_set_counts_and_exact_entries(lib):
    from model_matching_amd.estimator import symmetry_set
    for sym3, n, K in (((0, 0, 0), 72, 1), ((90, 0, 0), 72, 4), ((180, 90, 0), 72, 8), ((0, 0, 360), 72, 72), ((0, 0, 360), 5, 5), ((7, 360, 0), 3, 3)):
        S = symmetry_set(sym3, n)
        assert S.shape == (K, 16) and S.dtype == F
        assert S[0].tobytes() == ref.IDENTITY.tobytes()                       # entry 0 is the identity, +0 zeros included
        Mx = _mats(S)
        assert np.abs(Mx[:, :3, :3] @ Mx[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
        assert np.all(Mx[:, 3, :] == [0, 0, 0, 1]) and np.all(Mx[:, :3, 3] == 0)
    for sym3 in ((90, 0, 0), (180, 90, 0), (90, 90, 90), (0, 0, 360)):
        S = symmetry_set(sym3, 8)                                            # 8 steps: every second one is a multiple of 90 degrees
        quarter = S if sym3[2] != 360 else S[::2]
        assert np.all(np.isin(quarter, (0.0, 1.0, -1.0))) and not np.any(np.signbit(quarter) & (quarter == 0))
    S = symmetry_set((90, 0, 0))
    assert np.array_equal(_mats(S)[1][:3, :3], [[1, 0, 0], [0, 0, -1], [0, 1, 0]])      # x runs fastest: entry 1 is Rx(90)
    S = symmetry_set((90, 180, 0))
    assert np.array_equal(_mats(S)[4][:3, :3], [[-1, 0, 0], [0, 1, 0], [0, 0, -1]])     # entry 4 = (alpha 0, beta 180): Ry(180)
    S = symmetry_set((0, 0, 360), 72)
    assert np.abs(_mats(S)[1][:3, :3] - pc.rot((0, 0, 1), 5.0)).max() <= 1e-7


@pytest.mark.parametrize("sym3,n", [((90, 0, 0), 1), ((0, 180, 0), 1), ((0, 0, 360), 72), ((0, 360, 0), 7)])
def test_single_axis_set_is_closed_under_composition(lib, sym3, n):
    from model_matching_amd.estimator import symmetry_set
    Mx = _mats(symmetry_set(sym3, n, center=(0.01, -0.02, 0.03)))
    for a in Mx:
        for b in Mx:
            assert np.abs(Mx - (a @ b)[None]).reshape(len(Mx), -1).max(1).min() <= 1e-6


def test_symmetry_set_centre_is_a_fixed_point(lib):
    from model_matching_amd.estimator import symmetry_set
    c = np.array([0.125, -0.05, 0.3])
    for sym3 in ((0, 0, 360), (180, 90, 0)):
        Mx = _mats(symmetry_set(sym3, 9, center=c))
        assert np.abs(Mx[:, :3, :3] @ c + Mx[:, :3, 3] - c).max() <= 1e-6
        assert np.abs(Mx[1:, :3, 3]).max() > 1e-3                           # the centre is really used


def test_symmetry_set_refusals(lib):
    from model_matching_amd import capi
    s3, K = (C.c_float * 3)(180, 90, 0), C.c_int(-5)
    out = (C.c_float * (16 * 8))(*([7.0] * 128))
    assert lib.stocs_symmetry_set(s3, 72, None, out, 7, C.byref(K)) == -1 and K.value == 8 and all(v == 7.0 for v in out)    # cap < K: nothing written
    assert lib.stocs_symmetry_set(s3, 72, None, None, 0, C.byref(K)) == -1 and K.value == 8
    assert lib.stocs_symmetry_set(s3, 72, None, out, 8, C.byref(K)) == 0 and K.value == 8
    assert lib.stocs_symmetry_set(s3, 72, None, out, 8, None) == -1 and lib.stocs_symmetry_set(None, 72, None, out, 8, C.byref(K)) == -1
    s3 = (C.c_float * 3)(0, 0, 360)
    assert lib.stocs_symmetry_set(s3, 0, None, out, 8, C.byref(K)) == -1 and lib.stocs_symmetry_set(s3, -1, None, out, 8, C.byref(K)) == -1
    assert lib.stocs_symmetry_set((C.c_float * 3)(90, 0, 0), 0, None, out, 8, C.byref(K)) == 0 and K.value == 4               # no continuous axis: n is not read
    bad = (C.c_float * 3)(0.0, float("nan"), 0.0)
    assert lib.stocs_symmetry_set(s3, 4, bad, out, 8, C.byref(K)) == -1
    with pytest.raises(capi.StocsError):
        from model_matching_amd.estimator import symmetry_set
        symmetry_set((360, 0, 0), 0)


def _fold_errors(co, symmetry_set, d, s, deg):
    """-> (the clustering oracle's folded rotation error, the smallest unfolded error over the generated set) for a turn of deg about axis d"""
    sym3 = [0.0, 0.0, 0.0]; sym3[d] = float(s)
    S = symmetry_set(sym3, 360)                  # a continuous axis in 1-degree steps: the grid's angles are in the set
    K = len(S)
    turned = pc.pose(pc.rot(np.eye(3)[d], float(deg)))
    folded = co.pair_eval(co._Prep(np.stack([pc.pose(), turned])), [0], 1, 0.02, 15.0, tuple(sym3))["re"][0]
    unfolded = co.pair_eval(co._Prep(np.concatenate([S, turned[None]])), np.arange(K), K, 0.02, 15.0, (0.0, 0.0, 0.0))["re"]    # test pose k = identity o S_k
    return folded, np.nanmin(unfolded)


@pytest.mark.parametrize("d,s", [(0, 90), (1, 90), (2, 90), (0, 180), (1, 180), (2, 180), (0, 360), (1, 360), (2, 360), (1, 0)])
def test_generated_set_agrees_with_the_clustering_fold(lib, d, s):
    """rotations about axis d on a 1-degree grid: the smallest UNFOLDED rotation error over the generated set equals the clustering
    oracle's folded error for the same descriptor, to 1e-3 degrees: for x and z over the whole turn, for y only for turns of less than
    90 degrees (the next test says why)."""
    from model_matching_amd.estimator import symmetry_set
    from oracle import cluster_oracle as co
    for deg in (range(-89, 90) if d == 1 else range(-179, 180)):
        folded, unfolded = _fold_errors(co, symmetry_set, d, s, deg)
        assert abs(unfolded - folded) <= 1e-3, (deg, unfolded, folded)


@pytest.mark.parametrize("s", [90, 180, 360])
def test_beyond_a_quarter_turn_about_y_the_clustering_fold_is_not_the_set(lib, s):
    """The clustering takes the pitch of the pose difference by asin, which folds it into +-90 degrees BEFORE any symmetry is folded: a turn
    of more than 90 degrees about y reads as roll 180, pitch 180 - |deg|, yaw 180, and a y descriptor folds only the pitch, so the folded
    error is 180 degrees whatever the descriptor.  The generated set holds the true rotations about y, under which such a turn is as near
    as its angle says.  So a clustering with a y descriptor and the errors under symmetry_set of the same descriptor DISAGREE there; this
    pins it (at every angle of the grid beyond 90 degrees, and at the example Ry(100) under (0, 360, 0): 180 against 0)."""
    from model_matching_amd.estimator import symmetry_set
    from oracle import cluster_oracle as co
    for deg in list(range(-179, -90)) + list(range(91, 180)):
        folded, unfolded = _fold_errors(co, symmetry_set, 1, s, deg)
        assert abs(folded - 180.0) <= 1e-3 and unfolded <= 90.0 + 1e-3, (deg, unfolded, folded)
    if s == 360:
        folded, unfolded = _fold_errors(co, symmetry_set, 1, 360, 100)
        assert abs(folded - 180.0) <= 1e-3 and unfolded <= 1e-3


def test_pose_recall_sym():
    from model_matching_amd.estimator import _POSE_ERROR_SYM_DTYPE, pose_recall_sym
    r = np.zeros(5, _POSE_ERROR_SYM_DTYPE)
    r["valid"] = [1, 1, 1, 1, 0]
    r["mssd"] = [0.004, 0.012, 0.026, 0.2, np.inf]       # diameter 0.1: thresholds 0.005 .. 0.05 -> below 10, 8, 5, 0 of the ten
    r["mspd"] = [4.0, 12.0, 26.0, np.inf, np.inf]        # width 640: thresholds 5 .. 50 -> 10, 8, 5, 0
    r["add"] = [0.001, 0.0099, 0.0101, 0.5, np.inf]
    ar3, ar2, ra, nv = pose_recall_sym(r, 0.1, image_width=640)
    assert nv == 4 and abs(ar3 - 23 / 40) < 1e-12 and abs(ar2 - 23 / 40) < 1e-12 and ra == 0.5
    ar3, ar2, ra, nv = pose_recall_sym(r, 0.1)
    assert nv == 4 and abs(ar3 - 23 / 40) < 1e-12 and np.isnan(ar2) and ra == 0.5
    _, ar2, _, _ = pose_recall_sym(r, 0.1, image_width=1280)   # thresholds 10 .. 100 pixels -> 10, 9, 8, 0
    assert abs(ar2 - 27 / 40) < 1e-12
    assert pose_recall_sym(r[4:], 0.1)[3] == 0 and all(np.isnan(v) for v in pose_recall_sym(r[4:], 0.1)[:3])
