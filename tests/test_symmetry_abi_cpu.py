"""CPU-side checks of the symmetry-finding C ABI (stocs_symmetry_errors, stocs_symmetry_errors_detail, stocs_symmetry_axes,
stocs_symmetry_rotation, stocs_symmetry_close, stocs_find_symmetries): the library exports them, the header that declares them still
compiles as C99, the ctypes structs match the C layout, the bindings exist, and the host helpers do what the header says.  No GPU compute."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stocs_symmetry_errors", "stocs_symmetry_errors_detail", "stocs_symmetry_axes", "stocs_symmetry_rotation", "stocs_symmetry_close",
         "stocs_default_symmetry_search", "stocs_find_symmetries")
STRUCTS = {"stocs_symmetry_params": "SymmetryParams", "stocs_symmetry_error": "SymmetryError", "stocs_symmetry_search": "SymmetrySearch",
           "stocs_symmetry_axis": "SymmetryAxis"}
F = np.float32


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


@pytest.fixture(scope="module")
def est_mod(capi):
    from model_matching_amd import estimator
    return estimator


def test_library_exports_the_symbols(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name


def test_header_declares_them_as_c99(tmp_path):
    src = tmp_path / "symmetry_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* T, stocs_symmetry_error* out, float* s, int32_t* nn, float* dot) {\n"
        "    stocs_symmetry_params p = {0.01f, 0.5f, {0, 0}};\n"
        "    stocs_symmetry_search q;\n"
        "    stocs_symmetry_axis ax[4];\n"
        "    float axes[9], R[16], set[16 * 8], sym3[3];\n"
        "    const float z[3] = {0.0f, 0.0f, 1.0f};\n"
        "    int n = 0, K = 0, tr = 0, flags = 0;\n"
        "    int rc = stocs_symmetry_axes(3, axes, 3, &n);\n"
        "    rc = rc ? rc : stocs_symmetry_rotation(z, 90.0, NULL, R);\n"
        "    rc = rc ? rc : stocs_symmetry_close(R, 1, 1.0f, set, 8, &K, &tr);\n"
        "    rc = rc ? rc : stocs_symmetry_errors(c, T, 2, &p, out);\n"
        "    rc = rc ? rc : stocs_symmetry_errors_detail(c, T, &p, s, nn, dot);\n"
        "    stocs_default_symmetry_search(&q);\n"
        "    rc = rc ? rc : stocs_find_symmetries(c, &q, NULL, ax, 4, &n, set, 8, &K, sym3, &flags);\n"
        "    return rc ? rc : (int)out->sum_fix + (int)(out->mean + out->max) + out->n_far + out->n_normal_bad + out->valid + out->reserved + ax[0].order\n"
        "                     + STOCS_SYMMETRY_THREADS + STOCS_SYMMETRY_MAX_LAUNCH + STOCS_SYMMETRY_GRID_SPAN\n"
        "                     + (flags & (STOCS_SYMMETRY_DESCRIPTOR_INEXACT | STOCS_SYMMETRY_SET_TRUNCATED | STOCS_SYMMETRY_NOTHING_FOUND));\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_ctypes_structs_match_the_c_layout(capi, tmp_path, cname):
    S = getattr(capi, STRUCTS[cname])
    fields = [f[0] for f in S._fields_]
    src = tmp_path / "layout.c"
    body = "".join('    printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f in fields)
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\nint main(void) {\n"
                   '    printf("%%zu\\n", sizeof(%s));\n%s    return 0;\n}\n' % (cname, body))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(S) == out[0]
    assert [getattr(S, f).offset for f in fields] == out[1:]
    if cname == "stocs_symmetry_error":
        assert out[0] == 32


def test_capi_and_estimator_bind_them(capi, est_mod):
    L = capi.load()
    for name, nargs in (("stocs_symmetry_errors", 5), ("stocs_symmetry_errors_detail", 6), ("stocs_symmetry_axes", 4), ("stocs_symmetry_rotation", 4),
                        ("stocs_symmetry_close", 7), ("stocs_find_symmetries", 11)):
        assert getattr(L, name).restype is C.c_int and len(getattr(L, name).argtypes) == nargs, name
    import symmetry_ref as ref
    assert ref.DTYPE == est_mod._SYMMETRY_ERROR_DTYPE and ref.AXIS_DTYPE == est_mod._SYMMETRY_AXIS_DTYPE
    assert [n for n in ref.DTYPE.names] == [f[0] for f in capi.SymmetryError._fields_]
    for name in ("symmetry_errors", "symmetry_errors_detail", "find_symmetries"):
        assert callable(getattr(est_mod.StocsEstimator, name)), name
    for name in ("symmetry_axes", "symmetry_rotation", "symmetry_close", "symmetry_search"):
        assert callable(getattr(est_mod, name)), name
    assert (capi.SYMMETRY_DESCRIPTOR_INEXACT, capi.SYMMETRY_SET_TRUNCATED, capi.SYMMETRY_NOTHING_FOUND) == (ref.INEXACT, ref.TRUNCATED, ref.NOTHING)


def test_defaults_are_the_documented_ones(est_mod):
    import symmetry_ref as ref
    p = est_mod.symmetry_search()
    for k, v in ref.DEFAULTS.items():
        assert getattr(p, k) == (F(v) if isinstance(v, float) else v), k


def test_argument_checks_that_need_no_device(capi):
    L = capi.load()
    out = (capi.SymmetryError * 1)()
    T = (C.c_float * 16)()
    prm = capi.SymmetryParams(0.01, 0.5, (C.c_int32 * 2)(0, 0))
    assert L.stocs_symmetry_errors(None, T, 1, C.byref(prm), out) == -1
    assert L.stocs_symmetry_errors(None, T, 0, C.byref(prm), out) == -1
    assert L.stocs_symmetry_errors_detail(None, T, C.byref(prm), None, None, None) == -1
    s = capi.SymmetrySearch()
    L.stocs_default_symmetry_search(C.byref(s))
    n, K, fl = C.c_int(7), C.c_int(7), C.c_int(7)
    sym3 = (C.c_float * 3)()
    set16 = (C.c_float * 16)()
    assert L.stocs_find_symmetries(None, C.byref(s), None, None, 0, C.byref(n), set16, 1, C.byref(K), sym3, C.byref(fl)) == -1
    L.stocs_default_symmetry_search(None)   # a NULL is ignored


# ---- stocs_symmetry_axes ----
def test_axes_start_with_the_coordinate_axes_and_follow_the_formula(capi, est_mod):
    import symmetry_ref as ref
    a = est_mod.symmetry_axes(2048)
    assert a.shape == (2048, 3) and a.dtype == F
    assert np.array_equal(a[:3], np.eye(3, dtype=F))
    assert np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -23
    assert np.all(a[:, 2] >= 0) and np.all(a[3:, 2] > 0)
    assert a.tobytes() == est_mod.symmetry_axes(2048).tobytes()
    assert np.abs(a.astype(np.float64) - ref.axes(2048).astype(np.float64)).max() <= 2.0 ** -24   # the formula (libm's cos and sin may differ in the last bit)
    assert np.array_equal(est_mod.symmetry_axes(3), np.eye(3, dtype=F))
    assert np.array_equal(est_mod.symmetry_axes(100), ref.axes(100)) or np.abs(est_mod.symmetry_axes(100) - ref.axes(100)).max() <= 2.0 ** -24
    # every direction has a lattice neighbour within twice the nominal spacing, none nearer than a third of it
    d = a[3:].astype(np.float64)
    c = np.clip(d @ d.T, -1, 1); np.fill_diagonal(c, -1)
    near = np.arccos(c.max(1))
    sp = ref.lattice_spacing(2048)
    assert near.max() <= 2 * sp and near.min() >= sp / 3


def test_axes_refuse_and_write_nothing(capi):
    L = capi.load()
    buf = np.full((8, 3), 7, F)
    n = C.c_int(-5)
    assert L.stocs_symmetry_axes(8, buf.ctypes.data_as(capi._fp), 7, C.byref(n)) == -1 and n.value == 8 and np.all(buf == 7)
    assert L.stocs_symmetry_axes(8, None, 8, C.byref(n)) == -1 and n.value == 8
    assert L.stocs_symmetry_axes(2, buf.ctypes.data_as(capi._fp), 8, C.byref(n)) == -1 and n.value == 0 and np.all(buf == 7)
    assert L.stocs_symmetry_axes(8, buf.ctypes.data_as(capi._fp), 8, None) == -1


# ---- stocs_symmetry_rotation ----
def test_quarter_turns_about_coordinate_axes_are_exact(est_mod):
    for d in range(3):
        axis = np.eye(3)[d]
        for k in range(-4, 9):
            R = est_mod.symmetry_rotation(axis, 90.0 * k)
            assert set(np.unique(R)) <= {F(-1), F(0), F(1)} and not np.any(np.signbit(R) & (R == 0))
            want = np.rint(__import__("pose_error_cases").rot(axis, 90.0 * k))
            assert np.array_equal(R.reshape(4, 4).T[:3, :3], want.astype(F))
    S = est_mod.symmetry_set((0, 0, 90))
    for k in range(4):
        assert np.array_equal(est_mod.symmetry_rotation((0, 0, 1), 90.0 * k), S[k])
    c = (0.25, -0.5, 2.0)
    S = est_mod.symmetry_set((0, 0, 90), center=c)
    for k in range(4):
        assert np.array_equal(est_mod.symmetry_rotation((0, 0, 5), 90.0 * k, c), S[k])


def test_rotation_follows_the_formula_and_refuses(capi, est_mod):
    import symmetry_ref as ref
    rng = np.random.default_rng(3)
    for _ in range(20):
        a, ang, c = rng.normal(size=3).astype(F), float(rng.uniform(-400, 400)), rng.normal(0, 0.1, 3).astype(F)
        got, want = est_mod.symmetry_rotation(a, ang, c), ref.rotation(a, ang, c)
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23
        R = got.reshape(4, 4).T.astype(np.float64)
        assert np.abs(R[:3, :3] @ R[:3, :3].T - np.eye(3)).max() < 1e-6 and np.abs(R[:3, :3] @ c + R[:3, 3] - c).max() < 1e-6
        assert np.array_equal(got[[3, 7, 11, 15]], np.array([0, 0, 0, 1], F))
    L = capi.load()
    out = (C.c_float * 16)()
    zero, nan = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(float("nan"), 0, 1)
    z = (C.c_float * 3)(0, 0, 1)
    assert L.stocs_symmetry_rotation(zero, 90.0, None, out) == -1 and L.stocs_symmetry_rotation(nan, 90.0, None, out) == -1
    assert L.stocs_symmetry_rotation(z, float("inf"), None, out) == -1 and L.stocs_symmetry_rotation(z, 90.0, nan, out) == -1
    assert L.stocs_symmetry_rotation(None, 90.0, None, out) == -1 and L.stocs_symmetry_rotation(z, 90.0, None, None) == -1


# ---- stocs_symmetry_close ----
def _is_group(S):
    M = [s.reshape(4, 4).T.astype(np.float64) for s in S]
    for a in M:
        for b in M:
            if min(np.abs(a @ b - c).max() for c in M) > 1e-5:
                return False
    return True


def test_close_builds_the_groups(est_mod):
    import symmetry_ref as ref
    rot = est_mod.symmetry_rotation
    S, tr = est_mod.symmetry_close([rot((0, 0, 1), 90.0)], 1.0)
    assert len(S) == 4 and not tr and np.array_equal(S[0], ref.IDENTITY)
    assert np.array_equal(S, np.stack([rot((0, 0, 1), 90.0 * k) for k in range(4)]))   # breadth first: the powers in order, exact
    S, tr = est_mod.symmetry_close([rot((1, 0, 0), 180.0), rot((0, 1, 0), 180.0), rot((0, 0, 1), 180.0)], 1.0)
    assert len(S) == 4 and not tr and np.array_equal(S[0], ref.IDENTITY) and _is_group(S)
    assert np.array_equal(S, est_mod.symmetry_close([rot((1, 0, 0), 180.0), rot((0, 1, 0), 180.0)], 1.0)[0][[0, 1, 2, 3]])
    steps = [rot((0, 0, 1), 5.0 * k) for k in range(72)]
    S, tr = est_mod.symmetry_close(steps + [rot((1, 0, 0), 180.0)], 1.25)
    assert len(S) == 144 and not tr and _is_group(S)
    S1, _ = est_mod.symmetry_close([rot((0, 0, 1), 5.0), rot((1, 0, 0), 180.0)], 1.25)
    assert len(S1) == 144
    c = (0.01, -0.02, 0.03)
    S, tr = est_mod.symmetry_close([rot((0.3, -0.5, 0.81), 120.0, c)], 1.0)
    assert len(S) == 3 and not tr and _is_group(S)
    again, _ = est_mod.symmetry_close([rot((0.3, -0.5, 0.81), 120.0, c)] * 2, 1.0)
    assert np.array_equal(S, again)                                                   # a duplicated generator changes nothing
    S, tr = est_mod.symmetry_close(np.zeros((0, 16), F), 1.0)
    assert len(S) == 1 and not tr and np.array_equal(S[0], ref.IDENTITY)
    for gens, deg in (([rot((0, 0, 1), 90.0)], 1.0), ([rot((0, 0, 1), 5.0), rot((1, 0, 0), 180.0)], 1.25), ([rot((0.3, -0.5, 0.81), 120.0, c)], 1.0)):
        got, want = est_mod.symmetry_close(gens, deg)[0], ref.close(gens, deg)[0]
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-6


def test_close_truncates_at_its_cap(capi, est_mod):
    rot = est_mod.symmetry_rotation
    S, tr = est_mod.symmetry_close([rot((0, 0, 1), 5.0), rot((1, 0, 0), 180.0)], 1.25, cap=100)
    assert len(S) == 100 and tr
    S, tr = est_mod.symmetry_close([rot((0, 0, 1), 5.0), rot((1, 0, 0), 180.0)], 1.25, cap=144)
    assert len(S) == 144 and not tr
    S, tr = est_mod.symmetry_close([rot((0, 0, 1), 5.0), rot((1, 0, 0), 5.0)], 1.25, cap=300)   # two continuous axes: a sphere
    assert len(S) == 300 and tr
    L = capi.load()
    K, t = C.c_int(0), C.c_int(0)
    out = np.empty((4, 16), F)
    g = rot((0, 0, 1), 90.0)
    gp = g.ctypes.data_as(capi._fp)
    assert L.stocs_symmetry_close(gp, 1, 1.0, out.ctypes.data_as(capi._fp), 0, C.byref(K), C.byref(t)) == -1
    assert L.stocs_symmetry_close(gp, 1, 1.0, out.ctypes.data_as(capi._fp), 4097, C.byref(K), C.byref(t)) == -1
    assert L.stocs_symmetry_close(gp, 1, 1.0, None, 4, C.byref(K), C.byref(t)) == -1
    assert L.stocs_symmetry_close(None, 1, 1.0, out.ctypes.data_as(capi._fp), 4, C.byref(K), C.byref(t)) == -1
    assert L.stocs_symmetry_close(gp, 1, 1.0, out.ctypes.data_as(capi._fp), 4, None, C.byref(t)) == -1
    bad = g.copy(); bad[5] = np.nan
    assert L.stocs_symmetry_close(bad.ctypes.data_as(capi._fp), 1, 1.0, out.ctypes.data_as(capi._fp), 4, C.byref(K), C.byref(t)) == -1
