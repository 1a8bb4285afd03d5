"""CPU-side checks of the C ABI of the contour term of the visible-surface refinement: the exported symbols with the bindings'
signatures, struct sizes and offsets against the header compiled as C99, the defaults, every refusal of
stocs_check_refine_visible_contour_params with the damped parameters in front, and the argument checks that need no device.  The
refusals that need a context ("no mesh", "no frame", "no class image") are in tests/test_refine_visible_contour_gpu.py.  No GPU compute."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def _defaults(capi):
    p = capi.RefineVisibleContourParams()
    capi.load().stocs_default_refine_visible_contour_params(C.byref(p))
    return p


def test_struct_sizes_and_offsets(capi):
    P, R = capi.RefineVisibleContourParams, capi.RefineVisibleContourResult
    assert (C.sizeof(P), C.sizeof(R)) == (64, 80)
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("damped", 0), ("contour_weight", 52), ("pull_radius_px", 56), ("pull_distance", 60)]
    assert [(f, getattr(R, f).offset) for f, _ in R._fields_] == [("damped", 0), ("object_px", 56), ("uncovered", 60), ("unreached", 64), ("beyond", 68), ("pulled", 72),
                                                                   ("pull_rms", 76)]
    assert dict(P._fields_)["damped"] is capi.RefineVisibleDampedParams and dict(R._fields_)["damped"] is capi.RefineVisibleDampedResult
    from model_matching_amd import estimator
    D = estimator._REFINE_VISIBLE_CONTOUR_DTYPE
    assert D.itemsize == 80 and D.fields["object_px"][1] == 56 and D.fields["pull_rms"][1] == 76 and D.fields["evaluations"][1] == 40


def test_header_agrees_with_the_bindings(capi, tmp_path):
    src = tmp_path / "refine_visible_contour_sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\n"
        "int main(void) {\n"
        "    printf(\"%d %d %d %d %d %d %d %d\\n\", (int)sizeof(stocs_refine_visible_contour_params), (int)sizeof(stocs_refine_visible_contour_result),\n"
        "           (int)offsetof(stocs_refine_visible_contour_params, contour_weight), (int)offsetof(stocs_refine_visible_contour_params, pull_radius_px),\n"
        "           (int)offsetof(stocs_refine_visible_contour_params, pull_distance), (int)offsetof(stocs_refine_visible_contour_result, object_px),\n"
        "           (int)offsetof(stocs_refine_visible_contour_result, pulled), (int)offsetof(stocs_refine_visible_contour_result, pull_rms));\n"
        "    return 0;\n}\n")
    exe = tmp_path / "refine_visible_contour_sizes"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [64, 80, 52, 56, 60, 56, 72, 76]


def test_library_exports_the_symbols(capi):
    lib = C.CDLL(capi.LIB_PATH)
    L = capi.load()
    assert hasattr(lib, "stocs_default_refine_visible_contour_params") and L.stocs_default_refine_visible_contour_params.restype is None
    for name, n_args in {"stocs_check_refine_visible_contour_params": 1, "stocs_refine_poses_visible_contour": 7, "stocs_refine_visible_contour_detail": 6,
                         "stocs_refine_visible_contour_last_device_ms": 2}.items():
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args, name
    from model_matching_amd import estimator
    assert callable(estimator.StocsEstimator.refine_poses_visible_contour) and callable(estimator.StocsEstimator.refine_visible_contour_detail)


def test_header_declares_them_as_c99(capi, tmp_path):
    src = tmp_path / "refine_visible_contour_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* poses, float* out16, stocs_refine_visible_contour_result* rec, stocs_refine_visible_trace* tr, uint8_t* st, int32_t* nn,\n"
        "         double* sums) {\n"
        "    stocs_refine_visible_contour_params p;\n"
        "    int rc;\n"
        "    stocs_default_refine_visible_contour_params(&p);\n"
        "    p.damped.base.max_iterations = 3; p.pull_radius_px = 64; p.contour_weight = 0.25f; p.pull_distance = 0.05f;\n"
        "    rc = stocs_check_refine_visible_contour_params(&p);\n"
        "    rc = rc ? rc : stocs_refine_poses_visible_contour(c, poses, 2, &p, out16, rec, tr);\n"
        "    rc = rc ? rc : stocs_refine_poses_visible_contour(c, poses, 2, &p, out16, rec, NULL);\n"
        "    rc = rc ? rc : stocs_refine_visible_contour_detail(c, poses, &p, st, nn, sums);\n"
        "    return rc ? rc : rec->damped.base.counted + rec->object_px + rec->uncovered + rec->unreached + rec->beyond + rec->pulled + (rec->pull_rms > 0.0f);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_defaults(capi):
    p = _defaults(capi)
    f = lambda x: C.c_float(x).value
    d = capi.RefineVisibleDampedParams()
    capi.load().stocs_default_refine_visible_damped_params(C.byref(d))
    assert bytes(p.damped) == bytes(d)
    assert (p.contour_weight, p.pull_radius_px, p.pull_distance) == (1.0, 16, f(0.03))
    assert capi.load().stocs_check_refine_visible_contour_params(C.byref(p)) == 0
    capi.load().stocs_default_refine_visible_contour_params(None)   # a no-op


def test_every_refusal_of_the_parameter_check(capi):
    L = capi.load()
    assert L.stocs_check_refine_visible_contour_params(None) == INVALID and b"NULL" in L.stocs_last_error()
    nan, inf = float("nan"), float("inf")
    refused = [("damped.base.max_distance", 0.0, b"max_distance"), ("damped.base.max_iterations", -1, b"max_iterations"), ("damped.lambda_up", 0.5, b"lambda_up"),
               ("damped.pivot", 2, b"pivot"),
               ("contour_weight", -0.5, b"contour_weight"), ("contour_weight", inf, b"contour_weight"), ("contour_weight", nan, b"contour_weight"),
               ("pull_radius_px", 0, b"pull_radius_px"), ("pull_radius_px", -3, b"pull_radius_px"), ("pull_radius_px", 65, b"pull_radius_px"),
               ("pull_distance", 0.0, b"pull_distance"), ("pull_distance", -0.01, b"pull_distance"), ("pull_distance", inf, b"pull_distance"),
               ("pull_distance", nan, b"pull_distance")]

    def put(q, field, value):
        obj = q
        parts = field.split(".")
        for name in parts[:-1]:
            obj = getattr(obj, name)
        setattr(obj, parts[-1], value)

    for field, value, word in refused:
        q = _defaults(capi)
        put(q, field, value)
        assert L.stocs_check_refine_visible_contour_params(C.byref(q)) == INVALID, (field, value)
        assert word in L.stocs_last_error() and b"stocs_check_refine_visible_contour_params" in L.stocs_last_error(), (field, value, L.stocs_last_error())
    for field, value in [("contour_weight", 0.0), ("contour_weight", 4.0), ("pull_radius_px", 1), ("pull_radius_px", 64), ("pull_distance", 1e-6),
                         ("damped.base.max_iterations", 0)]:
        q = _defaults(capi)
        put(q, field, value)
        assert L.stocs_check_refine_visible_contour_params(C.byref(q)) == 0, (field, value)
    # the order: the plain parameters, the damped ones, the new ones
    q = _defaults(capi)
    q.damped.base.max_distance = 0.0; q.damped.lambda0 = -1.0; q.pull_radius_px = 0
    assert L.stocs_check_refine_visible_contour_params(C.byref(q)) == INVALID and b"max_distance" in L.stocs_last_error()
    q.damped.base.max_distance = 0.02
    assert L.stocs_check_refine_visible_contour_params(C.byref(q)) == INVALID and b"lambda0" in L.stocs_last_error()
    q.damped.lambda0 = 1.0; q.contour_weight = -1.0
    assert L.stocs_check_refine_visible_contour_params(C.byref(q)) == INVALID and b"contour_weight" in L.stocs_last_error()
    q.contour_weight = 1.0
    assert L.stocs_check_refine_visible_contour_params(C.byref(q)) == INVALID and b"pull_radius_px" in L.stocs_last_error()


def test_argument_checks_that_need_no_device(capi):
    L = capi.load()
    P = (C.c_float * 16)(); out = (C.c_float * 16)(); rec = (capi.RefineVisibleContourResult * 1)(); sums = (C.c_double * 29)()
    p = _defaults(capi)
    for n in (0, 1, -1):
        assert L.stocs_refine_poses_visible_contour(None, P, n, C.byref(p), out, rec, None) == INVALID and b"NULL context" in L.stocs_last_error()
        assert b"stocs_refine_poses_visible_contour" in L.stocs_last_error()
    assert L.stocs_refine_visible_contour_detail(None, P, C.byref(p), None, None, sums) == INVALID and b"stocs_refine_visible_contour_detail" in L.stocs_last_error()
    assert L.stocs_refine_visible_contour_last_device_ms(None, None) == INVALID
