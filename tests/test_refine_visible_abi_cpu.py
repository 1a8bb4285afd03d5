"""CPU-side checks of the C ABI of the visible-surface refinement: struct sizes and offsets, the exported symbols with the bindings'
signatures, the header compiles as C99, the defaults, every refusal of stocs_check_refine_visible_params and the argument checks that need
no device.  No GPU compute."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"stocs_check_refine_visible_params": 1, "stocs_refine_visible_groups": 2, "stocs_refine_poses_visible": 6, "stocs_refine_visible_detail": 6,
         "stocs_refine_visible_last_device_ms": 4}
INVALID = -1


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def test_struct_sizes_and_offsets(capi):
    P, R = capi.RefineVisibleParams, capi.RefineVisibleResult
    assert C.sizeof(P) == 16 and C.sizeof(R) == 40
    assert [(getattr(P, f).offset, getattr(P, f).size) for f, _ in P._fields_] == [(0, 4), (4, 4), (8, 4), (12, 4)]
    assert [f for f, _ in P._fields_] == ["max_iterations", "max_distance", "min_view_cos", "class_threshold"]
    assert [f for f, _ in R._fields_] == ["present", "no_depth", "off_class", "too_far", "grazing", "counted", "iterations", "frozen", "rms", "reserved"]
    assert [getattr(R, f).offset for f, _ in R._fields_] == list(range(0, 40, 4))
    assert dict(R._fields_)["rms"] is C.c_float


def test_header_agrees_with_the_bindings(capi, tmp_path):
    src = tmp_path / "refine_visible_sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\n"
        "int main(void) {\n"
        "    printf(\"%d %d %d %d %d %d\\n\", (int)sizeof(stocs_refine_visible_params), (int)sizeof(stocs_refine_visible_result),\n"
        "           (int)offsetof(stocs_refine_visible_params, class_threshold), (int)offsetof(stocs_refine_visible_result, counted),\n"
        "           (int)offsetof(stocs_refine_visible_result, rms), (int)offsetof(stocs_refine_visible_result, reserved));\n"
        "    return 0;\n}\n")
    exe = tmp_path / "refine_visible_sizes"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [16, 40, 12, 20, 32, 36]


def test_library_exports_the_symbols(capi):
    lib = C.CDLL(capi.LIB_PATH)
    L = capi.load()
    assert hasattr(lib, "stocs_default_refine_visible_params") and L.stocs_default_refine_visible_params.restype is None
    for name, n_args in NAMES.items():
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args, name
    from model_matching_amd import estimator
    for name in ("refine_poses_visible", "refine_visible_detail", "refine_visible_last_device_ms"):
        assert callable(getattr(estimator.StocsEstimator, name)), name


def test_header_declares_them_as_c99(capi, tmp_path):
    src = tmp_path / "refine_visible_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* poses, float* out16, stocs_refine_visible_result* rec, uint64_t* keys, uint8_t* st, double* sums) {\n"
        "    stocs_refine_visible_params p;\n"
        "    float ms[3];\n"
        "    int rc;\n"
        "    stocs_default_refine_visible_params(&p);\n"
        "    rc = stocs_check_refine_visible_params(&p);\n"
        "    rc = rc ? rc : stocs_refine_poses_visible(c, poses, 2, &p, out16, rec);\n"
        "    rc = rc ? rc : stocs_refine_visible_detail(c, poses, &p, keys, st, sums);\n"
        "    rc = rc ? rc : stocs_refine_visible_last_device_ms(c, &ms[0], &ms[1], &ms[2]);\n"
        "    return rc ? rc : rec->counted + stocs_refine_visible_groups(640, 480) + (ms[0] > ms[2]);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_defaults_and_every_refusal_of_the_parameter_check(capi):
    L = capi.load()
    p = capi.RefineVisibleParams()
    L.stocs_default_refine_visible_params(C.byref(p))
    assert (p.max_iterations, p.max_distance, p.min_view_cos, p.class_threshold) == (5, C.c_float(0.02).value, 0.0, C.c_float(0.10).value)
    assert L.stocs_check_refine_visible_params(C.byref(p)) == 0
    assert L.stocs_check_refine_visible_params(None) == INVALID and b"NULL" in L.stocs_last_error()
    L.stocs_default_refine_visible_params(None)   # a no-op
    nan, inf = float("nan"), float("inf")
    refused = [("max_iterations", -1, b"max_iterations"), ("max_distance", 0.0, b"max_distance"), ("max_distance", -0.01, b"max_distance"),
               ("max_distance", inf, b"max_distance"), ("max_distance", nan, b"max_distance"), ("min_view_cos", -0.1, b"min_view_cos"),
               ("min_view_cos", 1.0, b"min_view_cos"), ("min_view_cos", nan, b"min_view_cos"), ("class_threshold", inf, b"class_threshold"),
               ("class_threshold", nan, b"class_threshold")]
    for field, value, word in refused:
        q = capi.RefineVisibleParams()
        L.stocs_default_refine_visible_params(C.byref(q))
        setattr(q, field, value)
        assert L.stocs_check_refine_visible_params(C.byref(q)) == INVALID, (field, value)
        assert word in L.stocs_last_error(), (field, value, L.stocs_last_error())
    accepted = [("max_iterations", 0), ("max_distance", 1e-6), ("min_view_cos", 0.0), ("min_view_cos", 0.999), ("class_threshold", -5.0)]
    for field, value in accepted:
        q = capi.RefineVisibleParams()
        L.stocs_default_refine_visible_params(C.byref(q))
        setattr(q, field, value)
        assert L.stocs_check_refine_visible_params(C.byref(q)) == 0, (field, value)


def test_groups_are_a_function_of_the_frame_size(capi):
    L = capi.load()
    assert L.stocs_refine_visible_groups(0, 5) == 0 and L.stocs_refine_visible_groups(5, -1) == 0
    for W, H in [(1, 1), (64, 48), (96, 72), (128, 96), (640, 480), (1920, 1080)]:
        assert L.stocs_refine_visible_groups(W, H) == min(64, max(1, (W * H) // 2048)), (W, H)


def test_argument_checks_that_need_no_device(capi):
    L = capi.load()
    P = (C.c_float * 16)(); out = (C.c_float * 16)(); rec = (capi.RefineVisibleResult * 1)(); sums = (C.c_double * 29)()
    p = capi.RefineVisibleParams(); L.stocs_default_refine_visible_params(C.byref(p))
    for n in (0, 1, -1):
        assert L.stocs_refine_poses_visible(None, P, n, C.byref(p), out, rec) == INVALID and b"NULL context" in L.stocs_last_error()
    assert L.stocs_refine_visible_detail(None, P, C.byref(p), None, None, sums) == INVALID and b"stocs_refine_visible_detail" in L.stocs_last_error()
    assert L.stocs_refine_visible_last_device_ms(None, None, None, None) == INVALID


def test_the_build_lists_the_new_file(capi):
    mk = open(os.path.join(ROOT, "model_matching_amd", "csrc", "Makefile")).read()
    assert "refine_visible.hip" in mk
