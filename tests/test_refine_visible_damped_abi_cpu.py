"""CPU-side checks of the C ABI of the damped visible-surface refinement: the exported symbols with the bindings' signatures, struct
sizes and offsets against the header compiled as C99, the defaults, every refusal of stocs_check_refine_visible_damped_params and the
argument checks that need no device.  No GPU compute."""
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
    p = capi.RefineVisibleDampedParams()
    capi.load().stocs_default_refine_visible_damped_params(C.byref(p))
    return p


def test_struct_sizes_and_offsets(capi):
    P, R, T = capi.RefineVisibleDampedParams, capi.RefineVisibleDampedResult, capi.RefineVisibleTrace
    assert (C.sizeof(P), C.sizeof(R), C.sizeof(T)) == (52, 56, 88)
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("base", 0), ("lambda0", 16), ("lambda_down", 20), ("lambda_up", 24), ("max_step_rotation", 28),
                                                                   ("max_step_translation", 32), ("pivot", 36), ("pivot_model", 40)]
    assert [(f, getattr(R, f).offset) for f, _ in R._fields_] == [("base", 0), ("evaluations", 40), ("rejected", 44), ("cost", 48), ("lambda_", 52)]
    assert [(f, getattr(T, f).offset) for f, _ in T._fields_] == [("pose", 0), ("cost", 64), ("lambda_", 72), ("accepted", 80), ("state", 84)]
    assert dict(P._fields_)["base"] is capi.RefineVisibleParams and dict(R._fields_)["base"] is capi.RefineVisibleResult
    from model_matching_amd import estimator
    assert estimator._REFINE_VISIBLE_DAMPED_DTYPE.itemsize == 56 and estimator._REFINE_VISIBLE_TRACE_DTYPE.itemsize == 88
    assert estimator._REFINE_VISIBLE_TRACE_DTYPE.fields["cost"][1] == 64 and estimator._REFINE_VISIBLE_DAMPED_DTYPE.fields["evaluations"][1] == 40


def test_header_agrees_with_the_bindings(capi, tmp_path):
    src = tmp_path / "refine_visible_damped_sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\n"
        "int main(void) {\n"
        "    printf(\"%d %d %d %d %d %d %d %d %d %d\\n\", (int)sizeof(stocs_refine_visible_damped_params), (int)sizeof(stocs_refine_visible_damped_result),\n"
        "           (int)sizeof(stocs_refine_visible_trace), (int)offsetof(stocs_refine_visible_damped_params, lambda0),\n"
        "           (int)offsetof(stocs_refine_visible_damped_params, pivot), (int)offsetof(stocs_refine_visible_damped_params, pivot_model),\n"
        "           (int)offsetof(stocs_refine_visible_damped_result, evaluations), (int)offsetof(stocs_refine_visible_damped_result, lambda),\n"
        "           (int)offsetof(stocs_refine_visible_trace, cost), (int)offsetof(stocs_refine_visible_trace, state));\n"
        "    return 0;\n}\n")
    exe = tmp_path / "refine_visible_damped_sizes"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [52, 56, 88, 16, 36, 40, 40, 52, 64, 84]


def test_library_exports_the_symbols(capi):
    lib = C.CDLL(capi.LIB_PATH)
    L = capi.load()
    assert hasattr(lib, "stocs_default_refine_visible_damped_params") and L.stocs_default_refine_visible_damped_params.restype is None
    for name, n_args in {"stocs_check_refine_visible_damped_params": 1, "stocs_refine_poses_visible_damped": 7}.items():
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args, name
    from model_matching_amd import estimator
    assert callable(estimator.StocsEstimator.refine_poses_visible_damped)


def test_header_declares_them_as_c99(capi, tmp_path):
    src = tmp_path / "refine_visible_damped_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* poses, float* out16, stocs_refine_visible_damped_result* rec, stocs_refine_visible_trace* tr) {\n"
        "    stocs_refine_visible_damped_params p;\n"
        "    int rc;\n"
        "    stocs_default_refine_visible_damped_params(&p);\n"
        "    p.base.max_iterations = 3; p.pivot_model[2] = 0.01f;\n"
        "    rc = stocs_check_refine_visible_damped_params(&p);\n"
        "    rc = rc ? rc : stocs_refine_poses_visible_damped(c, poses, 2, &p, out16, rec, tr);\n"
        "    rc = rc ? rc : stocs_refine_poses_visible_damped(c, poses, 2, &p, out16, rec, NULL);\n"
        "    return rc ? rc : rec->base.counted + rec->evaluations + rec->rejected + (rec->cost > rec->lambda) + tr[7].accepted + (tr[7].cost > tr[7].lambda);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_defaults(capi):
    p = _defaults(capi)
    f = lambda x: C.c_float(x).value
    assert (p.base.max_iterations, p.base.max_distance, p.base.min_view_cos, p.base.class_threshold) == (5, f(0.02), 0.0, f(0.10))
    assert (p.lambda0, p.lambda_down, p.lambda_up) == (1.0, 4.0, 16.0)
    assert abs(p.max_step_rotation - 5.0 * 3.141592653589793 / 180.0) <= 2.0 ** -27 and p.max_step_translation == f(0.01)
    assert p.pivot == 1 and list(p.pivot_model) == [0.0, 0.0, 0.0]
    assert capi.load().stocs_check_refine_visible_damped_params(C.byref(p)) == 0
    capi.load().stocs_default_refine_visible_damped_params(None)   # a no-op


def test_every_refusal_of_the_parameter_check(capi):
    L = capi.load()
    assert L.stocs_check_refine_visible_damped_params(None) == INVALID and b"NULL" in L.stocs_last_error()
    nan, inf = float("nan"), float("inf")
    refused = [("base.max_iterations", -1, b"max_iterations"), ("base.max_distance", 0.0, b"max_distance"), ("base.max_distance", inf, b"max_distance"),
               ("base.min_view_cos", 1.0, b"min_view_cos"), ("base.class_threshold", nan, b"class_threshold"),
               ("lambda0", -0.5, b"lambda0"), ("lambda0", inf, b"lambda0"), ("lambda0", nan, b"lambda0"),
               ("lambda_down", 0.99, b"lambda_down"), ("lambda_down", inf, b"lambda_down"), ("lambda_down", nan, b"lambda_down"),
               ("lambda_up", 0.5, b"lambda_up"), ("lambda_up", inf, b"lambda_up"), ("lambda_up", nan, b"lambda_up"),
               ("max_step_rotation", 0.0, b"max_step_rotation"), ("max_step_rotation", -1.0, b"max_step_rotation"), ("max_step_rotation", nan, b"max_step_rotation"),
               ("max_step_translation", 0.0, b"max_step_translation"), ("max_step_translation", -0.01, b"max_step_translation"),
               ("max_step_translation", nan, b"max_step_translation"), ("pivot", 2, b"pivot"), ("pivot", -1, b"pivot"),
               ("pivot_model.0", nan, b"pivot_model"), ("pivot_model.1", inf, b"pivot_model"), ("pivot_model.2", -inf, b"pivot_model")]

    def put(q, field, value):
        head, _, tail = field.partition(".")
        if head == "base":
            setattr(q.base, tail, value)
        elif head == "pivot_model":
            q.pivot_model[int(tail)] = value
        else:
            setattr(q, head, value)

    for field, value, word in refused:
        q = _defaults(capi)
        put(q, field, value)
        assert L.stocs_check_refine_visible_damped_params(C.byref(q)) == INVALID, (field, value)
        assert word in L.stocs_last_error(), (field, value, L.stocs_last_error())
    accepted = [("base.max_iterations", 0), ("lambda0", 0.0), ("lambda_down", 1.0), ("lambda_up", 1.0), ("max_step_rotation", inf), ("max_step_translation", inf),
                ("max_step_rotation", 1e-6), ("pivot", 0), ("pivot_model.1", -3.5)]
    for field, value in accepted:
        q = _defaults(capi)
        put(q, field, value)
        assert L.stocs_check_refine_visible_damped_params(C.byref(q)) == 0, (field, value)
    # the base parameters are checked in front of the new ones
    q = _defaults(capi)
    q.base.max_distance = 0.0; q.lambda0 = -1.0
    assert L.stocs_check_refine_visible_damped_params(C.byref(q)) == INVALID and b"max_distance" in L.stocs_last_error()


def test_argument_checks_that_need_no_device(capi):
    L = capi.load()
    P = (C.c_float * 16)(); out = (C.c_float * 16)(); rec = (capi.RefineVisibleDampedResult * 1)()
    p = _defaults(capi)
    for n in (0, 1, -1):
        assert L.stocs_refine_poses_visible_damped(None, P, n, C.byref(p), out, rec, None) == INVALID and b"NULL context" in L.stocs_last_error()
        assert b"stocs_refine_poses_visible_damped" in L.stocs_last_error()
