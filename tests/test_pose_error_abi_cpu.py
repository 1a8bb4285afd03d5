"""CPU-side checks of the pose-error C ABI (stocs_pose_errors, stocs_pose_errors_detail, stocs_model_diameter): the library exports them,
the header that declares them still compiles as C99, and the ctypes struct matches the C layout.  No GPU compute here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stocs_pose_errors", "stocs_pose_errors_detail", "stocs_model_diameter")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def test_library_exports_pose_error_symbols(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name


def test_header_declares_pose_errors_as_c99(tmp_path):
    src = tmp_path / "pose_error_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* est, const float* gt, stocs_pose_error* out, float* e, float* s, int32_t* nn) {\n"
        "    float d;\n"
        "    int rc = stocs_pose_errors(c, est, 2, gt, 1, out);\n"
        "    rc = rc ? rc : stocs_pose_errors_detail(c, est, gt, e, s, nn);\n"
        "    rc = rc ? rc : stocs_model_diameter(c, &d);\n"
        "    return rc ? rc : (int)(out->add_fix + out->adds_fix) + (int)(out->add + out->add_max + out->adds + out->adds_max + d) + out->valid + out->reserved\n"
        "                     + STOCS_POSE_ERROR_THREADS + STOCS_POSE_ERROR_CHUNK + STOCS_POSE_ERROR_TILE;\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ctypes_struct_matches_the_c_layout(capi, tmp_path):
    S = capi.PoseError
    fields = [f[0] for f in S._fields_]
    src = tmp_path / "layout.c"
    body = "".join('    printf("%%zu\\n", offsetof(stocs_pose_error, %s));\n' % f for f in fields)
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\nint main(void) {\n"
                   '    printf("%%zu\\n", sizeof(stocs_pose_error));\n%s    return 0;\n}\n' % body)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(S) == out[0] == 40
    assert [getattr(S, f).offset for f in fields] == out[1:]


def test_capi_and_estimator_bind_the_pose_errors(capi):
    L = capi.load()
    assert L.stocs_pose_errors.restype is C.c_int and len(L.stocs_pose_errors.argtypes) == 6
    assert L.stocs_pose_errors_detail.restype is C.c_int and len(L.stocs_pose_errors_detail.argtypes) == 6
    assert L.stocs_model_diameter.restype is C.c_int and len(L.stocs_model_diameter.argtypes) == 2
    from model_matching_amd import estimator
    assert estimator._POSE_ERROR_DTYPE.itemsize == C.sizeof(capi.PoseError)
    assert [n for n in estimator._POSE_ERROR_DTYPE.names] == [f[0] for f in capi.PoseError._fields_]
    for name in ("pose_errors", "pose_errors_detail", "model_diameter"):
        assert callable(getattr(estimator.StocsEstimator, name)), name
    assert callable(estimator.pose_recall)


def test_the_test_restatement_has_the_same_record(capi):
    import sys
    if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import pose_error_ref as ref
    from model_matching_amd import estimator
    assert ref.DTYPE == estimator._POSE_ERROR_DTYPE


def test_argument_checks_that_need_no_device(capi):
    """NULL context: STOCS_ERR_INVALID from all three calls before anything touches a device; n == 0 with a NULL context is still invalid"""
    L = capi.load()
    out = (capi.PoseError * 1)()
    P = (C.c_float * 16)()
    d = C.c_float()
    assert L.stocs_pose_errors(None, P, 1, P, 1, out) == -1
    assert L.stocs_pose_errors_detail(None, P, P, None, None, None) == -1
    assert L.stocs_model_diameter(None, C.byref(d)) == -1


def test_pose_recall():
    from model_matching_amd.estimator import _POSE_ERROR_DTYPE, pose_recall
    r = np.zeros(5, _POSE_ERROR_DTYPE)
    r["valid"] = [1, 1, 1, 1, 0]
    r["add"] = [0.001, 0.0099, 0.0101, 0.5, np.inf]
    r["adds"] = [0.001, 0.002, 0.003, 0.0099, np.inf]
    ra, rs, nv = pose_recall(r, 0.1, k=0.1)      # threshold 0.01, strict
    assert nv == 4 and ra == 0.5 and rs == 1.0
    ra, rs, nv = pose_recall(r[4:], 0.1)
    assert nv == 0 and np.isnan(ra) and np.isnan(rs)
