"""CPU-side checks of the symmetry-aware pose-error C ABI (stocs_pose_errors_sym, stocs_pose_errors_sym_detail, stocs_symmetry_set): the
library exports them, the header that declares them still compiles as C99, and the ctypes struct matches the C layout.  No GPU compute."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stocs_pose_errors_sym", "stocs_pose_errors_sym_detail", "stocs_symmetry_set")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def test_library_exports_the_symbols(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name


def test_header_declares_them_as_c99(tmp_path):
    src = tmp_path / "pose_error_sym_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* est, const float* gt, const stocs_camera* cam, stocs_pose_error_sym* out, uint64_t* af, float* m3, float* m2) {\n"
        "    float sym[16 * 4];\n"
        "    const float d[3] = {0.0f, 0.0f, 90.0f};\n"
        "    int K = 0;\n"
        "    int rc = stocs_symmetry_set(d, 1, NULL, sym, 4, &K);\n"
        "    rc = rc ? rc : stocs_pose_errors_sym(c, est, 2, gt, 1, sym, K, cam, out);\n"
        "    rc = rc ? rc : stocs_pose_errors_sym_detail(c, est, gt, sym, K, NULL, af, m3, m2);\n"
        "    return rc ? rc : (int)out->add_fix + (int)(out->add + out->mssd + out->mspd + out->reserved_f) + out->k_add + out->k_mssd + out->k_mspd + out->valid\n"
        "                     + STOCS_POSE_SYM_MAX + STOCS_POSE_SYM_THREADS + STOCS_POSE_SYM_BLOCK;\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ctypes_struct_matches_the_c_layout(capi, tmp_path):
    S = capi.PoseErrorSym
    fields = [f[0] for f in S._fields_]
    src = tmp_path / "layout.c"
    body = "".join('    printf("%%zu\\n", offsetof(stocs_pose_error_sym, %s));\n' % f for f in fields)
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\nint main(void) {\n"
                   '    printf("%%zu\\n", sizeof(stocs_pose_error_sym));\n%s    return 0;\n}\n' % body)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(S) == out[0] == 40
    assert [getattr(S, f).offset for f in fields] == out[1:]


def test_capi_and_estimator_bind_them(capi):
    L = capi.load()
    assert L.stocs_pose_errors_sym.restype is C.c_int and len(L.stocs_pose_errors_sym.argtypes) == 9
    assert L.stocs_pose_errors_sym_detail.restype is C.c_int and len(L.stocs_pose_errors_sym_detail.argtypes) == 9
    assert L.stocs_symmetry_set.restype is C.c_int and len(L.stocs_symmetry_set.argtypes) == 6
    from model_matching_amd import estimator
    assert estimator._POSE_ERROR_SYM_DTYPE.itemsize == C.sizeof(capi.PoseErrorSym)
    assert [n for n in estimator._POSE_ERROR_SYM_DTYPE.names] == [f[0] for f in capi.PoseErrorSym._fields_]
    for name in ("pose_errors_sym", "pose_errors_sym_detail"):
        assert callable(getattr(estimator.StocsEstimator, name)), name
    assert callable(estimator.symmetry_set) and callable(estimator.pose_recall_sym)


def test_the_test_restatement_has_the_same_record(capi):
    if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import pose_error_sym_ref as ref
    from model_matching_amd import estimator
    assert ref.DTYPE == estimator._POSE_ERROR_SYM_DTYPE


def test_argument_checks_that_need_no_device(capi):
    """a NULL context is STOCS_ERR_INVALID from both device calls before anything touches a device, whatever n"""
    L = capi.load()
    out = (capi.PoseErrorSym * 1)()
    P = (C.c_float * 16)()
    assert L.stocs_pose_errors_sym(None, P, 1, P, 1, P, 1, None, out) == -1
    assert L.stocs_pose_errors_sym(None, P, 0, P, 1, P, 1, None, out) == -1
    assert L.stocs_pose_errors_sym_detail(None, P, P, P, 1, None, None, None, None) == -1
