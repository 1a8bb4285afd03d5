"""CPU-side checks of the batched pose refinement's C ABI (stocs_refine_poses and its detail form stocs_refine_detail): the library
exports them, the header that declares them still compiles as C99, and the ctypes binding resolves them.  No GPU compute here."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def test_library_exports_refine_poses(capi):
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "stocs_refine_poses")


def test_header_declares_refine_poses_as_c99(tmp_path):
    src = tmp_path / "refine_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* T, float* out) {\n"
        "    int32_t nc[1], it[1]; float lcp[1];\n"
        "    return stocs_refine_poses(c, T, 1, NULL, 0, 5, 0.035f, out, NULL, lcp, nc, it);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_capi_binds_refine_poses(capi):
    L = capi.load()
    fn = L.stocs_refine_poses
    assert fn.restype is C.c_int and len(fn.argtypes) == 12
    assert "stocs_refine_poses" in capi.SIGNATURES
    from model_matching_amd.estimator import StocsEstimator
    assert callable(getattr(StocsEstimator, "refine_poses"))


def test_library_exports_refine_detail(capi):
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "stocs_refine_detail")


def test_header_declares_refine_detail_as_c99(tmp_path):
    src = tmp_path / "refine_detail_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* T, const int32_t* idx) {\n"
        "    int32_t match[4]; uint8_t counted[4]; double sums[28];\n"
        "    return stocs_refine_detail(c, T, idx, 4, 0.035f, match, counted, sums) + stocs_refine_detail(c, T, NULL, 0, 0.035f, match, counted, NULL);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_capi_binds_refine_detail(capi):
    L = capi.load()
    fn = L.stocs_refine_detail
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    assert "stocs_refine_detail" in capi.SIGNATURES
    from model_matching_amd.estimator import StocsEstimator
    assert callable(getattr(StocsEstimator, "refine_detail"))
