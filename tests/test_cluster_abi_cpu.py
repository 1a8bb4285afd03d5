"""CPU-side checks of the C ABI of the device clustering's own entry point (stocs_cluster_trials_device): the library exports it, the
header that declares it still compiles as C99, and the ctypes binding resolves it.  No GPU compute here."""
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


def test_library_exports_cluster_trials_device(capi):
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "stocs_cluster_trials_device")


def test_header_declares_cluster_trials_device_as_c99(tmp_path):
    src = tmp_path / "cluster_trials_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* P, const float* lcp, const int32_t* off, const float* best, const float* sym) {\n"
        "    int32_t out_off[3], out_cnt[2], out_idx[8], surv[2];\n"
        "    return stocs_cluster_trials_device(c, P, lcp, off, best, 2, 0.8f, 3, 0.02f, 15.0f, sym, out_off, out_cnt, out_idx, 8, surv)\n"
        "         + stocs_cluster_trials_device(c, P, lcp, off, best, 2, 0.8f, 3, 0.02f, 15.0f, sym, out_off, out_cnt, out_idx, 8, NULL);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_capi_binds_cluster_trials_device(capi):
    L = capi.load()
    fn = L.stocs_cluster_trials_device
    assert fn.restype is C.c_int and len(fn.argtypes) == 16
    assert "stocs_cluster_trials_device" in capi.SIGNATURES
    from model_matching_amd.estimator import StocsEstimator
    assert callable(getattr(StocsEstimator, "cluster_trials_device"))
