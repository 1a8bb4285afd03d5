"""CPU-side checks of the robust refinement's C ABI (stocs_refine_poses_robust, stocs_refine_robust_detail and the workspace query):
the library exports them, the header that declares them compiles as C99, the parameter struct is 16 bytes on both sides, and the ctypes
binding resolves them.  No GPU compute here."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def test_library_exports_the_robust_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("stocs_refine_poses_robust", "stocs_refine_robust_detail", "stocs_refine_robust_workspace"):
        assert hasattr(lib, name), name


def test_header_declares_them_as_c99(tmp_path):
    src = tmp_path / "refine_robust_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* T, const int32_t* idx, float* out) {\n"
        "    stocs_refine_robust_params p;\n"
        "    int32_t nc[1], ncand[1], it[1], match[4], k, n; uint8_t cand[4], kept[4]; uint32_t rank[4]; float lcp[1]; double sums[28];\n"
        "    void* at; uint64_t bytes;\n"
        "    p.max_iterations = 5; p.max_correspondence_distance = 0.035f; p.keep_ratio = 0.7f; p.min_normal_cos = -2.0f;\n"
        "    return stocs_refine_poses_robust(c, T, 1, NULL, 0, &p, out, NULL, lcp, nc, ncand, it)\n"
        "         + stocs_refine_robust_detail(c, T, idx, 4, &p, match, cand, kept, rank, &k, &n, sums)\n"
        "         + stocs_refine_robust_detail(c, T, idx, 4, &p, match, cand, kept, rank, NULL, NULL, NULL)\n"
        "         + stocs_refine_robust_workspace(c, &at, &bytes) + (STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES > 0);\n"
        "}\n")
    r = subprocess.run(GCC + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_parameter_struct_is_16_bytes_on_both_sides(capi, tmp_path):
    src = tmp_path / "size.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\n"
        "int main(void) {\n"
        "    printf(\"%d %d %d %d %d\\n\", (int)sizeof(stocs_refine_robust_params), (int)offsetof(stocs_refine_robust_params, max_iterations),\n"
        "           (int)offsetof(stocs_refine_robust_params, max_correspondence_distance), (int)offsetof(stocs_refine_robust_params, keep_ratio),\n"
        "           (int)offsetof(stocs_refine_robust_params, min_normal_cos));\n"
        "    return 0;\n"
        "}\n")
    exe = tmp_path / "size"
    r = subprocess.run(GCC + [str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [16, 0, 4, 8, 12]
    P = capi.RefineRobustParams
    assert [C.sizeof(P), P.max_iterations.offset, P.max_correspondence_distance.offset, P.keep_ratio.offset, P.min_normal_cos.offset] == got


def test_capi_binds_them(capi):
    L = capi.load()
    assert L.stocs_refine_poses_robust.restype is C.c_int and len(L.stocs_refine_poses_robust.argtypes) == 12
    assert L.stocs_refine_robust_detail.restype is C.c_int and len(L.stocs_refine_robust_detail.argtypes) == 12
    assert L.stocs_refine_robust_workspace.restype is C.c_int and len(L.stocs_refine_robust_workspace.argtypes) == 3
    for name in ("stocs_refine_poses_robust", "stocs_refine_robust_detail", "stocs_refine_robust_workspace"):
        assert name in capi.SIGNATURES
    from model_matching_amd.estimator import StocsEstimator
    for name in ("refine_poses_robust", "refine_robust_detail", "refine_robust_workspace", "robust_params"):
        assert callable(getattr(StocsEstimator, name)), name
    # the conversion the Python layer documents: degrees -> cosine once, in float; None: gate off
    p = StocsEstimator.robust_params(5, 0.035, 0.7, 30.0)
    assert abs(p.min_normal_cos - 0.8660254) < 1e-6 and abs(p.keep_ratio - 0.7) < 1e-7 and p.max_iterations == 5
    assert StocsEstimator.robust_params(5, 0.035, 1.0, None).min_normal_cos < -1.0
    assert StocsEstimator.robust_params(5, 0.035, 1.0, 0.0).min_normal_cos == 1.0
    # no context: INVALID with a message, never a crash
    assert L.stocs_refine_poses_robust(None, None, 0, None, 0, None, None, None, None, None, None, None) == capi.ERR_INVALID
    assert L.stocs_refine_robust_detail(None, None, None, 0, None, None, None, None, None, None, None, None) == capi.ERR_INVALID
    assert L.stocs_refine_robust_workspace(None, None, None) == capi.ERR_INVALID and len(L.stocs_last_error()) > 0
