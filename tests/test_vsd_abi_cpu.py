"""CPU-side checks of the VSD C ABI (stocs_default_vsd_params, stocs_check_vsd_params, stocs_render_depth, stocs_pose_errors_vsd): the
library exports them, the header that declares them still compiles as C99, the ctypes structs match the C layout, the defaults are the
documented ones, and every STOCS_ERR_INVALID that returns before a device is touched does.  No GPU compute."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stocs_default_vsd_params", "stocs_check_vsd_params", "stocs_render_depth", "stocs_pose_errors_vsd")
INVALID = -1


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
    src = tmp_path / "vsd_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* est, const float* gt, stocs_vsd_record* out, float* depth) {\n"
        "    stocs_vsd_params p;\n"
        "    int rc;\n"
        "    stocs_default_vsd_params(&p);\n"
        "    p.n_tau = 1; p.tau[0] = 0.01f;\n"
        "    rc = stocs_check_vsd_params(&p);\n"
        "    rc = rc ? rc : stocs_render_depth(c, est, 2, &p, depth);\n"
        "    rc = rc ? rc : stocs_pose_errors_vsd(c, est, 2, gt, 1, &p, out);\n"
        "    return rc ? rc : out->px_est + out->px_gt + out->vis_est + out->vis_gt + out->inter + out->uni + out->far[STOCS_VSD_MAX_TAU - 1]\n"
        "                     + (int)out->e[0] + out->valid + out->reserved + STOCS_VSD_POINTS;\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("cname, pyname, size", [("stocs_vsd_params", "VsdParams", 80), ("stocs_vsd_record", "VsdRecord", 160)])
def test_ctypes_structs_match_the_c_layout(capi, tmp_path, cname, pyname, size):
    S = getattr(capi, pyname)
    fields = [f[0] for f in S._fields_]
    src = tmp_path / "layout.c"
    body = "".join('    printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f in fields)
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\nint main(void) {\n"
                   '    printf("%%zu\\n", sizeof(%s));\n%s    return 0;\n}\n' % (cname, body))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(S) == out[0] == size
    assert [getattr(S, f).offset for f in fields] == out[1:]


def test_capi_and_estimator_bind_them(capi):
    L = capi.load()
    assert L.stocs_pose_errors_vsd.restype is C.c_int and len(L.stocs_pose_errors_vsd.argtypes) == 7
    assert L.stocs_render_depth.restype is C.c_int and len(L.stocs_render_depth.argtypes) == 5
    assert L.stocs_check_vsd_params.restype is C.c_int and len(L.stocs_check_vsd_params.argtypes) == 1
    from model_matching_amd import estimator
    assert estimator._VSD_DTYPE.itemsize == C.sizeof(capi.VsdRecord) == 160
    assert [n for n in estimator._VSD_DTYPE.names] == [f[0] for f in capi.VsdRecord._fields_]
    for name in ("render_depth", "pose_errors_vsd"):
        assert callable(getattr(estimator.StocsEstimator, name)), name
    assert callable(estimator.pose_recall_vsd)
    assert len(estimator.BOP_VSD_TAUS) == 10 and len(estimator.BOP_VSD_THRESHOLDS) == 10


def test_the_test_restatement_has_the_same_record(capi):
    if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import vsd_ref as ref
    from model_matching_amd import estimator
    assert ref.DTYPE == estimator._VSD_DTYPE


def _defaults(capi):
    p = capi.VsdParams()
    capi.load().stocs_default_vsd_params(C.byref(p))
    return p


def test_defaults(capi):
    p = _defaults(capi)
    assert p.surfel_radius == C.c_float(0.006).value and p.max_splat_px == 16 and p.delta == C.c_float(0.015).value
    assert p.n_tau == 0 and list(p.tau) == [0.0] * 16
    capi.load().stocs_default_vsd_params(None)            # a NULL is ignored
    assert capi.load().stocs_check_vsd_params(C.byref(p)) == INVALID      # the taus are the caller's to set


def test_parameter_ranges(capi):
    L = capi.load()

    def good():
        p = _defaults(capi)
        p.n_tau = 2; p.tau[0] = 0.01; p.tau[1] = 0.02
        return p

    assert L.stocs_check_vsd_params(C.byref(good())) == 0
    assert L.stocs_check_vsd_params(None) == INVALID
    p = good(); p.n_tau = 16
    assert L.stocs_check_vsd_params(C.byref(p)) == INVALID                # tau[2..15] are 0
    for t in range(16):
        p.tau[t] = 0.01
    assert L.stocs_check_vsd_params(C.byref(p)) == 0
    p.max_splat_px = 0
    assert L.stocs_check_vsd_params(C.byref(p)) == 0
    bad = [("surfel_radius", 0.0), ("surfel_radius", -0.001), ("surfel_radius", math.inf), ("surfel_radius", math.nan),
           ("max_splat_px", -1), ("max_splat_px", 17),
           ("delta", 0.0), ("delta", -1.0), ("delta", math.inf), ("delta", math.nan),
           ("n_tau", 0), ("n_tau", -1), ("n_tau", 17)]
    for k, v in bad:
        p = good(); setattr(p, k, v)
        assert L.stocs_check_vsd_params(C.byref(p)) == INVALID, (k, v)
        assert k.split("_")[0] in L.stocs_last_error().decode(), (k, L.stocs_last_error())
    for v in (0.0, -0.01, math.inf, math.nan):
        p = good(); p.tau[1] = v
        assert L.stocs_check_vsd_params(C.byref(p)) == INVALID, v
        p = good(); p.tau[2] = v                            # beyond n_tau: not read
        assert L.stocs_check_vsd_params(C.byref(p)) == 0, v


def test_argument_checks_that_need_no_device(capi):
    """a NULL context is STOCS_ERR_INVALID from both device calls before anything touches a device, whatever n"""
    L = capi.load()
    out = (capi.VsdRecord * 1)()
    P = (C.c_float * 16)()
    D = (C.c_float * 4)()
    p = _defaults(capi); p.n_tau = 1; p.tau[0] = 0.01
    assert L.stocs_pose_errors_vsd(None, P, 1, P, 1, C.byref(p), out) == INVALID
    assert L.stocs_pose_errors_vsd(None, P, 0, P, 1, C.byref(p), out) == INVALID
    assert L.stocs_render_depth(None, P, 1, C.byref(p), D) == INVALID
    assert L.stocs_render_depth(None, P, 0, C.byref(p), D) == INVALID
