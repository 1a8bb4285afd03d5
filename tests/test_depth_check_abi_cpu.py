"""CPU-side checks of the depth-check C ABI (stocs_ctx_set_frame, stocs_depth_check_poses, stocs_default_depth_params): the library
exports them, the header that declares them still compiles as C99, and the ctypes structs match the C layout.  No GPU compute here."""
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


def test_library_exports_depth_check_symbols(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("stocs_ctx_set_frame", "stocs_depth_check_poses", "stocs_default_depth_params"):
        assert hasattr(lib, name), name


def test_defaults(capi):
    p = capi.DepthParams()
    capi.load().stocs_default_depth_params(C.byref(p))
    assert (p.tolerance, p.class_threshold, p.occlusion_margin) == (C.c_float(0.01).value, C.c_float(0.10).value, C.c_float(0.01).value)
    assert (p.self_occlusion, p.cell_px) == (1, 8)
    capi.load().stocs_default_depth_params(None)   # tolerated


def test_header_declares_depth_check_as_c99(tmp_path):
    src = tmp_path / "depth_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const stocs_camera* cam, const uint16_t* depth, const uint16_t* prob, const float* P, stocs_depth_result* out) {\n"
        "    stocs_depth_params p;\n"
        "    int rc;\n"
        "    stocs_default_depth_params(&p);\n"
        "    p.tolerance = 0.005f; p.class_threshold = 0.1f; p.self_occlusion = 0; p.cell_px = 4; p.occlusion_margin = 0.0f;\n"
        "    rc = stocs_ctx_set_frame(c, cam, depth, prob);\n"
        "    rc = rc ? rc : stocs_depth_check_poses(c, P, 1, &p, out);\n"
        "    return rc ? rc : out->facing + out->in_image + out->self_occluded + out->no_depth + out->agree + out->in_front + out->behind + out->on_mask\n"
        "                     + (int)(out->score + out->violation);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _c_layout(tmp_path, struct, fields):
    """sizeof and offsetof of a struct of stocs_hip.h, from a small C program compiled with the system compiler"""
    src = tmp_path / ("layout_%s.c" % struct)
    body = "".join('    printf("%%zu\\n", offsetof(%s, %s));\n' % (struct, f) for f in fields)
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\nint main(void) {\n"
                   '    printf("%%zu\\n", sizeof(%s));\n%s    return 0;\n}\n' % (struct, body))
    exe = tmp_path / ("layout_%s" % struct)
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    return out[0], out[1:]


@pytest.mark.parametrize("struct,cls", [("stocs_depth_params", "DepthParams"), ("stocs_depth_result", "DepthResult")])
def test_ctypes_structs_match_the_c_layout(capi, tmp_path, struct, cls):
    S = getattr(capi, cls)
    fields = [f[0] for f in S._fields_]
    size, offs = _c_layout(tmp_path, struct, fields)
    assert C.sizeof(S) == size
    assert [getattr(S, f).offset for f in fields] == offs


def test_capi_and_estimator_bind_the_depth_check(capi):
    L = capi.load()
    assert L.stocs_ctx_set_frame.restype is C.c_int and len(L.stocs_ctx_set_frame.argtypes) == 4
    assert L.stocs_depth_check_poses.restype is C.c_int and len(L.stocs_depth_check_poses.argtypes) == 5
    assert L.stocs_default_depth_params.restype is None and len(L.stocs_default_depth_params.argtypes) == 1
    from model_matching_amd.estimator import StocsEstimator, _DEPTH_DTYPE
    assert _DEPTH_DTYPE.itemsize == C.sizeof(capi.DepthResult)
    assert [n for n in _DEPTH_DTYPE.names] == [f[0] for f in capi.DepthResult._fields_]
    assert callable(getattr(StocsEstimator, "set_frame")) and callable(getattr(StocsEstimator, "depth_check_poses"))


def test_argument_checks_that_need_no_device(capi):
    """NULL context: STOCS_ERR_INVALID from both calls before anything touches a device"""
    L = capi.load()
    p = capi.DepthParams()
    L.stocs_default_depth_params(C.byref(p))
    out = (capi.DepthResult * 1)()
    P = (C.c_float * 16)()
    assert L.stocs_depth_check_poses(None, P, 1, C.byref(p), out) == -1
    assert L.stocs_ctx_set_frame(None, None, None, None) == -1
