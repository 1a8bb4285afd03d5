"""CPU-side checks of the joint-rendering C ABI (stocs_render_poses, stocs_render_resolve, stocs_render_labels, stocs_explain_poses,
stocs_default_render_params): the header declares them as C99, the library exports them, and the ctypes structs match the C layout.
No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("stocs_default_render_params", "stocs_render_poses", "stocs_render_resolve", "stocs_render_labels", "stocs_explain_poses")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def test_header_and_library_have_the_symbols(capi):
    header = open(os.path.join(ROOT, "include", "stocs_hip.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name


def test_defaults(capi):
    p = capi.RenderParams()
    capi.load().stocs_default_render_params(C.byref(p))
    assert (p.point_radius, p.tolerance, p.class_threshold) == (C.c_float(0.005).value, C.c_float(0.01).value, C.c_float(0.10).value)
    assert p.max_splat_px == 8
    capi.load().stocs_default_render_params(None)   # tolerated


def test_header_declares_the_render_calls_as_c99(tmp_path):
    src = tmp_path / "render_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* a, stocs_ctx* b, const float* Pa, const float* Pb, void* zkey, stocs_render_result* out, int32_t* labels, uint8_t* state) {\n"
        "    stocs_render_params p;\n"
        "    int rc;\n"
        "    stocs_default_render_params(&p);\n"
        "    p.point_radius = 0.004f; p.max_splat_px = 4; p.tolerance = 0.005f; p.class_threshold = 0.1f;\n"
        "    rc = stocs_render_poses(a, Pa, 2, 0, &p, zkey, 1);\n"
        "    rc = rc ? rc : stocs_render_poses(b, Pb, 1, 2, &p, zkey, 0);\n"
        "    rc = rc ? rc : stocs_render_resolve(a, Pa, 2, 0, &p, zkey, out);\n"
        "    rc = rc ? rc : stocs_render_resolve(b, Pb, 1, 2, &p, zkey, out + 2);\n"
        "    rc = rc ? rc : stocs_render_labels(a, zkey, &p, labels, state);\n"
        "    rc = rc ? rc : stocs_explain_poses(a, Pa, 2, &p, out, labels, NULL);\n"
        "    return rc ? rc : out->footprint + out->visible + out->hidden + out->no_depth + out->agree + out->in_front + out->behind + out->on_mask;\n"
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


@pytest.mark.parametrize("struct,cls,fields", [
    ("stocs_render_params", "RenderParams", ["point_radius", "max_splat_px", "tolerance", "class_threshold"]),
    ("stocs_render_result", "RenderResult", ["footprint", "visible", "hidden", "no_depth", "agree", "in_front", "behind", "on_mask"])])
def test_ctypes_structs_match_the_c_layout(capi, tmp_path, struct, cls, fields):
    S = getattr(capi, cls)
    assert [f[0] for f in S._fields_] == fields          # the field order the contract states
    size, offs = _c_layout(tmp_path, struct, fields)
    assert C.sizeof(S) == size
    assert [getattr(S, f).offset for f in fields] == offs


def test_capi_and_estimator_bind_the_render_calls(capi):
    L = capi.load()
    assert L.stocs_default_render_params.restype is None and len(L.stocs_default_render_params.argtypes) == 1
    for name, nargs in (("stocs_render_poses", 7), ("stocs_render_resolve", 7), ("stocs_render_labels", 5), ("stocs_explain_poses", 7)):
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == nargs, name
    from model_matching_amd.estimator import StocsEstimator, _RENDER_DTYPE
    assert _RENDER_DTYPE.itemsize == C.sizeof(capi.RenderResult) == 32
    assert list(_RENDER_DTYPE.names) == [f[0] for f in capi.RenderResult._fields_]
    for m in ("render_poses", "render_resolve", "render_labels", "explain_poses"):
        assert callable(getattr(StocsEstimator, m)), m


def test_argument_checks_that_need_no_device(capi):
    """NULL context: STOCS_ERR_INVALID from every call before anything touches a device"""
    L = capi.load()
    p = capi.RenderParams()
    L.stocs_default_render_params(C.byref(p))
    out = (capi.RenderResult * 1)()
    P = (C.c_float * 16)()
    lab = (C.c_int32 * 1)()
    assert L.stocs_render_poses(None, P, 1, 0, C.byref(p), None, 1) == -1
    assert L.stocs_render_resolve(None, P, 1, 0, C.byref(p), None, out) == -1
    assert L.stocs_render_labels(None, None, C.byref(p), lab, None) == -1
    assert L.stocs_explain_poses(None, P, 1, C.byref(p), out, None, None) == -1
