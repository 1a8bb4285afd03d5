"""CPU-side checks of the scene-selection C ABI (stocs_scene_row_words, stocs_scene_footprints, stocs_scene_select,
stocs_default_scene_params): the header declares them as C99, the library exports them, the ctypes structs match the C layout, the row
length is what the contract states and the defaults are as documented.  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("stocs_default_scene_params", "stocs_scene_row_words", "stocs_scene_footprints", "stocs_scene_select")


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
    p = capi.SceneParams()
    capi.load().stocs_default_scene_params(C.byref(p))
    assert (p.max_selected, p.min_pixels) == (64, 50)
    assert (p.min_exclusive_fraction, p.max_violation_fraction) == (C.c_float(0.5).value, C.c_float(0.2).value)
    capi.load().stocs_default_scene_params(None)   # tolerated


def test_row_words(capi):
    L = capi.load()
    for npix, want in ((1, 4), (31, 4), (32, 4), (33, 4), (127, 4), (128, 4), (129, 8), (1 << 19, 16384)):
        assert L.stocs_scene_row_words(npix, 1) == want == L.stocs_scene_row_words(1, npix), npix
        assert want % 4 == 0 and want * 32 >= npix > (want - 4) * 32
    assert L.stocs_scene_row_words(1024, 512) == 16384 and L.stocs_scene_row_words(640, 480) == 9600 and L.stocs_scene_row_words(43, 3) == 8
    assert L.stocs_scene_row_words(0, 5) == 0 and L.stocs_scene_row_words(5, -1) == 0
    from model_matching_amd.estimator import scene_row_words
    assert scene_row_words((480, 640)) == 9600


def test_header_declares_the_scene_calls_as_c99(tmp_path):
    src = tmp_path / "scene_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* a, stocs_ctx* b, const float* Pa, const float* Pb, void* rows, const float* score, const int32_t* group, int32_t* selected) {\n"
        "    stocs_render_params r;\n"
        "    stocs_scene_params p;\n"
        "    stocs_scene_record rec[3];\n"
        "    stocs_scene_result out[3];\n"
        "    int rc, ns = 0;\n"
        "    stocs_default_render_params(&r);\n"
        "    stocs_default_scene_params(&p);\n"
        "    p.max_selected = 2; p.min_pixels = 10; p.min_exclusive_fraction = 0.25f; p.max_violation_fraction = 0.5f;\n"
        "    rc = stocs_scene_row_words(640, 480) == 9600 ? 0 : 1;\n"
        "    rc = rc ? rc : stocs_scene_footprints(a, Pa, 2, 0, 3, &r, 0, rows, rec);\n"
        "    rc = rc ? rc : stocs_scene_footprints(b, Pb, 1, 2, 3, &r, 1, rows, rec + 2);\n"
        "    rc = rc ? rc : stocs_scene_select(a, rows, 3, 640, 480, score, group, rec, 2, NULL, &p, out, selected, &ns);\n"
        "    return rc ? rc : ns + out->rank + out->own + out->exclusive + out->reason + rec->footprint + rec->no_depth + rec->agree + rec->in_front\n"
        "                     + rec->behind + rec->on_mask + rec->claimed;\n"
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


@pytest.mark.parametrize("struct,cls,fields,size", [
    ("stocs_scene_record", "SceneRecord", ["footprint", "no_depth", "agree", "in_front", "behind", "on_mask", "claimed"], 28),
    ("stocs_scene_params", "SceneParams", ["max_selected", "min_pixels", "min_exclusive_fraction", "max_violation_fraction"], 16),
    ("stocs_scene_result", "SceneResult", ["rank", "own", "exclusive", "reason"], 16)])
def test_ctypes_structs_match_the_c_layout(capi, tmp_path, struct, cls, fields, size):
    S = getattr(capi, cls)
    assert [f[0] for f in S._fields_] == fields          # the field order the contract states
    c_size, offs = _c_layout(tmp_path, struct, fields)
    assert C.sizeof(S) == c_size == size
    assert [getattr(S, f).offset for f in fields] == offs


def test_capi_and_estimator_bind_the_scene_calls(capi):
    L = capi.load()
    assert L.stocs_default_scene_params.restype is None and len(L.stocs_default_scene_params.argtypes) == 1
    for name, nargs in (("stocs_scene_row_words", 2), ("stocs_scene_footprints", 9), ("stocs_scene_select", 14)):
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == nargs, name
    from model_matching_amd import estimator as E
    assert E._SCENE_RECORD_DTYPE.itemsize == C.sizeof(capi.SceneRecord) and list(E._SCENE_RECORD_DTYPE.names) == [f[0] for f in capi.SceneRecord._fields_]
    assert E._SCENE_RESULT_DTYPE.itemsize == C.sizeof(capi.SceneResult) and list(E._SCENE_RESULT_DTYPE.names) == [f[0] for f in capi.SceneResult._fields_]
    for m in ("scene_footprints", "scene_select"):
        assert callable(getattr(E.StocsEstimator, m)), m
    assert callable(E.select_scene) and E.SCENE_CLAIMS == {"agree": 0, "on_mask": 1}


def test_argument_checks_that_need_no_device(capi):
    """NULL context: STOCS_ERR_INVALID from both calls before anything touches a device"""
    L = capi.load()
    r = capi.RenderParams(); L.stocs_default_render_params(C.byref(r))
    p = capi.SceneParams(); L.stocs_default_scene_params(C.byref(p))
    rec = (capi.SceneRecord * 1)()
    out = (capi.SceneResult * 1)()
    P = (C.c_float * 16)()
    s = (C.c_float * 1)(); g = (C.c_int32 * 1)(); sel = (C.c_int32 * 1)(); ns = C.c_int(0)
    assert L.stocs_scene_footprints(None, P, 1, 0, 1, C.byref(r), 0, None, rec) == -1
    assert L.stocs_scene_select(None, None, 1, 4, 4, s, g, rec, 1, None, C.byref(p), out, sel, C.byref(ns)) == -1
