"""CPU-side checks of the C ABI of the mesh forms of the joint renderer and of scene selection: the library exports the symbols with the
bindings' signatures, the header that declares them compiles as C99, the Python layer has the methods, and the argument checks that need
no device answer as the contract says.  No GPU compute."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"stocs_render_poses_mesh": 6, "stocs_render_resolve_mesh": 7, "stocs_explain_poses_mesh": 7, "stocs_scene_footprints_mesh": 9,
         "stocs_render_mesh_last_device_ms": 3}
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
    L = capi.load()
    for name, n_args in NAMES.items():
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args, name
    from model_matching_amd import estimator
    for name in ("render_poses_mesh", "render_resolve_mesh", "explain_poses_mesh", "scene_footprints_mesh", "render_mesh_last_device_ms"):
        assert callable(getattr(estimator.StocsEstimator, name)), name
    assert inspect.signature(estimator.select_scene).parameters["surface"].default is None


def test_header_declares_them_as_c99(capi, tmp_path):
    src = tmp_path / "render_mesh_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* poses, void* zkey, void* rows, stocs_render_result* out, stocs_scene_record* rec, int32_t* lab, uint8_t* st) {\n"
        "    stocs_render_params p;\n"
        "    float ms[2];\n"
        "    int rc;\n"
        "    stocs_default_render_params(&p);\n"
        "    rc = stocs_render_poses_mesh(c, poses, 2, 0, zkey, 1);\n"
        "    rc = rc ? rc : stocs_render_resolve_mesh(c, poses, 2, 0, &p, zkey, out);\n"
        "    rc = rc ? rc : stocs_render_labels(c, zkey, &p, lab, st);\n"
        "    rc = rc ? rc : stocs_explain_poses_mesh(c, poses, 2, &p, out, lab, st);\n"
        "    rc = rc ? rc : stocs_scene_footprints_mesh(c, poses, 2, 0, 2, &p, 0, rows, rec);\n"
        "    rc = rc ? rc : stocs_render_mesh_last_device_ms(c, &ms[0], &ms[1]);\n"
        "    return rc ? rc : out->footprint + rec->claimed + (ms[0] > ms[1]);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_argument_checks_that_need_no_device(capi):
    L = capi.load()
    P = (C.c_float * 16)(); out = (capi.RenderResult * 1)(); rec = (capi.SceneRecord * 1)()
    lab = (C.c_int32 * 4)(); st = (C.c_uint8 * 4)()
    key = C.c_void_p(0)
    p = capi.RenderParams(); L.stocs_default_render_params(C.byref(p))
    # a NULL context is refused whatever n is, as for the splat forms
    for n in (0, 1, -1):
        assert L.stocs_render_poses_mesh(None, P, n, 0, key, 1) == INVALID and b"NULL context" in L.stocs_last_error()
        assert L.stocs_render_resolve_mesh(None, P, n, 0, C.byref(p), key, out) == INVALID and b"stocs_render_resolve_mesh" in L.stocs_last_error()
        assert L.stocs_explain_poses_mesh(None, P, n, C.byref(p), out, lab, st) == INVALID and b"stocs_explain_poses_mesh" in L.stocs_last_error()
        assert L.stocs_scene_footprints_mesh(None, P, n, 0, 1, C.byref(p), 0, key, rec) == INVALID and b"stocs_scene_footprints_mesh" in L.stocs_last_error()
    assert L.stocs_render_mesh_last_device_ms(None, None, None) == INVALID


def test_the_build_lists_the_new_file(capi):
    mk = open(os.path.join(ROOT, "model_matching_amd", "csrc", "Makefile")).read()
    assert "render_mesh.hip" in mk
    assert os.path.exists(os.path.join(ROOT, "model_matching_amd", "csrc", "render_shared.h"))
