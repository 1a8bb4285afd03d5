"""CPU-side checks of stocs_get_grid_info: the library exports it, the header that declares it still compiles as C99, the ctypes struct
matches the C layout, the estimator binds it, and the argument and state checks that come before any device is touched answer as
documented.  No GPU compute."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = -1, -5


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def test_library_exports_the_symbol(capi):
    assert hasattr(C.CDLL(capi.LIB_PATH), "stocs_get_grid_info")


def test_header_declares_it_as_c99(tmp_path):
    src = tmp_path / "grid_info_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "long long call(stocs_ctx* c) {\n"
        "    stocs_grid_info g;\n"
        "    int rc = stocs_get_grid_info(c, &g);\n"
        "    if (rc) return rc;\n"
        "    return (long long)g.origin[2] + (long long)g.h + (long long)g.inv_h + g.div + g.cells[2] + g.bricks[2] + g.centre_sorted + g.pruned\n"
        "           + g.has_nearest + g.has_cones + g.has_flat + (g.sort == STOCS_GRID_SORT_OWN) + (g.sort == STOCS_GRID_SORT_ROCPRIM)\n"
        "           + g.prune_group + g.prune_k + g.longest_list + g.reserved + g.n_incidences + g.n_cells + g.n_bricks + g.n_entries;\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ctypes_struct_matches_the_c_layout(capi, tmp_path):
    S = capi.GridInfo
    fields = [f[0] for f in S._fields_]
    src = tmp_path / "layout.c"
    body = "".join('    printf("%%zu\\n", offsetof(stocs_grid_info, %s));\n' % f for f in fields)
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\nint main(void) {\n"
                   '    printf("%%zu\\n", sizeof(stocs_grid_info));\n%s    printf("%%d %%d\\n", STOCS_GRID_SORT_ROCPRIM, STOCS_GRID_SORT_OWN);\n    return 0;\n}\n' % body)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(S) == out[0] == 120
    assert [getattr(S, f).offset for f in fields] == out[1:-2]
    assert (capi.GRID_SORT_ROCPRIM, capi.GRID_SORT_OWN) == tuple(out[-2:]) == (1, 2)


def test_capi_and_estimator_bind_it(capi):
    L = capi.load()
    assert L.stocs_get_grid_info.restype is C.c_int and len(L.stocs_get_grid_info.argtypes) == 2
    from model_matching_amd import estimator
    assert callable(estimator.StocsEstimator.grid_info)


def test_null_arguments(capi):
    L = capi.load()
    gi = capi.GridInfo()
    gi.div = 77
    assert L.stocs_get_grid_info(None, C.byref(gi)) == INVALID
    assert b"NULL context" in L.stocs_last_error()
    assert gi.div == 77                                    # a refused call writes nothing
    fake = C.create_string_buffer(1 << 16)                # read as a context, a block of zeros has no scene
    assert L.stocs_get_grid_info(C.cast(fake, C.c_void_p), None) == INVALID
    assert b"NULL info" in L.stocs_last_error()
    assert L.stocs_get_grid_info(None, None) == INVALID


def test_a_context_without_a_scene_is_a_state_error_and_zeroes_the_info(capi):
    """No device is touched before the scene check: the context here is a block of zeros, which is what a context whose last scene
    was refused looks like to this call (no points, no grid tables).  test_grid_forms_gpu.py repeats it on a real refused scene."""
    L = capi.load()
    fake = C.create_string_buffer(1 << 16)
    gi = capi.GridInfo()
    C.memset(C.byref(gi), 0xAB, C.sizeof(gi))
    assert L.stocs_get_grid_info(C.cast(fake, C.c_void_p), C.byref(gi)) == STATE
    assert b"no scene" in L.stocs_last_error()
    assert bytes(gi) == bytes(C.sizeof(gi))
