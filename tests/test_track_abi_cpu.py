"""CPU-side checks of the pose tracking C ABI (stocs_track_poses, stocs_track_get_round): the library exports both, the header that
declares them still compiles as C99, and the ctypes structs match the C layout.  No GPU compute here."""
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


def test_library_exports_track_symbols(capi):
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "stocs_track_poses") and hasattr(lib, "stocs_track_get_round")


def test_header_declares_track_as_c99(tmp_path):
    src = tmp_path / "track_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* P, stocs_track_result* out, float* T, float* l) {\n"
        "    stocs_track_params p;\n"
        "    int n = 0, rc;\n"
        "    p.rounds = 4; p.samples = 64; p.max_translation = 0.02f; p.max_rotation_deg = 10.0f; p.shrink = 0.5f; p.seed = 1u;\n"
        "    p.refine_iterations = 0; p.max_correspondence_distance = 0.035f; p.keep_details = 1;\n"
        "    rc = stocs_track_poses(c, P, 1, &p, out);\n"
        "    return rc ? rc : stocs_track_get_round(c, 0, 0, T, l, STOCS_TRACK_MAX_ROUNDS + STOCS_TRACK_MAX_CANDIDATES, &n);\n"
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


@pytest.mark.parametrize("struct,cls", [("stocs_track_params", "TrackParams"), ("stocs_track_result", "TrackResult")])
def test_ctypes_structs_match_the_c_layout(capi, tmp_path, struct, cls):
    S = getattr(capi, cls)
    fields = [f[0] for f in S._fields_]
    size, offs = _c_layout(tmp_path, struct, fields)
    assert C.sizeof(S) == size
    assert [getattr(S, f).offset for f in fields] == offs


def test_capi_and_estimator_bind_tracking(capi):
    L = capi.load()
    assert L.stocs_track_poses.restype is C.c_int and len(L.stocs_track_poses.argtypes) == 5
    assert L.stocs_track_get_round.restype is C.c_int and len(L.stocs_track_get_round.argtypes) == 7
    from model_matching_amd.estimator import StocsEstimator, _TRACK_DTYPE
    assert _TRACK_DTYPE.itemsize == C.sizeof(capi.TrackResult)
    assert callable(getattr(StocsEstimator, "track_poses")) and callable(getattr(StocsEstimator, "track_round"))
