"""CPU-side checks of the mesh C ABI: the library exports the symbols, the header that declares them compiles as C99, the PLY mesh reader
and writer on files written here (ascii and binary, list types, polygons fanned, no faces), and stocs_mesh_check, the host check that
stocs_ctx_set_mesh runs before it touches a device.  No GPU compute."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stocs_ply_read_mesh", "stocs_ply_write_mesh", "stocs_mesh_check", "stocs_mesh_small_px", "stocs_ctx_set_mesh", "stocs_ctx_mesh_info",
         "stocs_render_depth_mesh", "stocs_pose_errors_vsd_mesh", "stocs_mesh_last_call_timing")
INVALID, CAPACITY = -1, None
F = np.float32


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
    L = capi.load()
    assert L.stocs_pose_errors_vsd_mesh.restype is C.c_int and len(L.stocs_pose_errors_vsd_mesh.argtypes) == 7
    from model_matching_amd import cloudio, estimator, synth
    for name in ("set_mesh", "mesh_info", "render_depth_mesh", "pose_errors_vsd_mesh"):
        assert callable(getattr(estimator.StocsEstimator, name)), name
    assert callable(cloudio.read_ply_mesh) and callable(cloudio.write_ply_mesh) and callable(synth.make_model_mesh)


def test_header_declares_them_as_c99(capi, tmp_path):
    src = tmp_path / "mesh_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* v, const int32_t* t, const float* est, const float* gt, stocs_vsd_record* out, float* depth, float* pos, int32_t* tri) {\n"
        "    stocs_vsd_params p;\n"
        "    int rc, nv = 0, nt = 0, n = 0;\n"
        "    const char* labels[4]; double ms[4];\n"
        "    stocs_default_vsd_params(&p);\n"
        "    p.n_tau = 1; p.tau[0] = 0.01f;\n"
        "    rc = stocs_ply_read_mesh(\"m.ply\", pos, 8, &nv, tri, 12, &nt);\n"
        "    rc = rc ? rc : stocs_ply_write_mesh(\"m.ply\", pos, nv, tri, nt);\n"
        "    rc = rc ? rc : stocs_mesh_check(v, 8, t, 12);\n"
        "    rc = rc ? rc : stocs_ctx_set_mesh(c, v, 8, t, 12);\n"
        "    rc = rc ? rc : stocs_ctx_mesh_info(c, &nv, &nt);\n"
        "    rc = rc ? rc : stocs_render_depth_mesh(c, est, 2, depth);\n"
        "    rc = rc ? rc : stocs_pose_errors_vsd_mesh(c, est, 2, gt, 1, &p, out);\n"
        "    rc = rc ? rc : stocs_mesh_last_call_timing(c, labels, ms, 4, &n);\n"
        "    return rc ? rc : out->uni + nv + nt + n + STOCS_MESH_SMALL_PX + stocs_mesh_small_px();\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hdr = open(os.path.join(ROOT, "include", "stocs_hip.h")).read()
    assert "#define STOCS_MESH_SMALL_PX %d\n" % capi.load().stocs_mesh_small_px() in hdr


# ---- PLY ----

VERTS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0.5, 1.5, 0.25), (-0.125, 0.5, 1e-3)], F)


def _header(fmt, nv, face_lines, extra_vertex=()):
    return ("ply\nformat %s 1.0\ncomment test\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s%send_header\n"
            % (fmt, nv, "".join("property %s\n" % p for p in extra_vertex), face_lines)).encode()


def _read(capi, path):
    from model_matching_amd import cloudio
    return cloudio.read_ply_mesh(path)


def test_ascii_triangles_a_quad_and_a_pentagon(capi, tmp_path):
    p = tmp_path / "a.ply"
    body = "".join("%r %r %r\n" % tuple(float(x) for x in v) for v in VERTS)
    faces = "3 0 1 2\n4 0 1 2 3\n5 0 1 2 4 3\n"
    p.write_bytes(_header("ascii", 6, "element face 3\nproperty list uchar int vertex_indices\n") + (body + faces).encode())
    v, t = _read(capi, p)
    assert np.array_equal(v, VERTS)
    assert t.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 4], [0, 4, 3]]      # fans from corner 0


@pytest.mark.parametrize("count_t, index_t, cf, xf", [("uchar", "int", "B", "i"), ("uchar", "uint", "B", "I"), ("int", "int", "i", "i"), ("ushort", "ushort", "H", "H"),
                                                       ("uint8", "int32", "B", "i")])
def test_binary_with_every_list_type_and_other_properties(capi, tmp_path, count_t, index_t, cf, xf):
    p = tmp_path / "b.ply"
    hdr = _header("binary_little_endian", 6, "element face 2\nproperty uchar flags\nproperty list %s %s vertex_index\nproperty float area\n" % (count_t, index_t),
                  extra_vertex=("uchar red", "double quality"))
    body = b"".join(struct.pack("<fffBd", *[float(x) for x in v], 7, 0.5) for v in VERTS)
    faces = struct.pack("<B" + cf + "3" + xf + "f", 1, 3, 5, 4, 3, 2.0) + struct.pack("<B" + cf + "4" + xf + "f", 0, 4, 0, 1, 2, 3, 1.0)
    p.write_bytes(hdr + body + faces)
    v, t = _read(capi, p)
    assert np.array_equal(v, VERTS) and t.tolist() == [[5, 4, 3], [0, 1, 2], [0, 2, 3]]


def test_no_faces_is_no_error(capi, tmp_path):
    body = "".join("%r %r %r\n" % tuple(float(x) for x in v) for v in VERTS).encode()
    for face_lines in ("element face 0\nproperty list uchar int vertex_indices\n", ""):
        p = tmp_path / "c.ply"
        p.write_bytes(_header("ascii", 6, face_lines) + body)
        v, t = _read(capi, p)
        assert np.array_equal(v, VERTS) and t.shape == (0, 3)


def test_write_then_read_round_trips(capi, tmp_path):
    from model_matching_amd import cloudio, synth
    v, t = synth.make_model_mesh(1)
    p = tmp_path / "d.ply"
    cloudio.write_ply_mesh(p, v, t)
    v2, t2 = cloudio.read_ply_mesh(p)
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(t2, t)
    L = capi.load()
    nv, nt = C.c_int(0), C.c_int(0)
    assert L.stocs_ply_read_mesh(str(p).encode(), None, 0, C.byref(nv), None, 0, C.byref(nt)) == 0 and (nv.value, nt.value) == (len(v), len(t))
    small = np.zeros((len(t) - 1, 3), np.int32)
    assert L.stocs_ply_read_mesh(str(p).encode(), v2.ctypes.data_as(capi._fp), len(v), C.byref(nv), small.ctypes.data_as(capi._ip), len(small), C.byref(nt)) not in (0, INVALID)
    assert L.stocs_ply_read_mesh(str(p).encode(), v2.ctypes.data_as(capi._fp), len(v) - 1, C.byref(nv), t2.ctypes.data_as(capi._ip), len(t), C.byref(nt)) not in (0, INVALID)


def test_bad_files_are_refused(capi, tmp_path):
    L = capi.load()
    nv, nt = C.c_int(0), C.c_int(0)
    q = lambda p: L.stocs_ply_read_mesh(str(p).encode(), None, 0, C.byref(nv), None, 0, C.byref(nt))
    body = "".join("%r %r %r\n" % tuple(float(x) for x in v) for v in VERTS)
    p = tmp_path / "e.ply"
    p.write_bytes(_header("ascii", 6, "element face 1\nproperty list uchar int vertex_indices\n") + (body + "2 0 1\n").encode())
    assert q(p) == INVALID and b"corners" in L.stocs_last_error()
    p.write_bytes(_header("ascii", 6, "element face 2\nproperty list uchar int vertex_indices\n") + (body + "3 0 1 2\n").encode())
    assert q(p) == INVALID
    p.write_bytes(_header("ascii", 6, "element face 1\nproperty int material\n") + (body + "3\n").encode())
    assert q(p) == INVALID
    assert q(tmp_path / "missing.ply") == INVALID
    assert L.stocs_ply_read_mesh(None, None, 0, C.byref(nv), None, 0, C.byref(nt)) == INVALID


# ---- the host check of stocs_ctx_set_mesh ----

def test_mesh_check(capi):
    L = capi.load()
    from model_matching_amd import synth
    v, t = synth.make_model_mesh(0)
    vp, tp = v.ctypes.data_as(capi._fp), t.ctypes.data_as(capi._ip)
    assert L.stocs_mesh_check(vp, len(v), tp, len(t)) == 0
    for bad in (-1, len(v), 2 ** 31 - 1):
        t2 = t.copy(); t2[7, 1] = bad
        assert L.stocs_mesh_check(vp, len(v), t2.ctypes.data_as(capi._ip), len(t2)) == INVALID and b"index" in L.stocs_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        v2 = v.copy(); v2[3, 2] = bad
        assert L.stocs_mesh_check(v2.ctypes.data_as(capi._fp), len(v2), tp, len(t)) == INVALID and b"finite" in L.stocs_last_error()
    v2 = v.copy(); v2[-1, 0] = np.nan                       # a vertex nobody uses counts too
    assert L.stocs_mesh_check(v2.ctypes.data_as(capi._fp), len(v2), t[:4].copy().ctypes.data_as(capi._ip), 4) == INVALID
    assert L.stocs_mesh_check(None, len(v), tp, len(t)) == INVALID and L.stocs_mesh_check(vp, len(v), None, len(t)) == INVALID
    assert L.stocs_mesh_check(vp, -1, tp, len(t)) == INVALID and L.stocs_mesh_check(vp, len(v), tp, -1) == INVALID
    assert L.stocs_mesh_check(vp, 2 ** 24 + 1, tp, 0) not in (0, INVALID) and L.stocs_mesh_check(vp, len(v), tp, 2 ** 22 + 1) not in (0, INVALID)
    assert L.stocs_mesh_check(None, 0, None, 0) == 0


def test_argument_checks_that_need_no_device(capi):
    L = capi.load()
    P = (C.c_float * 16)(); D = (C.c_float * 4)(); out = (capi.VsdRecord * 1)()
    p = capi.VsdParams(); L.stocs_default_vsd_params(C.byref(p)); p.n_tau = 1; p.tau[0] = 0.01
    assert L.stocs_ctx_set_mesh(None, None, 0, None, 0) == INVALID
    assert L.stocs_ctx_mesh_info(None, None, None) == INVALID
    assert L.stocs_render_depth_mesh(None, P, 0, D) == INVALID
    assert L.stocs_pose_errors_vsd_mesh(None, P, 1, P, 1, C.byref(p), out) == INVALID
    assert L.stocs_mesh_last_call_timing(None, None, None, 0, None) == INVALID
