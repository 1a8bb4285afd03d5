"""CPU-side checks of the mesh sampling C ABI: the library exports the symbols, the header that declares them compiles as C99, and every
argument check answers before a device is looked for, in the order the header states.  No GPU compute."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stocs_mesh_sample_counts", "stocs_mesh_sample", "stocs_preprocess_model_mesh")
INVALID, CAPACITY = -1, -4
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
    assert len(L.stocs_mesh_sample_counts.argtypes) == 11 and len(L.stocs_mesh_sample.argtypes) == 13 and len(L.stocs_preprocess_model_mesh.argtypes) == 14
    from model_matching_amd import estimator, synth
    for name in ("mesh_sample_counts", "mesh_sample", "preprocess_model_mesh"):
        assert callable(getattr(estimator, name)), name
    v, t = synth.box_mesh((0.1, 0.06, 0.04))
    assert v.shape == (8, 3) and v.dtype == F and t.shape == (12, 3) and t.dtype == np.int32
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    assert np.all((n * v[t].mean(axis=1)).sum(axis=1) > 0)                           # outward winding
    assert np.isclose(0.5 * np.linalg.norm(n, axis=1).sum(), 2 * (0.1 * 0.06 + 0.1 * 0.04 + 0.06 * 0.04))


def test_header_declares_them_as_c99(tmp_path):
    src = tmp_path / "mesh_sample_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(const float* v, const int32_t* t, float* pos, float* nrm, int32_t* tri, int32_t* counts) {\n"
        "    double area = 0; int64_t total = 0; int skipped = 0, n = 0, rc;\n"
        "    uint64_t seed = 0xFFFFFFFFFFFFFFFFu;\n"
        "    rc = stocs_mesh_sample_counts(v, 8, t, 12, 0.001f, seed, -1, counts, &area, &total, &skipped);\n"
        "    rc = rc ? rc : stocs_mesh_sample(v, 8, t, 12, 0.001f, seed, STOCS_MESH_ORIENT_WINDING, -1, pos, nrm, tri, 100, &n);\n"
        "    rc = rc ? rc : stocs_preprocess_model_mesh(v, 8, t, 12, 0.0f, seed, STOCS_MESH_ORIENT_ORIGIN, 0.005f, 1.0f, -1, pos, nrm, 100, &n);\n"
        "    return rc ? rc : n + skipped + (int)total + (area > 0);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _mesh(capi):
    from model_matching_amd import synth
    v, t = synth.box_mesh((0.1, 0.06, 0.04))
    return v, t, v.ctypes.data_as(capi._fp), t.ctypes.data_as(capi._ip)


def test_sample_checks_answer_without_a_device_in_the_stated_order(capi):
    L = capi.load()
    v, t, vp, tp = _mesh(capi)
    n = C.c_int(-7)
    err = lambda: L.stocs_last_error()
    call = lambda vp_=vp, nv=8, tp_=tp, nt=12, h=0.001, orient=0, cap=0, n_=C.byref(n): L.stocs_mesh_sample(vp_, nv, tp_, nt, h, 1, orient, -1, None, None, None, cap, n_)
    # each line breaks one more argument than the line before it fixes: the earlier check answers
    assert call(nv=-1, h=np.nan, orient=2, cap=-1, n_=None) == INVALID and b"n_out" in err()
    assert call(nv=-1, h=np.nan, orient=2, cap=-1) == INVALID and b"< 0" in err()
    assert call(vp_=None, h=np.nan, orient=2, cap=-1) == INVALID and b"NULL vertices" in err()
    assert call(nt=2 ** 22 + 1, h=np.nan, orient=2, cap=-1) == CAPACITY
    t2 = t.copy(); t2[5, 2] = 8
    assert call(tp_=t2.ctypes.data_as(capi._ip), h=np.nan, orient=2, cap=-1) == INVALID and b"index" in err()
    v2 = v.copy(); v2[3, 1] = np.inf
    assert call(vp_=v2.ctypes.data_as(capi._fp), h=np.nan, orient=2, cap=-1) == INVALID and b"finite" in err()
    for h in (np.nan, np.inf, 0.0, -0.001):
        assert call(h=h, orient=2, cap=-1) == INVALID and b"spacing" in err()
    for orient in (-1, 2):
        assert call(orient=orient, cap=-1) == INVALID and b"orient" in err()
    assert call(cap=-1) == INVALID and b"cap" in err()
    assert n.value == -7                                                              # a refused call writes nothing
    assert call(nv=0, vp_=None, nt=0, tp_=None) == 0 and n.value == 0                   # no triangle: no sample, and no device needed


def test_counts_checks(capi):
    L = capi.load()
    v, t, vp, tp = _mesh(capi)
    err = lambda: L.stocs_last_error()
    call = lambda vp_=vp, nv=8, tp_=tp, nt=12, h=0.001: L.stocs_mesh_sample_counts(vp_, nv, tp_, nt, h, 1, -1, None, None, None, None)
    assert call(nt=-1, h=np.nan) == INVALID and b"< 0" in err()
    assert call(tp_=None, h=np.nan) == INVALID and b"NULL" in err()
    assert call(nv=2 ** 24 + 1, h=np.nan) == CAPACITY
    t2 = t.copy(); t2[0, 0] = -1
    assert call(tp_=t2.ctypes.data_as(capi._ip), h=np.nan) == INVALID and b"index" in err()
    v2 = v.copy(); v2[3, 1] = np.nan                                                   # a non-finite corner is a skipped triangle, not an error:
    assert call(vp_=v2.ctypes.data_as(capi._fp), h=np.nan) == INVALID and b"spacing" in err()      # the spacing is what is refused here
    for h in (np.nan, -np.inf, 0.0, -1.0):
        assert call(h=h) == INVALID and b"spacing" in err()
    area, total, skipped = C.c_double(1.0), C.c_int64(1), C.c_int(1)
    assert L.stocs_mesh_sample_counts(None, 0, None, 0, 0.001, 1, -1, None, C.byref(area), C.byref(total), C.byref(skipped)) == 0
    assert (area.value, total.value, skipped.value) == (0.0, 0, 0)


def test_preprocess_model_mesh_checks(capi):
    L = capi.load()
    v, t, vp, tp = _mesh(capi)
    n = C.c_int(-7)
    err = lambda: L.stocs_last_error()
    call = lambda vp_=vp, nv=8, tp_=tp, nt=12, h=0.0, orient=0, voxel=0.005, scale=1.0, cap=0, n_=C.byref(n): L.stocs_preprocess_model_mesh(
        vp_, nv, tp_, nt, h, 1, orient, voxel, scale, -1, None, None, cap, n_)
    assert call(nv=-1, h=np.nan, orient=2, voxel=0.0, scale=np.nan, cap=-1, n_=None) == INVALID and b"n_out" in err()
    assert call(nv=-1, h=np.nan, orient=2, voxel=0.0, scale=np.nan, cap=-1) == INVALID and b"< 0" in err()
    v2 = v.copy(); v2[0, 0] = np.nan
    assert call(vp_=v2.ctypes.data_as(capi._fp), h=np.nan, orient=2, voxel=0.0, scale=np.nan, cap=-1) == INVALID and b"finite" in err()
    for h in (np.nan, np.inf, -0.001):
        assert call(h=h, orient=2, voxel=0.0, scale=np.nan, cap=-1) == INVALID and b"spacing" in err()
    assert call(orient=2, voxel=0.0, scale=np.nan, cap=-1) == INVALID and b"orient" in err()      # spacing 0 is the default, not an error
    for voxel in (0.0, -0.005, np.nan, np.inf):
        assert call(voxel=voxel, scale=np.nan, cap=-1) == INVALID and b"voxel_size" in err()
    assert call(scale=np.nan, cap=-1) == INVALID and b"model_scale" in err()
    assert call(cap=-1) == INVALID and b"cap" in err()
    assert n.value == -7
    assert call(nv=0, vp_=None, nt=0, tp_=None) == 0 and n.value == 0
