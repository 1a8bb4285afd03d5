"""CPU-side checks of the multi-object frame ingest's C ABI (stocs_ingest_scene_multi): the library exports it, the header that
declares it still compiles as C99, and the ctypes binding resolves it.  No GPU compute here."""
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


def test_library_exports_ingest_scene_multi(capi):
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "stocs_ingest_scene_multi")


def test_header_declares_ingest_scene_multi_as_c99(tmp_path):
    src = tmp_path / "multi_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(const stocs_camera* cam, const uint16_t* depth, const uint16_t* probs, float* pos, float* nrm, float* prob, int32_t* px) {\n"
        "    float thr[2] = {0.1f, 0.5f};\n"
        "    int32_t off[STOCS_MAX_FRAME_OBJECTS + 1];\n"
        "    return stocs_ingest_scene_multi(cam, depth, 2, probs, thr, 0.005f, -1, pos, nrm, prob, px, 100, off);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_capi_binds_ingest_scene_multi(capi):
    L = capi.load()
    fn = L.stocs_ingest_scene_multi
    assert fn.restype is C.c_int and len(fn.argtypes) == 13
    assert "stocs_ingest_scene_multi" in capi.SIGNATURES
    from model_matching_amd import estimator
    assert callable(estimator.ingest_scene_multi) and callable(estimator.estimate_objects)


def test_argument_errors_come_before_any_device_work(capi):
    """n_objects outside 1..64, NULL images and a non-finite threshold are STOCS_ERR_INVALID whether or not a GPU is present."""
    import numpy as np
    L = capi.load()
    H, W = 8, 8
    cam = capi.Camera(500.0, 4.0, 500.0, 4.0, 1e-3, W, H, 0)
    d = np.ones((H, W), np.uint16); p = np.ones((65, H, W), np.uint16); thr = np.full(65, 0.1, np.float32)
    off = np.zeros(66, np.int32)
    u16 = C.POINTER(C.c_uint16)

    def call(n, depth=d, probs=p, t=thr):
        return L.stocs_ingest_scene_multi(C.byref(cam), None if depth is None else depth.ctypes.data_as(u16), n,
                                          None if probs is None else probs.ctypes.data_as(u16), t.ctypes.data_as(capi._fp), 0.005, -1,
                                          None, None, None, None, 0, off.ctypes.data_as(capi._ip))
    assert call(0) == capi.ERR_INVALID and call(65) == capi.ERR_INVALID
    assert call(2, depth=None) == capi.ERR_INVALID and call(2, probs=None) == capi.ERR_INVALID
    bad = thr.copy(); bad[1] = np.nan
    assert call(2, t=bad) == capi.ERR_INVALID
    bad[1] = np.inf
    assert call(2, t=bad) == capi.ERR_INVALID
