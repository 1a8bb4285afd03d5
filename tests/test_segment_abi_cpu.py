"""CPU-side checks of the C ABI of the depth-only segmentation: struct sizes and offsets, the header against the bindings, the exported
symbols, the header as C99, the defaults and every refusal of stocs_check_segment_params, the argument checks that need no device in the order
the header states, and the Makefile.  No GPU compute."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import segment_cases as sc
import segment_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"stocs_check_segment_params": 1, "stocs_segment_frame": 10, "stocs_segment_tile": 2, "stocs_segment_last_device_ms": 2, "stocs_segment_last_moments": 1}
INVALID, CAPACITY = -1, -4
FIELDS_P = ["max_depth", "plane_hypotheses", "score_stride", "plane_tolerance", "plane_min_share", "max_height", "jump_abs", "jump_rel", "min_pixels", "seed"]
FIELDS_R = ["plane", "plane_found", "winner", "winner_count", "n_valid", "n_scored", "n_refit", "n_on_plane", "n_above", "n_below", "n_components", "n_segments",
            "reserved"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def defaults(capi, **kw):
    p = capi.SegmentParams()
    capi.load().stocs_default_segment_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_struct_sizes_and_offsets(capi):
    P, R, S = capi.SegmentParams, capi.SegmentResult, capi.SegmentRecord
    assert (C.sizeof(P), C.sizeof(R), C.sizeof(S)) == (48, 64, 32)
    assert [f for f, _ in P._fields_] == FIELDS_P and [f for f, _ in R._fields_] == FIELDS_R
    assert [getattr(P, f).offset for f in FIELDS_P] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    assert [getattr(R, f).offset for f in FIELDS_R] == [0] + list(range(16, 64, 4))
    assert [f for f, _ in S._fields_] == ["root", "pixels", "c0", "r0", "c1", "r1", "zmin", "zmax"]
    assert [getattr(S, f).offset for f, _ in S._fields_] == list(range(0, 32, 4))
    assert dict(S._fields_)["zmin"] is C.c_float and dict(P._fields_)["seed"] is C.c_uint64


def test_header_agrees_with_the_bindings(capi, tmp_path):
    src = tmp_path / "segment_sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\n"
        "int main(void) {\n"
        "    printf(\"%d %d %d %d %d %d %d %d %d\\n\", (int)sizeof(stocs_segment_params), (int)sizeof(stocs_segment_result), (int)sizeof(stocs_segment_record),\n"
        "           (int)offsetof(stocs_segment_params, min_pixels), (int)offsetof(stocs_segment_params, seed), (int)offsetof(stocs_segment_params, jump_rel),\n"
        "           (int)offsetof(stocs_segment_result, plane_found), (int)offsetof(stocs_segment_result, n_segments), (int)offsetof(stocs_segment_record, zmin));\n"
        "    return 0;\n}\n")
    exe = tmp_path / "segment_sizes"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [48, 64, 32, 32, 40, 28, 16, 56, 24]


def test_library_exports_the_symbols(capi):
    lib = C.CDLL(capi.LIB_PATH)
    L = capi.load()
    assert hasattr(lib, "stocs_default_segment_params") and L.stocs_default_segment_params.restype is None
    for name, n_args in NAMES.items():
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args, name
    from model_matching_amd import estimator
    for name in ("segment_frame", "segment_class_images", "segment_params", "segment_last_device_ms", "segment_last_moments"):
        assert callable(getattr(estimator, name)), name


def test_header_declares_them_as_c99(capi, tmp_path):
    src = tmp_path / "segment_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(const stocs_camera* cam, const uint16_t* depth, uint16_t* cls, int32_t* lab, uint8_t* edge, stocs_segment_record* rec, int64_t* mom) {\n"
        "    stocs_segment_params p;\n"
        "    stocs_segment_result out;\n"
        "    float ms[2];\n"
        "    int w, h, rc;\n"
        "    stocs_default_segment_params(&p);\n"
        "    rc = stocs_check_segment_params(&p);\n"
        "    rc = rc ? rc : stocs_segment_frame(cam, depth, &p, -1, cls, lab, edge, rec, 16, &out);\n"
        "    rc = rc ? rc : stocs_segment_tile(&w, &h);\n"
        "    rc = rc ? rc : stocs_segment_last_device_ms(&ms[0], &ms[1]);\n"
        "    rc = rc ? rc : stocs_segment_last_moments(mom);\n"
        "    return rc ? rc : out.n_segments + rec[0].pixels + w + h + (ms[0] > ms[1]);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_defaults_and_every_refusal_of_the_parameter_check(capi):
    L = capi.load()
    p = defaults(capi)
    f = lambda v: C.c_float(v).value
    assert (p.max_depth, p.plane_hypotheses, p.score_stride, p.plane_tolerance, p.plane_min_share, p.max_height, p.jump_abs, p.jump_rel, p.min_pixels, p.seed) == \
        (2.0, 1024, 4, f(0.01), f(0.15), 0.5, f(0.005), f(0.01), 200, 1)
    for k, v in sr.DEFAULTS.items():                        # the restatement's defaults are the library's
        assert getattr(p, k) == (f(v) if isinstance(v, float) else v), k
    assert L.stocs_check_segment_params(C.byref(p)) == 0
    assert L.stocs_check_segment_params(None) == INVALID and b"NULL" in L.stocs_last_error()
    L.stocs_default_segment_params(None)   # a no-op
    nan, inf = float("nan"), float("inf")
    refused = [("max_depth", v) for v in (0.0, -1.0, inf, nan)] + [("plane_hypotheses", -1), ("plane_hypotheses", (1 << 20) + 1), ("score_stride", 0), ("score_stride", -3)] + \
        [("plane_tolerance", v) for v in (0.0, -0.01, inf, nan)] + [("plane_min_share", v) for v in (-0.01, 1.01, nan, inf)] + \
        [("max_height", v) for v in (0.0, -0.5, inf, nan)] + [("jump_abs", v) for v in (-0.001, inf, nan)] + [("jump_rel", v) for v in (-0.001, inf, nan)] + \
        [("min_pixels", 0), ("min_pixels", -7)]
    for field, value in refused:
        q = defaults(capi, **{field: value})
        assert L.stocs_check_segment_params(C.byref(q)) == INVALID, (field, value)
        assert field.encode() in L.stocs_last_error(), (field, value, L.stocs_last_error())
    accepted = [("max_depth", 1e-6), ("max_depth", 60.0), ("plane_hypotheses", 0), ("plane_hypotheses", 1 << 20), ("score_stride", 1), ("score_stride", 1000),
                ("plane_tolerance", 1e-9), ("plane_min_share", 0.0), ("plane_min_share", 1.0), ("max_height", 1e-6), ("jump_abs", 0.0), ("jump_rel", 0.0),
                ("min_pixels", 1), ("seed", (1 << 64) - 1)]
    for field, value in accepted:
        assert L.stocs_check_segment_params(C.byref(defaults(capi, **{field: value}))) == 0, (field, value)


def test_the_tile_is_the_one_the_cases_are_built_for(capi):
    L = capi.load()
    w, h = C.c_int(0), C.c_int(0)
    assert L.stocs_segment_tile(C.byref(w), C.byref(h)) == 0 and (w.value, h.value) == sc.TILE
    assert L.stocs_segment_tile(None, None) == 0
    assert any(W % w.value == 0 for W, _ in sc.SIZES) and any(W % w.value == 1 for W, _ in sc.SIZES) and any(W % w.value == w.value - 1 for W, _ in sc.SIZES)
    assert {H - h.value for _, H in sc.SIZES} >= {-1, 0, 1}


def test_argument_checks_that_need_no_device_in_the_stated_order(capi, monkeypatch):
    L = capi.load()
    u16p = C.POINTER(C.c_uint16)
    depth = np.full((4, 8), 1000, np.uint16)
    dp = depth.ctypes.data_as(u16p)
    cam = capi.Camera(10.0, 3.5, 10.0, 1.5, 0.001, 8, 4, 0)
    good, bad = defaults(capi), defaults(capi, min_pixels=0)
    out = capi.SegmentResult()
    rec = (capi.SegmentRecord * 4)()
    call = lambda c, d, p, r, cap, o: L.stocs_segment_frame(c, d, p, -1, None, None, None, r, cap, o)
    nocam = capi.Camera(10.0, 3.5, 10.0, 1.5, 0.001, 0, 4, 0)
    # 1. NULL arguments come first: with them, a bad size, bad parameters and bad records go unnoticed
    for args in ((None, dp, C.byref(bad), None, 3, C.byref(out)), (C.byref(nocam), None, C.byref(bad), None, 3, C.byref(out)), (C.byref(nocam), dp, None, None, 3, C.byref(out)),
                 (C.byref(nocam), dp, C.byref(bad), None, 3, None)):
        assert call(*args) == INVALID and b"NULL camera" in L.stocs_last_error()
    # 2. then the size
    for w, h in ((0, 4), (8, 0), (-1, 4)):
        c2 = capi.Camera(10.0, 3.5, 10.0, 1.5, 0.001, w, h, 0)
        assert call(C.byref(c2), dp, C.byref(bad), None, 3, C.byref(out)) == INVALID and b"pixels" in L.stocs_last_error()
    # 3. then the parameters
    assert call(C.byref(cam), dp, C.byref(bad), None, 3, C.byref(out)) == INVALID and b"min_pixels" in L.stocs_last_error()
    # 4. then the records
    assert call(C.byref(cam), dp, C.byref(good), None, 3, C.byref(out)) == INVALID and b"cap_records" in L.stocs_last_error()
    assert call(C.byref(cam), dp, C.byref(good), rec, -1, C.byref(out)) == INVALID and b"cap_records" in L.stocs_last_error()
    # 5. then the frame's size against the moments' range, and the form
    big = capi.Camera(10.0, 3.5, 10.0, 1.5, 0.001, 4096, 1025, 0)
    assert call(C.byref(big), dp, C.byref(good), rec, 4, C.byref(out)) == CAPACITY and b"2^22" in L.stocs_last_error()
    monkeypatch.setenv("STOCS_SEGMENT_FORM", "3")
    assert call(C.byref(cam), dp, C.byref(good), rec, 4, C.byref(out)) == INVALID and b"STOCS_SEGMENT_FORM" in L.stocs_last_error()
    monkeypatch.delenv("STOCS_SEGMENT_FORM")
    assert L.stocs_segment_last_moments(None) == INVALID
    from model_matching_amd import estimator
    with pytest.raises(TypeError):
        estimator.segment_params(no_such_field=1)
    with pytest.raises(capi.StocsError):
        estimator.segment_params(min_pixels=0)
    stack = estimator.segment_class_images(np.array([[0, 1, 2], [2, 2, 3]]), ids=[2, [1, 3]])
    assert stack.dtype == np.uint16 and stack.tolist() == [[[0, 0, 10000], [10000, 10000, 0]], [[0, 10000, 0], [0, 0, 10000]]]


def test_the_build_lists_the_new_file(capi):
    mk = open(os.path.join(ROOT, "model_matching_amd", "csrc", "Makefile")).read()
    assert "segment.hip" in mk.split("SRCS =")[1].split("\n")[0]
