"""CPU-side checks of the C ABI of the concavity cut: struct sizes and offsets, the header against the bindings, the exported symbols, the
header as C99, the defaults and every refusal of stocs_check_segment_convex_params, and the argument checks that need no device in the order
the header states.  No GPU compute."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import segment_convex_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"stocs_check_segment_convex_params": 1, "stocs_segment_frame_convex": 14, "stocs_segment_last_bend_ms": 1}
INVALID, CAPACITY = -1, -4
FIELDS_P = ["bend_radius", "smooth_radius", "bend_cos", "reserved"]
FIELDS_R = ["n_tested_h", "n_tested_v", "n_cut_h", "n_cut_v", "n_cut", "reserved"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def defaults(capi, **kw):
    cp = capi.SegmentConvexParams()
    capi.load().stocs_default_segment_convex_params(C.byref(cp))
    for k, v in kw.items():
        setattr(cp, k, v)
    return cp


def plain_defaults(capi, **kw):
    p = capi.SegmentParams()
    capi.load().stocs_default_segment_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_struct_sizes_and_offsets(capi):
    P, R = capi.SegmentConvexParams, capi.SegmentConvexResult
    assert (C.sizeof(P), C.sizeof(R)) == (16, 32)
    assert [f for f, _ in P._fields_] == FIELDS_P and [f for f, _ in R._fields_] == FIELDS_R
    assert [getattr(P, f).offset for f in FIELDS_P] == [0, 4, 8, 12] and [getattr(R, f).offset for f in FIELDS_R] == [0, 4, 8, 12, 16, 20]
    assert dict(P._fields_)["bend_cos"] is C.c_float and dict(P._fields_)["bend_radius"] is C.c_int32
    assert (C.sizeof(capi.SegmentParams), C.sizeof(capi.SegmentResult), C.sizeof(capi.SegmentRecord)) == (48, 64, 32)       # the older structs did not move


def test_header_agrees_with_the_bindings(capi, tmp_path):
    src = tmp_path / "segment_convex_sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\n"
        "int main(void) {\n"
        "    printf(\"%d %d %d %d %d %d %d\\n\", (int)sizeof(stocs_segment_convex_params), (int)sizeof(stocs_segment_convex_result),\n"
        "           (int)offsetof(stocs_segment_convex_params, smooth_radius), (int)offsetof(stocs_segment_convex_params, bend_cos), (int)offsetof(stocs_segment_convex_params, reserved),\n"
        "           (int)offsetof(stocs_segment_convex_result, n_cut), (int)offsetof(stocs_segment_convex_result, reserved));\n"
        "    return 0;\n}\n")
    exe = tmp_path / "segment_convex_sizes"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [16, 32, 4, 8, 12, 16, 20]


def test_library_exports_the_symbols(capi):
    lib = C.CDLL(capi.LIB_PATH)
    L = capi.load()
    assert hasattr(lib, "stocs_default_segment_convex_params") and L.stocs_default_segment_convex_params.restype is None
    for name, n_args in NAMES.items():
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args, name
    from model_matching_amd import estimator
    for name in ("segment_frame", "segment_convex_params", "segment_last_bend_ms"):
        assert callable(getattr(estimator, name)), name


def test_header_declares_them_as_c99(capi, tmp_path):
    src = tmp_path / "segment_convex_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(const stocs_camera* cam, const uint16_t* depth, uint16_t* cls, int32_t* lab, uint8_t* edge, uint8_t* cut, float* zs, stocs_segment_record* rec) {\n"
        "    stocs_segment_params p;\n"
        "    stocs_segment_convex_params cp;\n"
        "    stocs_segment_result out;\n"
        "    stocs_segment_convex_result cout;\n"
        "    float ms;\n"
        "    int rc;\n"
        "    stocs_default_segment_params(&p);\n"
        "    stocs_default_segment_convex_params(&cp);\n"
        "    rc = stocs_check_segment_convex_params(&cp);\n"
        "    rc = rc ? rc : stocs_segment_frame_convex(cam, depth, &p, &cp, -1, cls, lab, edge, cut, zs, rec, 16, &out, &cout);\n"
        "    rc = rc ? rc : stocs_segment_last_bend_ms(&ms);\n"
        "    return rc ? rc : out.n_segments + cout.n_cut + cout.n_tested_h + cout.reserved[2] + (ms > 0);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_defaults_and_every_refusal_of_the_parameter_check(capi):
    L = capi.load()
    cp = defaults(capi)
    f = lambda v: C.c_float(v).value
    assert (cp.bend_radius, cp.smooth_radius, cp.bend_cos, cp.reserved) == (4, 2, f(0.90630779), 0)
    assert abs(cp.bend_cos - np.cos(np.deg2rad(25.0))) < 1e-7
    for k, v in cr.CONVEX_DEFAULTS.items():                  # the restatement's defaults are the library's
        assert getattr(cp, k) == (f(v) if isinstance(v, float) else v), k
    assert L.stocs_check_segment_convex_params(C.byref(cp)) == 0
    assert L.stocs_check_segment_convex_params(None) == INVALID and b"NULL" in L.stocs_last_error()
    L.stocs_default_segment_convex_params(None)   # a no-op
    nan, inf = float("nan"), float("inf")
    refused = [("bend_radius", -1), ("bend_radius", 9), ("smooth_radius", -1), ("smooth_radius", 5)] + [("bend_cos", v) for v in (-0.01, 1.01, nan, inf, -inf)] + \
        [("reserved", 1), ("reserved", -1)]
    for field, value in refused:
        q = defaults(capi, **{field: value})
        assert L.stocs_check_segment_convex_params(C.byref(q)) == INVALID, (field, value)
        assert field.encode() in L.stocs_last_error(), (field, value, L.stocs_last_error())
    for field, value in [("bend_radius", 0), ("bend_radius", 8), ("smooth_radius", 0), ("smooth_radius", 4), ("bend_cos", 0.0), ("bend_cos", 1.0)]:
        assert L.stocs_check_segment_convex_params(C.byref(defaults(capi, **{field: value}))) == 0, (field, value)


def test_argument_checks_that_need_no_device_in_the_stated_order(capi, monkeypatch):
    L = capi.load()
    u16p = C.POINTER(C.c_uint16)
    depth = np.full((4, 8), 1000, np.uint16)
    dp = depth.ctypes.data_as(u16p)
    cam = capi.Camera(10.0, 3.5, 10.0, 1.5, 0.001, 8, 4, 0)
    nocam = capi.Camera(10.0, 3.5, 10.0, 1.5, 0.001, 0, 4, 0)
    good, bad = plain_defaults(capi), plain_defaults(capi, min_pixels=0)
    cgood, cbad = defaults(capi), defaults(capi, bend_radius=9)
    out, cout = capi.SegmentResult(), capi.SegmentConvexResult()
    rec = (capi.SegmentRecord * 4)()
    call = lambda c, d, p, cp, r, cap, o, co: L.stocs_segment_frame_convex(c, d, p, cp, -1, None, None, None, None, None, r, cap, o, co)
    # 1. NULL arguments come first, cp and cout among them: with one, a bad size, bad parameters and bad records go unnoticed
    B = C.byref
    for args in ((None, dp, B(bad), B(cbad), None, 3, B(out), B(cout)), (B(nocam), None, B(bad), B(cbad), None, 3, B(out), B(cout)),
                 (B(nocam), dp, None, B(cbad), None, 3, B(out), B(cout)), (B(nocam), dp, B(bad), None, None, 3, B(out), B(cout)),
                 (B(nocam), dp, B(bad), B(cbad), None, 3, None, B(cout)), (B(nocam), dp, B(bad), B(cbad), None, 3, B(out), None)):
        assert call(*args) == INVALID and b"stocs_segment_frame_convex: NULL camera" in L.stocs_last_error()
    # 2. then the size
    for w, h in ((0, 4), (8, 0), (-1, 4)):
        c2 = capi.Camera(10.0, 3.5, 10.0, 1.5, 0.001, w, h, 0)
        assert call(B(c2), dp, B(bad), B(cbad), None, 3, B(out), B(cout)) == INVALID and b"pixels" in L.stocs_last_error()
    # 3. then the parameters, 4. the convex parameters right after them
    assert call(B(cam), dp, B(bad), B(cbad), None, 3, B(out), B(cout)) == INVALID and b"min_pixels" in L.stocs_last_error()
    assert call(B(cam), dp, B(good), B(cbad), None, 3, B(out), B(cout)) == INVALID and b"bend_radius" in L.stocs_last_error()
    # 5. then the records
    assert call(B(cam), dp, B(good), B(cgood), None, 3, B(out), B(cout)) == INVALID and b"cap_records" in L.stocs_last_error()
    assert call(B(cam), dp, B(good), B(cgood), rec, -1, B(out), B(cout)) == INVALID and b"cap_records" in L.stocs_last_error()
    # 6. then the frame's size against the moments' range, the label form, the bend form
    big = capi.Camera(10.0, 3.5, 10.0, 1.5, 0.001, 4096, 1025, 0)
    assert call(B(big), dp, B(good), B(cgood), rec, 4, B(out), B(cout)) == CAPACITY and b"2^22" in L.stocs_last_error()
    monkeypatch.setenv("STOCS_SEGMENT_FORM", "3")
    monkeypatch.setenv("STOCS_SEGMENT_BEND_FORM", "3")
    assert call(B(cam), dp, B(good), B(cgood), rec, 4, B(out), B(cout)) == INVALID and b"STOCS_SEGMENT_FORM" in L.stocs_last_error()
    monkeypatch.delenv("STOCS_SEGMENT_FORM")
    assert call(B(cam), dp, B(good), B(cgood), rec, 4, B(out), B(cout)) == INVALID and b"STOCS_SEGMENT_BEND_FORM" in L.stocs_last_error()
    # the plain entry point does not read the bend form
    r = L.stocs_segment_frame(B(cam), dp, B(bad), -1, None, None, None, rec, 4, B(out))
    assert r == INVALID and b"min_pixels" in L.stocs_last_error()
    monkeypatch.delenv("STOCS_SEGMENT_BEND_FORM")
    from model_matching_amd import estimator
    with pytest.raises(TypeError):
        estimator.segment_convex_params(no_such_field=1)
    with pytest.raises(capi.StocsError):
        estimator.segment_convex_params(smooth_radius=5)
    assert estimator.segment_convex_params(bend_radius=8, bend_cos=0.5).bend_cos == 0.5


def test_the_driver_refuses_the_option_without_segment(capi, tmp_path):
    app = os.path.join(ROOT, "model_matching_amd", "apps", "stocs_single")
    for extra in (["--segment-convex"], ["--segment-convex", "4,2,25"], ["--segment", "--segment-convex", "9"], ["--segment", "--segment-convex", "4,5"],
                  ["--segment", "--segment-convex", "4,2,91"], ["--segment", "--segment-convex", "4,2,25,1"]):
        r = subprocess.run([app, str(tmp_path), "no_object"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--segment-convex [r[,s[,deg]]] needs --segment" in r.stderr, (extra, r.stderr)
