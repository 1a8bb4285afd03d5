"""CPU-side checks of the C ABI of the segment shapes and the size gate: struct sizes, the header against the bindings, the defaults and
the edges of stocs_check_segment_gate_params, the argument checks that need no device in the order the header states, and the host-only
gate against the restatement, with the widest extent exactly at either threshold and one float either side.  No GPU compute."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import segment_shapes_cases as shc  # noqa: E402
import segment_shapes_ref as shr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, CAPACITY = -1, -4
F = np.float32


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def gate_params(capi, **kw):
    g = capi.SegmentGateParams()
    capi.load().stocs_default_segment_gate_params(C.byref(g))
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_struct_sizes_and_the_bindings(capi):
    S, R, O, G = capi.SegmentShape, capi.SegmentShapesResult, capi.ObjectSize, capi.SegmentGateParams
    assert (C.sizeof(S), C.sizeof(R), C.sizeof(O), C.sizeof(G)) == (128, 32, 16, 16)
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 20, 32, 68, 80, 92, 104]
    assert capi.SHAPE_DTYPE.itemsize == 128 and capi.OBJECT_DTYPE.itemsize == 16 and capi.SHAPE_DTYPE == shr.SHAPE_DTYPE
    assert [capi.SHAPE_DTYPE.fields[f][1] for f, _ in S._fields_] == [getattr(S, f).offset for f, _ in S._fields_]
    assert [f for f, _ in R._fields_] == ["n_labelled", "n_used", "n_invalid", "n_far", "n_out_of_range", "reserved"]
    assert (capi.SHAPE_EMPTY, capi.SHAPE_NONFINITE) == (shr.EMPTY, shr.NONFINITE)
    assert (capi.GATE_TOO_LARGE, capi.GATE_TOO_SMALL, capi.GATE_NO_SHAPE) == (shr.TOO_LARGE, shr.TOO_SMALL, shr.NO_SHAPE)
    from model_matching_amd import estimator
    for name in ("segment_shapes", "points_shape", "object_size", "segment_gate", "segment_assign", "segment_gate_params"):
        assert callable(getattr(estimator, name)), name


def test_header_agrees_as_c99(capi, tmp_path):
    src = tmp_path / "shape_sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\n"
        "int main(void) {\n"
        "    printf(\"%d %d %d %d %d %d %d %d %d %d %d\\n\", (int)sizeof(stocs_segment_shape), (int)sizeof(stocs_segment_shapes_result), (int)sizeof(stocs_object_size),\n"
        "           (int)sizeof(stocs_segment_gate_params), (int)offsetof(stocs_segment_shape, axis), (int)offsetof(stocs_segment_shape, extent),\n"
        "           (int)offsetof(stocs_segment_shape, reserved), STOCS_SHAPE_EMPTY, STOCS_GATE_TOO_LARGE | STOCS_GATE_TOO_SMALL | STOCS_GATE_NO_SHAPE,\n"
        "           STOCS_MAX_FRAME_OBJECTS, (int)(stocs_segment_assign != 0 && stocs_points_shape != 0 && stocs_segment_shapes != 0 && stocs_segment_gate != 0));\n"
        "    return 0;\n}\n")
    exe = tmp_path / "shape_sizes"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-Wno-address", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", os.path.dirname(capi.LIB_PATH), "-lstocs_hip", "-Wl,-rpath," + os.path.dirname(capi.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [128, 32, 16, 16, 32, 92, 104, 1, 7, capi.MAX_FRAME_OBJECTS, 1]


def test_defaults_and_the_edges_of_the_parameter_check(capi):
    L = capi.load()
    g = gate_params(capi)
    assert (g.slack, g.min_ratio, g.min_used, g.reserved) == (0.25, 0.5, 3, 0)
    assert shr.GATE_DEFAULTS == dict(slack=g.slack, min_ratio=g.min_ratio, min_used=g.min_used)
    assert L.stocs_check_segment_gate_params(C.byref(g)) == 0
    assert L.stocs_check_segment_gate_params(None) == INVALID and b"NULL" in L.stocs_last_error()
    L.stocs_default_segment_gate_params(None)
    nan, inf = float("nan"), float("inf")
    for field, value in [("slack", -1e-6), ("slack", inf), ("slack", nan), ("min_ratio", -1e-6), ("min_ratio", 1.0001), ("min_ratio", nan), ("min_ratio", inf), ("min_used", 0),
                         ("min_used", -2), ("reserved", 1)]:
        assert L.stocs_check_segment_gate_params(C.byref(gate_params(capi, **{field: value}))) == INVALID, (field, value)
        assert field.encode() in L.stocs_last_error()
    for field, value in [("slack", 0.0), ("slack", 1e6), ("min_ratio", 0.0), ("min_ratio", 1.0), ("min_used", 1), ("min_used", 1 << 30)]:
        assert L.stocs_check_segment_gate_params(C.byref(gate_params(capi, **{field: value}))) == 0, (field, value)
    n = C.c_int(0)
    assert L.stocs_segment_shapes_table(C.byref(n)) == 0 and n.value == shc.TABLE_SLOTS and L.stocs_segment_shapes_table(None) == 0


def test_argument_checks_that_need_no_device_in_the_stated_order(capi):
    L = capi.load()
    depth = np.full((4, 8), 1000, np.uint16); lab = np.ones((4, 8), np.int32)
    dp, lp = depth.ctypes.data_as(C.POINTER(C.c_uint16)), lab.ctypes.data_as(capi._ip)
    cam = capi.Camera(10.0, 3.5, 10.0, 1.5, 0.001, 8, 4, 0)
    res = capi.SegmentShapesResult()
    shapes = (capi.SegmentShape * 2)()
    obj = (capi.ObjectSize * 2)(); obj[0].diameter = 0.2; obj[1].diameter = 0.3
    reasons = (C.c_uint8 * 4)(); stack = (C.c_uint16 * 64)()
    bad_g = gate_params(capi, min_used=0)
    err = L.stocs_last_error

    def call(c=C.byref(cam), d=dp, l=lp, nl=2, md=2.0, o=obj, no=2, g=None, s=shapes, rs=reasons, st=stack, r=C.byref(res)):
        return L.stocs_segment_assign(c, d, l, nl, md, o, no, g, -1, s, None, rs, st, r)
    # 1. the NULLs first: a bad n_labels, n_objects and parameters beside them go unnoticed
    for kw in (dict(c=None), dict(d=None), dict(l=None), dict(r=None)):
        assert call(nl=-1, no=99, md=-1.0, **kw) == INVALID and b"NULL camera" in err()
    # 2. n_labels and the frame
    assert call(nl=-1, no=99) == INVALID and b"n_labels" in err()
    assert call(nl=(1 << 22) + 1, no=99) == INVALID and b"n_labels" in err()
    for w, h in ((0, 4), (8, -1)):
        assert call(c=C.byref(capi.Camera(10.0, 3.5, 10.0, 1.5, 0.001, w, h, 0)), no=99) == INVALID and b"pixels" in err()
    assert call(c=C.byref(capi.Camera(10.0, 3.5, 10.0, 1.5, 0.001, 4096, 1025, 0)), no=99) == CAPACITY and b"2^22" in err()
    # 3. n_objects
    for no in (-1, capi.MAX_FRAME_OBJECTS + 1):
        assert call(no=no, s=None) == INVALID and b"n_objects" in err()
    # 4. the outputs the counts require
    assert call(s=None, md=-1.0) == INVALID and b"NULL shapes" in err()
    for kw in (dict(o=None), dict(rs=None), dict(st=None)):
        assert call(md=-1.0, **kw) == INVALID and b"class_stack" in err()
    # 5. the parameters
    assert call(md=0.0, g=C.byref(bad_g)) == INVALID and b"max_depth" in err()
    assert call(md=float("inf")) == INVALID and b"max_depth" in err()
    assert call(g=C.byref(bad_g)) == INVALID and b"min_used" in err()
    obj[1].extent[2] = -0.1
    assert call() == INVALID and b"object 1" in err()
    obj[1].extent[2] = 0.0
    # the shapes call and the points call
    assert L.stocs_segment_shapes(None, dp, lp, 2, 2.0, -1, shapes, None, C.byref(res)) == INVALID and b"NULL camera" in err()
    assert L.stocs_segment_shapes(C.byref(cam), dp, lp, 2, 2.0, -1, None, None, C.byref(res)) == INVALID and b"NULL shapes" in err()
    pts = np.zeros((4, 3), np.float32)
    assert L.stocs_points_shape(pts.ctypes.data_as(capi._fp), 4, -1, None, None) == INVALID
    assert L.stocs_points_shape(None, 4, -1, shapes, None) == INVALID
    assert L.stocs_points_shape(pts.ctypes.data_as(capi._fp), -1, -1, shapes, None) == INVALID
    assert L.stocs_points_shape(pts.ctypes.data_as(capi._fp), (1 << 22) + 1, -1, shapes, None) == CAPACITY
    from model_matching_amd import estimator
    with pytest.raises(TypeError):
        estimator.segment_gate_params(no_such_field=1)
    with pytest.raises(capi.StocsError):
        estimator.segment_gate_params(min_ratio=2.0)


def shapes_with(extents, n_used=10, flags=0):
    s = np.zeros(len(extents), shr.SHAPE_DTYPE)
    s["extent"] = np.asarray(extents, F); s["n_used"] = n_used; s["flags"] = flags
    return s


def test_host_gate_against_the_restatement_at_its_edges(capi):
    from model_matching_amd import estimator
    up, down = (lambda v: np.nextafter(F(v), F(np.inf))), (lambda v: np.nextafter(F(v), F(-np.inf)))
    for slack, min_ratio, diam, m in ((0.25, 0.5, 0.31, (0.25, 0.17, 0.06)), (0.1, 0.7, 0.123, (0.1, 0.07, 0.03)), (0.0, 1.0, 1.0, (0.9, 0.9, 0.1))):
        widest = F(F(1) + F(slack)) * F(diam)
        least = F(min_ratio) * np.sort(np.asarray(m, F))[::-1][1]
        e1 = [down(widest), widest, up(widest), down(least), least, up(least)]
        shapes = shapes_with([[0.0, e, 0.001] for e in e1])              # the widest extent in the middle slot: the gate sorts by value
        obj = np.zeros(1, capi.OBJECT_DTYPE); obj["diameter"] = diam; obj["extent"] = (m[2], m[0], m[1])
        got = estimator.segment_gate(shapes, obj, slack=slack, min_ratio=min_ratio)
        want = shr.gate(shapes, [(F(diam), np.asarray(obj["extent"][0], F))], slack=slack, min_ratio=min_ratio)
        assert got.tolist() == want.tolist()
        L, S = shr.TOO_LARGE, shr.TOO_SMALL
        assert got[0].tolist() == [0, 0, L, S, 0, 0], (slack, min_ratio, got)
    # NO_SHAPE: min_used at its edge, either flag
    shapes = shapes_with([[0.2, 0.1, 0.1]] * 4)
    shapes["n_used"] = (2, 3, 10, 10); shapes["flags"] = (0, 0, shr.EMPTY, shr.NONFINITE)
    obj = np.zeros(2, capi.OBJECT_DTYPE); obj["diameter"] = (0.25, 0.25); obj["extent"] = ((0.2, 0.1, 0.1), (0.2, 0.2, 0.1))
    got = estimator.segment_gate(shapes, obj)
    assert got.tolist() == [[4, 0, 4, 4], [4, 0, 4, 4]] and got.tolist() == shr.gate(shapes, [(o["diameter"], o["extent"]) for o in obj]).tolist()
    assert estimator.segment_gate(shapes, obj, min_used=2)[0].tolist() == [0, 0, 4, 4]
    assert estimator.segment_gate(shapes[:0], obj).shape == (2, 0) and estimator.segment_gate(shapes, obj[:0]).shape == (0, 4)
    # the ray-cast scenes through the host gate
    for name in shc.GATE_SCENES:
        c, objects = shc.gate_scene(name)
        s, _, _ = shr.segment_shapes(c["depth"], c["labels"], c["K"], c["scale"], c["n_labels"], c["max_depth"])
        o = np.zeros(len(objects), capi.OBJECT_DTYPE)
        for k, (d, e) in enumerate(objects):
            o[k]["diameter"] = d; o[k]["extent"] = e
        assert estimator.segment_gate(s, o).tolist() == shr.gate(s, objects).tolist()


def test_the_build_lists_the_new_file(capi):
    mk = open(os.path.join(ROOT, "model_matching_amd", "csrc", "Makefile")).read()
    assert "segment_shapes.hip" in mk.split("SRCS =")[1].split("\n")[0]
