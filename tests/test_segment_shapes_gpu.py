"""stocs_segment_shapes, stocs_points_shape and stocs_segment_assign on the GPU against the numpy restatement (tests/segment_shapes_ref.py).
Bit for bit: the counts, all ten moments, the centroid (the double formula cast once), lo, hi and extent given the device's own centroid
and axes, the reasons and the class stack.  The axes and eigenvalues are judged against numpy's float64 eigh of the covariance formed from
the integer moments, on the cases named in segment_shapes_cases.SEPARATED (eigenvalue gaps of at least 5 % of the largest): an angle of
at most 1e-6 rad (the cast to float moves a unit vector by about 1.1e-7 rad at most, the double Jacobi error at that gap is below 1e-12:
a factor of ten is left) and eigenvalues within 1e-6 relative.  Every call goes through buffers with sentinel bytes behind them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import segment_shapes_cases as shc  # noqa: E402
import segment_shapes_ref as shr  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0xA5
PAD = 64
COUNTS = ("n_labelled", "n_used", "n_invalid", "n_far", "n_out_of_range")
MAX_ANGLE, MAX_REL = 1e-6, 1e-6


@pytest.fixture(scope="module")
def lib():
    from model_matching_amd import capi
    return capi, capi.load()


def padded(nbytes):
    return np.full(nbytes + PAD, SENTINEL, np.uint8)


def call(lib, c, objects=None, gate=None, want_moments=True, entry="assign"):
    """the raw entry point on sentinel-padded buffers: (rc, shapes, moments, reasons, stack, counts)"""
    capi, L = lib
    d, lab, n = c["depth"], c["labels"], c["n_labels"]
    H, W = d.shape
    no = 0 if objects is None else len(objects)
    raw = {"shapes": padded(128 * n), "moments": padded(80 * n), "reasons": padded(no * n), "stack": padded(2 * no * W * H), "result": padded(32)}
    obj = (capi.ObjectSize * max(no, 1))()
    for k in range(no):
        obj[k].diameter = float(objects[k][0])
        for j in range(3):
            obj[k].extent[j] = float(objects[k][1][j])
    g = None
    if gate is not None:
        g = capi.SegmentGateParams()
        L.stocs_default_segment_gate_params(C.byref(g))
        for k, v in gate.items():
            setattr(g, k, v)
    cam = capi.Camera(c["K"][0], c["K"][1], c["K"][2], c["K"][3], c["scale"], W, H, 0)
    ps = raw["shapes"].ctypes.data_as(C.POINTER(capi.SegmentShape)) if n else None
    pm = raw["moments"].ctypes.data_as(capi._i64p) if want_moments and n else None
    pr = raw["result"].ctypes.data_as(C.POINTER(capi.SegmentShapesResult))
    front = (C.byref(cam), d.ctypes.data_as(C.POINTER(C.c_uint16)), lab.ctypes.data_as(capi._ip), n, c["max_depth"])
    if entry == "shapes":
        rc = L.stocs_segment_shapes(*front, -1, ps, pm, pr)
    else:
        rc = L.stocs_segment_assign(*front, obj if no else None, no, C.byref(g) if g is not None else None, -1, ps, pm,
                                    raw["reasons"].ctypes.data_as(capi._u8p) if no and n else None, raw["stack"].ctypes.data_as(C.POINTER(C.c_uint16)) if no else None, pr)
    for name, a in raw.items():
        assert (a[-PAD:] == SENTINEL).all(), "bytes behind %s were written" % name
    if not want_moments:
        assert (raw["moments"] == SENTINEL).all()
    res = capi.SegmentShapesResult.from_buffer_copy(raw["result"][:32].tobytes())
    return (rc, np.frombuffer(raw["shapes"][:128 * n].tobytes(), shr.SHAPE_DTYPE), raw["moments"][:80 * n].view(np.int64).reshape(n, 10),
            raw["reasons"][:no * n].reshape(no, n), raw["stack"][:2 * no * W * H].view(np.uint16).reshape(no, H, W), {f: getattr(res, f) for f in COUNTS})


_REF = {}


def reference(case_id):
    """the restatement of a frame case, computed once and left unchanged: (case, P, lab, used, counts, moments)"""
    if case_id not in _REF:
        c = shc.big() if case_id == "big" else shc.frame(case_id)
        P, lab, used, counts = shr.used_pixels(c["depth"], c["labels"], c["K"], c["scale"], c["n_labels"], c["max_depth"])
        M = shr.moments(P, lab, used, c["n_labels"])
        for a in (P, lab, used, M, c["depth"], c["labels"]):
            a.setflags(write=False)
        _REF[case_id] = (c, P, lab, used, counts, M)
    return _REF[case_id]


def check_shapes(shapes, P, lab, used, M, n_labels, separated=False):
    """the records against the moments: n_used, flags, the centroid bit for bit, lo / hi / extent bit for bit on the device's own centroid and axes"""
    assert shapes["n_used"].tolist() == M[:, 0].tolist()
    assert shapes["flags"].tolist() == [shr.EMPTY if m == 0 else 0 for m in M[:, 0]]
    assert not shapes["reserved"].any()
    for l in range(n_labels):
        if M[l, 0] == 0:
            assert shapes[l].tobytes() == bytes(4) + (1).to_bytes(4, "little") + bytes(120)
            continue
        c64, _ = shr.covariance(M[l])
        assert shapes[l]["centroid"].tobytes() == np.array(c64, np.float64).astype(F).tobytes(), l
        ax = shapes[l]["axis"].astype(np.float64)
        assert np.abs(ax @ ax.T - np.eye(3)).max() < 1e-6, l                                    # unit and orthogonal to float precision, every case
        for k in range(3):
            assert ax[k][np.argmax(np.abs(ax[k]))] > 0
        assert list(shapes[l]["eigenvalue"]) == sorted(shapes[l]["eigenvalue"], reverse=True)
        if separated:
            w, a64 = shr.eigh64(M[l])
            assert min(w[0] - w[1], w[1] - w[2]) >= shc.MIN_GAP * w[0]
            for k in range(3):
                ang = shr.angle(shapes[l]["axis"][k], a64[k])
                rel = abs(float(shapes[l]["eigenvalue"][k]) - w[k]) / w[k]
                print("label %d axis %d: angle %.3g rad, eigenvalue off by %.3g relative" % (l + 1, k, ang, rel))
                assert ang <= MAX_ANGLE and rel <= MAX_REL, (l, k, ang, rel)
    lo, hi, ext = shr.extents(P, lab, used, shapes["centroid"], shapes["axis"], n_labels)
    assert shapes["lo"].tobytes() == lo.tobytes() and shapes["hi"].tobytes() == hi.tobytes() and shapes["extent"].tobytes() == ext.tobytes()


@pytest.mark.parametrize("case_id", shc.FRAME_IDS)
def test_frames_bit_for_bit(lib, case_id):
    c, P, lab, used, counts, M = reference(case_id)
    rc, shapes, mom, _, _, got = call(lib, c, entry="shapes")
    assert rc == 0, lib[1].stocs_last_error()
    assert got == counts
    assert mom.tolist() == M.tolist()
    check_shapes(shapes, P, lab, used, M, c["n_labels"], separated=case_id in shc.SEPARATED)


def test_big_frame_sums_approach_two_to_the_62(lib):
    c, P, lab, used, counts, M = reference("big")
    rc, shapes, mom, _, _, got = call(lib, c, entry="shapes")
    assert rc == 0, lib[1].stocs_last_error()
    assert got == counts and counts["n_used"] == 1 << 22
    assert mom.tolist() == M.tolist() and 2 ** 61 < int(mom[0, 9]) < 2 ** 62
    check_shapes(shapes, P, lab, used, M, 1)


@pytest.mark.parametrize("name", sorted(shc.GATE_SCENES))
def test_assign_reasons_and_stack(lib, name):
    c, objects = shc.gate_scene(name)
    P, lab, used, counts = shr.used_pixels(c["depth"], c["labels"], c["K"], c["scale"], c["n_labels"], c["max_depth"])
    M = shr.moments(P, lab, used, c["n_labels"])
    for gate in (None, dict(slack=0.0, min_ratio=0.9, min_used=1)):
        rc, shapes, mom, reasons, stack, got = call(lib, c, objects=objects, gate=gate)
        assert rc == 0, lib[1].stocs_last_error()
        assert got == counts and mom.tolist() == M.tolist()
        check_shapes(shapes, P, lab, used, M, c["n_labels"])
        want = shr.gate(shapes, objects, **(gate or shr.GATE_DEFAULTS))
        assert reasons.tolist() == want.tolist()
        assert stack.tobytes() == shr.stack(c["labels"], c["n_labels"], want).tobytes()
    # under the defaults the device's shapes decide as the restatement's own do (test_segment_shapes_cases_cpu.py says what that is)
    rc, shapes, _, reasons, _, _ = call(lib, c, objects=objects)
    ref_shapes, _ = shr.shapes_from(P, lab, used, c["n_labels"])
    assert reasons.tolist() == shr.gate(ref_shapes, objects).tolist()


def test_assign_many_labels_many_objects_and_none(lib):
    capi, L = lib
    c, P, lab, used, counts, M = reference("overflow-129x33")
    rng = np.random.default_rng(7)
    objects = [(F(d), np.array([d * 0.8, d * 0.5, d * 0.3], F)) for d in rng.uniform(0.005, 0.6, capi.MAX_FRAME_OBJECTS)]
    rc, shapes, mom, reasons, stack, got = call(lib, c, objects=objects)
    assert rc == 0, L.stocs_last_error()
    assert got == counts and mom.tolist() == M.tolist()
    want = shr.gate(shapes, objects)
    assert reasons.tolist() == want.tolist() and len({tuple(r) for r in want.tolist()}) > 3
    assert stack.tobytes() == shr.stack(c["labels"], c["n_labels"], want).tobytes() and stack.any()
    # labels outside [0, n_labels] are 0 in the stack too
    c, P, lab, used, counts, M = reference("mixed-65x17")
    rc, shapes, _, reasons, stack, got = call(lib, c, objects=objects[:3], gate=dict(slack=1e6, min_ratio=0.0, min_used=1))
    assert rc == 0 and got == counts and reasons.tolist() == [[0, 4, 4]] * 3
    assert stack.tobytes() == shr.stack(c["labels"], 3, reasons).tobytes() and not stack[:, c["labels"] == 4].any() and not stack[:, c["labels"] == -1].any()
    # n_labels == 0: not an error, the stack comes back zero
    c, P, lab, used, counts, M = reference("no_labels")
    rc, shapes, _, reasons, stack, got = call(lib, c, objects=objects[:2])
    assert rc == 0 and got == counts and len(shapes) == 0 and stack.shape[0] == 2 and not stack.any()
    # n_objects == 0 through stocs_segment_assign is the shapes call: the same bytes
    c = reference("blobs17-65x17")[0]
    a = call(lib, c, entry="assign")
    b = call(lib, c, entry="shapes")
    assert a[0] == 0 and b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[5] == b[5]
    # the optional output: no moments asked for, nothing written there, the same records
    n = call(lib, c, want_moments=False, entry="shapes")
    assert n[0] == 0 and n[1].tobytes() == b[1].tobytes()


def test_points_shape_equals_the_frame_form(lib):
    from model_matching_amd import estimator
    for case_id in ("whole-129x33", "whole-63x15"):
        c, P, lab, used, counts, M = reference(case_id)
        rc, shapes, mom, _, _, _ = call(lib, c, entry="shapes")
        assert rc == 0
        pts = np.ascontiguousarray(P[used])                      # the frame's used points, in the frame's order
        s, m = estimator.points_shape(pts, moments=True)
        assert m.tolist() == M[0].tolist() and s.tobytes() == shapes[0].tobytes()
        s2, _ = estimator.points_shape(pts[::-1], moments=True)  # the sums and the extremes do not depend on the order
        assert s2.tobytes() == s.tobytes()
    # more than one tile of points, a point at 16 m and a NaN are skipped; the restatement on the same points
    rng = np.random.default_rng(11)
    pts = (rng.normal(0, 1, (2500, 3)) * np.array([0.3, 0.1, 0.02]) + np.array([0.1, -0.2, 1.0])).astype(F)
    pts[7] = (16.0, 0.0, 1.0); pts[1500] = (np.nan, 0.0, 1.0)
    s, m = estimator.points_shape(pts, moments=True)
    rs, rm = shr.points_shape(pts)
    assert m.tolist() == rm.tolist() and s["n_used"] == 2498 and s["centroid"].tobytes() == rs["centroid"].tobytes()
    Pp, lp, up = shr.points_used(pts)
    lo, hi, ext = shr.extents(Pp, lp, up, s["centroid"][None], s["axis"][None], 1)
    assert s["lo"].tobytes() == lo.tobytes() and s["hi"].tobytes() == hi.tobytes() and s["extent"].tobytes() == ext.tobytes()
    w, a64 = shr.eigh64(rm)
    assert all(shr.angle(s["axis"][k], a64[k]) <= MAX_ANGLE for k in range(3))
    e = estimator.points_shape(np.zeros((0, 3), F))
    assert e["flags"] == shr.EMPTY and e["n_used"] == 0 and not e["extent"].any()
    o = estimator.object_size(pts)
    assert o["extent"].tobytes() == s["extent"].tobytes() and o["diameter"] == F(np.sqrt(np.sum(s["extent"].astype(np.float64) ** 2)))
    assert estimator.object_size(pts, diameter=0.5)["diameter"] == F(0.5)


def test_wrappers_no_allocation_on_a_second_call_and_trim(lib):
    capi, L = lib
    from model_matching_amd import estimator
    c, objects = shc.gate_scene("sphere_and_big_box")
    obj = np.zeros(2, capi.OBJECT_DTYPE)
    for k, (d, e) in enumerate(objects):
        obj[k]["diameter"] = d; obj[k]["extent"] = e
    first = estimator.segment_assign(c["depth"], c["labels"], c["K"], c["scale"], obj)
    before = L.stocs_device_alloc_count()
    again = estimator.segment_assign(c["depth"], c["labels"], c["K"], c["scale"], obj)
    small = shc.frame("checker-63x15")
    estimator.segment_shapes(small["depth"], small["labels"], small["K"], small["scale"])
    estimator.points_shape(np.ones((100, 3), F))
    assert L.stocs_device_alloc_count() == before
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], again[:3])) and first[3] == again[3]
    assert first[1].tolist() == [[0, shr.TOO_LARGE], [shr.TOO_SMALL, 0]]
    assert first[2].shape == (2,) + c["depth"].shape and estimator.segment_gate(first[0], obj).tolist() == first[1].tolist()
    assert L.stocs_trim() == 0
    after = estimator.segment_assign(c["depth"], c["labels"], c["K"], c["scale"], obj)
    assert L.stocs_device_alloc_count() > before
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], after[:3]))
    shapes, counts, mom = estimator.segment_shapes(c["depth"], c["labels"], c["K"], c["scale"], moments=True)
    assert shapes.tobytes() == first[0].tobytes() and counts == first[3] and mom.shape == (2, 10)
