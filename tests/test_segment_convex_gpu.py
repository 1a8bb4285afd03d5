"""stocs_segment_frame_convex on the GPU against the numpy restatement (tests/segment_convex_ref.py), under both bend forms and both label
forms: the cut image, the smoothed depth, labels, class image, edge image, records and every count are equal bit for bit, steps 4-7
re-synchronised on the library's float plane as test_segment_gpu.py does.  Frames hold at most 160 x 120 pixels.  Every call goes through
buffers with sentinel bytes behind them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import segment_cases as sc  # noqa: E402
import segment_convex_cases as cc  # noqa: E402
import segment_convex_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0xA5
PAD = 64
COUNTS = ("plane_found", "winner", "winner_count", "n_valid", "n_scored", "n_refit", "n_on_plane", "n_above", "n_below", "n_components", "n_segments")
IMAGES = {"class_prob": 2, "labels": 4, "edge": 1, "cut": 1, "smoothed": 4}
DTYPES = {"class_prob": np.uint16, "labels": np.int32, "edge": np.uint8, "cut": np.uint8, "smoothed": np.float32}
REC_DTYPE = np.dtype([("root", np.int32), ("pixels", np.int32), ("c0", np.int32), ("r0", np.int32), ("c1", np.int32), ("r1", np.int32), ("zmin", np.float32),
                      ("zmax", np.float32)])


@pytest.fixture(scope="module")
def lib():
    from model_matching_amd import capi
    return capi, capi.load()


@pytest.fixture(params=[("1", "1"), ("1", "2"), ("2", "1"), ("2", "2"), (None, None)], ids=["bend1-label1", "bend1-label2", "bend2-label1", "bend2-label2", "defaults"])
def forms(request, monkeypatch):
    for name, v in zip(("STOCS_SEGMENT_BEND_FORM", "STOCS_SEGMENT_FORM"), request.param):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    return request.param


def padded(nbytes):
    return np.full(nbytes + PAD, SENTINEL, np.uint8)


def call(lib, depth, K, convex, cap=None, want=tuple(IMAGES), **kw):
    """the raw entry point on sentinel-padded buffers (convex None: stocs_segment_frame): (rc, result dict, records, images dict, raw buffers)"""
    capi, L = lib
    d = np.ascontiguousarray(depth, np.uint16)
    H, W = d.shape
    p = capi.SegmentParams()
    L.stocs_default_segment_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    cap = (W * H) // p.min_pixels if cap is None else cap
    raw = {name: padded(size * W * H) for name, size in IMAGES.items()}
    raw.update(records=padded(32 * cap), out=padded(64), cout=padded(32))
    ptr = lambda name, t: raw[name].ctypes.data_as(t) if name in want else None
    cam = capi.Camera(K[0], K[1], K[2], K[3], sc.SCALE, W, H, 0)
    rec = raw["records"].ctypes.data_as(C.POINTER(capi.SegmentRecord)) if cap > 0 else None
    u16 = C.POINTER(C.c_uint16)
    if convex is None:
        want = tuple(w for w in want if w in ("class_prob", "labels", "edge"))
        rc = L.stocs_segment_frame(C.byref(cam), d.ctypes.data_as(u16), C.byref(p), -1, ptr("class_prob", u16), ptr("labels", capi._ip), ptr("edge", capi._u8p), rec, cap,
                                   raw["out"].ctypes.data_as(C.POINTER(capi.SegmentResult)))
    else:
        cp = capi.SegmentConvexParams()
        L.stocs_default_segment_convex_params(C.byref(cp))
        for k, v in convex.items():
            setattr(cp, k, v)
        rc = L.stocs_segment_frame_convex(C.byref(cam), d.ctypes.data_as(u16), C.byref(p), C.byref(cp), -1, ptr("class_prob", u16), ptr("labels", capi._ip),
                                          ptr("edge", capi._u8p), ptr("cut", capi._u8p), ptr("smoothed", capi._fp), rec, cap,
                                          raw["out"].ctypes.data_as(C.POINTER(capi.SegmentResult)), raw["cout"].ctypes.data_as(C.POINTER(capi.SegmentConvexResult)))
    for name, a in raw.items():
        assert (a[-PAD:] == SENTINEL).all(), "bytes behind %s were written" % name
        if name in IMAGES and name not in want:
            assert (a == SENTINEL).all(), name
    out = capi.SegmentResult.from_buffer_copy(raw["out"][:64].tobytes())
    res = {f: getattr(out, f) for f in COUNTS}
    res["plane"] = np.array(list(out.plane), F)
    if convex is not None:
        co = capi.SegmentConvexResult.from_buffer_copy(raw["cout"][:32].tobytes())
        res.update({f: getattr(co, f) for f in cr.COUNTS})
        assert list(co.reserved) == [0, 0, 0]
    n = max(0, min(res["n_segments"], cap)) if rc == 0 else 0
    records = np.frombuffer(raw["records"][:32 * n].tobytes(), REC_DTYPE)
    images = {name: raw[name][:size * W * H].view(DTYPES[name]).reshape(H, W) for name, size in IMAGES.items() if name in want}
    return rc, res, records, images, raw


_REF = {}


def reference(key, depth, K, plane, convex, **kw):
    """the restatement, once per case, plane and parameters (the forms share it)"""
    k = (key, None if plane is None else plane.tobytes(), tuple(sorted(convex.items())), tuple(sorted(kw.items())))
    if k not in _REF:
        _REF[k] = cr.segment_frame_convex(depth, K, sc.SCALE, plane=plane, convex=convex, **kw)
    return _REF[k]


def check(lib, key, depth, K, convex, **kw):
    rc, res, records, images, _ = call(lib, depth, K, convex, **kw)
    assert rc == 0, lib[1].stocs_last_error()
    ref = reference(key, depth, K, res["plane"] if res["plane_found"] else None, convex, **kw)
    for f in COUNTS + cr.COUNTS:
        assert res[f] == ref[f], (key, f, res[f], ref[f])
    for name in IMAGES:
        assert images[name].dtype == ref[name].dtype, name
        assert images[name].tobytes() == ref[name].tobytes(), (key, name, int((images[name].view(np.uint8) != ref[name].view(np.uint8)).sum()))      # NaNs too
    want = np.array(ref["records"], REC_DTYPE) if ref["records"] else np.zeros(0, REC_DTYPE)
    assert records.tobytes() == want.tobytes(), key
    return res, ref


@pytest.mark.parametrize("W,H", cc.SIZES)
def test_label_frames_equal_the_restatement(lib, forms, W, H):
    frames = cc.label_frames(W, H)
    assert len(frames) >= 8
    cuts = 0
    for name, (depth, cv) in sorted(frames.items()):
        res, ref = check(lib, "%s-%dx%d" % (name, W, H), depth, sc.camera(W, H), cv, **cc.LABEL)
        assert res["plane_found"] == 0
        cuts += res["n_cut"]
        if name.startswith("valley-col") or name.startswith("valley-row"):
            assert res["n_cut"] > 0 and res["n_components"] == 2, name
        if name.startswith("ridge"):
            assert res["n_cut"] == 0 and res["n_tested_h"] > 0, name
    assert cuts > 0


@pytest.mark.parametrize("noise", cc.NOISES)
@pytest.mark.parametrize("name", sorted(cc.SCENES))
def test_scenes_equal_the_restatement_and_touching_objects_come_apart(lib, forms, name, noise):
    depth, K, obj = cc.scene(name, noise)
    res, ref = check(lib, "scene-%s-%g" % (name, noise), depth, K, dict(cr.CONVEX_DEFAULTS), **cc.SCENE_PARAMS)
    rc, plain, _, _, _ = call(lib, depth, K, None, **cc.SCENE_PARAMS)
    assert rc == 0 and res["plane_found"] == 1 and plain["n_segments"] == 1
    assert res["n_segments"] == (1 if name.startswith("lone") else 2)


@pytest.mark.parametrize("cv", [dict(bend_radius=1, smooth_radius=4), dict(bend_radius=8, smooth_radius=0), dict(bend_radius=8, smooth_radius=4, bend_cos=0.5),
                                dict(bend_radius=3, smooth_radius=1, bend_cos=1.0), dict(bend_radius=5, smooth_radius=3, bend_cos=0.0)],
                         ids=lambda cv: "-".join("%s=%s" % kv for kv in cv.items()))
def test_parameters_off_their_defaults_on_a_noisy_table(lib, forms, cv):
    depth, K, _, _ = sc.table_frame(seed=4, noise_mm=1.0, W=129, H=96)
    check(lib, "table", depth, K, dict(cr.CONVEX_DEFAULTS, **cv), seed=11, min_pixels=50, jump_rel=0.02)


def test_radius_zero_equals_the_plain_entry_point_byte_for_byte(lib, forms):
    depth, K, _ = cc.scene("two_spheres", 1.0)
    rc0, plain, rec0, img0, raw0 = call(lib, depth, K, None, **cc.SCENE_PARAMS)
    rc1, res, rec1, img1, raw1 = call(lib, depth, K, dict(bend_radius=0), **cc.SCENE_PARAMS)
    assert rc0 == 0 and rc1 == 0
    for name in ("class_prob", "labels", "edge", "records", "out"):
        assert raw0[name].tobytes() == raw1[name].tobytes(), name
    assert not img1["cut"].any() and all(res[f] == 0 for f in cr.COUNTS)
    ref = reference("zero", depth, K, res["plane"], dict(cr.CONVEX_DEFAULTS, bend_radius=0), **cc.SCENE_PARAMS)
    assert img1["smoothed"].tobytes() == ref["smoothed"].tobytes()


def test_cut_and_smoothed_may_be_null(lib, forms):
    depth, K, _ = cc.scene("box_behind_box", 2.0)
    cv = dict(cr.CONVEX_DEFAULTS)
    _, full_res, full_rec, full, _ = call(lib, depth, K, cv, **cc.SCENE_PARAMS)
    for want in (("class_prob", "labels", "edge", "cut"), ("class_prob", "labels", "edge", "smoothed"), ("labels",), ()):
        rc, res, rec, images, _ = call(lib, depth, K, cv, want=want, **cc.SCENE_PARAMS)
        assert rc == 0 and rec.tobytes() == full_rec.tobytes() and all(res[f] == full_res[f] for f in COUNTS + cr.COUNTS)
        for name in want:
            assert images[name].tobytes() == full[name].tobytes(), name


def test_capacity_one_below_writes_nothing(lib, forms):
    capi, L = lib
    W, H = 129, 33
    depth, cv = cc.label_frames(W, H)["blobs-r4s2"]
    rc, res, _, _, _ = call(lib, depth, sc.camera(W, H), cv, **cc.LABEL)
    assert rc == 0 and res["n_segments"] >= 3
    rc2, res2, _, _, raw = call(lib, depth, sc.camera(W, H), cv, cap=res["n_segments"] - 1, **cc.LABEL)
    assert rc2 == capi.ERR_CAPACITY and b"segments" in L.stocs_last_error()
    assert all(res2[f] == res[f] for f in COUNTS + cr.COUNTS)                                # `out` and `cout` are filled
    for name in tuple(IMAGES) + ("records",):
        assert (raw[name] == SENTINEL).all(), name
    rc3, _, rec3, _, _ = call(lib, depth, sc.camera(W, H), cv, cap=res["n_segments"], **cc.LABEL)
    assert rc3 == 0 and rec3.size == res["n_segments"]


def test_a_second_call_allocates_nothing(lib, forms):
    capi, L = lib
    depth, K, _ = cc.scene("two_spheres", 0.0)
    cv = dict(cr.CONVEX_DEFAULTS)
    a = call(lib, depth, K, cv, **cc.SCENE_PARAMS)
    before = L.stocs_device_alloc_count()
    b = call(lib, depth, K, cv, **cc.SCENE_PARAMS)
    c = call(lib, depth, K, None, **cc.SCENE_PARAMS)
    d = call(lib, cc.scene("lone_box", 2.0)[0], K, dict(bend_radius=8, smooth_radius=4), want=("labels",), **cc.SCENE_PARAMS)
    assert L.stocs_device_alloc_count() == before
    assert a[0] == b[0] == c[0] == d[0] == 0 and a[3]["labels"].tobytes() == b[3]["labels"].tobytes() and a[3]["cut"].tobytes() == b[3]["cut"].tobytes()


def test_the_clock_reports_the_bend_step(lib, forms, monkeypatch):
    capi, L = lib
    depth, K, _ = cc.scene("two_spheres", 0.0)
    s, l, b = C.c_float(-1), C.c_float(-1), C.c_float(-1)
    monkeypatch.delenv("STOCS_SEGMENT_CLOCK", raising=False)
    call(lib, depth, K, dict(cr.CONVEX_DEFAULTS), **cc.SCENE_PARAMS)
    assert L.stocs_segment_last_bend_ms(C.byref(b)) == capi.ERR_STATE
    monkeypatch.setenv("STOCS_SEGMENT_CLOCK", "1")
    assert call(lib, depth, K, dict(cr.CONVEX_DEFAULTS), **cc.SCENE_PARAMS)[0] == 0
    assert L.stocs_segment_last_bend_ms(C.byref(b)) == 0 and 0 < b.value < 1000
    assert L.stocs_segment_last_device_ms(C.byref(s), C.byref(l)) == 0 and 0 < s.value < 1000 and 0 < l.value < 1000
    assert L.stocs_segment_last_bend_ms(None) == 0
    assert call(lib, depth, K, None, **cc.SCENE_PARAMS)[0] == 0                              # a plain call has no bend step to time
    assert L.stocs_segment_last_bend_ms(C.byref(b)) == capi.ERR_STATE and L.stocs_segment_last_device_ms(C.byref(s), C.byref(l)) == 0


def test_the_estimator_wrapper(lib, forms):
    from model_matching_amd import estimator
    depth, K, obj = cc.scene("box_behind_box", 1.0)
    plain = estimator.segment_frame(depth, K, sc.SCALE, **cc.SCENE_PARAMS)
    none = estimator.segment_frame(depth, K, sc.SCALE, convex=None, **cc.SCENE_PARAMS)
    rc, raw_res, raw_rec, raw_img, _ = call(lib, depth, K, None, **cc.SCENE_PARAMS)
    assert rc == 0 and sorted(plain[0]) == sorted(none[0]) == sorted(COUNTS + ("plane",)) and sorted(none[2]) == ["class_prob", "edge", "labels"]
    for a in (plain, none):                                                                  # convex=None: the call and what it returns are the plain ones
        assert all(a[0][f] == raw_res[f] for f in COUNTS) and a[1].tobytes() == raw_rec.tobytes() and all(np.array_equal(a[2][k], raw_img[k]) for k in a[2])
    res, records, images = estimator.segment_frame(depth, K, sc.SCALE, convex=True, images=("labels", "cut", "smoothed"), **cc.SCENE_PARAMS)
    ref = reference("scene-box_behind_box-1", depth, K, res["plane"], dict(cr.CONVEX_DEFAULTS), **cc.SCENE_PARAMS)
    assert sorted(images) == ["cut", "labels", "smoothed"] and all(res[f] == ref[f] for f in COUNTS + cr.COUNTS)
    assert images["cut"].tobytes() == ref["cut"].tobytes() and images["smoothed"].tobytes() == ref["smoothed"].tobytes() and np.array_equal(images["labels"], ref["labels"])
    assert res["n_segments"] == 2 == len(records) and all(share == 1.0 for _, _, _, share in cc.purity(images["labels"], obj))
    res2, _, images2 = estimator.segment_frame(depth, K, sc.SCALE, convex=dict(bend_radius=8, smooth_radius=4, bend_cos=0.8), **cc.SCENE_PARAMS)
    assert sorted(images2) == ["class_prob", "edge", "labels"] and res2["n_tested_h"] > 0
    with pytest.raises(TypeError):
        estimator.segment_frame(depth, K, sc.SCALE, convex=dict(no_such_field=1))
    with pytest.raises(capi_error(lib)):
        estimator.segment_frame(depth, K, sc.SCALE, convex=dict(bend_radius=9))


def capi_error(lib):
    return lib[0].StocsError
