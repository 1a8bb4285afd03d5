"""stocs_segment_frame on the GPU against the numpy restatement of its contract (tests/segment_ref.py), under the default label form and both
forced ones: every count of the result, the winner, the ten moments, the three images and the records are equal bit for bit, steps 4-7
re-synchronised on the library's float plane.  The plane itself is judged against the float64 fit of the unquantised inliers, within the
bound segment_cases.plane_bound derives from the quantisation step and the inliers' spread, plus half a float32 ulp for the cast.  Frames hold
at most 129 x 96 pixels.  Every call goes through buffers with sentinel bytes behind them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import segment_cases as sc  # noqa: E402
import segment_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0xA5
PAD = 64
FORMS = [None, "1", "2"]
COUNTS = ("plane_found", "winner", "winner_count", "n_valid", "n_scored", "n_refit", "n_on_plane", "n_above", "n_below", "n_components", "n_segments")
REC_DTYPE = np.dtype([("root", np.int32), ("pixels", np.int32), ("c0", np.int32), ("r0", np.int32), ("c1", np.int32), ("r1", np.int32), ("zmin", np.float32),
                      ("zmax", np.float32)])


@pytest.fixture(scope="module")
def lib():
    from model_matching_amd import capi
    return capi, capi.load()


@pytest.fixture(params=FORMS, ids=["default", "form1", "form2"])
def form(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("STOCS_SEGMENT_FORM", raising=False)
    else:
        monkeypatch.setenv("STOCS_SEGMENT_FORM", request.param)
    return request.param


def padded(nbytes):
    return np.full(nbytes + PAD, SENTINEL, np.uint8)


def call(lib, depth, K, cap=None, want=("class_prob", "labels", "edge"), **kw):
    """the raw entry point on sentinel-padded buffers: (rc, result dict, records, images dict, raw buffers dict)"""
    capi, L = lib
    d = np.ascontiguousarray(depth, np.uint16)
    H, W = d.shape
    p = capi.SegmentParams()
    L.stocs_default_segment_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    cap = (W * H) // p.min_pixels if cap is None else cap
    raw = {"class_prob": padded(2 * W * H), "labels": padded(4 * W * H), "edge": padded(W * H), "records": padded(32 * cap), "out": padded(64)}
    ptr = lambda name, t: raw[name].ctypes.data_as(t) if name in want else None
    cam = capi.Camera(K[0], K[1], K[2], K[3], sc.SCALE, W, H, 0)
    rc = L.stocs_segment_frame(C.byref(cam), d.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(p), -1, ptr("class_prob", C.POINTER(C.c_uint16)), ptr("labels", capi._ip),
                               ptr("edge", capi._u8p), raw["records"].ctypes.data_as(C.POINTER(capi.SegmentRecord)) if cap > 0 else None, cap,
                               raw["out"].ctypes.data_as(C.POINTER(capi.SegmentResult)))
    for name, a in raw.items():
        assert (a[-PAD:] == SENTINEL).all(), "bytes behind %s were written" % name
        if name in ("class_prob", "labels", "edge") and name not in want:
            assert (a == SENTINEL).all(), name
    out = capi.SegmentResult.from_buffer_copy(raw["out"][:64].tobytes())
    res = {f: getattr(out, f) for f in COUNTS}
    res["plane"] = np.array(list(out.plane), F)
    n = max(0, min(res["n_segments"], cap)) if rc == 0 else 0
    records = np.frombuffer(raw["records"][:32 * n].tobytes(), REC_DTYPE)
    images = {"class_prob": raw["class_prob"][:2 * W * H].view(np.uint16).reshape(H, W), "labels": raw["labels"][:4 * W * H].view(np.int32).reshape(H, W),
              "edge": raw["edge"][:W * H].reshape(H, W)}
    return rc, res, records, {k: v for k, v in images.items() if k in want}, raw


_REF = {}


def reference(key, depth, K, plane, **kw):
    """the restatement, once per case and plane (the forms share it)"""
    k = (key, None if plane is None else plane.tobytes(), tuple(sorted(kw.items())))
    if k not in _REF:
        _REF[k] = sr.segment_frame(depth, K, sc.SCALE, plane=plane, **kw)
    return _REF[k]


def moments(lib):
    m = np.zeros(10, np.int64)
    assert lib[1].stocs_segment_last_moments(m.ctypes.data_as(lib[0]._i64p)) == 0
    return m.tolist()


def check(lib, key, depth, K, **kw):
    rc, res, records, images, _ = call(lib, depth, K, **kw)
    assert rc == 0, lib[1].stocs_last_error()
    ref = reference(key, depth, K, res["plane"] if res["plane_found"] else None, **kw)
    for f in COUNTS:
        assert res[f] == ref[f], (f, res[f], ref[f])
    assert moments(lib) == ref["moments"]
    if not res["plane_found"]:
        assert not res["plane"].any()
    for name in ("labels", "class_prob", "edge"):
        assert images[name].dtype == ref[name].dtype and np.array_equal(images[name], ref[name]), name
    want = np.array(ref["records"], REC_DTYPE) if ref["records"] else np.zeros(0, REC_DTYPE)
    assert records.tobytes() == want.tobytes()
    return res, ref


TABLES = {"clean": dict(seed=0), "noisy": dict(seed=1, noise_mm=1.5), "steep": dict(seed=2, tilt_deg=68.0, noise_mm=0.5, W=129, H=95),
          "shallow": dict(seed=3, tilt_deg=30.0, dist=0.8, W=127, H=96, wall_z=1.4)}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_a_table_frame_equals_the_restatement_and_its_plane_the_float64_fit(lib, form, name):
    depth, K, (n, d), masks = sc.table_frame(**TABLES[name])
    res, ref = check(lib, "table-" + name, depth, K, seed=7)
    assert res["plane_found"] == 1 and res["n_refit"] >= 3 and res["n_segments"] >= 2
    pts = ref["P"][ref["inl"]].astype(np.float64)
    n64, d64 = sr.fit64(pts)
    theta, bound_d, _ = sc.plane_bound(pts)
    cast_n, cast_d = np.sqrt(3.0) * 2.0 ** -25, max(float(np.spacing(F(d64))) / 2, 2.0 ** -25)     # half a float32 ulp per component
    en, ed = float(np.linalg.norm(res["plane"][:3].astype(np.float64) - n64)), abs(float(res["plane"][3]) - d64)
    print("[segment plane] %s form %s: |dn| %.3g bound %.3g ratio %.3g; |dd| %.3g bound %.3g ratio %.3g"      # the largest ratio seen: profiles/segment.md
          % (name, form, en, theta + cast_n, en / (theta + cast_n), ed, bound_d + cast_d, ed / (bound_d + cast_d)))
    assert en <= theta + cast_n and ed <= bound_d + cast_d
    assert res["plane"][3] > 0 and abs(float(np.linalg.norm(res["plane"][:3].astype(np.float64))) - 1.0) < 1e-6


@pytest.mark.parametrize("kw", [dict(score_stride=1), dict(score_stride=3, plane_hypotheses=65), dict(score_stride=7, plane_hypotheses=300, min_pixels=1),
                                dict(plane_min_share=1.0), dict(plane_hypotheses=1), dict(max_depth=1.2, jump_rel=0.0, jump_abs=0.002),
                                dict(plane_tolerance=0.002, max_height=0.1, min_pixels=50)], ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()))
def test_parameters_off_their_defaults(lib, form, kw):
    depth, K, _, _ = sc.table_frame(seed=4, noise_mm=1.0, W=128, H=96)
    res, _ = check(lib, "params", depth, K, seed=11, **kw)
    if kw.get("plane_min_share") == 1.0:
        assert res["plane_found"] == 0 and res["winner"] >= 0


@pytest.mark.parametrize("W,H", sc.SIZES)
@pytest.mark.parametrize("kind", ["blobs", "serpentine", "whole", "diagonal"])
def test_label_frames_across_every_kind_of_border(lib, form, kind, W, H):
    depth = {"blobs": lambda: sc.blobs(W, H, W + H), "serpentine": lambda: sc.serpentine(W, H), "whole": lambda: sc.blank(W, H, 1000),
             "diagonal": lambda: sc.diagonal_pair(W, H)}[kind]()
    res, _ = check(lib, "%s-%dx%d" % (kind, W, H), depth, sc.camera(W, H), **dict(sc.LABEL, min_pixels=3))
    assert res["plane_found"] == 0 and res["winner"] == -1
    if kind in ("serpentine", "whole"):
        assert res["n_components"] == 1 and res["n_segments"] == 1
    if kind == "diagonal":
        assert res["n_components"] == 2 and res["n_segments"] == 2
    if kind == "blobs":
        assert res["n_components"] >= res["n_segments"] >= 2 and res["n_components"] >= 10


def test_a_checkerboard_has_no_joins(lib, form):
    W, H = 65, 17
    depth = sc.checkerboard(W, H)
    res, _ = check(lib, "checker-2", depth, sc.camera(W, H), **dict(sc.LABEL, min_pixels=2))
    assert res["n_components"] == W * H and res["n_segments"] == 0
    res, _ = check(lib, "checker-1", depth, sc.camera(W, H), **dict(sc.LABEL, min_pixels=1))
    assert res["n_components"] == W * H and res["n_segments"] == W * H          # every pixel a segment: the cap is the frame


def test_a_jump_at_the_threshold_joins_and_one_float_above_it_does_not(lib, form):
    W, H = 65, 17
    depth, step = sc.jump_pair(W, H)
    at, _ = check(lib, "jump-at", depth, sc.camera(W, H), **dict(sc.LABEL, jump_abs=float(step), min_pixels=1))
    assert at["n_components"] == 1
    above, _ = check(lib, "jump-above", depth, sc.camera(W, H), **dict(sc.LABEL, jump_abs=float(np.nextafter(step, F(0))), min_pixels=1))
    assert above["n_components"] == 2
    rel = F(0.004)
    ja = F(step - F(rel * F(F(1000) * F(sc.SCALE))))
    r, _ = check(lib, "jump-rel", depth, sc.camera(W, H), **dict(sc.LABEL, jump_abs=float(ja), jump_rel=float(rel), min_pixels=1))
    assert r["n_components"] == 1


def test_min_pixels_keeps_exactly_and_drops_one_below(lib, form):
    W, H = 65, 17
    depth = sc.two_sizes(W, H, 150)
    res, ref = check(lib, "two-sizes", depth, sc.camera(W, H), **dict(sc.LABEL, min_pixels=150))
    assert res["n_components"] == 2 and res["n_segments"] == 1 and ref["records"][0][1] == 150
    res, _ = check(lib, "two-sizes-149", depth, sc.camera(W, H), **dict(sc.LABEL, min_pixels=149))
    assert res["n_segments"] == 2


def test_capacity_one_below_writes_nothing(lib, form):
    capi, L = lib
    W, H = 128, 33
    depth = sc.blobs(W, H, 9)
    kw = dict(sc.LABEL, min_pixels=3)
    rc, res, _, _, _ = call(lib, depth, sc.camera(W, H), **kw)
    assert rc == 0 and res["n_segments"] >= 3
    rc2, res2, _, _, raw = call(lib, depth, sc.camera(W, H), cap=res["n_segments"] - 1, **kw)
    assert rc2 == capi.ERR_CAPACITY and b"segments" in L.stocs_last_error()
    assert all(res2[f] == res[f] for f in COUNTS) and np.array_equal(res2["plane"], res["plane"])                                             # `out` is filled
    for name in ("class_prob", "labels", "edge", "records"):
        assert (raw[name] == SENTINEL).all(), name
    rc3, res3, rec3, _, _ = call(lib, depth, sc.camera(W, H), cap=res["n_segments"], **kw)                                                      # exactly enough
    assert rc3 == 0 and rec3.size == res["n_segments"]
    rc4, res4, _, _, _ = call(lib, sc.blank(W, H), sc.camera(W, H), cap=0, **kw)                                                                # no records asked, none there
    assert rc4 == 0 and res4["n_segments"] == 0


def test_a_frame_with_no_valid_pixel(lib, form):
    W, H = 65, 17
    for depth in (sc.blank(W, H), sc.blank(W, H, 3000)):                                      # nothing measured; everything beyond max_depth
        rc, res, records, images, _ = call(lib, depth, sc.camera(W, H))
        assert rc == 0 and all(res[f] == (-1 if f == "winner" else 0) for f in COUNTS) and not res["plane"].any() and records.size == 0
        assert not images["labels"].any() and not images["class_prob"].any() and not images["edge"].any()
        assert moments(lib) == [0] * 10


def test_no_plane_search_and_all_hypotheses_dead(lib, form):
    depth, K, _, _ = sc.table_frame(seed=6)
    res, _ = check(lib, "no-search", depth, K, plane_hypotheses=0, min_pixels=20)
    assert res["plane_found"] == 0 and res["winner"] == -1 and res["n_on_plane"] == 0
    W, H = 65, 17
    two = sc.blank(W, H)
    two[3, 4] = two[3, 5] = 1000                                                             # two valid pixels: no three distinct valid draws
    res, ref = check(lib, "all-dead", two, sc.camera(W, H), min_pixels=2, score_stride=1)
    assert res["plane_found"] == 0 and res["winner"] == -1 and max(ref["counts"]) == 0 and res["n_segments"] == 1


def test_a_winner_decided_by_the_tie_rule(lib, form):
    W, H = 128, 32
    depth = sc.two_planes(W, H)
    K = sc.camera(W, H)
    res, ref = check(lib, "tie", depth, K, plane_hypotheses=64, plane_tolerance=0.005, seed=3, min_pixels=10)
    best = max(ref["counts"])
    tied = [h for h, c in enumerate(ref["counts"]) if c == best]
    sides = {bool(sr.draws(3, h, W * H)[0] % W >= W // 2) for h in tied}
    assert len(tied) >= 2 and sides == {False, True}                                         # both planes reach the same count
    assert res["winner"] == tied[0] and res["winner_count"] == best == ref["n_scored"] // 2


def test_each_optional_output_may_be_null(lib, form):
    depth, K, _, _ = sc.table_frame(seed=0)
    _, full_res, full_rec, full, _ = call(lib, depth, K)
    for want in (("labels", "edge"), ("class_prob", "edge"), ("class_prob", "labels"), ()):
        rc, res, rec, images, _ = call(lib, depth, K, want=want)
        assert rc == 0 and rec.tobytes() == full_rec.tobytes() and all(res[f] == full_res[f] for f in COUNTS)
        for name in want:
            assert np.array_equal(images[name], full[name])


def test_a_second_call_allocates_nothing_and_trim_gives_the_memory_back(lib, form):
    capi, L = lib
    depth, K, _, _ = sc.table_frame(seed=1)
    call(lib, depth, K)
    before = L.stocs_device_alloc_count()
    a = call(lib, depth, K)
    b = call(lib, sc.blobs(128, 96, 1), K, **dict(sc.LABEL, min_pixels=200))
    assert L.stocs_device_alloc_count() == before
    assert L.stocs_trim() == 0
    c = call(lib, depth, K)
    assert L.stocs_device_alloc_count() > before                                             # it had to allocate again
    assert c[1]["n_segments"] == a[1]["n_segments"] and np.array_equal(c[3]["labels"], a[3]["labels"]) and b[0] == 0


def test_the_clock_reports_both_kernel_groups(lib, form, monkeypatch):
    capi, L = lib
    depth, K, _, _ = sc.table_frame(seed=2)
    s, l = C.c_float(-1), C.c_float(-1)
    monkeypatch.delenv("STOCS_SEGMENT_CLOCK", raising=False)
    call(lib, depth, K)
    assert L.stocs_segment_last_device_ms(C.byref(s), C.byref(l)) == capi.ERR_STATE
    monkeypatch.setenv("STOCS_SEGMENT_CLOCK", "1")
    rc, res, _, _, _ = call(lib, depth, K)
    assert rc == 0 and L.stocs_segment_last_device_ms(C.byref(s), C.byref(l)) == 0 and 0 < s.value < 1000 and 0 < l.value < 1000


def test_the_estimator_wrapper(lib, form):
    from model_matching_amd import estimator
    depth, K, _, masks = sc.table_frame(seed=0)
    res, records, images = estimator.segment_frame(depth, K, sc.SCALE, seed=7)
    ref = reference("table-clean", depth, K, res["plane"], seed=7)
    assert res["n_segments"] == ref["n_segments"] == len(records) and np.array_equal(images["labels"], ref["labels"]) and np.array_equal(images["edge"], ref["edge"])
    assert records["pixels"].tolist() == [r[1] for r in ref["records"]] and estimator.segment_last_moments().tolist() == ref["moments"]
    stack = estimator.segment_class_images(images["labels"])
    assert stack.shape == (res["n_segments"],) + depth.shape and np.array_equal(stack.max(axis=0), images["class_prob"])
    only = estimator.segment_frame(depth, K, sc.SCALE, images=("labels",), seed=7)[2]
    assert list(only) == ["labels"]
