"""stocs_refine_poses_visible / stocs_refine_visible_detail on the GPU against the numpy restatement of their contract
(tests/refine_visible_ref.py).  Keys, states, counts and everything that is decided by a float comparison are compared for equality; the
29 sums within (count + 8) 2^-53 sum |products|; a pose after one iteration within 4 float ulps + cond(A^T A) 2^-50 of a longdouble solve of
the restatement's rows (oracle/refine_oracle.py's pose_tolerance, the bound of tests/test_refine_edges_gpu.py); k iterations step by step,
re-synchronised on the library's own pose; the end of the convergence cases within max(2 e_ref, depth_scale).  Frames are at most
128 x 96.  Every call of the batch entry point goes through buffers with sentinel bytes behind them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_cases as mc  # noqa: E402
import mesh_ref  # noqa: E402
import refine_visible_cases as rc  # noqa: E402
import refine_visible_ref as ref  # noqa: E402
import vsd_cases as vc  # noqa: E402
from oracle import refine_oracle as ro  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0x5A
CONVERGE = rc.convergence_cases()
STATES = rc.state_cases()
W0, H0 = 128, 96


def _est():
    from model_matching_amd.estimator import StocsEstimator
    rng = np.random.default_rng(1)
    sp = rng.normal(0, 0.05, (32, 3)).astype(F)
    sn = sp / np.linalg.norm(sp, axis=1, keepdims=True)
    return StocsEstimator(sp, sn, np.ones(32, F), None, sp[:8], sn[:8], build_index=False)


class Ctx:
    """one context with the case's mesh and frame; the raw C entry point on padded host buffers"""
    def __init__(self, case, est=None):
        from model_matching_amd import capi
        self.capi, self.L = capi, capi.load()
        self.est = est or _est()
        self.set(case)

    def set(self, case):
        self.case = case
        self.est.set_mesh(case.verts, case.tris)
        self.est.set_frame(case.depth, case.prob, case.K, case.depth_scale)

    def params(self, **kw):
        p = self.capi.RefineVisibleParams()
        self.L.stocs_default_refine_visible_params(C.byref(p))
        for k, v in dict(self.case.prm, **kw).items():
            setattr(p, k, v)
        return p

    def refine(self, poses, **kw):
        P, pP = self.capi.f32(poses)
        n = P.size // 16
        out = np.empty(n * 16 + 8, F); out.view(np.uint8)[:] = SENTINEL
        rec = np.empty((n + 1) * 40, np.uint8); rec[:] = SENTINEL
        p = self.params(**kw)
        self.capi.check(self.L.stocs_refine_poses_visible(self.est.h, pP, n, C.byref(p), out.ctypes.data_as(self.capi._fp),
                                                          rec.ctypes.data_as(C.POINTER(self.capi.RefineVisibleResult))))
        assert np.all(out[n * 16:].view(np.uint8) == SENTINEL) and np.all(rec[n * 40:] == SENTINEL), "bytes behind an output were written"
        from model_matching_amd.estimator import _REFINE_VISIBLE_DTYPE
        return out[: n * 16].reshape(n, 16).copy(), rec[: n * 40].view(_REFINE_VISIBLE_DTYPE).copy()

    def detail(self, pose, **kw):
        P, pP = self.capi.f32(pose)
        npix = self.case.W * self.case.H
        keys = np.empty(npix + 4, np.uint64); st = np.empty(npix + 16, np.uint8); sums = np.empty(29 + 4, np.float64)
        for a in (keys, st, sums):
            a.view(np.uint8)[:] = SENTINEL
        p = self.params(**kw)
        self.capi.check(self.L.stocs_refine_visible_detail(self.est.h, pP, C.byref(p), keys.ctypes.data_as(C.POINTER(C.c_uint64)), st.ctypes.data_as(self.capi._u8p),
                                                           sums.ctypes.data_as(C.POINTER(C.c_double))))
        assert np.all(keys[npix:].view(np.uint8) == SENTINEL) and np.all(st[npix:] == SENTINEL) and np.all(sums[29:].view(np.uint8) == SENTINEL)
        return keys[:npix].copy(), st[:npix].copy(), sums[:29].copy()

    def ref_eval(self, pose, **kw):
        return ref.evaluate(pose, *self.case.args(), **dict(self.case.prm, **kw))

    def close(self):
        self.est.close()


def _check_evaluation(cx, pose, **kw):
    """keys, state and counts equal; sums within the bound; the record of a zero-iteration call is the detail call's; one iteration within
    the pose bound of the longdouble solve"""
    keys, st, sums = cx.detail(pose, **kw)
    ev = cx.ref_eval(pose, **kw)
    assert np.array_equal(keys, ev["keys"]), "keys differ at %d pixels" % int((keys != ev["keys"]).sum())
    assert np.array_equal(st, ev["state"]), "states differ at %d pixels" % int((st != ev["state"]).sum())
    assert sums[27] == ev["sums"][27] == int((st == ref.COUNTED).sum())
    err, bound = np.abs(sums - ev["sums"]), ref.sums_bound(ev)
    print("SUMS %s n=%d max err/bound %.3g" % (cx.case.name, int(sums[27]), float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    P0, r0 = cx.refine(np.asarray(pose, F)[None], max_iterations=0, **kw)
    want = ref.record_of(ev)
    assert np.array_equal(P0[0].view(np.uint32), np.asarray(pose, F).view(np.uint32))
    assert all(int(r0[k][0]) == want[k] for k in ref.RECORD_FIELDS if k != "rms"), (r0, want)
    assert abs(float(r0["rms"][0]) - float(want["rms"])) <= 4 * np.spacing(F(want["rms"])) + 1e-12
    _check_one_step(cx, pose, ev, **kw)
    return ev


def _check_one_step(cx, pose, ev, **kw):
    P1, r1 = cx.refine(np.asarray(pose, F)[None], max_iterations=1, **kw)
    T34, cond = ref.update_longdouble(pose, ev)
    if T34 is None:
        assert r1["frozen"][0] == 1 and r1["iterations"][0] == 0 and np.array_equal(P1[0].view(np.uint32), np.asarray(pose, F).view(np.uint32))
        return P1[0]
    tol = ro.pose_tolerance(T34.astype(np.float64), cond)
    dev = np.abs(np.asarray(P1[0], F).reshape(4, 4).T.astype(np.float64)[:3, :] - T34.astype(np.float64))
    print("POSE %s cond %.3g max dev %.3g max dev/tol %.3g" % (cx.case.name, cond, dev.max(), (dev / tol).max()))
    assert r1["iterations"][0] == 1 and r1["frozen"][0] == 0 and (dev <= tol).all(), ((dev / tol).max(), cond)
    assert np.array_equal(P1[0][[3, 7, 11, 15]].view(np.uint32), np.asarray(pose, F)[[3, 7, 11, 15]].view(np.uint32))
    return P1[0]


# ---------------------------------------------------------------- the rasteriser's tiers and forms
def _small_triangle_case(px_w, px_h, n=24):
    v, t = mc.grid_of_small_triangles(n, px_w, px_h, mc.K_EXACT, W0, z=1.0)
    depth = rc.frame_of(mc.IDENTITY, v, t, mc.K_EXACT, W0, H0, depth_scale=rc.POW2_SCALE)
    start = vc.pose16(vc.translation(0.0004, -0.0003, 0.002))
    return rc.Case("lane_%dx%d" % (px_w, px_h), v, t, mc.K_EXACT, W0, H0, depth, None, mc.IDENTITY, start, depth_scale=rc.POW2_SCALE, max_distance=0.02)


def _box_case():
    v, t = mc.box(0.2, 0.15, 0.1)           # faces of a thousand pixels: above the lane tier, below the workgroup tier
    K = vc.small_camera(W0, H0)
    G = rc.pose_at((1.0, 1.0, 0.3), 32.0, (0.01, -0.01, 0.85))      # three faces in view: the system is well conditioned
    depth = rc.frame_of(vc.pose16(G), v, t, K, W0, H0)
    return rc.Case("wave_box", v, t, K, W0, H0, depth, None, vc.pose16(G), vc.pose16(rc.perturbed(G, (1, 0.2, 0.1), 1.0, (0.002, 0.001, -0.003))), max_distance=0.02)


def _full_frame_triangle_case():
    """one triangle whose box is the whole 128 x 96 frame (12 288 pixels, above the workgroup tier's 8192), tilted so that it constrains a pose"""
    v, t = mc.triangle((-1.3, -1.1, 0.25), (2.4, -0.9, -0.2), (-0.9, 2.3, 0.1))
    K = vc.small_camera(W0, H0)
    G = rc.pose_at((0.3, 1.0, 0.0), 12.0, (0.0, 0.0, 1.6))
    depth = rc.frame_of(vc.pose16(G), v, t, K, W0, H0)
    return rc.Case("group_triangle", v, t, K, W0, H0, depth, None, vc.pose16(G), vc.pose16(rc.perturbed(G, (0, 1, 0.3), 0.5, (0.001, 0.0, 0.004))), max_distance=0.05)


def _tier_cases():
    from model_matching_amd import capi
    small = capi.load().stocs_mesh_small_px()
    assert small == 120
    return [_small_triangle_case(10, 12), _small_triangle_case(11, 11), _box_case(), _full_frame_triangle_case()]


@pytest.mark.parametrize("which", range(4), ids=["lane_at_small_px", "lane_above_small_px", "wavefront_box", "workgroup_triangle"])
def test_keys_state_sums_and_one_iteration_in_every_tier(which):
    case = _tier_cases()[which]
    cx = Ctx(case)
    ev = _check_evaluation(cx, case.start16)
    assert ev["sums"][27] > 50
    if which == 3:
        assert (ev["keys"] != ref.EMPTY_KEY).sum() > 8192
    cx.close()


@pytest.mark.parametrize("form", [1, 2, 16])
def test_every_kernel_form_gives_the_same_keys(form, monkeypatch):
    cx = Ctx(_box_case())
    cases = [_box_case(), _small_triangle_case(10, 12), _full_frame_triangle_case()]
    for case in cases:
        cx.set(case)
        monkeypatch.delenv("STOCS_MESH_FORM", raising=False)
        k0, s0, sums0 = cx.detail(case.start16)
        monkeypatch.setenv("STOCS_MESH_FORM", str(form))
        k1, s1, sums1 = cx.detail(case.start16)
        ev = cx.ref_eval(case.start16)
        assert np.array_equal(k1, ev["keys"]) and np.array_equal(s1, ev["state"])
        assert np.array_equal(k0, k1) and np.array_equal(sums0.view(np.uint64), sums1.view(np.uint64))
    cx.close()


def test_duplicated_triangle_and_reversed_winding():
    case = STATES["counted"]
    cx = Ctx(case)
    k0, s0, sums0 = cx.detail(case.start16)
    t0 = (k0 & np.uint64(0xFFFFFFFF)).astype(np.int64)
    which = int(np.bincount(t0[k0 != ref.EMPTY_KEY]).argmax())
    for front in (True, False):
        v, t = rc.duplicated(case.verts, case.tris, which, front)
        dup = rc.Case("dup", v, t, case.K, case.W, case.H, case.depth, None, case.G16, case.start16)
        cx.set(dup)
        k, s, sums = cx.detail(case.start16)
        ev = cx.ref_eval(case.start16)
        assert np.array_equal(k, ev["keys"]) and np.array_equal(s, ev["state"])
        won = (t0 == which) & (k0 != ref.EMPTY_KEY)
        assert np.all((k[won] & np.uint64(0xFFFFFFFF)).astype(np.int64) == (0 if front else which))
        assert np.array_equal(sums.view(np.uint64), sums0.view(np.uint64))   # the same facets under other names, pixel by pixel
    rev = rc.Case("reversed", case.verts, case.tris[:, [0, 2, 1]], case.K, case.W, case.H, case.depth, None, case.G16, case.start16)
    cx.set(rev)
    k, s, sums = cx.detail(case.start16)
    ev = cx.ref_eval(case.start16)
    assert np.array_equal(k, ev["keys"]) and np.array_equal(s, ev["state"])
    assert np.array_equal(k, k0) and np.array_equal(s, s0)                   # the mesh contract: winding changes no depth bit
    assert (np.abs(sums - sums0) <= ref.sums_bound(ev)).all()                # the normal faces the camera either way
    cx.close()


@pytest.mark.parametrize("name", ["counted", "no_depth", "off_class", "too_far", "grazing"])
def test_state_classes(name):
    cx = Ctx(STATES[name])
    ev = _check_evaluation(cx, STATES[name].start16)
    assert ref.record_of(ev)[name] > 20
    cx.close()


# ---------------------------------------------------------------- iterations
@pytest.mark.parametrize("case", CONVERGE, ids=repr)
def test_iterations_step_by_step_and_convergence(case):
    cx = Ctx(case)
    K_IT = 4
    lib = [cx.refine(case.start16[None], max_iterations=k)[0][0] for k in range(K_IT + 1)]
    assert np.array_equal(lib[0].view(np.uint32), case.start16.view(np.uint32))
    for k in range(K_IT):       # re-synchronised: the library's pose after k iterations, one step of the restatement, the library's after k + 1
        ev = cx.ref_eval(lib[k])
        T34, cond = ref.update_longdouble(lib[k], ev)
        tol = ro.pose_tolerance(T34.astype(np.float64), cond)
        dev = np.abs(lib[k + 1].reshape(4, 4).T.astype(np.float64)[:3, :] - T34.astype(np.float64))
        print("STEP %s k=%d cond %.3g max dev/tol %.3g" % (case.name, k, cond, (dev / tol).max()))
        assert (dev <= tol).all(), (k, (dev / tol).max())
    P, rec = cx.refine(case.start16[None])
    Pr, rr, _ = ref.refine(case.start16, *case.args(), **case.prm)
    e0, e_ref, e_gpu = (ref.vertex_error(x, case.G16, case.verts) for x in (case.start16, Pr, P[0]))
    print("CONVERGENCE %s e0 %.4g e_ref %.4g e_gpu %.4g" % (case.name, e0, e_ref, e_gpu))
    assert e_ref <= 0.1 * e0
    assert e_gpu <= max(2 * e_ref, case.depth_scale)
    assert rec["iterations"][0] == case.prm["max_iterations"] and rec["frozen"][0] == 0
    cx.close()


# ---------------------------------------------------------------- edges
def _rect_case(px_w, px_h):
    """one triangle whose clamped box, the pose's rectangle, is px_w x px_h pixels"""
    v, t = mc.grid_of_small_triangles(1, px_w, px_h, mc.K_EXACT, W0, z=1.0)
    depth = rc.frame_of(mc.IDENTITY, v, t, mc.K_EXACT, W0, H0, depth_scale=rc.POW2_SCALE)
    depth[depth > 0] += 3                  # the surface three raw units behind the model: residuals that are not zero
    return rc.Case("rect_%dx%d" % (px_w, px_h), v, t, mc.K_EXACT, W0, H0, depth, None, mc.IDENTITY, mc.IDENTITY, depth_scale=rc.POW2_SCALE, max_distance=0.02)


def test_rectangle_widths_and_row_counts_around_the_split():
    from model_matching_amd import capi
    G = capi.load().stocs_refine_visible_groups(W0, H0)
    assert G == 6
    cx = Ctx(_rect_case(63, G - 1))
    for w, h in [(63, G - 1), (64, G), (65, G + 1), (6, 5), (65, 4 * G + 3), (120, 90)]:
        case = _rect_case(w, h)
        cx.set(case)
        ev = _check_evaluation(cx, case.start16)
        assert ev["sums"][27] > 0
    cx.close()


def test_rectangles_at_the_image_borders():
    """the full-frame triangle touches all four borders; a triangle that projects just outside the right (bottom) border leaves a
    rectangle of one column (row) in which no pixel is hit"""
    case = _full_frame_triangle_case()
    cx = Ctx(case)
    ev = _check_evaluation(cx, case.start16)
    present = (ev["keys"] != ref.EMPTY_KEY).reshape(H0, W0)
    assert present[0].any() and present[-1].any() and present[:, 0].any() and present[:, -1].any()
    for dx, dy in [(W0 + 0.3, 10.0), (10.0, H0 + 0.3)]:
        pts = [((c - 0.0) / 64.0, (r - 0.0) / 64.0, 1.0) for c, r in ((dx, dy), (dx + 0.4, dy), (dx, dy + 0.4))]
        v, t = mc.triangle(*pts)
        depth = np.full((H0, W0), 8192, np.uint16)
        edge = rc.Case("width_one", v, t, mc.K_EXACT, W0, H0, depth, None, mc.IDENTITY, mc.IDENTITY, depth_scale=rc.POW2_SCALE)
        cx.set(edge)
        keys, st, sums = cx.detail(edge.start16)
        ev = cx.ref_eval(edge.start16)
        assert np.array_equal(keys, ev["keys"]) and not st.any() and not sums.any()
        P, rec = cx.refine(edge.start16[None])
        assert rec["present"][0] == 0 and rec["frozen"][0] == 1 and np.array_equal(P[0].view(np.uint32), edge.start16.view(np.uint32))
    cx.close()


def _plane_case(raw, **prm):
    """a fronto-parallel triangle at z = 1 that covers the optical axis, under K_EXACT and the identity pose: the rendered z is exactly 1
    on every pixel; the frame holds `raw` everywhere, a power-of-two depth unit"""
    v, t = mc.triangle((-0.1, -0.1, 1.0), (1.0, -0.1, 1.0), (-0.1, 1.0, 1.0))
    depth = np.full((48, 64), raw, np.uint16)
    return rc.Case("plane", v, t, mc.K_EXACT, 64, 48, depth, None, mc.IDENTITY, mc.IDENTITY, depth_scale=rc.POW2_SCALE, **prm)


def test_distance_exactly_at_the_threshold_is_counted():
    md = 2.0 ** -5                                  # raw = 8192 + 256: d = 1 + 2^-5, on the axis D = 2^-10 = max_distance^2 exactly
    cx = Ctx(_plane_case(8192 + 256, max_distance=md))
    keys, st, sums = cx.detail(mc.IDENTITY)
    assert (keys[0] >> np.uint64(32)) == np.uint64(F(1.0).view(np.uint32))
    assert st[0] == ref.COUNTED and np.all(st[1:][keys[1:] != ref.EMPTY_KEY] == ref.TOO_FAR) and sums[27] == 1
    assert np.array_equal(st, cx.ref_eval(mc.IDENTITY)["state"])
    below = float(np.nextafter(F(md), F(0)))        # the threshold one float lower: D is the next float above it
    keys, st, sums = cx.detail(mc.IDENTITY, max_distance=below)
    assert st[0] == ref.TOO_FAR and sums[27] == 0
    cx.set(_plane_case(8192 + 257, max_distance=md))   # the frame one raw unit farther
    keys, st, sums = cx.detail(mc.IDENTITY)
    assert st[0] == ref.TOO_FAR and sums[27] == 0
    cx.close()


def test_class_image_present_absent_and_at_the_threshold():
    case = STATES["counted"]
    prob = np.full((case.H, case.W), 1000, np.uint16)       # cp = (float)(1000 * 1e-4) is the float 0.1f: not below the threshold 0.1f
    prob[:, : case.W // 2] = 999
    with_prob = rc.Case("class_threshold", case.verts, case.tris, case.K, case.W, case.H, case.depth, prob, case.G16, case.start16, class_threshold=0.1)
    cx = Ctx(with_prob)
    ev = _check_evaluation(cx, case.start16)
    st = ev["state"].reshape(case.H, case.W)
    lib_st = cx.detail(case.start16)[1].reshape(case.H, case.W)
    left, right = lib_st[:, : case.W // 2], lib_st[:, case.W // 2:]
    assert not np.any(right == ref.OFF_CLASS) and np.any(right == ref.COUNTED)
    assert np.any(left == ref.OFF_CLASS) and not np.any(left == ref.COUNTED) and np.array_equal(lib_st, st)
    cx.set(case)                                            # no class image: the threshold is not read
    k, s, sums = cx.detail(case.start16, class_threshold=5.0)
    assert not np.any(s == ref.OFF_CLASS) and np.array_equal(s, cx.ref_eval(case.start16)["state"])
    cx.close()


def test_view_cosine_at_the_threshold():
    """a facet with m = (-1/4, 0, -3/16) exactly, seen on the optical axis: cos = 0.6.  The float threshold at which s s < c c (mm pp) turns is
    found in float32 from the rendered z; at it the pixel is counted, one float above it is grazing"""
    v, t = mc.triangle((-3 / 64, -0.5, 1.0625), (-3 / 64, 0.5, 1.0625), (9 / 64, -0.5, 0.8125))
    depth = np.full((48, 64), 8192, np.uint16)
    case = rc.Case("view_cos", v, t, mc.K_EXACT, 64, 48, depth, None, mc.IDENTITY, mc.IDENTITY, depth_scale=rc.POW2_SCALE, max_distance=0.25)
    cx = Ctx(case)
    keys, st, sums = cx.detail(mc.IDENTITY)
    assert keys[0] != ref.EMPTY_KEY and st[0] == ref.COUNTED
    z = np.uint32(keys[0] >> np.uint64(32)).view(F)
    m = [F(-0.25), F(0), F(-3 / 16)]
    s = m[0] * F(0) + (m[1] * F(0) + m[2] * z)
    mm = m[0] * m[0] + (m[1] * m[1] + m[2] * m[2])
    pp = F(0) * F(0) + (F(0) * F(0) + z * z)
    lhs = s * s
    c = F(0.5999)
    while not lhs < (F(np.nextafter(c, F(1))) * F(np.nextafter(c, F(1)))) * (mm * pp):
        c = F(np.nextafter(c, F(1)))
    assert 0.599 < c < 0.601
    up = float(np.nextafter(c, F(1)))
    for cos, want in ((float(c), ref.COUNTED), (up, ref.GRAZING)):
        keys, st, sums = cx.detail(mc.IDENTITY, min_view_cos=cos)
        assert st[0] == want and np.array_equal(st, cx.ref_eval(mc.IDENTITY, min_view_cos=cos)["state"]), (cos, st[0])
    cx.close()


def test_degenerate_facet_is_grazing():
    case = rc.degenerate_case()
    cx = Ctx(case)
    keys, st, sums = cx.detail(case.start16)
    ev = cx.ref_eval(case.start16)
    assert np.array_equal(keys, ev["keys"]) and np.array_equal(st, ev["state"])
    assert (keys[0] & np.uint64(0xFFFFFFFF)) == 1 and st[0] == ref.GRAZING and sums[27] == ev["sums"][27] > 100
    cx.close()


def test_five_counted_pixels_freeze_and_six_update():
    case = STATES["counted"]
    ev = ref.evaluate(case.start16, *case.args())
    counted = np.flatnonzero(ev["state"] == ref.COUNTED)
    pick = counted[np.linspace(0, len(counted) - 1, 6).astype(int)]
    cx = Ctx(case)
    for n_px in (5, 6):
        d = np.zeros(case.W * case.H, np.uint16)
        d[pick[:n_px]] = case.depth.reshape(-1)[pick[:n_px]]
        few = rc.Case("few_%d" % n_px, case.verts, case.tris, case.K, case.W, case.H, d.reshape(case.H, case.W), None, case.G16, case.start16)
        cx.set(few)
        keys, st, sums = cx.detail(case.start16)
        assert sums[27] == n_px and np.array_equal(st, cx.ref_eval(case.start16)["state"])
        P, rec = cx.refine(case.start16[None], max_iterations=3)
        if n_px == 5:
            assert rec["frozen"][0] == 1 and rec["iterations"][0] == 0 and rec["counted"][0] == 5
            assert np.array_equal(P[0].view(np.uint32), case.start16.view(np.uint32))
        else:
            assert rec["iterations"][0] >= 1 and not np.array_equal(P[0], case.start16)
            _check_one_step(cx, case.start16, cx.ref_eval(case.start16))
    cx.close()


def test_one_fronto_parallel_plane_is_singular_and_freezes():
    cx = Ctx(_plane_case(8192 + 64, max_distance=0.25))
    keys, st, sums = cx.detail(mc.IDENTITY)
    assert sums[27] > 500 and np.all(st[keys != ref.EMPTY_KEY] == ref.COUNTED)
    assert not sums[[2, 3, 4]].any()                        # the columns of gamma, t_x and t_y are exactly zero
    P, rec = cx.refine(mc.IDENTITY[None], max_iterations=4)
    assert rec["frozen"][0] == 1 and rec["iterations"][0] == 0 and rec["counted"][0] == sums[27]
    assert np.array_equal(P[0].view(np.uint32), mc.IDENTITY.view(np.uint32))
    cx.close()


def test_invalid_poses_inside_a_batch():
    case = CONVERGE[1]
    cx = Ctx(case)
    behind = case.start16.copy(); behind[14] = F(-0.8)
    nan = case.start16.copy(); nan[5] = F(np.nan)
    inf = case.start16.copy(); inf[12] = F(np.inf)
    zero = np.zeros(16, F)
    batch = np.stack([case.start16, behind, nan, case.start16, zero, inf, case.start16])
    P, rec = cx.refine(batch, max_iterations=3)
    alone_P, alone_rec = cx.refine(case.start16[None], max_iterations=3)
    for i in (0, 3, 6):
        assert np.array_equal(P[i].view(np.uint32), alone_P[0].view(np.uint32)) and rec[i] == alone_rec[0] and rec["iterations"][i] == 3
    for i in (2, 4, 5):         # renders nothing, comes back bit for bit with a zero record
        assert np.array_equal(P[i].view(np.uint32), batch[i].view(np.uint32)) and rec[i].tobytes() == bytes(40)
    assert np.array_equal(P[1].view(np.uint32), behind.view(np.uint32))       # a valid pose that shows nothing: no pixel, frozen
    assert rec["present"][1] == 0 and rec["frozen"][1] == 1 and rec["iterations"][1] == 0
    cx.close()


# ---------------------------------------------------------------- determinism
def _seven(case):
    rng = np.random.default_rng(11)
    G = np.asarray(case.G16, F).reshape(4, 4).T.astype(np.float64)
    return np.stack([vc.pose16(rc.perturbed(G, rng.normal(size=3), rng.uniform(0.5, 2.0), rng.normal(0, 0.002, 3))) for _ in range(7)])


def test_batch_position_and_order_change_no_bit():
    case = CONVERGE[0]
    cx = Ctx(case)
    poses = _seven(case)
    P, rec = cx.refine(poses, max_iterations=4)
    assert len(set(P[i].tobytes() for i in range(7))) == 7
    for i in range(7):
        Pi, ri = cx.refine(poses[i][None], max_iterations=4)
        assert np.array_equal(Pi[0].view(np.uint32), P[i].view(np.uint32)) and ri[0].tobytes() == rec[i].tobytes(), i
    Pr, rr = cx.refine(poses[::-1].copy(), max_iterations=4)
    assert np.array_equal(Pr[::-1].view(np.uint32), P.view(np.uint32)) and rr[::-1].tobytes() == rec.tobytes()
    cx.close()


def test_chunks_change_no_bit(monkeypatch):
    case = CONVERGE[1]
    cx = Ctx(case)
    poses = _seven(case)[:5]
    monkeypatch.delenv("STOCS_REFINE_VISIBLE_CHUNK", raising=False)
    P, rec = cx.refine(poses, max_iterations=3)
    for chunk in (1, 2, 3):
        monkeypatch.setenv("STOCS_REFINE_VISIBLE_CHUNK", str(chunk))
        Pc, rc_ = cx.refine(poses, max_iterations=3)
        assert np.array_equal(Pc.view(np.uint32), P.view(np.uint32)) and rc_.tobytes() == rec.tobytes(), chunk
    cx.close()


# ---------------------------------------------------------------- housekeeping
def test_second_call_allocates_nothing_and_other_entry_points_keep_their_bits():
    case = CONVERGE[0]
    cx = Ctx(case)
    poses = _seven(case)
    depth0 = cx.est.render_depth_mesh(poses[:3])
    exp0 = cx.est.explain_poses_mesh(poses[:3], labels=True, tolerance=0.02)
    P, rec = cx.refine(poses)
    cx.detail(poses[0])
    before = cx.L.stocs_device_alloc_count()
    P2, rec2 = cx.refine(poses)
    P3, rec3 = cx.refine(poses[:4])
    cx.detail(poses[1])
    assert cx.L.stocs_device_alloc_count() == before
    assert np.array_equal(P2.view(np.uint32), P.view(np.uint32)) and rec2.tobytes() == rec.tobytes() and np.array_equal(P3.view(np.uint32), P[:4].view(np.uint32))
    depth1 = cx.est.render_depth_mesh(poses[:3])
    exp1 = cx.est.explain_poses_mesh(poses[:3], labels=True, tolerance=0.02)
    assert np.array_equal(depth0.view(np.uint32), depth1.view(np.uint32))
    assert exp0[0].tobytes() == exp1[0].tobytes() and np.array_equal(exp0[1], exp1[1]) and np.array_equal(exp0[2], exp1[2])
    cx.close()


def test_errors_come_in_the_documented_order():
    from model_matching_amd import capi
    L = capi.load()
    INVALID, STATE = -1, capi.ERR_STATE if hasattr(capi, "ERR_STATE") else None
    est = _est()
    case = STATES["counted"]
    P, pP = capi.f32(case.start16)
    out = (C.c_float * 16)(); rec = (capi.RefineVisibleResult * 1)(); sums = (C.c_double * 29)()
    p = capi.RefineVisibleParams(); L.stocs_default_refine_visible_params(C.byref(p))
    bad = capi.RefineVisibleParams(); L.stocs_default_refine_visible_params(C.byref(bad)); bad.max_distance = 0.0
    call = lambda ctx, poses, n, prm, o, r: L.stocs_refine_poses_visible(ctx, poses, n, prm, o, r)
    # 1. NULL ctx, n < 0
    assert call(None, pP, 1, C.byref(p), out, rec) == INVALID and b"NULL context" in L.stocs_last_error()
    assert call(est.h, pP, -1, C.byref(bad), out, rec) == INVALID and b"n -1" in L.stocs_last_error()
    # 2. n == 0: a no-op, whatever else is wrong
    assert call(est.h, None, 0, None, None, None) == 0
    # 3. NULL pointers, parameters: before the mesh and the frame are looked at (the context has neither)
    assert call(est.h, None, 1, C.byref(p), out, rec) == INVALID and b"NULL" in L.stocs_last_error()
    assert call(est.h, pP, 1, None, out, rec) == INVALID and call(est.h, pP, 1, C.byref(p), None, rec) == INVALID and call(est.h, pP, 1, C.byref(p), out, None) == INVALID
    assert call(est.h, pP, 1, C.byref(bad), out, rec) == INVALID and b"max_distance" in L.stocs_last_error()
    # 4. no mesh
    rc_mesh = call(est.h, pP, 1, C.byref(p), out, rec)
    assert rc_mesh not in (0, INVALID) and b"no mesh" in L.stocs_last_error()
    est.set_frame(case.depth, None, case.K, case.depth_scale)
    assert call(est.h, pP, 1, C.byref(p), out, rec) == rc_mesh and b"no mesh" in L.stocs_last_error()      # the mesh comes before the frame
    # 5. no frame
    est2 = _est()
    est2.set_mesh(case.verts, case.tris)
    assert call(est2.h, pP, 1, C.byref(p), out, rec) == rc_mesh and b"no frame" in L.stocs_last_error()   # the same code: STOCS_ERR_STATE
    assert L.stocs_refine_visible_detail(est2.h, pP, C.byref(p), None, None, sums) == rc_mesh and b"no frame" in L.stocs_last_error()
    assert L.stocs_refine_visible_detail(est2.h, pP, C.byref(bad), None, None, sums) == INVALID
    assert L.stocs_refine_visible_detail(est2.h, pP, C.byref(p), None, None, None) == INVALID
    if STATE is not None:
        assert rc_mesh == STATE
    est.close(); est2.close()
