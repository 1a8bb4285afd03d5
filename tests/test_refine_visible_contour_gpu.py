"""stocs_refine_poses_visible_contour / stocs_refine_visible_contour_detail on the GPU against the numpy restatement of their contract
(tests/refine_visible_contour_ref.py).  Contour states and nearest-silhouette indices are compared for equality; the 29 contour sums
within (3 pulled + 8) 2^-53 sum |products| of a longdouble sum; every trace row against the longdouble restatement stepped from the
library's own state, as tests/test_refine_visible_damped_gpu.py does it: the evaluated pose within 4 float ulps + cond(M'') 2^-50, the cost
within the rounding bound of its sums over the divisor, the decision equal wherever the costs differ by more than their bounds (no
comparison of these cases falls inside), lambda equal as a double, counts bit for bit.  Frames hold at most 128 x 96 pixels; the two cases
whose grown rectangle is 128 and 129 columns wide live on a 144 x 80 frame (fewer pixels, wide enough).  Every call of the batch entry
point goes through buffers with sentinel bytes behind them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import refine_visible_cases as rc  # noqa: E402
import refine_visible_contour_cases as cc  # noqa: E402
import refine_visible_contour_ref as cref  # noqa: E402
import refine_visible_damped_ref as dref  # noqa: E402
import refine_visible_ref as ref  # noqa: E402
from oracle import refine_oracle as ro  # noqa: E402
from test_refine_visible_damped_gpu import BASE_FIELDS, DCtx  # noqa: E402
from test_refine_visible_gpu import SENTINEL, _est, _seven  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
DETAIL = cc.detail_cases()
CONTOUR_KEYS = tuple(cref.CONTOUR_DEFAULTS)


def _damped_only(prm):
    return dict((k, v) for k, v in prm.items() if k not in CONTOUR_KEYS)


class CCtx(DCtx):
    """the damped form's test context with the raw contour entry points on padded host buffers"""
    def dparams(self, **kw):
        return DCtx.dparams(self, **_damped_only(dict(kw)))

    def set(self, case):
        DCtx.set(self, case)
        self._damped_case_prm = _damped_only(case.prm)

    def cparams(self, **kw):
        p = self.capi.RefineVisibleContourParams()
        self.L.stocs_default_refine_visible_contour_params(C.byref(p))
        for k, v in dict(self.case.prm, **kw).items():
            if k == "pivot_model":
                p.damped.pivot_model[:] = [float(x) for x in v]
            elif k in dict(self.capi.RefineVisibleParams._fields_):
                setattr(p.damped.base, k, v)
            elif k in CONTOUR_KEYS:
                setattr(p, k, v)
            else:
                setattr(p.damped, k, v)
        return p

    def damped(self, poses, trace=True, **kw):
        keep, self.case.prm = self.case.prm, self._damped_case_prm
        try:
            return DCtx.damped(self, poses, trace=trace, **_damped_only(kw))
        finally:
            self.case.prm = keep

    def contour(self, poses, trace=True, **kw):
        from model_matching_amd.estimator import _REFINE_VISIBLE_CONTOUR_DTYPE, _REFINE_VISIBLE_TRACE_DTYPE
        P, pP = self.capi.f32(poses)
        n = P.size // 16
        p = self.cparams(**kw)
        rows = p.damped.base.max_iterations + 1
        out = np.empty(n * 16 + 8, F); out.view(np.uint8)[:] = SENTINEL
        rec = np.empty((n + 1) * 80, np.uint8); rec[:] = SENTINEL
        tr = np.empty((n * rows + 1) * 88, np.uint8); tr[:] = SENTINEL
        self.capi.check(self.L.stocs_refine_poses_visible_contour(self.est.h, pP, n, C.byref(p), out.ctypes.data_as(self.capi._fp),
                                                                  rec.ctypes.data_as(C.POINTER(self.capi.RefineVisibleContourResult)),
                                                                  tr.ctypes.data_as(C.POINTER(self.capi.RefineVisibleTrace)) if trace else None))
        assert np.all(out[n * 16:].view(np.uint8) == SENTINEL) and np.all(rec[n * 80:] == SENTINEL), "bytes behind an output were written"
        assert np.all(tr[n * rows * 88 if trace else 0:] == SENTINEL), "bytes behind the trace were written"
        return out[: n * 16].reshape(n, 16).copy(), rec[: n * 80].view(_REFINE_VISIBLE_CONTOUR_DTYPE).copy(), \
            (tr[: n * rows * 88].view(_REFINE_VISIBLE_TRACE_DTYPE).copy().reshape(n, rows) if trace else None)

    def cdetail(self, pose, **kw):
        P, pP = self.capi.f32(pose)
        npix = self.case.W * self.case.H
        st = np.empty(npix + 16, np.uint8); near = np.empty(npix + 4, np.int32); sums = np.empty(29 + 4, np.float64)
        for a in (st, near, sums):
            a.view(np.uint8)[:] = SENTINEL
        p = self.cparams(**kw)
        self.capi.check(self.L.stocs_refine_visible_contour_detail(self.est.h, pP, C.byref(p), st.ctypes.data_as(self.capi._u8p), near.ctypes.data_as(self.capi._ip),
                                                                   sums.ctypes.data_as(C.POINTER(C.c_double))))
        assert np.all(st[npix:] == SENTINEL) and np.all(near[npix:].view(np.uint8) == SENTINEL) and np.all(sums[29:].view(np.uint8) == SENTINEL)
        return st[:npix].copy(), near[:npix].copy(), sums[:29].copy()

    def ref_pass(self, pose, **kw):
        """the restatement's evaluation and contour pass of one pose under the case's parameters"""
        K, base, d, con = cref.split(dict(self.case.prm, **kw))
        ev, cp = cref.evaluate(pose, *self.case.args(), base, dict(con, w=con["w"] or 1.0))
        return ev, cp


def _check_detail(cx, pose, **kw):
    st, near, sums = cx.cdetail(pose, **kw)
    ev, cp = cx.ref_pass(pose, **kw)
    assert np.array_equal(st, cp["state"]), "states differ at %d pixels" % int((st != cp["state"]).sum())
    assert np.array_equal(near.astype(np.int64), cp["nearest"]), "nearest indices differ at %d pixels" % int((near != cp["nearest"]).sum())
    L = np.longdouble
    want, _ = cref.sums_of(cp["A"].astype(L), cp["b"].astype(L), cp["pulled"], dtype=L)
    err, bound = np.abs(sums.astype(L) - want).astype(np.float64), cref.sums_bound(cp)
    print("CONTOUR SUMS %s unreached %d beyond %d pulled %d max err/bound %.3g" % (cx.case.name, cp["unreached"], cp["beyond"], cp["pulled"],
                                                                                  float((err / np.maximum(bound, 1e-300)).max())))
    assert sums[27] == cp["pulled"] and (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    return ev, cp


@pytest.mark.parametrize("name", sorted(DETAIL))
def test_states_and_nearest_pixels_are_the_restatements(name):
    case = DETAIL[name]
    cx = CCtx(case)
    ev, cp = _check_detail(cx, case.start16)
    assert cp["pulled"] > 0 and cp["unreached"] > 0 or name.startswith("solid_R64")
    # the record of a K = 0 call carries the same counts
    P, rec, _ = cx.contour(case.start16[None], trace=False, max_iterations=0)
    r = cref.tally(ev, cp, cp["object_px"])
    assert np.array_equal(P[0].view(np.uint32), case.start16.view(np.uint32))
    assert all(int(rec[k][0]) == r[k] for k in ("object_px", "uncovered", "unreached", "beyond", "pulled") + tuple(BASE_FIELDS)), (rec, r)
    assert abs(float(rec["pull_rms"][0]) - float(r["pull_rms"])) <= 4 * np.spacing(F(r["pull_rms"])) + 1e-12
    cx.close()


@pytest.mark.parametrize("R", [1, 3, 8, 40, 64])
def test_other_radii_on_the_tie_and_corner_cases(R):
    cx = CCtx(cc.tie_case(R))
    _, cp = _check_detail(cx, cx.case.start16)
    W = cx.case.W
    if R >= 3:
        assert cp["nearest"][20 * W + 33] == 20 * W + 30 and cp["nearest"][43 * W + 50] == 40 * W + 50 and cp["nearest"][32 * W + 82] == 30 * W + 80
    cx.set(cc.corner_case(R))
    _check_detail(cx, cx.case.start16)
    cx.close()


def test_the_gate_at_equality_is_not_beyond():
    case = cc.tie_case()
    cx = CCtx(case)
    u = 20 * case.W + 27                                   # three columns left of the seed (20, 30) on the plane z = 1: e = (3 / 64, 0, 0) exactly
    at = 3.0 / 64.0
    below = float(np.nextafter(F(at), F(0)))
    _, cp = _check_detail(cx, case.start16, pull_distance=at)
    assert cp["nearest"][u] == 20 * case.W + 30 and cp["state"][u] == cref.PULLED          # D == pull_distance^2
    _, cp = _check_detail(cx, case.start16, pull_distance=below)
    assert cp["state"][u] == cref.BEYOND                                                     # D one float step of the distance above
    cx.close()


@pytest.mark.parametrize("form", [1, 2, 16])
def test_every_mesh_form_gives_the_same_contour(form, monkeypatch):
    case = cc.solid_case(16)
    cx = CCtx(case)
    monkeypatch.delenv("STOCS_MESH_FORM", raising=False)
    s0, n0, sums0 = cx.cdetail(case.start16)
    monkeypatch.setenv("STOCS_MESH_FORM", str(form))
    s1, n1, sums1 = cx.cdetail(case.start16)
    assert np.array_equal(s0, s1) and np.array_equal(n0, n1) and np.array_equal(sums0.view(np.uint64), sums1.view(np.uint64))
    _check_detail(cx, case.start16)
    cx.close()


def _follow(cx, start, P, rec, trace, **kw):
    """one pose: the library's trace against the restatement, stepped from the library's own state -> the number of comparisons made"""
    prm = dict(cx.case.prm, **kw)
    K, base, d, con = cref.split(prm)
    w = con["w"]
    args = cx.case.args()
    start = np.asarray(start, F)
    if not ref.pose_valid(start):
        assert np.array_equal(P.view(np.uint32), start.view(np.uint32)) and rec.tobytes() == bytes(80) and trace.tobytes() == bytes(88 * (K + 1))
        return 0
    n_object = int(cref.object_mask(cx.case.depth, cx.case.prob, base["class_threshold"]).sum())
    L = np.longdouble

    def measured(pose):
        ev, cp = cref.evaluate(pose, *args, base, con)
        r = cref.tally(ev, cp, n_object)
        C_ = cref.cost_of(ev["sums"][28], cp["sums"][28] if cp is not None else 0.0, r, base["max_distance"], con["pull_distance"], w)
        return dict(ev=ev, cp=cp, r=r, C=C_, bound=cref.cost_bound(ev, cp, r, w))

    def totals_long(m):
        Sc = cref.sums_of(m["cp"]["A"].astype(L), m["cp"]["b"].astype(L), m["cp"]["pulled"], dtype=L)[0] if m["cp"] is not None else None
        return cref.totals(dref.sums_longdouble(m["ev"]), Sc, w, dtype=L)

    Pa = ma = lam = Ca_lib = None
    n_acc = n_rej = n_eval = frozen = compared = 0
    for e in range(K + 1):
        row = trace[e]
        if frozen:
            assert row.tobytes() == bytes(88), e
            continue
        assert row["state"] & 1, e
        Pt = row["pose"].copy()
        m = measured(Pt)
        if np.isinf(m["C"]):
            assert row["cost"] == np.inf, e
        else:
            assert abs(row["cost"] - m["C"]) <= m["bound"], (e, row["cost"], m["C"], m["bound"])
        n_eval += 1
        if e == 0:
            assert np.array_equal(Pt.view(np.uint32), start.view(np.uint32)) and row["accepted"] == 1 and row["lambda"] == d["lambda0"]
            ok = True
        else:
            nt = dref.next_trial(Pa, totals_long(ma), lam, d, dtype=L)
            T34 = nt["T34"].astype(np.float64)
            tol = ro.pose_tolerance(T34, nt["cond"])
            dev = np.abs(Pt.reshape(4, 4).T.astype(np.float64)[:3, :] - T34)
            print("TRIAL %s e=%d cond %.3g s %.3g max dev/tol %.3g cost %.6g pulled %d" % (cx.case.name, e, nt["cond"], nt["s"], (dev / tol).max(), row["cost"], m["r"]["pulled"]))
            assert (dev <= tol).all(), (e, (dev / tol).max(), nt["cond"])
            assert np.array_equal(Pt[[3, 7, 11, 15]].view(np.uint32), start[[3, 7, 11, 15]].view(np.uint32))
            decided = np.isinf(m["C"]) or abs(m["C"] - ma["C"]) > m["bound"] + ma["bound"]
            assert decided, "a decision of case %s falls inside the rounding bound at e = %d: the cap is zero" % (cx.case.name, e)
            compared += 1
            ok = bool(row["accepted"])
            assert ok == (m["C"] < ma["C"]), (e, m["C"], ma["C"])
            assert ok == (row["cost"] < Ca_lib)
            assert row["lambda"] == dref.decide(m["C"], ma["C"], lam, d)[1], (e, row["lambda"], lam)
        lam = float(row["lambda"])
        if ok:
            Pa, ma, Ca_lib = Pt, m, float(row["cost"])
            n_acc += e > 0
        else:
            n_rej += 1
        if e < K:
            few = ma["r"]["counted"] + 3 * ma["r"]["pulled"] < 6
            froze = (e == 0 and few) or dref.next_trial(Pa, cref.totals(ma["ev"]["sums"], ma["cp"]["sums"] if ma["cp"] is not None else None, w), lam, d)["T34"] is None
            assert bool(row["state"] & 2) == froze, e
            frozen = 1 if froze else 0
        else:
            assert row["state"] == 1
    want = ma["r"]
    assert np.array_equal(P.view(np.uint32), Pa.view(np.uint32))
    assert all(int(rec[k]) == want[k] for k in BASE_FIELDS + ["object_px", "uncovered", "unreached", "beyond", "pulled"]), (rec, want)
    assert abs(float(rec["rms"]) - float(want["rms"])) <= 4 * np.spacing(F(want["rms"])) + 1e-12
    assert abs(float(rec["pull_rms"]) - float(want["pull_rms"])) <= 4 * np.spacing(F(want["pull_rms"])) + 1e-12
    assert (int(rec["iterations"]), int(rec["rejected"]), int(rec["evaluations"]), int(rec["frozen"])) == (n_acc, n_rej, n_eval, frozen)
    with np.errstate(over="ignore"):
        assert rec["cost"] == F(Ca_lib) and rec["lambda"] == F(lam) and rec["reserved"] == 0
    return compared


def _check_call(cx, poses, **kw):
    """a call with the trace, followed pose by pose; the same call without the trace gives the same bits"""
    poses = np.asarray(poses, F).reshape(-1, 16)
    P, rec, tr = cx.contour(poses, **kw)
    compared = sum(_follow(cx, poses[h], P[h], rec[h], tr[h], **kw) for h in range(len(poses)))
    P2, rec2, none = cx.contour(poses, trace=False, **kw)
    assert none is None and np.array_equal(P2.view(np.uint32), P.view(np.uint32)) and rec2.tobytes() == rec.tobytes()
    return P, rec, tr, compared


@pytest.mark.parametrize("weight", [0.25, 1.0, 4.0])
def test_one_pose_follows_the_restatement(weight):
    case = cc.small_solid_case(contour_weight=weight)
    cx = CCtx(case)
    P, rec, tr, compared = _check_call(cx, case.start16[None])
    assert compared == case.prm["max_iterations"] and rec["evaluations"][0] == compared + 1
    assert cx.contour(case.start16[None], trace=False, max_iterations=0)[1]["pulled"][0] > 0          # the start is pulled
    cx.close()


def test_the_capture_case_ends_where_the_restatement_ends():
    case = cc.capture_case()
    cx = CCtx(case)
    Pd, rd, _ = cx.damped(case.start16[None], trace=False)
    assert rd["frozen"][0] == 1 and rd["counted"][0] == 0 and np.array_equal(Pd[0].view(np.uint32), case.start16.view(np.uint32))
    P, rec, tr, compared = _check_call(cx, case.start16[None])
    want = cref.refine(case.start16, *case.args(), **case.prm)
    e0, e_gpu, e_ref = (ref.vertex_error(p, case.G16, case.verts) for p in (case.start16, P[0], want["pose"]))
    print("CAPTURE e0 %.5f e_gpu %.5f e_ref %.5f accepted %d rejected %d" % (e0, e_gpu, e_ref, rec["iterations"][0], rec["rejected"][0]))
    assert rec["frozen"][0] == 0 and e_gpu < 0.5 * e0
    assert abs(e_gpu - e_ref) <= 0.5e-3 * e_ref                      # four digits
    assert (int(rec["iterations"][0]), int(rec["rejected"][0])) == (want["record"]["iterations"], want["record"]["rejected"])
    cx.close()


def test_weight_zero_and_no_object_pixel_are_the_damped_entry_point_bit_for_bit():
    case = cc.small_solid_case()
    cx = CCtx(case)
    poses = _seven(case)[:4]
    Pd, rd, td = cx.damped(poses)
    P0, r0, t0 = cx.contour(poses, contour_weight=0.0)
    assert np.array_equal(P0.view(np.uint32), Pd.view(np.uint32)) and t0.tobytes() == td.tobytes()
    assert all(r0[h].tobytes()[:56] == rd[h].tobytes() for h in range(4))
    assert (r0["object_px"] == int((case.prob > 0).sum())).all() and not r0["pulled"].any() and not r0["unreached"].any() and not r0["beyond"].any()
    assert (r0["uncovered"] == r0["object_px"] - (r0["too_far"] + r0["grazing"] + r0["counted"])).all()
    Pw, rw, tw = cx.contour(poses)
    assert not np.array_equal(Pw, Pd)
    cx.set(rc.Case("no_object", case.verts, case.tris, case.K, case.W, case.H, case.depth, np.zeros_like(case.prob), case.G16, case.start16, **dict(case.prm, class_threshold=0.5)))
    Pd, rd, td = cx.damped(poses)
    Pn, rn, tn = cx.contour(poses)
    assert np.array_equal(Pn.view(np.uint32), Pd.view(np.uint32)) and tn.tobytes() == td.tobytes() and all(rn[h].tobytes()[:56] == rd[h].tobytes() for h in range(4))
    assert not rn["object_px"].any() and not rn["uncovered"].any() and not rn["pulled"].any()
    cx.close()


def test_batch_position_order_and_chunks_change_no_bit(monkeypatch):
    case = cc.small_solid_case(max_iterations=3)
    cx = CCtx(case)
    poses = _seven(case)[:5]
    monkeypatch.delenv("STOCS_REFINE_VISIBLE_CHUNK", raising=False)
    P, rec, tr, _ = _check_call(cx, poses)
    assert len(set(P[i].tobytes() for i in range(5))) == 5 and rec["pulled"].any()
    for i in (0, 3):
        Pi, ri, ti = cx.contour(poses[i][None])
        assert np.array_equal(Pi[0].view(np.uint32), P[i].view(np.uint32)) and ri[0].tobytes() == rec[i].tobytes() and ti[0].tobytes() == tr[i].tobytes(), i
    Pr, rr, tr_r = cx.contour(poses[::-1].copy())
    assert np.array_equal(Pr[::-1].view(np.uint32), P.view(np.uint32)) and rr[::-1].tobytes() == rec.tobytes() and tr_r[::-1].tobytes() == tr.tobytes()
    for chunk in (1, 2, 3):
        monkeypatch.setenv("STOCS_REFINE_VISIBLE_CHUNK", str(chunk))
        Pc, rc_, tc = cx.contour(poses)
        assert np.array_equal(Pc.view(np.uint32), P.view(np.uint32)) and rc_.tobytes() == rec.tobytes() and tc.tobytes() == tr.tobytes(), chunk
    cx.close()


def test_invalid_and_all_zero_poses_come_back_with_a_zero_record():
    case = cc.small_solid_case(max_iterations=2)
    cx = CCtx(case)
    s = case.start16
    nan = s.copy(); nan[5] = F(np.nan)
    inf = s.copy(); inf[12] = F(np.inf)
    behind = s.copy(); behind[14] = F(-0.8)          # a valid pose that shows nothing: no key, no pull, frozen at e = 0
    batch = np.stack([s, nan, np.zeros(16, F), behind, inf, s])
    P, rec, tr, _ = _check_call(cx, batch)
    for i in (1, 2, 4):
        assert np.array_equal(P[i].view(np.uint32), batch[i].view(np.uint32)) and rec[i].tobytes() == bytes(80) and tr[i].tobytes() == bytes(88 * 3)
    assert rec["frozen"][3] == 1 and rec["present"][3] == 0 and rec["pulled"][3] == 0 and rec["uncovered"][3] == rec["object_px"][3] > 0
    assert rec["cost"][3] == np.inf and np.array_equal(P[3].view(np.uint32), behind.view(np.uint32))
    assert rec[0].tobytes() == rec[5].tobytes() and np.array_equal(P[0].view(np.uint32), P[5].view(np.uint32))
    cx.close()


def test_the_plain_and_damped_forms_keep_their_bits_and_a_second_call_allocates_nothing():
    case = cc.small_solid_case()
    poses = _seven(case)[:4]
    plain_prm = dict((k, v) for k, v in case.prm.items() if k in dref.BASE_KEYS or k == "max_iterations")
    fresh = CCtx(case)
    Pd0, rd0, td0 = fresh.damped(poses)
    Pp0, rp0 = fresh.refine(poses, **plain_prm)
    fresh.close()
    cx = CCtx(case)
    P, rec, tr = cx.contour(poses)
    cx.cdetail(poses[0])
    Pd, rd, td = cx.damped(poses)
    Pp, rp = cx.refine(poses, **plain_prm)
    assert np.array_equal(Pd.view(np.uint32), Pd0.view(np.uint32)) and rd.tobytes() == rd0.tobytes() and td.tobytes() == td0.tobytes()
    assert np.array_equal(Pp.view(np.uint32), Pp0.view(np.uint32)) and rp.tobytes() == rp0.tobytes()
    before = cx.L.stocs_device_alloc_count()
    P2, rec2, tr2 = cx.contour(poses)
    P3, rec3, _ = cx.contour(poses[:2], trace=False)
    cx.cdetail(poses[1])
    assert cx.L.stocs_device_alloc_count() == before
    assert np.array_equal(P2.view(np.uint32), P.view(np.uint32)) and rec2.tobytes() == rec.tobytes() and tr2.tobytes() == tr.tobytes()
    assert np.array_equal(P3.view(np.uint32), P[:2].view(np.uint32)) and rec3.tobytes() == rec[:2].tobytes()
    cx.close()


def test_the_python_call_is_the_raw_call():
    case = cc.small_solid_case()
    cx = CCtx(case)
    P, rec, tr = cx.est.refine_poses_visible_contour(case.start16, trace=True, **case.prm)
    Pr, rr, trr = cx.contour(case.start16[None])
    assert np.array_equal(P.view(np.uint32), Pr.view(np.uint32)) and rec.tobytes() == rr.tobytes() and tr.tobytes() == trr.tobytes()
    st, near, sums = cx.est.refine_visible_contour_detail(case.start16, **case.prm)
    s2, n2, sums2 = cx.cdetail(case.start16)
    assert np.array_equal(st.reshape(-1), s2) and np.array_equal(near.reshape(-1), n2) and np.array_equal(sums.view(np.uint64), sums2.view(np.uint64))
    with pytest.raises(TypeError):
        cx.est.refine_poses_visible_contour(case.start16, no_such_parameter=1)
    cx.close()


def test_errors_come_in_the_documented_order():
    from model_matching_amd import capi
    L = capi.load()
    INVALID = -1
    est = _est()
    case = cc.small_solid_case()
    P, pP = capi.f32(case.start16)
    out = (C.c_float * 16)(); rec = (capi.RefineVisibleContourResult * 1)(); sums = (C.c_double * 29)()
    mk = lambda: (lambda p: (L.stocs_default_refine_visible_contour_params(C.byref(p)), p)[1])(capi.RefineVisibleContourParams())
    p, bad_damped, bad_new, bad_both = mk(), mk(), mk(), mk()
    bad_damped.damped.lambda_up = 0.5
    bad_new.pull_radius_px = 65
    bad_both.damped.base.min_view_cos = 2.0; bad_both.contour_weight = -1.0
    call = lambda ctx, poses, n, prm, o, r: L.stocs_refine_poses_visible_contour(ctx, poses, n, prm, o, r, None)
    assert call(None, pP, 1, C.byref(p), out, rec) == INVALID and b"NULL context" in L.stocs_last_error()
    assert call(est.h, pP, -1, C.byref(bad_new), out, rec) == INVALID and b"n -1" in L.stocs_last_error()
    assert call(est.h, None, 0, None, None, None) == 0
    assert call(est.h, None, 1, C.byref(p), out, rec) == INVALID and b"NULL" in L.stocs_last_error()
    assert call(est.h, pP, 1, None, out, rec) == INVALID and call(est.h, pP, 1, C.byref(p), None, rec) == INVALID and call(est.h, pP, 1, C.byref(p), out, None) == INVALID
    assert call(est.h, pP, 1, C.byref(bad_damped), out, rec) == INVALID and b"lambda_up" in L.stocs_last_error()
    assert call(est.h, pP, 1, C.byref(bad_new), out, rec) == INVALID and b"pull_radius_px" in L.stocs_last_error()
    assert call(est.h, pP, 1, C.byref(bad_both), out, rec) == INVALID and b"min_view_cos" in L.stocs_last_error()     # the damped parameters first
    rc_mesh = call(est.h, pP, 1, C.byref(p), out, rec)
    assert rc_mesh == capi.ERR_STATE and b"no mesh" in L.stocs_last_error()
    est.set_frame(case.depth, None, case.K, case.depth_scale)
    assert call(est.h, pP, 1, C.byref(p), out, rec) == rc_mesh and b"no mesh" in L.stocs_last_error()
    est2 = _est()
    est2.set_mesh(case.verts, case.tris)
    assert call(est2.h, pP, 1, C.byref(p), out, rec) == rc_mesh and b"no frame" in L.stocs_last_error()
    est2.set_frame(case.depth, None, case.K, case.depth_scale)          # a frame without a class image: behind "no frame"
    assert call(est2.h, pP, 1, C.byref(p), out, rec) == capi.ERR_STATE and b"no class image" in L.stocs_last_error()
    assert L.stocs_refine_visible_contour_detail(est2.h, pP, C.byref(p), None, None, sums) == capi.ERR_STATE and b"no class image" in L.stocs_last_error()
    assert call(est2.h, pP, 1, C.byref(bad_new), out, rec) == INVALID                                                   # parameters in front of the state
    est2.set_frame(case.depth, case.prob, case.K, case.depth_scale)
    assert call(est2.h, pP, 1, C.byref(p), out, rec) == 0
    est.close(); est2.close()
