"""stocs_refine_poses_visible_damped on the GPU against the numpy restatement of its contract (tests/refine_visible_damped_ref.py),
followed step by step through the trace and re-synchronised on the library's own state: at every (pose, e) the evaluated pose is within
4 float ulps + cond(M'') 2^-50 of a longdouble restatement of the step from the library's accepted state (oracle/refine_oracle.py's
pose_tolerance, as for the plain form), its cost within the rounding bound of the double sum over the divisor, the decision equal
wherever the costs differ by more than their bounds (no comparison of these cases falls inside: the cap is zero), lambda equal as a
double; counts and records bit for bit.  Frames are at most 128 x 96.  Every call goes through buffers with sentinel bytes behind them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import refine_visible_cases as rc  # noqa: E402
import refine_visible_damped_cases as dc  # noqa: E402
import refine_visible_damped_ref as dref  # noqa: E402
import refine_visible_ref as ref  # noqa: E402
import vsd_cases as vc  # noqa: E402
from oracle import refine_oracle as ro  # noqa: E402
from test_refine_visible_gpu import Ctx, SENTINEL, _est, _seven  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
FEATURES = dc.feature_cases()


class DCtx(Ctx):
    """the plain form's test context with the raw damped entry point on padded host buffers"""
    def dparams(self, **kw):
        p = self.capi.RefineVisibleDampedParams()
        self.L.stocs_default_refine_visible_damped_params(C.byref(p))
        for k, v in dict(self.case.prm, **kw).items():
            if k == "pivot_model":
                p.pivot_model[:] = [float(x) for x in v]
            elif k in dict(self.capi.RefineVisibleParams._fields_):
                setattr(p.base, k, v)
            else:
                setattr(p, k, v)
        return p

    def damped(self, poses, trace=True, **kw):
        from model_matching_amd.estimator import _REFINE_VISIBLE_DAMPED_DTYPE, _REFINE_VISIBLE_TRACE_DTYPE
        P, pP = self.capi.f32(poses)
        n = P.size // 16
        p = self.dparams(**kw)
        rows = p.base.max_iterations + 1
        out = np.empty(n * 16 + 8, F); out.view(np.uint8)[:] = SENTINEL
        rec = np.empty((n + 1) * 56, np.uint8); rec[:] = SENTINEL
        tr = np.empty((n * rows + 1) * 88, np.uint8); tr[:] = SENTINEL
        self.capi.check(self.L.stocs_refine_poses_visible_damped(self.est.h, pP, n, C.byref(p), out.ctypes.data_as(self.capi._fp),
                                                                 rec.ctypes.data_as(C.POINTER(self.capi.RefineVisibleDampedResult)),
                                                                 tr.ctypes.data_as(C.POINTER(self.capi.RefineVisibleTrace)) if trace else None))
        assert np.all(out[n * 16:].view(np.uint8) == SENTINEL) and np.all(rec[n * 56:] == SENTINEL), "bytes behind an output were written"
        assert np.all(tr[n * rows * 88 if trace else 0:] == SENTINEL), "bytes behind the trace were written"
        return out[: n * 16].reshape(n, 16).copy(), rec[: n * 56].view(_REFINE_VISIBLE_DAMPED_DTYPE).copy(), \
            (tr[: n * rows * 88].view(_REFINE_VISIBLE_TRACE_DTYPE).copy().reshape(n, rows) if trace else None)

    def cost0(self, poses, **kw):
        """the cost of each pose as a K = 0 call gives it, and that call's records"""
        P, rec, _ = self.damped(poses, trace=False, **dict(kw, max_iterations=0))
        assert np.array_equal(P.view(np.uint32), np.asarray(poses, F).reshape(-1, 16).view(np.uint32))
        return rec["cost"].copy(), rec


BASE_FIELDS = [k for k in ref.RECORD_FIELDS if k not in ("iterations", "frozen", "rms")]


def _follow(cx, start, P, rec, trace, **kw):
    """one pose: the library's trace against the restatement, stepped from the library's own state -> the number of comparisons made"""
    prm = dict(cx.case.prm, **kw)
    K, base, d = dref.split(prm)
    args = cx.case.args()
    start = np.asarray(start, F)
    if not ref.pose_valid(start):
        assert np.array_equal(P.view(np.uint32), start.view(np.uint32)) and rec.tobytes() == bytes(56) and not trace["state"].any()
        assert trace.tobytes() == bytes(88 * (K + 1))
        return 0
    Pa = ev_a = Ca = lam = None
    n_acc = n_rej = n_eval = frozen = compared = 0
    Ca_lib = None
    for e in range(K + 1):
        row = trace[e]
        if frozen:
            assert row.tobytes() == bytes(88), e
            continue
        assert row["state"] & 1, e
        Pt = row["pose"].copy()
        ev = ref.evaluate(Pt, *args, **base)
        r = ref.record_of(ev)
        Cr = dref.cost_of(ev["sums"], r["counted"], r["too_far"], base["max_distance"])
        bound = dref.cost_bound(ev, r["too_far"])
        if np.isinf(Cr):
            assert row["cost"] == np.inf, e
        else:
            assert abs(row["cost"] - Cr) <= bound, (e, row["cost"], Cr, bound)
        n_eval += 1
        if e == 0:
            assert np.array_equal(Pt.view(np.uint32), start.view(np.uint32)) and row["accepted"] == 1 and row["lambda"] == d["lambda0"]
            ok = True
        else:
            nt = dref.next_trial(Pa, dref.sums_longdouble(ev_a), lam, d, dtype=np.longdouble)
            T34 = nt["T34"].astype(np.float64)
            tol = ro.pose_tolerance(T34, nt["cond"])
            dev = np.abs(Pt.reshape(4, 4).T.astype(np.float64)[:3, :] - T34)
            print("TRIAL %s e=%d cond %.3g s %.3g max dev/tol %.3g cost %.6g" % (cx.case.name, e, nt["cond"], nt["s"], (dev / tol).max(), row["cost"]))
            assert (dev <= tol).all(), (e, (dev / tol).max(), nt["cond"])
            assert np.array_equal(Pt[[3, 7, 11, 15]].view(np.uint32), start[[3, 7, 11, 15]].view(np.uint32))
            both = bound + dref.cost_bound(ev_a, ref.record_of(ev_a)["too_far"])
            decided = np.isinf(Cr) or abs(Cr - Ca) > both
            assert decided, "a decision of case %s falls inside the rounding bound at e = %d: the cap is zero" % (cx.case.name, e)
            compared += 1
            ok = bool(row["accepted"])
            assert ok == (Cr < Ca), (e, Cr, Ca)
            assert ok == (row["cost"] < Ca_lib)
            assert row["lambda"] == dref.decide(Cr, Ca, lam, d)[1], (e, row["lambda"], lam)
        lam = float(row["lambda"])
        if ok:
            Pa, ev_a, Ca, Ca_lib = Pt, ev, Cr, float(row["cost"])
            n_acc += e > 0
        else:
            n_rej += 1
        if e < K:
            froze = (e == 0 and ref.record_of(ev_a)["counted"] < 6) or dref.next_trial(Pa, ev_a["sums"], lam, d)["T34"] is None
            assert bool(row["state"] & 2) == froze, e
            frozen = 1 if froze else 0
        else:
            assert row["state"] == 1
    want = ref.record_of(ev_a)
    assert np.array_equal(P.view(np.uint32), Pa.view(np.uint32))
    assert all(int(rec[k]) == want[k] for k in BASE_FIELDS), (rec, want)
    assert abs(float(rec["rms"]) - float(want["rms"])) <= 4 * np.spacing(F(want["rms"])) + 1e-12
    assert (int(rec["iterations"]), int(rec["rejected"]), int(rec["evaluations"]), int(rec["frozen"])) == (n_acc, n_rej, n_eval, frozen)
    with np.errstate(over="ignore"):
        assert rec["cost"] == F(Ca_lib) and rec["lambda"] == F(lam) and rec["reserved"] == 0
    return compared


def _check_call(cx, poses, **kw):
    """a call with the trace, followed pose by pose; the same call without the trace gives the same bits; the records are a K = 0 call's on
    the returned poses bit for bit; the cost of what comes back is not above the cost of what went in"""
    poses = np.asarray(poses, F).reshape(-1, 16)
    P, rec, tr = cx.damped(poses, **kw)
    compared = sum(_follow(cx, poses[h], P[h], rec[h], tr[h], **kw) for h in range(len(poses)))
    P2, rec2, none = cx.damped(poses, trace=False, **kw)
    assert none is None and np.array_equal(P2.view(np.uint32), P.view(np.uint32)) and rec2.tobytes() == rec.tobytes()
    c_in, _ = cx.cost0(poses, **kw)
    c_out, rec0 = cx.cost0(P, **kw)
    for h in range(len(poses)):
        assert c_out[h] <= c_in[h] or (np.isnan(c_out[h]) and np.isnan(c_in[h])), (h, c_out[h], c_in[h])
        assert c_out[h] == rec["cost"][h]
        assert all(rec0[k][h] == rec[k][h] for k in BASE_FIELDS + ["rms"]), h      # the record describes the returned pose, bit for bit
    return P, rec, tr, compared


@pytest.mark.parametrize("name", sorted(FEATURES))
def test_one_pose_follows_the_restatement(name):
    case = FEATURES[name]
    cx = DCtx(case)
    G = cx.L.stocs_refine_visible_groups(case.W, case.H)
    assert G == (1 if name == "cm_small_frame" else case.W * case.H // 2048)
    P, rec, tr, compared = _check_call(cx, case.start16[None])
    K, _, d = dref.split(case.prm)
    assert compared == K and rec["evaluations"][0] == K + 1
    if name == "cm_rejection" or name.startswith("converge"):
        assert rec["rejected"][0] >= 1
        e = int(np.flatnonzero(tr[0]["accepted"] == 0)[0])
        assert tr[0]["lambda"][e] == tr[0]["lambda"][e - 1] * d["lambda_up"] and rec["iterations"][0] + rec["rejected"][0] == K
    if name.endswith("_bound"):      # the library's own first trial is at the bound: the step from the start, measured on its pose
        nt = dref.next_trial(case.start16, cx.ref_eval(case.start16, **dref.split(case.prm)[1])["sums"], d["lambda0"], d)
        assert nt["s"] < 1
        got = np.asarray(tr[0]["pose"][1], F).reshape(4, 4).T.astype(np.float64)
        assert np.abs(got[:3, :] - nt["T34"]).max() <= 4 * 2.0 ** -24
    if name.startswith("converge"):
        e0, e1 = ref.vertex_error(case.start16, case.G16, case.verts), ref.vertex_error(P[0], case.G16, case.verts)
        print("CONVERGENCE %s e0 %.4g e_gpu %.4g" % (name, e0, e1))
        assert e1 <= 0.1 * e0
    cx.close()


def test_pivots_differ_and_pivot_zero_ignores_pivot_model():
    cx = DCtx(FEATURES["box_pivot_camera"])
    P0, r0, _ = cx.damped(cx.case.start16[None])
    P0b, r0b, _ = cx.damped(cx.case.start16[None], pivot_model=(0.5, 0.5, 0.5))
    P1, r1, _ = cx.damped(cx.case.start16[None], pivot=1)
    assert np.array_equal(P0.view(np.uint32), P0b.view(np.uint32)) and r0.tobytes() == r0b.tobytes()
    assert not np.array_equal(P0, P1)
    cx.close()


def test_batch_position_and_order_change_no_bit():
    case = FEATURES["converge_ellipsoid2"]
    cx = DCtx(case)
    poses = _seven(case)
    P, rec, tr, _ = _check_call(cx, poses, max_iterations=4)
    assert len(set(P[i].tobytes() for i in range(7))) == 7
    for i in range(7):
        Pi, ri, ti = cx.damped(poses[i][None], max_iterations=4)
        assert np.array_equal(Pi[0].view(np.uint32), P[i].view(np.uint32)) and ri[0].tobytes() == rec[i].tobytes() and ti[0].tobytes() == tr[i].tobytes(), i
    Pr, rr, tr_r = cx.damped(poses[::-1].copy(), max_iterations=4)
    assert np.array_equal(Pr[::-1].view(np.uint32), P.view(np.uint32)) and rr[::-1].tobytes() == rec.tobytes() and tr_r[::-1].tobytes() == tr.tobytes()
    cx.close()


def test_chunks_change_no_bit(monkeypatch):
    case = FEATURES["converge_ellipsoid1"]
    cx = DCtx(case)
    poses = _seven(case)[:5]
    monkeypatch.delenv("STOCS_REFINE_VISIBLE_CHUNK", raising=False)
    P, rec, tr = cx.damped(poses, max_iterations=3)
    for chunk in (1, 2, 3):
        monkeypatch.setenv("STOCS_REFINE_VISIBLE_CHUNK", str(chunk))
        Pc, rc_, tc = cx.damped(poses, max_iterations=3)
        assert np.array_equal(Pc.view(np.uint32), P.view(np.uint32)) and rc_.tobytes() == rec.tobytes() and tc.tobytes() == tr.tobytes(), chunk
    cx.close()


def test_invalid_frozen_and_lost_poses_inside_a_batch():
    case = dc.lost_pixels_case()
    cx = DCtx(case)
    s = case.start16
    behind = s.copy(); behind[14] = F(-0.8)                      # a valid pose that shows nothing: fewer than 6 counted pixels at e = 0
    nan = s.copy(); nan[5] = F(np.nan)
    inf = s.copy(); inf[12] = F(np.inf)
    batch = np.stack([s, nan, behind, np.zeros(16, F), s, inf])
    P, rec, tr, _ = _check_call(cx, batch)
    for i in (0, 4):          # the trial counts no pixel: C = +inf, rejected at e = 1 and 2, the start comes back
        assert np.array_equal(P[i].view(np.uint32), s.view(np.uint32)) and rec["rejected"][i] == 2 and rec["iterations"][i] == 0 and rec["frozen"][i] == 0
        assert rec["counted"][i] == 6 and tr[i]["cost"][1] == np.inf and not tr[i]["accepted"][1:].any()
    for i in (1, 3, 5):
        assert np.array_equal(P[i].view(np.uint32), batch[i].view(np.uint32)) and rec[i].tobytes() == bytes(56) and tr[i].tobytes() == bytes(88 * 3)
    assert rec["frozen"][2] == 1 and rec["present"][2] == 0 and rec["evaluations"][2] == 1 and np.array_equal(P[2].view(np.uint32), behind.view(np.uint32))
    cx.set(dc.five_pixels_case())                                   # five counted pixels at e = 0
    P, rec, tr, _ = _check_call(cx, s[None])
    assert rec["counted"][0] == 5 and rec["frozen"][0] == 1 and rec["cost"][0] == np.inf and tr[0]["state"][0] == 3 and np.array_equal(P[0].view(np.uint32), s.view(np.uint32))
    P, rec, _ = cx.damped(s[None], trace=False, max_iterations=0)   # K = 0: the plain record, not frozen
    Pp, rp = cx.refine(s[None], max_iterations=0)
    assert rec["frozen"][0] == 0 and rec[0].tobytes()[:40] == rp[0].tobytes() and np.array_equal(P.view(np.uint32), Pp.view(np.uint32))
    cx.close()


def test_zero_iterations_are_the_plain_record():
    for name in ("converge_box", "class_image"):
        case = FEATURES[name]
        cx = DCtx(case)
        poses = _seven(case)[:3]
        P, rec, tr = cx.damped(poses, max_iterations=0)
        Pp, rp = cx.refine(poses, max_iterations=0, **dict((k, v) for k, v in case.prm.items() if k in dref.BASE_KEYS))
        assert np.array_equal(P.view(np.uint32), poses.view(np.uint32)) and np.array_equal(Pp.view(np.uint32), P.view(np.uint32))
        for h in range(3):
            assert rec[h].tobytes()[:40] == rp[h].tobytes() and rec["evaluations"][h] == 1 and rec["rejected"][h] == 0 and tr.shape == (3, 1)
            _follow(cx, poses[h], P[h], rec[h], tr[h], max_iterations=0)
        cx.close()


def test_the_plain_form_keeps_its_bits_and_a_second_call_allocates_nothing():
    case = FEATURES["converge_ellipsoid2"]
    plain_prm = dict((k, v) for k, v in case.prm.items() if k in dref.BASE_KEYS or k == "max_iterations")
    plain_case = rc.Case(case.name, case.verts, case.tris, case.K, case.W, case.H, case.depth, case.prob, case.G16, case.start16, case.depth_scale, **plain_prm)
    fresh = Ctx(plain_case)
    poses = _seven(case)
    P_fresh, rec_fresh = fresh.refine(poses)
    fresh.close()
    cx = DCtx(case)
    P, rec, tr = cx.damped(poses)
    cx.set(plain_case)
    P_plain, rec_plain = cx.refine(poses)
    assert np.array_equal(P_plain.view(np.uint32), P_fresh.view(np.uint32)) and rec_plain.tobytes() == rec_fresh.tobytes()
    cx.set(case)
    before = cx.L.stocs_device_alloc_count()
    P2, rec2, tr2 = cx.damped(poses)
    P3, rec3, _ = cx.damped(poses[:4], trace=False)
    assert cx.L.stocs_device_alloc_count() == before
    assert np.array_equal(P2.view(np.uint32), P.view(np.uint32)) and rec2.tobytes() == rec.tobytes() and tr2.tobytes() == tr.tobytes()
    assert np.array_equal(P3.view(np.uint32), P[:4].view(np.uint32)) and rec3.tobytes() == rec[:4].tobytes()
    cx.close()


def test_the_python_call_pivots_about_the_mean_vertex():
    case = FEATURES["box_pivot_off_origin"]
    cx = DCtx(case)
    base = dict((k, v) for k, v in case.prm.items() if k != "pivot_model")
    v = case.verts + F(0.01)                                # a mesh whose mean vertex is off the origin
    shifted = rc.Case("shifted", v, case.tris, case.K, case.W, case.H, case.depth, None, case.G16, case.start16, **base)
    cx.set(shifted)
    P, rec, tr = cx.est.refine_poses_visible_damped(case.start16, trace=True, **base)
    Pr, rr, trr = cx.damped(case.start16[None], pivot_model=dc.pivot_of(shifted))
    assert np.array_equal(P.view(np.uint32), Pr.view(np.uint32)) and rec.tobytes() == rr.tobytes() and tr.tobytes() == trr.tobytes()
    Po, _, _ = cx.damped(case.start16[None], pivot_model=(0.0, 0.0, 0.0))
    assert not np.array_equal(P, Po)
    P2, rec2 = cx.est.refine_poses_visible_damped(case.start16, **base)
    assert np.array_equal(P2.view(np.uint32), P.view(np.uint32)) and rec2.tobytes() == rec.tobytes()
    with pytest.raises(TypeError):
        cx.est.refine_poses_visible_damped(case.start16, no_such_parameter=1)
    cx.close()


def test_errors_come_in_the_documented_order():
    from model_matching_amd import capi
    L = capi.load()
    INVALID = -1
    est = _est()
    case = rc.state_cases()["counted"]
    P, pP = capi.f32(case.start16)
    out = (C.c_float * 16)(); rec = (capi.RefineVisibleDampedResult * 1)()
    mk = lambda: (lambda p: (L.stocs_default_refine_visible_damped_params(C.byref(p)), p)[1])(capi.RefineVisibleDampedParams())
    p, bad_base, bad_new, bad_both = mk(), mk(), mk(), mk()
    bad_base.base.max_distance = 0.0
    bad_new.lambda_up = 0.5
    bad_both.base.min_view_cos = 2.0; bad_both.pivot = 7
    call = lambda ctx, poses, n, prm, o, r: L.stocs_refine_poses_visible_damped(ctx, poses, n, prm, o, r, None)
    assert call(None, pP, 1, C.byref(p), out, rec) == INVALID and b"NULL context" in L.stocs_last_error()
    assert call(est.h, pP, -1, C.byref(bad_new), out, rec) == INVALID and b"n -1" in L.stocs_last_error()
    assert call(est.h, None, 0, None, None, None) == 0
    assert call(est.h, None, 1, C.byref(p), out, rec) == INVALID and b"NULL" in L.stocs_last_error()
    assert call(est.h, pP, 1, None, out, rec) == INVALID and call(est.h, pP, 1, C.byref(p), None, rec) == INVALID and call(est.h, pP, 1, C.byref(p), out, None) == INVALID
    assert call(est.h, pP, 1, C.byref(bad_base), out, rec) == INVALID and b"max_distance" in L.stocs_last_error()
    assert call(est.h, pP, 1, C.byref(bad_new), out, rec) == INVALID and b"lambda_up" in L.stocs_last_error()
    assert call(est.h, pP, 1, C.byref(bad_both), out, rec) == INVALID and b"min_view_cos" in L.stocs_last_error()     # the base parameters first
    rc_mesh = call(est.h, pP, 1, C.byref(p), out, rec)
    assert rc_mesh == capi.ERR_STATE and b"no mesh" in L.stocs_last_error()
    est.set_frame(case.depth, None, case.K, case.depth_scale)
    assert call(est.h, pP, 1, C.byref(p), out, rec) == rc_mesh and b"no mesh" in L.stocs_last_error()
    est2 = _est()
    est2.set_mesh(case.verts, case.tris)
    assert call(est2.h, pP, 1, C.byref(p), out, rec) == rc_mesh and b"no frame" in L.stocs_last_error()
    est.close(); est2.close()
