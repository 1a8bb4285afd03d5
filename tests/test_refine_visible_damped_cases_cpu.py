"""The numpy restatement of the damped visible-surface refinement (tests/refine_visible_damped_ref.py) against the plain form's
restatement and against itself, without a GPU: K = 0 is the plain record, the accepted cost never rises, the undamped, unbounded form
about the camera's origin walks the plain form's trail, the sums about a pivot are the sums of the moved rows, the bounds bind, a
rejection raises lambda, and the Cm case on which the plain form fails ends nearer than it started."""
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
from oracle import refine_oracle as ro  # noqa: E402

F = np.float32
CONVERGE = rc.convergence_cases()
FEATURES = dc.feature_cases()


def _run(case, **prm):
    return dref.refine(case.start16, *case.args(), **dict(case.prm, **prm))


@pytest.mark.parametrize("case", CONVERGE + [rc.state_cases()["too_far"]], ids=repr)
def test_zero_iterations_give_the_plain_record_and_the_pose(case):
    out = _run(case, max_iterations=0)
    P, rec, _ = ref.refine(case.start16, *case.args(), **dict(case.prm, max_iterations=0))
    assert np.array_equal(out["pose"].view(np.uint32), case.start16.view(np.uint32)) and np.array_equal(P.view(np.uint32), out["pose"].view(np.uint32))
    assert all(out["record"][k] == rec[k] for k in ref.RECORD_FIELDS)
    assert out["record"]["evaluations"] == 1 and out["record"]["rejected"] == 0 and len(out["trace"]) == 1 and out["trace"][0]["accepted"] == 1
    ev = out["evs"][0]
    want = (ev["sums"][28] + float(F(case.prm.get("max_distance", 0.02)) * F(case.prm.get("max_distance", 0.02))) * rec["too_far"]) / (rec["counted"] + rec["too_far"])
    assert out["trace"][0]["cost"] == want and out["record"]["cost"] == F(want)


@pytest.mark.parametrize("name", sorted(FEATURES))
def test_the_accepted_cost_never_rises(name):
    out = _run(FEATURES[name])
    Ca, lam, n_acc, n_rej = None, None, 0, 0
    for e, row in enumerate(out["trace"]):
        assert row["state"] & dref.TRACE_EVALUATED
        if e == 0:
            assert row["accepted"] == 1
        elif row["accepted"]:
            assert row["cost"] < Ca and row["lambda_"] == max(lam / out_prm(FEATURES[name], "lambda_down"), 1e-9)
            n_acc += 1
        else:
            assert not row["cost"] < Ca and row["lambda_"] == min(lam * out_prm(FEATURES[name], "lambda_up"), 1e9)
            n_rej += 1
        Ca = row["cost"] if row["accepted"] else Ca
        lam = row["lambda_"]
    r = out["record"]
    assert (r["iterations"], r["rejected"], r["evaluations"]) == (n_acc, n_rej, n_acc + n_rej + 1) and r["cost"] == F(Ca) and r["lambda_"] == F(lam)
    last = max(e for e, row in enumerate(out["trace"]) if row["accepted"])
    assert np.array_equal(out["pose"].view(np.uint32), out["trace"][last]["pose"].view(np.uint32))
    assert all(r[k] == ref.record_of(out["evs"][last])[k] for k in ref.RECORD_FIELDS if k not in ("iterations", "frozen"))


def out_prm(case, key):
    return dref.split(case.prm)[2][key]


@pytest.mark.parametrize("case", CONVERGE, ids=repr)
def test_undamped_unbounded_steps_about_the_camera_walk_the_plain_trail(case):
    """lambda0 = 0, no bounds, pivot 0, as long as every step is accepted.  The first trial is made with lambda exactly 0 and equals the
    plain restatement's first update float for float.  Behind the first accepted step the contract's floor makes lambda 1e-9, not 0, so a
    later trial is, float for float, the plain form's own step functions (system_of, solve6, delta_of, apply_update) on the accepted
    evaluation with the diagonal times (1 + 1e-9), and lies next to the plain trail within 4 float ulps + 4 lambda cond(M) |x|: from
    (M + lambda D) x' = v, |x' - x| <= lambda |M^-1| |D| |x'| <= lambda cond(M) |x'|, and a pose entry moves by at most
    (1 + |t|) sqrt(3) < 4 times that."""
    out = _run(case, **dc.PLAIN_LIKE)
    _, _, trail = ref.refine(case.start16, *case.args(), **case.prm)
    assert out["trace"][0]["lambda_"] == 0.0 and np.array_equal(out["trace"][1]["pose"].view(np.uint32), trail[1].view(np.uint32))
    n = 1
    for e in range(1, len(out["trace"]) - 1):
        if not out["trace"][e]["accepted"]:
            break
        Pa, lam = out["trace"][e]["pose"], out["trace"][e]["lambda_"]
        assert lam == 1e-9 and np.array_equal(Pa.view(np.uint32), trail[e].view(np.uint32)) or n > 1
        M, v = ref.system_of(out["evs"][e]["sums"])
        cond = np.linalg.cond(M)
        for i in range(6):
            M[i, i] = M[i, i] * (1.0 + lam)
        x = ref.solve6(M, v)
        want = ref.apply_update(Pa, (ref.delta_of(x) @ Pa.reshape(4, 4).T.astype(np.float64))[:3, :])
        got = out["trace"][e + 1]["pose"]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), e
        plain_next = ref.step(Pa, *case.args(), **dict((k, v_) for k, v_ in case.prm.items() if k in dref.BASE_KEYS))[0]
        tol = 4 * np.spacing(np.abs(plain_next)) + 4 * lam * cond * np.linalg.norm(x)
        assert (np.abs(got.astype(np.float64) - plain_next.astype(np.float64)) <= tol).all(), e
        n += 1
    print("PLAIN TRAIL %s trials compared %d" % (case.name, n))
    assert n >= 3


@pytest.mark.parametrize("case", CONVERGE, ids=repr)
def test_the_first_undamped_trial_does_not_depend_on_the_pivot(case):
    """This pins T.  The undamped Gauss-Newton SOLUTION does not depend on the pivot: with lambda0 = 0 and no bounds the rotation
    about a point of the object is the rotation about the camera's origin and the translations differ by omega x c, within the solve's
    term of the pose tolerance, cond 2^-50.  The composed trial is the same only to first order: step 6 turns about c by R(x) c, not by
    c + omega x c, so the translation columns differ by (R - I - [omega]x) c, at most 2 |omega|^2 |c| (every entry of R - I - [omega]x is a
    sum of at most two products of two of the angles' sines and 1 - cosines); the trials agree within the pose tolerance plus that term,
    and their rotations within the pose tolerance alone.  Damped, they differ by far more."""
    ev = ref.evaluate(case.start16, *case.args(), **dict((k, v) for k, v in case.prm.items() if k in dref.BASE_KEYS))
    d0 = dref.split(dict(dc.PLAIN_LIKE))[2]
    d1 = dref.split(dict(dc.PLAIN_LIKE, pivot=1, pivot_model=dc.pivot_of(case)))[2]
    a, b = dref.next_trial(case.start16, ev["sums"], 0.0, d0), dref.next_trial(case.start16, ev["sums"], 0.0, d1)
    c = b["c"]
    assert np.linalg.norm(c) > 0.5 and not np.any(a["c"])
    cond = max(a["cond"], b["cond"])
    dx = np.abs(np.concatenate([b["x"][:3] - a["x"][:3], b["x"][3:] - (a["x"][3:] + np.cross(a["x"][:3], c))]))
    print("PIVOT %s cond %.3g / %.3g max |dx| %.3g of %.3g" % (case.name, a["cond"], b["cond"], dx.max(), cond * 2.0 ** -50))
    assert (dx <= cond * 2.0 ** -50).all()
    tol = ro.pose_tolerance(a["T34"], cond)
    dev = np.abs(a["T34"] - b["T34"])
    second = 2 * np.linalg.norm(a["x"][:3]) ** 2 * np.linalg.norm(c)
    assert (dev[:, :3] <= tol[:, :3]).all() and (dev[:, 3] <= tol[:, 3] + second).all()
    # the moved sums are the sums of the moved rows
    A = ev["A"].copy()
    A[:, :3] -= np.cross(np.broadcast_to(b["c"], (len(A), 3)), A[:, 3:])
    M, v = dref.system_about(ev["sums"], b["c"])
    assert np.allclose(M, A.T @ A, rtol=0, atol=1e-9 * np.abs(ref.system_of(ev["sums"])[0]).max()) and np.allclose(v, A.T @ ev["b"], rtol=0, atol=1e-12)
    a1, b1 = dref.next_trial(case.start16, ev["sums"], 1.0, d0), dref.next_trial(case.start16, ev["sums"], 1.0, d1)
    assert (np.abs(a1["T34"] - b1["T34"]) > 100 * tol).any()


@pytest.mark.parametrize("name,which", [("cm_rotation_bound", 0), ("cm_translation_bound", 1)])
def test_a_bounded_step_is_at_its_bound(name, which):
    case = FEATURES[name]
    out = _run(case)
    d = dref.split(case.prm)[2]
    hit = 0
    for st in out["steps"]:
        if st is None:
            continue
        nr, nt = np.linalg.norm(st["x"][:3]), np.linalg.norm(st["x"][3:])
        assert nr <= d["max_step_rotation"] * (1 + 4e-16) and nt <= d["max_step_translation"] * (1 + 4e-16)
        if st["s"] < 1:
            got, want = (nr, d["max_step_rotation"]) if which == 0 else (nt, d["max_step_translation"])
            assert abs(got - want) <= 4e-16 * want
            hit += 1
    assert hit >= 1
    free = _run(case, **dc.NO_BOUNDS)["steps"][0]
    assert free["s"] == 1.0 and (np.linalg.norm(free["x"][:3]), np.linalg.norm(free["x"][3:]))[which] > (d["max_step_rotation"], d["max_step_translation"])[which]


def test_a_rejection_raises_lambda_and_keeps_the_accepted_pose():
    out = _run(FEATURES["cm_rejection"])
    assert out["record"]["rejected"] >= 1
    e = next(e for e, row in enumerate(out["trace"]) if not row["accepted"])
    assert out["trace"][e]["lambda_"] > out["trace"][e - 1]["lambda_"] and out["trace"][e]["lambda_"] == out["trace"][e - 1]["lambda_"] * 16
    assert not np.array_equal(out["pose"], out["trace"][e]["pose"])


def test_a_trial_without_pixels_is_rejected_and_fewer_than_six_freeze():
    lost = dc.lost_pixels_case()
    out = _run(lost)
    assert ref.record_of(out["evs"][0])["counted"] == 6 and ref.record_of(out["evs"][1])["counted"] == 0
    assert out["trace"][1]["cost"] == np.inf and out["trace"][1]["accepted"] == 0 and out["record"]["rejected"] == 2 and out["record"]["frozen"] == 0
    assert np.array_equal(out["pose"].view(np.uint32), lost.start16.view(np.uint32)) and out["record"]["counted"] == 6
    five = dc.five_pixels_case()
    out = _run(five)
    r = out["record"]
    assert (r["counted"], r["frozen"], r["iterations"], r["evaluations"]) == (5, 1, 0, 1) and r["cost"] == np.inf
    assert out["trace"][0]["state"] == dref.TRACE_EVALUATED | dref.TRACE_FROZE and out["trace"][1]["state"] == 0
    assert np.array_equal(out["pose"].view(np.uint32), five.start16.view(np.uint32))
    for bad in (np.zeros(16, F), np.where(np.arange(16) == 13, np.nan, five.start16).astype(F)):
        out = dref.refine(bad, *five.args(), **five.prm)
        assert np.array_equal(out["pose"].view(np.uint32), bad.view(np.uint32)) and not any(out["record"].values()) and out["trace"][0]["state"] == 0


def test_the_cm_case_where_the_plain_form_fails():
    """The 160 x 120 analytic Cm frame, the level-4 mesh, two starts 10 mm / 4 degrees off: five plain iterations end at more than five
    times the start's ADD (measured: 10.5 mm -> 135.8 and 131.6 mm); the damped form with its defaults and K = 10 ends below the start's
    (measured: 0.88 and 6.11 mm)."""
    pts = dc.cm_points()
    assert dc.cm_frame(160, 120)[2] == 1992
    for start in dc.CM_STARTS:
        case = dc.cm_case(start, max_distance=0.02)
        assert len(case.tris) == 6400
        a0 = dref.add_error(case.start16, case.G16, pts)
        P, _, _ = ref.refine(case.start16, *case.args(), max_iterations=5, max_distance=0.02)
        a_plain = dref.add_error(P, case.G16, pts)
        out = dref.refine(case.start16, *case.args(), max_iterations=10, max_distance=0.02, pivot_model=dc.pivot_of(case))
        a_damped = dref.add_error(out["pose"], case.G16, pts)
        print("CM start %.2f mm plain %.2f mm damped %.2f mm (accepted %d, rejected %d)" % (a0 * 1e3, a_plain * 1e3, a_damped * 1e3, out["record"]["iterations"],
                                                                                           out["record"]["rejected"]))
        assert 0.009 < a0 < 0.012 and a_plain > 5 * a0
        assert a_damped < a0


@pytest.mark.parametrize("case", CONVERGE, ids=repr)
def test_convergence_cases_reach_a_tenth_within_eight(case):
    out = _run(case, max_iterations=8, pivot_model=dc.pivot_of(case))
    e0, e1 = ref.vertex_error(case.start16, case.G16, case.verts), ref.vertex_error(out["pose"], case.G16, case.verts)
    print("CONVERGENCE %s e0 %.4g e_damped %.4g accepted %d rejected %d" % (case.name, e0, e1, out["record"]["iterations"], out["record"]["rejected"]))
    assert e1 <= 0.1 * e0
