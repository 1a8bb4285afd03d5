"""numpy restatement of the damped visible-surface refinement contract written at stocs_refine_poses_visible_damped in
include/stocs_hip.h, on the plain form's restatement (refine_visible_ref.evaluate, system_of, solve6, delta_of, apply_update): the cost of
an evaluation, the accept / reject decision and lambda, the sums about a pivot, the damped solve, the bound, the motion about the pivot
and the loop over K + 1 evaluations on float32 poses.  Written from the contract, not from the kernel.  No GPU, numpy only."""
import numpy as np

import refine_visible_ref as ref

F = np.float32
LAMBDA_MIN, LAMBDA_MAX = 1e-9, 1e9
DAMPED_DEFAULTS = dict(lambda0=1.0, lambda_down=4.0, lambda_up=16.0, max_step_rotation=float(F(np.deg2rad(5.0))), max_step_translation=0.01, pivot=1,
                       pivot_model=(0.0, 0.0, 0.0))
BASE_KEYS = ("max_distance", "min_view_cos", "class_threshold")
TRACE_EVALUATED, TRACE_FROZE = 1, 2       # bits of a trace row's state; 0: the row was not evaluated (the pose was invalid or frozen)


def split(prm):
    """parameters -> (K, the plain form's gates as evaluate takes them, the damped ones as floats of the struct)"""
    p = dict(ref.DEFAULTS, **DAMPED_DEFAULTS)
    for k, v in prm.items():
        if k not in p:
            raise TypeError("unknown parameter %r" % (k,))
        p[k] = v
    base = dict((k, p[k]) for k in BASE_KEYS)
    d = dict((k, float(F(p[k]))) for k in ("lambda0", "lambda_down", "lambda_up", "max_step_rotation", "max_step_translation"))
    d["pivot"] = int(p["pivot"])
    d["pivot_model"] = np.asarray(p["pivot_model"], F).astype(np.float64)
    return int(p["max_iterations"]), base, d


def counts_of(ev):
    return ref.record_of(ev)


def cost_of(sums, counted, too_far, max_distance):
    """C = (S[28] + (double)max_d2 too_far) / (counted + too_far), max_d2 the float product; +inf when counted < 6"""
    if counted < 6:
        return np.inf
    md2 = F(max_distance) * F(max_distance)
    return float((np.float64(sums[28]) + np.float64(md2) * np.float64(too_far)) / np.float64(counted + too_far))


def cost_bound(ev, too_far):
    """the rounding bound of a cost: the bound of the sum S[28] over the divisor"""
    n = ev["sums"][27] + too_far
    return float(ref.sums_bound(ev)[28] / n) if n > 0 else 0.0


def skew(c):
    return np.array([[0, -c[2], c[1]], [c[2], 0, -c[0]], [-c[1], c[0], 0]], c.dtype)


def pivot_of(Pa16, d, dtype=np.float64):
    """step 1: c = 0, or Ra pivot_model + ta from the float entries of Pa"""
    if d["pivot"] == 0:
        return np.zeros(3, dtype)
    T = np.asarray(Pa16, F).reshape(4, 4).T.astype(dtype)
    pm = d["pivot_model"].astype(dtype)
    return np.array([((T[r, 0] * pm[0] + T[r, 1] * pm[1]) + T[r, 2] * pm[2]) + T[r, 3] for r in range(3)], dtype)


def system_about(sums, c, dtype=np.float64):
    """step 2: M' = T M T^T, v' = T v with T = [[I, -[c]x], [0, I]]"""
    M, v = ref.system_of(np.asarray(sums, dtype), dtype)
    T = np.eye(6, dtype=dtype)
    T[:3, 3:] = -skew(np.asarray(c, dtype))
    return (T @ M) @ T.T, T @ v


def next_trial(Pa16, sums, lam, d, dtype=np.float64):
    """steps 1-7 from an accepted state -> dict: T34 (the next trial's 3x4 before the rounding to float, None when the solve fails),
    cond (of M''), x (after the bound), s, c"""
    c = pivot_of(Pa16, d, dtype)
    M, v = system_about(sums, c, dtype)
    Md = M.copy()
    for i in range(6):
        Md[i, i] = M[i, i] * (dtype(1) + dtype(lam))
    x = ref.solve6(Md, v)
    if x is None:
        return dict(T34=None, cond=np.inf, x=None, s=1.0, c=c)
    s = dtype(1)
    nr = np.sqrt(x[0] * x[0] + (x[1] * x[1] + x[2] * x[2]))
    nt = np.sqrt(x[3] * x[3] + (x[4] * x[4] + x[5] * x[5]))
    with np.errstate(all="ignore"):
        if nr > 0:
            s = min(s, dtype(d["max_step_rotation"]) / nr)
        if nt > 0:
            s = min(s, dtype(d["max_step_translation"]) / nt)
    x = s * x
    D = ref.delta_of(x)
    R = D[:3, :3]
    Rc = np.array([(R[r, 0] * c[0] + R[r, 1] * c[1]) + R[r, 2] * c[2] for r in range(3)], dtype)
    D[:3, 3] = (x[3:] + c) - Rc
    T = np.asarray(Pa16, F).reshape(4, 4).T.astype(dtype)
    return dict(T34=(D @ T)[:3, :], cond=float(np.linalg.cond(Md.astype(np.float64))), x=x, s=float(s), c=c)


def sums_longdouble(ev):
    """the 29 sums of an evaluation's rows in longdouble"""
    L = np.longdouble
    A, b = ev["A"].astype(L), ev["b"].astype(L)
    sums = np.zeros(29, L)
    j = 0
    for r in range(6):
        for c in range(r, 6):
            sums[j] = (A[:, r] * A[:, c]).sum(); j += 1
    for r in range(6):
        sums[21 + r] = (A[:, r] * b).sum()
    sums[27] = len(b)
    sums[28] = (b * b).sum()
    return sums


def decide(C, Ca, lam, d):
    """the decision on a trial of cost C against the accepted cost Ca -> (accepted, the lambda after it)"""
    if C < Ca:
        return True, max(lam / d["lambda_down"], LAMBDA_MIN)
    return False, min(lam * d["lambda_up"], LAMBDA_MAX)


def zero_record():
    r = dict((k, F(0) if k == "rms" else 0) for k in ref.RECORD_FIELDS)
    r.update(evaluations=0, rejected=0, cost=F(0), lambda_=F(0))
    return r


def refine(pose16, verts, tris, depth_u16, prob_u16, K, depth_scale, **prm):
    """stocs_refine_poses_visible_damped for one pose -> dict: pose (the returned float32 pose Pa), record (the fields of
    stocs_refine_visible_damped_result; lambda is lambda_), trace (K + 1 rows: pose, cost, lambda, accepted, state; rows that were not
    evaluated are zero), steps (per evaluated row what next_trial gave, None behind the last), evs (the evaluations)"""
    Kit, base, d = split(prm)
    P = np.asarray(pose16, F).reshape(16).copy()
    zero_row = dict(pose=np.zeros(16, F), cost=0.0, lambda_=0.0, accepted=0, state=0)
    trace = [dict(zero_row, pose=np.zeros(16, F)) for _ in range(Kit + 1)]
    steps, evs = [None] * (Kit + 1), [None] * (Kit + 1)
    if not ref.pose_valid(P):
        return dict(pose=P, record=zero_record(), trace=trace, steps=steps, evs=evs)
    ev = ref.evaluate(P, verts, tris, depth_u16, prob_u16, K, depth_scale, **base)
    rec = ref.record_of(ev)
    Pa, Sa, rec_a = P.copy(), ev["sums"].copy(), rec
    Ca = cost_of(ev["sums"], rec["counted"], rec["too_far"], base["max_distance"])
    lam = d["lambda0"]
    its = rejected = frozen = 0
    evaluations = 1
    evs[0] = ev
    trace[0] = dict(pose=P.copy(), cost=Ca, lambda_=lam, accepted=1, state=TRACE_EVALUATED)
    if Kit > 0 and rec["counted"] < 6:
        frozen = 1
        trace[0]["state"] |= TRACE_FROZE
    for e in range(Kit):
        if frozen:
            break
        nt = next_trial(Pa, Sa, lam, d)
        steps[e] = nt
        if nt["T34"] is None:
            frozen = 1
            trace[e]["state"] |= TRACE_FROZE
            break
        Pt = ref.apply_update(Pa, nt["T34"])
        ev = ref.evaluate(Pt, verts, tris, depth_u16, prob_u16, K, depth_scale, **base)
        rec = ref.record_of(ev)
        C = cost_of(ev["sums"], rec["counted"], rec["too_far"], base["max_distance"])
        ok, lam = decide(C, Ca, lam, d)
        evaluations += 1
        evs[e + 1] = ev
        if ok:
            Pa, Sa, rec_a, Ca = Pt.copy(), ev["sums"].copy(), rec, C
            its += 1
        else:
            rejected += 1
        trace[e + 1] = dict(pose=Pt.copy(), cost=C, lambda_=lam, accepted=1 if ok else 0, state=TRACE_EVALUATED)
    with np.errstate(over="ignore"):
        record = dict(rec_a, iterations=its, frozen=frozen, evaluations=evaluations, rejected=rejected, cost=F(Ca), lambda_=F(lam))
    return dict(pose=Pa, record=record, trace=trace, steps=steps, evs=evs)


def add_error(pose16, gt16, points):
    """ADD: the mean distance between the points under the two poses, in float64"""
    v = np.asarray(points, np.float64).reshape(-1, 3)
    A = np.asarray(pose16, F).reshape(4, 4).T.astype(np.float64)
    B = np.asarray(gt16, F).reshape(4, 4).T.astype(np.float64)
    return float(np.linalg.norm((v @ A[:3, :3].T + A[:3, 3]) - (v @ B[:3, :3].T + B[:3, 3]), axis=1).mean())
