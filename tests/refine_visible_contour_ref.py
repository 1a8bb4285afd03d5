"""numpy restatement of the contour term of the visible-surface refinement, the contract written at stocs_refine_poses_visible_contour in
include/stocs_hip.h, on the plain and the damped restatements (refine_visible_ref.evaluate, refine_visible_damped_ref.next_trial, decide):
the frame's object pixels, the pose's rectangle grown by R, the nearest silhouette pixel of every uncovered object pixel under the
(d2, linear index) minimum, the gate in float32 one operation at a time, the three rows per pulled pixel and the 29 contour sums in
float64, the totals, the cost and the loop over K + 1 evaluations.  Written from the contract, not from the kernels.  No GPU, numpy only."""
import numpy as np

import mesh_ref
import refine_visible_damped_ref as dref
import refine_visible_ref as ref
import vsd_ref

F = np.float32
NOT_WALKED, UNREACHED, BEYOND, PULLED = range(4)
CONTOUR_DEFAULTS = dict(contour_weight=1.0, pull_radius_px=16, pull_distance=0.03)
CONTOUR_FIELDS = ("object_px", "uncovered", "unreached", "beyond", "pulled", "pull_rms")


def split(prm):
    """parameters -> (K, the plain gates, the damped parameters, the contour ones: w as the double of the float, R, pull_distance)"""
    c = dict(CONTOUR_DEFAULTS)
    rest = {}
    for k, v in prm.items():
        if k in c:
            c[k] = v
        else:
            rest[k] = v
    K, base, d = dref.split(rest)
    return K, base, d, dict(w=float(F(c["contour_weight"])), R=int(c["pull_radius_px"]), pull_distance=c["pull_distance"])


def object_mask(depth_u16, prob_u16, class_threshold):
    """O: raw != 0 and cp >= class_threshold, (H, W) bool"""
    raw = np.ascontiguousarray(depth_u16, np.uint16)
    cp = (np.ascontiguousarray(prob_u16, np.uint16).astype(np.float64) * (1.0 / 10000)).astype(F)
    return (raw != 0) & (cp >= F(class_threshold))


def rectangle(pose16, verts, tris, K, W, H):
    """the pose's rectangle (r0, r1, c0, c1): the union of its live triangles' clamped boxes; None when nothing is rendered"""
    if not vsd_ref.pose_finite(pose16) or len(np.asarray(tris).reshape(-1, 3)) == 0:
        return None
    g = mesh_ref.setup(pose16, verts, tris, K, W, H)
    live = np.flatnonzero(g["live"])
    if len(live) == 0:
        return None
    return int(g["r_lo"][live].min()), int(g["r_hi"][live].max()), int(g["c_lo"][live].min()), int(g["c_hi"][live].max())


def grown(rect, R, W, H):
    r0, r1, c0, c1 = rect
    return max(r0 - R, 0), min(r1 + R, H - 1), max(c0 - R, 0), min(c1 + R, W - 1)


def nearest_map(present, wanted, R):
    """present, wanted: (H, W) bool -> (H * W) int64: for every wanted pixel the linear index of the present pixel with the minimum of
    (d2, index) inside its (2 R + 1)^2 window, -1 where there is none or the pixel is not wanted"""
    H, W = present.shape
    out = np.full(H * W, -1, np.int64)
    rs, cs = np.nonzero(present)
    if len(rs) == 0:
        return out
    idx = rs.astype(np.int64) * W + cs
    for r, c in zip(*np.nonzero(wanted)):
        dr, dc = rs - r, cs - c
        m = (np.abs(dr) <= R) & (np.abs(dc) <= R)
        if m.any():
            key = (dr[m] * dr[m] + dc[m] * dc[m]).astype(np.int64) * (H * W) + idx[m]     # index < H W: the order of (d2, index)
            out[r * W + c] = idx[m][int(np.argmin(key))]
    return out


def rows_of(p, e):
    """the three rows of one pulled pixel from float32 p and e = q - p, in float64: A (3, 6) = [p x u_k, u_k], b (3,) = e"""
    px, py, pz = (np.float64(x) for x in p)
    A = np.array([[0.0, pz, -py, 1.0, 0.0, 0.0], [-pz, 0.0, px, 0.0, 1.0, 0.0], [py, -px, 0.0, 0.0, 0.0, 1.0]])
    return A, np.array([np.float64(x) for x in e])


def sums_of(A, b, pulled, dtype=np.float64):
    """the 29 contour sums of the stacked rows and the sums of the products' magnitudes: [27] counts pixels, not rows"""
    A, b = A.astype(dtype), b.astype(dtype)
    sums, mag = np.zeros(29, dtype), np.zeros(29, dtype)
    j = 0
    for i0 in range(6):
        for i1 in range(i0, 6):
            sums[j] = (A[:, i0] * A[:, i1]).sum(); mag[j] = np.abs(A[:, i0] * A[:, i1]).sum(); j += 1
    for i0 in range(6):
        sums[21 + i0] = (A[:, i0] * b).sum(); mag[21 + i0] = np.abs(A[:, i0] * b).sum()
    sums[27] = mag[27] = pulled
    sums[28] = mag[28] = (b * b).sum()
    return sums, mag


def contour_pass(keys, rect, depth_u16, prob_u16, K, depth_scale, class_threshold=0.10, pull_radius_px=16, pull_distance=0.03, **_):
    """the contour pass on the keys of one render whose rectangle is rect -> dict: state, nearest (H * W), sums, mag (29), A (3 pulled x 6),
    b, object_px, unreached, beyond, pulled"""
    depth = np.ascontiguousarray(depth_u16, np.uint16)
    H, W = depth.shape
    R = int(pull_radius_px)
    O = object_mask(depth, prob_u16, class_threshold)
    state = np.zeros(H * W, np.uint8)
    nearest = np.full(H * W, -1, np.int64)
    A, b = np.zeros((0, 6)), np.zeros(0)
    if rect is not None:
        present = (np.asarray(keys, np.uint64) != ref.EMPTY_KEY).reshape(H, W)
        er0, er1, ec0, ec1 = grown(rect, R, W, H)
        wanted = np.zeros((H, W), bool)
        wanted[er0: er1 + 1, ec0: ec1 + 1] = True
        wanted &= O & ~present
        nearest = nearest_map(present, wanted, R)
        state[wanted.reshape(-1)] = UNREACHED
        u = np.flatnonzero(nearest >= 0)
        fx, cx, fy, cy = (F(x) for x in K)
        s = nearest[u]
        with np.errstate(all="ignore"):
            z = (np.asarray(keys, np.uint64)[s] >> np.uint64(32)).astype(np.uint32).view(F)
            xs, ys = ((s % W).astype(F) - cx) / fx, ((s // W).astype(F) - cy) / fy
            xu, yu = ((u % W).astype(F) - cx) / fx, ((u // W).astype(F) - cy) / fy
            d = depth.reshape(-1)[u].astype(F) * F(depth_scale)
            p = [xs * z, ys * z, z]
            q = [xu * d, yu * d, d]
            e = [q[k] - p[k] for k in range(3)]
            D = e[0] * e[0] + (e[1] * e[1] + e[2] * e[2])
            assert all(x.dtype == F for x in (D, d, z) + tuple(p) + tuple(e))
            far = D > F(pull_distance) * F(pull_distance)
        state[u[far]] = BEYOND
        state[u[~far]] = PULLED
        rows = [rows_of([p[0][i], p[1][i], p[2][i]], [e[0][i], e[1][i], e[2][i]]) for i in np.flatnonzero(~far)]
        if rows:
            A, b = np.concatenate([x[0] for x in rows]), np.concatenate([x[1] for x in rows])
    pulled = int((state == PULLED).sum())
    sums, mag = sums_of(A, b, pulled)
    return dict(state=state, nearest=nearest, sums=sums, mag=mag, A=A, b=b, object_px=int(O.sum()), unreached=int((state == UNREACHED).sum()),
                beyond=int((state == BEYOND).sum()), pulled=pulled)


def evaluate(pose16, verts, tris, depth_u16, prob_u16, K, depth_scale, base, con):
    """one evaluation of the contour contract: the plain evaluation and the contour pass on its keys (not run when w == 0) ->
    (plain evaluation, contour pass or None)"""
    ev = ref.evaluate(pose16, verts, tris, depth_u16, prob_u16, K, depth_scale, **base)
    if con["w"] == 0:
        return ev, None
    H, W = np.asarray(depth_u16).shape
    cp = contour_pass(ev["keys"], rectangle(pose16, verts, tris, K, W, H), depth_u16, prob_u16, K, depth_scale, class_threshold=base["class_threshold"],
                      pull_radius_px=con["R"], pull_distance=con["pull_distance"])
    return ev, cp


def sums_bound(cp):
    """the bound on a double sum of 3 pulled products: (3 pulled + 8) 2^-53 sum |products|"""
    return (3 * cp["pulled"] + 8) * 2.0 ** -53 * cp["mag"]


def totals(S, Sc, w, dtype=np.float64):
    """M and v as 27 sums: S + w Sc entry by entry; [27] and [28] are S's"""
    out = np.asarray(S, dtype).copy()
    if Sc is not None:
        out[:27] = np.asarray(S, dtype)[:27] + dtype(w) * np.asarray(Sc, dtype)[:27]
    return out


def tally(ev, cp, n_object):
    """the counts of an evaluation: the plain record's and uncovered, unreached, beyond, pulled, pull_rms"""
    r = ref.record_of(ev)
    r["object_px"] = n_object
    r["uncovered"] = n_object - (r["too_far"] + r["grazing"] + r["counted"])
    for k in ("unreached", "beyond", "pulled"):
        r[k] = cp[k] if cp is not None else 0
    r["pull_rms"] = F(np.sqrt(F(cp["sums"][28] / r["pulled"]))) if r["pulled"] else F(0)
    return r


def cost_of(S28, Sc28, r, max_distance, pull_distance, w):
    """C = ((S[28] + max_d2 too_far) + w (Sc[28] + pull_d2 (uncovered - pulled))) / ((counted + too_far) + w uncovered); +inf when
    counted + 3 pulled < 6"""
    if r["counted"] + 3 * r["pulled"] < 6:
        return np.inf
    md2 = np.float64(F(max_distance) * F(max_distance))
    pd2 = np.float64(F(pull_distance) * F(pull_distance))
    num = (np.float64(S28) + md2 * np.float64(r["too_far"])) + np.float64(w) * (np.float64(Sc28) + pd2 * np.float64(r["uncovered"] - r["pulled"]))
    return float(num / (np.float64(r["counted"] + r["too_far"]) + np.float64(w) * np.float64(r["uncovered"])))


def cost_bound(ev, cp, r, w):
    """the rounding bound of a cost: the bounds of S[28] and of w Sc[28] over the divisor"""
    den = (r["counted"] + r["too_far"]) + w * r["uncovered"]
    b = ref.sums_bound(ev)[28] + (w * sums_bound(cp)[28] if cp is not None else 0.0)
    return float(b / den) if den > 0 else 0.0


def zero_record():
    r = dref.zero_record()
    r.update(dict((k, F(0) if k == "pull_rms" else 0) for k in CONTOUR_FIELDS))
    return r


def refine(pose16, verts, tris, depth_u16, prob_u16, K, depth_scale, **prm):
    """stocs_refine_poses_visible_contour for one pose -> dict: pose, record (the fields of stocs_refine_visible_contour_result; lambda is
    lambda_), trace (K + 1 rows as refine_visible_damped_ref.refine's), evs (per evaluated row (plain evaluation, contour pass))"""
    Kit, base, d, con = split(prm)
    if prob_u16 is None:
        raise ValueError("the contour term needs a class image")
    w = con["w"]
    P = np.asarray(pose16, F).reshape(16).copy()
    trace = [dict(pose=np.zeros(16, F), cost=0.0, lambda_=0.0, accepted=0, state=0) for _ in range(Kit + 1)]
    evs = [None] * (Kit + 1)
    if not ref.pose_valid(P):
        return dict(pose=P, record=zero_record(), trace=trace, evs=evs)
    n_object = int(object_mask(depth_u16, prob_u16, base["class_threshold"]).sum())
    args = (verts, tris, depth_u16, prob_u16, K, depth_scale, base, con)

    def measured(pose):
        ev, cp = evaluate(pose, *args)
        r = tally(ev, cp, n_object)
        return ev, cp, r, cost_of(ev["sums"][28], cp["sums"][28] if cp is not None else 0.0, r, base["max_distance"], con["pull_distance"], w)

    ev, cp, rec_a, Ca = measured(P)
    Pa, Sa = P.copy(), totals(ev["sums"], cp["sums"] if cp is not None else None, w)
    lam = d["lambda0"]
    its = rejected = frozen = 0
    evaluations = 1
    evs[0] = (ev, cp)
    trace[0] = dict(pose=P.copy(), cost=Ca, lambda_=lam, accepted=1, state=dref.TRACE_EVALUATED)
    if Kit > 0 and rec_a["counted"] + 3 * rec_a["pulled"] < 6:
        frozen = 1
        trace[0]["state"] |= dref.TRACE_FROZE
    for e in range(Kit):
        if frozen:
            break
        nt = dref.next_trial(Pa, Sa, lam, d)
        if nt["T34"] is None:
            frozen = 1
            trace[e]["state"] |= dref.TRACE_FROZE
            break
        Pt = ref.apply_update(Pa, nt["T34"])
        ev, cp, r, C = measured(Pt)
        ok, lam = dref.decide(C, Ca, lam, d)
        evaluations += 1
        evs[e + 1] = (ev, cp)
        if ok:
            Pa, Sa, rec_a, Ca = Pt.copy(), totals(ev["sums"], cp["sums"] if cp is not None else None, w), r, C
            its += 1
        else:
            rejected += 1
        trace[e + 1] = dict(pose=Pt.copy(), cost=C, lambda_=lam, accepted=1 if ok else 0, state=dref.TRACE_EVALUATED)
    with np.errstate(over="ignore"):
        record = dict(rec_a, iterations=its, frozen=frozen, evaluations=evaluations, rejected=rejected, cost=F(Ca), lambda_=F(lam))
    return dict(pose=Pa, record=record, trace=trace, evs=evs)
