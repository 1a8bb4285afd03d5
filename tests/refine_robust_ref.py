"""Float64 restatement of the robust refinement (stocs_refine_poses_robust, csrc/refine_robust.h): the candidate rule (double distance
test and normal gate), the trim by (distance, source position) and the whole loop, on the float32 values the context holds.  numpy and
scipy only; no GPU.  What oracle/refine_oracle.py already gives (classes, sums, the one-iteration pose) is taken from there.

Ambiguity, with refine_oracle's margin 2^-20: a hypothesis is CLEAR at an iteration when no source point that can be matched has two
model points within a relative 2^-20 of each other at the minimum, no matched pair lies within a relative 2^-20 of the distance
threshold, no pair that passes the distance test has |c - min_cos| <= 2^-20, and the k-th and (k+1)-th distances of the trim differ by
more than a relative 2^-20.  The device forms its squared distance in float (relative error below 2^-22) and everything else in double:
where the restatement is clear, the device must choose the same pairs."""
import math

import numpy as np
from scipy.spatial import cKDTree

from oracle import refine_oracle as ro

F = np.float32
MARGIN = ro.MARGIN
GATE_BAND = 2.0 ** -20
NOT_CANDIDATE = 0xFFFFFFFF


def unit_normals(n):
    """normalized3 of the context, in float (oracle/refine_oracle.py Case.unit_normals)"""
    n = np.asarray(n, F)
    z = np.sqrt((n[:, 0] * n[:, 0] + (n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])).astype(F)).astype(F)
    return (n / z[:, None]).astype(F)


def min_cos_of_degrees(deg):
    """StocsEstimator.robust_params: the cosine in double, rounded to float once; None: gate off"""
    return None if deg is None else float(F(math.cos(float(deg) * math.pi / 180.0)))


def inv34(M):
    """csrc/refine.hip inv34: the 3x4 inverse by the adjugate, operation for operation, in double"""
    a, b, c, d, e, f, g, h, k = (float(M[0, 0]), float(M[0, 1]), float(M[0, 2]), float(M[1, 0]), float(M[1, 1]), float(M[1, 2]), float(M[2, 0]),
                                 float(M[2, 1]), float(M[2, 2]))
    A, B, Cc = e * k - f * h, f * g - d * k, d * h - e * g
    det = a * A + b * B + c * Cc
    if not (det != 0.0) or not math.isfinite(det):
        return None
    r = 1.0 / det
    I = np.zeros((3, 4))
    I[0, 0] = A * r; I[0, 1] = (c * h - b * k) * r; I[0, 2] = (b * f - c * e) * r
    I[1, 0] = B * r; I[1, 1] = (a * k - c * g) * r; I[1, 2] = (c * d - a * f) * r
    I[2, 0] = Cc * r; I[2, 1] = (b * g - a * h) * r; I[2, 2] = (a * e - b * d) * r
    for i in range(3):
        I[i, 3] = -(I[i, 0] * float(M[0, 3]) + I[i, 1] * float(M[1, 3]) + I[i, 2] * float(M[2, 3]))
    return I


def hyp_inverse(T16):
    """Tinv (3x4, double) of a column-major float hypothesis, as refine_init_kernel forms it; None: singular"""
    M = np.asarray(T16, F).reshape(4, 4).T[:3, :].astype(np.float64)
    return inv34(M)


def _affine(M, x):
    """M[:, :3] x + M[:, 3] per row, left to right, one operation at a time (x: (n, 3) float64) -> (n, 3)"""
    return np.stack([((M[r, 0] * x[:, 0] + M[r, 1] * x[:, 1]) + M[r, 2] * x[:, 2]) + M[r, 3] for r in range(3)], 1)


def _linear(M, x):
    return np.stack([(M[r, 0] * x[:, 0] + M[r, 1] * x[:, 1]) + M[r, 2] * x[:, 2] for r in range(3)], 1)


def source(Tinv, U, x):
    """-> (s double (n, 3), f float32 (n, 3)): float(Tinv x), then U in double, then its float image (what the walk searches with)"""
    s0 = _affine(Tinv, np.asarray(x, F).astype(np.float64)).astype(F)
    s = _affine(U, s0.astype(np.float64))
    return s, s.astype(F)


def gate_c(Tinv, U, ns, n):
    """c = (g.x n.x + g.y n.y) + g.z n.z with g = U_R (Tinv_R ns), in double, left to right"""
    g = _linear(U, _linear(Tinv, np.asarray(ns, F).astype(np.float64)))
    n = np.asarray(n, F).astype(np.float64)
    return (g[:, 0] * n[:, 0] + g[:, 1] * n[:, 1]) + g[:, 2] * n[:, 2]


def device_ratio(keep_ratio):
    """the keep ratio as the C ABI carries it: a float"""
    return float(F(keep_ratio))


def keep_count(keep_ratio, n_cand):
    """k = floor(keep_ratio n_cand) with the ratio AS GIVEN (a double): the device receives a float, so whoever restates the device
    passes device_ratio(r); the table of DESIGN.md 7.11's restatement was made with the double 0.7"""
    return int(math.floor(float(keep_ratio) * n_cand))


def kept_by_sort(rank, keep_ratio):
    """the k smallest by (rank word, position) of the words that are not NOT_CANDIDATE -> (kept uint8 mask, k, n_cand): integer sort"""
    rank = np.asarray(rank, np.uint32)
    cand = np.nonzero(rank != NOT_CANDIDATE)[0]
    k = keep_count(keep_ratio, len(cand))
    order = cand[np.argsort(rank[cand].astype(np.int64), kind="stable")]   # stable: the lower position first on equal words
    kept = np.zeros(len(rank), np.uint8)
    kept[order[:k]] = 1
    return kept, k, len(cand)


def ratio_for_k(k, n_cand):
    """a float keep_ratio in (0, 1] with floor(ratio n_cand) == k (1 <= k <= n_cand)"""
    r = F(1.0) if k == n_cand else F((k + 0.5) / n_cand)
    assert keep_count(r, n_cand) == k and 0.0 < float(r) <= 1.0, (k, n_cand, r)
    return float(r)


def evaluate(Tinv, U, scene_c, scene_n, model_c, model_n, dist, keep_ratio, min_cos, src_idx=None, tree=None):
    """one evaluation in float64 -> dict: s, f, match (-1 none), cand, kept, d2 (float64 squared distance of the float source to its
    match: what the rank word approximates), c, k, n_cand, clear"""
    idx = np.arange(len(scene_c)) if src_idx is None else np.asarray(src_idx, np.int64)
    s, f = source(Tinv, U, scene_c[idx])
    m64 = np.asarray(model_c, F).astype(np.float64)
    tree = tree or cKDTree(m64)
    kk = min(2, len(m64))
    d, j = tree.query(f.astype(np.float64), k=kk)
    if kk == 1:
        d = np.stack([d, np.full(len(d), np.inf)], 1); j = np.stack([j, j], 1)
    j1 = j[:, 0]
    t = m64[j1]
    dq = ((f.astype(np.float64) - t) ** 2).sum(1)                      # the walk's distance, exact
    d2nd = ((f.astype(np.float64) - m64[j[:, 1]]) ** 2).sum(1) if kk == 2 else np.full(len(f), np.inf)
    dd = s - t
    dth = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]   # the double threshold test's
    D2 = float(F(dist)) ** 2
    near = dth <= D2
    clear = True
    reach = dq <= D2 * (1.0 + 4 * MARGIN)
    if (reach & (d2nd <= dq * (1.0 + MARGIN))).any():
        clear = False                                                  # a second model point as near: the match may differ
    if (np.abs(dth - D2) <= D2 * MARGIN).any():
        clear = False
    c = np.full(len(f), np.nan)
    cand = near.copy()
    if min_cos is not None:
        c = gate_c(Tinv, U, np.asarray(scene_n, F)[idx], np.asarray(model_n, F)[j1])
        if (near & (np.abs(c - float(F(min_cos))) <= GATE_BAND)).any():
            clear = False
        cand = near & (c >= float(F(min_cos)))
    ci = np.nonzero(cand)[0]
    k = keep_count(keep_ratio, len(ci))
    order = ci[np.argsort(dq[ci], kind="stable")]
    kept = np.zeros(len(f), bool)
    kept[order[:k]] = True
    if 0 < k < len(ci):
        a, b = dq[order[k - 1]], dq[order[k]]
        if b <= a * (1.0 + MARGIN):
            clear = False
    match = np.where(dq <= D2 * (1.0 + 1e-5), j1, -1)
    return dict(s=s, f=f, match=match, j=j1, cand=cand, kept=kept, d2=dq, c=c, k=k, n_cand=len(ci), clear=clear)


def _update(x):
    ca, sa, cb, sb, cg, sg = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    N = np.zeros((3, 4))
    N[:, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa], [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa], [-sb, cb * sa, cb * ca]]
    N[:, 3] = x[3:]
    return N


def robust_loop(T16, scene_c, scene_n, model_c, model_n, iters, dist, keep_ratio=1.0, min_cos=None, src_idx=None, tree=None):
    """the whole loop for one hypothesis -> dict: T (4x4 float64, T U^-1), k, n_cand (of the last evaluated iteration), iterations,
    clear (at every evaluated iteration)"""
    T = np.asarray(T16, F).reshape(4, 4).T.astype(np.float64)
    Tinv = hyp_inverse(T16)
    out = dict(T=T, k=0, n_cand=0, iterations=0, clear=True)
    if Tinv is None:
        return out
    m64 = np.asarray(model_c, F).astype(np.float64)
    n64 = np.asarray(model_n, F).astype(np.float64)
    tree = tree or cKDTree(m64)
    U = np.eye(4)[:3, :]
    for _ in range(iters):
        e = evaluate(Tinv, U, scene_c, scene_n, model_c, model_n, dist, keep_ratio, min_cos, src_idx, tree)
        out["k"], out["n_cand"] = e["k"], e["n_cand"]
        out["clear"] = out["clear"] and e["clear"]
        if e["k"] < 6:
            break
        s, t, n = e["s"][e["kept"]], m64[e["j"][e["kept"]]], n64[e["j"][e["kept"]]]
        A = np.concatenate([np.cross(s, n), n], axis=1)
        b = ((t - s) * n).sum(1)
        x = ro._solve(A.T @ A, A.T @ b)
        N = _update(x)
        U4 = np.eye(4); U4[:3, :] = U
        N4 = np.eye(4); N4[:3, :] = N
        U = (N4 @ U4)[:3, :]
        out["iterations"] += 1
    if out["iterations"]:
        Ui = np.eye(4); Ui[:3, :] = inv34(U)
        out["T"] = T @ Ui
    return out


def add_error(T_est, T_gt, model_c):
    """ADD in the centred frames: the mean distance between the model points under the two poses (metres)"""
    m = np.asarray(model_c, F).astype(np.float64)
    a = m @ np.asarray(T_est)[:3, :3].T + np.asarray(T_est)[:3, 3]
    b = m @ np.asarray(T_gt)[:3, :3].T + np.asarray(T_gt)[:3, 3]
    return float(np.linalg.norm(a - b, axis=1).mean())
