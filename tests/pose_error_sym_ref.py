"""float32 numpy restatement of the symmetry-aware pose-error contract written at stocs_pose_errors_sym in include/stocs_hip.h (steps 0-6
there), on top of the plain restatement's transform / sqdist / root / fix (tests/pose_error_ref.py), one operation at a time so that every
intermediate is rounded to float32 exactly where the contract rounds it; and a float64 brute force of the same quantities to measure it
against.  Written from the contract, not from the kernel; the GPU tests compare the library's records with the restatement for equality.
No GPU, numpy only.  A camera is the four intrinsics (fx, cx, fy, cy), the order of stocs_camera."""
import numpy as np

import pose_error_ref as base

F = np.float32
DTYPE = np.dtype([("add_fix", np.uint64), ("add", np.float32), ("mssd", np.float32), ("mspd", np.float32), ("reserved_f", np.float32),
                  ("k_add", np.int32), ("k_mssd", np.int32), ("k_mspd", np.int32), ("valid", np.int32)])
INF = F(np.inf)
IDENTITY = np.eye(4, dtype=F).reshape(16)


def compose(gt16, sym16):
    """step 0 -> the composed pose (C, u) as 16 floats, column-major"""
    G, S = np.asarray(gt16, F).reshape(16), np.asarray(sym16, F).reshape(16)
    C = np.zeros(16, F); C[15] = 1
    with np.errstate(all="ignore"):
        for a in range(3):
            for b in range(3):
                C[4 * b + a] = G[a] * S[4 * b] + (G[4 + a] * S[4 * b + 1] + G[8 + a] * S[4 * b + 2])
            C[12 + a] = (G[a] * S[12] + (G[4 + a] * S[13] + G[8 + a] * S[14])) + G[12 + a]
    return C


def project(cam, x):
    """step 4's a, b for (M, 3) float32 points"""
    fx, cx, fy, cy = [F(v) for v in cam]
    with np.errstate(all="ignore"):
        a = (fx * x[:, 0]) / x[:, 2] + cx
        b = (fy * x[:, 1]) / x[:, 2] + cy
    assert a.dtype == F and b.dtype == F
    return a, b


def per_symmetry(est16, gt16, syms, pts, cam=None):
    """steps 0-4 of one pair -> (add_fix (K,) uint64, max3 (K,) float32, max2 (K,) float32); what stocs_pose_errors_sym_detail returns"""
    syms = np.asarray(syms, F).reshape(-1, 16)
    K = len(syms)
    p = base.transform(est16, pts)
    add_fix, max3, max2 = np.zeros(K, np.uint64), np.zeros(K, F), np.full(K, INF, F)
    if cam is not None:
        pa, pb = project(cam, p)
    for k in range(K):
        g = base.transform(compose(gt16, syms[k]), pts)
        e = base.root(base.sqdist(p, g))
        add_fix[k] = base.fix(e).sum(dtype=np.uint64)
        max3[k] = e.max()
        if cam is not None:
            ga, gb = project(cam, g)
            with np.errstate(all="ignore"):
                da, db = pa - ga, pb - gb
                P = (da * da) + (db * db)
            bad = ~(p[:, 2] > F(1e-6)) | ~(g[:, 2] > F(1e-6)) | np.isnan(P)
            P = np.where(bad, INF, P).astype(F)
            max2[k] = base.root(P.max()[None])[0]
    return add_fix, max3, max2


def _first_min(v, inf):
    """index-ordered minimum starting at `inf`, replaced only on `<` -> (value, lowest k that attains it or -1)"""
    best, arg = inf, -1
    for k in range(len(v)):
        if v[k] < best:
            best, arg = v[k], k
    return best, arg


def record(est16, gt16, syms, pts, cam=None):
    r = np.zeros((), DTYPE)
    if not base.valid_pair(est16, gt16):
        r["add"] = r["mssd"] = r["mspd"] = np.inf
        r["k_add"] = r["k_mssd"] = r["k_mspd"] = -1
        return r
    add_fix, max3, max2 = per_symmetry(est16, gt16, syms, pts, cam)
    M = len(np.asarray(pts).reshape(-1, 3))
    af, r["k_add"] = _first_min([int(x) for x in add_fix], 1 << 64)
    r["add_fix"] = af
    r["add"] = F(np.float64(af) / 4294967296.0 / np.float64(M))
    r["mssd"], r["k_mssd"] = _first_min(max3, INF)
    r["mspd"], r["k_mspd"] = _first_min(max2, INF)
    r["valid"] = 1
    return r


def records(est, gt, syms, pts, cam=None):
    est, gt = np.asarray(est, F).reshape(-1, 16), np.asarray(gt, F).reshape(-1, 16)
    assert len(gt) in (1, len(est))
    return np.array([record(est[k], gt[0 if len(gt) == 1 else k], syms, pts, cam) for k in range(len(est))], DTYPE).reshape(len(est))


def records_equal(a, b):
    """bit equality of every field"""
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in DTYPE.names)


# ---- float64 brute force of the same quantities (no fixed point, no saturation) ----
def _mat64(p16):
    return np.asarray(p16, np.float64).reshape(4, 4).T


def per_symmetry64(est16, gt16, syms, pts, cam=None):
    """-> (e (K, M) distances, q (K, M) projected distances or None)"""
    P, G = _mat64(est16), _mat64(gt16)
    m = np.asarray(pts, np.float64).reshape(-1, 3)
    p = m @ P[:3, :3].T + P[:3, 3]
    e, q = [], []
    for S in np.asarray(syms, np.float64).reshape(-1, 16):
        Cm = G @ _mat64(S)
        g = m @ Cm[:3, :3].T + Cm[:3, 3]
        e.append(np.linalg.norm(p - g, axis=1))
        if cam is not None:
            fx, cx, fy, cy = [float(F(v)) for v in cam]
            q.append(np.hypot((fx * p[:, 0] / p[:, 2] + cx) - (fx * g[:, 0] / g[:, 2] + cx), (fy * p[:, 1] / p[:, 2] + cy) - (fy * g[:, 1] / g[:, 2] + cy)))
    return np.array(e), (np.array(q) if cam is not None else None)


def measures64(est16, gt16, syms, pts, cam=None):
    """-> dict(mssd, k_mssd, add, k_add, mspd, k_mspd) in float64 (mspd None without a camera)"""
    e, q = per_symmetry64(est16, gt16, syms, pts, cam)
    out = dict(mssd=float(e.max(1).min()), k_mssd=int(e.max(1).argmin()), add=float(e.mean(1).min()), k_add=int(e.mean(1).argmin()), mspd=None, k_mspd=-1)
    if q is not None:
        out.update(mspd=float(q.max(1).min()), k_mspd=int(q.max(1).argmin()))
    return out
