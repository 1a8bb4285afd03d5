"""float32 numpy restatement of the pose-error contract written at stocs_pose_errors in include/stocs_hip.h (steps 1-6 there), one operation
at a time so that every intermediate is rounded to float32 exactly where the contract rounds it, and a float64 brute force of the same
quantities to measure it against.  Written from the contract, not from the kernel; the GPU tests compare the library's records with the
restatement for equality.  No GPU, numpy only."""
import numpy as np

F = np.float32
DTYPE = np.dtype([("add_fix", np.uint64), ("adds_fix", np.uint64), ("add", np.float32), ("add_max", np.float32), ("adds", np.float32),
                  ("adds_max", np.float32), ("valid", np.int32), ("reserved", np.int32)])
USED = [i for i in range(15) if i % 4 != 3]   # the twelve R_ab, t_a of a column-major pose
ROWS = 256                                    # queries per block of the all-pairs walk (memory only; the result does not depend on it)


def transform(pose16, pts):
    """step 1 -> (M, 3) float32"""
    P = np.asarray(pose16, F).reshape(16)
    m = np.ascontiguousarray(pts, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        p = [(P[a] * m[:, 0] + (P[4 + a] * m[:, 1] + P[8 + a] * m[:, 2])) + P[12 + a] for a in range(3)]
    assert all(v.dtype == F for v in p)
    return np.stack(p, axis=1)


def sqdist(p, g):
    """step 2 for broadcastable (..., 3) float32 arrays"""
    with np.errstate(all="ignore"):
        d = p - g
        D = (d[..., 0] * d[..., 0]) + ((d[..., 1] * d[..., 1]) + (d[..., 2] * d[..., 2]))
    assert D.dtype == F
    return D


def root(D):
    """r(x): +inf for NaN, else the correctly rounded float32 square root"""
    with np.errstate(all="ignore"):
        r = np.sqrt(D)
    assert r.dtype == F
    return np.where(np.isnan(D), F(np.inf), r).astype(F)


def nearest(p, g):
    """min_j D(i, j) and the lowest j that attains it (-1: none) for every row of p; a NaN never wins"""
    n = len(p)
    best = np.full(n, np.inf, F)
    arg = np.full(n, -1, np.int32)
    for a in range(0, n, ROWS):
        D = sqdist(p[a:a + ROWS, None, :], g[None, :, :])
        D = np.where(np.isnan(D), F(np.inf), D)     # +inf is never `<` the start value either
        j = np.argmin(D, axis=1)                    # the first (lowest) index of the minimum
        v = D[np.arange(len(j)), j]
        best[a:a + ROWS] = v
        arg[a:a + ROWS] = np.where(v < F(np.inf), j, -1)
    return best, arg


def detail(est16, gt16, pts):
    """steps 1-3 of one pair -> (e, s, nn)"""
    p, g = transform(est16, pts), transform(gt16, pts)
    e = root(sqdist(p, g))
    best, nn = nearest(p, g)
    return e, root(best), nn


def fix(x):
    """q(x) of step 4 as Python-exact uint64"""
    with np.errstate(all="ignore"):
        v = np.minimum(np.asarray(x, F), F(32768.0)) * F(4294967296.0)
    assert v.dtype == F
    return np.floor(v.astype(np.float64)).astype(np.uint64)


def valid_pair(est16, gt16):
    P, G = np.asarray(est16, F).reshape(16), np.asarray(gt16, F).reshape(16)
    return bool(np.all(np.isfinite(P[USED])) and np.all(np.isfinite(G[USED])) and not np.all(P == 0))


def record(est16, gt16, pts):
    r = np.zeros((), DTYPE)
    if not valid_pair(est16, gt16):
        r["add"] = r["add_max"] = r["adds"] = r["adds_max"] = np.inf
        return r
    e, s, _ = detail(est16, gt16, pts)
    M = len(e)
    af, sf = int(fix(e).sum(dtype=np.uint64)), int(fix(s).sum(dtype=np.uint64))
    r["add_fix"], r["adds_fix"] = af, sf
    r["add"] = F(np.float64(af) / 4294967296.0 / np.float64(M))
    r["adds"] = F(np.float64(sf) / 4294967296.0 / np.float64(M))
    r["add_max"], r["adds_max"] = e.max(), s.max()
    r["valid"] = 1
    return r


def records(est, gt, pts):
    est, gt = np.asarray(est, F).reshape(-1, 16), np.asarray(gt, F).reshape(-1, 16)
    assert len(gt) in (1, len(est))
    return np.array([record(est[k], gt[0 if len(gt) == 1 else k], pts) for k in range(len(est))], DTYPE).reshape(len(est))


def diameter(pts):
    """step 6: max over i < j of r(D(i, j)), points untransformed; 0 for one point"""
    m = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n = len(m)
    best = F(0)
    for a in range(0, n, ROWS):
        D = sqdist(m[a:a + ROWS, None, :], m[None, :, :])
        i = np.arange(a, min(a + ROWS, n))[:, None]
        r = root(D)
        r = np.where(np.arange(n)[None, :] > i, r, F(0))
        best = max(best, F(r.max()))
    return F(best)


def records_equal(a, b):
    """bit equality of every field"""
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in DTYPE.names)


# ---- float64 brute force of the same quantities (no fixed point, no saturation) ----
def detail64(est16, gt16, pts):
    P, G = np.asarray(est16, np.float64).reshape(4, 4).T, np.asarray(gt16, np.float64).reshape(4, 4).T
    m = np.asarray(pts, np.float64).reshape(-1, 3)
    p, g = m @ P[:3, :3].T + P[:3, 3], m @ G[:3, :3].T + G[:3, 3]
    e = np.linalg.norm(p - g, axis=1)
    s = np.empty(len(m))
    for a in range(0, len(m), ROWS):
        s[a:a + ROWS] = np.sqrt(((p[a:a + ROWS, None, :] - g[None, :, :]) ** 2).sum(-1).min(1))
    return e, s


def diameter64(pts):
    m = np.asarray(pts, np.float64).reshape(-1, 3)
    best = 0.0
    for a in range(0, len(m), ROWS):
        best = max(best, float(np.sqrt(((m[a:a + ROWS, None, :] - m[None, :, :]) ** 2).sum(-1).max())))
    return best
