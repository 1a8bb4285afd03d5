"""Float32 numpy restatement of stocs_segment_frame (include/stocs_hip.h, steps 1-7): every integer and every image bit for bit.  Each
float step is one IEEE float32 operation, 3-term sums are e0 + (e1 + e2), a comparison with NaN is false.  Steps 4-7 take the plane as
input, so a test re-synchronises on the library's float plane; fit64 is the float64 fit the plane is judged against."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

M64 = (1 << 64) - 1
F = np.float32

DEFAULTS = dict(max_depth=2.0, plane_hypotheses=1024, score_stride=4, plane_tolerance=0.01, plane_min_share=0.15, max_height=0.5, jump_abs=0.005,
                jump_rel=0.01, min_pixels=200, seed=1)


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        assert k in p, k
    p.update(kw)
    return p


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def rng64(seed, attempt, k):
    z = mix64((seed + 0x9E3779B97F4A7C15) & M64)
    z = mix64(z ^ ((attempt * 0xD1B54A32D192ED03 + 0x8CB92BA72F3D8DD7) & M64))
    return mix64(z ^ (((k + 1) * 0xDB4F0B9175AE2165) & M64))


def draws(seed, h, npix):
    return [(((rng64(seed, h, k) >> 32) * npix) >> 32) for k in range(3)]


def points(depth_u16, K, depth_scale, max_depth):
    """step 1: (H, W, 3) float32 points and the valid mask"""
    fx, cx, fy, cy = (F(v) for v in K)
    raw = np.asarray(depth_u16, np.uint16)
    H, W = raw.shape
    z = raw.astype(F) * F(depth_scale)
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    zd = z.astype(np.float64)
    P = np.stack([((jj - np.float64(cx)) * zd / np.float64(fx)).astype(F), ((ii - np.float64(cy)) * zd / np.float64(fy)).astype(F), z], axis=-1)
    return P, (raw != 0) & (z <= F(max_depth))


def hypothesis(P, valid, seed, h, tol):
    """step 2 for one hypothesis: (A, m, tol^2 mm, alive, the three indices)"""
    Pf, vf = P.reshape(-1, 3), valid.reshape(-1)
    ix = draws(seed, h, Pf.shape[0])
    A, B, Cc = Pf[ix[0]], Pf[ix[1]], Pf[ix[2]]
    e1, e2 = B - A, Cc - A
    m = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], F)
    with np.errstate(all="ignore"):
        mm = F(m[0] * m[0]) + F(F(m[1] * m[1]) + F(m[2] * m[2]))
        t2 = F(F(tol) * F(tol)) * mm
    alive = bool(vf[ix[0]] and vf[ix[1]] and vf[ix[2]] and len(set(ix)) == 3 and mm > 0 and np.isfinite(mm))
    return A.copy(), m, F(t2), alive, ix


def inliers(X, A, m, t2):
    """s = m0 dx + (m1 dy + m2 dz), s s <= tol^2 mm; X: (..., 3) float32"""
    with np.errstate(all="ignore"):
        d = X - A
        s = m[0] * d[..., 0] + (m[1] * d[..., 1] + m[2] * d[..., 2])
        return s * s <= t2


def plane_search(P, valid, p):
    """steps 2-3 up to the moments: dict(plane_found, winner, winner_count, n_scored, counts, moments (10 python ints), inlier mask)"""
    H, W = valid.shape
    s = p["score_stride"]
    lat = np.zeros((H, W), bool); lat[::s, ::s] = True
    scored = P[lat & valid]
    out = dict(plane_found=0, winner=-1, winner_count=0, n_scored=int(scored.shape[0]), moments=[0] * 10, hyp=None, inl=np.zeros((H, W), bool), counts=[])
    best = 0
    hyps = {}
    for h in range(p["plane_hypotheses"]):
        A, m, t2, alive, _ = hypothesis(P, valid, p["seed"], h, p["plane_tolerance"])
        c = int(inliers(scored, A, m, t2).sum()) if alive else 0
        out["counts"].append(c)
        if alive and c > 0:
            key = (c << 32) | (0xFFFFFFFF - h)
            if key > best:
                best = key; hyps = {h: (A, m, t2)}
    if not best:
        return out
    h = 0xFFFFFFFF - (best & 0xFFFFFFFF)
    out["winner"], out["winner_count"], out["hyp"] = h, best >> 32, hyps[h]
    if float(out["winner_count"]) < float(np.float64(F(p["plane_min_share"])) * np.float64(out["n_scored"])):
        return out
    out["plane_found"] = 1
    A, m, t2 = hyps[h]
    with np.errstate(all="ignore"):
        inl = valid & inliers(P, A, m, t2) & (np.abs(P) < F(16)).all(axis=-1)
    out["inl"] = inl
    q = np.rint(P[inl].astype(np.float64) * 65536.0).astype(np.int64)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    out["moments"] = [int(q.shape[0])] + [int(v.sum()) for v in (x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)]
    return out


def orient(n, d):
    return (-n, -d) if d < 0 else (n, d)


def fit64(points64):
    """the float64 least-squares plane of unquantised points: (unit normal, d), d >= 0"""
    c = points64.mean(axis=0)
    _, _, vt = np.linalg.svd(points64 - c, full_matrices=False)
    n = vt[2] / np.linalg.norm(vt[2])
    return orient(n, -float(n @ c))


def plane_from_moments(M):
    """the plane of the ten integer moments in float64 (numpy's eigh; the library iterates Jacobi sweeps): (normal, d)"""
    n = float(M[0]); u = 1.0 / 65536.0
    c = np.array([M[1], M[2], M[3]], np.float64) / n * u
    S = np.array([[M[4], M[5], M[6]], [M[5], M[7], M[8]], [M[6], M[8], M[9]]], np.float64) / n * (u * u) - np.outer(c, c)
    w, v = np.linalg.eigh(S)
    nv = v[:, 0] / np.linalg.norm(v[:, 0])
    return orient(nv, -float(nv @ c))


def components(fg, z, jump_abs, jump_rel):
    """step 5: the root image (lowest linear index of the pixel's component, -1 off the foreground)"""
    H, W = fg.shape
    idx = np.arange(H * W).reshape(H, W)
    ja, jr = F(jump_abs), F(jump_rel)

    def join(a, b, fa, fb):
        with np.errstate(all="ignore"):
            return fa & fb & (np.abs(a - b) <= ja + jr * np.minimum(a, b))
    jh = join(z[:, 1:], z[:, :-1], fg[:, 1:], fg[:, :-1])
    jv = join(z[1:, :], z[:-1, :], fg[1:, :], fg[:-1, :])
    a = np.concatenate([idx[:, 1:][jh], idx[1:, :][jv]]); b = np.concatenate([idx[:, :-1][jh], idx[:-1, :][jv]])
    _, comp = connected_components(coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(H * W, H * W)), directed=False)
    low = np.full(comp.max() + 1, H * W, np.int64)
    np.minimum.at(low, comp, idx.reshape(-1))
    root = low[comp].reshape(H, W)
    root[~fg] = -1
    return root


def classify(P, valid, plane, p):
    """step 4: dict(on, above, below, fg) masks; plane None: no plane"""
    if plane is None:
        zero = np.zeros(valid.shape, bool)
        return dict(on=zero, above=zero, below=zero, fg=valid.copy())
    n0, n1, n2, d = (F(v) for v in plane)
    tol, mh = F(p["plane_tolerance"]), F(p["max_height"])
    with np.errstate(all="ignore"):
        h = (n0 * P[..., 0] + (n1 * P[..., 1] + n2 * P[..., 2])) + d
        on, above, below = valid & (np.abs(h) <= tol), valid & (h > tol), valid & (h < -tol)
        return dict(on=on, above=above, below=below, fg=above & (h <= mh))


def edge_image(labels):
    H, W = labels.shape
    e = labels != 0
    e[:, 1:] &= labels[:, 1:] == labels[:, :-1]; e[:, :-1] &= labels[:, :-1] == labels[:, 1:]
    e[1:, :] &= labels[1:, :] == labels[:-1, :]; e[:-1, :] &= labels[:-1, :] == labels[1:, :]
    return np.where(e, 255, 0).astype(np.uint8)


def segments(P, valid, plane, p):
    """steps 4-7 on a given float plane (None: none): counts, images, records"""
    cl = classify(P, valid, plane, p)
    z = P[..., 2]
    root = components(cl["fg"], z, p["jump_abs"], p["jump_rel"])
    H, W = valid.shape
    flat = root.reshape(-1)
    roots, size = np.unique(flat[flat >= 0], return_counts=True)
    kept = roots[size >= p["min_pixels"]]
    number = np.zeros(H * W + 1, np.int32)
    number[kept] = np.arange(1, kept.size + 1)
    labels = np.where(root >= 0, number[np.maximum(root, 0)], 0).astype(np.int32)
    records = []
    for k, (r, n) in enumerate(zip(kept.tolist(), size[size >= p["min_pixels"]].tolist())):
        ii, jj = np.nonzero(labels == k + 1)
        zz = z[ii, jj]
        records.append((r, n, int(jj.min()), int(ii.min()), int(jj.max()), int(ii.max()), F(zz.min()), F(zz.max())))
    return dict(n_on_plane=int(cl["on"].sum()), n_above=int(cl["above"].sum()), n_below=int(cl["below"].sum()), n_components=int(roots.size),
                n_segments=int(kept.size), labels=labels, class_prob=np.where(labels != 0, 10000, 0).astype(np.uint16), edge=edge_image(labels),
                records=records, root=root, fg=cl["fg"])


def segment_frame(depth_u16, K, depth_scale, plane=None, **kw):
    """The whole call.  plane: the library's float plane to run steps 4-7 on; None: the restatement's own float64 plane of the moments
    cast to float32 (equal to the library's up to the rounding of its Jacobi iteration)."""
    p = params(**kw)
    P, valid = points(depth_u16, K, depth_scale, p["max_depth"])
    s = plane_search(P, valid, p)
    used = None
    if s["plane_found"]:
        if plane is None:
            if s["moments"][0] >= 3:
                n, d = plane_from_moments(s["moments"])
            else:
                A, m, _ = s["hyp"]
                n = m.astype(np.float64) / np.linalg.norm(m.astype(np.float64)); n, d = orient(n, -float(n @ A.astype(np.float64)))
            plane = np.array([n[0], n[1], n[2], d], F)
        used = np.asarray(plane, F)
    out = segments(P, valid, used, p)
    out.update(plane_found=s["plane_found"], winner=s["winner"], winner_count=s["winner_count"], n_valid=int(valid.sum()), n_scored=s["n_scored"],
               n_refit=s["moments"][0] if s["plane_found"] else 0, moments=s["moments"], plane=used if used is not None else np.zeros(4, F), inl=s["inl"],
               P=P, valid=valid, counts=s["counts"])
    return out
