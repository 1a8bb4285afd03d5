"""float32 numpy restatement of the self-distance contract written at stocs_symmetry_errors in include/stocs_hip.h (steps 1-4 there), built
on the pose-error restatement's transform, sqdist, nearest, root and fix; a float64 brute force of the same quantities; and a plain-Python
restatement of the steps of stocs_find_symmetries and of the host helpers, driven by either scorer.  Written from the contract, not from
the kernel: there is no grid here, every query looks at every target.  No GPU, numpy only."""
import math

import numpy as np

import pose_error_ref as base

F = np.float32
DTYPE = np.dtype([("sum_fix", np.uint64), ("mean", np.float32), ("max", np.float32), ("n_far", np.int32), ("n_normal_bad", np.int32),
                  ("valid", np.int32), ("reserved", np.int32)])
AXIS_DTYPE = np.dtype([("axis", np.float32, (3,)), ("order", np.int32), ("max", np.float32), ("mean", np.float32), ("n_normal_bad", np.int32),
                       ("reserved", np.int32)])
IDENTITY = np.eye(4, dtype=F).reshape(16)
COS30 = 0.8660254037844387
INEXACT, TRUNCATED, NOTHING = 1, 2, 4
POSE_SYM_MAX = 4096
GRID_SPAN = 60


def unit_normals(nrm):
    """the normals as the context keeps them: divided by their float length where its square is > 0, else as given"""
    n = np.ascontiguousarray(nrm, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        z = n[:, 0] * n[:, 0] + (n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        r = np.sqrt(z)
        out = np.where((z > 0)[:, None], n / r[:, None], n)
    assert out.dtype == F
    return out


def detail(S16, pts, nrm, reach, cos_normal=COS30):
    """steps 1-4 of one transform -> (s, nn, dot, matched, Dmin)"""
    S = np.asarray(S16, F).reshape(16)
    m = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n = unit_normals(nrm)
    p = base.transform(S, m)
    Dmin, nn = base.nearest(p, m)
    with np.errstate(all="ignore"):
        r2 = F(reach) * F(reach)
        matched = (Dmin <= r2) & (Dmin < F(np.inf))
        s = np.where(matched, base.root(Dmin), F(np.inf)).astype(F)
        nn = np.where(matched, nn, -1).astype(np.int32)
        rn = [S[a] * n[:, 0] + (S[4 + a] * n[:, 1] + S[8 + a] * n[:, 2]) for a in range(3)]
        t = n[np.maximum(nn, 0)]
        dot = rn[0] * t[:, 0] + (rn[1] * t[:, 1] + rn[2] * t[:, 2])
    assert dot.dtype == F
    dot = np.where(matched, dot, F(0)).astype(F)
    return s, nn, dot, matched, Dmin


def record(S16, pts, nrm, reach, cos_normal=COS30):
    s, nn, dot, matched, _ = detail(S16, pts, nrm, reach, cos_normal)
    M = len(s)
    r = np.zeros((), DTYPE)
    c = np.where(matched, s, F(reach)).astype(F)
    sf = int(base.fix(c).sum(dtype=np.uint64))
    r["sum_fix"] = sf
    r["mean"] = F(np.float64(sf) / 4294967296.0 / np.float64(M))
    r["max"] = s[matched].max() if matched.any() else F(0)
    r["n_far"] = int((~matched).sum())
    with np.errstate(all="ignore"):
        r["n_normal_bad"] = int((matched & ~(dot >= F(cos_normal))).sum())
    r["valid"] = 1
    return r


def records(S, pts, nrm, reach, cos_normal=COS30):
    S = np.asarray(S, F).reshape(-1, 16)
    return np.array([record(k, pts, nrm, reach, cos_normal) for k in S], DTYPE).reshape(len(S))


def records_equal(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in DTYPE.names)


def grid_edge(reach, pts):
    """the cell edge and the origin of the library's grid, as the header states them (case builders put points on cell faces with it)"""
    m = np.ascontiguousarray(pts, F).reshape(-1, 3)
    ext = float((m.max(0).astype(np.float64) - m.min(0).astype(np.float64)).max())
    return F(max(float(F(reach)) * 65.0 / 64.0, ext / GRID_SPAN)), m.min(0)


# ---- float64 brute force (no fixed point, no clamp of far points beyond the definition) ----
def record64(S16, pts, nrm, reach, cos_normal=COS30):
    """-> dict(mean, max, n_far, n_normal_bad) in float64"""
    S = np.asarray(S16, np.float64).reshape(4, 4).T
    m = np.asarray(pts, np.float64).reshape(-1, 3)
    n = np.asarray(nrm, np.float64).reshape(-1, 3)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 0, n / np.where(ln > 0, ln, 1), n)
    p = m @ S[:3, :3].T + S[:3, 3]
    d = np.empty(len(m)); nn = np.empty(len(m), np.int64)
    for a in range(0, len(m), base.ROWS):
        D = ((p[a:a + base.ROWS, None, :] - m[None, :, :]) ** 2).sum(-1)
        nn[a:a + base.ROWS] = D.argmin(1)
        d[a:a + base.ROWS] = np.sqrt(D.min(1))
    matched = d <= reach
    dot = ((n @ S[:3, :3].T) * n[nn]).sum(1)
    return dict(mean=float(np.where(matched, d, reach).mean()), max=float(d[matched].max()) if matched.any() else 0.0, n_far=int((~matched).sum()),
                n_normal_bad=int((matched & ~(dot >= cos_normal)).sum()))


def scorer64(pts, nrm, reach, cos_normal=COS30):
    """the float64 scores of many transforms at once, for the search restatement: the same quantities as record64 with the nearest
    neighbour taken from a kd-tree (scipy), whose float64 distances are the brute force's -> score(transforms) -> records (DTYPE)"""
    from scipy.spatial import cKDTree
    m = np.asarray(pts, np.float64).reshape(-1, 3)
    n = np.asarray(nrm, np.float64).reshape(-1, 3)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 0, n / np.where(ln > 0, ln, 1), n)
    tree = cKDTree(m)

    def score(S):
        S = np.asarray(S, F).reshape(-1, 16).astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
        out = np.zeros(len(S), DTYPE)
        for a in range(0, len(S), 512):
            R, t = S[a:a + 512, :3, :3], S[a:a + 512, :3, 3]
            p = np.einsum("kab,ib->kia", R, m) + t[:, None, :]
            d, nn = tree.query(p.reshape(-1, 3))
            d, nn = d.reshape(len(R), -1), nn.reshape(len(R), -1)
            matched = d <= reach
            dot = (np.einsum("kab,ib->kia", R, n) * n[nn]).sum(-1)
            o = out[a:a + 512]
            o["mean"] = np.where(matched, d, reach).mean(1)
            o["max"] = np.where(matched, d, 0.0).max(1)
            o["n_far"] = (~matched).sum(1)
            o["n_normal_bad"] = (matched & ~(dot >= cos_normal)).sum(1)
            o["valid"] = 1
        return out
    return score


# ---- the host helpers, restated ----
GOLDEN = math.pi * (3.0 - math.sqrt(5.0))


def _norm3(v):
    n = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return [v[0] / n, v[1] / n, v[2] / n]


def axes(n_axes):
    out = np.zeros((n_axes, 3), F)
    out[0, 0] = out[1, 1] = out[2, 2] = 1
    L = n_axes - 3
    for k in range(L):
        z = 1.0 - (k + 0.5) / L
        r = math.sqrt(1.0 - z * z)
        out[3 + k] = _norm3([r * math.cos(k * GOLDEN), r * math.sin(k * GOLDEN), z])
    return out


def lattice_spacing(n_axes):
    L = n_axes - 3
    return math.sqrt(2.0 * math.pi / L) if L > 0 else math.pi / 4.0


def rotation64(axis, angle_deg, center=None):
    """T(c) R T(-c) as a 4x4 float64 (row, column) matrix"""
    a = _norm3([float(x) for x in axis])
    c = np.zeros(3) if center is None else np.asarray([float(x) for x in center])
    q = angle_deg / 90.0
    if q == math.floor(q):
        k = int(q) % 4
        cs, sn = (1.0, 0.0, -1.0, 0.0)[k], (0.0, 1.0, 0.0, -1.0)[k]
    else:
        cs, sn = math.cos(angle_deg * math.pi / 180.0), math.sin(angle_deg * math.pi / 180.0)
    X = [[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]]
    T = np.eye(4)
    for i in range(3):
        for j in range(3):
            T[i, j] = (cs if i == j else 0.0) + sn * X[i][j] + (1.0 - cs) * a[i] * a[j]
    for i in range(3):
        T[i, 3] = c[i] - (T[i, 0] * c[0] + T[i, 1] * c[1] + T[i, 2] * c[2])
    return T


def rotation(axis, angle_deg, center=None):
    return (rotation64(axis, angle_deg, center) + 0.0).T.reshape(16).astype(F)


def close(gens, same_deg, cap=POSE_SYM_MAX):
    """-> ((K, 16) float32, truncated)"""
    G = [np.asarray(g, F).reshape(4, 4).T.astype(np.float64) for g in np.asarray(gens, F).reshape(-1, 16)]
    for g in G:
        g[3] = (0, 0, 0, 1)
    scale = max([np.linalg.norm(g[:3, 3]) for g in G], default=0.0)
    same = same_deg * math.pi / 180.0
    min_trace, max_shift = 1.0 + 2.0 * math.cos(same), same * scale
    kept, truncated, at = [np.eye(4)], False, 0
    while at < len(kept) and not truncated:
        for h in G:
            prod = h @ kept[at]
            if any((prod[:3, :3] * B[:3, :3]).sum() >= min_trace and np.linalg.norm(prod[:3, 3] - B[:3, 3]) <= max_shift for B in kept):
                continue
            if len(kept) >= cap:
                truncated = True
                break
            kept.append(prod)
        at += 1
    return np.stack([(k + 0.0).T.reshape(16).astype(F) for k in kept]), truncated


# ---- the search, restated (steps 1-4 at stocs_find_symmetries) ----
DEFAULTS = dict(tol_max=0.0, cos_normal=COS30, max_normal_bad=1.0, n_axes=2048, max_order=6, n_continuous=72, n_refine=16, n_local=32, rounds=4,
                same_deg=6.0)


def centroid(pts):
    m = np.ascontiguousarray(pts, F).reshape(-1, 3)
    s = [0.0, 0.0, 0.0]
    for p in m:
        for d in range(3):
            s[d] += float(p[d])
    return np.array([s[d] / len(m) for d in range(3)]).astype(F)


def _axis_cos(a, b):
    return abs(float(a[0]) * float(b[0]) + float(a[1]) * float(b[1]) + float(a[2]) * float(b[2]))


def cone(axis, theta, n_local):
    """the n_local directions of one refinement round about a float32 axis"""
    a = [float(x) for x in axis]
    e = 0
    for d in (1, 2):
        if abs(a[d]) < abs(a[e]):
            e = d
    u = [-a[e] * a[0], -a[e] * a[1], -a[e] * a[2]]
    u[e] += 1.0
    u = _norm3(u)
    v = [a[1] * u[2] - a[2] * u[1], a[2] * u[0] - a[0] * u[2], a[0] * u[1] - a[1] * u[0]]
    out = np.empty((n_local, 3), F)
    for k in range(n_local):
        t = math.tan(theta * math.sqrt((k + 0.5) / n_local))
        cp, sn = math.cos(k * GOLDEN), math.sin(k * GOLDEN)
        out[k] = np.asarray(_norm3([a[d] + t * (cp * u[d] + sn * v[d]) for d in range(3)])) + 0.0
    return out


def find(score, M, tol, center, **search):
    """score(transforms (n, 16) float32) -> records (DTYPE) at reach = tol; M the model's size; tol the resolved tol_max (float32);
    center a float32 triple -> (axes (AXIS_DTYPE), set (K, 16), sym3, flags)"""
    s = dict(DEFAULTS); s.update(search)
    tol = F(tol)
    orders = list(range(2, s["max_order"] + 1))
    cos_same = math.cos(float(F(s["same_deg"])) * math.pi / 180.0)

    def run(ax, od):
        return score(np.stack([rotation(a, 360.0 / n, center) for a, n in zip(ax, od)]))

    # 1
    dirs = axes(s["n_axes"])
    ax = [d for d in dirs for _ in orders]
    od = [n for _ in dirs for n in orders]
    rec = run(ax, od)
    rank = sorted(range(len(od)), key=lambda k: (float(rec[k]["mean"]), k))
    # 2
    kept = []
    for k in rank:
        if len(kept) >= s["n_refine"]:
            break
        if all(_axis_cos(q["axis"], ax[k]) < cos_same for q in kept):
            kept.append(dict(axis=ax[k].copy(), order=od[k], mean=rec[k]["mean"]))
    spacing = lattice_spacing(s["n_axes"])
    for rnd in range(s["rounds"]):
        theta = spacing / float(1 << rnd)
        ax = [d for q in kept for d in cone(q["axis"], theta, s["n_local"])]
        od = [q["order"] for q in kept for _ in range(s["n_local"])]
        rec = run(ax, od)
        for i, q in enumerate(kept):
            for k in range(s["n_local"]):
                at = i * s["n_local"] + k
                if rec[at]["mean"] < q["mean"]:
                    q["mean"], q["axis"] = rec[at]["mean"], ax[at].copy()
    # 3
    ax = [q["axis"] for q in kept for _ in orders]
    od = [n for _ in kept for n in orders]
    rec = run(ax, od)
    found = []
    for i, q in enumerate(kept):
        passing = [n for j, n in enumerate(orders)
                   if rec[i * len(orders) + j]["n_far"] == 0 and rec[i * len(orders) + j]["max"] <= tol
                   and F(rec[i * len(orders) + j]["n_normal_bad"]) <= F(s["max_normal_bad"]) * F(M)]
        if not passing:
            continue
        continuous = len(passing) == len(orders)
        r = rec[i * len(orders) + ((s["max_order"] if continuous else passing[-1]) - 2)]
        A = np.zeros((), AXIS_DTYPE)
        A["axis"], A["order"], A["max"], A["mean"], A["n_normal_bad"] = q["axis"], 0 if continuous else passing[-1], r["max"], r["mean"], r["n_normal_bad"]
        found.append(A)
    final = []
    for k in sorted(range(len(found)), key=lambda k: (float(found[k]["mean"]), k)):
        if all(_axis_cos(q["axis"], found[k]["axis"]) < cos_same for q in final):
            final.append(found[k])
    # 4
    flags, exact, desc, gens = 0, True, [0.0, 0.0, 0.0], []
    for A in final:
        n = s["n_continuous"] if A["order"] == 0 else int(A["order"])
        gens.append(rotation(A["axis"], 360.0 / n, center))
        on = -1
        for d in range(3):
            if abs(float(A["axis"][d])) >= cos_same:
                on = d
        names = {0: 360.0, 2: 180.0, 4: 90.0}.get(int(A["order"]), 0.0)
        if on < 0 or names == 0.0 or desc[on] != 0.0:
            exact = False
        else:
            desc[on] = names
    if not final:
        flags |= NOTHING
    elif not exact:
        flags |= INEXACT
    sym3 = np.array(desc if (final and exact) else [0, 0, 0], F)
    close_deg = float(min(F(s["same_deg"]), F(90.0) / F(s["n_continuous"])))
    S, truncated = close(np.asarray(gens, F).reshape(-1, 16), close_deg, min(search.get("cap_set", POSE_SYM_MAX), POSE_SYM_MAX))
    if truncated:
        flags |= TRUNCATED
    return np.array(final, AXIS_DTYPE).reshape(len(final)), S, sym3, flags
