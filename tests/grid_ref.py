"""Reference of the scene grid's one job -- the restricted nearest neighbour of the scoring kernels (lcp.hip) -- restated in numpy
float32 in the kernels' own operation order (the library is built with -ffp-contract=off, so every float operation below is the
kernel's, bit for bit), next to a float64 brute force of the same question.  Also the host geometry of build_grid_gpu (grid.hip), the
centring of the clouds (ctx.hip) and the integer score (lcp.hip: lcp_add / lcp_finish).  No GPU, no library: numpy only.

Conventions: transforms are 16 floats, column-major (t0 t4 t8 t12 is the first row).  A hit index of -1 means no scene point within
epsilon.  Ties on the float32 squared distance go to the LARGEST scene index."""
import math

import numpy as np

F = np.float32
COS30 = math.cos(math.radians(30.0))


def centre(pos):
    """centroid_shift of ctx.hip: sequential float sums per axis, one division, one subtraction per point.  -> (centred, centroid)"""
    pos = np.ascontiguousarray(pos, F)
    c = np.zeros(3, F)
    if len(pos):
        c = np.add.accumulate(pos, axis=0, dtype=F)[-1] / F(len(pos))      # accumulate is sequential (np.sum is pairwise)
    return (pos - c).astype(F), c.astype(F)


def geometry(spos_centred, eps, div):
    """Host part of build_grid_gpu in float64, then the floats the kernels receive.  eps: the float32 distance threshold."""
    eps = float(F(eps))
    h = eps / div
    p = np.asarray(spos_centred, F).astype(np.float64)
    mn, mx = p.min(0), p.max(0)
    r = inclusion_radius(eps, mn, mx, div)
    pad = r + 2 * h
    o = mn - pad
    n = [int(math.floor(((mx[k] + pad) - o[k]) / h)) + 1 for k in range(3)]
    return dict(o=o, h64=h, r=r, pad=pad, div=div, eps=eps,
                origin=o.astype(F), h=F(h), inv_h=F(1.0 / h), cells=tuple(n), bricks=tuple((v + 7) // 8 for v in n))


def inclusion_radius(eps, mn, mx, div):
    """r of build_grid_gpu: a cell lists every point within r of its box.  1.001 epsilon, or -- once the float rounding of the kernels'
    cell computation, 3 * 2^-24 of the largest offset from the origin, comes near that margin -- epsilon + 2^-21 of that offset."""
    r0 = eps * 1.001
    h = eps / div
    reach = float(np.max(mx - mn)) + 2.0 * (r0 + 2 * h) + h
    return max(r0, eps + reach * (1.0 / 2097152.0))


def incidences(spos_centred, g):
    """incidence_kernel of grid.hip in float64, operation for operation: per scene point, the cells whose box (from the FLOAT origin,
    widened) lies within r.  -> dict: per_point (n,) counts, n_incidences, n_cells, n_bricks, longest (points in the fullest cell),
    n_entries_unpruned (lists padded to 8), cell (linear id per incidence) and point (index per incidence)."""
    p = np.asarray(spos_centred, F).astype(np.float64)
    of = g["origin"].astype(np.float64)
    h, r, n = g["h64"], g["r"], g["cells"]
    nb = g["bricks"]
    lo = np.maximum(0, np.floor((p - r - of) / h).astype(np.int64))
    hi = np.minimum(np.array(n) - 1, np.floor((p + r - of) / h).astype(np.int64))
    cnt = np.zeros(len(p), np.int64)
    cells, bricks, points = [], [], []
    w = int((hi - lo).max()) + 1
    for dz in range(w):
        for dy in range(w):
            for dx in range(w):
                c = lo + np.array([dx, dy, dz])
                ok = np.all(c <= hi, axis=1)
                b0 = of + c * h
                b1 = b0 + h
                d = np.where(p < b0, b0 - p, np.where(p > b1, p - b1, 0.0))
                d2 = (0.0 + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
                ok &= ~(d2 > r * r)
                cnt += ok
                c = c[ok]
                cells.append((c[:, 2] * n[1] + c[:, 1]) * n[0] + c[:, 0])
                bricks.append(((c[:, 2] >> 3) * nb[1] + (c[:, 1] >> 3)) * nb[0] + (c[:, 0] >> 3))
                points.append(np.nonzero(ok)[0])
    cells, bricks, points = np.concatenate(cells), np.concatenate(bricks), np.concatenate(points)
    _, per_cell = np.unique(cells, return_counts=True)
    return dict(per_point=cnt, n_incidences=int(cnt.sum()), n_cells=len(per_cell), n_bricks=len(np.unique(bricks)), longest=int(per_cell.max()),
                n_entries_unpruned=int(((per_cell + 7) // 8 * 8).sum()), cell=cells, point=points)


def box_dist2(p, cell, g):
    """box_dist2 of grid.hip: squared distance from points p (n,3) to the boxes of cells (n,3), float64 from the float origin."""
    p = np.asarray(p, F).astype(np.float64)
    b0 = g["origin"].astype(np.float64) + np.asarray(cell) * g["h64"]
    b1 = b0 + g["h64"]
    d = np.where(p < b0, b0 - p, np.where(p > b1, p - b1, 0.0))
    return (0.0 + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def cell_coord(q, g, sub=1):
    """floor((q - origin) * inv_h * sub) as the kernels compute it (sub = 4: the queue kernel's sub-cell index, inv_h4 = inv_h * 4)."""
    q = np.asarray(q, F)
    inv = F(g["inv_h"] * F(sub))
    return np.floor(((q - g["origin"]).astype(F) * inv).astype(F)).astype(np.int64)


def face_float(g, axis, k, sub=1):
    """The smallest float32 coordinate on `axis` that the kernels put into cell (or sub-cell) >= k: the face as the kernels see it."""
    o, inv = g["origin"][axis], F(g["inv_h"] * F(sub))
    x0 = g["o"][axis] + k * g["h64"] / sub
    idx = lambda v: math.floor(F(F(v - o) * inv))
    # floats as ordered integers (so that a bisection also crosses zero, where the floats are dense); idx is monotone
    key = lambda v: (lambda i: i if i >= 0 else -(i & 0x7FFFFFFF))(int(np.asarray(v, F).view(np.int32)))
    val = lambda j: np.array(j if j >= 0 else ((-j) | 0x80000000) - (1 << 32), np.int64).astype(np.int32).view(F)
    d = 16.0 * (float(np.spacing(F(abs(float(o)) + abs(x0)))) + 1e-30)
    a, b = key(F(x0 - d)), key(F(x0 + d))
    assert idx(val(a)) < k <= idx(val(b)), (axis, k, sub)
    while b - a > 1:
        m = (a + b) // 2
        if idx(val(m)) >= k:
            b = m
        else:
            a = m
    return F(val(b))


def transform(T16, mpos):
    """((t0 x + t4 y) + t8 z) + t12 per row, float32."""
    t = np.asarray(T16, F)
    x, y, z = (np.asarray(mpos, F)[:, k] for k in range(3))
    rows = []
    for a in range(3):
        rows.append((((t[a] * x).astype(F) + (t[4 + a] * y).astype(F)).astype(F) + (t[8 + a] * z).astype(F)).astype(F) + t[12 + a])
    return np.stack(rows, 1).astype(F)


def rotate_normal(T16, mnrm):
    """t0 x + (t4 y + t8 z) per row, float32."""
    t = np.asarray(T16, F)
    x, y, z = (np.asarray(mnrm, F)[:, k] for k in range(3))
    return np.stack([((t[a] * x).astype(F) + ((t[4 + a] * y).astype(F) + (t[8 + a] * z).astype(F)).astype(F)).astype(F) for a in range(3)], 1)


def sq_eps(eps):
    return F(F(eps) * F(eps))


def d2_f32(q, s):
    """dx*dx + (dy*dy + dz*dz) in float32; q (n,3) against s (m,3) -> (n,m)"""
    d = (np.asarray(q, F)[:, None, :] - np.asarray(s, F)[None, :, :]).astype(F)
    dd = (d * d).astype(F)
    return (dd[..., 0] + (dd[..., 1] + dd[..., 2]).astype(F)).astype(F)


def nn_f32(q, spos, eps, chunk=512):
    """The product's answer: nearest scene point by float32 d2, inclusive radius d2 <= fl(eps*eps), ties to the largest index.
    -> (hit (n,), d2 of the winner (n,) or inf)"""
    s2 = sq_eps(eps)
    nS = len(spos)
    hit = np.full(len(q), -1, np.int64); best = np.full(len(q), np.inf, F)
    for i in range(0, len(q), chunk):
        d2 = d2_f32(q[i:i + chunk], spos)
        j = nS - 1 - np.argmin(d2[:, ::-1], axis=1)          # last index of the minimum
        m = d2[np.arange(len(j)), j]
        ok = m <= s2
        hit[i:i + chunk] = np.where(ok, j, -1)
        best[i:i + chunk] = np.where(ok, m, np.inf)
    return hit, best


def nn_f64(q, spos, eps, chunk=512):
    """Float64 brute force on the same float32 inputs.  -> (hit, nearest distance, gap to the runner-up distance), hit = -1 beyond eps."""
    e = float(F(eps))
    q = np.asarray(q, F).astype(np.float64); s = np.asarray(spos, F).astype(np.float64)
    hit = np.full(len(q), -1, np.int64); dist = np.zeros(len(q)); gap = np.full(len(q), np.inf)
    for i in range(0, len(q), chunk):
        d = np.sqrt(((q[i:i + chunk, None, :] - s[None, :, :]) ** 2).sum(-1))
        j = len(s) - 1 - np.argmin(d[:, ::-1], axis=1)
        m = d[np.arange(len(j)), j]
        if len(s) > 1:
            d[np.arange(len(j)), j] = np.inf
            gap[i:i + chunk] = d.min(1) - m
        dist[i:i + chunk] = m
        hit[i:i + chunk] = np.where(m <= e, j, -1)
    return hit, dist, gap


def counted_flags(T16, mnrm, snrm, hit):
    """The 30-degree normal test of a hit: d = sn.x nx + (sn.y ny + sn.z nz) in float32, counted <=> dot_lo <= d <= 1.  The cases keep
    d far from dot_lo (asserted here), so cos 30 stands in for the library's exact float threshold.  -> (counted, d)"""
    n = rotate_normal(T16, mnrm)
    sn = np.asarray(snrm, F)[np.maximum(hit, 0)]
    d = ((sn[:, 0] * n[:, 0]).astype(F) + ((sn[:, 1] * n[:, 1]).astype(F) + (sn[:, 2] * n[:, 2]).astype(F)).astype(F)).astype(F)
    on = hit >= 0
    assert not np.any(on & (np.abs(d.astype(np.float64) - COS30) < 0.05)), "a case put a normal pair near the 30 degree threshold"
    return on & (d >= F(COS30)) & (d <= F(1.0)), d


def score(counted, hit, prob, M):
    """lcp_add / lcp_finish: sum of trunc(w * 2^32) over the counted points, / 2^32 / M in double, rounded to float."""
    w = np.asarray(prob, F)[np.maximum(hit, 0)]
    use = counted & (w > 0)
    total = int(np.sum(np.floor(w[use].astype(np.float64) * 4294967296.0).astype(np.uint64), dtype=np.uint64)) if use.any() else 0
    return F(float(total) * (1.0 / 4294967296.0) / float(M))


def reference(case):
    """Everything the GPU tests compare against, for every transform of a case: a list of dicts (q, hit, counted, score, hit64, dist64,
    gap64).  Computed once per case (cached on the case)."""
    if "_ref" in case:
        return case["_ref"]
    sc, cs = centre(case["spos"]); mc, cm = centre(case["mpos"])
    out = []
    for T in case["T"]:
        q = transform(T, mc)
        hit, best = nn_f32(q, sc, case["eps"])
        cnt, dot = counted_flags(T, case["mnrm"], case["snrm"], hit)
        h64, dist, gap = nn_f64(q, sc, case["eps"])
        out.append(dict(q=q, hit=hit, d2=best, counted=cnt, dot=dot, score=score(cnt, hit, case["sprob"], len(mc)), hit64=h64, dist64=dist, gap64=gap))
    case["_ref"] = out
    case["_centred"] = (sc, cs, mc, cm)
    return out
