"""float32 numpy restatement of the triangle-mesh rasteriser contract written at stocs_render_depth_mesh in include/stocs_hip.h: the
vertex transform, the triangle's skip rules and clamped box, the edge normals, the per-pixel edge rule and the z-buffer.  One operation at
a time, so that every intermediate is rounded to float32 exactly where the contract rounds it.  Vectorised over the triangles per offset
inside their boxes (small boxes) or over the pixels of one box (large boxes), never a Python loop per pixel.  Written from the contract,
not from the kernel; the GPU tests compare the library's z images and records with it for equality.  The compare pass and the record are
vsd_ref's, unchanged.  No GPU, numpy only."""
import numpy as np

import vsd_ref

F = np.float32
EMPTY = vsd_ref.EMPTY
compare = vsd_ref.compare
pixel_k = vsd_ref.pixel_k
bits_to_depth = vsd_ref.bits_to_depth
records_equal = vsd_ref.records_equal
DTYPE = vsd_ref.DTYPE
LARGE_BOX = 400            # pixels: above it a box is evaluated on its own, vectorised over its pixels


def setup(pose16, verts, tris, K, W, H):
    """steps 1-3 for every triangle -> dict: live (nt,), the boxes as int64, nA, nB, nC as lists of three (nt,) arrays, zA, zB, zC"""
    P = np.asarray(pose16, F).reshape(16)
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    t = np.ascontiguousarray(tris, np.int64).reshape(-1, 3)
    fx, cx, fy, cy = (F(x) for x in K)
    with np.errstate(all="ignore"):
        R = lambda a, b: P[4 * b + a]
        p = [(R(a, 0) * v[:, 0] + (R(a, 1) * v[:, 1] + R(a, 2) * v[:, 2])) + P[12 + a] for a in range(3)]
        assert all(x.dtype == F for x in p)
        A, B, C = ([p[k][t[:, j]] for k in range(3)] for j in range(3))
        finite = np.ones(len(t), bool)
        for X in (A, B, C):
            for k in range(3):
                finite &= np.isfinite(X[k])
        live = finite & (A[2] > F(1e-6)) & (B[2] > F(1e-6)) & (C[2] > F(1e-6))
        a = (fx * p[0]) / p[2] + cx
        b = (fy * p[1]) / p[2] + cy
        assert a.dtype == F and b.dtype == F
        xa, xb, xc = (a[t[:, j]] for j in range(3))
        ya, yb, yc = (b[t[:, j]] for j in range(3))
        c_lo = np.fmax(np.floor(np.fmin(xa, np.fmin(xb, xc))) - F(1), F(0))
        c_hi = np.fmin(np.floor(np.fmax(xa, np.fmax(xb, xc))) + F(2), F(W - 1))
        r_lo = np.fmax(np.floor(np.fmin(ya, np.fmin(yb, yc))) - F(1), F(0))
        r_hi = np.fmin(np.floor(np.fmax(ya, np.fmax(yb, yc))) + F(2), F(H - 1))
        assert c_lo.dtype == F and r_hi.dtype == F
        live &= (c_lo <= c_hi) & (r_lo <= r_hi)          # in float: a NaN skips
        cross = lambda u, w: [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
        nA, nB, nC = cross(B, C), cross(C, A), cross(A, B)
        assert all(x.dtype == F for x in nA + nB + nC)
    box = [np.where(live, x, 0).astype(np.int64) for x in (c_lo, c_hi, r_lo, r_hi)]
    return dict(live=live, c_lo=box[0], c_hi=box[1], r_lo=box[2], r_hi=box[3], nA=nA, nB=nB, nC=nC, zA=A[2], zB=B[2], zC=C[2])


def _pixels(zbuf, g, ti, r, c, K, W):
    """step 4 for the pixels (r, c) of the triangles ti (arrays of one length, or ti a scalar index)"""
    fx, cx, fy, cy = (F(x) for x in K)
    with np.errstate(all="ignore"):
        xn = (c.astype(F) - cx) / fx
        yn = (r.astype(F) - cy) / fy
        u = xn * g["nA"][0][ti] + (yn * g["nA"][1][ti] + g["nA"][2][ti])
        v = xn * g["nB"][0][ti] + (yn * g["nB"][1][ti] + g["nB"][2][ti])
        w = xn * g["nC"][0][ti] + (yn * g["nC"][1][ti] + g["nC"][2][ti])
        det = u + (v + w)
        z = (u * g["zA"][ti] + (v * g["zB"][ti] + w * g["zC"][ti])) / det
        assert z.dtype == F and det.dtype == F
        inside = ((u >= F(0)) & (v >= F(0)) & (w >= F(0))) | ((u <= F(0)) & (v <= F(0)) & (w <= F(0)))
        hit = (det != F(0)) & inside & (z > F(1e-6))
    np.minimum.at(zbuf, (r * W + c)[hit], np.ascontiguousarray(z[hit]).view(np.uint32))


def render_bits(pose16, verts, tris, K, W, H, every_pixel=False):
    """the z-buffer of one pose: (H * W) uint32 float bits, empty = all ones.  every_pixel: every live triangle is tested on every pixel
    of the image, not on its box (the rule the box must not change)"""
    zbuf = np.full(H * W, EMPTY, np.uint32)
    if not vsd_ref.pose_finite(pose16) or len(np.asarray(tris).reshape(-1, 3)) == 0:
        return zbuf
    g = setup(pose16, verts, tris, K, W, H)
    live = np.flatnonzero(g["live"])
    if len(live) == 0:
        return zbuf
    if every_pixel:
        rr, cc = np.divmod(np.arange(H * W, dtype=np.int64), W)
        for i in live:
            _pixels(zbuf, g, int(i), rr, cc, K, W)
        return zbuf
    w = g["c_hi"][live] - g["c_lo"][live] + 1
    h = g["r_hi"][live] - g["r_lo"][live] + 1
    large = w * h > LARGE_BOX
    for i in live[large]:                                    # one box at a time, all its pixels at once
        rr, cc = np.meshgrid(np.arange(g["r_lo"][i], g["r_hi"][i] + 1), np.arange(g["c_lo"][i], g["c_hi"][i] + 1), indexing="ij")
        _pixels(zbuf, g, int(i), rr.reshape(-1), cc.reshape(-1), K, W)
    s = live[~large]
    if len(s):
        ws, hs = w[~large], h[~large]
        for dy in range(int(hs.max())):                      # offset by offset: the triangles whose box reaches it
            for dx in range(int(ws.max())):
                ok = (hs > dy) & (ws > dx)
                if ok.any():
                    ti = s[ok]
                    _pixels(zbuf, g, ti, g["r_lo"][ti] + dy, g["c_lo"][ti] + dx, K, W)
    return zbuf


def render_depth(poses16, verts, tris, K, W, H):
    P = np.asarray(poses16, F).reshape(-1, 16)
    return np.stack([bits_to_depth(render_bits(P[i], verts, tris, K, W, H), W, H) for i in range(len(P))]) if len(P) else np.zeros((0, H, W), F)


def pose_errors_vsd_mesh(est16, gt16, verts, tris, depth_u16, K, depth_scale, taus, delta=0.015):
    """stocs_pose_errors_vsd_mesh -> records of vsd_ref.DTYPE; gt16 holds one pose or as many as est16"""
    H, W = depth_u16.shape
    E = np.asarray(est16, F).reshape(-1, 16)
    G = np.asarray(gt16, F).reshape(-1, 16)
    assert len(G) in (1, len(E))
    out = np.zeros(len(E), DTYPE)
    zG = None
    for i in range(len(E)):
        g = G[0] if len(G) == 1 else G[i]
        if zG is None or len(G) != 1:
            zG = render_bits(g, verts, tris, K, W, H)
        zE = render_bits(E[i], verts, tris, K, W, H)
        out[i], _ = compare(zE, zG, depth_u16, K, depth_scale, taus, delta=delta)
        out[i]["valid"] = 0 if (not vsd_ref.pose_finite(E[i]) or not vsd_ref.pose_finite(g) or not np.any(E[i] != 0)) else 1
    return out
