"""float32 numpy restatement of the surfel-renderer and visible-surface-discrepancy contract written at stocs_pose_errors_vsd in
include/stocs_hip.h: the surfel rule, the z-buffer, the per-pixel visibility and the record.  One operation at a time, so that every
intermediate is rounded to float32 exactly where the contract rounds it.  Vectorised over the points per offset of the surfel's square
(33 x 33 offsets at most), never a Python loop per point.  Written from the contract, not from the kernels; the GPU tests compare the
library's z images and records with it for equality.  No GPU, numpy only."""
import numpy as np

import depth_check_ref as dref

F = np.float32
EMPTY = np.uint32(0xFFFFFFFF)
MAX_TAU = 16
DTYPE = np.dtype([("px_est", np.int32), ("px_gt", np.int32), ("vis_est", np.int32), ("vis_gt", np.int32), ("inter", np.int32), ("uni", np.int32),
                  ("far", np.int32, (16,)), ("e", np.float32, (16,)), ("valid", np.int32), ("reserved", np.int32)])
DEFAULTS = dict(surfel_radius=0.006, max_splat_px=16, delta=0.015)
_USED = [i for i in range(15) if i % 4 != 3]


def pose_finite(P):
    return bool(np.all(np.isfinite(np.asarray(P, F).reshape(16)[_USED])))


def project(pose16, model_pos, model_unit_nrm, K, W, H):
    """steps 1-3 of the depth-check contract with p, q and f kept -> dict of per-point arrays"""
    P = np.asarray(pose16, F).reshape(16)
    m = np.ascontiguousarray(model_pos, F).reshape(-1, 3)
    k = np.ascontiguousarray(model_unit_nrm, F).reshape(-1, 3)
    fx, cx, fy, cy = (F(v) for v in K)
    with np.errstate(all="ignore"):
        R = lambda a, b: P[4 * b + a]
        p = [(R(a, 0) * m[:, 0] + (R(a, 1) * m[:, 1] + R(a, 2) * m[:, 2])) + P[12 + a] for a in range(3)]
        q = [R(a, 0) * k[:, 0] + (R(a, 1) * k[:, 1] + R(a, 2) * k[:, 2]) for a in range(3)]
        f = q[0] * p[0] + (q[1] * p[1] + q[2] * p[2])
        assert all(v.dtype == F for v in p + q + [f])
        facing = (f < F(0)) & (p[2] > F(1e-6))
        a = np.floor(((fx * p[0]) / p[2] + cx) + F(0.5))
        b = np.floor(((fy * p[1]) / p[2] + cy) + F(0.5))
        in_image = facing & (a >= F(0)) & (a < F(W)) & (b >= F(0)) & (b < F(H))
    col = np.where(in_image, a, 0).astype(np.int64)
    row = np.where(in_image, b, 0).astype(np.int64)
    return dict(p=p, q=q, f=f, in_image=in_image, col=col, row=row)


def render_bits(pose16, model_pos, model_unit_nrm, K, W, H, surfel_radius=0.006, max_splat_px=16, **_):
    """the z-buffer of one pose: (H * W) uint32 float bits, empty = all ones"""
    zbuf = np.full(H * W, EMPTY, np.uint32)
    if not pose_finite(pose16) or len(np.asarray(model_pos).reshape(-1, 3)) == 0:
        return zbuf
    g = project(pose16, model_pos, model_unit_nrm, K, W, H)
    sel = g["in_image"]
    if not sel.any():
        return zbuf
    p = [v[sel] for v in g["p"]]; q = [v[sel] for v in g["q"]]
    f, col, row = g["f"][sel], g["col"][sel], g["row"][sel]
    fx, cx, fy, cy = (F(v) for v in K)
    rad = F(surfel_radius)
    r2 = rad * rad
    with np.errstate(all="ignore"):
        s = np.minimum(np.floor((fx * rad) / p[2] + F(0.5)), F(max_splat_px))
    assert s.dtype == F and r2.dtype == F
    s = s.astype(np.int64)
    smax = int(s.max())
    for dy in range(-smax, smax + 1):                        # offset by offset: the surfels whose square reaches it
        for dx in range(-smax, smax + 1):
            r, c = row + dy, col + dx
            ok = (s >= max(abs(dy), abs(dx))) & (r >= 0) & (r < H) & (c >= 0) & (c < W)
            if not ok.any():
                continue
            r, c = r[ok], c[ok]
            with np.errstate(all="ignore"):
                xn = (c.astype(F) - cx) / fx
                yn = (r.astype(F) - cy) / fy
                dn = q[0][ok] * xn + (q[1][ok] * yn + q[2][ok])
                z = f[ok] / dn
                ex = xn * z - p[0][ok]; ey = yn * z - p[1][ok]; ez = z - p[2][ok]
                d2 = (ex * ex) + ((ey * ey) + (ez * ez))
                assert d2.dtype == F and z.dtype == F
                hit = (dn < F(0)) & (z > F(1e-6)) & (d2 <= r2)
            np.minimum.at(zbuf, (r * W + c)[hit], z[hit].view(np.uint32))
    return zbuf


def bits_to_depth(zbuf, W, H):
    """the z image of stocs_render_depth: 0 where empty"""
    return np.where(zbuf == EMPTY, np.uint32(0), zbuf).view(F).reshape(H, W)


def render_depth(poses16, model_pos, model_nrm, K, W, H, **params):
    P = np.asarray(poses16, F).reshape(-1, 16)
    k = dref.unit_normals(model_nrm)
    return np.stack([bits_to_depth(render_bits(P[i], model_pos, k, K, W, H, **params), W, H) for i in range(len(P))]) if len(P) else np.zeros((0, H, W), F)


def pixel_k(K, W, H):
    """per pixel: k = sqrt((xn xn + yn yn) + 1), flat row-major"""
    fx, cx, fy, cy = (F(v) for v in K)
    xn = (np.arange(W).astype(F) - cx) / fx
    yn = (np.arange(H).astype(F) - cy) / fy
    X, Y = np.meshgrid(xn, yn)
    k = np.sqrt((X * X + Y * Y) + F(1.0))
    assert k.dtype == F
    return k.reshape(-1)


def distances(zbuf, K, W, H):
    """(present, d = Z k) per pixel of a z-buffer"""
    present = zbuf != EMPTY
    with np.errstate(all="ignore"):
        d = zbuf.view(F) * pixel_k(K, W, H)
    return present, d


def compare(zE, zG, depth_u16, K, depth_scale, taus, delta=0.015, **_):
    """one record (without valid) from two z-buffers and the frame; also returns the per-pixel masks"""
    H, W = depth_u16.shape
    k = pixel_k(K, W, H)
    raw = np.ascontiguousarray(depth_u16, np.uint16).reshape(-1)
    pe, dE = distances(zE, K, W, H)
    pg, dG = distances(zG, K, W, H)
    dlt = F(delta)
    with np.errstate(all="ignore"):
        dS = (raw.astype(F) * F(depth_scale)) * k
        assert dS.dtype == F
        visG = pg & ((raw == 0) | (dG - dS <= dlt))
        visE = pe & ((raw == 0) | (dE - dS <= dlt) | visG)
        inter = visG & visE
        uni = visG | visE
        dd = np.abs(dG - dE)
    t = np.asarray(taus, F).reshape(-1)
    assert 1 <= len(t) <= MAX_TAU
    r = np.zeros((), DTYPE)
    r["px_est"], r["px_gt"], r["vis_est"], r["vis_gt"], r["inter"], r["uni"] = pe.sum(), pg.sum(), visE.sum(), visG.sum(), inter.sum(), uni.sum()
    for i in range(len(t)):
        with np.errstate(all="ignore"):
            r["far"][i] = int((inter & (dd >= t[i])).sum())
        n_u, n_i = int(r["uni"]), int(r["inter"])
        r["e"][i] = F(int(r["far"][i]) + (n_u - n_i)) / F(n_u) if n_u > 0 else F(1.0)
    return r, dict(visE=visE, visG=visG, inter=inter, uni=uni, pe=pe, pg=pg, dE=dE, dG=dG, dS=dS, dd=dd)


def pose_errors_vsd(est16, gt16, model_pos, model_nrm, depth_u16, K, depth_scale, taus, **params):
    """stocs_pose_errors_vsd -> records of DTYPE; gt16 holds one pose or as many as est16"""
    prm = dict(DEFAULTS); prm.update(params)
    H, W = depth_u16.shape
    E = np.asarray(est16, F).reshape(-1, 16)
    G = np.asarray(gt16, F).reshape(-1, 16)
    assert len(G) in (1, len(E))
    kn = dref.unit_normals(model_nrm)
    out = np.zeros(len(E), DTYPE)
    zG = None
    for i in range(len(E)):
        g = G[0] if len(G) == 1 else G[i]
        if zG is None or len(G) != 1:
            zG = render_bits(g, model_pos, kn, K, W, H, **prm)
        zE = render_bits(E[i], model_pos, kn, K, W, H, **prm)
        out[i], _ = compare(zE, zG, depth_u16, K, depth_scale, taus, **prm)
        out[i]["valid"] = 0 if (not pose_finite(E[i]) or not pose_finite(g) or not np.any(E[i] != 0)) else 1
    return out


def records_equal(a, b):
    """array_equal on the counts, bit equality on the errors"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    ok = all(np.array_equal(a[c], b[c]) for c in ("px_est", "px_gt", "vis_est", "vis_gt", "inter", "uni", "far", "valid", "reserved"))
    return ok and np.array_equal(np.ascontiguousarray(a["e"]).view(np.uint32), np.ascontiguousarray(b["e"]).view(np.uint32))


def pose_recall_vsd(records, n_tau=10):
    """the mean over the taus and over the correctness thresholds 0.05 .. 0.50 of the share of records with e[t] below the threshold,
    an invalid record counted as wrong (BOP's average recall of VSD written as plain loops, for the tests of estimator.pose_recall_vsd)"""
    records = np.asarray(records).reshape(-1)
    hits, total = 0, 0
    for r in records:
        for t in range(n_tau):
            for i in range(1, 11):
                total += 1
                hits += int(r["valid"] != 0 and r["e"][t] < F(0.05 * i))
    return hits / total
