"""float32 numpy restatement of the depth-check contract written at stocs_depth_check_poses in include/stocs_hip.h (steps 1-6 there), one
operation at a time so that every intermediate is rounded to float32 exactly where the contract rounds it.  Written from the contract,
not from the kernel; the GPU tests compare the library's records with it for equality.  No GPU, numpy only."""
import numpy as np

F = np.float32
COUNTS = ("facing", "in_image", "self_occluded", "no_depth", "agree", "in_front", "behind", "on_mask")
DTYPE = np.dtype([(k, np.int32) for k in COUNTS] + [("score", np.float32), ("violation", np.float32)])
DEFAULTS = dict(tolerance=0.01, class_threshold=0.10, self_occlusion=1, cell_px=8, occlusion_margin=0.01)


def unit_normals(nrm):
    """the context's unit normals: z = x x + (y y + z z); z > 0 ? n / sqrt(z) : n, in float32"""
    n = np.ascontiguousarray(nrm, F).reshape(-1, 3)
    z = n[:, 0] * n[:, 0] + (n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    with np.errstate(all="ignore"):
        u = n / np.sqrt(z)[:, None]
    return np.where((z > 0)[:, None], u, n).astype(F)


def point_flags(pose16, model_pos, model_unit_nrm, depth_u16, prob_u16, K, depth_scale, **params):
    """-> dict of boolean arrays per model point (the eight classes) plus col, row, z; pose16 column-major"""
    prm = dict(DEFAULTS); prm.update(params)
    P = np.asarray(pose16, F).reshape(16)
    m = np.ascontiguousarray(model_pos, F).reshape(-1, 3)
    k = np.ascontiguousarray(model_unit_nrm, F).reshape(-1, 3)
    n = len(m)
    H, W = depth_u16.shape
    fx, cx, fy, cy = (F(v) for v in K)
    scale, tol, thr, margin = F(depth_scale), F(prm["tolerance"]), F(prm["class_threshold"]), F(prm["occlusion_margin"])
    zero = np.zeros(n, bool)
    out = {c: zero.copy() for c in COUNTS}
    out.update(col=np.zeros(n, np.int64), row=np.zeros(n, np.int64), z=np.zeros(n, F))
    used = [i for i in range(15) if i % 4 != 3]
    if not np.all(np.isfinite(P[used])):
        return out
    with np.errstate(all="ignore"):
        R = lambda a, b: P[4 * b + a]
        p = [(R(a, 0) * m[:, 0] + (R(a, 1) * m[:, 1] + R(a, 2) * m[:, 2])) + P[12 + a] for a in range(3)]
        q = [R(a, 0) * k[:, 0] + (R(a, 1) * k[:, 1] + R(a, 2) * k[:, 2]) for a in range(3)]
        assert all(v.dtype == F for v in p + q)
        facing = ((q[0] * p[0] + (q[1] * p[1] + q[2] * p[2])) < F(0)) & (p[2] > F(1e-6))
        a = np.floor(((fx * p[0]) / p[2] + cx) + F(0.5))
        b = np.floor(((fy * p[1]) / p[2] + cy) + F(0.5))
        assert a.dtype == F and b.dtype == F
        in_image = facing & (a >= F(0)) & (a < F(W)) & (b >= F(0)) & (b < F(H))
    col = np.where(in_image, a, 0).astype(np.int64)
    row = np.where(in_image, b, 0).astype(np.int64)
    z = p[2]
    self_occ = zero.copy()
    if prm["self_occlusion"] == 1 and in_image.any():
        c0, c1, r0, r1 = col[in_image].min(), col[in_image].max(), row[in_image].min(), row[in_image].max()
        ext = int(max(c1 - c0 + 1, r1 - r0 + 1))
        s = max(int(prm["cell_px"]), (ext + 63) // 64)
        cell = ((row - r0) // s) * 64 + (col - c0) // s
        zmin = np.full(64 * 64, np.inf, F)
        np.minimum.at(zmin, cell[in_image], z[in_image])
        self_occ[in_image] = z[in_image] > (zmin[cell[in_image]] + margin)
    rest = in_image & ~self_occ
    raw = np.zeros(n, np.uint16)
    raw[rest] = depth_u16[row[rest], col[rest]]
    no_depth = rest & (raw == 0)
    have = rest & (raw != 0)
    zo = raw.astype(F) * scale
    d = z - zo
    assert d.dtype == F
    agree = have & (np.abs(d) <= tol)
    in_front = have & (d < -tol)
    behind = have & (d > tol)
    on_mask = zero.copy()
    if prob_u16 is not None:
        cp = (prob_u16[row, col].astype(np.float64) * (1.0 / 10000)).astype(F)
        on_mask = agree & ~(cp < thr)
    out.update(facing=facing, in_image=in_image, self_occluded=self_occ, no_depth=no_depth, agree=agree, in_front=in_front, behind=behind,
               on_mask=on_mask, col=col, row=row, z=z)
    return out


def check_pose(pose16, model_pos, model_unit_nrm, depth_u16, prob_u16, K, depth_scale, **params):
    """one record of DTYPE"""
    f = point_flags(pose16, model_pos, model_unit_nrm, depth_u16, prob_u16, K, depth_scale, **params)
    r = np.zeros((), DTYPE)
    for c in COUNTS:
        r[c] = int(f[c].sum())
    if r["facing"] > 0:
        r["score"] = F(r["agree"]) / F(r["facing"])
        r["violation"] = F(r["in_front"]) / F(r["facing"])
    return r


def check_poses(poses16, model_pos, model_nrm, depth_u16, prob_u16, K, depth_scale, **params):
    """records for n poses; model_nrm as handed to the context (normalised here as the context does)"""
    P = np.asarray(poses16, F).reshape(-1, 16)
    k = unit_normals(model_nrm)
    out = np.zeros(len(P), DTYPE)
    for i in range(len(P)):
        out[i] = check_pose(P[i], model_pos, k, depth_u16, prob_u16, K, depth_scale, **params)
    return out


def records_equal(a, b):
    """array_equal on the eight counts, bit equality on the two floats"""
    ok = all(np.array_equal(a[c], b[c]) for c in COUNTS)
    return ok and all(np.array_equal(np.asarray(a[c], F).view(np.uint32), np.asarray(b[c], F).view(np.uint32)) for c in ("score", "violation"))
