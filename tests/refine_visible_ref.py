"""numpy restatement of the visible-surface refinement contract written at stocs_refine_poses_visible in include/stocs_hip.h: the keys
of the triangle-key render (mesh_ref's setup and per-pixel rule under an arg-min that breaks ties to the lowest triangle index), the
per-pixel state in float32 one operation at a time, the rows, the 29 sums and the solve in float64, and one-step and k-step loops on
float32 poses.  Written from the contract, not from the kernels; the GPU tests compare keys and states for equality and sums and poses
within the rounding bounds of the double sums.  No GPU, numpy only."""
import numpy as np

import mesh_ref
import vsd_ref

F = np.float32
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
EMPTY, NO_DEPTH, OFF_CLASS, TOO_FAR, GRAZING, COUNTED = range(6)
DEFAULTS = dict(max_iterations=5, max_distance=0.02, min_view_cos=0.0, class_threshold=0.10)
RECORD_FIELDS = ("present", "no_depth", "off_class", "too_far", "grazing", "counted", "iterations", "frozen", "rms")


def pose_valid(pose16):
    """step 7: a pose that renders at all"""
    P = np.asarray(pose16, F).reshape(16)
    return vsd_ref.pose_finite(P) and bool(np.any(P != 0))


def keys(pose16, verts, tris, K, W, H):
    """the key buffer of one pose: (H * W) uint64, bits(z) << 32 | triangle, empty = all ones"""
    out = np.full(H * W, EMPTY_KEY, np.uint64)
    t = np.asarray(tris).reshape(-1, 3)
    if not vsd_ref.pose_finite(pose16) or len(t) == 0:
        return out
    g = mesh_ref.setup(pose16, verts, tris, K, W, H)
    tmp = np.full(H * W, mesh_ref.EMPTY, np.uint32)
    for i in np.flatnonzero(g["live"]):                       # one triangle alone, then the minimum over (bits, index)
        rr, cc = np.meshgrid(np.arange(g["r_lo"][i], g["r_hi"][i] + 1), np.arange(g["c_lo"][i], g["c_hi"][i] + 1), indexing="ij")
        rr, cc = rr.reshape(-1), cc.reshape(-1)
        mesh_ref._pixels(tmp, g, int(i), rr, cc, K, W)
        px = rr * W + cc
        px = px[tmp[px] != mesh_ref.EMPTY]
        out[px] = np.minimum(out[px], (tmp[px].astype(np.uint64) << np.uint64(32)) | np.uint64(i))
        tmp[px] = mesh_ref.EMPTY
    return out


def _camera_points(P, verts, idx):
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)[idx]
    return [(P[a] * v[:, 0] + (P[4 + a] * v[:, 1] + P[8 + a] * v[:, 2])) + P[12 + a] for a in range(3)]


def evaluate(pose16, verts, tris, depth_u16, prob_u16, K, depth_scale, max_distance=0.02, min_view_cos=0.0, class_threshold=0.10, **_):
    """one evaluation (steps 1-5) -> dict: keys (H*W uint64), state (H*W uint8), sums (29 float64), mag (29: the sums of the products'
    magnitudes, for the rounding bound), A (count x 6) and b (count) of the counted pixels in pixel order"""
    depth = np.ascontiguousarray(depth_u16, np.uint16)
    H, W = depth.shape
    P = np.asarray(pose16, F).reshape(16)
    key = keys(P, verts, tris, K, W, H)
    state = np.zeros(H * W, np.uint8)
    px = np.flatnonzero(key != EMPTY_KEY)
    fx, cx, fy, cy = (F(x) for x in K)
    T = np.asarray(tris, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        r, c = np.divmod(px, W)
        z = (key[px] >> np.uint64(32)).astype(np.uint32).view(F)
        t = (key[px] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        xn = (c.astype(F) - cx) / fx
        yn = (r.astype(F) - cy) / fy
        raw = depth.reshape(-1)[px]
        d = raw.astype(F) * F(depth_scale)
        p = [xn * z, yn * z, z]
        q = [xn * d, yn * d, d]
        e = [p[k] - q[k] for k in range(3)]
        D = e[0] * e[0] + (e[1] * e[1] + e[2] * e[2])
        A_, B_, C_ = (_camera_points(P, verts, T[t, j]) for j in range(3))
        u = [B_[k] - A_[k] for k in range(3)]
        w = [C_[k] - A_[k] for k in range(3)]
        m = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
        dot = lambda a, b: a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])
        s, mm, pp = dot(m, p), dot(m, m), dot(p, p)
        assert all(x.dtype == F for x in (D, s, mm, pp, d))
        md2 = F(max_distance) * F(max_distance)
        mc2 = F(min_view_cos) * F(min_view_cos)
        st = np.full(len(px), COUNTED, np.uint8)
        st[~(mm != F(0)) | (s * s < mc2 * (mm * pp))] = GRAZING          # later steps first: an earlier one overwrites
        st[D > md2] = TOO_FAR
        if prob_u16 is not None:
            cp = (np.ascontiguousarray(prob_u16, np.uint16).reshape(-1)[px].astype(np.float64) * (1.0 / 10000)).astype(F)
            st[cp < F(class_threshold)] = OFF_CLASS
        st[raw == 0] = NO_DEPTH
        state[px] = st
        k = st == COUNTED
        md = [x[k].astype(np.float64) for x in m]
        ln = np.sqrt(md[0] * md[0] + (md[1] * md[1] + md[2] * md[2]))
        sg = np.where(s[k] > F(0), -1.0, 1.0)
        n = [(sg * x) / ln for x in md]
        qd = [x[k].astype(np.float64) for x in q]
        pd = [x[k].astype(np.float64) for x in p]
        A = np.stack([qd[1] * n[2] - qd[2] * n[1], qd[2] * n[0] - qd[0] * n[2], qd[0] * n[1] - qd[1] * n[0], n[0], n[1], n[2]], axis=1).reshape(-1, 6)
        b = (n[0] * (qd[0] - pd[0]) + n[1] * (qd[1] - pd[1])) + n[2] * (qd[2] - pd[2])
    sums, mag = np.zeros(29), np.zeros(29)
    j = 0
    for i0 in range(6):
        for i1 in range(i0, 6):
            sums[j] = (A[:, i0] * A[:, i1]).sum(); mag[j] = np.abs(A[:, i0] * A[:, i1]).sum(); j += 1
    for i0 in range(6):
        sums[21 + i0] = (A[:, i0] * b).sum(); mag[21 + i0] = np.abs(A[:, i0] * b).sum()
    sums[27] = mag[27] = len(b)
    sums[28] = mag[28] = (b * b).sum()
    return dict(keys=key, state=state, sums=sums, mag=mag, A=A, b=b)


def sums_bound(ev):
    """7.1's bound on a double sum of `count` products: (count + 8) 2^-53 sum |products|"""
    return (ev["sums"][27] + 8) * 2.0 ** -53 * ev["mag"]


def solve6(A, b):
    """the 6x6 elimination with partial pivoting (first largest pivot) in the dtype of A; None when a pivot is below 1e-300"""
    A = A.copy(); b = b.copy()
    for c in range(6):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if np.abs(A[p, c]) < 1e-300:
            return None
        if p != c:
            A[[c, p]] = A[[p, c]]; b[[c, p]] = b[[p, c]]
        for r in range(c + 1, 6):
            f = A[r, c] / A[c, c]
            A[r, c:] -= f * A[c, c:]
            b[r] -= f * b[c]
    x = np.zeros(6, A.dtype)
    for r in range(5, -1, -1):
        x[r] = (b[r] - (A[r, r + 1:] * x[r + 1:]).sum()) / A[r, r]
    return x


def system_of(sums, dtype=np.float64):
    M = np.zeros((6, 6), dtype)
    j = 0
    for r in range(6):
        for c in range(r, 6):
            M[r, c] = M[c, r] = sums[j]; j += 1
    return M, np.asarray(sums[21:27], dtype)


def delta_of(x):
    """Delta = (Rz(gamma) Ry(beta) Rx(alpha), t) as a 4x4 in the dtype of x"""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    D = np.eye(4, dtype=x.dtype)
    D[:3, :3] = np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa], [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                          [-sb, cb * sa, cb * ca]], x.dtype)
    D[:3, 3] = x[3:]
    return D


def update_from_sums(pose16, sums, dtype=np.float64):
    """step 6 from given sums -> (the updated 3x4 [R | t] in `dtype` before the rounding to float, or None when frozen; cond(A^T A))"""
    if sums[27] < 6:
        return None, np.inf
    M, v = system_of(np.asarray(sums, dtype), dtype)
    x = solve6(M, v)
    if x is None:
        return None, np.inf
    T = np.asarray(pose16, F).reshape(4, 4).T.astype(dtype)
    return (delta_of(x) @ T)[:3, :], float(np.linalg.cond(M.astype(np.float64)))


def update_longdouble(pose16, ev):
    """step 6 in longdouble from the evaluation's rows (sums, solve and product) -> (3x4 before the rounding to float or None, cond)"""
    L = np.longdouble
    A, b = ev["A"].astype(L), ev["b"].astype(L)
    sums = np.zeros(29, L)
    j = 0
    for r in range(6):
        for c in range(r, 6):
            sums[j] = (A[:, r] * A[:, c]).sum(); j += 1
    for r in range(6):
        sums[21 + r] = (A[:, r] * b).sum()
    sums[27] = len(b)
    return update_from_sums(pose16, sums, L)


def apply_update(pose16, T34):
    """P <- (float)(Delta P): the twelve used entries replaced, the last row as it was"""
    out = np.asarray(pose16, F).reshape(16).copy()
    for c in range(4):
        for r in range(3):
            out[4 * c + r] = F(T34[r, c])
    return out


def record_of(ev, iterations=0, frozen=0):
    st = ev["state"]
    n = [int((st == k).sum()) for k in range(6)]
    cnt = n[COUNTED]
    rms = F(np.sqrt(F(ev["sums"][28] / cnt))) if cnt else F(0)
    return dict(present=sum(n[1:]), no_depth=n[NO_DEPTH], off_class=n[OFF_CLASS], too_far=n[TOO_FAR], grazing=n[GRAZING], counted=cnt,
                iterations=iterations, frozen=frozen, rms=rms)


def step(pose16, verts, tris, depth_u16, prob_u16, K, depth_scale, **prm):
    """one iteration on a float32 pose -> (the next float32 pose, the evaluation, frozen)"""
    ev = evaluate(pose16, verts, tris, depth_u16, prob_u16, K, depth_scale, **prm)
    if not pose_valid(pose16):
        return np.asarray(pose16, F).reshape(16).copy(), ev, True
    T34, _ = update_from_sums(pose16, ev["sums"])
    if T34 is None:
        return np.asarray(pose16, F).reshape(16).copy(), ev, True
    return apply_update(pose16, T34), ev, False


def refine(pose16, verts, tris, depth_u16, prob_u16, K, depth_scale, max_iterations=5, **prm):
    """stocs_refine_poses_visible for one pose -> (pose, record of the last evaluation, the poses after 0, 1, ... updates)"""
    P = np.asarray(pose16, F).reshape(16).copy()
    trail = [P.copy()]
    if not pose_valid(P):
        return P, dict((k, F(0) if k == "rms" else 0) for k in RECORD_FIELDS), trail
    if max_iterations == 0:
        return P, record_of(evaluate(P, verts, tris, depth_u16, prob_u16, K, depth_scale, **prm)), trail
    rec, its = None, 0
    for _ in range(max_iterations):
        Pn, ev, frozen = step(P, verts, tris, depth_u16, prob_u16, K, depth_scale, **prm)
        its += 0 if frozen else 1
        rec = record_of(ev, its, 1 if frozen else 0)
        if frozen:
            break
        P = Pn
        trail.append(P.copy())
    return P, rec, trail


def vertex_error(pose16, gt16, verts):
    """the largest distance between the mesh's vertices under the two poses, in float64"""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    A = np.asarray(pose16, F).reshape(4, 4).T.astype(np.float64)
    B = np.asarray(gt16, F).reshape(4, 4).T.astype(np.float64)
    return float(np.linalg.norm((v @ A[:3, :3].T + A[:3, 3]) - (v @ B[:3, :3].T + B[:3, 3]), axis=1).max())
