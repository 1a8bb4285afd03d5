"""float32 numpy restatement of the joint-rendering contract written at stocs_render_poses in include/stocs_hip.h: the splat rule, the
key buffer, resolve and labels.  Steps 1-3 come from depth_check_ref.point_flags (self-occlusion off: facing, in_image, p_2, col, row),
the classification restates the expressions of steps 5-6 there with p_2 := the float in the key's high word.  Written from the contract,
not from the kernels; the GPU tests compare the library's key buffers, records, labels and states with it for equality.  No GPU, numpy
only."""
import numpy as np

import depth_check_ref as dref

F = np.float32
COUNTS = ("footprint", "visible", "hidden", "no_depth", "agree", "in_front", "behind", "on_mask")
DTYPE = np.dtype([(k, np.int32) for k in COUNTS])
DEFAULTS = dict(point_radius=0.005, max_splat_px=8, tolerance=0.01, class_threshold=0.10)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _prm(params):
    prm = dict(DEFAULTS); prm.update(params)
    return prm


def empty_keys(W, H):
    return np.full(H * W, EMPTY, np.uint64)


def touched(pose16, model_pos, model_unit_nrm, K, W, H, **params):
    """the splat rule for one pose -> (pixel index, key high word) of every (point, touched pixel) pair, duplicates included"""
    prm = _prm(params)
    blank = np.zeros((H, W), np.uint16)
    f = dref.point_flags(pose16, model_pos, model_unit_nrm, blank, None, K, 1.0, self_occlusion=0)
    sel = f["in_image"]
    z, col, row = f["z"][sel], f["col"][sel], f["row"][sel]
    if len(z) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.uint32)
    fr = F(K[0]) * F(prm["point_radius"])
    with np.errstate(all="ignore"):
        s = np.minimum(np.floor(fr / z + F(0.5)), F(prm["max_splat_px"]))
    assert s.dtype == F
    s = s.astype(np.int64)
    pix, hi = [], []
    smax = int(s.max())
    for dy in range(-smax, smax + 1):                        # offset by offset: the points whose square reaches it
        for dx in range(-smax, smax + 1):
            r, c = row + dy, col + dx
            ok = (s >= max(abs(dy), abs(dx))) & (r >= 0) & (r < H) & (c >= 0) & (c < W)
            pix.append(r[ok] * W + c[ok]); hi.append(z[ok].view(np.uint32))
    return np.concatenate(pix), np.concatenate(hi)


def render(zkey, poses16, model_pos, model_nrm, K, W, H, id_base=0, clear=False, **params):
    """stocs_render_poses on a flat uint64 key buffer of W*H (in place; returned)"""
    P = np.asarray(poses16, F).reshape(-1, 16)
    k = dref.unit_normals(model_nrm)
    if clear and len(P):
        zkey[:] = EMPTY
    for h in range(len(P)):
        pix, hi = touched(P[h], model_pos, k, K, W, H, **params)
        key = (hi.astype(np.uint64) << np.uint64(32)) | np.uint64(id_base + h)
        np.minimum.at(zkey, pix, key)
    return zkey


def classify(zkey, depth_u16, prob_u16, depth_scale, **params):
    """per pixel of the key buffer -> uint8 state: 0 empty, 1 no_depth, 2 agree, 3 in_front, 4 behind, + 16 on_mask"""
    prm = _prm(params)
    tol, thr = F(prm["tolerance"]), F(prm["class_threshold"])
    empty = zkey == EMPTY
    z = (zkey >> np.uint64(32)).astype(np.uint32).view(F)
    raw = depth_u16.reshape(-1)
    zo = raw.astype(F) * F(depth_scale)
    with np.errstate(all="ignore"):
        d = z - zo
    assert d.dtype == F
    have = ~empty & (raw != 0)
    state = np.zeros(len(zkey), np.uint8)
    state[~empty & (raw == 0)] = 1
    with np.errstate(all="ignore"):
        agree = have & (np.abs(d) <= tol)
        state[agree] = 2
        state[have & (d < -tol)] = 3
        state[have & (d > tol)] = 4
    if prob_u16 is not None:
        cp = (prob_u16.reshape(-1).astype(np.float64) * (1.0 / 10000)).astype(F)
        state[agree & ~(cp < thr)] += 16
    return state


def resolve(zkey, poses16, model_pos, model_nrm, depth_u16, prob_u16, K, depth_scale, id_base=0, **params):
    """stocs_render_resolve -> records of DTYPE"""
    H, W = depth_u16.shape
    P = np.asarray(poses16, F).reshape(-1, 16)
    k = dref.unit_normals(model_nrm)
    state = classify(zkey, depth_u16, prob_u16, depth_scale, **params)
    low = (zkey & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out = np.zeros(len(P), DTYPE)
    for h in range(len(P)):
        pix, _ = touched(P[h], model_pos, k, K, W, H, **params)
        C = np.unique(pix)
        vis = (low[C] == id_base + h) & (zkey[C] != EMPTY)
        st = state[C][vis]
        out[h] = (len(C), int(vis.sum()), int((~vis).sum()), int(((st & 15) == 1).sum()), int(((st & 15) == 2).sum()), int(((st & 15) == 3).sum()),
                  int(((st & 15) == 4).sum()), int(((st & 16) != 0).sum()))
    return out


def labels(zkey, depth_u16, prob_u16, depth_scale, **params):
    """stocs_render_labels -> (labels int32 (H, W), state uint8 (H, W))"""
    H, W = depth_u16.shape
    lab = np.where(zkey == EMPTY, np.int64(-1), (zkey & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    return lab.reshape(H, W), classify(zkey, depth_u16, prob_u16, depth_scale, **params).reshape(H, W)


def explain(poses16, model_pos, model_nrm, depth_u16, prob_u16, K, depth_scale, **params):
    """stocs_explain_poses -> (records, labels, state, key buffer)"""
    H, W = depth_u16.shape
    zkey = render(empty_keys(W, H), poses16, model_pos, model_nrm, K, W, H, 0, True, **params)
    rec = resolve(zkey, poses16, model_pos, model_nrm, depth_u16, prob_u16, K, depth_scale, 0, **params)
    lab, st = labels(zkey, depth_u16, prob_u16, depth_scale, **params)
    return rec, lab, st, zkey


def records_equal(a, b):
    """array_equal on the eight counts"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and all(np.array_equal(a[c], b[c]) for c in COUNTS)
