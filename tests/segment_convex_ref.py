"""Float32 numpy restatement of steps 4a and 4b of stocs_segment_frame_convex (include/stocs_hip.h) on top of segment_ref: the smoothed depth,
the bend test per axis, and steps 5-7 of segment_ref run on the foreground minus the cut.  Every image and every count bit for bit; each
float step is one IEEE float32 operation, 3-term sums are e0 + (e1 + e2), a comparison with NaN is false."""
import numpy as np

import segment_ref as sr

F = np.float32
CONVEX_DEFAULTS = dict(bend_radius=4, smooth_radius=2, bend_cos=0.90630779)
COUNTS = ("n_tested_h", "n_tested_v", "n_cut_h", "n_cut_v", "n_cut")


def convex_params(**kw):
    cp = dict(CONVEX_DEFAULTS)
    for k in kw:
        assert k in cp, k
    cp.update(kw)
    return cp


def window_sums(raw, fg, depth_scale, jump_abs, jump_rel, s):
    """step 4a's integers: (S, N), int64 images; zero off the foreground"""
    raw = np.asarray(raw, np.uint16)
    H, W = raw.shape
    z = raw.astype(F) * F(depth_scale)
    ja, jr = F(jump_abs), F(jump_rel)
    S, N = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            y0, y1, x0, x1 = max(0, -dy), H - max(0, dy), max(0, -dx), W - max(0, dx)
            if y1 <= y0 or x1 <= x0:
                continue
            c, w = (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            with np.errstate(all="ignore"):
                ok = fg[c] & fg[w] & (np.abs(z[c] - z[w]) <= ja + jr * np.minimum(z[c], z[w]))
            S[c] += np.where(ok, raw[w].astype(np.int64), 0)
            N[c] += ok
    return S, N


def smoothed_points(raw, fg, K, depth_scale, jump_abs, jump_rel, s):
    """step 4a: (H, W, 3) float32 smoothed points (NaN off the foreground), S, N"""
    fx, cx, fy, cy = (F(v) for v in K)
    S, N = window_sums(raw, fg, depth_scale, jump_abs, jump_rel, s)
    H, W = fg.shape
    with np.errstate(all="ignore"):
        zs = np.where(fg, (S.astype(F) / N.astype(F)) * F(depth_scale), F(np.nan)).astype(F)
        jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        zd = zs.astype(np.float64)
        Ps = np.stack([((jj - np.float64(cx)) * zd / np.float64(fx)).astype(F), ((ii - np.float64(cy)) * zd / np.float64(fy)).astype(F), zs], axis=-1)
    return Ps, S, N


def dot3(a, b):
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def triple(Lp, Cp, Rp, r, jump_abs, jump_rel, bend_cos):
    """step 4b on arrays of smoothed points: dict(tested, toward, bend, cut, ab, aa, bb)"""
    ja, jr, rf = F(jump_abs), F(jump_rel), F(r)
    cos2 = F(bend_cos) * F(bend_cos)
    with np.errstate(all="ignore"):
        zl, zc, zr = Lp[..., 2], Cp[..., 2], Rp[..., 2]
        tested = (np.abs(zl - zc) <= rf * (ja + jr * np.minimum(zc, zl))) & (np.abs(zr - zc) <= rf * (ja + jr * np.minimum(zc, zr)))
        a, b, m = Cp - Lp, Rp - Cp, (Lp + Rp) - (Cp + Cp)
        ab, aa, bb = dot3(a, b), dot3(a, a), dot3(b, b)
        toward = dot3(m, Cp) < 0
        bend = (ab <= 0) | (ab * ab < cos2 * (aa * bb))
    return dict(tested=tested, toward=toward, bend=bend, cut=tested & toward & bend, ab=ab, aa=aa, bb=bb)


def bend(Ps, r, jump_abs, jump_rel, bend_cos):
    """step 4b over the frame: dict(tested_h, tested_v, cut_h, cut_v), bool images"""
    H, W, _ = Ps.shape
    out = {k: np.zeros((H, W), bool) for k in ("tested_h", "tested_v", "cut_h", "cut_v")}
    if r > 0 and W > 2 * r:
        t = triple(Ps[:, :-2 * r], Ps[:, r:-r], Ps[:, 2 * r:], r, jump_abs, jump_rel, bend_cos)
        out["tested_h"][:, r:-r], out["cut_h"][:, r:-r] = t["tested"], t["cut"]
    if r > 0 and H > 2 * r:
        t = triple(Ps[:-2 * r], Ps[r:-r], Ps[2 * r:], r, jump_abs, jump_rel, bend_cos)
        out["tested_v"][r:-r], out["cut_v"][r:-r] = t["tested"], t["cut"]
    return out


def convex_cut(raw, fg, K, depth_scale, p, cp):
    """steps 4a + 4b: dict(cut (uint8), smoothed (float32), Ps, S, N, the four masks, the five counts)"""
    Ps, S, N = smoothed_points(raw, fg, K, depth_scale, p["jump_abs"], p["jump_rel"], cp["smooth_radius"])
    b = bend(Ps, cp["bend_radius"], p["jump_abs"], p["jump_rel"], cp["bend_cos"])
    cut = (b["cut_h"].astype(np.uint8) | (b["cut_v"].astype(np.uint8) << 1)).astype(np.uint8)
    out = dict(b, cut=cut, smoothed=Ps[..., 2].copy(), Ps=Ps, S=S, N=N)
    out.update(n_tested_h=int(b["tested_h"].sum()), n_tested_v=int(b["tested_v"].sum()), n_cut_h=int(b["cut_h"].sum()), n_cut_v=int(b["cut_v"].sum()),
               n_cut=int((cut != 0).sum()))
    return out


def segment_frame_convex(depth_u16, K, depth_scale, plane=None, convex=None, **kw):
    """The whole call: segment_ref.segment_frame's dictionary with steps 5-7 run on the foreground minus the cut, plus cut, smoothed, the masks
    and the five counts; "plain" holds the dictionary of the call without the cut."""
    cp = convex_params(**(convex or {}))
    p = sr.params(**kw)
    plain = sr.segment_frame(depth_u16, K, depth_scale, plane=plane, **kw)
    c = convex_cut(depth_u16, plain["fg"], K, depth_scale, p, cp)
    left = plain["fg"] & (c["cut"] == 0)
    seg = sr.segments(plain["P"], left, None, p)          # no plane: its foreground is the mask it is given; steps 5-7 as they stand
    out = dict(plain)
    for k in ("n_components", "n_segments", "labels", "class_prob", "edge", "records", "root"):
        out[k] = seg[k]
    out.update(c, fg_left=left, plain=plain)
    return out
