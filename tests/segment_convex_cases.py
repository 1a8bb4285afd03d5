"""Cases for stocs_segment_frame_convex: a small ray-caster (a tilted support plane, spheres and boxes standing on it, axis-aligned in the
plane's frame, millimetre quantisation, seeded Gaussian depth noise) and hand-built label frames (plane_hypotheses = 0: every non-zero pixel is
foreground) placed where the bend kernels can go wrong.  Depths are uint16 millimetres (depth_scale 0.001)."""
import numpy as np

import segment_cases as sc

F = np.float32
SCALE = sc.SCALE
LABEL = dict(sc.LABEL, min_pixels=3)         # jump_abs 5 mm, jump_rel 0: a slope of up to 5 mm per pixel joins
SIZES = list(sc.SIZES) + [(160, 120)]


# ---- the ray-caster
def plane_frame(tilt_deg, dist):
    """the support plane n.X + d = 0 of segment_cases.table_frame and an orthonormal frame on it: origin O on the optical axis, u along the
    image's x, v away from the camera, n up (towards the camera's side)"""
    t = np.deg2rad(tilt_deg)
    n = np.array([0.0, -np.sin(t), -np.cos(t)])
    u = np.array([1.0, 0.0, 0.0])
    v = np.cross(n, u)
    return n, dist * np.cos(t), np.array([0.0, 0.0, dist]), u, v


def raycast(W, H, spheres=(), boxes=(), tilt_deg=55.0, dist=0.9, wall_z=2.5, noise_mm=0.0, seed=0):
    """spheres: (cu, cv, radius), resting on the plane; boxes: (u0, u1, v0, v1, height), standing on it; plane coordinates in metres.  Returns
    depth (uint16), K and the object image: -1 wall, 0 table, k = 1 .. for the spheres then the boxes."""
    K = sc.camera(W, H)
    n, d, O, u, v = plane_frame(tilt_deg, dist)
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack([(jj - K[1]) / K[0], (ii - K[3]) / K[2], np.ones((H, W))], axis=-1)
    nr = ray @ n
    with np.errstate(all="ignore"):
        t = np.where(nr < 0, -d / nr, np.inf)
        obj = np.zeros((H, W), np.int32)
        k = 0
        for (cu, cv, rad) in spheres:
            k += 1
            c = O + cu * u + cv * v + rad * n
            b, rr = ray @ c, (ray * ray).sum(-1)
            disc = b * b - rr * (c @ c - rad * rad)
            ts = np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0))) / rr, np.inf)
            hit = ts < t
            t, obj = np.where(hit, ts, t), np.where(hit, k, obj)
        o = np.array([-O @ u, -O @ v, -O @ n])
        dl = np.stack([ray @ u, ray @ v, ray @ n], axis=-1)
        for (u0, u1, v0, v1, h) in boxes:
            k += 1
            lo, hi = np.array([u0, v0, 0.0]), np.array([u1, v1, h])
            ta, tb = (lo - o) / dl, (hi - o) / dl
            tn, tf = np.minimum(ta, tb).max(-1), np.maximum(ta, tb).min(-1)
            hit = (tn <= tf) & (tn > 0) & (tn < t)
            t, obj = np.where(hit, tn, t), np.where(hit, k, obj)
    wall = t > wall_z
    z = np.where(wall, wall_z, t)
    obj = np.where(wall, -1, obj)
    z = z + np.random.default_rng(seed).normal(0.0, 1.0, z.shape) * noise_mm * 1e-3
    return np.clip(np.rint(z / SCALE), 1, 65535).astype(np.uint16), K, obj


# the scenes of the GPU tests (metres on the plane); test_segment_convex_cases_cpu.py holds the restatement to what they are named for first
SCENES = {
    "two_spheres": dict(spheres=((-0.06, 0.0, 0.06), (0.06, 0.0, 0.06))),
    "box_behind_box": dict(boxes=((-0.07, 0.07, -0.08, 0.0, 0.05), (-0.07, 0.07, 0.0, 0.09, 0.14))),
    "lone_sphere": dict(spheres=((0.0, 0.0, 0.07),)),
    "lone_box": dict(boxes=((-0.06, 0.06, -0.05, 0.05, 0.09),)),
}
SCENE_SIZE = (160, 120)
SCENE_PARAMS = dict(min_pixels=60, seed=5)
NOISES = (0.0, 1.0, 2.0)


def scene(name, noise_mm=0.0, size=SCENE_SIZE, seed=3):
    return raycast(size[0], size[1], noise_mm=noise_mm, seed=seed, **SCENES[name])


def purity(labels, obj):
    """per kept segment: (label, pixels, the object that holds most of them, the share of the segment on that object)"""
    out = []
    for k in range(1, int(labels.max()) + 1):
        ids, n = np.unique(obj[labels == k], return_counts=True)
        out.append((k, int(n.sum()), int(ids[n.argmax()]), float(n.max()) / float(n.sum())))
    return out


# ---- label frames
def valley(W, H, col=None, row=None, slope=4, top=500, on_pixel=False):
    """a V-shaped valley: the depth falls by `slope` mm per pixel either side of a crease that lies between columns col - 1 | col (or rows
    row - 1 | row; on_pixel: on column col itself); the crease is the farthest line, so the bend opens towards the camera"""
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    k = 0 if on_pixel else 1
    dist = np.abs(2 * jj - (2 * col - k)) if col is not None else np.abs(2 * ii - (2 * row - k))          # twice the distance to the crease
    return (top - (slope * dist) // 2).astype(np.uint16)


def ridge(W, H, col, slope=4, base=300):
    """the valley upside down: the crease is the nearest line, the bend opens away from the camera"""
    jj, _ = np.meshgrid(np.arange(W), np.arange(H))
    return (base + (slope * np.abs(2 * jj - (2 * col - 1))) // 2).astype(np.uint16)


def hole_and_jump(W, H):
    """a flat frame at 1000 mm with a zero-depth pixel at (4, 6) and, right of column W // 2, a second level 300 mm behind: windows near
    either hold pixels that must not count.  Returns depth and the pixels (row, col) to look at."""
    d = sc.blank(W, H, 1000)
    d[:, W // 2:] = 1300
    d[::2, :] += 2                                  # rows differ, so a wrong window shows in the mean
    d[4, 6] = 0
    return d, [(4, 5), (5, 6), (3, 7), (6, W // 2 - 1), (6, W // 2)]


def far_pixel_pair(W, H, r):
    """two flat frames at 1000 mm that differ in one pixel (row 5, col 9 + r): in the first its depth is the largest that still passes the
    r-scaled jump test against 1000 mm under LABEL (smooth_radius 0), in the second one raw unit more.  Returns (at, above, the centre (5, 9))."""
    zc, lim = F(1000) * F(SCALE), F(r) * (F(LABEL["jump_abs"]) + F(LABEL["jump_rel"]) * F(1000) * F(SCALE))
    raw = 1000
    while np.abs(F(raw + 1) * F(SCALE) - zc) <= lim:
        raw += 1
    at, above = sc.blank(W, H, 1000), sc.blank(W, H, 1000)
    at[5, 9 + r], above[5, 9 + r] = raw, raw + 1
    return at, above, (5, 9)


def label_frames(W, H):
    """name -> (depth, convex parameters): every hand-built frame that fits W x H"""
    out = {}
    for r, s in ((1, 0), (8, 4), (4, 2)):
        cv = dict(bend_radius=r, smooth_radius=s)
        tag = "r%ds%d" % (r, s)
        if W > 2 * r + 2:
            col = 64 if W > 64 + r else W // 2
            out["valley-col-" + tag] = (valley(W, H, col=col), cv)
            out["ridge-" + tag] = (ridge(W, H, col), cv)
            out["valley-border-" + tag] = (valley(W, H, col=r - 1, top=900, on_pixel=True), cv)
        if H > 2 * r + 2:
            out["valley-row-" + tag] = (valley(W, H, row=16 if H > 16 + r else H // 2), cv)
    out["hole-jump-s4"] = (hole_and_jump(W, H)[0], dict(bend_radius=1, smooth_radius=4))
    out["hole-jump-s0"] = (hole_and_jump(W, H)[0], dict(bend_radius=8, smooth_radius=0))
    if W > 9 + 8:
        for r in (1, 8):
            at, above, _ = far_pixel_pair(W, H, r)
            out["far-at-r%d" % r] = (at, dict(bend_radius=r, smooth_radius=0))
            out["far-above-r%d" % r] = (above, dict(bend_radius=r, smooth_radius=0))
    out["blobs-r4s2"] = (sc.blobs(W, H, W + H), dict(bend_radius=4, smooth_radius=2))
    return out
