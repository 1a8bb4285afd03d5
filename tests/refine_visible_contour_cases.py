"""Seeded cases of the contour term of the visible-surface refinement, shared by the CPU tests (the restatement alone) and the GPU tests (the
library against the restatement).  Every frame carries a class image.  Flat cases live under mesh_cases.K_EXACT (pixel (r, c) looks along
(c / 64, r / 64, 1)), so that silhouettes and rectangles are known by construction: quads whose grown rectangle has a chosen width and
height, single-pixel seeds for the tie rule, a quad over a frame corner.  Solid cases are refine_visible_cases' ellipsoid in front of a
wall, and the capture case: a box displaced across the rays by more than its projected width."""
import numpy as np

import mesh_cases as mc
import refine_visible_cases as rc
import refine_visible_contour_ref as cref
import vsd_cases as vc

F = np.float32
FULL = np.uint16(10000)
WIDE = (144, 80)        # 11 520 pixels (below 128 x 96 = 12 288) and wide enough for a grown rectangle of 129 columns


def quad(c_lo, c_hi, r_lo, r_hi, z=1.0):
    """two triangles at depth z whose projection under K_EXACT covers the pixel centres c_lo .. c_hi x r_lo .. r_hi exactly"""
    x0, x1, y0, y1 = (c_lo - 0.25) / 64, (c_hi + 0.25) / 64, (r_lo - 0.25) / 64, (r_hi + 0.25) / 64
    v = np.array([(x0 * z, y0 * z, z), (x1 * z, y0 * z, z), (x1 * z, y1 * z, z), (x0 * z, y1 * z, z)], F)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def seeds(pixels, z=1.0):
    """one small triangle around each pixel centre (r, c): it covers that pixel alone"""
    v, t = [], []
    for r, c in pixels:
        k = len(v)
        v += [((c - 0.3) / 64 * z, (r - 0.3) / 64 * z, z), ((c + 0.3) / 64 * z, (r - 0.3) / 64 * z, z), (c / 64 * z, (r + 0.3) / 64 * z, z)]
        t.append([k, k + 1, k + 2])
    return np.array(v, F), np.array(t, np.int32)


def flat_frame(W, H, z=1.0, far=None, far_z=1.25):
    """a plane at depth z over the whole frame (raw units of POW2_SCALE), pixels of the boolean image `far` at far_z instead; every pixel an
    object pixel"""
    d = np.full((H, W), z)
    if far is not None:
        d[far] = far_z
    return vc.raw_from_depth(d, rc.POW2_SCALE), np.full((H, W), FULL, np.uint16)


def flat_case(name, v, t, W, H, R, far=None, hole=None, **prm):
    depth, prob = flat_frame(W, H, far=far)
    if hole is not None:
        prob = prob.copy(); prob[hole] = 0
    return rc.Case(name, v, t, mc.K_EXACT, W, H, depth, prob, mc.IDENTITY, mc.IDENTITY, depth_scale=rc.POW2_SCALE,
                   **dict(dict(pull_radius_px=R, pull_distance=0.05, max_distance=0.02), **prm))


def width_case(width, height, R=2, c_start=5, r_start=3):
    """a quad whose rectangle grown by R is `width` x `height` pixels and starts at column c_start, row r_start (not clamped): the run and
    tile boundaries of the contour kernel.  The right fifth of the frame lies at 1.25 m: beyond."""
    W, H = WIDE
    c0, r0 = c_start + R, r_start + R                  # the rectangle is the silhouette's box grown by two pixels: measured below
    v, t = quad(c0 + 2, c0 + width - 2 * R - 3, r0 + 2, r0 + height - 2 * R - 3)
    far = np.zeros((H, W), bool); far[:, W - W // 5:] = True
    case = flat_case("grown_%dx%d_R%d" % (width, height, R), v, t, W, H, R, far=far)
    rect = cref.rectangle(mc.IDENTITY, v, t, mc.K_EXACT, W, H)
    er0, er1, ec0, ec1 = cref.grown(rect, R, W, H)
    assert (ec1 - ec0 + 1, er1 - er0 + 1, ec0, er0) == (width, height, c_start, r_start), (rect, width, height)
    return case


def width_cases():
    return [width_case(w, h) for w, h in ((63, 15), (64, 16), (65, 17), (128, 33), (129, 32))]


TIE_SEEDS = [(20, 30), (20, 36),          # a row: (20, 33) lies between them
             (40, 50), (46, 50),          # a column: (43, 50)
             (30, 80), (34, 84),          # a diagonal: (32, 82); (30, 84) and (34, 80) tie too
             (60, 20), (60, 21)]          # neighbours: no pixel between them


def tie_case(R=8):
    v, t = seeds(TIE_SEEDS)
    return flat_case("ties", v, t, 128, 96, R)


def corner_case(R=16):
    """a quad over the upper left corner of the frame, and one in the lower right corner: the window is cut by each edge and both corners"""
    W, H = 128, 96
    va, ta = quad(-6, 9, -4, 7)
    vb, tb = quad(W - 9, W + 4, H - 6, H + 3)
    hole = np.zeros((H, W), bool); hole[10:14, 12:20] = True        # not object pixels: not walked
    return flat_case("corners", np.concatenate([va, vb]), np.concatenate([ta, tb + 4]), W, H, R, hole=hole)


def solid_case(R, wall=1.2):
    """refine_visible_cases' ellipsoid at its perturbed start, a wall behind it, every pixel an object pixel: the wall is beyond, the ring
    of the solid that the start does not cover is pulled"""
    c = rc.state_cases()["counted"]
    depth = rc.frame_of(c.G16, c.verts, c.tris, c.K, c.W, c.H, wall)
    start = vc.pose16(rc.perturbed(np.asarray(c.G16, np.float64).reshape(4, 4).T, (0, 1, 0), 2.0, (0.006, -0.004, 0.002)))
    return rc.Case("solid_R%d" % R, c.verts, c.tris, c.K, c.W, c.H, depth, np.full((c.H, c.W), FULL, np.uint16), c.G16, start, pull_radius_px=R, pull_distance=0.03,
                   max_distance=0.02)


def detail_cases():
    """name -> case for the per-pixel comparison"""
    out = dict((c.name, c) for c in width_cases())
    out.update(dict((c.name, c) for c in (solid_case(1), solid_case(2), solid_case(16), solid_case(64), tie_case(), corner_case())))
    return out


def silhouette_class(depth):
    """the class image of an object alone in the frame: full where there is a measurement"""
    return np.where(np.asarray(depth) > 0, FULL, np.uint16(0)).astype(np.uint16)


CAPTURE_DX = 0.09       # m across the rays: 23 pixels at 0.8 m under small_camera(128, 96); the box's silhouette is 18 pixels wide
CAPTURE_PRM = dict(max_iterations=12, max_distance=0.02, pull_radius_px=48, pull_distance=0.12, max_step_translation=0.02, pivot_model=(0.0, 0.0, 0.0))
# Recorded with the restatement (tests/test_refine_visible_contour_cases_cpu.py asserts them): the start's corner error is 0.0900 m; the
# damped restatement counts no pixel and returns the start frozen; the contour restatement accepts 12 of 12 trials and ends at 0.0409 m.


def capture_case(**prm):
    W, H = 128, 96
    v, t = mc.box(0.06, 0.045, 0.03)
    K = vc.small_camera(W, H)
    G = rc.pose_at((0.5, 1.0, 0.3), 40.0, (0.0, 0.0, 0.80))
    depth = rc.frame_of(vc.pose16(G), v, t, K, W, H)
    S = G.copy(); S[0, 3] += CAPTURE_DX
    return rc.Case("capture", v, t, K, W, H, depth, silhouette_class(depth), vc.pose16(G), vc.pose16(S), **dict(CAPTURE_PRM, **prm))


def small_solid_case(**prm):
    """the ellipsoid alone in the frame with its true silhouette as the class image, from the perturbed start: a few updates with pulls"""
    c = rc.state_cases()["counted"]
    s = solid_case(16)
    return rc.Case("solid_alone", c.verts, c.tris, c.K, c.W, c.H, c.depth, silhouette_class(c.depth), c.G16, s.start16,
                   **dict(dict(max_iterations=4, max_distance=0.02, pull_radius_px=16, pull_distance=0.03, pivot_model=(0.0, 0.0, 0.0)), **prm))
