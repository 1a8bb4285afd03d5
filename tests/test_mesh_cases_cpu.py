"""The triangle rasteriser's contract on its own (tests/mesh_ref.py, no library): the surface it draws against the analytic solid, the
clamped box against testing every pixel, pinholes, and the independence from winding and triangle order."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_cases as mc  # noqa: E402
import mesh_ref as ref  # noqa: E402
import vsd_cases as vc  # noqa: E402
from model_matching_amd import synth  # noqa: E402

F = np.float32
SURFEL_MEDIAN_MM = 0.672      # profiles/vsd.md: the 6 mm surfels' median depth error on Cm's 5 000 points, the figure to beat


def _erode4(mask):
    m = mask.copy()
    m[1:, :] &= mask[:-1, :]; m[:-1, :] &= mask[1:, :]; m[:, 1:] &= mask[:, :-1]; m[:, :-1] &= mask[:, 1:]
    m[0, :] = m[-1, :] = False; m[:, 0] = m[:, -1] = False
    return m


def test_icosphere_is_closed_and_make_model_mesh_sits_on_the_cloud():
    for level, nt in ((0, 20), (1, 80), (3, 1280)):
        v, t = synth.icosphere(level)
        assert t.shape == (nt, 3) and len(v) == nt // 2 + 2 and np.allclose(np.linalg.norm(v, axis=1), 1.0)
        e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
        fwd = {(int(a), int(b)) for a, b in e}
        assert len(fwd) == len(e) and all((b, a) in fwd for a, b in fwd)          # every edge once in each direction
    for level, nt in ((3, 1600), (4, 6400), (0, 40)):
        v, t = synth.make_model_mesh(level)
        assert t.shape == (nt, 3) and v.dtype == F and t.dtype == np.int32 and t.min() == 0 and t.max() == len(v) - 1
    pos = synth.make_model(5000).pos
    v, _ = synth.make_model_mesh(4)
    assert np.all(np.abs(v.min(axis=0) - pos.min(axis=0)) < 0.002) and np.all(np.abs(v.max(axis=0) - pos.max(axis=0)) < 0.002)


def test_surface_quality_on_the_level_4_cm_mesh():
    """against the float64 ray-cast of the solid at VGA under the ground-truth pose: watertight inside the silhouette eroded by one
    pixel (4-neighbours: the inscribed mesh is smaller than the solid by a sagitta of about 0.05 mm, 0.07 pixels), nothing outside it
    (inscribed), and a median depth error below the surfels'"""
    v, t = mc.cm_mesh(4)
    W, H = 640, 480
    T = synth.gt_pose()
    z = ref.bits_to_depth(ref.render_bits(vc.pose16(T), v, t, vc.YCB_K, W, H), W, H)
    centre = vc.cm_ellipsoid_centre(synth.make_model(5000).pos)
    za = vc.cm_analytic_depth(T, centre, vc.YCB_K, W, H)
    sil = za > 0
    assert sil.sum() > 30000
    holes = int((_erode4(sil) & (z == 0)).sum())
    outside = int(((z > 0) & ~sil).sum())
    both = sil & (z > 0)
    err_mm = np.abs(z[both].astype(np.float64) - za[both]) * 1e3
    print("level 4: holes %d, outside %d, depth error median %.3f p99 %.3f max %.3f mm over %d pixels"
          % (holes, outside, np.median(err_mm), np.percentile(err_mm, 99), err_mm.max(), both.sum()))
    assert holes == 0
    assert outside == 0
    assert np.median(err_mm) < SURFEL_MEDIAN_MM


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_box_rule_equals_every_pixel_rule_and_leaves_no_pinhole(level):
    """seeded random poses of an ellipsoid on 96 x 72: the clamped box never cuts a hit pixel, and no empty pixel lies between two hit
    ones of its row or of its column (the ellipsoid's image is convex, so such a pixel would be a hole in the surface)"""
    W, H = 96, 72
    K = vc.small_camera(W, H)
    v, t = mc.ellipsoid(level)
    P = mc.random_poses(3, 40 + level, z=0.5, spread=0.03)
    for i in range(len(P)):
        zb = ref.render_bits(P[i], v, t, K, W, H)
        assert np.array_equal(zb, ref.render_bits(P[i], v, t, K, W, H, every_pixel=True))
        hit = (zb != ref.EMPTY).reshape(H, W)
        assert hit.sum() > 300
        for m in (hit, hit.T):
            first = np.argmax(m, axis=1); last = m.shape[1] - 1 - np.argmax(m[:, ::-1], axis=1)
            span = (np.arange(m.shape[1])[None, :] >= first[:, None]) & (np.arange(m.shape[1])[None, :] <= last[:, None]) & m.any(axis=1)[:, None]
            assert not (span & ~m).any()


@pytest.fixture(scope="module")
def wound():
    """the level-2 Cm mesh on 96 x 72 under two seeded poses, with its restatement's z-buffers (read-only)"""
    W, H = 96, 72
    K = vc.small_camera(W, H)
    v, t = mc.cm_mesh(2)
    P = mc.random_poses(2, 77, z=0.6)
    want = [ref.render_bits(P[i], v, t, K, W, H) for i in range(2)]
    for z in want:
        assert (z != ref.EMPTY).sum() > 300
        z.setflags(write=False)
    return dict(W=W, H=H, K=K, v=v, t=t, P=P, want=want)


def test_triangle_order_changes_no_bit(wound):
    g = wound
    rng = np.random.default_rng(5)
    for i in range(2):
        assert np.array_equal(ref.render_bits(g["P"][i], g["v"], g["t"][rng.permutation(len(g["t"]))], g["K"], g["W"], g["H"]), g["want"][i])


def test_reversed_winding_gives_the_same_bits(wound):
    """(i0, i2, i1): nA, nB, nC become -nA, -nC, -nB exactly, so u, v, w become -u, -w, -v; det = -(u + (w + v)) and the numerator of z
    -(u A_2 + (w C_2 + v B_2)) differ from the first winding's only by the order inside one addition, which IEEE addition does not see,
    and by a sign that the division cancels: the same bits, also with every second triangle alone reversed"""
    g = wound
    half = g["t"].copy(); half[::2] = half[::2][:, [0, 2, 1]]
    for i in range(2):
        for t in (g["t"][:, [0, 2, 1]], half):
            assert np.array_equal(ref.render_bits(g["P"][i], g["v"], t, g["K"], g["W"], g["H"]), g["want"][i])


def test_another_first_corner_hits_the_same_pixels(wound):
    """which corner a triangle starts with is not its winding: (i1, i2, i0) and (i2, i0, i1) permute u, v, w exactly, so the inside test
    and det != 0 answer alike and the same pixels are hit, in either winding; det and z are then summed in another order, and their last
    bits may differ (measured here: 175 to 202 of about 800 pixels, by at most 2 ulp).  The bound on that: inside a triangle u, v, w
    have one sign, so nothing cancels; det and z's numerator are two additions each on the same terms, within 2 * 2^-24 of their exact
    sums in either order, so within 4 * 2^-24 of each other; their quotient within 8 * 2^-24, and its own rounding adds 2^-24 on either
    side: 10 * 2^-24 relative, at most 10 ulp (an ulp is at least 2^-24 of its value).  A pixel's minimum over triangles keeps the bound"""
    g = wound
    for i in range(2):
        for perm in ([1, 2, 0], [2, 0, 1], [2, 1, 0], [1, 0, 2]):
            got = ref.render_bits(g["P"][i], g["v"], g["t"][:, perm], g["K"], g["W"], g["H"])
            assert np.array_equal(got != ref.EMPTY, g["want"][i] != ref.EMPTY)
            hit = got != ref.EMPTY
            assert np.abs(got[hit].astype(np.int64) - g["want"][i][hit].astype(np.int64)).max() <= 10


def test_a_ray_exactly_on_a_shared_edge_is_hit_through_both_triangles():
    """fx = fy = 64, cx = cy = 0, vertices at z = 1 with x = c / 64: the edge from (8, 2) to (8, 12) runs through the pixel centres of
    column 8, where its edge value is exactly 0 in both triangles, whichever way each walks the edge"""
    W, H = 16, 16
    at = lambda c, r, z=1.0: (c / 64.0 * z, r / 64.0 * z, z)
    left = mc.triangle(at(8, 2), at(8, 12), at(2, 7))
    right = mc.triangle(at(8, 2), at(8, 12), at(14, 7))
    right_rev = mc.triangle(at(8, 12), at(8, 2), at(14, 7))
    for tri in (left, right, right_rev):
        g = ref.setup(mc.IDENTITY, tri[0], tri[1], mc.K_EXACT, W, H)
        xn, yn = F(8.0 / 64.0), F(5.0 / 64.0)
        assert xn * g["nC"][0][0] + (yn * g["nC"][1][0] + g["nC"][2][0]) == 0      # nC = A x B: the shared edge's value at pixel (5, 8)
        z = ref.bits_to_depth(ref.render_bits(mc.IDENTITY, tri[0], tri[1], mc.K_EXACT, W, H), W, H)
        assert np.all(z[2:13, 8] == 1.0) and z[1, 8] == 0 and z[13, 8] == 0
    zl = ref.render_bits(mc.IDENTITY, *left, mc.K_EXACT, W, H) != ref.EMPTY
    zr = ref.render_bits(mc.IDENTITY, *right, mc.K_EXACT, W, H) != ref.EMPTY
    both = (zl & zr).reshape(H, W)
    assert np.array_equal(np.argwhere(both), np.array([(r, 8) for r in range(2, 13)]))


def test_skip_rules():
    W, H = 16, 16
    at = lambda c, r, z=1.0: (c / 64.0 * z, r / 64.0 * z, z)
    n_hit = lambda tri, P=mc.IDENTITY: int((ref.render_bits(P, tri[0], tri[1], mc.K_EXACT, W, H) != ref.EMPTY).sum())
    assert n_hit(mc.triangle(at(2, 2), at(12, 2), at(2, 12))) > 40
    assert n_hit(mc.triangle(at(2, 2), at(12, 2), (0.1, 0.1, float(F(1e-6))))) == 0       # z == 1e-6f exactly: not above it
    assert n_hit(mc.triangle(at(2, 2), at(12, 2), (0.1, 0.1, -0.5))) == 0
    assert n_hit(mc.triangle(at(-30, 2), at(-20, 2), at(-30, 12))) == 0                   # off the left side
    bad = mc.IDENTITY.copy(); bad[13] = np.nan
    assert n_hit(mc.triangle(at(2, 2), at(12, 2), at(2, 12)), bad) == 0
    assert n_hit(mc.triangle(at(2, 2), at(12, 2), at(2, 12)), np.zeros(16, F)) == 0
