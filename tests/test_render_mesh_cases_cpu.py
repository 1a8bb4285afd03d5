"""The restatement of the mesh forms of the joint renderer (tests/render_mesh_ref.py) on cases whose answer is known without it: order
independence, the id rule, footprints and overlaps of face-on boxes counted by hand, no pinholes in a closed surface, and the splat mask
of the same box as a strict superset of the mesh mask.  No GPU: numpy only."""
import os
import sys

import numpy as np

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_cases as mc  # noqa: E402
import render_mesh_ref as ref  # noqa: E402
import render_ref as rref  # noqa: E402
import vsd_cases as vc  # noqa: E402

F = np.float32
SCALE = float(2.0 ** -10)        # raw 1024 is exactly 1 m
W, H = 64, 48
K = (64.0, 32.0, 64.0, 24.0)     # the optical axis through pixel (24, 32); a point at depth z, x = k z / 64 lies k columns right of it
PRM = dict(tolerance=float(2.0 ** -7), class_threshold=0.1)
WALL = np.full((H, W), 1024, np.uint16)
# a box whose front face, face-on at depth 1, covers the pixel centres of columns 22 .. 42 and rows 16 .. 32 exactly (edges inclusive)
BOX = mc.box(20 / 64, 16 / 64, 0.25)


def face_on(front_z, dx_px=0, dy_px=0, depth=0.25):
    """the pose that puts the front face of a box of that depth at front_z, shifted by whole pixels at that depth"""
    return vc.pose16(vc.translation(dx_px * front_z / 64, dy_px * front_z / 64, front_z + depth / 2))


def test_keys_do_not_depend_on_the_order_of_the_poses():
    v, t = mc.ellipsoid(2)
    Kc = vc.small_camera(W, H)
    E = mc.random_poses(5, 7, z=0.8, spread=0.02)
    want = ref.render(ref.empty_keys(W, H), E, v, t, Kc, W, H, 10, True)
    assert (want != ref.EMPTY).sum() > 100 and len(np.unique(want[want != ref.EMPTY] & np.uint64(0xFFFFFFFF))) > 1
    for order in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
        z = ref.empty_keys(W, H)
        for h in order:                                                      # one call per pose, each under its own id
            ref.render(z, E[h], v, t, Kc, W, H, 10 + h)
        assert np.array_equal(z, want)
    z = ref.render(ref.render(ref.empty_keys(W, H), E[3:], v, t, Kc, W, H, 13), E[:3], v, t, Kc, W, H, 10)   # two batches, the later ids first
    assert np.array_equal(z, want)


def test_the_same_pose_under_two_ids_goes_to_the_lower():
    v, t = BOX
    P = face_on(1.0)
    for first, second in ((3, 8), (8, 3)):
        z = ref.render(ref.render(ref.empty_keys(W, H), P, v, t, K, W, H, first), P, v, t, K, W, H, second)
        assert set((z[z != ref.EMPTY] & np.uint64(0xFFFFFFFF)).tolist()) == {3}
        lo = ref.resolve(z, P, v, t, WALL, None, K, SCALE, 3, **PRM)[0]
        hi = ref.resolve(z, P, v, t, WALL, None, K, SCALE, 8, **PRM)[0]
        assert lo["hidden"] == 0 and lo["visible"] == lo["footprint"] > 0
        assert hi["hidden"] == hi["footprint"] == lo["footprint"] and hi["visible"] == 0


def test_a_face_on_box_alone_owns_its_rectangle():
    v, t = BOX
    rec, lab, st, zkey = ref.explain(face_on(1.0), v, t, WALL, None, K, SCALE, **PRM)
    assert rec["footprint"][0] == 21 * 17 == rec["visible"][0] == rec["agree"][0] and rec["hidden"][0] == 0
    want = np.full((H, W), -1, np.int32); want[16:33, 22:43] = 0
    assert np.array_equal(lab, want)
    assert set((zkey[zkey != ref.EMPTY] >> np.uint64(32)).tolist()) == {int(np.array(1.0, F).view(np.uint32))}   # the front face, not the back
    rec, lab, _, _ = ref.explain(face_on(1.0, 8, 4), v, t, WALL, None, K, SCALE, **PRM)     # the axis still inside the box: no side shows
    want = np.full((H, W), -1, np.int32); want[20:37, 30:51] = 0
    assert rec["footprint"][0] == 21 * 17 and np.array_equal(lab, want)


def test_the_rear_box_is_hidden_on_the_overlap_rectangle():
    v, t = BOX
    near = face_on(1.0, 8, 4)                                                # columns 30 .. 50, rows 20 .. 36
    rear = face_on(2.0)                                                      # half the size in pixels: columns 27 .. 37, rows 20 .. 28
    rec, lab, _, _ = ref.explain([near, rear], v, t, WALL, None, K, SCALE, **PRM)
    assert rec["footprint"].tolist() == [21 * 17, 11 * 9]
    assert rec["hidden"].tolist() == [0, 8 * 9]                              # columns 30 .. 37 of rows 20 .. 28
    assert rec["visible"].tolist() == [21 * 17, 3 * 9] and (lab == 1).sum() == 27
    assert rec["agree"][0] == 21 * 17 and rec["behind"][1] == 27             # the wall is at 1 m, the rear face at 2
    rec2, _, _, _ = ref.explain([rear, near], v, t, WALL, None, K, SCALE, **PRM)
    assert ref.records_equal(rec2, rec[::-1])


def test_every_row_of_an_ellipsoid_is_one_run():
    v, t = mc.ellipsoid(2)
    Kc = vc.small_camera(W, H)
    for P in mc.random_poses(4, 21, z=0.8, spread=0.01):
        _, lab, _, _ = ref.explain(P, v, t, WALL, None, Kc, SCALE, **PRM)
        own = lab == 0
        assert own.sum() > 50
        for r in np.flatnonzero(own.any(axis=1)):
            c = np.flatnonzero(own[r])
            assert c[-1] - c[0] + 1 == len(c), (r, c)


def box_cloud(sx, sy, sz, h):
    """points on the six faces of mesh_cases.box on a grid of spacing <= h, corners included, with outward normals"""
    half = np.array([sx, sy, sz]) / 2
    pos, nrm = [], []
    for ax in range(3):
        u, w = [a for a in range(3) if a != ax]
        gu = np.linspace(-half[u], half[u], int(np.ceil(2 * half[u] / h)) + 1)
        gw = np.linspace(-half[w], half[w], int(np.ceil(2 * half[w] / h)) + 1)
        U, Wg = np.meshgrid(gu, gw)
        for sgn in (-1, 1):
            p = np.zeros((U.size, 3)); p[:, u] = U.reshape(-1); p[:, w] = Wg.reshape(-1); p[:, ax] = sgn * half[ax]
            n = np.zeros((U.size, 3)); n[:, ax] = sgn
            pos.append(p); nrm.append(n)
    return np.concatenate(pos).astype(F), np.concatenate(nrm).astype(F)


def test_the_splat_mask_is_a_strict_superset_of_the_mesh_mask():
    """the same face-on box as a 2 mm cloud under the default radius (5 mm: one pixel of padding at fx = 256, depth 1) and as its mesh"""
    Wb, Hb, Kb = 160, 120, (256.0, 80.0, 256.0, 60.0)
    size = (80 / 256, 64 / 256, 0.25)                                        # the front face: columns 40 .. 120, rows 28 .. 92
    v, t = mc.box(*size)
    pos, nrm = box_cloud(*size, 0.002)
    P = vc.pose16(vc.translation(0, 0, 1.125))
    wall = np.full((Hb, Wb), 1024, np.uint16)
    _, lab_m, _, _ = ref.explain(P, v, t, wall, None, Kb, SCALE, **PRM)
    _, lab_s, _, _ = rref.explain(P, pos, nrm, wall, None, Kb, SCALE, **PRM)
    mesh, splat = lab_m == 0, lab_s == 0
    assert mesh.sum() == 81 * 65
    assert np.all(splat[mesh]) and splat.sum() > mesh.sum()
    assert splat.sum() == 83 * 67                                            # one pixel on every side (profiles/render_mesh.md)
