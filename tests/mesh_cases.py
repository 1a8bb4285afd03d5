"""Seeded builders of meshes, poses and cameras for the triangle rasteriser, shared by the CPU tests (the restatement alone) and the GPU
tests (the library against the restatement).  Vertices are float32 and triangles int32 as the library takes them; poses are column-major.
The cameras, pose helpers and frames are vsd_cases' own."""
import numpy as np

import vsd_cases as vc
from model_matching_amd import synth

F = np.float32
K_EXACT = (64.0, 0.0, 64.0, 0.0)           # fx = fy = 64, cx = cy = 0: a vertex at z = 1, x = c / 64 projects onto column c exactly
IDENTITY = vc.pose16(np.eye(4))


def ellipsoid(level, abc=(0.08, 0.08, 0.03)):
    """a closed icosphere of `level` (20 * 4^level triangles) scaled to an ellipsoid"""
    v, t = synth.icosphere(level)
    return np.ascontiguousarray(v * np.asarray(abc), F), t


def cm_mesh(level):
    return synth.make_model_mesh(level)


def box(sx, sy, sz):
    """a closed box of 8 vertices and 12 triangles, outward winding, centred on the origin"""
    v = np.array([(x, y, z) for z in (-sz, sz) for y in (-sy, sy) for x in (-sx, sx)], F) * F(0.5)
    q = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = np.array([f for a, b, c, d in q for f in ((a, b, c), (a, c, d))], np.int32)
    return v, t


def triangle(a, b, c):
    """a mesh of one triangle"""
    return np.array([a, b, c], F), np.array([[0, 1, 2]], np.int32)


def random_poses(n, seed, z=0.8, spread=0.02):
    """n poses near the optical axis at depth z: random rotations, translations spread by `spread`"""
    return vc.ball_poses(n, seed, z=z, spread=spread)


def grid_of_small_triangles(n, px_w, px_h, K, W, z=1.0):
    """n separate triangles in a row-major grid, each with a clamped box of exactly px_w x px_h pixels under the identity pose: the
    projections span px_w - 3 columns and px_h - 3 rows from a pixel centre plus a quarter (floor(min) - 1 .. floor(max) + 2)"""
    fx, cx, fy, cy = K
    per_row = max(1, (W - 2) // (px_w + 1))
    verts, tris = [], []
    for i in range(n):
        c0 = 1 + (i % per_row) * (px_w + 1) + 1.25
        r0 = 1 + (i // per_row) * (px_h + 1) + 1.25
        c1, r1 = c0 + (px_w - 4) + 0.5, r0 + (px_h - 4) + 0.5
        P = [((c - cx) / fx * z, (r - cy) / fy * z, z) for c, r in ((c0, r0), (c1, r0), (c0, r1))]
        tris.append([3 * i, 3 * i + 1, 3 * i + 2])
        verts += P
    return np.array(verts, F), np.array(tris, np.int32)
