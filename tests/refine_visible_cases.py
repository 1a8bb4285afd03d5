"""Seeded cases of the visible-surface refinement, shared by the CPU tests (the restatement against itself) and the GPU tests (the
library against the restatement): small frames (at most 128 x 96) rendered by mesh_ref at a known pose G, and perturbed starts.  Meshes,
cameras and pose helpers are mesh_cases' and vsd_cases' own."""
import numpy as np

import mesh_cases as mc
import mesh_ref
import vsd_cases as vc

F = np.float32
SCALE = vc.DEPTH_SCALE
POW2_SCALE = 2.0 ** -13                    # a depth unit that is a power of two: raw * scale is exact


class Case:
    """mesh, camera, frame (depth, prob or None), the pose G the frame was rendered at, the start pose, parameters"""
    def __init__(self, name, verts, tris, K, W, H, depth, prob, G16, start16, depth_scale=SCALE, **prm):
        self.name, self.verts, self.tris, self.K, self.W, self.H = name, np.ascontiguousarray(verts, F), np.ascontiguousarray(tris, np.int32), K, W, H
        self.depth, self.prob, self.G16, self.start16, self.depth_scale, self.prm = depth, prob, np.asarray(G16, F), np.asarray(start16, F), depth_scale, prm

    def args(self):
        return self.verts, self.tris, self.depth, self.prob, self.K, self.depth_scale

    def __repr__(self):
        return self.name


def pose_at(axis, deg, t):
    T = np.eye(4)
    T[:3, :3] = vc.rot(axis, deg)
    T[:3, 3] = t
    return T


def perturbed(G, axis, deg, dt):
    """Delta G with Delta a small motion in the camera frame about the object's position"""
    G = np.asarray(G, np.float64)
    D = np.eye(4)
    D[:3, :3] = vc.rot(axis, deg)
    D[:3, 3] = G[:3, 3] - D[:3, :3] @ G[:3, 3] + np.asarray(dt, np.float64)
    return D @ G


def frame_of(G16, verts, tris, K, W, H, wall=0.0, depth_scale=SCALE):
    """the depth image of the mesh at G in raw units; wall > 0: a wall at that depth wherever the mesh is not"""
    z = mesh_ref.render_depth(np.asarray(G16, F)[None], verts, tris, K, W, H)[0].astype(np.float64)
    if wall > 0:
        z = np.where(z > 0, z, wall)
    return vc.raw_from_depth(z, depth_scale)


def solids():
    return {"ellipsoid2": mc.ellipsoid(2, (0.08, 0.05, 0.03)), "ellipsoid1": mc.ellipsoid(1, (0.07, 0.05, 0.03)), "box": mc.box(0.12, 0.09, 0.06)}


def convergence_cases():
    """starts a few millimetres and degrees off G on noise-free frames: the restatement brings the vertex error below a tenth"""
    out = []
    specs = [("ellipsoid2", 128, 96, (1.0, 0.4, -0.3), 35.0, (0.012, -0.008, 0.80), (0.3, 1.0, 0.2), 2.0, (0.003, -0.002, 0.004), 0.0),
             ("ellipsoid1", 96, 72, (0.2, -1.0, 0.5), 50.0, (-0.01, 0.006, 0.78), (1.0, 0.1, -0.4), -1.5, (-0.002, 0.003, -0.003), 1.0),
             ("box", 128, 96, (0.5, 1.0, 0.3), 40.0, (0.005, 0.004, 0.82), (-0.2, 0.3, 1.0), 2.5, (0.002, 0.002, -0.004), 0.0)]
    for name, W, H, ax, deg, t, pax, pdeg, dt, wall in specs:
        v, tr = solids()[name]
        K = vc.small_camera(W, H)
        G = pose_at(ax, deg, t)
        G16 = vc.pose16(G)
        depth = frame_of(G16, v, tr, K, W, H, wall)
        out.append(Case("converge_" + name, v, tr, K, W, H, depth, None, G16, vc.pose16(perturbed(G, pax, pdeg, dt)), max_iterations=8, max_distance=0.02))
    return out


def class_image(W, H, seed, lo=0, hi=2001):
    return np.random.default_rng(seed).integers(lo, hi, (H, W)).astype(np.uint16)


def state_cases():
    """one case per state class, named for it: the class is hit (and the others need not be)"""
    v, tr = solids()["ellipsoid2"]
    W, H = 96, 72
    K = vc.small_camera(W, H)
    G = pose_at((1.0, 0.4, -0.3), 35.0, (0.004, -0.003, 0.80))
    G16 = vc.pose16(G)
    start = vc.pose16(perturbed(G, (0, 1, 0), 1.0, (0.001, 0.0, 0.002)))
    base = frame_of(G16, v, tr, K, W, H)
    out = {}
    out["counted"] = Case("state_counted", v, tr, K, W, H, base, None, G16, start)
    d = base.copy(); d[H // 2 - 3: H // 2 + 3, :] = 0
    out["no_depth"] = Case("state_no_depth", v, tr, K, W, H, d, None, G16, start)
    out["off_class"] = Case("state_off_class", v, tr, K, W, H, base, class_image(W, H, 5), G16, start, class_threshold=0.1)
    d = base.copy(); d[:, : W // 2] = np.where(d[:, : W // 2] > 0, d[:, : W // 2] - 600, 0).astype(np.uint16)   # an occluder 6 cm in front
    out["too_far"] = Case("state_too_far", v, tr, K, W, H, d, None, G16, start, max_distance=0.02)
    out["grazing"] = Case("state_grazing", v, tr, K, W, H, base, None, G16, start, min_view_cos=0.5)
    return out


def degenerate_case():
    """A facet whose normal has no length in float: a triangle of 2^-69 m around the optical axis at z = 1, in front of a plain one at
    z = 1.125.  Under K_EXACT the ray of pixel (0, 0) is the axis, the edge values there are denormal but not zero, so the facet wins
    that pixel; m = (0, 0, 2^-136) and m.m underflows to 0.  Frame: the plain triangle's depth everywhere it is."""
    e = 2.0 ** -70
    v = np.array([(-e, -e, 1.0), (e, -e, 1.0), (0.0, e, 1.0), (-0.05, -0.04, 1.125), (0.6, -0.03, 1.125), (-0.02, 0.5, 1.125)], F)
    t = np.array([[3, 4, 5], [0, 1, 2]], np.int32)
    W, H = 64, 48
    depth = frame_of(mc.IDENTITY, v, t[:1], mc.K_EXACT, W, H, depth_scale=POW2_SCALE)
    return Case("degenerate_facet", v, t, mc.K_EXACT, W, H, depth, None, mc.IDENTITY, mc.IDENTITY, depth_scale=POW2_SCALE, max_distance=0.25)


def duplicated(verts, tris, which, front):
    """the mesh with triangle `which` a second time: in front of all others (index 0) or behind them (the last index)"""
    t = np.asarray(tris, np.int32).reshape(-1, 3)
    dup = t[which: which + 1]
    return verts, np.ascontiguousarray(np.concatenate([dup, t]) if front else np.concatenate([t, dup]), np.int32)
