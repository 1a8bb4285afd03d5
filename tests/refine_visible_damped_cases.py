"""Seeded cases of the damped visible-surface refinement, shared by the CPU tests (the restatement alone) and the GPU tests (the library
against the restatement): refine_visible_cases' own cases, the analytic Cm frame on which the plain form fails (the level-4 mesh against a
ray-cast of the solid, so the frame is not the mesh's own image), and small frames built to hit a rejection, each bound and each pivot."""
import functools

import numpy as np

import mesh_cases as mc
import refine_visible_cases as rc
import vsd_cases as vc
from model_matching_amd import synth

F = np.float32
CM_WALL = 1.2
CM_T = (0.01, -0.005, 0.80)
# (axis, degrees, translation) of refine_visible_cases.perturbed: 4 degrees and 10 mm off the pose of the frame.  Chosen with the plain
# restatement (tests/test_refine_visible_damped_cases_cpu.py asserts it): 5 plain iterations end at more than five times the start's ADD.
CM_STARTS = [((-0.51, -0.84, -0.16), 4.0, (0.0035, 0.0093, 0.0009)), ((-0.45, -0.64, 0.62), -4.0, (0.0079, 0.0013, -0.006))]


def cm_pose():
    T = synth.gt_pose().copy()
    T[:3, 3] = CM_T
    return T


@functools.lru_cache(maxsize=None)
def cm_frame(W, H):
    """the analytic Cm frame under vsd_cases.small_camera(W, H): raw depth (a wall behind the solid, 0.1 mm unit), the camera"""
    K = vc.small_camera(W, H)
    za = vc.cm_analytic_depth(cm_pose(), vc.cm_ellipsoid_centre(synth.make_model(5000).pos), K, W, H)
    return vc.raw_from_depth(np.where(za > 0, za, CM_WALL), vc.DEPTH_SCALE), K, int((za > 0).sum())


def cm_case(start, W=160, H=120, level=4, **prm):
    """the Cm case at one start (axis, degrees, translation)"""
    v, t = synth.make_model_mesh(level)
    depth, K, _ = cm_frame(W, H)
    G = cm_pose()
    ax, deg, dt = start
    return rc.Case("cm_%dx%d_l%d" % (W, H, level), v, t, K, W, H, depth, None, vc.pose16(G), vc.pose16(rc.perturbed(G, ax, deg, dt)), **prm)


def cm_points():
    return synth.make_model(5000).pos


def pivot_of(case):
    """the Python layer's default pivot: the mean of the mesh's vertices"""
    return tuple(float(x) for x in np.asarray(case.verts, np.float64).reshape(-1, 3).mean(axis=0).astype(F))


def with_prm(case, name, **prm):
    """the case under other parameters"""
    return rc.Case(name, case.verts, case.tris, case.K, case.W, case.H, case.depth, case.prob, case.G16, case.start16, case.depth_scale, **dict(case.prm, **prm))


def small_cm_case(W, H, start, level=2, name=None, **prm):
    """a Cm frame small enough for a GPU test: the level-`level` mesh against the analytic frame"""
    c = cm_case(start, W, H, level, **prm)
    c.name = name or c.name
    return c


INF = float("inf")
PLAIN_LIKE = dict(lambda0=0.0, max_step_rotation=INF, max_step_translation=INF, pivot=0)
NO_BOUNDS = dict(max_step_rotation=INF, max_step_translation=INF)
LOST_PIXELS = [2919, 3013, 3404, 3512, 3784, 3896]   # six counted pixels of state_cases()["counted"] at its start


def lost_pixels_case():
    """refine_visible_cases' counted case with a measurement on six pixels alone: the undamped, unbounded step from them is so large
    that the trial counts no pixel (the CPU tests assert it): C = +inf, rejected, the start comes back"""
    case = rc.state_cases()["counted"]
    d = np.zeros(case.W * case.H, np.uint16)
    d[LOST_PIXELS] = case.depth.reshape(-1)[LOST_PIXELS]
    return rc.Case("lost_pixels", case.verts, case.tris, case.K, case.W, case.H, d.reshape(case.H, case.W), None, case.G16, case.start16, max_iterations=2,
                   **dict(PLAIN_LIKE, pivot_model=(0.0, 0.0, 0.0)))


def five_pixels_case():
    """the same with five of the six: fewer than 6 counted pixels at e = 0"""
    case = lost_pixels_case()
    d = case.depth.copy().reshape(-1)
    d[LOST_PIXELS[-1]] = 0
    return rc.Case("five_pixels", case.verts, case.tris, case.K, case.W, case.H, d.reshape(case.H, case.W), None, case.G16, case.start16, max_iterations=2)


def feature_cases():
    """name -> case (parameters complete, pivot_model included): the convergence cases under the defaults about the mesh's centre, a 40 x 30
    frame (G = 1), a rejection with lambda0 = 0, each bound, both pivots with a pivot_model off the origin, a class image"""
    out = {}
    for c in rc.convergence_cases():
        out[c.name] = with_prm(c, c.name, pivot_model=pivot_of(c))
    cm = small_cm_case(128, 96, CM_STARTS[0], level=2, max_distance=0.02, max_iterations=6)
    out["cm_small_frame"] = with_prm(small_cm_case(40, 30, CM_STARTS[0], level=2, max_distance=0.02, max_iterations=6), "cm_small_frame", pivot_model=pivot_of(cm))
    out["cm_rejection"] = with_prm(cm, "cm_rejection", lambda0=0.0, pivot_model=pivot_of(cm), **NO_BOUNDS)
    out["cm_rotation_bound"] = with_prm(cm, "cm_rotation_bound", max_iterations=3, max_step_rotation=0.005, max_step_translation=INF, pivot_model=pivot_of(cm))
    out["cm_translation_bound"] = with_prm(cm, "cm_translation_bound", max_iterations=3, max_step_rotation=INF, max_step_translation=0.001, pivot_model=pivot_of(cm))
    box = rc.convergence_cases()[2]
    off = (0.03, -0.02, 0.01)
    out["box_pivot_camera"] = with_prm(box, "box_pivot_camera", max_iterations=4, pivot=0, pivot_model=off)
    out["box_pivot_off_origin"] = with_prm(box, "box_pivot_off_origin", max_iterations=4, pivot=1, pivot_model=off)
    st = rc.state_cases()["off_class"]
    out["class_image"] = with_prm(st, "class_image", max_iterations=4, pivot_model=pivot_of(st))
    return out
