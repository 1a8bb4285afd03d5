"""Seeded cases for the symmetry-aware pose-error tests (tests/test_pose_error_sym_cases_cpu.py checks that each holds what it is named
for, without a GPU; tests/test_pose_error_sym_gpu.py runs the library on them).  A case is a model (M, 3) float32, estimates (n, 16),
ground truths (1 or n, 16), symmetries (K, 16) -- all column-major -- and possibly a camera (fx, cx, fy, cy).  Built on the plain
pose-error cases (tests/pose_error_cases.py); the sizes come from the constants the header names for the kernel."""
import os
import re

import numpy as np

import pose_error_cases as pc

F = np.float32
ROOT = pc.ROOT
CAM = (600.0, 320.0, 600.0, 240.0)
CAM_OFF = (570.3, 12.5, 585.1, 471.25)     # principal point far off the centre
EPS_Z = F(1e-6)                             # the depth a point must exceed to project


def kernel_sizes():
    """STOCS_POSE_SYM_MAX / _THREADS / _BLOCK of include/stocs_hip.h"""
    txt = open(os.path.join(ROOT, "include", "stocs_hip.h")).read()
    return {k: int(re.search(r"#define\s+STOCS_POSE_SYM_%s\s+(\d+)" % k, txt).group(1)) for k in ("MAX", "THREADS", "BLOCK")}


def model_sizes():
    """the issue's list plus one below / at / one above every size the header names"""
    s = {1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1025, 4097}
    for v in kernel_sizes().values():
        s |= {v - 1, v, v + 1}
    return sorted(v for v in s if v >= 1)


def sym_counts():
    kb = kernel_sizes()["BLOCK"]
    return sorted({1, 2, kb - 1, kb, kb + 1, 2 * kb + 1, 72})


def xform(R=None, t=(0, 0, 0)):
    return pc.pose(R, t)


def turns(K, axis=(0, 0, 1), centre=(0, 0, 0)):
    """K turns of 360 / K degrees about the axis through centre, identity first"""
    c = np.asarray(centre, np.float64)
    out = []
    for k in range(K):
        R = pc.rot(axis, 360.0 * k / K) if k else np.eye(3)
        out.append(xform(R, c - R @ c))
    return np.stack(out)


def random_syms(K, seed):
    """identity first, then arbitrary small rigid motions of the model frame (the contract asks nothing of a symmetry but finite entries)"""
    rng = np.random.default_rng(seed)
    return np.stack([xform()] + [xform(pc.rot(rng.normal(size=3), rng.uniform(0, 180)), rng.normal(0, 0.01, 3)) for _ in range(K - 1)])


def compose64(g16, s16):
    """gt o symmetry in float64, rounded once (exact for the dyadic cases)"""
    G, S = np.asarray(g16, np.float64).reshape(4, 4).T, np.asarray(s16, np.float64).reshape(4, 4).T
    return (G @ S).T.reshape(16).astype(F)


def turned_estimates(gt, syms, seed, deg=3.0, mm=2.0):
    """estimate k = ground truth k composed with a random symmetry of the set, then disturbed by a few degrees and millimetres"""
    rng = np.random.default_rng(seed)
    out = []
    for g in np.asarray(gt, F).reshape(-1, 16):
        D = np.eye(4); D[:3, :3] = pc.rot(rng.normal(size=3), rng.uniform(0, deg)); D[:3, 3] = rng.normal(0, mm * 1e-3, 3)
        out.append(compose64(compose64(g, syms[rng.integers(len(syms))]), D.T.reshape(16)))
    return np.stack(out)


def random_case(M, K, n, seed, n_gt=None, cam=None):
    model = pc.random_model(M)
    syms = turns(K) if seed % 2 else random_syms(K, seed)
    _, gt = pc.random_pairs(n, seed)
    est = turned_estimates(gt, syms, seed + 1)
    if n_gt == 1:
        gt = gt[:1]
    return dict(model=model, est=est, gt=gt, syms=syms, cam=cam)


# ---- exact rotations: dyadic coordinates, quarter turns, dyadic translations: every product, sum and distance is exact ----
RZ = [np.array(r, np.float64) for r in ([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[-1, 0, 0], [0, -1, 0], [0, 0, 1]],
                                        [[0, 1, 0], [-1, 0, 0], [0, 0, 1]])]
RX90 = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)
GT_EXACT = xform(RX90, (0.125, -0.25, 0.75))


def quarter_turns():
    return np.stack([xform(R) for R in RZ])


def dyadic_model():
    """a lattice cube plus three points that break every symmetry"""
    return np.concatenate([pc.lattice(3, 2.0 ** -5), np.array([[0.125, 0, 0], [0.125, 0.0625, 0], [0, 0.03125, 0.25]], F)])


def exact_hit(j):
    """the estimate is the ground truth composed with quarter turn j: symmetry j (and only j) gives exactly 0"""
    syms = quarter_turns()
    return dict(model=dyadic_model(), est=compose64(GT_EXACT, syms[j])[None], gt=GT_EXACT[None], syms=syms, cam=CAM, k=j)


def exact_listed_twice():
    """[I, Rz90, Rz90, Rz180] and an estimate turned by Rz90: indices 1 and 2 tie at 0, the lower wins"""
    q = quarter_turns()
    syms = np.stack([q[0], q[1], q[1], q[2]])
    return dict(model=dyadic_model(), est=compose64(GT_EXACT, q[1])[None], gt=GT_EXACT[None], syms=syms, cam=CAM, k=1)


def exact_invariant_model():
    """points ON the axis of the set: every symmetry fixes every point, so all k tie (at 0 for est == gt, and at one exact non-zero value
    for a shifted estimate) and index 0 wins.  (A model that is invariant only as a SET does not tie: the measures pair a point with itself)"""
    z = (np.arange(9) - 4) * 2.0 ** -5
    model = np.stack([np.zeros(9), np.zeros(9), z], axis=1).astype(F)
    shifted = GT_EXACT.copy(); shifted[12] += F(0.0625)
    return dict(model=model, est=np.stack([GT_EXACT, shifted]), gt=GT_EXACT[None], syms=quarter_turns(), cam=CAM, shift=F(0.0625))


def exact_none_right(n=5, h=2.0 ** -6):
    """a lattice cube, the estimate a quarter turn off, the set {I, Rz180}: under either symmetry the estimate is a quarter turn from the
    ground truth, a corner (a, a) moves by exactly 2a: both k tie at 2a, index 0 wins"""
    q = quarter_turns()
    a = (n - 1) / 2.0 * h
    return dict(model=pc.lattice(n, h), est=compose64(GT_EXACT, q[1])[None], gt=GT_EXACT[None], syms=np.stack([q[0], q[2]]), cam=None, mssd=F(2 * a))


# ---- projection edges ----
def _axis_model():
    """the origin and points further along +z"""
    return np.array([[0, 0, 0], [0, 0, 0.25], [0.0625, 0, 0.5], [0, -0.0625, 0.5]], F)


def depth_edge_ground_truth():
    """ground truth = identity pose; the symmetries shift the model along z by 2^-10, EXACTLY 1e-6f, one ulp above it, 2^-10: the origin
    lands at those depths, so k = 1 fails `x_2 > 1e-6f` and its max2 is +inf; the others are finite"""
    above = np.nextafter(EPS_Z, F(1))
    syms = np.stack([xform(None, (0, 0, z)) for z in (F(2.0 ** -10), EPS_Z, above, F(2.0 ** -10))])
    return dict(model=_axis_model(), est=xform(None, (0, 0, 2.0 ** -10))[None], gt=xform()[None], syms=syms, cam=CAM, inf_k=[1])


def depth_edge_estimate():
    """pair 0: the estimate puts the origin at exactly 1e-6f: every k is +inf; pair 1: one ulp above: every k is finite"""
    above = np.nextafter(EPS_Z, F(1))
    syms = np.stack([xform(None, (0, 0, z)) for z in (F(2.0 ** -10), F(2.0 ** -9))])
    return dict(model=_axis_model(), est=np.stack([xform(None, (0, 0, EPS_Z)), xform(None, (0, 0, above))]), gt=xform()[None], syms=syms, cam=CAM)


def behind_camera():
    """the ground truth is a metre behind the camera under every symmetry"""
    return dict(model=pc.random_model(65), est=xform(None, (0, 0, 0.8))[None], gt=xform(None, (0, 0, -1.0))[None], syms=turns(5), cam=CAM)


def optical_axis():
    """model points on the z axis, poses that turn about z and move along z: every projection is the principal point, da = db = 0 exactly"""
    z = (np.arange(7) * 2.0 ** -5).astype(F)
    model = np.stack([np.zeros(7, F), np.zeros(7, F), z], axis=1)
    return dict(model=model, est=xform(RZ[1], (0, 0, 0.5))[None], gt=xform(None, (0, 0, 0.75))[None], syms=quarter_turns(), cam=CAM_OFF)


# ---- saturation and validity ----
def far_apart(M=70, seed=8):
    """a translation of 10^5 m: every distance is beyond the 32 768 m saturation of the fixed-point sums"""
    c = random_case(M, 3, 1, seed, cam=CAM)
    c["est"][0, 12] += F(1.0e5)
    return c


def invalid_poses(M=70, seed=10):
    """pairs 0, 2, 4, 6 valid; 1: NaN in the estimate, 3: +inf in the ground truth, 5: the all-zero estimate, 7: -inf in the estimate
    and NaN in the ground truth.  Every invalid pair sits between valid ones or at the end"""
    c = random_case(M, 9, 8, seed, cam=CAM)
    c["est"][1, 5] = np.nan
    c["gt"][3, 14] = np.inf
    c["est"][5, :] = 0
    c["est"][7, 12] = -np.inf; c["gt"][7, 0] = np.nan
    c["valid"] = np.array([1, 0, 1, 0, 1, 0, 1, 0], np.int32)
    return c
