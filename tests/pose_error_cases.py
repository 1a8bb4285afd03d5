"""Seeded cases for the pose-error tests (tests/test_pose_error_cases_cpu.py checks that each holds what it is named for, without a GPU;
tests/test_pose_error_gpu.py runs the library on them).  A case is a model (M, 3) float32, estimates (n, 16) and ground truths (1 or n, 16),
column-major camera-frame poses.  The model sizes come from the sizes the header names for the kernel."""
import os
import re

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_sizes():
    """STOCS_POSE_ERROR_THREADS / _CHUNK / _TILE of include/stocs_hip.h"""
    txt = open(os.path.join(ROOT, "include", "stocs_hip.h")).read()
    return {k: int(re.search(r"#define\s+STOCS_POSE_ERROR_%s\s+(\d+)" % k, txt).group(1)) for k in ("THREADS", "CHUNK", "TILE")}


def model_sizes():
    """the issue's list, one below / at / one above every size the header names and every row count of a chunk (1 .. 4 rows of THREADS)"""
    k = kernel_sizes()
    s = {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097}
    for v in (k["THREADS"], k["CHUNK"], k["TILE"]):
        s |= {v - 1, v, v + 1}
    for r in range(1, k["CHUNK"] // k["THREADS"] + 1):
        s |= {r * k["THREADS"] - 1, r * k["THREADS"], r * k["THREADS"] + 1}
    return sorted(v for v in s if v >= 1)


def pose(R=None, t=(0, 0, 0)):
    P = np.eye(4)
    if R is not None:
        P[:3, :3] = R
    P[:3, 3] = t
    return P.T.reshape(16).astype(F)


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def random_pose(rng, t_scale=0.05, centre=(0.0, 0.0, 0.8)):
    return pose(rot(rng.normal(size=3), rng.uniform(0, 180)), np.asarray(centre) + rng.normal(0, t_scale, 3))


def random_model(M, seed=0, scale=0.06):
    """an object-sized cloud (metres): points on a bumpy ellipsoid"""
    rng = np.random.default_rng(1000 + seed + M)
    d = rng.normal(size=(M, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * np.array([1.0, 0.7, 0.45]) * scale * (1 + 0.1 * rng.uniform(size=(M, 1)))).astype(F)


def random_pairs(n, seed, near=False):
    """n estimates and n ground truths; near: the estimate is the ground truth disturbed by a few degrees and millimetres"""
    rng = np.random.default_rng(seed)
    gt = np.stack([random_pose(rng) for _ in range(n)])
    if not near:
        return np.stack([random_pose(rng) for _ in range(n)]), gt
    est = []
    for g in gt:
        G = g.reshape(4, 4).T.astype(np.float64)
        D = np.eye(4); D[:3, :3] = rot(rng.normal(size=3), rng.uniform(0, 5)); D[:3, 3] = rng.normal(0, 0.003, 3)
        est.append((G @ D).T.reshape(16).astype(F))
    return np.stack(est), gt


def lattice(n, h):
    """n^3 lattice centred on the origin, spacing h (a power of two: every coordinate and every difference is exact); x fastest"""
    a = (np.arange(n) - (n - 1) / 2.0) * h
    z, y, x = np.meshgrid(a, a, a, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(F)


def lattice_quarter_turn(n=5, h=2.0 ** -6):
    """lattice cube turned a quarter about z: the matrix holds 0 and +-1 only, so the cube maps onto itself exactly.  ADD is large, ADD-S is
    exactly 0, nn is the permutation (x, y, z) -> (-y, x, z)"""
    m = lattice(n, h)
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    ix = np.arange(n ** 3); x, y, z = ix % n, (ix // n) % n, ix // (n * n)
    perm = (z * n + x) * n + (n - 1 - y)    # point (x, y, z) lands on lattice site (n - 1 - y, x, z)
    t = (0.0, 0.0, 0.75)
    return dict(model=m, est=pose(R, t)[None], gt=pose(None, t)[None], perm=perm.astype(np.int32))


def ring_turn(K=12, radius=0.05):
    """K-gon ring turned by 360 / K degrees about its axis: maps onto itself up to float32 rounding of the corners and of the matrix"""
    a = 2 * np.pi * np.arange(K) / K
    m = np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(K)], axis=1).astype(F)
    return dict(model=m, est=pose(rot((0, 0, 1), 360.0 / K))[None], gt=pose()[None], perm=((np.arange(K) + 1) % K).astype(np.int32), radius=radius)


def duplicate_points(M=130, seed=3):
    """every point of the first half again in the second half, bit for bit: every minimum is attained at least twice, nn is the lower index"""
    half = random_model(M // 2, seed)
    est, gt = random_pairs(1, seed + 1, near=True)
    return dict(model=np.concatenate([half, half]), est=est, gt=gt)


def lattice_midpoints(ways, n=4, h=2.0 ** -5):
    """lattice under a shift of half a spacing along 1, 2 or 3 axes: an inner query is equally far from 2, 4 or 8 lattice points, exactly"""
    axes = {2: (1, 0, 0), 4: (1, 1, 0), 8: (1, 1, 1)}[ways]
    return dict(model=lattice(n, h), est=pose(None, np.asarray(axes) * (h / 2))[None], gt=pose()[None], ways=ways, h=h, n=n)


def millimetres(M=300, seed=5):
    """a model in millimetres (coordinates of tens), poses with translations of hundreds"""
    m = (random_model(M, seed).astype(np.float64) * 1000).astype(F)
    rng = np.random.default_rng(seed)
    mk = lambda: pose(rot(rng.normal(size=3), rng.uniform(0, 180)), (rng.normal(0, 50), rng.normal(0, 50), 800 + rng.normal(0, 50)))
    return dict(model=m, est=np.stack([mk(), mk()]), gt=np.stack([mk(), mk()]))


def far_from_origin(M=300, seed=6):
    """model coordinates 3 m from the origin: the rotations swing the cloud metres around, differences of millimetres ride on metres"""
    m = (random_model(M, seed).astype(np.float64) + np.array([3.0, -3.0, 3.0])).astype(F)
    est, gt = random_pairs(2, seed, near=True)
    return dict(model=m, est=est, gt=gt)


def nan_point(M=63, at=17, seed=7):
    """one model point is NaN: it never wins anybody's minimum, and its own row is +inf / -1.  63 points: from 64 points on a context sizes
    a field over the scene by the model's patch spheres, which a NaN point turns into NaN, and refuses the model"""
    m = random_model(M, seed); m[at] = np.nan
    est, gt = random_pairs(1, seed)
    return dict(model=m, est=est, gt=gt, at=at)


def far_apart(M=70, seed=8):
    """poses 10^6 m apart: every distance is beyond the 32 768 m saturation of the fixed-point sums"""
    est, gt = random_pairs(1, seed)
    est[0, 12] += F(1.0e6)
    return dict(model=random_model(M, seed), est=est, gt=gt)


def overflow(M=70, seed=9):
    """finite entries of 10^30: products of 10^28, squares that overflow to +inf, inf - inf = NaN further on; nothing faults, and the
    poses are valid (every entry is finite)"""
    est, gt = random_pairs(2, seed)
    est[0, 0] = est[0, 5] = F(1.0e30)     # the estimate blows up, the ground truth does not
    est[1, 13] = F(1.0e30); gt[1, 13] = F(-1.0e30)
    return dict(model=random_model(M, seed), est=est, gt=gt)


def invalid_poses(M=70, seed=10):
    """pairs 0-3 invalid (NaN in the estimate's rotation, +inf in the ground truth's translation, -inf in the estimate's translation, the
    all-zero estimate); pairs 4-6 valid: NaN only in the entries that are not among the twelve, a zero rotation with a translation, the
    all-zero GROUND TRUTH"""
    est, gt = random_pairs(7, seed)
    est[0, 5] = np.nan
    gt[1, 14] = np.inf
    est[2, 12] = -np.inf
    est[3, :] = 0
    est[4, 3] = np.nan; est[4, 15] = np.nan; gt[4, 7] = np.inf
    est[5, :12] = 0
    gt[6, :] = 0
    return dict(model=random_model(M, seed), est=est, gt=gt, valid=np.array([0, 0, 0, 0, 1, 1, 1], np.int32))


def diameter_tie():
    """the eight corners of a cube (its four space diagonals tie for the maximum, exactly) plus inner points"""
    h = 2.0 ** -4
    corners = lattice(2, 2 * h)
    inner = (random_model(40, 11).astype(np.float64) * 0.3).astype(F)
    return dict(model=np.concatenate([inner[:20], corners, inner[20:]]), d2=F(12.0) * F(h) * F(h))
