"""Seeded builders of models, poses, cameras and frames for the surfel renderer and VSD, shared by the CPU tests (the restatement alone)
and the GPU tests (the library against the restatement).  Everything is float32 as the library takes it; poses are column-major."""
import numpy as np

from model_matching_amd import synth

F = np.float32
YCB_K = tuple(float(v) for v in synth.YCB_INTRINSICS)
DEPTH_SCALE = 1.0e-4       # metres per depth unit: 0.1 mm, as the ycb example frames


def pose16(T):
    """a 4x4 (row-major, as numpy holds it) -> the 16 floats of the column-major pose"""
    return np.ascontiguousarray(np.asarray(T, np.float64).T.reshape(16), F)


def translation(x, y, z):
    T = np.eye(4); T[:3, 3] = (x, y, z)
    return T


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def small_camera(W, H):
    """a camera for a W x H image that sees a 0.1 m object at 0.8 m whole: the focal length scales with the width, the principal point is
    off the centre and off the pixel grid"""
    fx = 1.6 * W
    return (float(F(fx)), float(F(0.5 * W - 0.31)), float(F(fx * 1.0007)), float(F(0.5 * H + 0.23)))


def cm_model():
    m = synth.make_model(5000)
    return m.pos, m.nrm


def cm_pose():
    return pose16(synth.gt_pose())


def ball_model(M, seed, radius=0.04):
    """M points on a sphere with outward normals and a little noise on both"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(M, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    pos = (u * radius + rng.normal(0, 0.0005, (M, 3))).astype(F)
    n = u + rng.normal(0, 0.05, (M, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
    return pos, n.astype(F)


def ball_poses(n, seed, z=0.8, spread=0.01):
    """n poses of the ball model near the optical axis at depth z: random rotations, translations spread by `spread`"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 16), F)
    for i in range(n):
        T = np.eye(4)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = (rng.normal(0, spread), rng.normal(0, spread), z + rng.normal(0, spread))
        out[i] = pose16(T)
    return out


def raw_from_depth(z_img, depth_scale=DEPTH_SCALE, empty=0):
    """a depth image in metres -> uint16 raw values; 0 (no surface) -> `empty`"""
    z = np.asarray(z_img, np.float64)
    raw = np.clip(np.rint(z / depth_scale), 0, 65535).astype(np.uint16)
    raw[z <= 0] = empty
    return raw


def flat_frame(W, H, z, depth_scale=DEPTH_SCALE):
    """a wall at depth z (0: no measurement anywhere)"""
    return np.full((H, W), 0 if z <= 0 else int(round(z / depth_scale)), np.uint16)


def one_surfel(point, normal):
    """a model of one point"""
    return np.asarray([point], F), np.asarray([normal], F)


def cm_ellipsoid_centre(pos):
    """where the centre of synth.make_model's ellipsoid lies in the model frame (the model is centred on its points' mean, which the bump
    pulls off the ellipsoid's centre): a least-squares fit of the centre to the points away from the bump, in float64"""
    abc = np.array([0.08, 0.08, 0.03]); bc = np.array([0.05, 0.0, 0.02]); br = 0.02
    x = np.asarray(pos, np.float64)
    o = np.zeros(3)
    for _ in range(8):
        y = x - o
        r = ((y / abc) ** 2).sum(axis=1) - 1.0
        use = (np.linalg.norm(y - bc, axis=1) > br + 0.004) & (np.abs(r) < 0.1)
        J = -2.0 * y[use] / abc ** 2
        o = o + np.linalg.lstsq(J, -r[use], rcond=None)[0]
    return o


def cm_analytic_depth(T, centre, K, W, H):
    """float64 ray-cast of synth.make_model's solid (ellipsoid + spherical bump, centred at `centre` in the model frame) under the 4x4
    pose T through every pixel centre -> (H, W) depth z, 0 where the ray misses"""
    abc = np.array([0.08, 0.08, 0.03]); bc = np.array([0.05, 0.0, 0.02]); br = 0.02
    fx, cx, fy, cy = K
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    X, Y = np.meshgrid((np.arange(W) - cx) / fx, (np.arange(H) - cy) / fy)
    d = np.stack([X, Y, np.ones_like(X)], axis=-1).reshape(-1, 3) @ R          # R^T d per ray, as rows
    o = (-t) @ R - centre                                                     # the camera centre seen from the solid's centre
    best = np.full(len(d), np.inf)

    def first_root(A, B, Cc):
        disc = B * B - 4 * A * Cc
        with np.errstate(all="ignore"):
            s = (-B - np.sqrt(disc)) / (2 * A)
        return np.where((disc >= 0) & (s > 0), s, np.inf)

    de, oe = d / abc, o / abc
    best = np.minimum(best, first_root((de * de).sum(1), 2 * (de * oe).sum(1), (oe * oe).sum() - 1.0))
    ob = o - bc
    best = np.minimum(best, first_root((d * d).sum(1), 2 * (d * ob).sum(1), (ob * ob).sum() - br * br))
    return np.where(np.isfinite(best), best, 0.0).reshape(H, W)                # the ray is (xn, yn, 1): its parameter is z
