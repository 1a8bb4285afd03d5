"""stocs_ctx_set_frame / stocs_depth_check_poses on the GPU against the float32 restatement of their contract (tests/depth_check_ref.py):
every comparison is array_equal on the eight counts and bit equality on the two floats.  Shapes are the smallest at which the kernel can
go wrong: models either side of a wavefront (63 / 64 / 65), of a 256-point round (255 / 256 / 257) and of several rounds (1 025);
points exactly on the contract's decision boundaries, built from representable floats; z-buffers whose stride stays at cell_px and
grows beyond it."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depth_check_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
APP = os.path.join(ROOT, "model_matching_amd", "apps", "stocs_single")
PRE = os.path.join(ROOT, "model_matching_amd", "apps", "model_preprocess")
F = np.float32
EPS = float(2.0 ** -7)          # tolerance and margin of the hand-built cases: a representable float
SCALE = float(2.0 ** -10)       # depth unit of the hand-built frames: raw 1024 is exactly 1 m
K64 = (32.0, 32.0, 32.0, 24.0)  # 64 x 48 camera, everything a power of two or a small integer


def _est(model_pos, model_nrm):
    """a context around a model; the scene plays no part in the depth check (a handful of points serves)"""
    from model_matching_amd.estimator import StocsEstimator
    rng = np.random.default_rng(1)
    sp = rng.normal(0, 0.05, (32, 3)).astype(F)
    sn = sp / np.linalg.norm(sp, axis=1, keepdims=True)
    return StocsEstimator(sp, sn, np.ones(32, F), None, np.asarray(model_pos, F).reshape(-1, 3), np.asarray(model_nrm, F).reshape(-1, 3), build_index=False)


class Case:
    """one context + frame; check() compares the library with the restatement and returns the records"""
    def __init__(self, mpos, mnrm, depth, prob, K, scale):
        self.mpos, self.mnrm, self.depth, self.prob, self.K, self.scale = np.asarray(mpos, F).reshape(-1, 3), np.asarray(mnrm, F).reshape(-1, 3), depth, prob, K, scale
        self.est = _est(self.mpos, self.mnrm)
        self.est.set_frame(depth, prob, K, scale)

    def check(self, poses, **prm):
        poses = np.asarray(poses, F).reshape(-1, 16)
        got = self.est.depth_check_poses(poses, **prm)
        want = ref.check_poses(poses, self.mpos, self.mnrm, self.depth, self.prob, self.K, self.scale, **prm)
        assert got.dtype.names == want.dtype.names
        bad = [i for i in range(len(poses)) if not ref.records_equal(got[i], want[i])]
        assert not bad, (bad[:5], got[bad[:5]], want[bad[:5]])
        return got


def _pose(R=None, t=(0, 0, 0)):
    P = np.eye(4)
    if R is not None:
        P[:3, :3] = R
    P[:3, 3] = t
    return P.T.reshape(16).astype(F)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def _counts(r):
    return tuple(int(r[c]) for c in ref.COUNTS)


def flat_frame(W, H, raw=1024):
    """a wall at raw depth units with a hole (no depth) at pixel (row 24, col 33) when it exists, and a class image that is exactly at
    the 0.1 threshold at the centre pixel (raw 1000), just below it one column to the left (999), 1.0 elsewhere"""
    depth = np.full((H, W), raw, np.uint16)
    prob = np.full((H, W), 10000, np.uint16)
    if W > 33 and H > 24:
        depth[24, 33] = 0
        prob[24, 32] = 1000
        prob[24, 31] = 999
    return depth, prob


# (name, translation, counts) for ONE model point at the origin with normal (0, 0, -1) under the pose [I | t]: p = t exactly, q = (0, 0, -1).
# counts: facing, in_image, self_occluded, no_depth, agree, in_front, behind, on_mask on flat_frame(64, 48) with tolerance 2^-7, threshold 0.1
UP, DN = (lambda x, to: float(np.nextafter(F(x), F(to))))(1.0 + EPS, 2.0), (lambda x, to: float(np.nextafter(F(x), F(to))))(1.0 - EPS, 0.0)
TINY = float(F(1e-6))
BOUNDARY_POINTS = [
    ("centre, d = 0, class exactly at the threshold", (0, 0, 1), (1, 1, 0, 0, 1, 0, 0, 1)),
    ("class just below the threshold",               (-1 / 32, 0, 1), (1, 1, 0, 0, 1, 0, 0, 0)),
    ("x.5 rounds up to col 33: the hole",            (0.5 / 32, 0, 1), (1, 1, 0, 1, 0, 0, 0, 0)),
    ("a = -1",                                       (-33 / 32, 0, 1), (1, 0, 0, 0, 0, 0, 0, 0)),
    ("a = 0",                                        (-1.0, 0, 1), (1, 1, 0, 0, 1, 0, 0, 1)),
    ("a = width - 1",                                (31 / 32, 0, 1), (1, 1, 0, 0, 1, 0, 0, 1)),
    ("a = width",                                    (1.0, 0, 1), (1, 0, 0, 0, 0, 0, 0, 0)),
    ("b = -1",                                       (0, -25 / 32, 1), (1, 0, 0, 0, 0, 0, 0, 0)),
    ("b = 0",                                        (0, -24 / 32, 1), (1, 1, 0, 0, 1, 0, 0, 1)),
    ("b = height - 1",                               (0, 23 / 32, 1), (1, 1, 0, 0, 1, 0, 0, 1)),
    ("b = height",                                   (0, 24 / 32, 1), (1, 0, 0, 0, 0, 0, 0, 0)),
    ("p_2 = 1e-6f: not facing",                      (0, 0, TINY), (0, 0, 0, 0, 0, 0, 0, 0)),
    ("p_2 just above 1e-6f: in front of the wall",   (0, 0, float(np.nextafter(F(1e-6), F(1)))), (1, 1, 0, 0, 0, 1, 0, 0)),
    ("p_2 below 1e-6f",                              (0, 0, float(np.nextafter(F(1e-6), F(0)))), (0, 0, 0, 0, 0, 0, 0, 0)),
    ("behind the camera",                            (0, 0, -1), (0, 0, 0, 0, 0, 0, 0, 0)),
    ("d = +tolerance: agrees (inclusive)",           (0, 0, 1.0 + EPS), (1, 1, 0, 0, 1, 0, 0, 1)),
    ("d = -tolerance: agrees (inclusive)",           (0, 0, 1.0 - EPS), (1, 1, 0, 0, 1, 0, 0, 1)),
    ("d one ulp above +tolerance: behind",           (0, 0, UP), (1, 1, 0, 0, 0, 0, 1, 0)),
    ("d one ulp below -tolerance: in front",         (0, 0, DN), (1, 1, 0, 0, 0, 1, 0, 0)),
]


def boundary_batch():
    """the poses of BOUNDARY_POINTS, then q.p == 0 exactly, a zero pose, a NaN pose, an infinite translation, and the first pose again"""
    poses = [_pose(t=t) for _, t, _ in BOUNDARY_POINTS]
    expect = [c for _, _, c in BOUNDARY_POINTS]
    Rq = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], np.float64)      # q = -R[:, 2] = (1, 0, 0); p = (0, y, z): q.p == 0
    poses.append(_pose(Rq, (0, 0.25, 1))); expect.append((0,) * 8)
    poses.append(np.zeros(16, F)); expect.append((0,) * 8)
    poses.append(np.full(16, np.nan, F)); expect.append((0,) * 8)
    inf = _pose(t=(0, 0, 1)); inf[12] = np.inf
    poses.append(inf); expect.append((0,) * 8)
    poses.append(poses[0].copy()); expect.append(expect[0])
    return np.stack(poses), expect


def test_points_on_the_decision_boundaries():
    depth, prob = flat_frame(64, 48)
    case = Case([[0, 0, 0]], [[0, 0, -1]], depth, prob, K64, SCALE)
    poses, expect = boundary_batch()
    for so in (1, 0):
        got = case.check(poses, tolerance=EPS, class_threshold=0.1, self_occlusion=so, occlusion_margin=EPS)
        assert [_counts(r) for r in got] == expect
        assert got["score"][0] == 1.0 and got["violation"][18] == 1.0 and got["score"][21] == 0.0
    # no class image: on_mask is 0 everywhere, the other counts stay
    case.est.set_frame(depth, None, K64, SCALE); case.prob = None
    got = case.check(poses, tolerance=EPS, class_threshold=0.1, occlusion_margin=EPS)
    assert [_counts(r)[:7] for r in got] == [e[:7] for e in expect] and not got["on_mask"].any()
    # a new frame of another size is honoured: 1 x 1
    d1 = np.array([[1024]], np.uint16)
    case.est.set_frame(d1, None, (1.0, 0.0, 1.0, 0.0), SCALE); case.depth, case.K = d1, (1.0, 0.0, 1.0, 0.0)
    got = case.check([_pose(t=(0, 0, 1)), _pose(t=(0.5, 0, 1)), _pose(t=(0, -0.75, 1))], tolerance=EPS)
    assert [_counts(r)[:5] for r in got] == [(1, 1, 0, 0, 1), (1, 0, 0, 0, 0), (1, 0, 0, 0, 0)]


def seeded_model(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    pos = (u * np.array([0.06, 0.04, 0.03])).astype(F)
    nrm = (u / np.array([0.06, 0.04, 0.03])).astype(F)        # not unit: the context normalises
    return pos, nrm


def seeded_poses(n, seed, z=(0.3, 0.9), xy=0.25):
    rng = np.random.default_rng(seed)
    return np.stack([_pose(_rot(rng.normal(size=3), rng.uniform(0, 180)), (rng.uniform(-xy, xy), rng.uniform(-xy, xy), rng.uniform(*z))) for _ in range(n)])


def rough_frame(W, H, seed, raw=(4000, 9000)):
    rng = np.random.default_rng(seed)
    depth = rng.integers(raw[0], raw[1], (H, W)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.15] = 0
    prob = rng.integers(0, 3000, (H, W)).astype(np.uint16)
    return depth, prob


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_model_sizes_either_side_of_a_wavefront_and_a_round(n):
    depth, prob = rough_frame(64, 48, 3)
    K = (60.0, 31.5, 60.0, 23.5)
    pos, nrm = seeded_model(n, 100 + n)
    case = Case(pos, nrm, depth, prob, K, 1e-4)
    poses = seeded_poses(24, 200 + n)
    tot = np.zeros(8, np.int64)
    for prm in (dict(), dict(self_occlusion=0, tolerance=0.05), dict(cell_px=1, occlusion_margin=0.0, tolerance=0.2), dict(cell_px=2, tolerance=0.1, class_threshold=0.15)):
        got = case.check(poses, **prm)
        tot += np.array([got[c].sum() for c in ref.COUNTS])
        assert np.array_equal(got["in_image"], got["self_occluded"] + got["no_depth"] + got["agree"] + got["in_front"] + got["behind"])
    if n >= 255:
        assert (tot > 0).all(), dict(zip(ref.COUNTS, tot.tolist()))


def test_camera_640x480():
    raw = np.load(os.path.join(GOLD, "example_ycb_024_bowl_raw.npz"))
    K = [float(x) for x in raw["K"]]
    pos, nrm = seeded_model(1025, 9)
    case = Case(pos, nrm, raw["depth"], raw["prob"], K, float(raw["depth_scale"]))
    got = case.check(seeded_poses(32, 10, z=(0.4, 1.2)))
    assert got["in_image"].sum() > 1000 and got["agree"].sum() + got["in_front"].sum() + got["behind"].sum() > 1000


def test_self_occlusion_margin_is_exclusive():
    """three points on one view ray: the second farther than the first by exactly the margin stays visible, the third by twice the margin is hidden"""
    depth, prob = flat_frame(64, 48)
    case = Case([[0, 0, 0], [0, 0, EPS], [0, 0, 2 * EPS]], [[0, 0, -1]] * 3, depth, prob, K64, SCALE)
    P = _pose(t=(0, 0, 1))
    on = case.check([P], tolerance=EPS, occlusion_margin=EPS)[0]
    assert _counts(on) == (3, 3, 1, 0, 2, 0, 0, 2)
    off = case.check([P], tolerance=EPS, occlusion_margin=EPS, self_occlusion=0)[0]
    assert _counts(off) == (3, 3, 0, 0, 2, 0, 1, 2)
    zero = case.check([P], tolerance=EPS, occlusion_margin=0.0)[0]
    assert _counts(zero) == (3, 3, 2, 0, 1, 0, 0, 1)
    # the whole projection is one pixel; cell_px = 1
    one = case.check([P], tolerance=EPS, occlusion_margin=EPS, cell_px=1)[0]
    assert _counts(one) == _counts(on)


def two_layer_model(n, seed):
    """two parallel sheets 5 cm apart, both facing the camera under the identity rotation: the far sheet is hidden wherever the near one
    has a point in the same cell"""
    rng = np.random.default_rng(seed)
    pos = np.zeros((n, 3), F)
    pos[:, 0] = rng.uniform(-0.3, 0.3, n); pos[:, 1] = rng.uniform(-0.2, 0.2, n); pos[:, 2] = np.where(rng.random(n) < 0.5, 0.0, 0.05)
    nrm = np.tile(np.array([0, 0, -1], F), (n, 1))
    return pos, nrm


def test_z_buffer_stride_grows_with_the_projection():
    W, H = 640, 480
    depth = np.full((H, W), 10000, np.uint16)
    pos, nrm = two_layer_model(700, 4)
    case = Case(pos, nrm, depth, None, (600.0, 319.5, 600.0, 239.5), 1e-4)
    poses = np.stack([_pose(t=(0, 0, 1.0)), _pose(t=(0.1, -0.05, 0.8)), _pose(_rot((0, 0, 1), 30), (0, 0, 1.5)), _pose(t=(0, 0, 6.0))])
    for cell_px in (1, 2, 8):
        got = case.check(poses, cell_px=cell_px, tolerance=0.01, occlusion_margin=0.01)
        assert got["self_occluded"][0] > 0
    # the stride the contract prescribes for the first pose at cell_px = 1 is above 1: the projection spans more than 64 pixels
    f = ref.point_flags(poses[0], pos, ref.unit_normals(nrm), depth, None, case.K, case.scale, cell_px=1)
    assert np.ptp(f["col"][f["in_image"]]) + 1 > 64 * 1
    f = ref.point_flags(poses[3], pos, ref.unit_normals(nrm), depth, None, case.K, case.scale, cell_px=1)
    assert np.ptp(f["col"][f["in_image"]]) + 1 <= 64 * 1       # and the far pose stays at stride 1


def render_splat(pos, nrm, P4, K, W, H, scale, r=2):
    """depth image of the model's camera-facing points under P4: nearest z per pixel, each point splatted over (2r+1)^2 pixels"""
    p = pos.astype(np.float64) @ P4[:3, :3].T + P4[:3, 3]
    q = nrm.astype(np.float64) @ P4[:3, :3].T
    vis = ((q * p).sum(1) < 0) & (p[:, 2] > 1e-6)
    p = p[vis]
    col = np.floor(K[0] * p[:, 0] / p[:, 2] + K[1] + 0.5).astype(int); row = np.floor(K[2] * p[:, 1] / p[:, 2] + K[3] + 0.5).astype(int)
    z = np.full((H, W), np.inf)
    for dr in range(-r, r + 1):
        for dc in range(-r, r + 1):
            rr, cc = row + dr, col + dc
            ok = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
            np.minimum.at(z, (rr[ok], cc[ok]), p[ok, 2])
    z[~np.isfinite(z)] = 1.5                                    # a wall behind the object
    return np.round(z / scale).astype(np.uint16)


def test_closed_model_against_its_own_rendering():
    from model_matching_amd import synth
    m = synth.make_model_asym(2000)
    W, H, K, scale = 320, 240, (500.0, 159.5, 500.0, 119.5), 1e-4
    rng = np.random.default_rng(12)
    P = np.eye(4); P[:3, :3] = _rot(rng.normal(size=3), rng.uniform(0, 180)); P[:3, 3] = (0.02, -0.01, 0.6)
    depth = render_splat(m.pos, m.nrm, P, K, W, H, scale)
    case = Case(m.pos, m.nrm, depth, None, K, scale)
    ray = P[:3, 3] / np.linalg.norm(P[:3, 3])
    near, far = P.copy(), P.copy()
    near[:3, 3] -= 0.05 * ray; far[:3, 3] += 0.05 * ray
    got = case.check(np.stack([M.T.reshape(16).astype(F) for M in (P, near, far)]))
    assert got["in_front"][1] > got["in_front"][0] and got["in_front"][1] > got["in_front"][2]
    assert got["behind"][2] > got["behind"][0] and got["behind"][2] > got["behind"][1]
    assert got["score"][0] > got["score"][1] and got["score"][0] > got["score"][2] and got["score"][0] > 0.8


def test_batch_independence_and_no_allocation():
    from model_matching_amd import capi
    depth, prob = rough_frame(64, 48, 5)
    pos, nrm = seeded_model(257, 31)
    case = Case(pos, nrm, depth, prob, (60.0, 31.5, 60.0, 23.5), 1e-4)
    poses = seeded_poses(257, 32)
    poses[100] = 0; poses[200] = np.nan
    whole = case.check(poses, tolerance=0.05)
    L = capi.load()
    a0 = L.stocs_device_alloc_count()
    again = case.est.depth_check_poses(poses, tolerance=0.05)
    assert L.stocs_device_alloc_count() == a0
    assert again.tobytes() == whole.tobytes()
    assert case.est.depth_check_poses(poses[::-1], tolerance=0.05)[::-1].tobytes() == whole.tobytes()
    alone = np.concatenate([case.est.depth_check_poses(poses[i], tolerance=0.05) for i in range(len(poses))])
    assert alone.tobytes() == whole.tobytes()
    assert not any(whole[100][c] for c in ref.COUNTS) and not any(whole[200][c] for c in ref.COUNTS) and whole["facing"][[99, 101, 199, 201]].all()


def test_errors():
    from model_matching_amd import capi
    L = capi.load()
    pos, nrm = seeded_model(65, 2)
    est = _est(pos, nrm)
    prm = capi.DepthParams(); L.stocs_default_depth_params(C.byref(prm))
    out = (capi.DepthResult * 2)()
    P, pP = capi.f32(seeded_poses(2, 1))
    assert L.stocs_depth_check_poses(est.h, pP, 2, C.byref(prm), out) == -5              # no frame: STOCS_ERR_STATE
    assert L.stocs_depth_check_poses(est.h, pP, 0, C.byref(prm), out) == 0               # n == 0: no-op, whatever the state
    depth, prob = rough_frame(64, 48, 7)
    dp = depth.ctypes.data_as(C.POINTER(C.c_uint16))
    for w, h in ((0, 48), (64, 0), (-1, 48)):
        assert L.stocs_ctx_set_frame(est.h, C.byref(capi.Camera(60, 32, 60, 24, 1e-4, w, h, 0)), dp, None) == -1
    cam = capi.Camera(60, 32, 60, 24, 1e-4, 64, 48, 0)
    assert L.stocs_ctx_set_frame(est.h, None, dp, None) == -1 and L.stocs_ctx_set_frame(est.h, C.byref(cam), None, None) == -1
    assert L.stocs_depth_check_poses(est.h, pP, 2, C.byref(prm), out) == -5              # the failed calls set no frame
    est.set_frame(depth, prob, (60, 32, 60, 24), 1e-4)
    assert L.stocs_depth_check_poses(est.h, pP, 2, C.byref(prm), out) == 0
    assert L.stocs_depth_check_poses(est.h, pP, -1, C.byref(prm), out) == -1
    assert L.stocs_depth_check_poses(est.h, None, 2, C.byref(prm), out) == -1
    assert L.stocs_depth_check_poses(est.h, pP, 2, None, out) == -1
    assert L.stocs_depth_check_poses(est.h, pP, 2, C.byref(prm), None) == -1
    assert L.stocs_depth_check_poses(est.h, None, 0, None, None) == 0
    bad = [("tolerance", 0.0), ("tolerance", -1.0), ("tolerance", float("nan")), ("tolerance", float("inf")), ("self_occlusion", 2), ("self_occlusion", -1),
           ("cell_px", 0), ("occlusion_margin", -1e-3), ("occlusion_margin", float("nan")), ("occlusion_margin", float("inf")), ("class_threshold", float("nan"))]
    for k, v in bad:
        q = capi.DepthParams(); L.stocs_default_depth_params(C.byref(q)); setattr(q, k, v)
        assert L.stocs_depth_check_poses(est.h, pP, 2, C.byref(q), out) == -1, (k, v)
    with pytest.raises(capi.StocsError):
        est.depth_check_poses(P, tolerance=0.0)
    # a new frame of another size is honoured
    d2, p2 = rough_frame(17, 9, 8)
    est.set_frame(d2, p2, (20.0, 8.0, 20.0, 4.0), 1e-4)
    got = est.depth_check_poses(P)
    assert ref.records_equal(got, ref.check_poses(P, pos, nrm, d2, p2, (20.0, 8.0, 20.0, 4.0), 1e-4))


def _push(pose16, metres):
    """the pose moved along the view ray through its translation"""
    P = np.asarray(pose16, np.float64).copy()
    t = P[12:15]
    P[12:15] = t + metres * t / np.linalg.norm(t)
    return P.astype(F)


def rank_hypotheses(hyps, recs):
    """first maximum of score - violation (float32), ties to the higher lcp, then to the lower (trial, hypothesis): -> index into the flat lists"""
    key = [(-float(F(r["score"]) - F(r["violation"])), -float(l), i) for i, (r, l) in enumerate(zip(recs, hyps))]
    return min(key)[2]


@pytest.mark.parametrize("name,floor", [("ycb_024_bowl", 0.35), ("linemod_obj_06", 0.05)])
def test_example_frames(name, floor):
    """every hypothesis of an 8-trial batch, candidate pose and refined pose, equals the restatement; the winner by score - violation
    agrees with the frame at least as well as the same pose pushed 5 cm along the view ray, and at least to the floor
    tests/test_driver_gpu.py holds a single trial's winner to (within_10mm over the visible points)"""
    from model_matching_amd.estimator import StocsEstimator
    d = np.load(os.path.join(GOLD, "example_%s.npz" % name))
    raw = np.load(os.path.join(GOLD, "example_%s_raw.npz" % name))
    K, scale = [float(x) for x in raw["K"]], float(raw["depth_scale"])
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
    est.set_scene(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"])
    est.set_frame(raw["depth"], raw["prob"], K, scale)
    est.run_trials(list(range(7, 15)), 100, max_per_base=200, post=dict(maximum_pose_count=10, refine_iterations=5))
    hyps = np.concatenate([est.trials_get_hypotheses(t) for t in range(8)])
    assert len(hyps) >= 8
    for field in ("pose16", "refined_pose16"):
        got = est.depth_check_poses(hyps[field])
        want = ref.check_poses(hyps[field], d["model_pos"], d["model_nrm"], raw["depth"], raw["prob"], K, scale)
        assert ref.records_equal(got, want), field
    w = rank_hypotheses(hyps["refined_lcp"], got)
    pair = est.depth_check_poses(np.stack([hyps["refined_pose16"][w], _push(hyps["refined_pose16"][w], 0.05)]))
    assert ref.records_equal(pair[0], got[w]) and pair["score"][0] >= pair["score"][1]
    assert pair["score"][0] >= floor and pair["facing"][0] >= 100


def _write_example_tree(tmp_path, name):
    """the reference's directory layout rebuilt from the committed data fixtures (as tests/test_driver_gpu.py does)"""
    from PIL import Image
    raw = np.load(os.path.join(GOLD, "example_%s_raw.npz" % name))
    obj = name.split("_", 1)[1]
    scene = tmp_path / "scene"; (scene / "probability_maps").mkdir(parents=True)
    Image.fromarray(raw["depth"].astype(np.uint16)).save(scene / "depth.png")
    Image.fromarray(raw["prob"].astype(np.uint16)).save(scene / "probability_maps" / (obj + ".png"))
    mdir = tmp_path / "repo" / "models" / obj; mdir.mkdir(parents=True)
    with open(mdir / "textured_vertices.ply", "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment VCGLIB generated\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face 0\nproperty list uchar int vertex_indices\nend_header\n" % len(raw["model_raw"]))
        for p in raw["model_raw"]:
            f.write("%.9g %.9g %.9g \n" % (p[0], p[1], p[2]))
    return raw, obj, scene, tmp_path / "repo"


DEPTH_LINE = re.compile(r"^  depth (\d+)\.(\d+): facing (\d+) in_image (\d+) self_occluded (\d+) no_depth (\d+) agree (\d+) in_front (\d+) behind (\d+) on_mask (\d+) "
                        r"score (\S+) violation (\S+) lcp (\S+)$")


def test_driver_depth_check(tmp_path):
    from model_matching_amd import capi
    from model_matching_amd.estimator import StocsEstimator, ingest_scene
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    K, scale = [float(x) for x in raw["K"]], float(raw["depth_scale"])
    pre = subprocess.run([PRE, obj, "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                          "--model-scale", repr(float(raw["model_scale"]))], capture_output=True, text=True, timeout=300)
    assert pre.returncode == 0, pre.stdout + pre.stderr
    seed = 7
    base = [APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(scale), "--seed", str(seed),
            "--trials", "4", "--cluster", "1"]
    r0 = subprocess.run(base + ["--out", str(tmp_path / "plain.txt")], capture_output=True, text=True, timeout=300)
    r1 = subprocess.run(base + ["--out", str(tmp_path / "depth.txt"), "--depth-check"], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    # without the flag: the lines of the run with it, minus the depth lines
    timing = re.compile(r"total_microseconds=\d+")
    extra = re.compile(r"^(  depth \d+\.\d+: .*|depth check: .*|depth pose:.*)$")
    plain = [timing.sub("", ln) for ln in r0.stdout.splitlines()]
    flagged = [timing.sub("", ln) for ln in r1.stdout.splitlines()]
    assert [ln for ln in flagged if not extra.match(ln)] == plain and not any(extra.match(ln) for ln in plain)
    recs = [DEPTH_LINE.match(ln) for ln in r1.stdout.splitlines() if ln.startswith("  depth ")]
    assert recs and all(recs)
    # the Python route on the clouds the driver worked on
    L = capi.load()
    n, hn = C.c_int(), C.c_int()
    mp = str(repo / "models" / obj / "model_search.ply").encode()
    assert L.stocs_ply_read(mp, None, None, 0, C.byref(n), C.byref(hn)) == 0
    mpos = np.zeros((n.value, 3), F); mnrm = np.zeros((n.value, 3), F)
    assert L.stocs_ply_read(mp, mpos.ctypes.data_as(capi._fp), mnrm.ctypes.data_as(capi._fp), n.value, C.byref(n), C.byref(hn)) == 0
    spos, snrm, sprob, spix = ingest_scene(raw["depth"], raw["prob"], K, scale, 0.005, 0.10)
    est = StocsEstimator(spos, snrm, sprob, spix, mpos, mnrm, build_index=True)
    est.set_frame(raw["depth"], raw["prob"], K, scale)
    est.run_trials([seed + t for t in range(4)], 100, max_per_base=200, post=dict(maximum_pose_count=10))
    per_trial = [est.trials_get_hypotheses(t) for t in range(4)]
    hyps = np.concatenate(per_trial)
    got = est.depth_check_poses(hyps["pose16"])
    assert len(recs) == len(hyps)                                   # one record per hypothesis
    ids = [(t, i) for t in range(4) for i in range(len(per_trial[t]))]
    for mt, (t, i), r in zip(recs, ids, got):
        assert (int(mt.group(1)), int(mt.group(2))) == (t, i)
        assert tuple(int(mt.group(3 + j)) for j in range(8)) == _counts(r)
        assert F(mt.group(11)) == r["score"] and F(mt.group(12)) == r["violation"]
    w = rank_hypotheses(hyps["lcp"], got)
    vals = np.array((tmp_path / "depth.txt").read_text().split(), float)
    assert vals.shape == (12,) and np.allclose(vals.reshape(3, 4), hyps["pose16"][w].reshape(4, 4).T[:3], rtol=2e-5, atol=2e-6)
    assert ("depth check: hypotheses=%d best_trial=%d best_hypothesis=%d " % (len(hyps), ids[w][0], ids[w][1])) in r1.stdout
