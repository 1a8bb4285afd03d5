"""The float32 restatement of the depth-check contract (tests/depth_check_ref.py) against itself and against the float64 host check it
stands next to, tools/pose_check.py::depth_agreement, on the three example frames.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import depth_check_ref as ref  # noqa: E402
from pose_check import depth_agreement  # noqa: E402

FRAMES = ["ycb_024_bowl", "linemod_obj_06", "packed_dove"]


def _rot(axis, deg):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def frame_poses(name, n_perturbed=5):
    """the fixture's own best pose and seeded perturbations of it (<= 5 degrees about the model origin's image, <= 1 cm): column-major 16"""
    summ = json.load(open(os.path.join(ROOT, "tests", "golden", "example_summary.json")))[name]
    P0 = np.asarray(summ["best_pose16"], np.float64).reshape(4, 4).T
    rng = np.random.default_rng(20261017 + FRAMES.index(name))
    out = [P0]
    for _ in range(n_perturbed):
        T = np.eye(4)
        T[:3, :3] = _rot(rng.normal(size=3), rng.uniform(0.5, 5.0))
        c = P0[:3, 3]
        T[:3, 3] = c - T[:3, :3] @ c + rng.uniform(-0.01, 0.01, 3)   # turn about the object's position in the camera frame
        out.append(T @ P0)
    return np.stack([P.T.reshape(16) for P in out]).astype(np.float32)


def _load(name):
    raw = np.load(os.path.join(ROOT, "tests", "golden", "example_%s_raw.npz" % name))
    fix = np.load(os.path.join(ROOT, "tests", "golden", "example_%s.npz" % name))
    return raw["depth"], raw["prob"], [float(x) for x in raw["K"]], float(raw["depth_scale"]), fix["model_pos"], fix["model_nrm"]


def _f64_points(pose16, mpos, mnrm, depth, K, scale, tol):
    """depth_agreement's arithmetic (float64) per model point: facing, agree, and which points sit within the stated margins of a
    decision boundary (1e-9 of q.p = 0, 1e-4 px of a pixel rounding boundary, 1e-6 m of the tolerance)"""
    P = np.asarray(pose16, np.float64).reshape(4, 4).T[:3]
    R, t = P[:, :3], P[:, 3]
    fx, cx, fy, cy = K
    pts = np.asarray(mpos, np.float64) @ R.T + t
    nrm = np.asarray(mnrm, np.float64) @ R.T
    dot = (nrm * pts).sum(1)
    facing = (dot < 0.0) & (pts[:, 2] > 1e-6)
    near = np.abs(dot) < 1e-9
    H, W = depth.shape
    with np.errstate(all="ignore"):
        u = fx * pts[:, 0] / pts[:, 2] + cx + 0.5
        v = fy * pts[:, 1] / pts[:, 2] + cy + 0.5
    near |= facing & ((np.abs(u - np.round(u)) < 1e-4) | (np.abs(v - np.round(v)) < 1e-4))
    col = np.floor(u); row = np.floor(v)
    inside = facing & (row >= 0) & (row < H) & (col >= 0) & (col < W)
    r = np.where(inside, row, 0).astype(np.int64); c = np.where(inside, col, 0).astype(np.int64)
    zo = depth[r, c].astype(np.float64) * scale
    dz = np.abs(zo - pts[:, 2])
    agree = inside & (zo > 0) & (dz <= tol)
    near |= inside & (zo > 0) & (np.abs(dz - tol) < 1e-6)
    return facing, agree, near


@pytest.mark.parametrize("name", FRAMES)
def test_restatement_equals_depth_agreement_point_for_point(name):
    depth, prob, K, scale, mpos, mnrm = _load(name)
    unit = ref.unit_normals(mnrm)
    for pose in frame_poses(name):
        for tol, key in ((0.005, "within_5mm"), (0.010, "within_10mm")):
            facing64, agree64, near = _f64_points(pose, mpos, mnrm, depth, K, scale, tol)
            # the per-point float64 statement IS depth_agreement's: same totals
            da = depth_agreement(np.asarray(pose, np.float64).reshape(4, 4).T, mpos, mnrm, depth, prob, K, scale)
            assert da["visible_points"] == int(facing64.sum()) and da["visible_points"] >= 100
            assert round(da[key] * da["visible_points"]) == int(agree64.sum())
            # the cap on the excluded points is a condition on the float64 reference alone
            assert near.sum() <= 0.01 * facing64.sum(), (name, int(near.sum()), int(facing64.sum()))
            f = ref.point_flags(pose, mpos, unit, depth, prob, K, scale, self_occlusion=0, tolerance=tol)
            keep = ~near
            assert np.array_equal(f["facing"][keep], facing64[keep])
            assert np.array_equal(f["agree"][keep], agree64[keep])
            assert not f["self_occluded"].any()


def _seeded_case(seed):
    rng = np.random.default_rng(seed)
    W, H = int(rng.integers(1, 80)), int(rng.integers(1, 60))
    n = int(rng.integers(1, 700))
    mpos = rng.normal(0, 0.05, (n, 3)).astype(np.float32)
    mnrm = (mpos + rng.normal(0, 0.01, (n, 3))).astype(np.float32)     # roughly outward
    depth = rng.integers(0, 12000, (H, W)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.2] = 0
    prob = rng.integers(0, 10001, (H, W)).astype(np.uint16) if seed % 2 else None
    K = (float(rng.uniform(20, 80)), W / 2.0, float(rng.uniform(20, 80)), H / 2.0)
    P = np.eye(4)
    P[:3, :3] = _rot(rng.normal(size=3), rng.uniform(0, 180))
    P[:3, 3] = [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 1.2)]
    prm = dict(tolerance=float(rng.choice([0.005, 0.01, 0.2])), self_occlusion=int(seed % 3 != 0), cell_px=int(rng.choice([1, 2, 8])),
               occlusion_margin=float(rng.choice([0.0, 0.01])), class_threshold=0.1)
    return P.T.reshape(16).astype(np.float32), mpos, mnrm, depth, prob, K, 1e-4, prm


@pytest.mark.parametrize("seed", range(40))
def test_count_identity_on_seeded_cases(seed):
    pose, mpos, mnrm, depth, prob, K, scale, prm = _seeded_case(seed)
    r = ref.check_poses(pose, mpos, mnrm, depth, prob, K, scale, **prm)[0]
    assert r["facing"] >= r["in_image"] == r["self_occluded"] + r["no_depth"] + r["agree"] + r["in_front"] + r["behind"]
    assert r["on_mask"] <= r["agree"] and (prob is not None or r["on_mask"] == 0)
    assert prm["self_occlusion"] == 1 or r["self_occluded"] == 0
    if r["facing"]:
        assert r["score"] == np.float32(r["agree"]) / np.float32(r["facing"]) and r["violation"] == np.float32(r["in_front"]) / np.float32(r["facing"])
    else:
        assert r["score"] == 0 and r["violation"] == 0
    f = ref.point_flags(pose, mpos, ref.unit_normals(mnrm), depth, prob, K, scale, **prm)
    classes = np.stack([f[c] for c in ("self_occluded", "no_depth", "agree", "in_front", "behind")]).sum(0)
    assert np.array_equal(classes, f["in_image"].astype(int))       # every in-image point is in exactly one class


def test_the_seeded_cases_exercise_every_class():
    tot = np.zeros(8, np.int64)
    for seed in range(40):
        pose, mpos, mnrm, depth, prob, K, scale, prm = _seeded_case(seed)
        r = ref.check_poses(pose, mpos, mnrm, depth, prob, K, scale, **prm)[0]
        tot += np.array([r[c] for c in ref.COUNTS])
    assert (tot > 0).all(), dict(zip(ref.COUNTS, tot.tolist()))


def test_zero_and_non_finite_poses_give_zero_records():
    pose, mpos, mnrm, depth, prob, K, scale, prm = _seeded_case(5)
    bad = np.stack([np.zeros(16, np.float32), np.full(16, np.nan, np.float32), pose.copy(), pose.copy()])
    bad[2, 13] = np.inf; bad[3, 0] = -np.inf
    r = ref.check_poses(bad, mpos, mnrm, depth, prob, K, scale, **prm)
    for c in ref.COUNTS + ("score", "violation"):
        assert not r[c].any(), c
