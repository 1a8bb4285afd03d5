"""The float32 restatement of the joint-rendering contract (tests/render_ref.py) against itself: the identities and invariances the
contract states hold in the restatement the GPU tests compare the library with.  No GPU, numpy only."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import render_ref as ref  # noqa: E402

F = np.float32
W, H, K, SCALE = 64, 48, (60.0, 31.5, 60.0, 23.5), 1e-4
PRM = dict(point_radius=0.02, max_splat_px=3, tolerance=0.05, class_threshold=0.15)


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


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(5)
    u = rng.normal(size=(300, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    pos = (u * np.array([0.06, 0.04, 0.03])).astype(F)
    nrm = (u / np.array([0.06, 0.04, 0.03])).astype(F)
    poses = np.stack([_pose(_rot(rng.normal(size=3), rng.uniform(0, 180)), (rng.uniform(-0.1, 0.1), rng.uniform(-0.08, 0.08), rng.uniform(0.25, 0.6))) for _ in range(7)])
    depth = rng.integers(2000, 7000, (H, W)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.15] = 0
    prob = rng.integers(0, 3000, (H, W)).astype(np.uint16)
    return pos, nrm, poses, depth, prob


def test_count_identities_and_classes_all_occur(world):
    pos, nrm, poses, depth, prob = world
    rec, lab, st, zkey = ref.explain(poses, pos, nrm, depth, prob, K, SCALE, **PRM)
    assert np.array_equal(rec["footprint"], rec["visible"] + rec["hidden"])
    assert np.array_equal(rec["visible"], rec["no_depth"] + rec["agree"] + rec["in_front"] + rec["behind"])
    assert (rec["on_mask"] <= rec["agree"]).all()
    assert all(rec[c].sum() > 0 for c in ref.COUNTS)
    # every pixel has one owner: the visible counts add up to the labelled pixels
    assert rec["visible"].sum() == (lab >= 0).sum()
    for h in range(len(poses)):
        assert rec["visible"][h] == (lab == h).sum()


def test_footprint_is_the_pixel_count_of_the_pose_alone(world):
    pos, nrm, poses, depth, prob = world
    rec = ref.explain(poses, pos, nrm, depth, prob, K, SCALE, **PRM)[0]
    for h in range(len(poses)):
        alone = ref.render(ref.empty_keys(W, H), poses[h], pos, nrm, K, W, H, **PRM)
        assert rec["footprint"][h] == (alone != ref.EMPTY).sum()


def test_order_of_calls_and_batching_do_not_matter(world):
    pos, nrm, poses, depth, prob = world
    whole = ref.render(ref.empty_keys(W, H), poses, pos, nrm, K, W, H, **PRM)
    a, b = poses[:3], poses[3:]
    ab = ref.render(ref.render(ref.empty_keys(W, H), a, pos, nrm, K, W, H, 0, **PRM), b, pos, nrm, K, W, H, 3, **PRM)
    ba = ref.render(ref.render(ref.empty_keys(W, H), b, pos, nrm, K, W, H, 3, **PRM), a, pos, nrm, K, W, H, 0, **PRM)
    assert ab.tobytes() == ba.tobytes() == whole.tobytes()
    one = ref.empty_keys(W, H)
    for h in reversed(range(len(poses))):
        ref.render(one, poses[h], pos, nrm, K, W, H, h, **PRM)
    assert one.tobytes() == whole.tobytes()
    # clear forgets, no clear accumulates
    again = ref.render(whole.copy(), b, pos, nrm, K, W, H, 3, True, **PRM)
    assert again.tobytes() == ref.render(ref.empty_keys(W, H), b, pos, nrm, K, W, H, 3, **PRM).tobytes()


def test_a_pose_entirely_behind_another_is_invisible():
    # a dense near sheet and a smaller far one on the same view rays
    g = np.stack(np.meshgrid(np.linspace(-0.1, 0.1, 21), np.linspace(-0.1, 0.1, 21)), -1).reshape(-1, 2)
    pos = np.concatenate([g, np.zeros((len(g), 1))], 1).astype(F)
    nrm = np.tile(np.array([0, 0, -1], F), (len(g), 1))
    near, far = _pose(t=(0, 0, 0.5)), _pose(R=np.diag([0.5, 0.5, 1.0]), t=(0, 0, 0.8))
    depth = np.full((H, W), 5000, np.uint16)
    for order in ((near, far), (far, near)):
        rec, lab, st, _ = ref.explain(np.stack(order), pos, nrm, depth, None, K, SCALE, **PRM)
        f = 1 if order[0] is near else 0
        assert rec["footprint"][f] > 0 and rec["visible"][f] == 0 and rec["hidden"][f] == rec["footprint"][f]
        assert rec["visible"][1 - f] == rec["footprint"][1 - f] > 0
        assert not (lab == f).any()
    # equal depth: the lower id wins whatever its position
    rec = ref.explain(np.stack([near, near]), pos, nrm, depth, None, K, SCALE, **PRM)[0]
    assert rec["visible"][0] == rec["footprint"][0] and rec["visible"][1] == 0


def test_labels_are_minus_one_exactly_where_the_key_is_empty(world):
    pos, nrm, poses, depth, prob = world
    rec, lab, st, zkey = ref.explain(poses, pos, nrm, depth, prob, K, SCALE, **PRM)
    empty = (zkey == ref.EMPTY).reshape(H, W)
    assert empty.any() and not empty.all()
    assert np.array_equal(lab == -1, empty) and np.array_equal(st == 0, empty)
    assert set(np.unique(st)) <= {0, 1, 2, 3, 4, 18} and ((st & 15)[~empty] >= 1).all()
    assert lab.max() < len(poses)


def test_invalid_poses_touch_nothing(world):
    pos, nrm, poses, depth, prob = world
    bad = poses.copy(); bad[2] = 0; bad[4] = np.nan
    rec, lab, _, zkey = ref.explain(bad, pos, nrm, depth, prob, K, SCALE, **PRM)
    assert not any(rec[c][2] or rec[c][4] for c in ref.COUNTS) and not np.isin(lab, (2, 4)).any()
    keep = [0, 1, 3, 5, 6]
    want = ref.empty_keys(W, H)
    for h in keep:
        ref.render(want, poses[h], pos, nrm, K, W, H, h, **PRM)
    assert zkey.tobytes() == want.tobytes()
