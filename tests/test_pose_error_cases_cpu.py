"""The pose-error restatement (tests/pose_error_ref.py) against a float64 brute force, and the seeded cases (tests/pose_error_cases.py)
against what each is named for.  No GPU.

The bound.  u = 2^-24.  Step 1 forms p_a from three products and three sums, so |p_a - exact| <= g4 * A with g4 = 4u / (1 - 4u) and
A >= |R_a0 m_x| + |R_a1 m_y| + |R_a2 m_z| + |t_a| for every point, row and pose of the case (computed below in float64; the float32
inputs are exact in float64, so there is no input error).  A difference d_a = p_a - g_a then carries 2 g4 A + u |d_a|, the vector d at
most T = 2 sqrt(3) g4 A in length plus u |d|; the squares, the two sums and the root add less than (3u + 2u) / 2 + u < 4u relatively.
Hence |e32 - e64| <= T + 6u e.  A minimum moves by no more than its candidates do: |s32 - s64| <= T + 6u max(s32, s64).  The means add
the 2^-32 of the fixed point's floor and one rounding to float."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pose_error_cases as cases  # noqa: E402
import pose_error_ref as ref  # noqa: E402

F = np.float32
U = 2.0 ** -24
G4 = 4 * U / (1 - 4 * U)


def _A(model, poses):
    m = np.abs(np.asarray(model, np.float64))
    a = 0.0
    for P in np.asarray(poses, np.float64).reshape(-1, 16):
        M = P.reshape(4, 4).T
        a = max(a, float((m @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3])).max()))
    return a


def _check_against_float64(model, est, gt):
    est, gt = np.asarray(est, F).reshape(-1, 16), np.asarray(gt, F).reshape(-1, 16)
    T = 2 * np.sqrt(3.0) * G4 * _A(model, np.concatenate([est, gt]))
    rec = ref.records(est, gt, model)
    for k in range(len(est)):
        g = gt[0 if len(gt) == 1 else k]
        e, s, nn = ref.detail(est[k], g, model)
        e64, s64 = ref.detail64(est[k], g, model)
        assert np.all(np.abs(e - e64) <= T + 6 * U * e64), np.abs(e - e64).max()
        assert np.all(np.abs(s - s64) <= T + 6 * U * np.maximum(s, s64)), np.abs(s - s64).max()
        assert np.all(s.view(np.uint32) <= e.view(np.uint32))    # s_i <= e_i bit for bit (non-negative floats order as their bits)
        assert np.all((nn >= 0) & (nn < len(model)))
        assert rec[k]["valid"] == 1
        for name, x64 in (("add", e64), ("adds", s64)):
            tol = T + 6 * U * x64.max() + 2.0 ** -32 + U * x64.mean()
            assert abs(float(rec[k][name]) - x64.mean()) <= tol, (name, rec[k][name], x64.mean())
            assert abs(float(rec[k][name + "_max"]) - x64.max()) <= T + 6 * U * x64.max()
    return rec


@pytest.mark.parametrize("M", [1, 2, 65, 257, 1025])
def test_restatement_agrees_with_float64_on_random_pairs(M):
    model = cases.random_model(M)
    est, gt = cases.random_pairs(3, M)
    _check_against_float64(model, est, gt)
    est, gt = cases.random_pairs(3, M + 1, near=True)
    _check_against_float64(model, est, gt[:1])
    d, d64 = ref.diameter(model), ref.diameter64(model)
    assert abs(float(d) - d64) <= 6 * U * d64    # untransformed points: no step-1 error at all
    if M == 1:
        assert d == 0


def test_units_and_offsets_agree_with_float64():
    for c in (cases.millimetres(), cases.far_from_origin()):
        _check_against_float64(c["model"], c["est"], c["gt"])


def test_identical_poses_give_exact_zeros():
    model = cases.random_model(65)
    est, _ = cases.random_pairs(2, 1)
    rec = ref.records(est, est, model)
    for k in ("add_fix", "adds_fix", "add", "add_max", "adds", "adds_max"):
        assert np.all(rec[k] == 0), k
    assert np.all(rec["valid"] == 1)


def test_pure_translation_is_exact():
    model = cases.lattice(4, 2.0 ** -6)
    rec = ref.records(cases.pose(None, (0.125, 0, 0.5)), cases.pose(None, (0, 0, 0.5)), model)[0]
    assert rec["add"] == F(0.125) and rec["add_max"] == F(0.125) and rec["add_fix"] == len(model) * (1 << 29)
    assert rec["adds"] <= rec["add"]


def test_lattice_quarter_turn_maps_onto_itself():
    c = cases.lattice_quarter_turn()
    p, g = ref.transform(c["est"][0], c["model"]), ref.transform(c["gt"][0], c["model"])
    assert np.array_equal(p, g[c["perm"]])                       # really a symmetry, exactly
    e, s, nn = ref.detail(c["est"][0], c["gt"][0], c["model"])
    assert np.all(s == 0) and np.array_equal(nn, c["perm"])
    assert e.max() > 0.05 and ref.records(c["est"], c["gt"], c["model"])[0]["adds_fix"] == 0


def test_ring_turn_maps_onto_itself_within_ulps():
    c = cases.ring_turn()
    e, s, nn = ref.detail(c["est"][0], c["gt"][0], c["model"])
    assert np.array_equal(nn, c["perm"])
    assert s.max() <= 8 * U * c["radius"]                          # a few ulps of the coordinates
    assert e.min() > 0.5 * c["radius"] * 2 * np.sin(np.pi / 12)    # ADD sees the turn: each corner moved one side length


def test_duplicate_points_tie_and_the_lower_index_wins():
    c = cases.duplicate_points()
    m, half = c["model"], len(c["model"]) // 2
    assert np.array_equal(m[:half].view(np.uint32), m[half:].view(np.uint32))
    p, g = ref.transform(c["est"][0], m), ref.transform(c["gt"][0], m)
    D = ref.sqdist(p[:, None, :], g[None, :, :])
    assert np.all((D == D.min(1, keepdims=True)).sum(1) >= 2)      # the ties are real
    _, _, nn = ref.detail(c["est"][0], c["gt"][0], m)
    assert np.all(nn < half)


@pytest.mark.parametrize("ways", [2, 4, 8])
def test_lattice_midpoints_tie_exactly(ways):
    c = cases.lattice_midpoints(ways)
    m, n = c["model"], c["n"]
    p, g = ref.transform(c["est"][0], m), ref.transform(c["gt"][0], m)
    D = ref.sqdist(p[:, None, :], g[None, :, :])
    ties = (D == D.min(1, keepdims=True)).sum(1)
    assert ties.max() == ways and (ties == ways).sum() >= (n - 1) ** 3     # every query with all its neighbours inside the lattice
    e, s, nn = ref.detail(c["est"][0], c["gt"][0], m)
    first = np.array([np.flatnonzero(D[i] == D[i].min())[0] for i in range(len(m))])
    assert np.array_equal(nn, first)
    k = {2: 1, 4: 2, 8: 3}[ways]
    assert np.all(s.astype(np.float64) ** 2 <= k * (c["h"] / 2) ** 2 * (1 + 4 * U))


def test_nan_point_never_wins():
    c = cases.nan_point()
    e, s, nn = ref.detail(c["est"][0], c["gt"][0], c["model"])
    at = c["at"]
    assert np.isinf(e[at]) and np.isinf(s[at]) and nn[at] == -1
    rest = np.arange(len(e)) != at
    assert np.all(nn[rest] != at) and np.all(nn[rest] >= 0) and np.all(np.isfinite(s[rest])) and np.all(np.isfinite(e[rest]))
    rec = ref.records(c["est"], c["gt"], c["model"])[0]
    assert rec["valid"] == 1 and np.isinf(rec["add_max"]) and np.isinf(rec["adds_max"]) and rec["adds_fix"] >= (1 << 47)


def test_far_apart_saturates():
    c = cases.far_apart()
    rec = ref.records(c["est"], c["gt"], c["model"])[0]
    M = len(c["model"])
    assert rec["add_fix"] == M * (1 << 47) and rec["adds_fix"] == M * (1 << 47) and rec["add"] == F(32768) and rec["adds"] == F(32768)
    assert 0.9e6 < rec["adds_max"] <= rec["add_max"] < 1.1e6 and rec["valid"] == 1


def test_overflow_gives_inf_and_stays_valid():
    c = cases.overflow()
    rec = ref.records(c["est"], c["gt"], c["model"])
    assert np.all(rec["valid"] == 1) and np.all(np.isinf(rec["add_max"])) and np.all(np.isinf(rec["adds_max"]))
    assert np.all(rec["add"] == F(32768))
    _, s, nn = ref.detail(c["est"][0], c["gt"][0], c["model"])
    assert np.all(np.isinf(s)) and np.all(nn == -1)


def test_invalid_poses():
    c = cases.invalid_poses()
    rec = ref.records(c["est"], c["gt"], c["model"])
    assert np.array_equal(rec["valid"], c["valid"])
    bad = rec[c["valid"] == 0]
    assert np.all(bad["add_fix"] == 0) and np.all(bad["adds_fix"] == 0)
    for k in ("add", "add_max", "adds", "adds_max"):
        assert np.all(np.isposinf(bad[k])), k


def test_diameter_tie():
    c = cases.diameter_tie()
    m = c["model"]
    D = ref.sqdist(m[:, None, :], m[None, :, :])
    assert (np.triu(D == D.max(), 1)).sum() == 4 and D.max() == c["d2"]     # four space diagonals, exactly equal
    assert ref.diameter(m) == np.sqrt(c["d2"])


def test_model_sizes_cover_the_header_sizes():
    k = cases.kernel_sizes()
    s = cases.model_sizes()
    for v in k.values():
        assert {v - 1, v, v + 1} <= set(s)
    assert {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097} <= set(s)
