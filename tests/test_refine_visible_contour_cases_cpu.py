"""The numpy restatement of the contour term (tests/refine_visible_contour_ref.py) against a brute-force scan, against the damped
restatement and against itself, without a GPU: the nearest map on built silhouettes with the tie rule and windows cut by the frame, one
case per state, the gate at its edge, the linearisation of the three rows, the two equalities with the damped form, the price of a shed
pixel, and the capture case: a start that the damped form leaves frozen and the contour term brings nearer."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import refine_visible_contour_cases as cc  # noqa: E402
import refine_visible_contour_ref as cref  # noqa: E402
import refine_visible_damped_ref as dref  # noqa: E402
import refine_visible_ref as ref  # noqa: E402

F = np.float32


def brute_nearest(present, r, c, R):
    """a scan of the window pixel by pixel: the first pixel in index order with the smallest d2"""
    H, W = present.shape
    best, at = None, -1
    for rs in range(max(r - R, 0), min(r + R, H - 1) + 1):
        for cs in range(max(c - R, 0), min(c + R, W - 1) + 1):
            if present[rs, cs]:
                d2 = (rs - r) ** 2 + (cs - c) ** 2
                if best is None or d2 < best:
                    best, at = d2, rs * W + cs
    return at


def _silhouettes():
    H, W = 40, 48
    out = {}
    a = np.zeros((H, W), bool); a[17, 23] = True
    out["one_pixel"] = a
    a = np.zeros((H, W), bool); a[10:22, 14:30] = True
    out["box"] = a
    a = np.zeros((H, W), bool)
    for r in range(12):
        a[4 + r, 5: 5 + r + 1] = True
        a[22 + r, 40 - r: 41] = True
    out["two_triangles"] = a
    a = np.zeros((H, W), bool)
    for r, c in ((5, 10), (5, 16), (20, 8), (26, 8), (30, 30), (34, 34)):
        a[r, c] = True
    out["ties"] = a
    a = np.zeros((H, W), bool); a[0:3, 0:4] = True; a[H - 2:, W - 3:] = True; a[0:2, W - 5:] = True; a[H - 1, 0:2] = True; a[18:20, 0] = True; a[19, W - 1] = True
    out["edges_and_corners"] = a
    return out


@pytest.mark.parametrize("name", sorted(_silhouettes()))
@pytest.mark.parametrize("R", [1, 3, 7, 64])
def test_the_nearest_map_is_a_brute_force_scan_of_the_window(name, R):
    present = _silhouettes()[name]
    H, W = present.shape
    got = cref.nearest_map(present, ~present, R)
    for r in range(H):
        for c in range(W):
            want = -1 if present[r, c] else brute_nearest(present, r, c, R)
            assert got[r * W + c] == want, (r, c, got[r * W + c], want)


def test_the_tie_rule_takes_the_lowest_linear_index():
    present = _silhouettes()["ties"]
    W = present.shape[1]
    near = cref.nearest_map(present, ~present, 8)
    assert near[5 * W + 13] == 5 * W + 10          # between two seeds of a row: the left one
    assert near[23 * W + 8] == 20 * W + 8          # of a column: the upper one
    assert near[32 * W + 32] == 30 * W + 30        # on a diagonal: the upper left one
    assert near[30 * W + 34] == 30 * W + 30 and near[34 * W + 30] == 30 * W + 30   # the other diagonal: the upper row wins again


def _pass(case, pose=None, **kw):
    pose = case.start16 if pose is None else pose
    prm = dict(case.prm, **kw)
    ev = ref.evaluate(pose, *case.args(), **dict((k, prm[k]) for k in dref.BASE_KEYS if k in prm))
    rect = cref.rectangle(pose, case.verts, case.tris, case.K, case.W, case.H)
    return ev, cref.contour_pass(ev["keys"], rect, case.depth, case.prob, case.K, case.depth_scale, **prm), rect


def test_every_state_occurs_and_counts_add_up():
    case = cc.width_cases()[4]
    ev, cp, rect = _pass(case)
    st = cp["state"].reshape(case.H, case.W)
    assert all((st == k).any() for k in (cref.UNREACHED, cref.BEYOND, cref.PULLED, cref.NOT_WALKED))
    er0, er1, ec0, ec1 = cref.grown(rect, case.prm["pull_radius_px"], case.W, case.H)
    inside = np.zeros_like(st, bool); inside[er0: er1 + 1, ec0: ec1 + 1] = True
    assert not st[~inside].any() and not st[(ev["keys"] != ref.EMPTY_KEY).reshape(st.shape)].any()
    assert (st[inside & (ev["keys"] == ref.EMPTY_KEY).reshape(st.shape)] != 0).all()       # every pixel is an object pixel here
    assert cp["unreached"] + cp["beyond"] + cp["pulled"] == int((st != 0).sum()) and cp["sums"][27] == cp["pulled"] and len(cp["b"]) == 3 * cp["pulled"]
    assert ((cp["nearest"] >= 0) == (cp["state"] >= cref.BEYOND)).all()
    hole = cc.corner_case()
    _, cph, _ = _pass(hole)
    assert not cph["state"].reshape(hole.H, hole.W)[10:14, 12:20].any()                      # not object pixels


def test_the_gate_is_not_beyond_at_equality_and_beyond_one_float_above():
    case = cc.tie_case()
    ev, cp, _ = _pass(case)
    u = int(np.flatnonzero(cp["state"] == cref.PULLED)[0])
    s = int(cp["nearest"][u])
    # D of that pixel as the contract computes it: a pull_distance whose float square is exactly D, and the next float below
    z = (ev["keys"][s] >> np.uint64(32)).astype(np.uint32).view(F)
    fx, cx, fy, cy = (F(x) for x in case.K)
    W = case.W
    d = F(case.depth.reshape(-1)[u]) * F(case.depth_scale)
    p = [((F(s % W) - cx) / fx) * z, ((F(s // W) - cy) / fy) * z, z]
    q = [((F(u % W) - cx) / fx) * d, ((F(u // W) - cy) / fy) * d, d]
    e = [q[k] - p[k] for k in range(3)]
    D = e[0] * e[0] + (e[1] * e[1] + e[2] * e[2])
    root = F(np.sqrt(np.float64(D)))
    cands = [root, np.nextafter(root, F(0)), np.nextafter(root, F(1))]
    at = [x for x in cands if x * x == D]
    below = [x for x in cands if x * x < D]
    assert at and below, "the seeds are 3 pixels of 1/64 apart at z = 1: D is a square of a float"
    assert _pass(case, pull_distance=float(at[0]))[1]["state"][u] == cref.PULLED
    assert _pass(case, pull_distance=float(max(below)))[1]["state"][u] == cref.BEYOND


def test_the_three_rows_linearise_a_translation_and_a_rotation():
    rng = np.random.default_rng(3)
    p = rng.normal(0, 0.3, 3).astype(F); p[2] += F(1)
    for x in (np.array([0, 0, 0, 1e-6, -2e-6, 3e-6]), np.array([2e-6, -1e-6, 3e-6, 0, 0, 0])):
        q = (ref.delta_of(x) @ np.append(p.astype(np.float64), 1.0))[:3]          # the measurement lies where the motion x takes p
        A, b = cref.rows_of(p, (q - p.astype(np.float64)))
        assert np.abs(A @ x - b).max() <= 4 * np.abs(x).max() ** 2                # first order: the remainder is of second order
        assert np.linalg.matrix_rank(A.T @ A) == 3                                  # one pixel fixes three of the six


def test_weight_zero_and_no_object_pixel_are_the_damped_form_bit_for_bit():
    case = cc.small_solid_case()
    base = dict((k, v) for k, v in case.prm.items() if k not in cref.CONTOUR_DEFAULTS)
    want = dref.refine(case.start16, *case.args(), **base)
    empty = np.zeros_like(case.prob)
    for got in (cref.refine(case.start16, *case.args(), **dict(case.prm, contour_weight=0.0)),
                cref.refine(case.start16, case.verts, case.tris, case.depth, empty, case.K, case.depth_scale, **dict(case.prm, class_threshold=0.5))):
        w = want if got["record"]["object_px"] else dref.refine(case.start16, case.verts, case.tris, case.depth, empty, case.K, case.depth_scale, **dict(base, class_threshold=0.5))
        assert np.array_equal(got["pose"].view(np.uint32), w["pose"].view(np.uint32))
        assert all(np.float64(got["record"][k]).tobytes() == np.float64(w["record"][k]).tobytes() for k in w["record"])
        assert got["record"]["pulled"] == 0 and got["record"]["pull_rms"] == 0
        for a, b in zip(got["trace"], w["trace"]):
            assert np.array_equal(a["pose"].view(np.uint32), b["pose"].view(np.uint32))
            assert (np.float64(a["cost"]).tobytes(), a["lambda_"], a["accepted"], a["state"]) == (np.float64(b["cost"]).tobytes(), b["lambda_"], b["accepted"], b["state"])
    moved = cref.refine(case.start16, *case.args(), **case.prm)
    assert moved["record"]["pulled"] > 0 and not np.array_equal(moved["pose"], want["pose"])


def test_a_pose_that_sheds_object_pixels_pays_pull_d2_for_each():
    r = dict(counted=100, too_far=3, uncovered=10, pulled=4)
    S28, Sc28, w, md, pd = 1e-3, 2e-4, 1.0, 0.02, 0.03
    c0 = cref.cost_of(S28, Sc28, r, md, pd, w)
    pd2 = float(F(pd) * F(pd))
    for k in (1, 5):                 # k counted pixels of residual 0 leave the silhouette and are not reached: the divisor stays, the sum grows
        shed = dict(r, counted=r["counted"] - k, uncovered=r["uncovered"] + k)
        c1 = cref.cost_of(S28, Sc28, shed, md, pd, w)
        assert (r["counted"] + r["too_far"]) + w * r["uncovered"] == (shed["counted"] + shed["too_far"]) + w * shed["uncovered"]
        assert abs((c1 - c0) - k * pd2 / 113.0) <= 1e-18
    assert cref.cost_of(S28, Sc28, dict(r, counted=2, pulled=1), md, pd, w) == np.inf and cref.cost_of(S28, Sc28, dict(r, counted=0, pulled=2), md, pd, w) < np.inf


def test_the_capture_case_the_damped_form_freezes_and_the_contour_term_comes_nearer():
    case = cc.capture_case()
    base = dict((k, v) for k, v in case.prm.items() if k not in cref.CONTOUR_DEFAULTS)
    e0 = ref.vertex_error(case.start16, case.G16, case.verts)
    sil = np.flatnonzero((case.depth > 0).any(axis=0))
    shift_px = cc.CAPTURE_DX * case.K[0] / 0.80
    assert shift_px > sil.max() - sil.min() + 1 and shift_px < case.prm["pull_radius_px"]
    d = dref.refine(case.start16, *case.args(), **base)
    assert d["record"]["counted"] == 0 and d["record"]["frozen"] == 1 and np.array_equal(d["pose"].view(np.uint32), case.start16.view(np.uint32))
    c = cref.refine(case.start16, *case.args(), **case.prm)
    e1 = ref.vertex_error(c["pose"], case.G16, case.verts)
    print("CAPTURE e0 %.4f e_contour %.4f record %s" % (e0, e1, c["record"]))
    assert abs(e0 - 0.0900) < 5e-5 and abs(e1 - 0.0409) < 5e-4 and e1 < 0.5 * e0
    assert c["record"]["frozen"] == 0 and c["record"]["iterations"] == 12 and c["record"]["counted"] > 100 and c["record"]["pulled"] > 0
    costs = [row["cost"] for row in c["trace"] if row["accepted"]]
    assert all(b < a for a, b in zip(costs, costs[1:]))
