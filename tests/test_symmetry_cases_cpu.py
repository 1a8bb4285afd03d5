"""The conditions that keep the symmetry GPU tests honest, checked without a GPU: every search case has the margins it is named for (float64
brute force), the restated search finds on float64 scores what each case was built with, and on the kernel cases the float32 restatement
agrees with the existing pose-error restatement wherever a point is matched and shows what each case is named for."""
import math
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pose_error_ref as base  # noqa: E402
import symmetry_cases as cases  # noqa: E402
import symmetry_ref as ref  # noqa: E402

F = np.float32
KERNEL = cases.kernel_cases()
SEARCH = sorted(cases.SEARCH_CASES)


# ---- search cases: tolerances and margins ----
@pytest.mark.parametrize("name", SEARCH)
def test_expected_generators_lie_well_inside_the_tolerance(name):
    c = cases.search_case(name)
    tol = float(c["tol_resolved"])
    for axis, order in c["expect"]:
        for n in ([order] if order else range(2, 7)):
            r = ref.record64(ref.rotation(axis, 360.0 / n, c["center"]), c["model"], c["normals"], tol)
            assert r["n_far"] == 0 and r["max"] <= tol / 4, (axis, n, r)


@pytest.mark.parametrize("name", SEARCH)
def test_false_orders_and_false_axes_lie_well_outside(name):
    c = cases.search_case(name)
    tol = float(c["tol_resolved"])
    trials = [(a, n) for a in c["false_axes"] for n in range(2, 7)]
    for axis, order in c["expect"]:
        if order:
            trials += [(axis, n) for n in range(2, 7) if order % n]
    for axis, n in trials:
        r = ref.record64(ref.rotation(axis, 360.0 / n, c["center"]), c["model"], c["normals"], 4 * tol)
        assert r["n_far"] > 0 or r["max"] >= 4 * tol, (axis, n, r)
        r = ref.record64(ref.rotation(axis, 360.0 / n, c["center"]), c["model"], c["normals"], tol)
        assert r["n_far"] > 0, (axis, n, r)


def test_no_candidate_of_the_default_coarse_set_passes_on_the_blob_even_at_twice_the_tolerance():
    c = cases.search_case("blob")
    tol2 = 2 * float(c["tol_resolved"])
    dirs = ref.axes(ref.DEFAULTS["n_axes"])
    T = np.stack([ref.rotation(d, 360.0 / n, c["center"]) for d in dirs for n in range(2, ref.DEFAULTS["max_order"] + 1)])
    rec = ref.scorer64(c["model"], c["normals"], tol2)(T)
    assert len(rec) == 2048 * 5 and np.all((rec["n_far"] > 0) | (rec["max"] > tol2))


def test_the_kd_tree_scorer_is_the_brute_force():
    c = cases.search_case("c3_tilted")
    tol = float(c["tol_resolved"])
    rng = np.random.default_rng(0)
    T = np.stack([ref.rotation(C, 120.0, c["center"]) for C in (cases.C3_AXIS, (0, 0, 1))] + [cases.small_motion(rng, 4.0, 0.002) for _ in range(4)])
    got = ref.scorer64(c["model"], c["normals"], tol)(T)
    for k in range(len(T)):
        w = ref.record64(T[k], c["model"], c["normals"], tol)
        assert got[k]["n_far"] == w["n_far"] and got[k]["n_normal_bad"] == w["n_normal_bad"]
        assert got[k]["max"] == F(w["max"]) and got[k]["mean"] == F(w["mean"])


# ---- the restated search on float64 scores ----
@pytest.mark.parametrize("name", SEARCH)
def test_restated_search_returns_what_the_case_was_built_with(name):
    c = cases.search_case(name)
    axes, S, sym3, flags = cases.search_restated(name)
    assert len(axes) == len(c["expect"]) and len(S) == c["K"] and flags == c["flags"]
    assert np.array_equal(sym3, np.asarray(c["sym3"], F))
    bound = cases.axis_bound_deg()
    assert bound == pytest.approx(math.degrees(2 * math.sqrt(2 * math.pi / 2045) / 16))
    left = list(c["expect"])
    for a in axes:
        k = int(np.argmin([cases.angle_deg(a["axis"], e[0]) for e in left]))
        assert cases.angle_deg(a["axis"], left[k][0]) <= bound and a["order"] == left[k][1], (a, left[k])
        left.pop(k)
    assert np.array_equal(S[0], ref.IDENTITY)
    assert float(axes["mean"].max(initial=0)) <= float(c["tol_resolved"]) / 4


def test_the_restated_set_of_the_tilted_c3_is_the_three_turns():
    c = cases.search_case("c3_tilted")
    _, S, _, _ = cases.search_restated("c3_tilted")
    want = [ref.rotation64(cases.C3_AXIS, 120.0 * k, (0.01, -0.02, 0.03)) for k in range(3)]
    for k in range(3):
        got = S[k].reshape(4, 4).T.astype(np.float64)
        assert min(np.abs(got - w).max() for w in want) < 2e-3


# ---- kernel cases: the float32 restatement against the existing one, and what each case is named for ----
@pytest.mark.parametrize("name", sorted(KERNEL))
def test_restatement_agrees_with_the_pose_error_restatement_where_matched(name):
    c = KERNEL[name]
    for T in c["transforms"]:
        s, nn, dot, matched, _ = ref.detail(T, c["model"], c["normals"], c["reach"], c["cos_normal"])
        _, ws, wnn = base.detail(T, ref.IDENTITY, c["model"])
        assert s[matched].tobytes() == ws[matched].tobytes() and np.array_equal(nn[matched], wnn[matched])
        assert np.all(np.isinf(s[~matched])) and np.all(nn[~matched] == -1) and np.all(dot[~matched] == 0)


@pytest.mark.parametrize("name", sorted(KERNEL))
def test_identity_gives_zero(name):
    c = KERNEL[name]
    m = c["model"]
    ok = np.isfinite(m).all(1)
    r = ref.record(ref.IDENTITY, m, c["normals"], c["reach"])
    assert r["sum_fix"] == int(base.fix(np.full(int((~ok).sum()), c["reach"], F)).sum(dtype=np.uint64)) and r["max"] == 0 and r["n_far"] == int((~ok).sum())
    _, nn, _, _, _ = ref.detail(ref.IDENTITY, m, c["normals"], c["reach"])
    first = np.array([int(np.flatnonzero((m == m[i]).all(1))[0]) if ok[i] else -1 for i in range(len(m))])
    assert np.array_equal(nn, first)


def test_lattice_points_sit_on_cell_corners_and_ties_span_cells():
    for flip in (False, True):
        c = cases.lattice_case(flip)
        m, h = c["model"], c["h"]
        for r in c["reaches"].values():
            edge, o = ref.grid_edge(r, m)
            assert edge == h                                   # the box sets the edge: GRID_SPAN cells of h
            u = (m - o) * (F(1) / edge)
            assert u.dtype == F and np.array_equal(u, np.floor(u))
        wide = c["reaches"]["wide"]
        for t, ways in ((3, 2), (4, 4), (5, 8)):
            p = base.transform(c["transforms"][t], m)
            D = base.sqdist(p[:, None, :], m[None, :, :])
            inner = np.flatnonzero((D == D.min(1, keepdims=True)).sum(1) == ways)
            assert len(inner) > 0
            i = inner[0]
            tied = np.flatnonzero(D[i] == D[i].min())
            cells = {tuple(np.floor((m[j] - o) / edge).astype(int)) for j in tied}
            assert len(cells) == ways and D[i].min() <= wide * wide
            _, nn, _, matched, _ = ref.detail(c["transforms"][t], m, c["normals"], wide)
            assert matched[i] and nn[i] == tied.min()
            if flip:   # the lowest index lies in the cell with the highest coordinates
                assert tuple(np.floor((m[tied.min()] - o) / edge).astype(int)) == max(cells)


@pytest.mark.parametrize("lowest_last", [True, False])
def test_three_targets_tie_across_three_cells_and_the_lowest_index_wins(lowest_last):
    c = cases.three_way_case(lowest_last)
    m, i = c["model"], c["query"]
    edge, o = ref.grid_edge(c["reach"], m)
    assert edge == c["s"]                                  # the box sets the edge
    p = base.transform(c["transforms"][0], m)
    D = base.sqdist(p[i][None, :], m)
    tied = np.flatnonzero(D == D.min())
    ways = len(tied)
    assert ways == 3 and sorted(tied) == [0, 1, 2] and D.min() == c["a"] * c["a"] and D.min() <= c["reach"] * c["reach"]
    cell = lambda x: tuple(np.floor((x - o) * (F(1) / edge)).astype(int))
    cells = [cell(m[j]) for j in tied]
    assert len(set(cells)) == 3 and cell(p[i]) == (1, 1, 1) and cell(p[i]) not in cells
    assert all(max(abs(a - b) for a, b in zip(cl, (1, 1, 1))) == 1 for cl in cells)
    order = sorted(range(3), key=lambda k: (cells[k][2], cells[k][1], cells[k][0]))   # the walk: z, then y, then x ascending
    assert order[-1 if lowest_last else 0] == 0            # target 0, the lowest index, is met last (first)
    _, nn, _, matched, _ = ref.detail(c["transforms"][0], m, c["normals"], c["reach"])
    assert matched[i] and nn[i] == 0


def test_pairs_exactly_at_the_reach_and_one_ulp_off():
    c = cases.lattice_case(False)
    m, T = c["model"], c["transforms"][3]
    at, below, above = c["reaches"]["at"], c["reaches"]["below"], c["reaches"]["above"]
    D = base.nearest(base.transform(T, m), m)[0]
    assert np.all(D == at * at) and below < at < above
    assert ref.record(T, m, c["normals"], at)["n_far"] == 0 and ref.record(T, m, c["normals"], above)["n_far"] == 0
    r = ref.record(T, m, c["normals"], below)
    assert r["n_far"] == len(m) and r["max"] == 0 and r["sum_fix"] == len(m) * int(base.fix(below))


def test_outside_duplicates_and_normals_hold_what_they_are_named_for():
    c = cases.outside_case()
    rec = ref.records(c["transforms"], c["model"], c["normals"], c["reach"])
    M = len(c["model"])
    assert rec[0]["n_far"] == M and rec[3]["n_far"] == M and rec[0]["max"] == 0 and rec[0]["sum_fix"] == M * int(base.fix(c["reach"]))
    lo, hi = c["model"].min(0), c["model"].max(0)
    inside = np.all((base.transform(c["transforms"][1], c["model"]) >= lo) & (base.transform(c["transforms"][1], c["model"]) <= hi), axis=1)
    assert 0.25 * M <= inside.sum() <= 0.75 * M and 0 < rec[1]["n_far"] < M
    assert rec[2]["n_far"] == M
    c = cases.duplicates_case()
    _, nn, _, matched, _ = ref.detail(c["transforms"][1], c["model"], c["normals"], c["reach"])
    assert matched.any() and np.all(nn[matched] < len(nn) // 2)
    c = cases.bad_normals_case()
    s, nn, dot, matched, _ = ref.detail(ref.IDENTITY, c["model"], c["normals"], c["reach"], c["cos_normal"])
    assert matched.all() and np.isnan(dot[5]) and dot[9] == 0 and ref.record(ref.IDENTITY, c["model"], c["normals"], c["reach"])["n_normal_bad"] == 2
    n = ref.unit_normals(c["normals"])
    ok = np.ones(len(n), bool); ok[[5, 9]] = False
    assert np.abs(np.linalg.norm(n[ok].astype(np.float64), axis=1) - 1).max() < 1e-6
    c = cases.nan_point_case()
    for T in c["transforms"]:
        s, nn, _, matched, _ = ref.detail(T, c["model"], c["normals"], c["reach"])
        assert not matched[c["at"]] and not np.any(nn == c["at"])


def test_span_cases_straddle_the_grid_span():
    span = cases.kernel_sizes()["GRID_SPAN"]
    for k in (span - 1, span, span + 1):
        c = cases.span_case(k)
        m = c["model"]
        ext = float((m.max(0).astype(np.float64) - m.min(0).astype(np.float64)).max())
        edge, _ = ref.grid_edge(c["reach"], m)
        by_reach = F(float(c["reach"]) * 65.0 / 64.0)
        assert (edge == by_reach) == (k <= span) or abs(float(by_reach) - ext / span) < 1e-9
        assert edge >= by_reach


def test_float32_restatement_is_near_the_float64_brute_force():
    c = KERNEL["random_M257"]
    for T in c["transforms"]:
        r, w = ref.record(T, c["model"], c["normals"], c["reach"]), ref.record64(T, c["model"], c["normals"], float(c["reach"]))
        assert abs(int(r["n_far"]) - w["n_far"]) <= 1 and abs(float(r["max"]) - w["max"]) < 1e-6 + 0.01 * (r["n_far"] != w["n_far"])
        assert abs(float(r["mean"]) - w["mean"]) < 1e-6 + float(c["reach"]) / 257
