"""The refinement's reference (oracle/refine_oracle.py) checked against itself, so that a failure of tests/test_refine_edges_gpu.py
can only be the kernel's: brute force against a kd-tree, no ambiguity in the constructed cases, ties / thresholds / cell faces that
really are exact, the grid branches the cases are meant to take, and the one-iteration pose in two precisions.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest
from scipy.spatial import cKDTree

from oracle import refine_oracle as ro

F = np.float32
CASES = ro.all_cases()
CONSTRUCTED = [c for c in CASES if c.exact or c.family == "cell_faces"]
RANDOM = [c for c in CASES if c.family.startswith("random_")]


def _ids(cs):
    return [c.id for c in cs]


@pytest.fixture(scope="module")
def classified():
    out = {}
    for c in CASES:
        sc, mc, src = c.held()
        out[c.id] = (sc, mc, src, ro.classify(src, mc))
    return out


def test_every_family_is_there():
    fam = {c.family for c in CASES}
    assert fam >= {"lattice_ties", "duplicates", "cell_faces", "prune_margin", "box_and_threshold", "grid_shapes", "lds_budget", "octant_switch", "millimetres", "n_src",
                   "random_uniform", "random_clustered", "random_surface"}
    assert {c.name for c in CASES if c.family == "n_src"} == {str(n) for n in ro.N_SRC}
    assert {c.name for c in CASES if c.family == "grid_shapes"} == {"single_point", "collinear", "planar", "one_cell", "cell_cap"}


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_brute_force_equals_kdtree_on_clear_points(case, classified):
    sc, mc, src, cl = classified[case.id]
    if len(src) == 0:
        return
    _, j = cKDTree(mc.astype(np.float64)).query(src.astype(np.float64))
    clear = cl["cls"] == ro.CLEAR
    assert np.array_equal(j[clear], cl["low"][clear])


@pytest.mark.parametrize("case", CONSTRUCTED, ids=_ids(CONSTRUCTED))
def test_constructed_cases_are_centred_and_unambiguous(case, classified):
    sc, mc, src, cl = classified[case.id]
    assert np.array_equal(ro.centre(case.scene)[1], np.zeros(3, F)) and np.array_equal(ro.centre(case.model)[1], np.zeros(3, F))
    assert np.array_equal(sc, case.scene) and np.array_equal(mc, case.model)
    assert ro.ambiguous_share(src, mc, case.dist, case.exact, cl) == 0.0   # cell_faces: the threshold band is empty too


@pytest.mark.parametrize("case", RANDOM, ids=_ids(RANDOM))
def test_random_cases_ambiguous_share_is_capped(case, classified):
    sc, mc, src, cl = classified[case.id]
    assert ro.ambiguous_share(src, mc, case.dist, False, cl) <= 0.01
    g = ro.predict_grid(mc, case.dist)
    m, k = ro.expected_detail(src, mc, case.dist, g, cl)
    assert k.sum() >= 0.3 * len(src) and (m < 0).sum() >= 0.02 * len(src)      # both outcomes are exercised


def _exact_d2(s, t):
    return sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(s, t))


@pytest.mark.parametrize("case", [c for c in CASES if "ties" in c.expect], ids=[c.id for c in CASES if "ties" in c.expect])
def test_intended_ties_are_bitwise(case, classified):
    sc, mc, src, cl = classified[case.id]
    assert case.expect["ties"] <= set(cl["ntie"].tolist())
    tied = np.nonzero(cl["ntie"] >= 2)[0]
    assert len(tied) >= 50
    # lowest index is not simply the first of the tied points in cell order: among the tied sets the winner's cell key is often larger
    for i in tied[:60]:
        d = ((src[i].astype(np.float64) - mc.astype(np.float64)) ** 2).sum(1)
        mem = np.nonzero(d == cl["d1"][i])[0]
        assert len(mem) == cl["ntie"][i] and mem[0] == cl["low"][i]
        ex = {_exact_d2(src[i], mc[j]) for j in mem}
        assert len(ex) == 1                                                       # equal as rationals, not only after rounding
        v = float(ex.pop())
        assert float(F(v)) == v                                                   # and a float32: the kernel's fma chain rounds nowhere
        # float32 restatement of the kernel's expression gives the same bits for every member
        dd = (src[i][None, :] - mc[mem]).astype(F)
        f = (dd[:, 2] * dd[:, 2] + (dd[:, 1] * dd[:, 1] + dd[:, 0] * dd[:, 0]).astype(F)).astype(F)
        assert len(set(f.view(np.uint32).tolist())) == 1 and float(f[0]) == v


def test_lowest_index_is_not_first_in_cell_order(classified):
    case = next(c for c in CASES if c.family == "lattice_ties")
    sc, mc, src, cl = classified[case.id]
    g = ro.predict_grid(mc, case.dist)
    cell = lambda p: tuple(int(np.floor(ro.cell_units(g, p[k], k))) for k in range(3))
    key = lambda p: (lambda c: (c[2] * g["n3"][1] + c[1]) * g["n3"][0] + c[0])(cell(p))
    later = 0
    for i in np.nonzero(cl["ntie"] >= 2)[0][:200]:
        d = ((src[i].astype(np.float64) - mc.astype(np.float64)) ** 2).sum(1)
        mem = np.nonzero(d == cl["d1"][i])[0]
        later += int(key(mc[mem[0]]) > min(key(mc[j]) for j in mem[1:]))
    assert later >= 20


def test_threshold_and_box_points_are_exact(classified):
    case = next(c for c in CASES if c.family == "box_and_threshold")
    sc, mc, src, cl = classified[case.id]
    g = ro.predict_grid(mc, case.dist)
    D2 = float(F(case.dist)) ** 2
    F2 = float(F(D2 * (1.0 + 1e-5)))
    inside = ro.in_box(g, src)
    on = cl["d1"] == D2
    assert on.sum() >= 2 * 27 * 6
    for i in np.nonzero(on)[0][:40]:
        assert _exact_d2(src[i], mc[cl["low"][i]]) == Fraction(D2)
    just_over = (cl["d1"] > D2) & (cl["d1"] <= F2 * (1 - ro.MARGIN))
    assert (just_over & inside).sum() >= 100 and (just_over & ~inside).sum() >= 50    # found but not counted / one float outside the box
    on_box = ((src == g["lo"]) | (src == g["hi"])).any(1) & inside
    assert (on_box & on).sum() >= 50                                                  # exactly on the widened box, exactly at the distance
    assert (cl["d1"] > F2 * 2).sum() >= 100                                           # well beyond: nothing
    m, k = ro.expected_detail(src, mc, case.dist, g, cl)
    assert ((m >= 0) & (k == 0)).sum() >= 100


@pytest.mark.parametrize("n_half", [1300, 300])
def test_cell_face_coordinates_reproduce_floorf_on_both_sides(n_half):
    case = ro.cell_faces(n_half)
    mc = ro.centre(case.model)[0]
    g = ro.predict_grid(mc, case.dist)
    assert g["octants"] == case.expect["octants"] == (n_half == 1300)
    n_face = 0
    for k in range(3):
        for face in range(g["n3"][k] + 1):
            for half in (False, True):
                lo, hi = ro.face_floats(g, k, face, half)
                t = face + (0.5 if half else 0.0)
                assert hi == np.nextafter(lo, F(np.inf)) and ro.cell_units(g, lo, k) < t <= ro.cell_units(g, hi, k)
                if not half:
                    assert int(np.floor(ro.cell_units(g, lo, k))) == face - 1 and int(np.floor(ro.cell_units(g, hi, k))) == face
                n_face += int(((case.scene[:, k] == lo) | (case.scene[:, k] == hi)).sum())
    assert n_face >= 200


PRUNE = [c for c in CASES if c.family == "prune_margin"]


def _box_of(g, p, octant):
    """the cell (octant: and the half of each axis) refine_keys_kernel files model point p under -> (lower corner in cell units, size)"""
    lo = []
    for k in range(3):
        u = ro.cell_units(g, p[k], k)
        c = min(max(int(np.floor(u)), 0), g["n3"][k] - 1)
        lo.append(c + (0.5 if octant and u - F(c) >= F(0.5) else 0.0))
    return lo, 0.5 if octant else 1.0


@pytest.mark.parametrize("case", PRUNE, ids=_ids(PRUNE))
def test_prune_margin_instances_need_the_margin(case, classified):
    sc, mc, src, cl = classified[case.id]
    g = ro.predict_grid(mc, case.dist)
    kinds = {i["kind"] for i in case.instances}
    assert len(case.instances) >= 10 and {("face", 0), ("face", 1), ("face", 2)} <= kinds
    if g["octants"]:
        assert any(kd[0] == "mid-plane" for kd in kinds)
    assert (cl["ntie"] == 2).all()
    for n, ins in enumerate(case.instances):
        s, p, q, r = ins["s"], ins["p"], ins["q"], ins["r"]
        assert np.array_equal(src[2 * n], s) and np.array_equal(mc[2 * n], q) and np.array_equal(mc[2 * len(case.instances) + 2 * n], p)
        assert cl["low"][2 * n] == 2 * n                                            # q, the lower index, is the expected match
        assert _exact_d2(s, p) == _exact_d2(s, q) == Fraction(r) ** 2 and float(F(r * r)) == r * r
        # q is the first float beyond its plane: moving it one float towards s puts it into the source's cell (or octant)
        half = ins["kind"][0] == "mid-plane"
        k = ins["kind"][1]
        lo_q, size = _box_of(g, q, half)
        step = q.copy(); step[k] = np.nextafter(q[k], s[k])
        assert _box_of(g, step, half)[0][k] != lo_q[k] and _box_of(g, s, half) == _box_of(g, p, half)
        # the walk's bound on q's box: above the tied distance without the margin (q's box would be pruned), far below it with it
        assert ro.box_bound(g, s, lo_q, size, 0.0) > F(r * r)
        assert ro.box_bound(g, s, lo_q, size, ro.margin_u(g)) < F(r * r) * F(1 - 1e-3)


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_prune_comparison_is_never_at_equality_for_the_nearest_points_box(case, classified):
    """With the margin in place the bound of the box that holds the expected match is 0 (own or adjoining box: compared with a
    positive key unless the source IS the model point, which lies in the source's own box) or lies below d1 by more than 1e-3 d1
    ((gap + margin)^2 against gap^2 with gap <= 1, margin >= 1e-3), a thousand times the float rounding of either side.  So `>` and
    `>=` in the prune are the same function on every box that matters: the comparison's strictness is not observable while
    margin_u is there, and the prune_margin cases hold margin_u."""
    sc, mc, src, cl = classified[case.id]
    g = ro.predict_grid(mc, case.dist)
    D2 = float(F(case.dist)) ** 2
    mu = ro.margin_u(g)
    idx = [i for i in range(len(src)) if cl["d1"][i] <= D2 and ro.in_box(g, src[i:i + 1])[0]][:250]
    for i in idx:
        for octant in ((False, True) if g["octants"] else (False,)):
            lo, size = _box_of(g, mc[cl["low"][i]], octant)
            b = float(ro.box_bound(g, src[i], lo, size, mu))
            assert b == 0.0 or b < cl["d1"][i] * (1 - 1e-3), (i, b, cl["d1"][i])
            if cl["d1"][i] == 0.0:
                assert _box_of(g, src[i], octant)[0] == lo


@pytest.mark.parametrize("case", [c for c in CASES if c.expect], ids=[c.id for c in CASES if c.expect])
def test_grid_branch_predictions(case):
    mc = ro.centre(case.model)[0]
    g = ro.predict_grid(mc, case.dist)
    e = case.expect
    if "lds" in e:
        assert g["lds"] == e["lds"]
        nM = len(mc)
        assert abs(nM * 16 + (8 * g["cells"] + 1) * 4 - ro.LDS_BYTES) <= 32 + 28     # within two points of the budget
    if "octants" in e:
        assert g["octants"] == e["octants"]
        if case.family == "octant_switch":
            assert abs(len(mc) - 32 * g["cells"]) <= 2
    if "cells" in e:
        assert g["cells"] == e["cells"]
    if "thin" in e:
        assert all(g["n3"][k] == 1 for k in e["thin"]) and max(g["n3"]) > 1
    if "raised" in e:
        ext = (mc.max(0) - mc.min(0)).astype(np.float64)
        h0 = float(F(F(case.dist) * F(1.001)))
        assert np.prod(np.floor(ext / h0) + 1) > ro.MAX_CELLS                         # from the model's extent: the first edge does not fit
        assert g["raised"] >= 1 and g["cells"] <= ro.MAX_CELLS and float(g["h"]) > h0


def test_budget_pairs_share_everything_but_late_duplicates():
    for fam in ("lds_budget", "octant_switch"):
        a, b = [c for c in CASES if c.family == fam]
        assert np.array_equal(a.scene, b.scene) and np.array_equal(b.model[:len(a.model)], a.model) and len(b.model) == len(a.model) + 2
        assert all((a.model == p).all(1).any() for p in b.model[len(a.model):])


def test_exact_sums_two_ways():
    case = next(c for c in CASES if c.family == "random_surface")
    sc, mc, src = case.held()
    g = ro.predict_grid(mc, case.dist)
    m, k = ro.expected_detail(src[:250], mc, case.dist, g)
    n = case.unit_normals()
    a, ba = ro.exact_sums(src[:250], mc, n, m, k, use_fractions=True)
    b, bb = ro.exact_sums(src[:250], mc, n, m, k, use_fractions=False)
    assert k.sum() > 50 and a[27] == k.sum()
    assert (np.abs(a - b) <= 0.01 * ba + 1e-300).all() and np.array_equal(ba, bb)


POSE = [c for c in CASES if c.family in ro.POSE_FAMILIES]


@pytest.mark.parametrize("case", POSE, ids=_ids(POSE))
def test_one_iteration_pose_in_two_precisions(case, classified):
    sc, mc, src, cl = classified[case.id]
    g = ro.predict_grid(mc, case.dist)
    m, k = ro.expected_detail(src, mc, case.dist, g, cl)
    n = case.unit_normals()
    Td, cond = ro.one_iteration(case.T16, src, mc, n, m, k, np.float64)
    Tl, _ = ro.one_iteration(case.T16, src, mc, n, m, k, np.longdouble)
    tol = ro.pose_tolerance(Tl, cond)
    assert (np.abs(Td[:3, :] - Tl[:3, :]).astype(np.float64) <= 0.25 * tol).all(), (np.abs(Td[:3, :] - Tl[:3, :]).max(), tol.min(), cond)


def test_scaled_hypothesis_pose_in_two_precisions(classified):
    """the non-rigid hypothesis of tests/test_refine_edges_gpu.py: its source comes from the general inverse"""
    case = next(c for c in CASES if c.family == "random_surface")
    sc, mc, _, _ = classified[case.id]
    T = ro.scaled_hyp(case.T16)
    src = ro.source_general(sc, T)
    g = ro.predict_grid(mc, case.dist)
    cl = ro.classify(src, mc)
    assert ro.ambiguous_share(src, mc, case.dist, False, cl) <= 0.01
    m, k = ro.expected_detail(src, mc, case.dist, g, cl)
    assert k.sum() >= 100
    n = case.unit_normals()
    Td, cond = ro.one_iteration(T, src, mc, n, m, k, np.float64)
    Tl, _ = ro.one_iteration(T, src, mc, n, m, k, np.longdouble)
    tol = ro.pose_tolerance(Tl, cond)
    assert (np.abs(Td[:3, :] - Tl[:3, :]).astype(np.float64) <= 0.25 * tol).all(), (np.abs(Td[:3, :] - Tl[:3, :]).max(), tol.min(), cond)
