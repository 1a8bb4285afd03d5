"""The adversarial grid cases (grid_cases.py) checked against themselves on the CPU, so that none of them can pass vacuously on the
GPU: every query that was built for a face lands where it was meant to in the kernels' float arithmetic, the float32 reference
(grid_ref.py) agrees with a float64 brute force wherever the answer is not within 1e-5 of the radius or of a tie, every case has
hits and misses, and the list lengths, tie counts and threshold sides the cases are named after are what they hold.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_cases as cases  # noqa: E402
import grid_ref as ref  # noqa: E402

F = np.float32


@pytest.mark.parametrize("name", cases.NAMES)
def test_case_is_what_it_claims(name):
    case = cases.build(name)
    R = ref.reference(case)
    sc, cs, mc, cm = case["_centred"]
    nS, nM = len(sc), len(mc)
    assert nS == len(case["snrm"]) == len(case["sprob"]) == len(case["spix"]) and nM == len(case["mnrm"]) and nM <= 65535
    assert len(R) == len(case["T"]) >= 3
    # the geometry is fixed by the anchors alone
    geoms = {d: ref.geometry(sc, case["eps"], d) for d in case["divs"]}
    if case["box"] is not None:
        for d, g in geoms.items():
            a = cases.box_geoms(case["box"], case["eps"], (d,))[d]
            assert np.array_equal(a["origin"], g["origin"]) and a["cells"] == g["cells"] and a["inv_h"] == g["inv_h"]
    # 1. queries land where intended
    for ti, mi, d, axis, sub, k in case["intent"]:
        got = ref.cell_coord(R[ti]["q"][mi][None], geoms[d], sub)[0, axis] if d in geoms else k
        assert got == k, (name, ti, mi, d, axis, sub, k, got)
    if name.startswith(("faces", "extent")):
        per_div = {d: sum(1 for i in case["intent"] if i[2] == d) for d in case["divs"]}
        assert min(per_div.values()) >= 30, per_div
        assert any(i[4] == 4 for i in case["intent"]) and any(i[5] % 8 == 0 and i[4] == 1 for i in case["intent"])
    # 2. float32 reference against the float64 brute force, off the radius and off ties
    e = float(case["eps"])
    hits = misses = checked = 0
    for r in R:
        clear = (np.abs(r["dist64"] - e) > 1e-5 * e) & ((r["gap64"] > 1e-5 * np.maximum(r["dist64"], 1e-30)) | (r["dist64"] > e))
        assert np.array_equal(r["hit"][clear], r["hit64"][clear]), name
        checked += int(clear.sum()); hits += int((r["hit"] >= 0).sum()); misses += int((r["hit"] < 0).sum())
        w = r["hit"] >= 0
        assert np.all(r["d2"][w] <= ref.sq_eps(case["eps"])) and not np.any(r["counted"] & ~w)
    # 3. nothing passes vacuously
    assert hits >= case["min_hits"] and misses >= case["min_misses"], (name, hits, misses)
    assert checked >= (hits + misses) // 4, (name, checked, hits + misses)
    assert sum(int(r["counted"].sum()) for r in R) >= min(4, case["min_hits"] // 2) and any(r["score"] > 0 for r in R)
    assert any(np.any((r["hit"] >= 0) & ~r["counted"]) for r in R), "no hit with an opposed normal"


@pytest.mark.parametrize("name", ["faces", "faces_pow2", "radius", "radius_pow2"])
def test_scene_points_sit_a_few_float_steps_from_the_radius(name):
    case = cases.build(name)
    steps = np.asarray(case["partner_steps"])
    assert np.all(np.abs(steps) <= 5), (steps.min(), steps.max())
    assert (steps <= 0).sum() >= 32 and (steps > 0).sum() >= 32
    if name.startswith("radius"):
        for u in (-1, 0, 1):
            assert (steps == u).sum() >= 26, u
    # and the reference sees them so: at the identity the query of probe i is model point 2i, its scene point 2(i+1) (after the anchor)
    r = ref.reference(case)[0]
    n = len(steps)
    hit = r["hit"][0:2 * n:2]
    assert np.array_equal(hit[steps <= 0], (2 * (np.arange(n) + 1))[steps <= 0])
    assert np.all(hit[steps > 0] != (2 * (np.arange(n) + 1))[steps > 0])


def test_ties_are_exact_ties():
    case = cases.build("ties")
    r = ref.reference(case)[0]
    sc = case["_centred"][0]
    d2 = ref.d2_f32(r["q"], sc)
    m = d2.min(1)
    n_tied = (d2 == m[:, None]).sum(1)
    inside = m <= ref.sq_eps(case["eps"])
    for k in (2, 4, 8, 3):
        assert ((n_tied == k) & inside).sum() >= 12, k
    last = sc.shape[0] - 1 - np.argmax((d2 == m[:, None])[:, ::-1], axis=1)
    assert np.array_equal(r["hit"][inside], last[inside])


@pytest.mark.parametrize("name", ["lists", "lists_sparse"])
def test_list_lengths_and_the_prune_group_threshold(name):
    case = cases.build(name)
    sc = ref.reference(case) and case["_centred"][0]
    for d in case["divs"]:
        g = ref.geometry(sc, case["eps"], d)
        inc = ref.incidences(sc, g)
        ids, cnt = np.unique(inc["cell"], return_counts=True)
        for c, N in zip(case["cluster_centres"], cases.LIST_LENGTHS):
            k = np.floor((c - g["origin"].astype(np.float64)) / g["h64"]).astype(np.int64)
            cell = (k[2] * g["cells"][1] + k[1]) * g["cells"][0] + k[0]
            assert cnt[np.searchsorted(ids, cell)] == N, (d, N)
        assert inc["longest"] == 129
        if d == 1:
            assert (inc["n_incidences"] <= 12 * inc["n_cells"]) == (name == "lists_sparse"), (inc["n_incidences"], inc["n_cells"])


def test_sort_threshold_scenes_straddle_65536_incidences():
    lo, hi = cases.build("sort_below"), cases.build("sort_above")
    assert 2 <= len(hi["spos"]) - len(lo["spos"]) <= 4 and np.array_equal(hi["spos"][:len(lo["spos"])], lo["spos"])
    for case, above in ((lo, False), (hi, True)):
        g = ref.geometry(case["spos"], case["eps"], 1)
        n = ref.incidences(case["spos"], g)["n_incidences"]
        assert n == case["n_incidences_div1"] and (n >= 65536) == above and abs(n - 65536) < 200, n


def test_extent_ratios():
    for name, ratio in (("extent_500", 500), ("extent_4000", 4000), ("extent_max", cases.extent_ratio_max())):
        case = cases.build(name)
        g = ref.geometry(case["spos"], case["eps"], 1)
        assert abs(g["cells"][0] - ratio) < 16 and g["cells"][2] < 16
        bricks = g["bricks"][0] * g["bricks"][1] * g["bricks"][2]
        assert bricks < 31.0e6 and (name != "extent_max" or bricks > 29.0e6), bricks
        # the probes sit at the far corner: offsets from the origin of nearly the whole extent
        q = ref.reference(case)[0]["q"][[i[1] for i in case["intent"] if i[0] == 0]]
        w = case["worst_face_offsets"]
        assert (w > 0).sum() >= 12 and (w < 0).sum() >= 12
        if name == "extent_max":          # the kernels' faces are off by more than a thousandth of epsilon, either way
            assert w.max() > 1.2e-3 and w.min() < -1.0e-3, (w.min(), w.max())
        assert len(q) > 60 and np.all((q[:, :2] - g["origin"][:2]) > (ratio - 110) * float(case["eps"]))


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_answer_is_in_the_list_of_the_cell_the_kernels_look_in(name):
    """The grid's exactness claim, checked without a GPU: for every hit of the reference, the scene point lies within the build's
    inclusion radius of the box of the cell that the kernels' FLOAT arithmetic assigns the query to -- so the build lists it there.
    (At the largest extent over epsilon this fails with a radius of 1.001 epsilon: the kernels' faces are up to 1.5e-3 epsilon off.)"""
    case = cases.build(name)
    R = ref.reference(case)
    sc = case["_centred"][0]
    n = 0
    for d in case["divs"]:
        g = ref.geometry(sc, case["eps"], d)
        for r in R:
            w = r["hit"] >= 0
            cell = ref.cell_coord(r["q"][w], g)
            assert np.all(cell >= 0) and np.all(cell < np.array(g["cells"]))
            d2 = ref.box_dist2(sc[r["hit"][w]], cell, g)
            assert not np.any(d2 > g["r"] * g["r"]), (name, d, float(np.sqrt(d2.max())) / g["eps"], g["r"] / g["eps"])
            n += int(w.sum())
    assert n >= case["min_hits"]


def test_coincident_scene_centres_to_the_origin():
    case = cases.coincident(65535)
    sc, cs = ref.centre(case["spos"])
    assert not sc.any() and len(sc) == 65535
    r = ref.reference(case)[0]
    assert (r["hit"] == 65534).sum() >= 16 and (r["hit"] < 0).sum() >= 16 and set(np.unique(r["hit"])) == {-1, 65534}
