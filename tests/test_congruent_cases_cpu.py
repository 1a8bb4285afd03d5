"""The edge models of the congruent join (congruent_cases.py) checked against themselves on the CPU, so that none of them passes vacuously
on the GPU: from the oracle's index and the cell functions (the reference's own ref_index_pos / ref_index_normal where the reference
library was built, numpy restatements of them asserted equal otherwise) every edge a family is named after is actually reached, and
every base has the number of quads it was built to have -- a case in which nothing joins does not pass.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import congruent_cases as cases  # noqa: E402

F = np.float32
AXES = {(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)}


@pytest.fixture(scope="module")
def ref_cells():
    from oracle import pyref
    if not pyref.available():
        return None, None
    ra = pyref.RefAccel()
    return ra.index_pos_rows, ra.index_normal_rows


@pytest.fixture(scope="module")
def analysed(oracle_lib, ref_cells):
    memo = {}

    def get(name):
        if name not in memo:
            case = cases.build(name)
            orc = cases.make_oracle(oracle_lib, case)
            recs = cases.analyse(oracle_lib, orc, case, *ref_cells)
            if ref_cells[0] is not None:                     # the numpy restatement of the cell functions == the reference's own
                for a, b in zip(recs, cases.analyse(oracle_lib, orc, case)):
                    for s in "PQ":
                        assert np.array_equal(a[s]["cell"], b[s]["cell"]) and np.array_equal(a[s]["dcell"], b[s]["dcell"]), name
            quads = [orc.find_congruent(ids, float(inv[0]), float(inv[1])) for ids, inv in zip(case["ids"], case["inv"])]
            memo[name] = case, recs, quads
        return memo[name]
    return get


def _entries(recs, key):
    return np.concatenate([r[s][key] for r in recs for s in "PQ" if len(r[s][key])])


def _axes_on_faces(x):
    return ((x * F(cases.EG)) == np.rint(x * F(cases.EG))).sum(1)


def _axial(d):
    return {tuple(int(c) for c in v) for v in d if (np.abs(v) == 1).sum() == 1 and (v == 0).sum() == 2}


def _cell_coords(cell, n):
    return np.stack([cell % n, (cell // n) % n, cell // (n * n)], -1)


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_base_has_the_quads_it_was_built_to_have(analysed, name):
    case, recs, quads = analysed(name)
    assert len(case["ids"]) == len(case["expect_quads"]) >= 2
    assert [len(q) for q in quads] == list(case["expect_quads"]), name
    assert sum(len(q) > 0 for q in quads) >= len(quads) // 2
    assert set(np.unique(case["inv"]).tolist()) <= {0.0, 0.25, 0.5, 1.0}                       # dyadic invariants
    assert np.array_equal(case["mpos"][0::2], -case["mpos"][1::2])                            # point-mirrored, interleaved
    for ids in case["ids"]:
        assert (ids < len(case["mpos"]) - 2).all()                                            # no base uses an anchor


def test_lattice_reaches_cell_faces_and_the_exact_axes(analysed):
    """Intersection points with p * egSize exactly an integer on one, two and three axes (and none on no axis: x is always on a face);
    Q directions exactly +-x, +-y, +-z -- -z is the exactly anti-parallel branch of quat_from_z with its x2 == 0 axis choice -- and with
    them direction-cell coordinates 0 and 6 on every axis."""
    case, recs, _ = analysed("lattice")
    assert len(case["mpos"]) == 2 * (108 + 1)
    on = np.bincount(_axes_on_faces(_entries(recs, "x")), minlength=4)
    assert on[0] == 0 and on[1] >= 100 and on[2] >= 50 and on[3] >= 10, on
    qdirs = np.concatenate([r["Q"]["dir"] for r in recs])
    assert _axial(qdirs) == AXES
    assert sum((0, 0, -1) in _axial(r["Q"]["dir"]) for r in recs) >= 3
    dc = _cell_coords(_entries(recs, "dcell"), 7)
    for ax in range(3):
        assert {0, 6} <= set(dc[:, ax].tolist()), ax
    # every dyadic invariant occurs on both sides
    assert set(case["inv"][:, 0].tolist()) == set(case["inv"][:, 1].tolist()) == {0.0, 0.25, 0.5, 1.0}


@pytest.mark.parametrize("name", ["clusters", "clusters_64k"])
def test_cluster_runs_have_the_lengths_they_are_named_after(analysed, name):
    """Base k's P list has a run of exactly runs[k] entries in ONE position cell, Q entries of the base query that cell, and the whole run
    sits in one direction cell (so a histogram counter of join_count_kernel reaches the run length: 65 535 in the large case)."""
    case, recs, _ = analysed(name)
    want = {"clusters": (63, 64, 65, 255, 256, 260), "clusters_64k": (65535, 65536)}[name]
    assert case["runs"] == want
    for r, run in zip(recs, case["runs"]):
        hit = [c for c, n in r["runs"].items() if n == run and c in r["queried"]]
        assert len(hit) >= 1, (name, run, sorted(r["runs"].values())[-4:])
        c = hit[0]
        assert len(set(r["P"]["dcell"][r["P"]["cell"] == c].tolist())) == 1
        nq = int((r["Q"]["cell"] == c).sum())
        assert 12 <= nq <= 300, nq                             # a Q side of a few hundred entries at most
        # nothing sits on a face here: the clusters are at cell centres
        assert _axes_on_faces(r["P"]["x"][r["P"]["cell"] == c]).max() == 0


def test_borders_reach_the_first_and_last_cells(analysed):
    """Intersection points of both lists in position cells 0 and 127 of every axis, pair directions exactly along the axes there, direction-cell
    coordinates 0 and 6.  (A unit coordinate of exactly 0 or 1 cannot be built at this scale: ratio = extent + 0.001 > extent keeps every unit
    coordinate inside (0, 1) until the extent exceeds 2^15 m, where 0.001 is lost to rounding; the anchors sit at 0.0005 and 0.9995.)"""
    case, recs, _ = analysed("borders")
    for s in "PQ":
        pc = _cell_coords(np.concatenate([r[s]["cell"] for r in recs]), cases.EG)
        for ax in range(3):
            assert {0, 127} <= set(pc[:, ax].tolist()), (s, ax)
    unit = case["mpos"] + F(0.5)
    assert unit.min() == F(0.5) - cases.A_ANCHOR and unit.max() == F(0.5) + cases.A_ANCHOR and 0 < unit.min() < 1 / 128 and 127 / 128 < unit.max() < 1
    assert _axial(np.concatenate([r["Q"]["dir"] for r in recs])) == AXES
    dc = _cell_coords(_entries(recs, "dcell"), 7)
    for ax in range(3):
        assert {0, 6} <= set(dc[:, ax].tolist()), ax


def test_degenerate_models_are_degenerate(analysed):
    case, recs, quads = analysed("degenerate_coincident")
    _, counts = np.unique(case["mpos"], axis=0, return_counts=True)
    assert (counts == 2).sum() >= 50 and (counts == 3).sum() == 2      # every lattice point twice, one three times (and its mirror image)
    assert any((ids[:2] == ids[2:]).all() for ids in case["ids"])                                       # a base whose two pairs are the same pair
    case, recs, quads = analysed("degenerate_planar")
    assert (case["mpos"][:-2, 2] == 0).all() and any((ids[:2] == ids[2:]).all() for ids in case["ids"])
    case, recs, quads = analysed("degenerate_collinear")
    assert (case["mpos"][:-2, 1:] == 0).all()
    for r in recs:                                                                                      # every pair direction is exactly +-x
        for s in "PQ":
            assert _axial(r[s]["dir"]) <= {(1, 0, 0), (-1, 0, 0)} and len(r[s]["dir"]) == len(r[s]["pairs"]) > 0
    for name in ("degenerate_coincident", "degenerate_planar", "degenerate_collinear"):
        case, _, _ = analysed(name)
        assert {0.0, 1.0} <= set(case["inv"].ravel().tolist()), name                                    # invariants 0 and 1
