"""The instance-selection reference (tests/instances_ref.py) and the shared cases (tests/instances_cases.py) checked against themselves
and against the CPU oracle: no GPU.  What the GPU tests then compare the library with is known to say what the contract says."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import instances_cases as cases  # noqa: E402
import instances_ref as ref  # noqa: E402

F = np.float32


def _run(case, **kw):
    return ref.select(case["hit"], case["counted"], case["lcp"], **case["prm"], **kw)


@pytest.mark.parametrize("case", cases.crafted_cases(), ids=lambda c: c["name"])
def test_crafted_cases_end_as_they_were_built_to(case):
    rec, sel = _run(case)
    n = len(case["lcp"])
    assert len(rec) == n and sel.dtype == np.int32
    assert [int(rec["rank"][h]) for h in sel] == list(range(len(sel)))
    assert sorted(np.flatnonzero(rec["rank"] >= 0).tolist()) == sorted(sel.tolist())
    if "selected" in case:
        assert sel.tolist() == case["selected"]
    if case["name"] == "one scene point":
        assert rec["own"].tolist() == [1, 1]
    if case["name"] == "identical":
        assert (int(rec["rank"][1]), int(rec["exclusive"][1])) == (-1, 0)
    if case["name"].startswith("max_instances"):
        m = case["prm"]["max_instances"]
        assert rec["exclusive"][m:5].tolist() == [10] * (5 - m)          # disjoint from everything selected
        assert int(rec["exclusive"][5]) == 5 and int(rec["rank"][5]) == -1   # half of it lies under hypothesis 0
    if case["name"] == "uncounted hits":
        assert rec["own"].tolist() == [10, 10, 0]


def test_pack_best_is_the_librarys_key():
    assert ref.pack_best(0.0, 3) == 0 and ref.pack_best(-1.0, 3) == 0 and ref.pack_best(float("nan"), 3) == 0
    assert ref.pack_best(0.5, 0) == (0x3F000000 << 32) | 0xFFFFFFFF
    assert ref.pack_best(0.5, 7) < ref.pack_best(0.5, 6) < ref.pack_best(0.75, 9)


def test_order_rule_on_equal_scores():
    lcp = np.array([0.25, 0.5, 0.25, 0.0, 0.5, -1.0, 0.0], F)
    assert ref.order_of(lcp) == [1, 4, 0, 2, 3, 5, 6]   # not positive: all key 0, in index order
    c = cases.equal_scores()
    rec, sel = _run(c)
    assert sel.tolist() == [0, 2] and rec["rank"].tolist() == [0, -1, 1, -1]
    # the same rows with the duplicate in front: the lower index still goes first
    rec2, sel2 = ref.select(c["hit"][[1, 0, 2, 3]], c["counted"][[1, 0, 2, 3]], c["lcp"], **c["prm"])
    assert sel2.tolist() == [0, 2]


@pytest.mark.parametrize("seed", range(20))
def test_walk_is_monotone_on_random_rows(seed):
    """testing pending hypotheses early, against a cover that is a subset of their final one, and dropping those that fail changes
    no record: what lets the kernel test sixteen per round"""
    case = cases.random_rows(seed)
    rec, sel = _run(case)
    for k in range(3):
        rec2, sel2 = _run(case, early=np.random.default_rng(100 * seed + k))
        assert ref.records_equal(rec, rec2) and np.array_equal(sel, sel2)
    if seed == 0:   # the cases exercise the walk: some selected, some rejected for overlap, some for size
        assert 0 < len(sel) and (rec["own"] == 0).any() and ((rec["rank"] < 0) & (rec["own"] >= case["prm"]["min_points"])).any()


def test_monotone_on_crafted_cases():
    for case in cases.crafted_cases():
        rec, sel = _run(case)
        rec2, sel2 = _run(case, early=np.random.default_rng(5))
        assert ref.records_equal(rec, rec2) and np.array_equal(sel, sel2), case["name"]


def test_thresholds_are_exact():
    assert ref.passes(4, 8, 1, 0.5) and not ref.passes(3, 8, 1, 0.5)
    assert ref.passes(6, 8, 6, 0.125) and not ref.passes(5, 8, 6, 0.125)
    # one float32 multiply: 0.3f * 10 rounds to 3 in float32, so 3 of 10 passes at 0.3f; the product in double is above 3 and would fail it
    assert np.float32(0.3) * np.float32(10) == np.float32(3) and float(np.float32(0.3)) * 10 > 3 and ref.passes(3, 10, 1, float(np.float32(0.3)))


@pytest.fixture(scope="module")
def planted(oracle_lib):
    fr = cases.planted_frame()
    m = fr["model"]
    orc = oracle_lib.Oracle(fr["scene_pos"], fr["scene_nrm"], fr["scene_prob"], fr["scene_pixel"], m.pos, m.nrm)
    cs, cm = orc.centroids()
    T = cases.planted_hypotheses(fr, cs, cm)
    rows = [orc.lcp_detail(t) for t in T]
    hit = np.stack([r[0] for r in rows]); counted = np.stack([r[1] for r in rows])
    lcp = np.array([orc.lcp(t) for t in T], F)
    return fr, orc, T, hit, counted, lcp


def test_planted_frame_selects_the_planted_instances_by_the_oracle_alone(planted):
    fr, orc, T, hit, counted, lcp = planted
    assert 2800 <= len(fr["scene_pos"]) <= 3200 and len(T) == cases.N_PLANTED * (1 + cases.N_PERTURBED) + cases.N_RANDOM
    rec, sel = ref.select(hit, counted, lcp)
    assert sorted(sel.tolist()) == [0, 1, 2], (sel, rec)
    assert (rec["own"][:3] >= 100).all() and (rec["exclusive"][:3] == rec["own"][:3]).all()   # the copies stand apart
    dup = rec[3:3 + cases.N_PLANTED * cases.N_PERTURBED]
    assert (dup["rank"] == -1).all() and (dup["own"] >= 40).all()          # found, and rejected as found twice
    assert (dup["exclusive"].astype(np.float64) < 0.5 * dup["own"]).all()
    assert (rec["rank"][-cases.N_RANDOM:] == -1).all()


def test_planted_frame_has_no_near_ties(planted):
    """no two scene points equidistant from a transformed model point within 1e-7 relative (float64 brute force): the library's and the
    oracle's nearest-neighbour answers cannot differ by a tie rule on this frame"""
    fr, orc, T, hit, counted, lcp = planted
    S = np.asarray(orc.scene_centred(), np.float64).reshape(-1, 3)
    M = np.asarray(orc.model_centred(), np.float64).reshape(-1, 3)
    eps = 0.005
    worst = np.inf
    for t in T:
        A = t.astype(np.float64).reshape(4, 4).T
        q = M @ A[:3, :3].T + A[:3, 3]
        d = np.sqrt(((q[:, None, :] - S[None, :, :]) ** 2).sum(-1))
        two = np.partition(d, 1, axis=1)[:, :2]
        near = two[:, 0] <= 2 * eps
        if near.any():
            worst = min(worst, float(((two[near, 1] - two[near, 0]) / two[near, 1]).min()))
    assert worst > 1e-7, worst
