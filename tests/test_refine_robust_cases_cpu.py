"""The robust refinement's cases and restatement against themselves (tests/refine_robust_cases.py, tests/refine_robust_ref.py): the
built cases hold what they are named for, the ambiguity caps the GPU tests rely on, and the restatement against
oracle/ingest_oracle.py::icp and against the table of the issue it answers.  No GPU."""
import os
import sys

import numpy as np
import pytest

from oracle import refine_oracle as ro

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import refine_robust_cases as rc  # noqa: E402
import refine_robust_ref as rr  # noqa: E402

F = np.float32
NOT = rr.NOT_CANDIDATE
CUT_CASES = rc.cut_cases()


def _words_by_brute_force(case):
    """float32(d1) bits where the nearest model point is within the distance and the source inside the widened box, else NOT"""
    sc, mc, src = case.held()
    cl = ro.classify(src, mc)
    g = ro.predict_grid(mc, case.dist)
    cand = ro.in_box(g, src) & (cl["d1"] <= float(F(case.dist)) ** 2)
    assert (cl["ntie"][cand] == 1).all()                       # the lattice point is the only neighbour
    assert (cl["d1"].astype(F).astype(np.float64) == cl["d1"])[cand].all()   # exact in float: the word is known bit for bit
    return np.where(cand, cl["d1"].astype(F).view(np.uint32), NOT).astype(np.uint32), cl


@pytest.mark.parametrize("case", CUT_CASES + [rc.gate_exact()], ids=[c.id for c in CUT_CASES] + ["gate-axis_normals"])
def test_built_cases_have_the_words_they_claim(case):
    sc, mc, src = case.held()
    assert not ro.centre(case.scene)[1].any() and not ro.centre(case.model)[1].any()
    words, cl = _words_by_brute_force(case)
    assert np.array_equal(words, case.source_words())
    # a BEYOND point: matched by the walk's bound, no candidate
    D2 = float(F(case.dist)) ** 2
    if case.src_idx is None:
        beyond = (cl["d1"] > D2) & (cl["d1"] <= float(F(D2 * (1.0 + 1e-5))))
        assert beyond.any() and (case.words[beyond] == NOT).all()


def test_tie_groups_bytes_and_kept_counts():
    one = rc.one_level()
    w = one.words[one.words != NOT]
    assert len(w) == 120 and len(set(w.tolist())) == 1
    two = rc.two_levels()
    w = two.words[two.words != NOT]
    lv, cnt = np.unique(w, return_counts=True)
    assert cnt.tolist() == [2 * rc.NEAR_PAIRS, 2 * rc.FAR_PAIRS] and lv[0] < lv[1]
    na, nb = cnt.tolist()
    ks = rc.ks_for(two)
    assert {na, na // 2, na + nb // 2, na - 1, na + 1, na + nb}.issubset(ks)
    for byte, (a, b) in rc.BYTE_PAIRS.items():
        x = rc.word_of(a) ^ rc.word_of(b)
        assert x != 0 and (x & ~(0xFF << (8 * byte))) == 0, (byte, hex(x))
    by = rc.byte_levels()
    have = set(by.words.tolist())
    assert {rc.word_of(o) for p in rc.BYTE_PAIRS.values() for o in p}.issubset(have)
    assert rc.word_of(rc.COINCIDENT) == 0 and 0 in have
    top = rc.word_of(rc.AT_THRESHOLD)
    assert top in have and top == int(np.array([float(F(rc.D)) ** 2], F).view(np.uint32)[0]) and max(have - {NOT}) == top
    for j, c in enumerate(rc.few_candidates()):
        assert int((c.source_words() != NOT).sum()) == j
    assert [len(c.src_idx) for c in rc.source_sizes()] == list(rc.SIZES) == [1, 255, 256, 257, 1025]
    last = rc.last_chunk()
    ci = np.nonzero(last.source_words() != NOT)[0]
    assert len(last.src_idx) == 600 and ci.min() >= 512 and len(ci) == 88
    rep = rc.repeated_point()
    a, b = rep.twice
    assert rep.src_idx[a] == rep.src_idx[b] and len(set(rep.src_idx.tolist())) == len(rep.src_idx) - 1
    for case in CUT_CASES:
        n_cand = int((case.source_words() != NOT).sum())
        for k in rc.ks_for(case):
            r = rr.ratio_for_k(k, n_cand)
            assert rr.keep_count(rr.device_ratio(r), n_cand) == k and float(F(r)) == r
        if n_cand >= 6:
            assert {5, 6}.issubset(rc.ks_for(case)) or case.name in ("two_levels", "byte_levels")
    # the integer sort the GPU tests compare with: stable on equal words
    kept, k, n = rr.kept_by_sort(np.array([5, NOT, 3, 5, 3, NOT, 5], np.uint32), 0.6)
    assert (k, n) == (3, 5) and kept.tolist() == [1, 0, 1, 0, 1, 0, 0]


def test_gate_cases():
    case = rc.gate_exact()
    sc, mc, src = case.held()
    cl = ro.classify(src, mc)
    near = case.words != NOT
    c = rr.gate_c(rr.hyp_inverse(case.T16), np.eye(4)[:3, :], rr.unit_normals(case.scene_nrm), case.unit_normals()[cl["low"]])
    vals, cnt = np.unique(c[near], return_counts=True)
    assert vals.tolist() == [-1.0, 0.0, 1.0] and cnt.min() >= 10
    # the random cloud: at most 1 % of the pairs inside the band where the device may differ
    case = rc.gate_random()
    sc, mc, src = case.held()
    cl = ro.classify(src, mc)
    near = ro.in_box(ro.predict_grid(mc, case.dist), src) & (cl["d1"] <= float(F(case.dist)) ** 2)
    c = rr.gate_c(rr.hyp_inverse(case.T16), np.eye(4)[:3, :], rr.unit_normals(case.scene_nrm), case.unit_normals()[cl["low"]])
    mcos = rr.min_cos_of_degrees(30.0)
    assert abs(mcos - np.cos(np.pi / 6)) < 1e-7
    band = near & (np.abs(c - mcos) <= rr.GATE_BAND)
    assert near.sum() > 1000 and band.sum() <= 0.01 * near.sum() and 0 < (near & (c >= mcos)).sum() < 0.5 * near.sum()


def _held(name):
    from model_matching_amd import synth
    m, s, _ = synth.workload(name)
    sc, cs = ro.centre(s.pos)
    mc, cm = ro.centre(m.pos)
    Tgt = synth.centred_gt(s.T_gt, cs.astype(np.float64), cm.astype(np.float64))
    return sc, rr.unit_normals(s.nrm), mc, rr.unit_normals(m.nrm), Tgt


def test_restatement_with_everything_kept_is_the_oracle_icp_on_tiny():
    from oracle import ingest_oracle
    sc, sn, mc, mn, Tgt = _held("tiny")
    for h in rc.table_hypotheses(Tgt, 4, seed=12):
        T = np.asarray(h, F).reshape(4, 4).T.astype(np.float64)
        Ti = np.linalg.inv(T)
        src = (Ti[:3, :3] @ sc.T.astype(np.float64) + Ti[:3, 3:]).T
        U, nc = ingest_oracle.icp(src, mc, mn, 5, 0.035)
        want = T @ np.linalg.inv(U)
        got = rr.robust_loop(h, sc, sn, mc, mn, 5, 0.035, 1.0, None)
        assert got["iterations"] == 5 and got["k"] == got["n_cand"]
        # the oracle takes the source in float64, the restatement rounds it to float as the device does: 1e-5 / 2e-5 as test_refine_gpu
        assert abs(got["k"] - nc) <= 2
        assert np.abs(got["T"][:3, :3] - want[:3, :3]).max() <= 1e-5 and np.abs(got["T"][:3, 3] - want[:3, 3]).max() <= 2e-5


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_everything_kept_with_the_gate_on_is_clear_for_all_six(name):
    """keep 1 with the 30 degree gate (the accumulation's gate-on form): the restatement of the six table hypotheses is clear at every
    iteration, so tests/test_refine_robust_gpu.py may compare all six with it.  k about 180 to 185 on tiny, 506 to 513 on small."""
    sc, sn, mc, mn, Tgt = _held(name)
    mcos = rr.min_cos_of_degrees(30.0)
    for h in rc.table_hypotheses(Tgt):
        ref = rr.robust_loop(h, sc, sn, mc, mn, 5, 0.035, 1.0, mcos)
        print(name, "clear", ref["clear"], "iterations", ref["iterations"], "k", ref["k"], "n_cand", ref["n_cand"])
        assert ref["clear"] and ref["iterations"] == 5 and ref["k"] == ref["n_cand"]


@pytest.fixture(scope="module")
def small_rows():
    """ADD in mm of the six table hypotheses on `small`: before, and after 5 iterations of each form, with the clear flags of the
    device-ratio run the GPU test compares with"""
    sc, sn, mc, mn, Tgt = _held("small")
    H = rc.table_hypotheses(Tgt)
    mcos = rr.min_cos_of_degrees(30.0)
    rows = []
    for h in H:
        r = [rr.add_error(h.reshape(4, 4).T.astype(np.float64), Tgt, mc)]
        for keep, g in ((1.0, None), (0.7, None), (1.0, mcos), (0.7, mcos)):   # the table's restatement took the keep ratio as the double 0.7
            r.append(rr.add_error(rr.robust_loop(h, sc, sn, mc, mn, 5, 0.035, keep, g)["T"], Tgt, mc))
        rows.append(r)
    clear = [rr.robust_loop(h, sc, sn, mc, mn, 5, 0.035, rr.device_ratio(0.7), mcos)["clear"] for h in H]
    return np.array(rows) * 1e3, clear


def test_restatement_reproduces_the_small_row_of_the_table(small_rows):
    """before 4.03 | plain 52.2 (55.7) | keep 0.7 12.1 (26.7) | gate 3.35 (3.69) | both 0.60 (0.72): median (maximum) in mm, each to
    the digits the table prints"""
    a, _ = small_rows
    med, mx = np.median(a, 0), a.max(0)
    print("median", med, "max", mx)
    assert abs(med[0] - 4.03) <= 0.005
    for col, (m_, x_, half) in enumerate([(52.2, 55.7, 0.05), (12.1, 26.7, 0.05), (3.35, 3.69, 0.005), (0.60, 0.72, 0.005)], start=1):
        assert abs(med[col] - m_) <= half and abs(mx[col] - x_) <= half, (col, med[col], mx[col])


def test_at_least_four_of_the_six_hypotheses_are_clear(small_rows):
    """seed rc.TABLE_SEED = 5, the table's own: five of the six are clear at every iteration with the device's float keep ratio"""
    _, clear = small_rows
    print("clear", clear)
    assert sum(clear) >= 4
