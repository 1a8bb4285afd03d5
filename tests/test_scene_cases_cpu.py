"""The restatement of the scene-selection contract (tests/scene_ref.py) checked against itself and against the inputs of the hand-built
cases (tests/scene_cases.py): the record of a pose equals render_ref.explain of that pose alone, the count identities hold, the
sequential walk equals a sixteen-per-round walk, the reasons agree with the ranks, and every hand-built pool reaches the branch it is
named for.  No GPU."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import render_ref as rref  # noqa: E402
import scene_cases as cases  # noqa: E402
import scene_ref as ref  # noqa: E402

F = np.float32


def test_row_words_and_packing():
    assert [ref.row_words(n) for n in (1, 31, 32, 33, 127, 128, 129, 1 << 19)] == [4, 4, 4, 4, 4, 4, 8, 16384]
    rng = np.random.default_rng(0)
    for npix in (1, 31, 32, 33, 129):
        m = rng.random((3, npix)) < 0.5
        m[0, npix - 1] = True
        rows = ref.pack_rows(m)
        assert rows.shape == (3, ref.row_words(npix)) and rows.dtype == np.uint32
        assert (rows[0, (npix - 1) >> 5] >> np.uint32((npix - 1) & 31)) & 1 == 1
        assert np.array_equal(ref.unpack_rows(rows, npix), m)


@pytest.mark.parametrize("claim", ["agree", "on_mask"])
def test_a_footprint_record_is_explain_of_the_pose_alone(claim):
    depth, prob = cases.rough_frame(64, 48, 3)
    pos, nrm = cases.seeded_model(257, 4)
    poses = cases.seeded_poses(9, 5, xy=0.15)
    poses[3] = np.nan; poses[6] = 0
    rec, masks, z = ref.footprints(poses, pos, nrm, depth, prob, cases.K_ROUGH, 1e-4, claim, **cases.PRM_ROUGH)
    for h in range(len(poses)):
        e, lab, st, zkey = rref.explain(poses[h], pos, nrm, depth, prob, cases.K_ROUGH, 1e-4, **cases.PRM_ROUGH)
        assert e["hidden"][0] == 0 and e["visible"][0] == e["footprint"][0]
        assert all(rec[k][h] == e[k][0] for k in ("footprint", "no_depth", "agree", "in_front", "behind", "on_mask"))
        want = (st.reshape(-1) & 15) == 2 if claim == "agree" else (st.reshape(-1) & 16) != 0
        assert np.array_equal(masks[h], want) and rec["claimed"][h] == want.sum() == (rec["agree"][h] if claim == "agree" else rec["on_mask"][h])
        assert np.array_equal(z[h] != 0xFFFFFFFF, lab.reshape(-1) == 0)
    assert np.array_equal(rec["footprint"], rec["no_depth"] + rec["agree"] + rec["in_front"] + rec["behind"])
    assert not any(rec[3].tolist()) and not any(rec[6].tolist()) and not masks[3].any() and not masks[6].any()
    assert rec["footprint"][[0, 1, 2]].all() and rec["agree"].sum() > 0 and rec["in_front"].sum() > 0 and rec["on_mask"].sum() > 0
    assert (rec["on_mask"] <= rec["agree"]).all()


def _consistent(c, rec, sel):
    """what must hold between ranks, reasons and counts whatever the pool"""
    prm = dict(ref.DEFAULTS); prm.update(c["params"])
    assert np.array_equal(rec["reason"] == 0, rec["rank"] >= 0)
    assert sorted(rec["rank"][rec["rank"] >= 0].tolist()) == list(range(len(sel))) and np.array_equal(rec["rank"][sel], np.arange(len(sel)))
    assert len(sel) <= min(prm["max_selected"], len(rec))
    assert np.array_equal(rec["own"], c["masks"].sum(axis=1)) and (rec["exclusive"] <= rec["own"]).all()
    cover = c["masks"][sel].any(axis=0) if len(sel) else np.zeros(c["masks"].shape[1], bool)
    assert np.array_equal(rec["exclusive"][rec["rank"] < 0], (c["masks"][rec["rank"] < 0] & ~cover).sum(axis=1))
    assert sum(rec["exclusive"][sel]) == cover.sum()                                       # the selected slots' exclusive pixels partition the cover
    if (rec["reason"] == 4).any():
        assert len(sel) == prm["max_selected"]
    if c["cap"] is not None:
        cnt = np.bincount(c["group"][sel], minlength=c["n_groups"])
        assert (cnt <= c["cap"]).all() and all(cnt[c["group"][h]] == c["cap"][c["group"][h]] for h in np.flatnonzero(rec["reason"] == 3))
    else:
        assert not (rec["reason"] == 3).any()
    for h in np.flatnonzero(rec["reason"] == 1):
        assert not ref.eligible(c["score"][h], int(rec["own"][h]), c["rec"][h], prm)
    keys = [ref.pack_best(c["score"][h], h) for h in sel]
    assert keys == sorted(keys, reverse=True)                                              # ranks follow the order


def test_the_sequential_walk_equals_sixteen_per_round_on_300_seeded_pools():
    reasons = set()
    for seed in range(300):
        c = cases.random_pool(seed)
        rec, sel = cases.run_ref(c)
        for k in (16, 3):
            rec_k, sel_k = cases.run_ref(c, per_round=k)
            assert ref.records_equal(rec, rec_k) and np.array_equal(sel, sel_k), (seed, k)
        _consistent(c, rec, sel)
        reasons |= set(rec["reason"].tolist())
    assert reasons == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("seed", range(3))
def test_the_two_references_agree_on_the_walk_pairs(seed):
    """the inputs of the GPU test that feeds both entry points of the shared walk: if the references disagreed, the inputs would be wrong"""
    import instances_ref
    rows, c = cases.walk_pair(seed)
    (i_rec, i_sel), (s_rec, s_sel) = instances_ref.select(rows["hit"], rows["counted"], rows["lcp"], **rows["prm"]), cases.run_ref(c)
    assert all(np.array_equal(i_rec[f], s_rec[f]) for f in ("rank", "own", "exclusive")) and np.array_equal(i_sel, s_sel)
    assert len(i_sel) >= 2 and (i_rec["rank"] < 0).any()   # something is selected and something is not


@pytest.mark.parametrize("name", sorted(cases.hand_pools()))
def test_hand_built_pools_reach_their_branch(name):
    c = cases.hand_pools()[name]
    rec, sel = cases.run_ref(c)
    rec16, sel16 = cases.run_ref(c, per_round=16)
    assert ref.records_equal(rec, rec16) and np.array_equal(sel, sel16)
    _consistent(c, rec, sel)
    if name in cases.EXPECT:
        ranks, reasons = cases.EXPECT[name]
        assert rec["rank"].tolist() == ranks and rec["reason"].tolist() == reasons, (rec["rank"].tolist(), rec["reason"].tolist())


def test_the_named_branches_follow_from_the_inputs():
    P = cases.hand_pools()
    # mid_round: slot 6 would pass against the empty cover it is first tested against, and fails only because slot 5, in the same round, went first
    c = P["mid_round"]
    prm = dict(ref.DEFAULTS); prm.update(c["params"])
    assert ref.passes(int(c["masks"][6].sum()), int(c["masks"][6].sum()), prm) and np.array_equal(c["masks"][5], c["masks"][6])
    assert 0 < 5 < 16 and len(c["score"]) > 16 and list(ref.order_of(c["score"])) == list(range(len(c["score"])))
    # round_boundary: the first selection is the sixteenth of round 0, the second the first of round 1
    c = P["round_boundary"]
    rec, sel = cases.run_ref(c, per_round=16)
    assert sel.tolist()[:2] == [15, 16] and (c["masks"][:15].sum(axis=1) < c["params"]["min_pixels"]).all()
    # max_selected_mid_round: the limit falls on the third slot of a round of sixteen that would all pass
    c = P["max_selected_mid_round"]
    assert c["params"]["max_selected"] == 3 and not (c["masks"].sum(axis=0) > 1).any()
    # the thresholds, from the numbers alone
    assert ref.passes(5, 10, dict(min_pixels=5, min_exclusive_fraction=0.1)) and not ref.passes(4, 10, dict(min_pixels=5, min_exclusive_fraction=0.1))
    assert ref.passes(4, 8, dict(min_pixels=1, min_exclusive_fraction=0.5)) and not ref.passes(3, 8, dict(min_pixels=1, min_exclusive_fraction=0.5))
    r = cases.records_for(np.ones((2, 4), bool), in_front=[1, 2], footprint=[4, 7])
    q = dict(min_pixels=1, max_violation_fraction=0.25)
    assert ref.eligible(0.5, 4, r[0], q) and not ref.eligible(0.5, 4, r[1], q)
    # equal scores: the lower slot packs to the larger key
    assert ref.pack_best(0.5, 0) > ref.pack_best(0.5, 1) > 0 == ref.pack_best(0.0, 3) == ref.pack_best(float("nan"), 3) == ref.pack_best(-1.0, 3)
    assert ref.order_of(np.array([0.0, np.nan, 0.5, -1.0, 0.5], F)) == [2, 4, 0, 1, 3]


def test_the_scene_of_two():
    """the end-to-end scene of the GPU test, in the restatement: the true poses win, the duplicates lose their pixels to them, the box laid in
    front of the disc violates free space, the box laid on the disc's surface finds it taken"""
    s = cases.scene_of_two()
    foot, masks = [], []
    for (pos, nrm), prob, poses in zip(s["models"], s["probs"], s["pools"]):
        r, m, _ = ref.footprints(poses, pos, nrm, s["depth"], prob, s["K"], s["scale"], **s["prm"])
        foot.append(r); masks.append(m)
    foot, masks = np.concatenate(foot), np.concatenate(masks)
    score = ref.default_score(foot)
    group = np.array([0, 0, 0, 0, 1, 1], np.int32)
    rec, sel = ref.select(masks, score, group, foot, 2, None, min_pixels=20)
    assert score[0] == 1.0 and score[5] == 1.0 and score[1] < 1.0 and score[4] < 1.0 and 0 < score[3] < 1.0 and score[2] == 0.0
    assert sorted(sel.tolist()) == [0, 5] and rec["reason"].tolist() == [0, 2, 1, 2, 2, 0]
    assert foot["in_front"][2] > 0.2 * foot["footprint"][2] and foot["in_front"][[0, 1, 3, 4, 5]].sum() == 0
