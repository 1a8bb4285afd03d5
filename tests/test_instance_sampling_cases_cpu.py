"""The cases of tests/instance_sampling_cases.py checked with the CPU oracle alone: every condition the GPU tests of
tests/test_instance_sampling_edges_gpu.py rely on, so that a case cannot go vacuous unnoticed.  These are conditions on the inputs, not on
the code under test.  No GPU."""
import numpy as np
import pytest

import instance_sampling_cases as ic

_REF = {}


def _ref(oracle_lib, case):
    """one oracle run per (scene, map, dispersion, attempts): the working-set form and the cut into calls do not reach the oracle"""
    k = ic.reference_key(case)
    if k not in _REF:
        _REF[k] = ic.run_oracle(oracle_lib, case, with_lcp=False)
    return _REF[k]


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    _REF.clear()


def test_the_table_holds_what_the_issue_lists():
    cases = ic.cases()
    have = {(c[1], c[2], c[4], c[5], c[6]) for c in cases}
    no_lds = (ic.NO_LDS,)
    for S in ic.SIZES:
        n = 254 if S <= 65 else 60
        assert (S, "box_and_lines", 0.9, ((0, n),), ()) in have and (S, "dense_speckle", 0.9, ((0, n),), ()) in have
        assert ((S, "dense_speckle", 0.9, ((0, n),), no_lds) in have) == (S <= 16000)
    for kind in ic.EDGE_MAPS:
        for S in (4097, 16000, 16001):
            assert (S, kind, 0.9, ((0, 60),), ()) in have
        assert (4097, kind, 0.9, ((0, 60),), no_lds) in have
    for S in (4097, 16001):
        for d in (0.0, 1.0):
            assert (S, "box_and_lines", d, ((0, 60),), ()) in have
    for env in ((), no_lds):
        assert (4097, "box_and_lines", 0.9, ((0, 254),), env) in have and (4097, "box_and_lines", 0.9, ((0, 100), (100, 154)), env) in have
    assert (4097, "dense_speckle", 0.9, ((0, 60),), (ic.TIMING,)) in have
    for c in cases:
        assert c[3] == ic.image_size(c[2]) and ic.n_attempts(c) <= 254
        assert not c[2].startswith("rows64") or c[1] >= 4097       # (at 65 points the oracle finds no base under these maps)
    assert {ic.working_set_form(c) for c in cases} == {"instance_lds", "instance_device_memory"}


@pytest.mark.parametrize("case", ic.cases(), ids=[c[0] for c in ic.cases()])
def test_every_case_gives_the_gpu_test_something_to_compare(oracle_lib, case):
    name, S, kind, (H, W), disp, calls, env = case
    sc = ic.scene(S)
    edge, pix = ic.case_input(S, kind)
    assert len(sc.pos) == S and pix.shape == (S, 2) and edge.shape == (H, W) and edge.dtype == np.uint8
    r = _ref(oracle_lib, case)
    n_valid, changed = int(r["valid"].sum()), int((r["prob"] != r["prob0"]).sum())
    print("%s: valid=%d of %d, largest segment=%d, points decayed=%d, failed first draws=%d"
          % (name, n_valid, len(r["valid"]), r["seg_sizes"].max(), changed, len(r["failed_first"])))
    assert n_valid >= 3, (name, n_valid)
    assert r["seg_sizes"].max() > 0
    if disp == 1.0:
        assert changed == 0
    else:
        assert changed > 0 and (r["prob"] <= r["prob0"]).all()
    prior_on = sc.prob > 0
    if kind.startswith("rows64"):
        assert ic.count_runs(edge) == (ic.INST_MAX_NODES if kind == "rows64_16384" else ic.INST_MAX_NODES + 1)
        assert ic.count_runs(edge[:-1]) == 63 * 256                # the whole image is needed for the count: a disc of radius >= 63
    if kind == "top_left":
        assert (pix[prior_on, 0] == 0).any() and (pix[prior_on, 1] == 0).any()
        assert (edge[pix[prior_on & (pix[:, 0] == 0), 0], pix[prior_on & (pix[:, 0] == 0), 1]] != 0).any()   # and is not pruned there
    if kind == "bottom_right":
        assert (pix[prior_on, 0] == H - 1).any() and (pix[prior_on, 1] == W - 1).any()
        assert (edge[pix[prior_on & (pix[:, 0] == H - 1), 0], pix[prior_on & (pix[:, 0] == H - 1), 1]] != 0).any()
    if kind == "lattice8":
        _, inverse, counts = np.unique(pix, axis=0, return_inverse=True, return_counts=True)
        assert (counts[inverse.ravel()] > 1).sum() * 2 >= S and not (pix % 8).any()
    if kind == "dense_speckle":                                    # any 110 rows hold more runs than the LDS parents take
        per_row = np.array([ic.count_runs(edge[r:r + 1]) for r in range(H)])
        assert np.convolve(per_row, np.ones(110, int), "valid").min() > ic.INST_MAX_NODES and 70000 < per_row.sum() < 85000
    if S >= 1025 and kind in ("box_and_lines", "dense_speckle"):   # these scenes already hold several points per pixel
        assert len(np.unique(sc.pixel, axis=0)) < S


def test_dispersion_zero_starves_the_first_draw_in_both_forms(oracle_lib):
    """the dispersion 0 cases are where the first draw of an attempt finds every weight zero: one with the working set in LDS, one in device memory"""
    for name in ("4097-box_and_lines-disp0", "16001-box_and_lines-disp0"):
        r = _ref(oracle_lib, ic.case_by_id(name))
        assert len(r["failed_first"]) >= 1 and not r["valid"][r["failed_first"]].any()
    assert ic.working_set_form(ic.case_by_id("4097-box_and_lines-disp0")) == "instance_lds"
    assert ic.working_set_form(ic.case_by_id("16001-box_and_lines-disp0")) == "instance_device_memory"


def test_a_restarted_oracle_equals_a_fresh_one(oracle_lib):
    """the two-launch batch of the GPU test runs its trials on one oracle, restarted between them (Oracle.restart_trial)"""
    S, kind, n = ic.MANY_S, "box_and_lines", ic.MANY_ATTEMPTS
    orc = ic.make_oracle(oracle_lib, S, kind)
    first = [ic.oracle_trial(oracle_lib, orc, S, kind, seed, n, 0.9, with_lcp=False) for seed in (9100, 9113) if orc.restart_trial() is None]
    for seed, got in zip((9100, 9113), first):
        want = ic.oracle_trial(oracle_lib, ic.make_oracle(oracle_lib, S, kind), S, kind, seed, n, 0.9, with_lcp=False)
        for k in ("valid", "ids", "inv", "seg_sizes", "segment", "prob"):
            assert np.array_equal(got[k], want[k]), (seed, k)
        assert got["valid"].sum() >= 3 and (got["prob"] != got["prob0"]).any()
    assert not np.array_equal(first[0]["ids"], first[1]["ids"])


def test_the_form_rule_at_its_threshold():
    f = ic.expected_form
    assert f(16000) == dict(kernel="instance_lds", threads=1024, lds_bytes=161568, cap=0, launches=1, redone=0)
    assert f(16001) == dict(kernel="instance_device_memory", threads=1024, lds_bytes=65552, cap=0, launches=1, redone=0)
    assert f(63)["lds_bytes"] == 65552 + 256 + 126 + 16 and f(4097, (ic.NO_LDS,))["kernel"] == "instance_device_memory"
    assert f(16000)["lds_bytes"] <= 160 * 1024 - 2048               # MAX_DYNAMIC_LDS of sample.hip
    assert [f(1025, n_trials=t, n_cu=256)["launches"] for t in (1, 128, 129, 256, 257)] == [1, 1, 2, 2, 3]
    assert f(1025, n_trials=3, n_cu=1)["launches"] == 3


def test_the_paths_of_the_attempt_records():
    assert ic.path_of((0, -1, 0, 0)) == "failed_first_draw" and ic.path_of((5, 7, 1, -1)) == "reused_mask"
    assert ic.path_of((5, 7, 1, 16384)) == "fill_parents_lds" and ic.path_of((0, 7, 1, 16385)) == "fill_parents_device_memory"
    assert ic.path_of((0, 7, 1, 0)) == "fill_parents_lds"           # a disc whose rows hold no passable pixel
    assert ic.path_counts([(0, -1, 0, 0), (5, 7, 1, -1), (5, 7, 1, -1)]) == dict(fill_parents_lds=0, fill_parents_device_memory=0, reused_mask=2, failed_first_draw=1)
