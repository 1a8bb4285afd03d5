"""stocs_select_instances / stocs_select_instances_rows on the GPU against the numpy restatement of their contract
(tests/instances_ref.py) on the cases of tests/instances_cases.py: every comparison is integer equality, or bit equality on the score;
no tolerance and no excluded case."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import instances_cases as cases  # noqa: E402
import instances_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
APP = os.path.join(ROOT, "model_matching_amd", "apps", "stocs_single")
CHILD = os.path.join(ROOT, "tests", "instances_child.py")


def _same(got, want):
    (g_rec, g_sel), (w_rec, w_sel) = got, want
    assert g_rec.dtype.names == w_rec.dtype.names and g_sel.dtype == np.int32
    assert np.array_equal(g_sel, w_sel), (g_sel, w_sel)
    bad = [i for i in range(len(w_rec)) if not ref.records_equal(g_rec[i], w_rec[i])]
    assert not bad and len(g_rec) == len(w_rec), (bad[:5], g_rec[bad[:5]], w_rec[bad[:5]])


# ---- the rows entry point ----
@pytest.fixture(scope="module")
def any_est():
    """a context for its device and workspace; the rows form does not look at its scene"""
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, _ = synth.workload("tiny")
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    yield est
    est.close()


def _rows(est, case):
    return est.select_instances_rows(case["hit"], case["counted"], case["lcp"], case["nS"], **case["prm"])


@pytest.mark.parametrize("case", cases.crafted_cases(), ids=lambda c: c["name"])
def test_rows_crafted(any_est, case):
    got = _rows(any_est, case)
    _same(got, ref.select(case["hit"], case["counted"], case["lcp"], **case["prm"]))
    if "selected" in case:
        assert got[1].tolist() == case["selected"]


@pytest.mark.parametrize("seed", range(20))
def test_rows_random(any_est, seed):
    case = cases.random_rows(seed)
    _same(_rows(any_est, case), ref.select(case["hit"], case["counted"], case["lcp"], **case["prm"]))


def test_rows_limits(any_est):
    from model_matching_amd.capi import StocsError
    c = cases.ends_of_largest_scene()
    with pytest.raises(StocsError) as e:
        any_est.select_instances_rows(c["hit"], c["counted"], c["lcp"], (1 << 18) + 1, **c["prm"])
    assert e.value.code == -4
    with pytest.raises(StocsError) as e:   # a counted hit at nS: found on the host, nothing is uploaded
        any_est.select_instances_rows(c["hit"], c["counted"], c["lcp"], (1 << 18) - 1, **c["prm"])
    assert e.value.code == -1
    _same(_rows(any_est, c), ref.select(c["hit"], c["counted"], c["lcp"], **c["prm"]))   # the context still works


def test_rows_second_call_allocates_nothing(any_est):
    case = cases.random_rows(3)
    _rows(any_est, case)
    a0 = any_est.L.stocs_device_alloc_count()
    got = _rows(any_est, case)
    small = cases.count_case(17)
    _rows(any_est, small)
    assert any_est.L.stocs_device_alloc_count() == a0
    _same(got, ref.select(case["hit"], case["counted"], case["lcp"], **case["prm"]))


# ---- the poses entry point on the planted frame ----
@pytest.fixture(scope="module")
def planted(oracle_lib):
    from model_matching_amd.estimator import StocsEstimator
    fr = cases.planted_frame()
    m = fr["model"]
    est = StocsEstimator(fr["scene_pos"], fr["scene_nrm"], fr["scene_prob"], fr["scene_pixel"], m.pos, m.nrm, build_index=False)
    orc = oracle_lib.Oracle(fr["scene_pos"], fr["scene_nrm"], fr["scene_prob"], fr["scene_pixel"], m.pos, m.nrm)
    cs, cm = orc.centroids()
    assert np.array_equal(cs, est.get_scene_centroid()) and np.array_equal(cm, est.get_model_centroid())
    T = cases.planted_hypotheses(fr, cs, cm)
    yield est, orc, T
    est.close()


def _own_rows(est, T):
    rows = [est.lcp_detail(t) for t in T]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


@pytest.mark.parametrize("exact", [0, 1])
def test_poses_equal_the_reference_on_the_contexts_own_rows(planted, exact):
    est, orc, T = planted
    est.set_option("exact_ties", exact)
    try:
        got = est.select_instances(T)
        hit, counted = _own_rows(est, T)
        lcp = est.score_transforms(T)
        _same(got, ref.select(hit, counted, lcp))
        if exact:   # and on the oracle's rows; the three planted poses are the three selected
            rows = [orc.lcp_detail(t) for t in T]
            _same(got, ref.select(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), lcp))
        assert sorted(got[1].tolist()) == [0, 1, 2]
    finally:
        est.set_option("exact_ties", 0)


def test_poses_records_do_not_depend_on_the_batch(planted):
    est, orc, T = planted
    rec, sel = est.select_instances(T)
    for h in (0, 4, 9, 14, len(T) - 1):
        one, _ = est.select_instances(T[h:h + 1])
        assert int(one["own"][0]) == int(rec["own"][h]) and one["lcp"].view(np.uint32)[0] == rec["lcp"].view(np.uint32)[h]
    rev, _ = est.select_instances(T[::-1].copy())
    assert np.array_equal(rev["own"][::-1], rec["own"]) and np.array_equal(rev["lcp"][::-1].view(np.uint32), rec["lcp"].view(np.uint32))


def test_poses_invalid_hypotheses_get_zero_records(planted):
    est, orc, T = planted
    rec, sel = est.select_instances(T)
    bad_nan = T[1].copy(); bad_nan[13] = np.nan
    bad_inf = T[2].copy(); bad_inf[0] = np.inf
    T2 = np.concatenate([T[:5], bad_nan[None], np.zeros((1, 16), F), T[5:], bad_inf[None]])
    keep = [i for i in range(len(T2)) if i not in (5, 6, len(T2) - 1)]
    rec2, sel2 = est.select_instances(T2)
    for i in (5, 6, len(T2) - 1):
        assert (int(rec2["rank"][i]), int(rec2["own"][i]), int(rec2["exclusive"][i])) == (-1, 0, 0) and rec2["lcp"].view(np.uint32)[i] == 0
    assert ref.records_equal(rec2[keep], rec) and np.array_equal(np.array(keep)[sel], sel2)


def test_poses_second_call_allocates_nothing(planted):
    est, orc, T = planted
    first = est.select_instances(T)
    a0 = est.L.stocs_device_alloc_count()
    again = est.select_instances(T)
    est.select_instances(T[:7])
    assert est.L.stocs_device_alloc_count() == a0
    _same(again, first)


def test_poses_across_a_chunk_boundary_in_a_fresh_process(planted, tmp_path):
    """STOCS_INSTANCES_CHUNK=5: 23 hypotheses in chunks of 5, 5, 5, 5, 3"""
    est, orc, T = planted
    want = est.select_instances(T)
    env = dict(os.environ, STOCS_INSTANCES_CHUNK="5")
    r = subprocess.run([sys.executable, CHILD, str(tmp_path / "out.npz")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(tmp_path / "out.npz")
    assert np.array_equal(z["T"], T)
    _same((z["rec"].view(ref.DTYPE).reshape(-1), z["sel"]), want)


def test_poses_need_a_scene_argument_checks(planted):
    from model_matching_amd.capi import StocsError
    est, orc, T = planted
    rec, sel = est.select_instances(T[:0])
    assert len(rec) == 0 and len(sel) == 0
    for kw in (dict(max_instances=0), dict(min_points=0), dict(min_exclusive_fraction=0.0), dict(min_exclusive_fraction=1.5)):
        with pytest.raises(StocsError) as e:
            est.select_instances(T, **kw)
        assert e.value.code == -1


# ---- the packed example frame ----
@pytest.fixture(scope="module")
def packed():
    from model_matching_amd.estimator import StocsEstimator, trial_post
    d = np.load(os.path.join(ROOT, "tests", "golden", "example_packed_dove.npz"))
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
    est.run_trials(list(range(8)), 100, max_per_base=200, post=trial_post())
    hyps = [est.trials_get_hypotheses(t) for t in range(8)]
    P = np.concatenate([h["pose16"] for h in hyps]).astype(F).reshape(-1, 16)
    ids = [(t, i) for t, h in enumerate(hyps) for i in range(len(h))]
    T = cases.centred_from_camera(P, est.get_scene_centroid(), est.get_model_centroid())
    yield d, est, P, T, ids
    est.close()


def test_packed_fixture_equals_the_reference(packed):
    d, est, P, T, ids = packed
    assert len(T) >= 8
    got = est.select_instances(T)
    hit, counted = _own_rows(est, T)
    _same(got, ref.select(hit, counted, est.score_transforms(T)))
    print("packed/dove: %d hypotheses, %d selected: %s" % (len(T), len(got[1]), got[0][got[1]].tolist()))


# ---- the driver ----
def _strip(stdout):
    """the driver's lines without the wall clock of the batch and without the lines --instances adds"""
    keep = [l for l in stdout.splitlines() if not l.startswith("instance ") and not l.startswith("instances: ")]
    return [re.sub(r"total_microseconds=\d+", "total_microseconds=*", l) for l in keep]


def test_driver_instances_option(packed, tmp_path):
    from model_matching_amd import cloudio
    d, est, P, T, ids = packed
    cloudio.write_stcl(tmp_path / "scene.stcl", d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"])
    cloudio.write_stcl(tmp_path / "model.stcl", d["model_pos"], d["model_nrm"])
    runs = {}
    for name, extra in (("plain", []), ("inst", ["--instances", "4"])):
        out = tmp_path / name / "pose.txt"
        os.makedirs(out.parent)
        r = subprocess.run([APP, "--clouds", str(tmp_path / "scene.stcl"), str(tmp_path / "model.stcl"), "--seed", "0", "--trials", "8", "--cluster", "1",
                            "--out", str(out)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[name] = (r.stdout, out)
    # without the flag: no instance line, no instance file; with it, every other line and file is the same
    assert _strip(runs["plain"][0]) == [re.sub(r"total_microseconds=\d+", "total_microseconds=*", l) for l in runs["plain"][0].splitlines()]
    assert sorted(os.listdir(tmp_path / "plain")) == ["pose.txt"]
    assert _strip(runs["inst"][0]) == _strip(runs["plain"][0])
    assert sorted(os.listdir(tmp_path / "inst")) == ["pose.txt", "pose_instances_model.txt"]
    assert runs["inst"][1].read_bytes() == runs["plain"][1].read_bytes()
    # the selection is the Python call's on the same hypotheses
    rec, sel = est.select_instances(T, max_instances=4)
    rows = np.array((tmp_path / "inst" / "pose_instances_model.txt").read_text().split(), np.float64).astype(F).reshape(-1, 12)
    assert len(rows) == len(sel)
    assert np.array_equal(rows, P[sel].reshape(-1, 4, 4).transpose(0, 2, 1)[:, :3, :].reshape(-1, 12))
    lines = [l for l in runs["inst"][0].splitlines() if l.startswith("instance ")]
    for r, (l, h) in enumerate(zip(lines, sel)):
        w = l.split()
        assert w[1] == "%d:" % r and w[2] == "%d.%d" % ids[h] and (int(w[4]), int(w[6])) == (int(rec["own"][h]), int(rec["exclusive"][h])), l
        assert F(float(w[8])) == rec["lcp"][h], l
    assert len(lines) == len(sel) and ("instances: hypotheses=%d selected=%d" % (len(T), len(sel))) in runs["inst"][0]
