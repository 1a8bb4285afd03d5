"""The robust refinement behind the tracker (stocs_track_poses_robust): the rounds are stocs_track_poses's, the refined fields are
stocs_refine_poses_robust of the final incumbents, a prior is independent of the others, keep 1 with the gate off is the plain call;
on a cluttered frame the robust form improves the incumbent where the plain form pulls it off the object; groups change no byte;
a repeated call allocates nothing; the argument checks; the facade's overloads (tests/cpp/refine_paths_robust_facade_check.cpp)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import refine_robust_cases as rc  # noqa: E402
from test_track_gpu import PARITY, _perturbed, _workload  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBUST = dict(keep_ratio=0.7, max_normal_deg=30.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(np.asarray(a[f]).view(np.uint32), np.asarray(b[f]).view(np.uint32)) for f in a.dtype.names)


@pytest.mark.parametrize("name", ["tiny", "Cm", "ycb"])
def test_parity_by_composition(name):
    est, P0 = _workload(name)
    priors = _perturbed(P0, 8, seed=5, max_t=0.01, max_deg=6.0)
    prm = PARITY
    rounds = prm["rounds"]
    plain = est.track_poses(priors, keep_details=True, **prm)
    plain_rounds = [[est.track_round(p, r) for r in range(rounds)] for p in range(8)]
    res = est.track_poses(priors, keep_details=True, **prm, **ROBUST)
    # the rounds: candidates, scores, incumbents, as without the setting
    finals = []
    for p in range(8):
        for r in range(rounds):
            T, l = est.track_round(p, r)
            assert np.array_equal(_bits(T), _bits(plain_rounds[p][r][0])) and np.array_equal(_bits(l), _bits(plain_rounds[p][r][1])), (name, p, r)
        finals.append(T[int(np.flatnonzero(l == l.max())[0])])      # the last round's first maximum: the final incumbent
    for f in ("prior_lcp", "lcp", "pose16"):
        assert np.array_equal(np.asarray(res[f]).view(np.uint32), np.asarray(plain[f]).view(np.uint32)), (name, f)
    # the refined fields: stocs_refine_poses_robust of the final incumbents
    finals = np.stack(finals)
    To, Po, lr, nc, ncand, it = est.refine_poses_robust(finals, prm["refine_iterations"], prm["max_correspondence_distance"], **ROBUST)
    assert np.array_equal(_bits(res["refined_pose16"]), _bits(Po))
    assert np.array_equal(_bits(res["refined_lcp"]), _bits(lr))
    assert np.array_equal(res["n_correspondences"], nc) and np.array_equal(res["iterations"], it)
    assert (it > 0).any() and (nc < plain["n_correspondences"]).any()
    # a prior's results do not depend on the other priors of the call
    one = est.track_poses(priors[:1], keep_details=True, **prm, **ROBUST)
    assert _same(one[:1], res[:1])
    for r in range(rounds):
        T1, l1 = est.track_round(0, r)
        assert np.array_equal(_bits(T1), _bits(plain_rounds[0][r][0])) and np.array_equal(_bits(l1), _bits(plain_rounds[0][r][1]))
    # everything kept, the gate off: the plain call, byte for byte
    kept = est.track_poses(priors, keep_details=True, **prm, keep_ratio=1.0, max_normal_deg=None)
    assert kept.tobytes() == plain.tobytes()


def test_the_robust_form_improves_the_incumbent_where_the_plain_form_does_not():
    """small (5 000 x 1 000), the six hypotheses of DESIGN.md 7.11's table as priors, one round of one sample (the incumbent is the
    prior), 5 iterations at 3.5 cm.  For every prior ADD(robust refined) < ADD(incumbent) < ADD(plain refined); only the ordering is
    asserted (tests/test_refine_robust_cases_cpu.py reproduces the row on the CPU: before 4.03 mm, plain 52.2 mm, robust 0.60 mm)."""
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, _ = synth.workload("small")
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    Tgt = synth.centred_gt(s.T_gt, est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64))
    priors = est.refine_poses_robust(rc.table_hypotheses(Tgt), 0)[1]          # the six hypotheses in the camera frame
    assert len(priors) == 6
    kw = dict(rounds=1, samples=1, refine_iterations=5, max_correspondence_distance=0.035)
    plain = est.track_poses(priors, **kw)
    robust = est.track_poses(priors, **kw, **ROBUST)
    assert np.array_equal(_bits(plain["pose16"]), _bits(robust["pose16"]))
    gt = np.asarray(s.T_gt, np.float64).T.reshape(16).astype(np.float32)
    inc, rob, pla = (est.pose_errors(P, gt)["add"].astype(np.float64) for P in (robust["pose16"], robust["refined_pose16"], plain["refined_pose16"]))
    print("ADD mm incumbent %s robust %s plain %s" % (np.round(inc * 1e3, 3), np.round(rob * 1e3, 3), np.round(pla * 1e3, 3)))
    print("ADD mm means: incumbent %.3f robust %.3f (max %.3f) plain %.3f (max %.3f)" % (inc.mean() * 1e3, rob.mean() * 1e3, rob.max() * 1e3, pla.mean() * 1e3,
                                                                                     pla.max() * 1e3))
    assert (rob < inc).all() and (inc < pla).all()
    est.close()


def test_groups_give_the_same_records(monkeypatch):
    est, P0 = _workload("tiny")
    priors = _perturbed(P0, 8, seed=5, max_t=0.01, max_deg=6.0)
    whole = est.track_poses(priors, **PARITY, **ROBUST)
    assert (whole["iterations"] > 0).any()
    for demand in (est.nS * 8, 3 * est.nS * 8):                    # groups of one prior; of three, the last one partial
        monkeypatch.setenv("STOCS_REFINE_ROBUST_GROUP_BYTES", str(demand))
        grouped = est.track_poses(priors, **PARITY, **ROBUST)
        monkeypatch.delenv("STOCS_REFINE_ROBUST_GROUP_BYTES")
        assert grouped.tobytes() == whole.tobytes(), demand


def test_repeated_call_allocates_nothing():
    from model_matching_amd import capi
    est, P0 = _workload("tiny")
    L = capi.load()
    priors = _perturbed(P0, 8, seed=3, max_t=0.01, max_deg=5.0)
    kw = dict(refine_iterations=5, keep_details=True, **ROBUST)
    first = est.track_poses(priors, **kw)
    ws, n0 = est.refine_robust_workspace(), L.stocs_device_alloc_count()
    assert ws[0] != 0 and ws[1] >= 8 * est.nS * 8
    again = est.track_poses(priors, **kw)
    assert est.refine_robust_workspace() == ws and L.stocs_device_alloc_count() == n0
    assert again.tobytes() == first.tobytes()


def test_errors():
    from model_matching_amd import capi, synth
    from model_matching_amd.estimator import StocsEstimator
    L = capi.load()
    m, s, _ = synth.workload("tiny")
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    good = s.T_gt.T.reshape(1, 16).astype(np.float32)
    out = (capi.TrackResult * 8)()

    def prm(**kw):
        d = dict(rounds=2, samples=8, max_translation=0.01, max_rotation_deg=5.0, shrink=0.5, seed=1, refine_iterations=3,
                 max_correspondence_distance=0.035, keep_details=0)
        d.update(kw)
        return capi.TrackParams(*[d[f] for f, _ in capi.TrackParams._fields_])

    def call(P=good, n=None, h=est.h, keep=0.7, mc=0.5, **kw):
        p = prm(**kw)
        return L.stocs_track_poses_robust(h, None if P is None else P.ctypes.data_as(capi._fp), len(P) if n is None else n, C.byref(p), keep, mc, out)

    assert call() == 0
    for keep, mc in ((1.0, 0.5), (0.7, 1.0), (0.7, -1.0), (0.7, -2.0), (0.7, float("-inf")), (1e-6, 0.5)):
        assert call(keep=keep, mc=mc) == 0, (keep, mc)
    nan, inf = float("nan"), float("inf")
    # tests/test_refine_robust_gpu.py's list of invalid settings
    for keep, mc in ((0.0, 0.5), (-0.1, 0.5), (1.0000001, 0.5), (nan, 0.5), (inf, 0.5), (0.7, 1.0000001), (0.7, nan), (0.7, inf)):
        assert call(keep=keep, mc=mc) == capi.ERR_INVALID, (keep, mc)
        assert len(L.stocs_last_error()) > 0
    # the plain entry point's own errors, unchanged
    assert call(P=None, n=0) == 0
    bad = good.copy(); bad[0, 13] = np.nan
    assert call(P=bad) == capi.ERR_INVALID and b"prior 0" in L.stocs_last_error()
    for kw in (dict(h=None), dict(n=-1), dict(P=None, n=1), dict(rounds=0), dict(rounds=65), dict(samples=0), dict(max_translation=0.0), dict(max_rotation_deg=180.0),
               dict(shrink=1.5), dict(refine_iterations=-1), dict(max_correspondence_distance=0.0), dict(max_correspondence_distance=nan),
               dict(samples=(1 << 20) + 1)):
        assert call(**kw) == capi.ERR_INVALID, kw
    est.close()


def test_the_facades_overloads(tmp_path):
    from model_matching_amd import cloudio, synth
    from model_matching_amd.estimator import StocsEstimator, trial_post
    m, s, _ = synth.workload("tiny")
    cloudio.write_stcl(tmp_path / "scene.stcl", s.pos, s.nrm, s.prob, s.pixel)
    cloudio.write_stcl(tmp_path / "model.stcl", m.pos, m.nrm)
    prior = np.asarray(s.T_gt, np.float64)[:3, :]
    (tmp_path / "prior.txt").write_text(" ".join("%.9g" % x for x in prior.ravel()) + "\n")
    exe = tmp_path / "refine_paths_robust_facade_check"
    lib = os.path.join(ROOT, "model_matching_amd")
    r = subprocess.run(["g++", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "refine_paths_robust_facade_check.cpp"), "-O2", "-std=c++11", "-pthread", "-Wall",
                        "-Werror", "-I", os.path.join(ROOT, "include"), "-L", lib, "-lstocs_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(tmp_path / "scene.stcl"), str(tmp_path / "model.stcl"), str(tmp_path / "prior.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # the library's own results for the same batch and the same prior
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    est.run_trials([5, 6, 7, 8], 100, max_per_base=200, post=trial_post(refine_iterations=5), robust=ROBUST)
    want = []
    for t in range(4):
        for k, h in enumerate(est.trials_get_hypotheses(t)):
            want.append(("batch", t, k, int(h["base_index"]), np.concatenate([[h["refined_lcp"]], h["refined_pose16"]]).astype(np.float32)))
    P16 = np.eye(4, dtype=np.float32)
    P16[:3, :] = np.array((tmp_path / "prior.txt").read_text().split(), np.float64).astype(np.float32).reshape(3, 4)
    tr = est.track_poses(P16.T.reshape(1, 16), rounds=2, samples=64, refine_iterations=5, **ROBUST)[0]
    est.close()
    got = [ln.split() for ln in r.stdout.splitlines()]
    batch = [g for g in got if g[0] == "batch"]
    assert len(batch) == len(want) > 0
    for g, w in zip(batch, want):
        assert (int(g[1]), int(g[2]), int(g[3])) == w[1:4]
        assert np.array_equal(np.array(g[4:], np.float64).astype(np.float32), w[4]), g[:3]
    track = [g for g in got if g[0] == "track"]
    assert len(track) == 1
    g = track[0]
    assert np.array_equal(np.array(g[2:4], np.float64).astype(np.float32), np.array([tr["lcp"], tr["refined_lcp"]], np.float32))
    assert (int(g[4]), int(g[5])) == (int(tr["n_correspondences"]), int(tr["iterations"]))
    assert np.array_equal(np.array(g[6:], np.float64).astype(np.float32), tr["refined_pose16"])
