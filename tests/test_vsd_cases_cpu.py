"""The surfel renderer and VSD as the contract states them (include/stocs_hip.h at stocs_pose_errors_vsd), checked on the float32 numpy
restatement alone (tests/vsd_ref.py): the quality of the rendered surface against the analytic surface of synth:Cm, and the cases of
BOP's visibility rules.  No GPU; the GPU tests (tests/test_vsd_gpu.py) hold the library equal to this restatement bit for bit."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depth_check_ref as dref  # noqa: E402
import vsd_cases as vc  # noqa: E402
import vsd_ref as ref  # noqa: E402
from model_matching_amd import synth  # noqa: E402

F = np.float32
W, H = 640, 480
K = vc.YCB_K
DIAMETER = 0.16                                          # of Cm, about: the taus need no more
TAUS = [F(0.05 * i) * F(DIAMETER) for i in range(1, 11)]


@pytest.fixture(scope="module")
def cm():
    """Cm, its pose, its z-buffer at the ground truth and a frame that shows it in front of a wall at 1.5 m (read-only)"""
    pos, nrm = vc.cm_model()
    kn = dref.unit_normals(nrm)
    gt = vc.cm_pose()
    zG = ref.render_bits(gt, pos, kn, K, W, H)
    z = ref.bits_to_depth(zG, W, H)
    frame = vc.raw_from_depth(np.where(z > 0, z, 1.5))
    for a in (pos, kn, gt, zG, frame):
        a.setflags(write=False)
    return dict(pos=pos, nrm=nrm, kn=kn, gt=gt, zG=zG, frame=frame)


def _render(cm, pose):
    return ref.render_bits(pose, cm["pos"], cm["kn"], K, W, H)


def _moved(cm, dx, dy, dz):
    return vc.pose16(vc.translation(dx, dy, dz) @ synth.gt_pose())


def test_surface_quality_against_the_analytic_cm(cm):
    """radius 0.006, max_splat_px 16, synth.gt_pose(): the restatement gives 0 empty pixels of 35 097 in the analytic silhouette, a
    median depth error of 0.67 mm and a 99th percentile of 2.7 mm (maximum 5.3 mm, on the silhouette); profiles/vsd.md has the table"""
    A = vc.cm_analytic_depth(synth.gt_pose(), vc.cm_ellipsoid_centre(cm["pos"]), K, W, H)
    z = ref.bits_to_depth(cm["zG"], W, H)
    sil, have = A > 0, z > 0
    assert 30000 < sil.sum() < 40000
    empty = int((sil & ~have).sum())
    err = np.abs(z.astype(np.float64) - A)[sil & have]
    print("silhouette %d empty %d median %.3f mm p99 %.3f mm max %.3f mm" % (sil.sum(), empty, np.median(err) * 1e3, np.percentile(err, 99) * 1e3, err.max() * 1e3))
    assert empty <= 0.001 * sil.sum()
    assert np.median(err) <= 0.001
    assert np.percentile(err, 99) <= 0.004


def test_the_ground_truth_against_itself_scores_zero(cm):
    r, _ = ref.compare(cm["zG"], cm["zG"], cm["frame"], K, vc.DEPTH_SCALE, TAUS)
    assert r["uni"] > 0 and r["inter"] == r["uni"] == r["vis_gt"] == r["vis_est"] == r["px_gt"]
    assert np.all(r["far"] == 0) and np.all(r["e"] == 0)


def test_an_estimate_pushed_back_scores_one(cm):
    zE = _render(cm, _moved(cm, 0, 0, 0.2))
    r, _ = ref.compare(zE, cm["zG"], cm["frame"], K, vc.DEPTH_SCALE, TAUS)
    assert r["uni"] > 0 and r["inter"] > 0
    assert np.all(r["far"][:10] == r["inter"]) and np.all(r["e"][:10] == 1) and np.all(r["e"][10:] == 0)


def test_an_occluder_over_the_whole_object_leaves_nothing_visible(cm):
    wall = vc.flat_frame(W, H, 0.5)                      # dS < dG - delta everywhere on the object
    r, _ = ref.compare(cm["zG"], cm["zG"], wall, K, vc.DEPTH_SCALE, TAUS)
    assert r["px_gt"] > 0 and r["uni"] == 0 and r["vis_gt"] == 0 and r["vis_est"] == 0
    assert np.all(r["e"][:10] == 1)


def test_no_measurement_makes_everything_rendered_visible(cm):
    zE = _render(cm, _moved(cm, 0.01, 0, 0.3))
    r, m = ref.compare(zE, cm["zG"], vc.flat_frame(W, H, 0), K, vc.DEPTH_SCALE, TAUS)
    assert r["vis_est"] == r["px_est"] > 0 and r["vis_gt"] == r["px_gt"] > 0
    assert r["uni"] == int((m["pe"] | m["pg"]).sum()) and r["inter"] == int((m["pe"] & m["pg"]).sum())


def test_an_estimate_behind_the_frame_is_visible_where_the_ground_truth_is(cm):
    """the frame shows the ground truth; the estimate lies 5 cm behind it, so on its own nearly every pixel of it that the object covers
    would be hidden (dE - dS > delta): the `or visG` clause makes the estimate visible wherever it is present and the ground truth is
    visible"""
    zE = _render(cm, _moved(cm, 0.002, 0, 0.05))
    r, m = ref.compare(zE, cm["zG"], cm["frame"], K, vc.DEPTH_SCALE, TAUS)
    with np.errstate(all="ignore"):
        alone = m["pe"] & (m["dE"] - m["dS"] <= F(0.015))
    by_clause = m["pe"] & m["visG"]
    assert by_clause.sum() > 10000 and (alone & m["pg"]).sum() < 0.01 * by_clause.sum()    # on its own the estimate is hidden on the object
    assert np.array_equal(m["visE"], alone | by_clause)
    assert r["vis_est"] == int((alone | by_clause).sum()) and r["inter"] == int(by_clause.sum())
    assert int((m["visE"] & m["pg"]).sum()) == int(by_clause.sum())           # on the object: exactly where the ground truth is visible


def test_records_of_the_whole_call(cm):
    """pose_errors_vsd of the restatement: one ground truth for all, one each, and the invalid pairs"""
    bad = cm["gt"].copy(); bad[13] = np.nan
    E = np.stack([cm["gt"], _moved(cm, 0, 0, 0.2), np.zeros(16, F), bad])
    a = ref.pose_errors_vsd(E, cm["gt"], cm["pos"], cm["nrm"], cm["frame"], K, vc.DEPTH_SCALE, TAUS)
    b = ref.pose_errors_vsd(E, np.tile(cm["gt"], (4, 1)), cm["pos"], cm["nrm"], cm["frame"], K, vc.DEPTH_SCALE, TAUS)
    assert ref.records_equal(a, b)
    assert list(a["valid"]) == [1, 1, 0, 0]
    assert np.all(a["e"][0] == 0) and np.all(a["e"][1][:10] == 1)
    for i in (2, 3):                                                          # nothing rendered: the arithmetic still runs and scores 1
        assert a["px_est"][i] == 0 and a["uni"][i] == a["vis_gt"][i] > 0 and np.all(a["e"][i][:10] == 1)
    c = ref.pose_errors_vsd(cm["gt"], bad, cm["pos"], cm["nrm"], cm["frame"], K, vc.DEPTH_SCALE, TAUS)
    assert c["valid"][0] == 0 and c["px_gt"][0] == 0 and np.all(c["e"][0][:10] == 1)


def test_pose_recall_vsd_on_hand_made_records():
    from model_matching_amd.estimator import _VSD_DTYPE, pose_recall_vsd
    assert _VSD_DTYPE == ref.DTYPE
    r = np.zeros(4, ref.DTYPE)
    r["valid"] = (1, 1, 1, 0)
    r["e"][0, :10] = 0.0            # right under every threshold: 1
    r["e"][1, :10] = 1.0            # wrong under every threshold: 0
    r["e"][2, :10] = 0.26           # below 0.30 .. 0.50: 5 of 10
    r["e"][3, :10] = 0.0            # invalid: counts as wrong although e says right
    ar, nv = pose_recall_vsd(r)
    assert nv == 3 and abs(ar - (1.0 + 0.0 + 0.5 + 0.0) / 4) < 1e-12 and abs(ar - ref.pose_recall_vsd(r)) < 1e-12
    r["e"][2, :5] = 0.0             # half of its taus right everywhere, the other half as before: 0.75
    ar, _ = pose_recall_vsd(r)
    assert abs(ar - (1.0 + 0.0 + 0.75 + 0.0) / 4) < 1e-12 and abs(ar - ref.pose_recall_vsd(r)) < 1e-12
    ar2, _ = pose_recall_vsd(r, n_tau=5)                                      # only the first five taus
    assert abs(ar2 - (1.0 + 0.0 + 1.0 + 0.0) / 4) < 1e-12
    thr = np.zeros(1, ref.DTYPE); thr["valid"] = 1; thr["e"][0, :10] = F(0.05)   # e equal to a threshold is not below it
    assert abs(pose_recall_vsd(thr)[0] - 0.9) < 1e-12
    assert np.isnan(pose_recall_vsd(np.zeros(0, ref.DTYPE))[0])
