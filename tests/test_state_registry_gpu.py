"""The per-feature state of a context (csrc/stocs_ctx.h, StateOwner): every owner makes its state at its first call and
stocs_ctx_destroy deletes whatever subset was made, in whatever order it was made.  One smallest call of each of the thirteen owners on
the tiny workload with a 64 x 48 frame and a two-triangle mesh, then close(); every other owner in reverse order on a second context;
a third context closed untouched."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vsd_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 64, 48
K = (64.0, 32.0, 64.0, 24.0)                      # fx, cx, fy, cy
IDENTITY = np.eye(4, dtype=F).reshape(16)
VERTS = np.array([[-0.2, -0.2, 1.0], [0.2, -0.2, 1.0], [0.2, 0.2, 1.0], [-0.2, 0.2, 1.0]], F)
TRIS = np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def _owners(est, gt):
    """name -> a call that makes that owner's state and returns how many records came back (1 expected of each)"""
    from model_matching_amd.estimator import scene_row_words

    def frame():
        est.set_frame(vc.flat_frame(W, H, 1.0), None, K, vc.DEPTH_SCALE)

    def mesh():
        est.set_mesh(VERTS, TRIS)

    def depth():
        frame()
        return len(est.depth_check_poses(gt))

    def scene():
        frame()
        rows = est.dev_alloc(scene_row_words((H, W)) * 4)
        try:
            return len(est.scene_footprints(gt, rows, 0, 1))
        finally:
            est.dev_free(rows)

    def explain():
        frame()
        return len(est.explain_poses(gt))

    def vsd():
        frame()
        return len(est.pose_errors_vsd(gt, gt, taus=[0.02]))

    def vsd_mesh():
        frame(); mesh()
        return len(est.pose_errors_vsd_mesh(gt, gt, taus=[0.02]))

    def explain_mesh():
        frame(); mesh()
        return len(est.explain_poses_mesh(gt))

    def refine_visible():
        frame(); mesh()
        poses, rec = est.refine_poses_visible(gt)
        assert poses.shape == (1, 16)
        return len(rec)

    return [
        ("refine", lambda: len(est.refine_poses(IDENTITY, max_iterations=1)[2])),
        ("track", lambda: len(est.track_poses(gt, rounds=1, samples=2, refine_iterations=0))),
        ("depth", depth),
        ("instances", lambda: len(est.select_instances(IDENTITY)[0])),
        ("render", explain),
        ("scene", scene),
        ("pose_error", lambda: len(est.pose_errors(gt, gt))),
        ("pose_error_sym", lambda: len(est.pose_errors_sym(gt, gt, IDENTITY))),
        ("symmetry", lambda: len(est.symmetry_errors(IDENTITY, 0.01))),
        ("vsd", vsd),
        ("mesh", vsd_mesh),
        ("render_mesh", explain_mesh),
        ("refine_visible", refine_visible),
    ]


def test_destroy_with_any_subset_of_features_made_in_any_order():
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    model, scene, _ = synth.workload("tiny")
    gt = scene.T_gt.T.reshape(1, 16).astype(F)

    def make():
        return StocsEstimator(scene.pos, scene.nrm, scene.prob, scene.pixel, model.pos, model.nrm, build_index=False)

    est = make()
    calls = _owners(est, gt)
    assert len(calls) == 13
    for name, call in calls:
        assert call() == 1, name
    est.close()

    est = make()
    for name, call in _owners(est, gt)[::2][::-1]:
        assert call() == 1, name
    est.close()

    make().close()
