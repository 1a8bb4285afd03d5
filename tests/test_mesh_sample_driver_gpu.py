"""From a mesh file to a pose and its evaluation with one model representation: the closed loop on the level-4 Cm mesh and on the box
(the mesh rendered at the ground truth is the frame, stocs_preprocess_model_mesh makes the model, sixteen trials search, ADD and the
mesh's own VSD judge the best trial), and the tool chain model_preprocess --mesh -> stocs_single on a tree of files.

"The best trial" is the one of the sixteen with the smallest ADD: the test asks whether the search finds the pose with this model, not
whether the score picks it.  On Cm it cannot ask the latter: the solid is an oblate ellipsoid of revolution with one bump, and the
project's own record (profiles/trial_recall.json) has 47 % of the trials' highest-scoring poses within 0.1 diameter by ADD at 100 % by
ADD-S -- the score does not tell the bump's side.  Here, on an MI355X: 2 of 16 trials within 0.1 diameter with the model from the mesh
(1 of 16 with make_model's cloud on the same frame), the highest-scoring trial at ADD 0.57 diameters and VSD 0.04; the box 16 of 16.
The figures are printed, and tools/mesh_sample_quality.py --recall records them in profiles/mesh_sample_quality.json."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_sample_cases as mc  # noqa: E402
from test_pose_error_gpu import APP, PRE, _write_example_tree  # noqa: E402
from model_matching_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
VSD_TAU_INDEX, VSD_THETA = 3, 0.3          # the single-threshold VSD criterion: tau = 0.20 diameters (BOP's fourth), error below 0.3


def _judge(r, what):
    best = r["best"]
    share = float((r["add_over_diameter"] < 0.1).mean())
    w = r["winner"]
    print("%s: %d scene points, %d model points, %d of %d trials within 0.1 diameter; the best (trial %d, score %.3f): ADD %.4f diameters, VSD %.3f at tau %d; "
          "the highest score (trial %d, %.3f): ADD %.4f diameters, VSD %.3f"
          % (what, r["scene_points"], r["model_points"], round(share * mc.LOOP_TRIALS), mc.LOOP_TRIALS, best, r["lcp"][best], r["add_over_diameter"][best],
             r["vsd"]["e"][VSD_TAU_INDEX], VSD_TAU_INDEX, w, r["lcp"][w], r["add_over_diameter"][w], r["vsd_winner"]["e"][VSD_TAU_INDEX]))
    assert r["add_over_diameter"][best] < 0.1, what                           # pose_recall's own threshold: k = 0.1 diameters
    assert r["vsd"]["valid"] == 1 and r["vsd"]["e"][VSD_TAU_INDEX] < VSD_THETA, what


def test_closed_loop_on_the_level_4_cm_mesh():
    v, t = synth.make_model_mesh(4)
    _judge(mc.closed_loop(v, t), "Cm level 4")


def test_closed_loop_on_the_box():
    """the box maps onto itself under a half turn about each of its axes, so a correct pose need not be the ground truth's: plain ADD is
    defeated by the symmetry and the error is pose_errors_sym's, under the set of the descriptor (180, 180, 180)"""
    from model_matching_amd.estimator import symmetry_set
    v, t = mc.box()
    _judge(mc.closed_loop(v, t, symmetries=symmetry_set((180, 180, 180))), "box")


def test_tool_chain_from_a_mesh_file(tmp_path):
    from model_matching_amd import capi, cloudio
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    K = [float(x) for x in raw["K"]]
    mdir = repo / "models" / obj
    # a mesh on the frame and at the scale of the example's raw model: an icosphere scaled to its bounding box
    lo, hi = raw["model_raw"].min(axis=0).astype(np.float64), raw["model_raw"].max(axis=0).astype(np.float64)
    sv, st = synth.icosphere(3)
    mesh = tmp_path / "model_mesh.ply"
    cloudio.write_ply_mesh(mesh, (sv * (hi - lo) / 2 + (hi + lo) / 2).astype(F), st)
    scale, voxel = float(raw["model_scale"]), float(raw["model_voxel"])
    base = [PRE, obj, "--repo", str(repo), "--voxel", repr(voxel), "--model-scale", repr(scale)]
    # the refusals, with the texts stocs_single --mesh uses; an option of the mesh path without --mesh
    for extra, text in ((["--mesh", str(scene / "depth.png")], "cannot read a mesh"), (["--mesh", str(mdir / "textured_vertices.ply")], "no faces"),
                        (["--spacing", "0.002"], "need --mesh"), (["--mesh", str(mesh), "--orient", "up"], "winding or origin")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and text in r.stderr and not (mdir / "ppf_map").exists(), (extra, r.stdout, r.stderr)
    r = subprocess.run(base + ["--mesh", str(mesh), "--sample-seed", "5", "--orient", "winding"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "After sampling |M|=" in r.stdout, r.stdout + r.stderr
    assert (mdir / "model_search.ply").exists() and (mdir / "ppf_map").stat().st_size > 0
    L = capi.load()
    n, hn = C.c_int(0), C.c_int(0)
    mp = str(mdir / "model_search.ply").encode()
    assert L.stocs_ply_read(mp, None, None, 0, C.byref(n), C.byref(hn)) == 0 and n.value > 100 and hn.value == 1
    mpos, mnrm = np.zeros((n.value, 3), F), np.zeros((n.value, 3), F)
    assert L.stocs_ply_read(mp, mpos.ctypes.data_as(capi._fp), mnrm.ctypes.data_as(capi._fp), n.value, C.byref(n), C.byref(hn)) == 0
    # what the file holds is what the C ABI gives for the same mesh (the file keeps nine significant digits: the same floats)
    from model_matching_amd.estimator import preprocess_model_mesh
    v, tt = cloudio.read_ply_mesh(mesh)
    wpos, wnrm = preprocess_model_mesh(v, tt, voxel, seed=5, model_scale=scale)
    assert len(wpos) == n.value and np.array_equal(mpos, wpos) and np.array_equal(mnrm, wnrm)
    centre = (hi + lo) / 2 * scale
    assert ((mpos - centre) * mnrm).sum(axis=1).min() > 0                       # outward, from the winding
    # the driver runs on the tree
    r = subprocess.run([APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(float(raw["depth_scale"])),
                        "--seed", "7", "--trials", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUNNING STOCS" in r.stdout, r.stdout + r.stderr
