"""A depth-only frame through the pipeline: one 640 x 480 closed loop in the manner of mesh_sample_cases.closed_loop with NO class image given.
The box rendered by tests/mesh_ref.py at synth.gt_pose() stands in front of a wall; segment_frame makes the class image from the depth image,
ingest_scene and preprocess_model_mesh feed the search, sixteen trials, judged as the existing box test is (the best trial below 0.1 diameters
by pose_errors_sym under the set of (180, 180, 180)).  The wall stands at 1.2 m: with the closed loop's own 1.5 m the box, at 0.8 m, is
0.7 m off the wall -- beyond the default max_height of 0.5 m -- and the restatement keeps nothing (checked on the CPU before the frame was
fixed); at 1.2 m it covers the whole silhouette and no wall pixel.  The same class image then goes to set_frame and
refine_poses_visible_contour runs from a displaced start -- the call a depth-only frame could not make -- and stocs_single --segment runs on a
written example tree."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_sample_cases as mc  # noqa: E402
import segment_ref as sr  # noqa: E402
import vsd_cases as vc  # noqa: E402
from test_pose_error_gpu import APP, PRE, _write_example_tree  # noqa: E402
from model_matching_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
WALL = 1.2
_FRAME = {}


def loop_frame():
    """the frame, the silhouette, the ground truth, the mesh: rendered once"""
    if not _FRAME:
        import mesh_ref
        v, t = mc.box()
        G = vc.pose16(synth.gt_pose())
        z = mesh_ref.render_depth(G, v, t, vc.YCB_K, 640, 480)[0]
        _FRAME.update(frame=vc.raw_from_depth(np.where(z > 0, z, WALL)), sil=z > 0, G=G, verts=v, tris=t)
    return _FRAME


def segmented(est_mod):
    f = loop_frame()
    if "seg" not in f:
        f["seg"] = est_mod.segment_frame(f["frame"], vc.YCB_K, vc.DEPTH_SCALE)
    return f["seg"]


def test_closed_loop_on_the_box_without_a_class_image():
    from model_matching_amd import estimator as E
    f = loop_frame()
    res, records, images = segmented(E)
    # the conditions, on the restatement alone (its own plane): at least 95 % of the silhouette, no wall pixel
    own = sr.segment_frame(f["frame"], vc.YCB_K, vc.DEPTH_SCALE)
    kept = own["labels"] > 0
    assert (kept & f["sil"]).sum() >= 0.95 * f["sil"].sum() and not (kept & ~f["sil"]).any()
    # and the library's images are the restatement's on the library's plane
    ref = sr.segment_frame(f["frame"], vc.YCB_K, vc.DEPTH_SCALE, plane=res["plane"])
    assert res["plane_found"] == 1 and res["n_segments"] == ref["n_segments"] >= 1
    assert np.array_equal(images["class_prob"], ref["class_prob"]) and np.array_equal(images["labels"], ref["labels"]) and np.array_equal(images["edge"], ref["edge"])
    cls = images["class_prob"]
    assert ((cls > 0) & f["sil"]).sum() >= 0.95 * f["sil"].sum() and not ((cls > 0) & ~f["sil"]).any()
    spos, snrm, sprob, spix = E.ingest_scene(f["frame"], cls, vc.YCB_K, vc.DEPTH_SCALE, voxel_size=mc.LOOP_VOXEL)
    mpos, mnrm = E.preprocess_model_mesh(f["verts"], f["tris"], mc.LOOP_VOXEL, seed=mc.SEED)
    est = E.StocsEstimator(spos, snrm, sprob, spix, mpos, mnrm, build_index=True)
    try:
        out = est.run_trials(np.arange(100, 100 + mc.LOOP_TRIALS, dtype=np.uint64), 100)
        P = np.stack([r["best_pose"] for r in out]).astype(F)
        dia = float(est.model_diameter())
        err = est.pose_errors_sym(P, f["G"], E.symmetry_set((180, 180, 180)))
        add = np.where(err["valid"] != 0, err["add"], np.inf) / dia
    finally:
        est.close()
    best = int(np.argmin(add))
    print("depth-only box: %d scene points, %d model points, %d of %d trials within 0.1 diameter, the best (trial %d) at %.4f diameters"
          % (len(spos), len(mpos), int((add < 0.1).sum()), mc.LOOP_TRIALS, best, add[best]))
    assert add[best] < 0.1


def test_the_contour_refinement_accepts_the_segmented_class_image():
    from model_matching_amd import estimator as E
    f = loop_frame()
    cls = segmented(E)[2]["class_prob"]
    spos, snrm, sprob, spix = E.ingest_scene(f["frame"], cls, vc.YCB_K, vc.DEPTH_SCALE, voxel_size=mc.LOOP_VOXEL)
    mpos, mnrm = E.preprocess_model_mesh(f["verts"], f["tris"], mc.LOOP_VOXEL, seed=mc.SEED)
    est = E.StocsEstimator(spos, snrm, sprob, spix, mpos, mnrm, build_index=False)
    try:
        est.set_mesh(f["verts"], f["tris"])
        start = np.asarray(f["G"], F).copy().reshape(16)
        start[12] += 0.012; start[13] -= 0.008; start[14] += 0.006                      # displaced across and along the rays
        est.set_frame(f["frame"], None, vc.YCB_K, vc.DEPTH_SCALE)
        with pytest.raises(Exception):                                                  # the depth-only frame as it was: refused
            est.refine_poses_visible_contour(start[None], max_iterations=3)
        est.set_frame(f["frame"], cls, vc.YCB_K, vc.DEPTH_SCALE)
        P, rec, tr = est.refine_poses_visible_contour(start[None], trace=True, max_iterations=5)
    finally:
        est.close()
    assert rec["object_px"][0] == int((cls > 0).sum()) > 0
    assert np.isfinite(tr[0, 0]["cost"]) and float(rec["cost"][0]) <= float(tr[0, 0]["cost"])
    moved = float(np.linalg.norm(P[0][12:15] - np.asarray(f["G"], F).reshape(16)[12:15]))
    print("contour refinement on the segmented class image: cost %.6g -> %.6g, translation error %.4f -> %.4f m"
          % (tr[0, 0]["cost"], rec["cost"][0], float(np.linalg.norm([0.012, 0.008, 0.006])), moved))


def test_the_driver_segments_a_written_example_tree(tmp_path):
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    K = [float(x) for x in raw["K"]]
    pre = subprocess.run([PRE, obj, "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                          "--model-scale", repr(float(raw["model_scale"]))], capture_output=True, text=True, timeout=300)
    assert pre.returncode == 0, pre.stdout + pre.stderr
    os.remove(scene / "probability_maps" / (obj + ".png"))                              # a depth-only tree: no class image anywhere
    base = [APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(float(raw["depth_scale"])), "--seed", "7",
            "--trials", "2"]
    r = subprocess.run(base + ["--segment-edges"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--segment-edges needs --segment" in r.stderr
    out = tmp_path / "pose.txt"
    r = subprocess.run(base + ["--segment", "0.01,200", "--segment-edges", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "segment: plane found" in r.stdout and "RUNNING STOCS" in r.stdout, r.stdout + r.stderr
    pose = np.loadtxt(out)
    assert pose.size >= 12 and np.isfinite(pose).all()
