"""Two objects of one depth-only frame through segment_frame and segment_assign: a 640 x 480 frame in the manner of
test_segment_driver_gpu.py -- mc.box() at synth.gt_pose() and a scaled copy of it 16 cm to its right, rendered by tests/mesh_ref.py in front
of a wall at 1.2 m, no class image -- and stocs_single <tree> a,b --segment on a written example tree.

The scale of the copy is 0.22, not 0.5.  Before the frame was fixed the condition was checked on the restatement alone (it still is, below):
each object's gated class image holds at least 95 % of its own silhouette and no pixel of the other box or of the wall.  At 0.5 the copy's
segment is 5.0 cm wide and the box's middle extent 6 cm: TOO_SMALL asks for less than min_ratio * 6 cm = 3 cm, so the box keeps the copy's
segment (3007 pixels of it) and the condition fails; the copy's widest view is its 0.123 m * scale diagonal, below 3 cm from scale 0.24 down.

The closed loop: estimate_objects on the gated stack, sixteen trials per object, each object's best trial below 0.1 diameters under the
(180, 180, 180) set; the same search on the true silhouettes in the same test, and per object the gated run may have at most one trial fewer
within 0.1 diameters than that one.  Both counts are printed and recorded in profiles/segment_shapes.md.  The copy's model is preprocessed at
the closed loop's voxel times the scale, so both models hold about the same number of points; the frame is ingested at the loop's 5 mm."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_sample_cases as mc  # noqa: E402
import segment_ref as sr  # noqa: E402
import segment_shapes_ref as shr  # noqa: E402
import vsd_cases as vc  # noqa: E402
from test_pose_error_gpu import APP, PRE, _write_example_tree  # noqa: E402
from model_matching_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
WALL = 1.2
SCALE = 0.22
SHIFT = (0.16, 0.05)
_FRAME = {}


def two_box_frame():
    """the frame, the two silhouettes, the two vertex sets: rendered once"""
    if not _FRAME:
        import mesh_ref
        v, t = mc.box()
        G = np.asarray(vc.pose16(synth.gt_pose()), np.float64).reshape(16)
        G2 = G.copy(); G2[12] += SHIFT[0]; G2[13] += SHIFT[1]
        z1 = mesh_ref.render_depth(G, v, t, vc.YCB_K, 640, 480)[0]
        z2 = mesh_ref.render_depth(G2, v * SCALE, t, vc.YCB_K, 640, 480)[0]
        assert not ((z1 > 0) & (z2 > 0)).any()
        z = np.where(z1 > 0, z1, np.where(z2 > 0, z2, WALL))
        _FRAME.update(frame=vc.raw_from_depth(z), sil=[z1 > 0, z2 > 0], verts=[v, v * SCALE], tris=t, G=[G.astype(F), G2.astype(F)])
    return _FRAME


def test_two_boxes_of_a_depth_only_frame_get_their_own_class_images():
    from model_matching_amd import estimator as E
    f = two_box_frame()
    ext = np.array(sorted(mc.BOX_SIZE, reverse=True), F)
    # the condition, on the restatement alone: its own labels, its own shapes, the objects' sizes from the boxes' dimensions
    own = sr.segment_frame(f["frame"], vc.YCB_K, vc.DEPTH_SCALE)
    n = int(own["labels"].max())
    shapes, _, _ = shr.segment_shapes(f["frame"], own["labels"], vc.YCB_K, vc.DEPTH_SCALE, n, 2.0)
    st = shr.stack(own["labels"], n, shr.gate(shapes, [shr.object_size(ext), shr.object_size(ext * F(SCALE))]))
    wall = ~f["sil"][0] & ~f["sil"][1]
    for k in range(2):
        assert ((st[k] > 0) & f["sil"][k]).sum() >= 0.95 * f["sil"][k].sum() and not ((st[k] > 0) & (f["sil"][1 - k] | wall)).any(), k
    # the library: its labels, the objects' sizes from their model clouds, one segment_assign; the stack is the restatement's on the same inputs
    res, records, images = E.segment_frame(f["frame"], vc.YCB_K, vc.DEPTH_SCALE)
    models = [E.preprocess_model_mesh(v, f["tris"], mc.LOOP_VOXEL * (1.0 if k == 0 else SCALE), seed=mc.SEED) for k, v in enumerate(f["verts"])]
    objects = np.stack([E.object_size(m[0]) for m in models])
    assert np.allclose(objects[0]["extent"], ext, atol=0.006) and objects[0]["diameter"] >= objects[0]["extent"].max()
    lshapes, reasons, stack, counts = E.segment_assign(f["frame"], images["labels"], vc.YCB_K, vc.DEPTH_SCALE, objects)
    assert res["n_segments"] == len(lshapes) == 2 and counts["n_used"] == counts["n_labelled"] == int((images["labels"] > 0).sum())
    want = shr.gate(lshapes, [(o["diameter"], o["extent"]) for o in objects])
    print("extents %s, objects %s, reasons %s" % (lshapes["extent"].tolist(), objects.tolist(), reasons.tolist()))
    assert reasons.tolist() == want.tolist() == [[0, shr.TOO_SMALL], [shr.TOO_LARGE, 0]]
    assert stack.tobytes() == shr.stack(images["labels"], 2, want).tobytes()
    for k in range(2):
        assert ((stack[k] > 0) & f["sil"][k]).sum() >= 0.95 * f["sil"][k].sum() and not ((stack[k] > 0) & (f["sil"][1 - k] | wall)).any(), k
    # and the stack is what the multi-object ingest takes: each object's cloud lies on its own box
    scenes = E.ingest_scene_multi(f["frame"], stack, vc.YCB_K, vc.DEPTH_SCALE, voxel_size=mc.LOOP_VOXEL)
    assert len(scenes) == 2 and len(scenes[0][0]) > 100
    for k in range(2):
        px = scenes[k][3]
        assert f["sil"][k][px[:, 0], px[:, 1]].all()
    # the closed loop: the search on the gated stack, and the same search with the true silhouettes as class images
    true = np.stack([np.where(sil, 10000, 0).astype(np.uint16) for sil in f["sil"]])
    within = {}
    for name, scn in (("gated", scenes), ("true silhouettes", E.ingest_scene_multi(f["frame"], true, vc.YCB_K, vc.DEPTH_SCALE, voxel_size=mc.LOOP_VOXEL))):
        out = E.estimate_objects(scn, models, np.arange(100, 100 + mc.LOOP_TRIALS, dtype=np.uint64), 100)
        for k in range(2):
            P = np.stack([r["best_pose"] for r in out[k]]).astype(F)
            est = E.StocsEstimator(*scn[k], *models[k], build_index=False)
            try:
                dia = float(est.model_diameter())
                err = est.pose_errors_sym(P, f["G"][k], E.symmetry_set((180, 180, 180)))
            finally:
                est.close()
            add = np.where(err["valid"] != 0, err["add"], np.inf) / dia
            within[name, k] = int((add < 0.1).sum())
            print("%s, object %d: %d scene points, %d model points, %d of %d trials within 0.1 diameters, the best at %.4f diameters (diameter %.4f m)"
                  % (name, k, len(scn[k][0]), len(models[k][0]), within[name, k], mc.LOOP_TRIALS, float(add.min()), dia))
            if name == "gated":
                assert add.min() < 0.1, (k, float(add.min()))
    for k in range(2):
        assert within["gated", k] >= within["true silhouettes", k] - 1, (k, within)


def test_the_driver_assigns_segments_to_two_objects_of_a_written_example_tree(tmp_path):
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    twin = obj + "_twin"                                                                   # the same model under a second name: objects of like size
    shutil.copytree(repo / "models" / obj, repo / "models" / twin)
    K = [float(x) for x in raw["K"]]
    for name in (obj, twin):
        pre = subprocess.run([PRE, name, "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                              "--model-scale", repr(float(raw["model_scale"]))], capture_output=True, text=True, timeout=300)
        assert pre.returncode == 0, pre.stdout + pre.stderr
    shutil.rmtree(scene / "probability_maps")                                              # a depth-only tree: no class image anywhere
    base = [APP, str(scene), obj + "," + twin, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(float(raw["depth_scale"])), "--seed", "7",
            "--trials", "2"]
    r = subprocess.run(base + ["--segment-gate", "0.25,0.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--segment-gate slack[,min_ratio] needs --segment" in r.stderr and "RUNNING STOCS" not in r.stdout
    r = subprocess.run(base + ["--segment", "--segment-gate", "0.25,1.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--segment-gate slack[,min_ratio] needs --segment" in r.stderr and "RUNNING STOCS" not in r.stdout
    r = subprocess.run(base + ["--segment", "0.01,200"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "segment: plane found" in r.stdout, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("segment assign: ")]
    assert len(lines) == 2 and lines[0].startswith("segment assign: %s: " % obj) and lines[1].startswith("segment assign: %s: " % twin), r.stdout
    counts = [l.split(": ")[2].split() for l in lines]                                     # "k of n segments"
    assert counts[0] == counts[1] and counts[0][1:] == ["of", counts[0][2], "segments"] and 1 <= int(counts[0][0]) <= int(counts[0][2])   # like sizes: the gate keeps the same segments
    for name in (obj, twin):
        pose = np.loadtxt(scene / ("best_pose_candidate_%s.txt" % name))
        assert pose.size >= 12 and np.isfinite(pose).all()
