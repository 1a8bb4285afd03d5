"""Two touching objects in a depth-only frame through the pipeline: one 640 x 480 closed loop in the manner of test_segment_driver_gpu.py.  The
box of mesh_sample_cases at synth.gt_pose() is the target; a second, longer and lower box (14 x 6 x 4 cm) lies against its long side, 2.5 cm
farther from the camera, in the same orientation, both in front of a wall at 1.2 m and with no class image.  Their depths meet without a jump, so
plain segmentation gives one segment over both; between the second box's front face and the exposed strip of the target's side face runs a
concave crease, and the cut takes them apart.  The second box is longer than the target on purpose: where two objects end together, the last
pixels of the crease have no triple that fits inside the foreground and the join survives there (checked on the restatement while the frame was
fixed: with a second box of the target's own length the two stay one segment through four pixels at the crease's end).  The conditions are
asserted on the CPU restatement first.  Then the search runs on the segment's class image and on the true silhouette, and stocs_single --segment
--segment-convex runs on a written example tree."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_sample_cases as mc  # noqa: E402
import segment_convex_ref as cr  # noqa: E402
import vsd_cases as vc  # noqa: E402
from test_pose_error_gpu import APP, PRE, _write_example_tree  # noqa: E402
from model_matching_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
WALL = 1.2
OTHER_SIZE, OTHER_OFFSET = (0.14, 0.06, 0.04), (0.0, -0.06, 0.025)        # in the target's own frame: against its -y side, 2.5 cm farther along +z
_FRAME = {}


def loop_frame():
    """the frame, the two silhouettes, the ground truth, the target's mesh: rendered once"""
    if not _FRAME:
        import mesh_ref
        v, t = mc.box()
        v2, t2 = synth.box_mesh(OTHER_SIZE)
        G = vc.pose16(synth.gt_pose())
        z1 = mesh_ref.render_depth(G, v, t, vc.YCB_K, 640, 480)[0]
        z2 = mesh_ref.render_depth(G, (v2 + np.asarray(OTHER_OFFSET, F)).astype(F), t2, vc.YCB_K, 640, 480)[0]
        a, b = np.where(z1 > 0, z1, np.inf), np.where(z2 > 0, z2, np.inf)
        z = np.minimum(a, b)
        _FRAME.update(frame=vc.raw_from_depth(np.where(np.isfinite(z), z, WALL)), target=(a <= b) & (z1 > 0), other=(b < a) & (z2 > 0), G=G, verts=v, tris=t)
    return _FRAME


def main_segment(labels, target):
    """the segment that holds most of the target's silhouette: (its number, the share of the silhouette it covers)"""
    ids, n = np.unique(labels[target & (labels > 0)], return_counts=True)
    return int(ids[n.argmax()]), float(n.max()) / float(target.sum())


def test_closed_loop_on_a_box_that_touches_another():
    from model_matching_amd import estimator as E
    f = loop_frame()
    target, other = f["target"], f["other"]
    # the conditions, on the restatement alone (its own plane)
    own = cr.segment_frame_convex(f["frame"], vc.YCB_K, vc.DEPTH_SCALE)
    plain = own["plain"]
    one = plain["labels"] == 1
    assert plain["n_segments"] == 1 and (one & target).sum() >= 0.95 * target.sum() and (one & other).sum() >= 0.95 * other.sum()      # one segment over both
    k, cover = main_segment(own["labels"], target)
    seg = own["labels"] == k
    print("touching boxes, restatement: %d segments with the cut, segment %d covers %.4f of the target's %d pixels, %.4f of it is the other box, %d pixels cut"
          % (own["n_segments"], k, cover, int(target.sum()), float((seg & other).sum()) / float(seg.sum()), own["n_cut"]))
    assert cover >= 0.85 and (seg & other).sum() <= 0.02 * seg.sum()
    # the library's images are the restatement's on the library's plane
    res, records, images = E.segment_frame(f["frame"], vc.YCB_K, vc.DEPTH_SCALE, convex=True, images=("class_prob", "labels", "edge", "cut"))
    ref = cr.segment_frame_convex(f["frame"], vc.YCB_K, vc.DEPTH_SCALE, plane=res["plane"])
    assert res["plane_found"] == 1 and res["n_segments"] == ref["n_segments"] >= 2 and all(res[c] == ref[c] for c in cr.COUNTS)
    assert all(np.array_equal(images[n], ref[n]) for n in ("class_prob", "labels", "edge", "cut"))
    k, cover = main_segment(images["labels"], target)
    seg = images["labels"] == k
    assert cover >= 0.85 and (seg & other).sum() <= 0.02 * seg.sum()
    # the same trials on that segment's class image and on the true silhouette
    mpos, mnrm = E.preprocess_model_mesh(f["verts"], f["tris"], mc.LOOP_VOXEL, seed=mc.SEED)
    best = {}
    for name, cls in (("segment", E.segment_class_images(images["labels"], ids=[k])[0]), ("silhouette", np.where(target, 10000, 0).astype(np.uint16))):
        spos, snrm, sprob, spix = E.ingest_scene(f["frame"], cls, vc.YCB_K, vc.DEPTH_SCALE, voxel_size=mc.LOOP_VOXEL)
        est = E.StocsEstimator(spos, snrm, sprob, spix, mpos, mnrm, build_index=True)
        try:
            out = est.run_trials(np.arange(100, 100 + mc.LOOP_TRIALS, dtype=np.uint64), 100)
            P = np.stack([r["best_pose"] for r in out]).astype(F)
            err = est.pose_errors_sym(P, f["G"], E.symmetry_set((180, 180, 180)))
            add = np.where(err["valid"] != 0, err["add"], np.inf) / float(est.model_diameter())
        finally:
            est.close()
        best[name] = float(add.min())
        print("touching boxes, %s class image: %d scene points, %d of %d trials within 0.1 diameter, the best at %.4f diameters"
              % (name, len(spos), int((add < 0.1).sum()), mc.LOOP_TRIALS, best[name]))
    if best["silhouette"] < 0.1:
        assert best["segment"] < 0.1


def test_the_driver_cuts_a_written_example_tree(tmp_path):
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    K = [float(x) for x in raw["K"]]
    pre = subprocess.run([PRE, obj, "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                          "--model-scale", repr(float(raw["model_scale"]))], capture_output=True, text=True, timeout=300)
    assert pre.returncode == 0, pre.stdout + pre.stderr
    os.remove(scene / "probability_maps" / (obj + ".png"))                              # a depth-only tree: no class image anywhere
    base = [APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(float(raw["depth_scale"])), "--seed", "7",
            "--trials", "2"]
    r = subprocess.run(base + ["--segment-convex", "4,2,25"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--segment-convex [r[,s[,deg]]] needs --segment" in r.stderr
    out = tmp_path / "pose.txt"
    r = subprocess.run(base + ["--segment", "0.01,200", "--segment-convex", "4,2,25", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "segment: plane found" in r.stdout and "RUNNING STOCS" in r.stdout, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("segment convex:")]
    assert len(line) == 1 and "radius 4, smoothing 2" in line[0] and "pixels cut" in line[0], r.stdout
    m = re.search(r": (\d+) \+ (\d+) triples tested, (\d+) \+ (\d+) cut, (\d+) pixels cut$", line[0])
    assert m, line[0]
    th, tv, ch, cv, cut = (int(x) for x in m.groups())
    assert th > 0 and tv > 0 and 0 < max(ch, cv) <= cut <= ch + cv, line[0]
    pose = np.loadtxt(out)
    assert pose.size >= 12 and np.isfinite(pose).all()
