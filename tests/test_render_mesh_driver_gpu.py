"""stocs_single ... --instances M --masks --mesh <ply> --surface mesh: the driver's mask lines and label image from the mesh, which go
through the façade (stocs_estimator::set_mesh, explain_poses_mesh), against the C ABI called from Python on the same mesh file, frame and
instance poses; and the two refusals of the new option."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_pose_error_gpu import APP, PRE, _write_example_tree  # noqa: E402
from test_vsd_driver_gpu import _estimator  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MASK_LINE = re.compile(r"^mask (\d+): footprint (\d+) visible (\d+) hidden (\d+) agree (\d+) in_front (\d+) behind (\d+) no_depth (\d+) on_mask (\d+) mesh=(\d+)$")


def test_driver_masks_from_the_mesh(tmp_path):
    from model_matching_amd import capi, cloudio, synth
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    K, scale = [float(x) for x in raw["K"]], float(raw["depth_scale"])
    pre = subprocess.run([PRE, obj, "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                          "--model-scale", repr(float(raw["model_scale"]))], capture_output=True, text=True, timeout=300)
    assert pre.returncode == 0, pre.stdout + pre.stderr
    # the model cloud the driver reads, and a synthetic mesh on its frame: an icosphere scaled to the cloud's bounding box
    L = capi.load()
    n, hn = C.c_int(0), C.c_int(0)
    mp = str(repo / "models" / obj / "model_search.ply").encode()
    assert L.stocs_ply_read(mp, None, None, 0, C.byref(n), C.byref(hn)) == 0
    mpos, mnrm = np.zeros((n.value, 3), F), np.zeros((n.value, 3), F)
    assert L.stocs_ply_read(mp, mpos.ctypes.data_as(capi._fp), mnrm.ctypes.data_as(capi._fp), n.value, C.byref(n), C.byref(hn)) == 0
    lo, hi = mpos.min(axis=0).astype(np.float64), mpos.max(axis=0).astype(np.float64)
    sv, st = synth.icosphere(3)
    mesh = tmp_path / "model_mesh.ply"
    cloudio.write_ply_mesh(mesh, (sv * (hi - lo) / 2 + (hi + lo) / 2).astype(F), st)
    base = [APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(scale), "--seed", "7",
            "--trials", "4", "--cluster", "1"]
    # refused before any search: --surface mesh without --mesh, without --masks; an unknown surface; and --mesh alone keeps its text
    for extra, text in ((["--instances", "4", "--masks", "--surface", "mesh"], "--surface mesh needs"),
                        (["--instances", "4", "--mesh", str(mesh), "--surface", "mesh"], "--surface mesh needs"),
                        (["--instances", "4", "--masks", "--surface", "surfels"], "--surface takes"),
                        (["--instances", "4", "--masks", "--mesh", str(mesh)], "--mesh <ply> needs --vsd and takes no --surfel-radius"),
                        (["--instances", "4", "--masks", "--mesh", str(mesh), "--surface", "points"], "--mesh <ply> needs --vsd and takes no --surfel-radius")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and text in r.stderr and "RUNNING STOCS" not in r.stdout, (extra, r.stderr)
    (tmp_path / "out").mkdir()
    r = subprocess.run(base + ["--instances", "4", "--masks", "--mesh", str(mesh), "--surface", "mesh", "--out", str(tmp_path / "out" / "pose.txt")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "out")) == ["labels_%s.pgm" % obj, "pose.txt", "pose_instances_%s.txt" % obj]
    # the same through the C ABI, from the poses the driver selected
    rows = np.array((tmp_path / "out" / ("pose_instances_%s.txt" % obj)).read_text().split(), np.float64).astype(F).reshape(-1, 12)
    assert len(rows) >= 1
    poses = np.stack([np.vstack([q.reshape(3, 4), [0, 0, 0, 1]]).T.reshape(16) for q in rows]).astype(F)
    v, t = cloudio.read_ply_mesh(mesh)
    est = _estimator(mpos, mnrm)
    est.set_frame(raw["depth"].astype(np.uint16), raw["prob"].astype(np.uint16), K, scale)
    est.set_mesh(v, t)
    rec, lab, _ = est.explain_poses_mesh(poses, labels=True)
    splat = est.explain_poses(poses)
    est.close()
    got = [MASK_LINE.match(ln) for ln in r.stdout.splitlines() if ln.startswith("mask ")]
    assert len(got) == len(rows) and all(got), [ln for ln in r.stdout.splitlines() if ln.startswith("mask ")]
    for i, (m, q) in enumerate(zip(got, rec)):
        assert int(m.group(1)) == i and int(m.group(10)) == len(t) == 1280
        assert tuple(int(m.group(2 + j)) for j in range(8)) == tuple(int(q[k]) for k in ("footprint", "visible", "hidden", "agree", "in_front", "behind", "no_depth", "on_mask"))
    assert rec["footprint"][0] > 1000 and rec["footprint"][0] != splat["footprint"][0]            # the mesh's mask, not the splats'
    pgm = (tmp_path / "out" / ("labels_%s.pgm" % obj)).read_bytes()
    head = b"P5\n640 480\n65535\n"
    assert pgm.startswith(head) and len(pgm) == len(head) + 640 * 480 * 2
    assert np.array_equal(np.frombuffer(pgm[len(head):], ">u2").reshape(480, 640).astype(np.int32), lab + 1)
