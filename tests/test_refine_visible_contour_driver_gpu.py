"""stocs_single ... --mesh <ply> --refine-visible K --damped [...] --contour [w[,radius_px[,dist_m]]]: the driver's record line and the pose
it writes, which go through the façade (stocs_estimator::refine_poses_visible_contour), against StocsEstimator.refine_poses_visible_contour
on the same mesh file, frame and pose; and the refusals of the option: without --damped the error names it."""
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
from test_refine_visible_driver_gpu import _pose16  # noqa: E402
from test_vsd_driver_gpu import _estimator  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
LINE = re.compile(r"^refine-visible (\S+): contour iterations=(\d+) rejected=(\d+) evaluations=(\d+) cost=(\S+) lambda=(\S+) frozen=(\d+) present=(\d+) no_depth=(\d+) "
                  r"off_class=(\d+) too_far=(\d+) grazing=(\d+) counted=(\d+) rms=(\S+) object_px=(\d+) uncovered=(\d+) unreached=(\d+) beyond=(\d+) pulled=(\d+) "
                  r"pull_rms=(\S+) mesh=(\d+)$")


def test_driver_refines_the_written_pose_with_the_contour_term(tmp_path):
    import ctypes as C
    from model_matching_amd import capi, cloudio, synth
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    K, scale = [float(x) for x in raw["K"]], float(raw["depth_scale"])
    pre = subprocess.run([PRE, obj, "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                          "--model-scale", repr(float(raw["model_scale"]))], capture_output=True, text=True, timeout=300)
    assert pre.returncode == 0, pre.stdout + pre.stderr
    L = capi.load()
    n, hn = C.c_int(0), C.c_int(0)
    mp = str(repo / "models" / obj / "model_search.ply").encode()
    assert L.stocs_ply_read(mp, None, None, 0, C.byref(n), C.byref(hn)) == 0
    mpos, mnrm = np.zeros((n.value, 3), F), np.zeros((n.value, 3), F)
    assert L.stocs_ply_read(mp, mpos.ctypes.data_as(capi._fp), mnrm.ctypes.data_as(capi._fp), n.value, C.byref(n), C.byref(hn)) == 0
    lo, hi = mpos.min(axis=0).astype(np.float64), mpos.max(axis=0).astype(np.float64)
    sv, st = synth.icosphere(3)                  # a synthetic mesh on the model's frame: an icosphere scaled to the cloud's bounding box
    mesh = tmp_path / "model_mesh.ply"
    cloudio.write_ply_mesh(mesh, (sv * (hi - lo) / 2 + (hi + lo) / 2).astype(F), st)
    out = tmp_path / "pose.txt"
    base = [APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(scale), "--seed", "7", "--out", str(out)]
    r = subprocess.run(base + ["--mesh", str(mesh), "--refine-visible", "5", "--contour"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--contour [w[,radius_px[,dist_m]]] needs --damped" in r.stderr and "RUNNING STOCS" not in r.stdout, r.stderr
    r = subprocess.run(base + ["--mesh", str(mesh), "--vsd", "--contour"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "needs --refine-visible" in r.stderr and "RUNNING STOCS" not in r.stdout, r.stderr
    for value in ("-1", "1,0", "1,65", "1,16,0", "1,16,0.03,2", "1,x"):
        r = subprocess.run(base + ["--mesh", str(mesh), "--refine-visible", "5", "--damped", "--contour", value], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--contour [w[,radius_px[,dist_m]]] needs w >= 0" in r.stderr and "RUNNING STOCS" not in r.stdout, (value, r.stderr)
    r = subprocess.run(base + ["--mesh", str(mesh), "--refine-visible", "5,0.03", "--damped", "0.5,3", "--contour", "0.5,24,0.04"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    got = [LINE.match(ln) for ln in lines if ln.startswith("refine-visible ")]
    assert len(got) == 1 and got[0], [ln for ln in lines if ln.startswith("refine-visible ")]
    m = got[0]
    poses = [ln for ln in lines if ln.startswith("pose:")]
    assert len(poses) == 2 and lines.index(poses[1]) > lines.index(m.group(0))
    v, t = cloudio.read_ply_mesh(mesh)
    est = _estimator(mpos, mnrm)
    est.set_frame(raw["depth"].astype(np.uint16), raw["prob"].astype(np.uint16), K, scale)
    est.set_mesh(v, t)
    first = _pose16(poses[0])                    # the driver refines the FILE's pose: the search's pose at the file's six significant digits
    filed = _pose16("pose: " + " ".join("%g" % x for x in first.reshape(4, 4).T[:3].reshape(12)))
    P, rec = est.refine_poses_visible_contour(filed, max_iterations=5, max_distance=0.03, lambda0=0.5, max_step_rotation=float(F(3.0 * np.pi / 180.0)), contour_weight=0.5,
                                              pull_radius_px=24, pull_distance=0.04)
    est.close()
    assert m.group(1) == obj and int(m.group(21)) == len(t) == 1280
    assert (int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(7))) == tuple(int(rec[k][0]) for k in ("iterations", "rejected", "evaluations", "frozen"))
    assert F(m.group(5)) == rec["cost"][0] and F(m.group(6)) == rec["lambda"][0] and F(m.group(14)) == rec["rms"][0] and F(m.group(20)) == rec["pull_rms"][0]
    names = ("present", "no_depth", "off_class", "too_far", "grazing", "counted")
    assert tuple(int(m.group(8 + j)) for j in range(6)) == tuple(int(rec[k][0]) for k in names)
    names = ("object_px", "uncovered", "unreached", "beyond", "pulled")
    assert tuple(int(m.group(15 + j)) for j in range(5)) == tuple(int(rec[k][0]) for k in names)
    assert int(m.group(15)) > 0 and int(m.group(4)) == 6 and int(m.group(2)) + int(m.group(3)) == 5
    assert np.array_equal(_pose16(poses[1]).view(np.uint32), P[0].view(np.uint32))
    written = np.array(out.read_text().split(), np.float64)
    assert written.shape == (12,) and np.all(np.isfinite(written))
    if int(m.group(2)) > 0:
        assert np.allclose(written, _pose16(poses[1]).reshape(4, 4).T[:3].reshape(12), rtol=1e-5, atol=1e-6)
