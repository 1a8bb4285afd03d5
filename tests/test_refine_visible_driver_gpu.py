"""stocs_single ... --mesh <ply> --refine-visible K[,dist[,cos]]: the driver's record line and the pose file it writes again, which go through
the façade (stocs_estimator::set_mesh, refine_poses_visible), against the C ABI called from Python on the same mesh file, frame and pose;
and the refusal of the option without a mesh."""
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
LINE = re.compile(r"^refine-visible (\S+): iterations=(\d+) frozen=(\d+) present=(\d+) no_depth=(\d+) off_class=(\d+) too_far=(\d+) grazing=(\d+) counted=(\d+) "
                  r"rms=(\S+) mesh=(\d+)$")


def _pose16(line):
    q = np.array(line.split()[1:], np.float64).astype(F).reshape(3, 4)
    return np.vstack([q, [0, 0, 0, 1]]).T.reshape(16).astype(F)


def test_driver_refines_the_written_pose_on_the_mesh(tmp_path):
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
    for extra in (["--refine-visible", "3"], ["--mesh", str(mesh), "--refine-visible", "3,-1"], ["--mesh", str(mesh), "--refine-visible", "3,0.02,1.5"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--refine-visible K[,dist[,cos]] needs" in r.stderr and "RUNNING STOCS" not in r.stdout, (extra, r.stderr)
    # ONE iteration: the record then describes the evaluation of the pose the search wrote (the icosphere is not the bowl, so further
    # iterations need not stay near it)
    r = subprocess.run(base + ["--mesh", str(mesh), "--refine-visible", "1,0.03"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    got = [LINE.match(ln) for ln in lines if ln.startswith("refine-visible ")]
    assert len(got) == 1 and got[0], [ln for ln in lines if ln.startswith("refine-visible ")]
    m = got[0]
    poses = [ln for ln in lines if ln.startswith("pose:")]
    assert len(poses) == 2 and lines.index(poses[1]) > lines.index(m.group(0))
    # the same through the C ABI from the pose the search printed
    v, t = cloudio.read_ply_mesh(mesh)
    est = _estimator(mpos, mnrm)
    est.set_frame(raw["depth"].astype(np.uint16), raw["prob"].astype(np.uint16), K, scale)
    est.set_mesh(v, t)
    # the driver refines the FILE's pose (what a reader of the file gets): the search's pose at the file's six significant digits
    first = _pose16(poses[0])
    filed = _pose16("pose: " + " ".join("%g" % x for x in first.reshape(4, 4).T[:3].reshape(12)))
    P, rec = est.refine_poses_visible(filed, max_iterations=1, max_distance=0.03)
    est.close()
    assert m.group(1) == obj and int(m.group(11)) == len(t) == 1280
    names = ("iterations", "frozen", "present", "no_depth", "off_class", "too_far", "grazing", "counted")
    assert tuple(int(m.group(2 + j)) for j in range(8)) == tuple(int(rec[k][0]) for k in names)
    assert F(m.group(10)) == rec["rms"][0]                                  # nine significant digits give the float back
    if rec["iterations"][0] > 0:
        assert np.array_equal(_pose16(poses[1]).view(np.uint32), P[0].view(np.uint32))
    assert int(m.group(4)) == sum(int(m.group(k)) for k in (5, 6, 7, 8, 9)) and int(m.group(4)) > 1000
    assert int(m.group(2)) + int(m.group(3)) >= 1
    written = np.array(out.read_text().split(), np.float64)
    assert written.shape == (12,) and np.all(np.isfinite(written))
    if int(m.group(2)) > 0:
        assert np.allclose(written, _pose16(poses[1]).reshape(4, 4).T[:3].reshape(12), rtol=1e-5, atol=1e-6)
        assert not np.allclose(written, first.reshape(4, 4).T[:3].reshape(12), rtol=1e-7, atol=1e-9)
