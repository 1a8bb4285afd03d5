"""stocs_single --gt ... --vsd --mesh <ply>: the driver's VSD lines from the mesh, which go through the façade (stocs_estimator::set_mesh,
pose_errors_vsd_mesh), against the C ABI called from Python on the same mesh file, the same frame and the same pose files; and the Python
path (set_mesh, pose_errors_vsd_mesh with BOP's taus, render_depth_mesh, pose_recall_vsd) on the level-4 Cm mesh at VGA against the numpy
restatement.  The driver prints floats with nine significant digits, which name a float32 uniquely, so the comparison is equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_cases as mc  # noqa: E402
import mesh_ref as ref  # noqa: E402
import vsd_cases as vc  # noqa: E402
from test_pose_error_gpu import APP, PRE, _gt_line, _write_example_tree  # noqa: E402
from test_vsd_driver_gpu import _estimator, _read_pose  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def test_driver_reports_the_mesh_vsd_the_c_abi_gives(tmp_path):
    from model_matching_amd import capi, cloudio, synth
    from model_matching_amd.estimator import _VSD_DTYPE, pose_recall_vsd
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    K = [float(x) for x in raw["K"]]
    scale = float(raw["depth_scale"])
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
    base = [APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(scale), "--seed", "7"]
    out = scene / ("best_pose_candidate_%s.txt" % obj)
    r = subprocess.run(base + ["--trials", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    own = _read_pose(out).astype(np.float64).reshape(4, 4).T
    gt = tmp_path / "gt.txt"
    gt.write_text("\n".join(" ".join("%.9g" % F(x) for x in row) for row in (vc.translation(0.003, 0.0, 0.004) @ own)[:3]) + "\n")
    # refused before any search: --mesh without --vsd, with a surfel radius, a file that is no mesh, a file without faces
    for extra, text in ((["--gt", str(gt), "--mesh", str(mesh)], "needs --vsd"), (["--gt", str(gt), "--vsd", "--mesh", str(mesh), "--surfel-radius", "0.01"], "needs --vsd"),
                        (["--gt", str(gt), "--vsd", "--mesh", str(gt)], "cannot read a mesh"), (["--gt", str(gt), "--vsd", "--mesh", mp.decode()], "no faces")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and text in r.stderr and "RUNNING STOCS" not in r.stdout, (extra, r.stderr)
    r = subprocess.run(base + ["--trials", "4", "--gt", str(gt), "--vsd", "--mesh", str(mesh)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _gt_line(r.stdout, "gt %s vsd: " % obj)
    rec = _gt_line(r.stdout, "gt %s vsd recall: " % obj)
    # the same through the C ABI
    v, t = cloudio.read_ply_mesh(mesh)
    est = _estimator(mpos, mnrm)
    est.set_frame(raw["depth"].astype(np.uint16), None, K, scale)
    est.set_mesh(v, t)
    want = est.pose_errors_vsd_mesh(_read_pose(out), _read_pose(gt))[0]          # taus None: BOP's, from the diameter
    surfels = est.pose_errors_vsd(_read_pose(out), _read_pose(gt))[0]
    est.close()
    assert got["taus"] == 10 and got["valid"] == 1 and F(got["delta"]) == F(0.015) and got["mesh"] == len(t) == 1280 and "surfel_radius" not in got
    for k in range(10):
        assert F(got["e%d" % k]) == want["e"][k], (k, got, want)
    for k in ("px_est", "px_gt", "vis_est", "vis_gt", "inter", "uni"):
        assert int(got[k]) == want[k], (k, got[k], want[k])
    assert want["px_est"] > 1000 and want["px_est"] != surfels["px_est"]                 # the mesh's image, not the surfels'
    w = np.zeros(4, _VSD_DTYPE)
    for i in range(4):
        line = _gt_line(r.stdout, "gt %s vsd trial %d: " % (obj, i))
        w["valid"][i] = int(line["valid"])
        for k in range(10):
            w["e"][i][k] = F(line["e%d" % k])
    ar, nv = pose_recall_vsd(w)
    assert rec["trials"] == 4 and rec["valid"] == nv and abs(rec["vsd"] - ar) < 1e-8, (rec, ar, nv)


def test_python_path_on_the_level_4_cm_mesh():
    """the 6 400-triangle Cm mesh at VGA on a frame that shows its ground truth in front of a wall: the ground truth against itself,
    pushed along z either way and turned a little, and no pose; BOP's taus from the model cloud's diameter"""
    from model_matching_amd import synth
    from model_matching_amd.estimator import pose_recall_vsd
    pos, nrm = vc.cm_model()
    v, t = mc.cm_mesh(4)
    W, H = 640, 480
    T = synth.gt_pose()
    G = vc.pose16(T)
    turn = np.eye(4); turn[:3, :3] = vc.rot((0, 0, 1), 10)
    E = np.stack([G, vc.pose16(vc.translation(0, 0, 0.03) @ T), vc.pose16(vc.translation(0, 0, -0.03) @ T), vc.pose16(T @ turn), np.zeros(16, F)])
    zG = ref.render_depth(G, v, t, vc.YCB_K, W, H)[0]
    frame = vc.raw_from_depth(np.where(zG > 0, zG, 1.5))
    est = _estimator(pos, nrm)
    est.set_frame(frame, None, vc.YCB_K, vc.DEPTH_SCALE)
    est.set_mesh(v, t)
    assert est.mesh_info() == (len(v), 6400)
    got = est.pose_errors_vsd_mesh(E, G)
    dia = F(est.model_diameter())
    z = est.render_depth_mesh(E[:2])
    est.close()
    taus = [F(0.05 * i) * dia for i in range(1, 11)]
    want = ref.pose_errors_vsd_mesh(E, G, v, t, frame, vc.YCB_K, vc.DEPTH_SCALE, taus)
    bad = [i for i in range(len(E)) if not ref.records_equal(got[i], want[i])]
    assert not bad, (bad, got[bad[0]], want[bad[0]])
    assert np.array_equal(z[0].view(np.uint32), zG.view(np.uint32))
    assert np.array_equal(z[1].view(np.uint32), ref.render_depth(E[1], v, t, vc.YCB_K, W, H)[0].view(np.uint32))
    assert got["uni"][0] == got["inter"][0] == got["px_gt"][0] > 30000 and np.all(got["e"][0] == 0)
    assert got["valid"].tolist() == [1, 1, 1, 1, 0] and np.all(got["e"][4][:10] == 1)
    ar, nv = pose_recall_vsd(got)
    assert nv == 4 and 0.2 <= ar < 1.0
