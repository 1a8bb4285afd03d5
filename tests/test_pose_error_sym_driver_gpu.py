"""stocs_single --gt ... --sym ...: the driver's symmetric lines, which go through the façade (stocs_estimator::pose_errors_sym,
stocs::symmetry_set), against the C ABI called from Python on the same model and the same pose files.  The driver prints floats with nine
significant digits, which name a float32 uniquely, so the comparison is equality of every float; the measures are integer sums and maxima,
so the order in which the façade hands the model over plays no part."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pose_error_cases as pc  # noqa: E402
from test_pose_error_gpu import APP, PRE, _est, _gt_line, _write_example_tree  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def _read_pose(path):
    v = np.array([float(x) for x in open(path).read().split()[:12]]).astype(F).reshape(3, 4)
    P = np.eye(4, dtype=F); P[:3] = v
    return P.T.reshape(16).copy()


def test_driver_reports_the_symmetric_errors_the_c_abi_gives(tmp_path):
    from model_matching_amd import capi
    from model_matching_amd.estimator import symmetry_set
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    K = [float(x) for x in raw["K"]]
    pre = subprocess.run([PRE, obj, "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                          "--model-scale", repr(float(raw["model_scale"]))], capture_output=True, text=True, timeout=300)
    assert pre.returncode == 0, pre.stdout + pre.stderr
    base = [APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(float(raw["depth_scale"])), "--seed", "7"]
    out = scene / ("best_pose_candidate_%s.txt" % obj)
    # refused before any search: --sym without --gt, a symmetry file that holds no whole transform
    r = subprocess.run(base + ["--sym", "0,0,360"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "needs --gt" in r.stderr and "RUNNING STOCS" not in r.stdout
    r = subprocess.run(base + ["--trials", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not [l for l in r.stdout.splitlines() if l.startswith("gt ")], r.stdout + r.stderr
    # the ground truth: this run's own pose turned by 137 degrees about the model's z and moved 2 mm
    own = _read_pose(out).astype(np.float64).reshape(4, 4).T
    D = np.eye(4); D[:3, :3] = pc.rot((0, 0, 1), 137.0); D[:3, 3] = (0.002, 0.0, 0.0)
    gt = tmp_path / "gt.txt"
    gt.write_text("\n".join(" ".join("%.9g" % F(x) for x in row) for row in (own @ D)[:3]) + "\n")
    bad = tmp_path / "bad_syms.txt"; bad.write_text("1 0 0 0 0 1 0\n")
    r = subprocess.run(base + ["--gt", str(gt), "--sym", "0,0,360", "--sym-file", str(bad)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "no symmetry set" in r.stderr and "RUNNING STOCS" not in r.stdout
    r = subprocess.run(base + ["--trials", "4", "--gt", str(gt), "--sym", "0,0,360", "--sym-steps", "72"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = _gt_line(r.stdout, "gt %s: " % obj)
    got = _gt_line(r.stdout, "gt %s sym: " % obj)
    rec = _gt_line(r.stdout, "gt %s sym recall: " % obj)
    # the same through the C ABI: model_search.ply as the driver read it, the two pose files as the driver reads them
    L = capi.load()
    n, hn = C.c_int(0), C.c_int(0)
    mp = str(repo / "models" / obj / "model_search.ply").encode()
    assert L.stocs_ply_read(mp, None, None, 0, C.byref(n), C.byref(hn)) == 0
    mpos, mnrm = np.zeros((n.value, 3), F), np.zeros((n.value, 3), F)
    assert L.stocs_ply_read(mp, mpos.ctypes.data_as(capi._fp), mnrm.ctypes.data_as(capi._fp), n.value, C.byref(n), C.byref(hn)) == 0
    est = _est(mpos)
    S = symmetry_set((0, 0, 360), 72)
    want = est.pose_errors_sym(_read_pose(out), _read_pose(gt), S, (K[0], K[1], K[2], K[3]))[0]
    d = est.model_diameter()
    est.close()
    assert got["symmetries"] == 72 and got["valid"] == 1
    for k in ("mssd", "add", "mspd"):
        assert F(got[k]) == want[k], (k, got[k], want[k])
    for k in ("k_mssd", "k_add", "k_mspd"):
        assert int(got[k]) == want[k], (k, got[k], want[k])
    assert plain["add"] > got["add"] and got["mssd"] < 0.1 * d < plain["add_max"]      # the turn is a symmetry's, nearly: 2 degrees and 2 mm remain
    # the recall line against pose_recall_sym on the records of the same four winners, which the driver prints one per line
    from model_matching_amd.estimator import _POSE_ERROR_SYM_DTYPE, pose_recall_sym
    w = np.zeros(4, _POSE_ERROR_SYM_DTYPE)
    for t in range(4):
        line = _gt_line(r.stdout, "gt %s sym trial %d: " % (obj, t))
        w["mssd"][t], w["add"][t], w["mspd"][t], w["valid"][t] = F(line["mssd"]), F(line["add"]), F(line["mspd"]), int(line["valid"])
    assert F(plain["diameter"]) == d
    ar3, ar2, ra, nv = pose_recall_sym(w, d, image_width=640)
    assert rec["trials"] == 4 and rec["valid"] == nv and nv >= 1
    assert abs(rec["mssd"] - ar3) < 1e-8 and abs(rec["mspd"] - ar2) < 1e-8 and abs(rec["add"] - ra) < 1e-8, (rec, ar3, ar2, ra)
