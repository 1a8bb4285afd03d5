"""stocs_single --gt ... --vsd: the driver's VSD lines, which go through the façade (stocs_estimator::pose_errors_vsd, default_vsd_params),
against the C ABI called from Python on the same model, the same frame and the same pose files; and the Python path (pose_errors_vsd with
BOP's taus, render_depth, pose_recall_vsd) on the ycb fixture against the numpy restatement.  The driver prints floats with nine
significant digits, which name a float32 uniquely, so the comparison is equality of every float; the counts are integer sums, so the
order in which the façade hands the model over plays no part."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vsd_cases as vc  # noqa: E402
import vsd_ref as ref  # noqa: E402
from test_pose_error_gpu import APP, PRE, _gt_line, _write_example_tree  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
GOLD = os.path.join(ROOT, "tests", "golden")


def _read_pose(path):
    v = np.array([float(x) for x in open(path).read().split()[:12]]).astype(F).reshape(3, 4)
    P = np.eye(4, dtype=F); P[:3] = v
    return P.T.reshape(16).copy()


def _estimator(mpos, mnrm):
    from model_matching_amd.estimator import StocsEstimator
    rng = np.random.default_rng(1)
    sp = rng.normal(0, 0.05, (32, 3)).astype(F)
    sn = sp / np.linalg.norm(sp, axis=1, keepdims=True)
    return StocsEstimator(sp, sn, np.ones(32, F), None, mpos, mnrm, build_index=False)


def test_driver_reports_the_vsd_the_c_abi_gives(tmp_path):
    from model_matching_amd import capi
    from model_matching_amd.estimator import _VSD_DTYPE, pose_recall_vsd
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    K = [float(x) for x in raw["K"]]
    scale = float(raw["depth_scale"])
    pre = subprocess.run([PRE, obj, "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                          "--model-scale", repr(float(raw["model_scale"]))], capture_output=True, text=True, timeout=300)
    assert pre.returncode == 0, pre.stdout + pre.stderr
    base = [APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(scale), "--seed", "7"]
    out = scene / ("best_pose_candidate_%s.txt" % obj)
    # refused before any search: --vsd without --gt, a delta that is no length
    r = subprocess.run(base + ["--vsd"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "needs --gt" in r.stderr and "RUNNING STOCS" not in r.stdout
    r = subprocess.run(base + ["--trials", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not [l for l in r.stdout.splitlines() if l.startswith("gt ")], r.stdout + r.stderr
    # the ground truth: this run's own pose moved 3 mm sideways and 4 mm back
    own = _read_pose(out).astype(np.float64).reshape(4, 4).T
    gt = tmp_path / "gt.txt"
    gt.write_text("\n".join(" ".join("%.9g" % F(x) for x in row) for row in (vc.translation(0.003, 0.0, 0.004) @ own)[:3]) + "\n")
    r = subprocess.run(base + ["--gt", str(gt), "--vsd", "--vsd-delta", "-1"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "positive, finite" in r.stderr and "RUNNING STOCS" not in r.stdout
    r = subprocess.run(base + ["--trials", "4", "--gt", str(gt), "--vsd", "--vsd-delta", "0.02"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = _gt_line(r.stdout, "gt %s: " % obj)
    got = _gt_line(r.stdout, "gt %s vsd: " % obj)
    rec = _gt_line(r.stdout, "gt %s vsd recall: " % obj)
    # the same through the C ABI: model_search.ply as the driver read it, the frame it read, the two pose files as the driver reads them
    L = capi.load()
    n, hn = C.c_int(0), C.c_int(0)
    mp = str(repo / "models" / obj / "model_search.ply").encode()
    assert L.stocs_ply_read(mp, None, None, 0, C.byref(n), C.byref(hn)) == 0
    mpos, mnrm = np.zeros((n.value, 3), F), np.zeros((n.value, 3), F)
    assert L.stocs_ply_read(mp, mpos.ctypes.data_as(capi._fp), mnrm.ctypes.data_as(capi._fp), n.value, C.byref(n), C.byref(hn)) == 0
    est = _estimator(mpos, mnrm)
    est.set_frame(raw["depth"].astype(np.uint16), None, K, scale)
    want = est.pose_errors_vsd(_read_pose(out), _read_pose(gt), delta=0.02)[0]          # taus None: BOP's, from the diameter
    d = est.model_diameter()
    est.close()
    assert got["taus"] == 10 and got["valid"] == 1 and F(got["delta"]) == F(0.02) and F(got["surfel_radius"]) == F(0.006) and F(plain["diameter"]) == d
    for t in range(10):
        assert F(got["e%d" % t]) == want["e"][t], (t, got, want)
    for k in ("px_est", "px_gt", "vis_est", "vis_gt", "inter", "uni"):
        assert int(got[k]) == want[k], (k, got[k], want[k])
    assert want["uni"] > 1000 and abs(got["mean"] - float(np.mean(want["e"][:10].astype(np.float64)))) < 1e-8
    assert want["e"][9] <= want["e"][0] < 1.0                                            # a near miss: not all wrong, and no worse under a looser tau
    # the recall line against pose_recall_vsd on the records of the same four winners, which the driver prints one per line
    w = np.zeros(4, _VSD_DTYPE)
    for t in range(4):
        line = _gt_line(r.stdout, "gt %s vsd trial %d: " % (obj, t))
        w["valid"][t] = int(line["valid"])
        for k in range(10):
            w["e"][t][k] = F(line["e%d" % k])
    ar, nv = pose_recall_vsd(w)
    assert rec["trials"] == 4 and rec["valid"] == nv and abs(rec["vsd"] - ar) < 1e-8, (rec, ar, nv)


def test_python_path_on_the_ycb_fixture():
    """the 472-point model on its own depth image: the winner of a trial batch as the ground truth, against itself, pushed along z either
    way and turned a little; BOP's taus from the model's diameter"""
    from model_matching_amd.estimator import StocsEstimator, pose_recall_vsd
    d = np.load(os.path.join(GOLD, "example_ycb_024_bowl.npz"))
    raw = np.load(os.path.join(GOLD, "example_ycb_024_bowl_raw.npz"))
    K, scale = [float(x) for x in raw["K"]], float(raw["depth_scale"])
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
    est.set_frame(raw["depth"], raw["prob"], K, scale)
    res = est.run_trials(list(range(7, 11)), 100, max_per_base=200)
    win = max(res, key=lambda r: r["best_lcp"])["best_pose"].astype(F).reshape(16)
    T = win.reshape(4, 4).T.astype(np.float64)
    turn = np.eye(4); turn[:3, :3] = vc.rot((0, 0, 1), 10)
    E = np.stack([win, vc.pose16(vc.translation(0, 0, 0.03) @ T), vc.pose16(vc.translation(0, 0, -0.03) @ T), vc.pose16(turn @ T), np.zeros(16, F)])
    got = est.pose_errors_vsd(E, win)
    dia = F(est.model_diameter())
    taus = [F(0.05 * i) * dia for i in range(1, 11)]
    z = est.render_depth(E[:2])
    est.close()
    H, W = raw["depth"].shape
    want = ref.pose_errors_vsd(E, win, d["model_pos"], d["model_nrm"], raw["depth"], K, scale, taus)
    bad = [i for i in range(len(E)) if not ref.records_equal(got[i], want[i])]
    assert not bad, (bad, got[bad[0]], want[bad[0]])
    wz = ref.render_depth(E[:2], d["model_pos"], d["model_nrm"], K, W, H)
    assert np.array_equal(z.view(np.uint32), wz.view(np.uint32)) and (z[0] > 0).sum() > 1000
    assert np.all(got["e"][0] == 0) and got["uni"][0] > 1000 and got["valid"].tolist() == [1, 1, 1, 1, 0] and np.all(got["e"][4][:10] == 1)
    ar, nv = pose_recall_vsd(got)
    assert nv == 4 and abs(ar - ref.pose_recall_vsd(got)) < 1e-12 and 0.19 < ar < 0.81      # the first is right everywhere, the last wrong everywhere
