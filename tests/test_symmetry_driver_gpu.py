"""The layers above the symmetry C ABI that only a program reaches: model_preprocess --find-symmetry (stocs::find_model_symmetries), whose
symmetry.txt must be exactly what stocs_single --sym-file reads, and the facade's own methods (tests/cpp/symmetry_facade_check.cpp, built
here against the library).  The tool prints floats with nine significant digits, which name a float32 uniquely, so the file is compared
with the C ABI's set for equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_pose_error_gpu import APP, PRE, _gt_line, _write_example_tree  # noqa: E402
from test_pose_error_sym_driver_gpu import _read_pose  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def test_model_preprocess_finds_the_bowls_axis_and_the_driver_reads_its_file(tmp_path):
    from model_matching_amd import capi
    from model_matching_amd.estimator import StocsEstimator
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    K = [float(x) for x in raw["K"]]
    tol = 0.008
    pre = subprocess.run([PRE, obj, "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                          "--model-scale", repr(float(raw["model_scale"])), "--find-symmetry", "--sym-tol", repr(tol), "--sym-steps", "36", "--voxel"],
                         capture_output=True, text=True, timeout=300)   # (a last option without its value is ignored, as it always was)
    assert pre.returncode == 0 and "After sampling |M|=" in pre.stdout, pre.stdout + pre.stderr
    mdir = repo / "models" / obj
    assert (mdir / "model_search.ply").exists() and (mdir / "ppf_map").exists() and (mdir / "symmetry.txt").exists()
    # the same search through the C ABI on model_search.ply as written
    L = capi.load()
    n, hn = C.c_int(0), C.c_int(0)
    mp = str(mdir / "model_search.ply").encode()
    assert L.stocs_ply_read(mp, None, None, 0, C.byref(n), C.byref(hn)) == 0
    mpos, mnrm = np.zeros((n.value, 3), F), np.zeros((n.value, 3), F)
    assert L.stocs_ply_read(mp, mpos.ctypes.data_as(capi._fp), mnrm.ctypes.data_as(capi._fp), n.value, C.byref(n), C.byref(hn)) == 0
    sp = np.array([[0.0, 0.0, 1.0]], F)
    est = StocsEstimator(sp, -sp, np.ones(1, F), None, mpos, mnrm, build_index=False)
    axes, S, sym3, flags = est.find_symmetries(tol_max=tol, n_continuous=36)
    assert len(axes) == 1 and axes[0]["order"] == 0 and abs(axes[0]["axis"][2]) > 0.99 and len(S) == 36 and flags == 0   # the bowl: continuous about z
    assert np.array_equal(sym3, np.array([0, 0, 360], F))
    text = np.array((mdir / "symmetry.txt").read_text().split(), np.float64).astype(F).reshape(-1, 16)
    assert text.shape == S.shape and text.tobytes() == S.tobytes()
    lines = pre.stdout.splitlines()
    assert "symmetry axes: 1" in lines and any(l.startswith("symmetry set: 36 transforms -> ") for l in lines)
    line = [l for l in lines if l.startswith("symmetry axis 0: ")][0]
    kv = dict(x.split("=") for x in line[len("symmetry axis 0: "):].split())
    assert int(kv["order"]) == 0 and int(kv["n_normal_bad"]) == axes[0]["n_normal_bad"]
    assert np.allclose([float(x) for x in kv["axis"].split(",")], axes[0]["axis"], atol=1e-6) and abs(float(kv["max"]) - axes[0]["max"]) < 1e-6
    use = [l for l in lines if l.startswith("use: --sym ")][0].split()
    assert use[2] == "0,0,360" and use[3] == "--sym-file" and use[4] == str(mdir / "symmetry.txt")
    # the driver takes the descriptor and the file as printed
    base = [APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(float(raw["depth_scale"])), "--seed", "7"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = scene / ("best_pose_candidate_%s.txt" % obj)
    own = _read_pose(out).astype(np.float64).reshape(4, 4).T
    turned = own @ S[13].reshape(4, 4).T.astype(np.float64)     # the run's own pose under the set's 14th transform: 130 degrees about the axis
    gt = tmp_path / "gt.txt"
    gt.write_text("\n".join(" ".join("%.9g" % F(x) for x in row) for row in turned[:3]) + "\n")
    r = subprocess.run(base + ["--gt", str(gt), "--sym", use[2], "--sym-file", use[4]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _gt_line(r.stdout, "gt %s sym: " % obj)
    plain = _gt_line(r.stdout, "gt %s: " % obj)
    want = est.pose_errors_sym(_read_pose(out), _read_pose(gt), S, (K[0], K[1], K[2], K[3]))[0]
    d = est.model_diameter()
    est.close()
    assert got["symmetries"] == 36 and got["valid"] == 1
    assert F(got["mssd"]) == want["mssd"] and F(got["add"]) == want["add"] and int(got["k_mssd"]) == want["k_mssd"]
    assert got["mssd"] < 1e-4 < 0.1 * d < plain["add_max"]      # the turn is the set's own: nothing remains under it


def test_the_facades_symmetry_methods(tmp_path):
    exe = tmp_path / "symmetry_facade_check"
    lib = os.path.join(ROOT, "model_matching_amd")
    r = subprocess.run(["g++", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "symmetry_facade_check.cpp"), "-O2", "-std=c++11", "-pthread", "-Wall", "-Werror",
                        "-I", os.path.join(ROOT, "include"), "-L", lib, "-lstocs_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "axes=1 order=4 K=4 sym3=0,0,90 flags=0"
