"""stocs_pose_errors / stocs_pose_errors_detail / stocs_model_diameter on the GPU against the float32 restatement of their contract
(tests/pose_error_ref.py): every comparison is bit equality on every field.  The model sizes are those of the issue plus one below, at
and one above every size include/stocs_hip.h names for the kernel (threads, chunk, tile) and every row count of a chunk
(tests/pose_error_cases.py::model_sizes).  The context accepts a one-point model, so the list starts at 1.  The scene plays no part (a
handful of points serves)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pose_error_cases as cases  # noqa: E402
import pose_error_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
APP = os.path.join(ROOT, "model_matching_amd", "apps", "stocs_single")
PRE = os.path.join(ROOT, "model_matching_amd", "apps", "model_preprocess")
F = np.float32


def _est(model_pos):
    from model_matching_amd.estimator import StocsEstimator
    m = np.asarray(model_pos, F).reshape(-1, 3)
    rng = np.random.default_rng(1)
    sp = rng.normal(0, 0.05, (32, 3)).astype(F)
    sn = sp / np.linalg.norm(sp, axis=1, keepdims=True)
    nrm = np.tile(np.array([0, 0, 1], F), (len(m), 1))
    return StocsEstimator(sp, sn, np.ones(32, F), None, m, nrm, build_index=False)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = [i for i in range(len(got)) if not ref.records_equal(got[i], want[i])]
    assert not bad, (bad[:5], got[bad[:5]], want[bad[:5]])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    d = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
    assert d.size == 0, (d[:5], a[d[:5]], b[d[:5]])


def _check(est, model, e, g):
    """records, for the first pair the detail, and the model's diameter against the restatement -> the records"""
    e, g = np.asarray(e, F).reshape(-1, 16), np.asarray(g, F).reshape(-1, 16)
    assert est.model_diameter().tobytes() == ref.diameter(model).tobytes()
    got = est.pose_errors(e, g)
    _same(got, ref.records(e, g, model))
    de, ds, dn = est.pose_errors_detail(e[0], g[0])
    we, ws, wn = ref.detail(e[0], g[0], model)
    _same_bits(de, we); _same_bits(ds, ws); _same_bits(dn, wn)
    assert np.all(ds.view(np.uint32) <= de.view(np.uint32))    # s_i <= e_i bit for bit
    return got


@pytest.mark.parametrize("M", cases.model_sizes())
def test_every_model_size(M):
    model = cases.random_model(M)
    est = _est(model)
    e, g = cases.random_pairs(3, M)
    _check(est, model, e, g)
    e2, g2 = cases.random_pairs(2, M + 7, near=True)
    _check(est, model, e2, g2[:1])
    assert est.model_diameter().tobytes() == ref.diameter(model).tobytes()
    assert est.model_diameter().tobytes() == ref.diameter(model).tobytes()     # the cached value
    if M == 1:
        assert est.model_diameter() == 0
    est.close()


@pytest.fixture(scope="module")
def batch():
    """one model across a chunk edge, 65 pairs, their restated records computed once"""
    model = cases.random_model(1025, seed=2)
    e, g = cases.random_pairs(65, 77)
    e[40:], g[40:] = cases.random_pairs(25, 78, near=True)
    est = _est(model)
    yield dict(model=model, est=est, e=e, g=g, each=ref.records(e, g, model), one=ref.records(e, g[:1], model))
    est.close()


@pytest.mark.parametrize("n", [1, 2, 65])
def test_batches_with_one_and_with_n_ground_truths(batch, n):
    b = batch
    _same(b["est"].pose_errors(b["e"][:n], b["g"][:n]), b["each"][:n])
    _same(b["est"].pose_errors(b["e"][:n], b["g"][:1]), b["one"][:n])


def test_a_record_does_not_depend_on_its_batch(batch):
    b = batch
    whole = b["est"].pose_errors(b["e"], b["g"])
    rev = b["est"].pose_errors(b["e"][::-1], b["g"][::-1])
    _same(rev[::-1].copy(), whole)
    for k in (0, 31, 64):
        _same(b["est"].pose_errors(b["e"][k], b["g"][k]), whole[k:k + 1])
    _same(whole, b["each"])
    assert b["est"].model_diameter().tobytes() == ref.diameter(b["model"]).tobytes()


def test_more_pairs_than_one_launch_holds():
    """65 537 pairs on a two-point model: the second launch's pairs land in their own records"""
    model = cases.random_model(2)
    est = _est(model)
    e, g = cases.random_pairs(16, 5)
    n = 65537
    E = np.tile(e, (n // 16 + 1, 1))[:n]
    got = est.pose_errors(E, g[:1])
    want = ref.records(e, g[:1], model)
    _same(got[:16], want); _same(got[65520:65536], want); _same(got[65536:], want[:1])
    est.close()


def test_identical_poses_give_exact_zeros(batch):
    got = batch["est"].pose_errors(batch["e"][:5], batch["e"][:5])
    for k in ("add_fix", "adds_fix", "add", "add_max", "adds", "adds_max", "reserved"):
        assert np.all(got[k] == 0), k
    assert np.all(got["valid"] == 1)
    e, s, nn = batch["est"].pose_errors_detail(batch["e"][0], batch["e"][0])
    assert np.all(e == 0) and np.all(s == 0) and np.all((nn >= 0) & (nn <= np.arange(len(nn))))


def test_pure_translation():
    model = cases.lattice(4, 2.0 ** -6)
    est = _est(model)
    got = _check(est, model, cases.pose(None, (0.125, 0, 0.5)), cases.pose(None, (0, 0, 0.5)))[0]
    assert got["add"] == F(0.125) and got["add_max"] == F(0.125) and got["add_fix"] == len(model) * (1 << 29)
    est.close()


def test_symmetric_models_turned_by_a_symmetry():
    c = cases.lattice_quarter_turn()
    est = _est(c["model"])
    got = _check(est, c["model"], c["est"], c["gt"])[0]
    _, s, nn = est.pose_errors_detail(c["est"][0], c["gt"][0])
    assert got["add"] > 0.03 and got["adds_fix"] == 0 and got["adds"] == 0 and np.all(s == 0) and np.array_equal(nn, c["perm"])
    est.close()
    c = cases.ring_turn()
    est = _est(c["model"])
    got = _check(est, c["model"], c["est"], c["gt"])[0]
    _, s, nn = est.pose_errors_detail(c["est"][0], c["gt"][0])
    assert got["add"] > 0.25 * c["radius"] and got["adds_max"] <= 8 * 2.0 ** -24 * c["radius"] and np.array_equal(nn, c["perm"])
    est.close()


def test_exact_ties_go_to_the_lowest_index():
    c = cases.duplicate_points()
    est = _est(c["model"])
    _check(est, c["model"], c["est"], c["gt"])
    assert np.all(est.pose_errors_detail(c["est"][0], c["gt"][0])[2] < len(c["model"]) // 2)
    est.close()
    for ways in (2, 4, 8):
        c = cases.lattice_midpoints(ways)
        est = _est(c["model"])
        _check(est, c["model"], c["est"], c["gt"])
        est.close()


def test_units_and_offsets():
    for c in (cases.millimetres(), cases.far_from_origin()):
        est = _est(c["model"])
        _check(est, c["model"], c["est"], c["gt"])
        assert est.model_diameter().tobytes() == ref.diameter(c["model"]).tobytes()
        est.close()


def test_nan_model_point():
    c = cases.nan_point()
    est = _est(c["model"])
    got = _check(est, c["model"], c["est"], c["gt"])[0]
    e, s, nn = est.pose_errors_detail(c["est"][0], c["gt"][0])
    at = c["at"]
    assert np.isposinf(e[at]) and np.isposinf(s[at]) and nn[at] == -1 and np.all(np.delete(nn, at) != at) and np.all(np.delete(nn, at) >= 0)
    assert got["valid"] == 1 and np.isposinf(got["add_max"]) and np.isposinf(got["adds_max"])
    assert np.isposinf(est.model_diameter()) and np.isposinf(ref.diameter(c["model"]))
    est.close()


def test_extreme_poses():
    c = cases.far_apart()
    est = _est(c["model"])
    got = _check(est, c["model"], c["est"], c["gt"])[0]
    assert got["add"] == F(32768) and got["adds"] == F(32768) and got["add_fix"] == len(c["model"]) * (1 << 47) and got["add_max"] > 0.9e6
    est.close()
    c2 = cases.overflow()
    est = _est(c2["model"])
    got = _check(est, c2["model"], c2["est"], c2["gt"])
    assert np.all(got["valid"] == 1) and np.all(np.isposinf(got["add_max"])) and np.all(np.isposinf(got["adds_max"]))
    est.close()


def test_invalid_poses():
    c = cases.invalid_poses()
    est = _est(c["model"])
    assert est.model_diameter().tobytes() == ref.diameter(c["model"]).tobytes()
    got = est.pose_errors(c["est"], c["gt"])
    _same(got, ref.records(c["est"], c["gt"], c["model"]))
    assert np.array_equal(got["valid"], c["valid"])
    bad = got[c["valid"] == 0]
    assert np.all(bad["add_fix"] == 0) and np.all(bad["adds_fix"] == 0)
    for k in ("add", "add_max", "adds", "adds_max"):
        assert np.all(np.isposinf(bad[k])), k
    # the same pairs against ONE ground truth that is itself invalid: every record is
    g = c["gt"][1:2]
    got = est.pose_errors(c["est"], g)
    _same(got, ref.records(c["est"], g, c["model"]))
    assert np.all(got["valid"] == 0)
    est.close()


def test_diameter_tie():
    c = cases.diameter_tie()
    est = _est(c["model"])
    assert est.model_diameter() == np.sqrt(c["d2"]) and est.model_diameter().tobytes() == ref.diameter(c["model"]).tobytes()
    est.close()


def test_second_call_allocates_nothing(batch):
    from model_matching_amd import capi
    L = capi.load()
    b = batch
    b["est"].pose_errors(b["e"], b["g"]); b["est"].pose_errors_detail(b["e"][0], b["g"][0]); b["est"].model_diameter()
    before = L.stocs_device_alloc_count()
    b["est"].pose_errors(b["e"], b["g"])
    b["est"].pose_errors(b["e"][:7], b["g"][:1])
    b["est"].pose_errors_detail(b["e"][1], b["g"][1])
    b["est"].model_diameter()
    assert L.stocs_device_alloc_count() == before


def test_call_timing_names_the_steps_and_the_kernel(batch):
    """stocs_last_call_timing(4): the host steps of the last pose_errors, and with the device_clock option the launches' HIP-event time"""
    b = batch
    steps = ["stage and enqueue", "wait for the device", "records"]
    b["est"].set_option("device_clock", 0)
    b["est"].pose_errors(b["e"], b["g"])
    t = b["est"].last_call_timing(4)
    assert [k for k, _ in t] == steps and all(ms >= 0 for _, ms in t)
    b["est"].set_option("device_clock", 1)
    got = b["est"].pose_errors(b["e"], b["g"])
    t = b["est"].last_call_timing(4)
    b["est"].set_option("device_clock", 0)
    assert [k for k, _ in t] == steps + ["device: kernel"] and all(ms >= 0 for _, ms in t) and dict(t)["device: kernel"] > 0
    _same(got, b["each"])                                                  # the events change no record


def test_invalid_arguments(batch):
    from model_matching_amd import capi
    L = capi.load()
    h = batch["est"].h
    P = np.ascontiguousarray(batch["e"][:4]); G = np.ascontiguousarray(batch["g"][:4])
    pP, pG = P.ctypes.data_as(capi._fp), G.ctypes.data_as(capi._fp)
    out = (capi.PoseError * 4)()
    d = C.c_float()
    assert L.stocs_pose_errors(h, pP, 4, pG, 4, out) == 0 and L.stocs_pose_errors(h, pP, 4, pG, 1, out) == 0
    assert L.stocs_pose_errors(h, None, 0, None, 0, None) == 0            # n == 0: a no-op
    for n_gt in (0, 2, 3, 5, -1):
        assert L.stocs_pose_errors(h, pP, 4, pG, n_gt, out) == -1, n_gt
    assert L.stocs_pose_errors(h, pP, -1, pG, 1, out) == -1
    assert L.stocs_pose_errors(h, None, 4, pG, 1, out) == -1
    assert L.stocs_pose_errors(h, pP, 4, None, 1, out) == -1
    assert L.stocs_pose_errors(h, pP, 4, pG, 1, None) == -1
    assert L.stocs_pose_errors(None, pP, 4, pG, 1, out) == -1
    assert L.stocs_pose_errors_detail(h, None, pG, None, None, None) == -1 and L.stocs_pose_errors_detail(h, pP, None, None, None, None) == -1
    assert L.stocs_pose_errors_detail(h, pP, pG, None, None, None) == 0    # every output may be NULL
    assert L.stocs_model_diameter(h, None) == -1 and L.stocs_model_diameter(h, C.byref(d)) == 0


def test_trial_winners_on_tiny():
    """the winners of a four-trial batch against T_gt: the library's records equal the restatement, and the recall helper counts them"""
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator, pose_recall
    model, scene, _ = synth.workload("tiny")
    est = StocsEstimator(scene.pos, scene.nrm, scene.prob, scene.pixel, model.pos, model.nrm, build_index=True)
    res = est.run_trials([11, 12, 13, 14])
    W = np.stack([r["best_pose"] for r in res]).astype(F)
    gt = scene.T_gt.T.reshape(16).astype(F)
    got = est.pose_errors(W, gt)
    _same(got, ref.records(W, gt, model.pos))
    d = est.model_diameter()
    assert d.tobytes() == ref.diameter(model.pos).tobytes()
    ra, rs, nv = pose_recall(got, d)
    assert nv == int((got["valid"] == 1).sum()) and 0 <= ra <= rs <= 1
    assert nv >= 1 and got["adds"][got["valid"] == 1].min() < 0.1 * d      # some trial finds the object on this workload
    est.close()


def _write_example_tree(tmp_path, name):
    """the reference's directory layout rebuilt from the committed fixtures, as tests/test_driver_gpu.py builds it"""
    from PIL import Image
    raw = np.load(os.path.join(ROOT, "tests", "golden", "example_%s_raw.npz" % name))
    obj = name.split("_", 1)[1]
    scene = tmp_path / "scene"; (scene / "probability_maps").mkdir(parents=True)
    Image.fromarray(raw["depth"].astype(np.uint16)).save(scene / "depth.png")
    Image.fromarray(raw["prob"].astype(np.uint16)).save(scene / "probability_maps" / (obj + ".png"))
    mdir = tmp_path / "repo" / "models" / obj; mdir.mkdir(parents=True)
    v = raw["model_raw"]
    with open(mdir / "textured_vertices.ply", "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment VCGLIB generated\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face 0\nproperty list uchar int vertex_indices\nend_header\n" % len(v))
        for p in v:
            f.write("%.9g %.9g %.9g \n" % (p[0], p[1], p[2]))
    return raw, obj, scene, tmp_path / "repo"


def _gt_line(stdout, head):
    line = [l for l in stdout.splitlines() if l.startswith(head)][-1]
    return {k: float(v) for k, v in (kv.split("=") for kv in line[len(head):].split())}


def test_driver_scores_its_own_pose_file_as_zero(tmp_path):
    """stocs_single --trials 4 on the ycb example frame, then again with --gt set to the first run's own pose file: same seeds, same pose
    file, ADD = ADD-S = 0, and the recall line counts the four winners; a --gt file that cannot be read ends the run before any search"""
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    K = [float(x) for x in raw["K"]]
    pre = subprocess.run([PRE, obj, "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                          "--model-scale", repr(float(raw["model_scale"]))], capture_output=True, text=True, timeout=300)
    assert pre.returncode == 0, pre.stdout + pre.stderr
    base = [APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(float(raw["depth_scale"])), "--seed", "7", "--trials", "4"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not [l for l in r.stdout.splitlines() if l.startswith("gt ")], r.stdout + r.stderr
    gt = tmp_path / "gt.txt"
    gt.write_text((scene / ("best_pose_candidate_%s.txt" % obj)).read_text())
    r = subprocess.run(base + ["--gt", str(gt)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    g = _gt_line(r.stdout, "gt %s: " % obj)
    assert g["add"] == 0 and g["adds"] == 0 and g["add_max"] == 0 and g["adds_max"] == 0 and g["valid"] == 1 and g["adds_over_diameter"] == 0
    assert 0.05 < g["diameter"] < 0.5                                         # a bowl
    rc = _gt_line(r.stdout, "gt %s recall: " % obj)
    assert rc["trials"] == 4 and 0 <= rc["valid"] <= 4 and 0 <= rc["add"] <= rc["adds"] <= 1 and abs(rc["threshold"] - 0.1 * g["diameter"]) < 1e-6
    r = subprocess.run(base + ["--gt", str(tmp_path / "missing.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "cannot read a 3x4 pose" in r.stderr and "RUNNING STOCS" not in r.stdout
