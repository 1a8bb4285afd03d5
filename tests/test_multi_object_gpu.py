"""Several objects of one frame (stocs_ingest_scene_multi, estimator.ingest_scene_multi / estimate_objects, stocs_single a,b,c):
one ingest for the frame, per object bitwise what the single-object path gives."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
APP = os.path.join(ROOT, "model_matching_amd", "apps", "stocs_single")
PRE = os.path.join(ROOT, "model_matching_amd", "apps", "model_preprocess")
NAMES = ["ycb_024_bowl", "linemod_obj_06", "packed_dove"]


def _raw(name):
    return np.load(os.path.join(GOLD, "example_%s_raw.npz" % name))


def _map_set(prob):
    """(map, threshold) pairs: own, rolled by 37 columns, complement, all 10000, all 0 (empty), all 999 (below 0.10: empty), own at 0.5"""
    p = np.asarray(prob, np.uint16)
    return [(p, 0.10), (np.roll(p, 37, axis=1), 0.10), (10000 - p, 0.10), (np.full_like(p, 10000), 0.10), (np.zeros_like(p), 0.10),
            (np.full_like(p, 999), 0.10), (p, 0.5)]


def _call(depth, maps, thr, K, ds, nm=0, cap=None, n_objects=None):
    """the raw entry point -> (rc, offsets, pos, nrm, prob, pixel)"""
    from model_matching_amd import capi
    L = capi.load()
    d = np.ascontiguousarray(depth, np.uint16)
    H, W = d.shape
    p = np.ascontiguousarray(np.stack(maps), np.uint16)
    t = np.ascontiguousarray(thr, np.float32)
    n = len(maps) if n_objects is None else n_objects
    cap = len(maps) * W * H if cap is None else cap
    cam = capi.Camera(K[0], K[1], K[2], K[3], ds, W, H, nm)
    off = np.full(max(n, 0) + 1, -7, np.int32)
    pos = np.zeros((max(cap, 1), 3), np.float32); nrm = np.zeros((max(cap, 1), 3), np.float32)
    pr = np.zeros(max(cap, 1), np.float32); px = np.zeros((max(cap, 1), 2), np.int32)
    rc = L.stocs_ingest_scene_multi(C.byref(cam), d.ctypes.data_as(C.POINTER(C.c_uint16)), n, p.ctypes.data_as(C.POINTER(C.c_uint16)), t.ctypes.data_as(capi._fp),
                                    0.005, -1, pos.ctypes.data_as(capi._fp), nrm.ctypes.data_as(capi._fp), pr.ctypes.data_as(capi._fp),
                                    px.ctypes.data_as(capi._ip), cap, off.ctypes.data_as(capi._ip))
    return rc, off, pos, nrm, pr, px


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("normal_method", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_equals_one_single_call_per_object(name, normal_method):
    from model_matching_amd.estimator import ingest_scene, ingest_scene_multi
    raw = _raw(name)
    K, ds, depth = [float(x) for x in raw["K"]], float(raw["depth_scale"]), np.ascontiguousarray(raw["depth"])
    ms = _map_set(raw["prob"])
    got = ingest_scene_multi(depth, [m for m, _ in ms], K, ds, class_thresholds=[t for _, t in ms], normal_method=normal_method)
    rc, off, *_ = _call(depth, [m for m, _ in ms], [t for _, t in ms], K, ds, normal_method)
    assert rc == 0 and off[0] == 0 and (np.diff(off) >= 0).all()
    assert len(got) == len(ms)
    for k, (m, t) in enumerate(ms):
        ref = ingest_scene(depth, m, K, ds, 0.005, t, normal_method=normal_method)
        assert len(got[k][0]) == len(ref[0]) == off[k + 1] - off[k], (k, len(got[k][0]), len(ref[0]))
        assert _same(got[k], ref), k
    assert len(got[0][0]) > 1000 and len(got[4][0]) == 0 and len(got[5][0]) == 0 and len(got[3][0]) >= len(got[0][0])


def test_capacity_arguments_and_order():
    from model_matching_amd import capi
    from model_matching_amd.estimator import ingest_scene
    raw = _raw("ycb_024_bowl")
    K, ds, depth, prob = [float(x) for x in raw["K"]], float(raw["depth_scale"]), np.ascontiguousarray(raw["depth"]), np.ascontiguousarray(raw["prob"])
    maps = [prob, np.roll(prob, 37, axis=1), 10000 - prob]
    thr = [0.1, 0.1, 0.3]
    rc, off, pos, nrm, pr, px = _call(depth, maps, thr, K, ds)
    assert rc == 0
    total = int(off[-1])
    # too small a cap: offsets filled, nothing written; a retry at exactly the total gives the same clouds
    rc2, off2, pos2, *_ = _call(depth, maps, thr, K, ds, cap=total - 1)
    assert rc2 == capi.ERR_CAPACITY and np.array_equal(off2, off) and not pos2.any()
    rc3, off3, pos3, nrm3, pr3, px3 = _call(depth, maps, thr, K, ds, cap=total)
    assert rc3 == 0 and np.array_equal(off3, off)
    assert _same((pos3, nrm3, pr3, px3), (pos[:total], nrm[:total], pr[:total], px[:total]))
    # arguments
    assert _call(depth, maps, thr, K, ds, n_objects=0)[0] == capi.ERR_INVALID
    L = capi.load()
    cam = capi.Camera(K[0], K[1], K[2], K[3], ds, depth.shape[1], depth.shape[0], 0)
    p65 = np.zeros((65,) + depth.shape, np.uint16); t65 = np.full(65, 0.1, np.float32); o = np.zeros(66, np.int32)
    u16 = C.POINTER(C.c_uint16)
    assert L.stocs_ingest_scene_multi(C.byref(cam), depth.ctypes.data_as(u16), 65, p65.ctypes.data_as(u16), t65.ctypes.data_as(capi._fp), 0.005, -1,
                                      None, None, None, None, 0, o.ctypes.data_as(capi._ip)) == capi.ERR_INVALID
    assert L.stocs_ingest_scene_multi(C.byref(cam), None, 2, p65.ctypes.data_as(u16), t65.ctypes.data_as(capi._fp), 0.005, -1,
                                      None, None, None, None, 0, o.ctypes.data_as(capi._ip)) == capi.ERR_INVALID
    assert L.stocs_ingest_scene_multi(C.byref(cam), depth.ctypes.data_as(u16), 2, None, t65.ctypes.data_as(capi._fp), 0.005, -1,
                                      None, None, None, None, 0, o.ctypes.data_as(capi._ip)) == capi.ERR_INVALID
    assert _call(depth, maps, [0.1, float("nan"), 0.1], K, ds)[0] == capi.ERR_INVALID
    # one object = the single call
    rc1, off1, p1, n1, r1, x1 = _call(depth, [prob], [0.1], K, ds)
    ref = ingest_scene(depth, prob, K, ds, 0.005, 0.1)
    assert rc1 == 0 and off1[1] == len(ref[0]) and _same((p1[:off1[1]], n1[:off1[1]], r1[:off1[1]], x1[:off1[1]]), ref)
    # reversed object order: the clouds are permuted, nothing else changes
    rcr, offr, posr, nrmr, prr, pxr = _call(depth, maps[::-1], thr[::-1], K, ds)
    assert rcr == 0 and offr[-1] == total
    for k in range(3):
        j = 2 - k
        a, b = slice(off[k], off[k + 1]), slice(offr[j], offr[j + 1])
        assert _same((pos[a], nrm[a], pr[a], px[a]), (posr[b], nrmr[b], prr[b], pxr[b])), k


def _frame_objects():
    """three models on the ycb frame, each with its own map: the bowl (own map), obj_06 and dove (derived maps)"""
    from model_matching_amd.estimator import preprocess_model
    raw = _raw("ycb_024_bowl")
    prob = np.ascontiguousarray(raw["prob"])
    maps = [prob, np.roll(prob, 37, axis=1), np.roll(prob, -60, axis=0)]
    models = []
    for name in NAMES:
        r = _raw(name)
        models.append(preprocess_model(r["model_raw"], float(r["normal_radius"]), float(r["model_voxel"]), float(r["model_scale"])))
    return raw, maps, models


def test_concurrent_objects_equal_each_object_alone():
    from model_matching_amd.estimator import StocsEstimator, estimate_objects, ingest_scene, ingest_scene_multi
    raw, maps, models = _frame_objects()
    K, ds, depth = [float(x) for x in raw["K"]], float(raw["depth_scale"]), np.ascontiguousarray(raw["depth"])
    scenes = ingest_scene_multi(depth, maps, K, ds)
    one = estimate_objects(scenes, models, 11)
    many = estimate_objects(scenes, models, [3, 4, 5, 6])
    for k in range(3):
        alone = ingest_scene(depth, maps[k], K, ds)
        assert _same(alone, scenes[k])
        est = StocsEstimator(*alone, *models[k], build_index=True)
        est.sample_bases(11, 100, mode=0, dispersion=0.9)
        est.find_congruent_all(); est.make_transforms(200, 11)
        lcp, idx, pose = est.compute_best_transform()
        assert (one[k][0], one[k][1], one[k][2].tobytes()) == (float(lcp), int(idx), pose.tobytes()), k
        res = est.run_trials([3, 4, 5, 6], 100, mode=0, dispersion=0.9)
        est.close()
        assert len(many[k]) == 4
        for a, b in zip(many[k], res):
            assert (a["best_lcp"], a["best_index"], a["best_pose"].tobytes()) == (b["best_lcp"], b["best_index"], b["best_pose"].tobytes()), k
    assert one[0][0] > 0.1   # the bowl on its own map is found


def _png16(path, a):
    from PIL import Image
    Image.fromarray(np.asarray(a).astype(np.uint16)).save(path)


def _write_tree(tmp_path, frame, objects):
    """the reference's layout: <scene>/{depth.png, probability_maps/<obj>.png[, edge.png]}, <repo>/models/<obj>/ model_search.ply + ppf_map
    (by model_preprocess from the fixtures' raw vertices).  objects: [(object name, fixture name of its model, probability map)]"""
    from PIL import Image
    raw = _raw(frame)
    fix = np.load(os.path.join(GOLD, "example_%s.npz" % frame))
    scene = tmp_path / "scene"; (scene / "probability_maps").mkdir(parents=True)
    _png16(scene / "depth.png", raw["depth"])
    if "edge_map" in fix.files:
        Image.fromarray(fix["edge_map"].astype(np.uint8)).save(scene / "probability_maps" / "edge.png")
    repo = tmp_path / "repo"
    for obj, model_name, pmap in objects:
        _png16(scene / "probability_maps" / (obj + ".png"), pmap)
        r = _raw(model_name)
        mdir = repo / "models" / obj; mdir.mkdir(parents=True)
        v = r["model_raw"]
        with open(mdir / "textured_vertices.ply", "w") as f:
            f.write("ply\nformat ascii 1.0\ncomment VCGLIB generated\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                    "element face 0\nproperty list uchar int vertex_indices\nend_header\n" % len(v))
            for p in v:
                f.write("%.9g %.9g %.9g \n" % (p[0], p[1], p[2]))
        pre = subprocess.run([PRE, obj, "--repo", str(repo), "--voxel", repr(float(r["model_voxel"])), "--normal-radius", repr(float(r["normal_radius"])),
                              "--model-scale", repr(float(r["model_scale"]))], capture_output=True, text=True, timeout=300)
        assert pre.returncode == 0, pre.stdout + pre.stderr
    common = ["--repo", str(repo), "--intrinsics", ",".join(repr(float(k)) for k in raw["K"]), "--depth-scale", repr(float(raw["depth_scale"]))]
    return scene, repo, common


def _driver_matches_single_runs(scene, objects, common, extra):
    names = [o for o, _, _ in objects]
    r = subprocess.run([APP, str(scene), ",".join(names)] + common + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    heads = [r.stdout.index("Object: %s ####" % o) for o in names]
    assert heads == sorted(heads)                                    # blocks in the order given
    got = {}
    for o in names:
        f = scene / ("best_pose_candidate_%s.txt" % o)
        got[o] = f.read_bytes()
        f.unlink()
    for o in names:
        s = subprocess.run([APP, str(scene), o] + common + extra, capture_output=True, text=True, timeout=600)
        assert s.returncode == 0, s.stdout + s.stderr
        assert (scene / ("best_pose_candidate_%s.txt" % o)).read_bytes() == got[o], o
        summ = [l for l in s.stdout.splitlines() if l.startswith("summary:") or l.startswith("trials:")][-1]
        assert summ.split("microseconds=")[0] in r.stdout, o       # the same counts / scores, in that object's block
    return r


def test_driver_several_objects_equal_single_runs(tmp_path):
    raw = _raw("ycb_024_bowl")
    prob = np.asarray(raw["prob"])
    objects = [("024_bowl", "ycb_024_bowl", prob), ("obj_06", "linemod_obj_06", np.roll(prob, 37, axis=1)), ("dove", "packed_dove", np.roll(prob, -60, axis=0))]
    scene, repo, common = _write_tree(tmp_path, "ycb_024_bowl", objects)
    _driver_matches_single_runs(scene, objects, common, ["--seed", "7"])
    _driver_matches_single_runs(scene, objects, common, ["--seed", "7", "--trials", "4"])
    # refused with a list: the single-object options
    r = subprocess.run([APP, str(scene), "024_bowl,obj_06", "--cluster", "1"] + common, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--cluster" in r.stderr
    # a missing probability map or index: non-zero before any work, the object named, no pose file
    # (ghost: map and model there, its ppf_map not)
    (scene / "probability_maps" / "ghost.png").write_bytes((scene / "probability_maps" / "obj_06.png").read_bytes())
    (repo / "models" / "ghost").mkdir()
    (repo / "models" / "ghost" / "model_search.ply").write_bytes((repo / "models" / "obj_06" / "model_search.ply").read_bytes())
    for f in scene.glob("best_pose_candidate_*.txt"):
        f.unlink()
    for bad in ("missing_obj", "ghost"):
        r = subprocess.run([APP, str(scene), "024_bowl,%s,obj_06" % bad] + common + ["--seed", "7"], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and bad in r.stderr, r.stdout + r.stderr
        assert not list(scene.glob("best_pose_candidate_*.txt"))


def test_driver_instance_mode_on_the_packed_frame(tmp_path):
    raw = _raw("packed_dove")
    prob = np.asarray(raw["prob"])
    objects = [("dove", "packed_dove", prob), ("obj_06", "linemod_obj_06", np.roll(prob, 37, axis=1))]
    scene, repo, common = _write_tree(tmp_path, "packed_dove", objects)
    assert (scene / "probability_maps" / "edge.png").exists()
    _driver_matches_single_runs(scene, objects, common, ["--seed", "5"])
