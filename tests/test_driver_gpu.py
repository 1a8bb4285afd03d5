"""The C++ driver (model_matching_amd/apps/stocs_single, host code on the façade include/stocs.hpp)
end to end on the GPU: same phases / output file as the reference's stocs_single."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "model_matching_amd", "apps", "stocs_single")
PRE = os.path.join(ROOT, "model_matching_amd", "apps", "model_preprocess")
PERCALL = os.path.join(ROOT, "model_matching_amd", "apps", "stocs_single_percall")


def _parse(stdout):
    """summary line + full-precision pose line of apps/stocs_single"""
    summ = dict(kv.split("=") for kv in [l for l in stdout.splitlines() if l.startswith("summary:")][-1].split()[1:])
    pose = [l for l in stdout.splitlines() if l.startswith("pose:")]
    P = np.array(pose[-1].split()[1:], np.float64).reshape(3, 4) if pose else None
    return {k: (float(v) if k == "best_lcp" else int(v)) for k, v in summ.items()}, P


def _pose_close(P, pose16_colmajor, mm=1.0, deg=1.0):
    Q = np.asarray(pose16_colmajor, np.float64).reshape(4, 4).T[:3, :]
    dR = P[:, :3].T @ Q[:, :3]
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2))))
    return ang <= deg and np.linalg.norm(P[:, 3] - Q[:, 3]) * 1e3 <= mm


@pytest.mark.gpu
def test_stocs_single_equals_oracle_run_on_tiny(tmp_path, oracle_lib):
    """The C++ driver (batched entry points, the library's one subset rule) against orc.run -- the restatement of the
    reference caller run_stocs_estimation (stocs_match_one_object.cpp:79-185): same number of bases, congruent sets and
    candidates, best LCP within 1e-5, winning pose within 1 mm / 1 degree (identical candidate -> identical pose)."""
    from model_matching_amd import synth, cloudio
    m, s, k = synth.workload("tiny")
    cloudio.write_stcl(tmp_path / "scene.stcl", s.pos, s.nrm, s.prob, s.pixel)
    cloudio.write_stcl(tmp_path / "model.stcl", m.pos, m.nrm)
    out = tmp_path / "best_pose_candidate_obj.txt"
    seed = 1234
    r = subprocess.run([APP, "--clouds", str(tmp_path / "scene.stcl"), str(tmp_path / "model.stcl"), "--seed", str(seed), "--out", str(out),
                        "--dbg", str(tmp_path), "--cluster", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for needle in ("Sampled ", " bases in ", "found ", " congruent sets in ", "evaluated transforms in ", "microseconds", "Transforms to verify: ", "maximum score: "):
        assert needle in r.stdout
    assert "clustered hypotheses:" in r.stdout and "cluster 0: base" in r.stdout
    orc = oracle_lib.Oracle(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm)
    ro = orc.run(seed, 100, 200)
    summ, P = _parse(r.stdout)
    assert (summ["bases"], summ["congruent_sets"], summ["candidates"], summ["best_index"]) == (ro.n_bases, ro.n_quads_total, ro.n_candidates, ro.best_index)
    assert abs(summ["best_lcp"] - ro.best_lcp) <= 1e-5
    assert _pose_close(P, ro.best_pose16)
    # the pose file: 12 numbers, 3x4 row-major, default ostream precision (stocs_match_one_object.cpp:171-180)
    vals = np.array(out.read_text().split(), float)
    assert vals.shape == (12,) and np.allclose(vals.reshape(3, 4), P, rtol=2e-5, atol=2e-6)
    dR = P[:, :3].T @ s.T_gt[:3, :3]
    assert math.degrees(math.acos(min(1.0, (np.trace(dR) - 1) / 2))) < 3.0 and np.linalg.norm(P[:, 3] - s.T_gt[:3, 3]) < 0.005
    # visualize_best_pose (stocs.hpp:136-149): the model under the best transform and the scene
    ply = (tmp_path / "best_pose.ply").read_text().splitlines()
    assert ply[0] == "ply" and ("element vertex %d" % len(m.pos)) in ply[:5] and (tmp_path / "scene.ply").exists()
    # .stcl round trip
    pos, nrm, prob, pix = cloudio.read_stcl(tmp_path / "scene.stcl")
    assert np.array_equal(pos, s.pos) and np.array_equal(prob, s.prob) and np.array_equal(pix, s.pixel)


def _write_example_tree(tmp_path, name):
    """The reference's directory layout (examples/<set>/{depth.png, probability_maps/<obj>.png[, edge.png]} and
    models/<obj>/textured_vertices.ply) rebuilt from the committed DATA fixtures (tests/golden/example_<name>_raw.npz)."""
    from PIL import Image
    raw = np.load(os.path.join(ROOT, "tests", "golden", "example_%s_raw.npz" % name))
    fix = np.load(os.path.join(ROOT, "tests", "golden", "example_%s.npz" % name))
    obj = name.split("_", 1)[1]
    scene = tmp_path / "scene"; (scene / "probability_maps").mkdir(parents=True)
    Image.fromarray(raw["depth"].astype(np.uint16)).save(scene / "depth.png")
    Image.fromarray(raw["prob"].astype(np.uint16)).save(scene / "probability_maps" / (obj + ".png"))
    if "edge_map" in fix.files:
        Image.fromarray(fix["edge_map"].astype(np.uint8)).save(scene / "probability_maps" / "edge.png")
    mdir = tmp_path / "repo" / "models" / obj; mdir.mkdir(parents=True)
    v = raw["model_raw"]
    with open(mdir / "textured_vertices.ply", "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment VCGLIB generated\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face 0\nproperty list uchar int vertex_indices\nend_header\n" % len(v))
        for p in v:
            f.write("%.9g %.9g %.9g \n" % (p[0], p[1], p[2]))
    return raw, fix, obj, scene, tmp_path / "repo"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ycb_024_bowl", "linemod_obj_06", "packed_dove"])
def test_reference_command_line_on_the_example_data(name, tmp_path, oracle_lib):
    """model_preprocess <object> then stocs_single <scene_path> <object_name> -- the reference's two commands
    (README.md:42-60) on the reference's own example data, file formats and directory layout -- against orc.run on the
    clouds the tools themselves produce (ingest and model preprocessing are parity-unpinned upstream rows; the hot path is
    compared GIVEN them): counts equal, best LCP within 1e-5, pose within 1 mm / 1 degree."""
    import ctypes as C
    from model_matching_amd import capi
    from model_matching_amd.estimator import ingest_scene
    raw, fix, obj, scene, repo = _write_example_tree(tmp_path, name)
    K = [float(x) for x in raw["K"]]
    pre = subprocess.run([PRE, obj, "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                          "--model-scale", repr(float(raw["model_scale"]))], capture_output=True, text=True, timeout=300)
    assert pre.returncode == 0 and "After sampling |M|=" in pre.stdout, pre.stdout + pre.stderr
    assert (repo / "models" / obj / "model_search.ply").exists() and (repo / "models" / obj / "ppf_map").exists()
    seed = 7
    r = subprocess.run([APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(float(raw["depth_scale"])),
                        "--seed", str(seed)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "############# RUNNING STOCS for Scene:" in r.stdout and "|M| = " in r.stdout and "|S|: " in r.stdout
    summ, P = _parse(r.stdout)
    # the clouds the tools worked on: model_search.ply as written, the scene through the same GPU ingest
    L = capi.load()
    n, hn = C.c_int(), C.c_int()
    mp = str(repo / "models" / obj / "model_search.ply").encode()
    assert L.stocs_ply_read(mp, None, None, 0, C.byref(n), C.byref(hn)) == 0 and hn.value == 1
    mpos = np.zeros((n.value, 3), np.float32); mnrm = np.zeros((n.value, 3), np.float32)
    assert L.stocs_ply_read(mp, mpos.ctypes.data_as(capi._fp), mnrm.ctypes.data_as(capi._fp), n.value, C.byref(n), C.byref(hn)) == 0
    spos, snrm, sprob, spix = ingest_scene(raw["depth"], raw["prob"], K, float(raw["depth_scale"]), 0.005, 0.10)
    assert ("|M| = %d," % len(mpos)) in r.stdout and ("|S|: %d" % len(spos)) in r.stdout
    orc = oracle_lib.Oracle(spos, snrm, sprob, spix, mpos, mnrm)
    instance = "edge_map" in fix.files
    if instance:
        orc.set_edge_map(fix["edge_map"])
    ro = orc.run(seed, 100, 200, instance_mode=instance, dispersion=0.9)
    assert (summ["bases"], summ["congruent_sets"], summ["candidates"], summ["best_index"]) == (ro.n_bases, ro.n_quads_total, ro.n_candidates, ro.best_index)
    assert abs(summ["best_lcp"] - ro.best_lcp) <= 1e-5 and summ["candidates"] > 50
    assert _pose_close(P, ro.best_pose16)
    vals = np.array((scene / ("best_pose_candidate_%s.txt" % obj)).read_text().split(), float)
    assert vals.shape == (12,) and np.allclose(vals.reshape(3, 4), P, rtol=2e-5, atol=2e-6)
    assert (scene / "dbg" / "best_pose.ply").exists() and (scene / "dbg" / "scene.ply").exists() and (scene / "dbg" / "sampled_scene.ply").exists()
    assert abs(np.linalg.det(P[:, :3]) - 1.0) < 1e-3 and 0.2 < P[2, 3] < 1.5      # a rotation, in front of the camera
    # The only reference-held evidence for the winner (the reference commits no expected pose): the frame's OWN depth image and
    # class-probability map.  The model under the pose, projected through K (tools/pose_check.py): its camera-facing points land on
    # the object's mask and a good part of them within a centimetre of the observed depth.  Floors are generous -- one trial of 100
    # bases is a weak estimator on the linemod frame (best LCP 0.04-0.06); tests/test_trials_gpu.py holds the best of 64 trials to more.
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from pose_check import depth_agreement
    da = depth_agreement(P, mpos, mnrm, raw["depth"], raw["prob"], K, float(raw["depth_scale"]))
    floors = {"ycb_024_bowl": (0.35, 0.90), "linemod_obj_06": (0.05, 0.80), "packed_dove": (0.45, 0.70)}[name]
    assert da["visible_points"] >= 100 and da["in_image"] >= 0.95 and da["with_depth"] >= 0.8, da
    assert da["within_10mm"] >= floors[0] and da["on_mask"] >= floors[1], da
    # the reference's per-call sequence restated (tests/cpp/reference_call_sequence.cpp): the facade serves its one-call-per-
    # attempt / per-base / per-quad loops from batched GPU passes (look-ahead block of class-mode attempts, one congruent search
    # for all sampled bases, candidates on the host).  Same bases and congruent sets; its own shuffle only matters for bases
    # with >= 200 sets (none on the two class-mode frames, most bases of the packed frame)
    env = dict(os.environ, STOCS_REPO_PATH=str(repo), STOCS_INTRINSICS=",".join(repr(k) for k in K), STOCS_DEPTH_SCALE=repr(float(raw["depth_scale"])),
               STOCS_SEED=str(seed))
    pc = subprocess.run([PERCALL, str(scene), obj], capture_output=True, text=True, timeout=600, env=env)
    assert pc.returncode == 0, pc.stdout + pc.stderr
    assert ("Sampled %d bases in" % ro.n_bases) in pc.stdout and ("found %d congruent sets in" % ro.n_quads_total) in pc.stdout
    # a base with >= 200 congruent sets is sub-sampled (stocs_match_one_object.cpp:126-142), by the caller's own shuffle in the
    # per-call sequence: then the two drivers verify different subsets (the packed frame always; the ycb frame since its scene
    # normals come from the depth gradient)
    _, _, cand_base = orc.candidates()
    subsampled = instance or (len(cand_base) and np.bincount(cand_base).max() >= 190) or ro.n_quads_total > 2 * ro.n_candidates
    if not subsampled:
        assert ("candidates %d," % ro.n_candidates) in pc.stdout
        vals2 = np.array((scene / ("best_pose_candidate_%s.txt" % obj)).read_text().split(), float)
        assert np.allclose(vals2, vals, rtol=2e-5, atol=2e-6)
    else:
        lcp2 = float(pc.stdout.split("best lcp")[1].split()[0])
        assert abs(lcp2 - ro.best_lcp) < 0.02 and lcp2 > 0.05            # another subset of the big bases' sets: a pose of the same quality


@pytest.mark.gpu
def test_facade_batching_is_invisible_to_a_per_call_caller(tmp_path):
    """tests/cpp/facade_percall_check.cpp: the look-ahead block of class-mode attempts, the one congruent search for all
    sampled bases and the per-base fallback give exactly what one C-ABI call per reference call gives (second context):
    130 attempts across the block boundary, searches out of order, a foreign base in between, sampling and searching
    interleaved."""
    from model_matching_amd import synth, cloudio
    m, s, k = synth.workload("tiny")
    cloudio.write_stcl(tmp_path / "scene.stcl", s.pos, s.nrm, s.prob, s.pixel)
    cloudio.write_stcl(tmp_path / "model.stcl", m.pos, m.nrm)
    exe = os.path.join(ROOT, "model_matching_amd", "apps", "facade_percall_check")
    r = subprocess.run([exe, str(tmp_path / "scene.stcl"), str(tmp_path / "model.stcl")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches 0" in r.stdout


def test_stocs_single_fails_loudly_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    if not os.path.exists(APP):
        import __graft_entry__ as g
        g.build()
    from model_matching_amd import synth, cloudio
    m = synth.make_model(50, seed=3)
    cloudio.write_stcl(tmp_path / "a.stcl", m.pos, m.nrm, np.ones(50, np.float32))
    r = subprocess.run([APP, "--clouds", str(tmp_path / "a.stcl"), str(tmp_path / "a.stcl")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_trial_sharding_tool_single_and_two_ranks():
    """tools/trials.py (BASELINE config 4): the 2-rank run (sharing the one GPU, gloo rehearsal) must pick
    the same winner as the single-process run over the same trials."""
    import json, socket, sys
    env = dict(os.environ, PYTHONPATH=ROOT)
    one = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "trials.py"), "--trials", "16", "--seed", "3"], capture_output=True, text=True,
                         timeout=600, env=env, cwd=ROOT)
    assert one.returncode == 0, one.stderr[-2000:]
    r1 = json.loads(one.stdout.strip().splitlines()[-1])
    assert r1["mode"] == "instance" and r1["best_lcp"] > 0.05 and r1["candidates_verified"] > 1000  # decayed class probabilities (Q8) keep instance-mode scores low
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    env2 = dict(env, STOCS_BENCH_REHEARSAL="1")
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(ROOT, "tools", "trials.py"), "--trials", "16", "--seed", "3"],
                         capture_output=True, text=True, timeout=900, env=env2, cwd=ROOT)
    assert two.returncode == 0, two.stderr[-3000:]
    r2 = json.loads([l for l in two.stdout.splitlines() if l.startswith("{")][-1])
    assert r2["n_gpus"] == 2 and r2["rehearsal"] is True and r2["world_size"] == 2 and r2["backend"] == "gloo"
    assert [x["rank"] for x in r2["ranks"]] == [0, 1] and [x["trials"] for x in r2["ranks"]] == [[0, 8], [8, 16]]
    assert (r2["best_lcp"], r2["best_trial"], r2["best_candidate"]) == (r1["best_lcp"], r1["best_trial"], r1["best_candidate"])
    assert r2["best_pose_row_major_3x4"] == r1["best_pose_row_major_3x4"] and r2["candidates_verified"] == r1["candidates_verified"]


@pytest.mark.gpu
def test_bench_gpus_2_without_a_launcher_runs_two_ranks():
    """`python bench.py --gpus 2` as ONE plain process (no WORLD_SIZE) must start two rank processes itself and report them
    (it used to run one rank and print n_gpus 1).  Both ranks share this box's one GPU over gloo (STOCS_BENCH_REHEARSAL=1):
    a rehearsal of the launch path, not a measurement; tools/trials.py --gpus 2 takes the same path."""
    import json, sys
    env = dict(os.environ, PYTHONPATH=ROOT, STOCS_BENCH_REHEARSAL="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-pmc", "--no-cpu-baseline",
                        "--no-pipeline", "--workload", "small"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rehearsal"] is True and out["distributed"]["world_size"] == 2 and out["distributed"]["backend"] == "gloo"
    assert out["distributed"]["ranks_reporting"] == [0, 1]          # (the per-rank records themselves are in the details file)
    assert len(lines[0]) < 4096 and out["value"] > 0 and out["config"]["candidates_per_step_per_gpu"] == 2048
    t = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "trials.py"), "--gpus", "2", "--trials", "4", "--seed", "3"], capture_output=True, text=True,
                       timeout=900, env=env, cwd=ROOT)
    assert t.returncode == 0, t.stderr[-3000:]
    rt = json.loads([l for l in t.stdout.splitlines() if l.startswith("{")][-1])
    assert rt["n_gpus"] == 2 and rt["world_size"] == 2 and [x["rank"] for x in rt["ranks"]] == [0, 1]


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_last_steps_scores(tmp_path, oracle_lib):
    """`bench.py --dump-outputs DIR` writes what the timed path computed in its last step -- every candidate's score and the
    arg-max -- as .npy files: the same files from run to run (seeded inputs), the oracle's scores on the same batch.  The line
    reports the --steps it was given and ms_per_step."""
    import json
    from model_matching_amd import synth
    dumps = []
    for run in range(2):
        d = tmp_path / ("dump%d" % run)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-pmc", "--no-cpu-baseline",
                            "--no-pipeline", "--no-c5", "--workload", "small", "--details", str(tmp_path / "details.json"), "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert sorted(a) == ["best_candidate_id.npy", "best_lcp.npy", "lcp_scores.npy"]
    for f in a:
        assert a[f].dtype in (np.float32, np.float64) and a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), f
    got = a["lcp_scores.npy"]
    assert got.shape == (2048,) and int(a["best_candidate_id.npy"][0]) == int(np.argmax(got)) and a["best_lcp.npy"][0] == got.max() > 0
    m, s, k = synth.workload("small")
    orc = oracle_lib.Oracle(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    cs, cm = orc.centroids()
    T = synth.make_candidates(synth.centred_gt(s.T_gt, cs.astype(np.float64), cm.astype(np.float64)), k, seed=synth.SEED_CAND)
    assert np.abs(orc.lcp_batch(T, nthreads=4) - got).max() <= 1e-5


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_full_adds_the_rest(tmp_path):
    """A plain `bench.py` run measures its timed steps and nothing else: no roofline, no CPU baseline, no oracle comparison, no
    whole-path report, in the line or in the details file.  `--full` adds them to the same timed steps."""
    import json
    recs = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-pmc", "--no-pipeline", "--cpu-seconds", "0.5"])):
        details = tmp_path / ("%s.json" % mode)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "small",
                            "--details", str(details)] + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        recs[mode] = json.loads(lines[0]), json.load(open(details))
    for line, _ in recs.values():
        assert line["metric"] == "candidate poses verified/sec" and line["unit"] == "poses/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f32" and line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["final_lcp_percent"] > 0
    line, det = recs["plain"]
    for k in ("roofline", "cpu_baseline", "cpu_baseline_all_cores", "oracle_check", "pipeline", "cpu_baseline_pipeline"):
        assert k not in line and k not in det, k
    line, det = recs["full"]
    assert line["roofline"]["kernel_ms"] > 0 and det["roofline"]["hits_per_pose"] > 0
    assert line["cpu_baseline"]["value"] > 0 and det["oracle_check"]["candidates_compared"] == 2048 and det["oracle_check"]["within_tolerance"]
    assert recs["full"][1]["final_lcp_percent"] == recs["plain"][1]["final_lcp_percent"]     # the same batch, the same last step


@pytest.mark.gpu
def test_stocs_single_instance_mode_on_packed_dove(tmp_path):
    """edge map present -> the driver takes the sample_instance_base path (stocs_match_one_object.cpp:90)."""
    from model_matching_amd import cloudio
    d = np.load(os.path.join(ROOT, "tests", "golden", "example_packed_dove.npz"))
    cloudio.write_stcl(tmp_path / "scene.stcl", d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"])
    cloudio.write_stcl(tmp_path / "model.stcl", d["model_pos"], d["model_nrm"])
    d["edge_map"].astype(np.uint8).tofile(tmp_path / "edge.u8")
    out = tmp_path / "pose.txt"
    r = subprocess.run([APP, "--clouds", str(tmp_path / "scene.stcl"), str(tmp_path / "model.stcl"), "--edge", str(tmp_path / "edge.u8"), "--seed", "5",
                        "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sampled " in r.stdout and "Transforms to verify: " in r.stdout
    n_tf = int(r.stdout.split("Transforms to verify: ")[1].split()[0])
    score = float(r.stdout.split("maximum score: ")[1].split()[0])
    assert n_tf > 500 and score > 0.03
    P = np.array(out.read_text().split(), float).reshape(3, 4)
    assert abs(np.linalg.det(P[:, :3]) - 1.0) < 1e-3 and 0.2 < P[2, 3] < 1.5      # a rotation, in front of the camera
    # The only reference-held evidence for the winner (the reference commits no expected pose): the frame's OWN depth image and
    # class-probability map.  The model under the pose, projected through K (tools/pose_check.py): its camera-facing points land on
    # the object's mask and a good part of them within a centimetre of the observed depth.  Floors are generous -- one trial of 100
    # bases is a weak estimator on the linemod frame (best LCP 0.04-0.06); tests/test_trials_gpu.py holds the best of 64 trials to more.
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from pose_check import depth_agreement
    raw = np.load(os.path.join(ROOT, "tests", "golden", "example_packed_dove_raw.npz"))
    da = depth_agreement(P, d["model_pos"], d["model_nrm"], raw["depth"], raw["prob"], [float(x) for x in raw["K"]], float(raw["depth_scale"]))
    assert da["visible_points"] >= 100 and da["in_image"] >= 0.95 and da["with_depth"] >= 0.8, da
    assert da["within_10mm"] >= 0.45 and da["on_mask"] >= 0.70, da


@pytest.mark.gpu
def test_stocs_single_trials_option_equals_the_library_batch(tmp_path):
    """stocs_single --trials N: N independent runs of the reference's loop (seeds seed, seed + 1, ...) through the facade's
    run_trials = one stocs_run_trials call; per-trial counts and best scores equal the ctypes mirror's, the best trial's pose is
    what gets written."""
    from model_matching_amd import cloudio
    from model_matching_amd.estimator import StocsEstimator
    d = np.load(os.path.join(ROOT, "tests", "golden", "example_ycb_024_bowl.npz"))
    cloudio.write_stcl(tmp_path / "scene.stcl", d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"])
    cloudio.write_stcl(tmp_path / "model.stcl", d["model_pos"], d["model_nrm"])
    out = tmp_path / "pose.txt"
    r = subprocess.run([APP, "--clouds", str(tmp_path / "scene.stcl"), str(tmp_path / "model.stcl"), "--seed", "40", "--trials", "6", "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
    res = est.run_trials([40 + t for t in range(6)], 100, max_per_base=200)
    lines = [l for l in r.stdout.splitlines() if l.startswith("trial ")]
    assert len(lines) == 6
    for t, l in enumerate(lines):
        w = l.split()
        assert (int(w[3]), int(w[6]), int(w[8])) == (res[t]["n_bases"], res[t]["n_quads"], res[t]["n_candidates"]), l
        assert abs(float(w[11]) - res[t]["best_lcp"]) <= 1e-5 * max(1.0, res[t]["best_lcp"]), l
    best = max(range(6), key=lambda t: (res[t]["best_lcp"], -t))
    summ = [l for l in r.stdout.splitlines() if l.startswith("trials: ")][0]
    assert ("best_trial=%d " % best) in summ
    P = np.array(out.read_text().split(), float).reshape(3, 4)
    assert np.allclose(P, res[best]["best_pose"].reshape(4, 4).T[:3], rtol=2e-5, atol=2e-6)
