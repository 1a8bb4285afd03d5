"""The workgroup-wide list of live sub-patches of the split scoring forms (lcp.hip, SPLIT and CU = 16): the four wavefronts of a
candidate test its sub-patches together, append the live ones to one LDS list in an order that differs from run to run, and take
the 64-lane steps of that list round-robin.  A score is an integer sum over the candidate's model points, so none of that may show:
a context that runs the split form (lcp_split 1), one that runs one wavefront per candidate with its own ring (lcp_split 0) and one
that runs the plain lane-per-query kernel (lcp_variant 0: no patch test, no rings) must return the same scores BITWISE -- on the
synthetic workloads, on models around the sizes where steps, sub-patches and windows end (models below 512 points are never split:
the three contexts still have to agree), on a model just over the size the shared list holds (the split form then walks per-wave
rings), on poses that leave no sub-patch or every sub-patch alive, and on batches of 1, 3 and 5 candidates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONTEXTS = [("split", "lcp_split", 1), ("one_wave", "lcp_split", 0), ("plain", "lcp_variant", 0)]


def _contexts(model_pos, model_nrm, scene):
    from model_matching_amd.estimator import StocsEstimator
    ests = {}
    for label, key, value in CONTEXTS:
        est = StocsEstimator(scene.pos, scene.nrm, scene.prob, scene.pixel, model_pos, model_nrm, build_index=False)
        est.set_option("lcp_cull", 2)          # the patch test from the first call on (the default waits for 1e9 point queries)
        est.set_option(key, value)
        ests[label] = est
    return ests


def _centred_gt(est, scene):
    from model_matching_amd import synth
    return synth.centred_gt(scene.T_gt, est.get_scene_centroid().astype(np.float64), est.get_model_centroid().astype(np.float64))


def _far_and_odd(near, Tgt, rng):
    """poses that put the model nowhere near the scene (no live sub-patch), and transforms that are not rigid or not finite"""
    from model_matching_amd import synth
    far = np.zeros((8, 4, 4))
    for i in range(8):
        far[i, :3, :3] = synth.random_rotation(rng)
        far[i, :3, 3] = Tgt[:3, 3] + np.array([(0.6, 0, 0), (0, -0.7, 0), (0, 0, 0.9), (-3, 2, 1), (0.4, 0.4, 0.4), (50, 0, 0), (0, 0, -0.5), (-0.6, 0.1, 0)][i])
        far[i, 3, 3] = 1.0
    far = np.ascontiguousarray(far.transpose(0, 2, 1).reshape(8, 16).astype(np.float32))
    odd = near[:8].copy()
    odd[0, 12] = np.nan; odd[1, 0] = np.inf; odd[2, :12] *= 1.7; odd[3, :] = 0.0; odd[4, 12:15] = [1e6, -1e6, 1e6]
    return far, odd


def _assert_same(ests, T, what):
    res = {label: est.score_transforms(T) for label, est in ests.items()}
    for label in ("one_wave", "plain"):
        assert np.array_equal(res[label].view(np.uint32), res["split"].view(np.uint32)), (what, label)
    again = ests["split"].score_transforms(T)      # the list's order differs from run to run: the scores do not
    assert np.array_equal(again.view(np.uint32), res["split"].view(np.uint32)), what
    return res["split"]


def _close(ests):
    for est in ests.values():
        est.close()


@pytest.mark.parametrize("name,n", [("tiny", 256), ("small", 2048), ("dense", 512), ("Cm", 4096), ("C5", 128)])
def test_synthetic_workloads(name, n):
    from model_matching_amd import synth
    m, s, k = synth.workload(name)
    ests = _contexts(m.pos, m.nrm, s)
    Tgt = _centred_gt(ests["split"], s)
    near = synth.make_candidates(Tgt, min(n, k))
    far, odd = _far_and_odd(near, Tgt, np.random.default_rng(23))
    got = _assert_same(ests, np.concatenate([near, far, odd]), name)
    assert got[: len(near)].max() > 0.05 and got[len(near) + 3] == 0.0 and got[len(near) + 5] == 0.0   # (metres away: nothing alive)
    for c in (1, 3, 5):
        _assert_same(ests, near[:c], (name, c))
    _close(ests)


@pytest.mark.parametrize("n", [15, 16, 17, 63, 64, 65, 1023, 8192, 8193, 8209])
def test_model_sizes(n):
    """15 .. 65: around one sub-patch and one step (never split, no field below 64 points); 1 023: 64 sub-patches less one point, one
    window; 8 192: 512 sub-patches, the shared list full when every one is live; 8 193 and 8 209: one point and one sub-patch over,
    the split form walks its per-wave rings"""
    from model_matching_amd import synth
    full = synth.make_model(max(n + 40, 400), seed=31 + n)
    assert len(full.pos) >= n
    pos, nrm = np.ascontiguousarray(full.pos[:n]), np.ascontiguousarray(full.nrm[:n])
    s = synth.make_scene(full, 6000, seed=57 + n)
    ests = _contexts(pos, nrm, s)
    Tgt = _centred_gt(ests["split"], s)
    near = synth.make_candidates(Tgt, 512)
    far, odd = _far_and_odd(near, Tgt, np.random.default_rng(n))
    got = _assert_same(ests, np.concatenate([near, far, odd]), n)
    assert got[512 + 3] == 0.0 and got[512 + 5] == 0.0   # (metres away: nothing alive)
    if n >= 1023:
        assert got[:512].max() > 0.02
    for c in (1, 3, 5):
        _assert_same(ests, near[7: 7 + c], (n, c))
    _close(ests)


@pytest.mark.parametrize("n", [1023, 5000, 8192, 8193])
def test_every_sub_patch_live_and_none(n):
    """the scene holds every model point (plus a plane of clutter), so the ground-truth pose leaves every sub-patch alive -- at 8 192
    points the list holds its 512 entries -- and half a metre away none is: alone, mixed in one batch, in batches of 1, 3 and 5"""
    from model_matching_amd import synth
    m = synth.make_model(n + 40, seed=91)
    pos, nrm = np.ascontiguousarray(m.pos[:n]), np.ascontiguousarray(m.nrm[:n])
    rng = np.random.default_rng(5 + n)
    T_gt = synth.gt_pose()
    R, t = T_gt[:3, :3], T_gt[:3, 3]
    obj = pos.astype(np.float64) @ R.T + t
    grid = np.stack(np.meshgrid(np.arange(-40, 40), np.arange(-40, 40), indexing="ij"), -1).reshape(-1, 2) * 0.004
    plane = np.concatenate([grid, np.full((len(grid), 1), 0.95)], axis=1) + [0.05, -0.03, 0.0]
    sp = np.concatenate([obj, plane]).astype(np.float32)
    sn = np.concatenate([nrm.astype(np.float64) @ R.T, np.tile([0.0, 0.0, -1.0], (len(plane), 1))]).astype(np.float32)
    idx = np.arange(len(sp))
    scene = synth.Scene(sp, sn, rng.uniform(0.3, 1.0, len(sp)).astype(np.float32), np.stack([idx // 640, idx % 640], 1).astype(np.int32), n, T_gt)
    ests = _contexts(pos, nrm, scene)
    Tgt = _centred_gt(ests["split"], scene)
    on = np.ascontiguousarray(Tgt.T.reshape(1, 16).astype(np.float32))   # the ground truth itself, column-major
    off = on.copy(); off[0, 12] += 0.5
    assert _assert_same(ests, on, (n, "all live"))[0] > 0.2   # (weights of 0.3 .. 1; a dot product that rounds above 1 is not counted)
    assert _assert_same(ests, off, (n, "none live"))[0] == 0.0
    mixed = np.concatenate([on, off, on, off, off])
    for c in (1, 3, 5):
        got = _assert_same(ests, mixed[:c], (n, "mixed", c))
        assert np.array_equal(got > 0, (np.arange(c) % 2 == 0) & (np.arange(c) < 3))
    _close(ests)
