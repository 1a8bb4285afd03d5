"""stocs_scene_footprints_mesh on the GPU against the restatement of its contract (tests/render_mesh_ref.py on tests/scene_ref.py): rows and
records equal bit for bit, the record equal to stocs_explain_poses_mesh of the pose alone, the neighbouring slots untouched, chunks that
end inside a batch, a pool that mixes splat and mesh slots walked by stocs_scene_select, and select_scene(..., surface=...)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_cases as mc  # noqa: E402
import render_mesh_ref as ref  # noqa: E402
import scene_ref as sref  # noqa: E402
import vsd_cases as vc  # noqa: E402
from test_render_mesh_gpu import _est, frame_for, meshes, poses_for  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SCALE = vc.DEPTH_SCALE
PRM = dict(tolerance=0.02, class_threshold=0.1)
ONES = np.uint32(0xFFFFFFFF)


def _footprints(est, shape, poses, slot_base, n_slots, claim, mesh=True, **prm):
    """-> (the whole pool (n_slots, Wr), pre-filled with ones; the records)"""
    from model_matching_amd.estimator import scene_row_words
    pool = np.full((n_slots, scene_row_words(shape)), ONES, np.uint32)
    d = est.dev_alloc(pool.nbytes)
    try:
        est.dev_upload(d, pool)
        rec = (est.scene_footprints_mesh if mesh else est.scene_footprints)(poses, d, slot_base, n_slots, claim, **prm)
        est.dev_download(d, pool)
    finally:
        est.dev_free(d)
    return pool, rec


@pytest.fixture(scope="module")
def est():
    e = _est()
    yield e
    e.close()


def _check(est, v, t, depth, prob, K, poses, claim):
    """slots 1 .. n of a pool of n + 2 against the restatement; the guard slots; every record against explain_poses_mesh of the pose alone"""
    est.set_mesh(v, t)
    est.set_frame(depth, prob, K, SCALE)
    poses = np.asarray(poses, F).reshape(-1, 16)
    n = len(poses)
    w_rec, w_masks = ref.footprints(poses, v, t, depth, prob, K, SCALE, claim, **PRM)
    pool, rec = _footprints(est, depth.shape, poses, 1, n + 2, claim, **PRM)
    assert (pool[0] == ONES).all() and (pool[-1] == ONES).all()
    assert np.array_equal(pool[1:-1], sref.pack_rows(w_masks)), [h for h in range(n) if not np.array_equal(pool[1 + h], sref.pack_rows(w_masks[h:h + 1])[0])][:5]
    assert sref.records_equal(rec, w_rec), (rec, w_rec)
    assert np.array_equal(rec["footprint"], rec["no_depth"] + rec["agree"] + rec["in_front"] + rec["behind"])
    assert np.array_equal(rec["claimed"], sref.unpack_rows(pool[1:-1], depth.size).sum(axis=1))
    return rec, pool[1:-1]


@pytest.mark.parametrize("claim", ["agree", "on_mask"])
@pytest.mark.parametrize("W, H, name", [(33, 17, "ellipsoid2"), (64, 48, "ellipsoid3"), (160, 120, "box"), (64, 48, "triangle")])
def test_rows_and_records(est, W, H, name, claim):
    v, t = meshes()[name]
    depth, prob = frame_for(W, H, 5)
    K = vc.small_camera(W, H)
    E = poses_for(name, 5, 40 + W)
    E[2, 12] = np.nan; E[4] = 0                              # an invalid pose and the all-zero record inside the batch
    rec, rows = _check(est, v, t, depth, prob, K, E, claim)
    assert rec["claimed"][[0, 1, 3]].all() and not rows[[2, 4]].any() and not any(rec[2].tolist()) and not any(rec[4].tolist())
    for h in range(5):                                       # the record of the pose alone in the joint renderer
        e = est.explain_poses_mesh(E[h:h + 1], **PRM)[0]
        assert e["hidden"] == 0 and e["visible"] == e["footprint"]
        assert all(rec[k][h] == e[k] for k in ("footprint", "no_depth", "agree", "in_front", "behind", "on_mask")), (h, rec[h], e)


def test_chunks_of_two_and_a_second_call_allocates_nothing(est, monkeypatch):
    from model_matching_amd import capi
    L = capi.load()
    v, t = mc.ellipsoid(2)
    W, H = 64, 48
    depth, prob = frame_for(W, H, 6)
    K = vc.small_camera(W, H)
    E = mc.random_poses(7, 17, z=0.8, spread=0.02)
    whole, rows = _check(est, v, t, depth, prob, K, E, "agree")
    monkeypatch.setenv("STOCS_SCENE_CHUNK", "2")             # chunks end inside the batch; 7 is no multiple
    d = est.dev_alloc(rows.nbytes)
    a0 = L.stocs_device_alloc_count()
    rec = est.scene_footprints_mesh(E, d, 0, 7, "agree", **PRM)
    assert L.stocs_device_alloc_count() == a0                # the workspace of the unchunked call serves
    pool = np.zeros_like(rows)
    est.dev_download(d, pool)
    est.dev_free(d)
    assert np.array_equal(pool, rows) and rec.tobytes() == whole.tobytes()
    pool, rec = _footprints(est, depth.shape, E[::-1], 0, 7, "agree", **PRM)
    assert np.array_equal(pool[::-1], rows) and rec[::-1].tobytes() == whole.tobytes()
    for h in (0, 6):
        pool, rec = _footprints(est, depth.shape, E[h], 0, 1, "agree", **PRM)
        assert np.array_equal(pool[0], rows[h]) and rec[0] == whole[h]


def test_errors_in_the_documented_order():
    from model_matching_amd import capi
    L = capi.load()
    e = _est()
    P, pP = capi.f32(mc.random_poses(2, 4))
    out = (capi.SceneRecord * 2)()
    prm = capi.RenderParams(); L.stocs_default_render_params(C.byref(prm))
    prm.point_radius = float("nan"); prm.max_splat_px = 99   # ignored, whatever they hold
    rows = e.dev_alloc(4 * 4096)
    call = lambda n=2, p=pP, base=0, slots=2, q=prm, claim=0, r=rows, o=out: L.stocs_scene_footprints_mesh(e.h, p, n, base, slots, C.byref(q) if q is not None else None, claim, r, o)
    STATE = L.stocs_depth_check_poses(e.h, pP, 1, C.byref(capi.DepthParams(0.01, 0.1, 0, 8, 0.01)), (capi.DepthResult * 1)())
    assert call(n=0, p=None, q=None, r=None, o=None) == 0
    assert call(n=-1) == -1 and call(p=None) == -1 and call(q=None) == -1 and call(r=None) == -1 and call(o=None) == -1
    assert call(claim=2) == -1 and call(base=-1) == -1 and call(base=1) == -1
    q = capi.RenderParams(); L.stocs_default_render_params(C.byref(q)); q.tolerance = 0.0
    assert call(q=q) == -1 and b"tolerance" in L.stocs_last_error()
    assert call() == STATE and b"no mesh" in L.stocs_last_error()
    v, t = mc.ellipsoid(1)
    e.set_mesh(v, t)
    assert call() == STATE and b"no frame" in L.stocs_last_error()
    e.set_frame(vc.flat_frame(64, 48, 0.8), None, vc.small_camera(64, 48), SCALE)
    assert call() == 0
    e.set_frame(vc.flat_frame(1024, 513, 0.8), None, vc.small_camera(1024, 513), SCALE)       # 2^19 + 1024 pixels
    assert call() not in (0, -1, STATE) and b"pixels" in L.stocs_last_error()
    e.dev_free(rows)
    e.close()


@pytest.fixture(scope="module")
def two_objects():
    """a ball as a point model and an ellipsoid as a mesh in front of a wall that shows two of the hypotheses"""
    W, H = 64, 48
    K = vc.small_camera(W, H)
    pos, nrm = vc.ball_model(400, 7)
    v, t = mc.ellipsoid(2)
    Pb = np.stack([vc.pose16(vc.translation(-0.07, 0.0, 0.8)), vc.pose16(vc.translation(-0.06, 0.01, 0.8)), vc.pose16(vc.translation(0.0, 0.05, 0.9))])
    Pm = np.stack([vc.pose16(vc.translation(0.08, 0.0, 0.8)), vc.pose16(vc.translation(0.075, -0.01, 0.81)), vc.pose16(vc.translation(-0.06, 0.0, 0.82))])
    import render_ref as rref
    zb = rref.render(rref.empty_keys(W, H), Pb[:1], pos, nrm, K, W, H, 0, True, point_radius=0.006)
    zm = ref.z_bits(Pm[0], v, t, K, W, H)
    z = np.minimum((zb >> np.uint64(32)).astype(np.uint32), zm)
    depth = vc.raw_from_depth(np.where(z != ref.EMPTY32, z.view(F), 1.0).reshape(H, W))
    return dict(W=W, H=H, K=K, pos=pos, nrm=nrm, v=v, t=t, Pb=Pb, Pm=Pm, depth=depth, sprm=dict(PRM, point_radius=0.006, max_splat_px=8))


def test_a_pool_of_splat_and_mesh_slots(two_objects):
    """the ball's slots from stocs_scene_footprints, the ellipsoid's from the mesh form, in one pool; stocs_scene_select walks it as
    scene_ref.select walks the restatement's masks"""
    import scene_ref
    from model_matching_amd.estimator import scene_row_words
    s = two_objects
    eb, em = _est(s["pos"], s["nrm"]), _est()
    em.set_mesh(s["v"], s["t"])
    for e in (eb, em):
        e.set_frame(s["depth"], None, s["K"], SCALE)
    shape = s["depth"].shape
    pool = np.full((8, scene_row_words(shape)), ONES, np.uint32)
    d = eb.dev_alloc(pool.nbytes)
    eb.dev_upload(d, pool)
    rm = em.scene_footprints_mesh(s["Pm"], d, 4, 8, "agree", **PRM)            # the later slots first
    rb = eb.scene_footprints(s["Pb"], d, 1, 8, "agree", **s["sprm"])
    eb.dev_download(d, pool)
    wb, mb, _ = scene_ref.footprints(s["Pb"], s["pos"], s["nrm"], s["depth"], None, s["K"], SCALE, "agree", **s["sprm"])
    wm, mm = ref.footprints(s["Pm"], s["v"], s["t"], s["depth"], None, s["K"], SCALE, "agree", **PRM)
    assert scene_ref.records_equal(rb, wb) and scene_ref.records_equal(rm, wm)
    assert np.array_equal(pool[1:4], scene_ref.pack_rows(mb)) and np.array_equal(pool[4:7], scene_ref.pack_rows(mm)) and (pool[[0, 7]] == ONES).all()
    # the walk over slots 1 .. 6 as a pool of their own
    d2 = eb.dev_alloc(pool[1:7].nbytes)
    eb.dev_upload(d2, pool[1:7])
    rec = np.concatenate([rb, rm])
    score = scene_ref.default_score(rec)
    group = np.array([0, 0, 0, 1, 1, 1], np.int32)
    got, sel = em.scene_select(d2, shape, score, group, rec, min_pixels=20)
    want, wsel = scene_ref.select(np.concatenate([mb, mm]), score, group, rec, 2, min_pixels=20)
    assert scene_ref.records_equal(got, want) and np.array_equal(sel, wsel)
    assert set(sel.tolist()) >= {0, 3}                       # the two hypotheses the frame shows
    eb.dev_free(d); eb.dev_free(d2)
    eb.close(); em.close()


def test_select_scene_with_a_surface_per_object(two_objects):
    from model_matching_amd.estimator import select_scene
    import render_ref as rref
    import scene_ref
    s = two_objects
    eb, em = _est(s["pos"], s["nrm"]), _est(s["pos"], s["nrm"])
    em.set_mesh(s["v"], s["t"])
    for e in (eb, em):
        e.set_frame(s["depth"], None, s["K"], SCALE)
    W, H, K = s["W"], s["H"], s["K"]
    got = select_scene([eb, em], [s["Pb"], s["Pm"]], labels=True, surface=["points", "mesh"], min_pixels=20, **s["sprm"])
    wb, mb, _ = scene_ref.footprints(s["Pb"], s["pos"], s["nrm"], s["depth"], None, K, SCALE, "agree", **s["sprm"])
    wm, mm = ref.footprints(s["Pm"], s["v"], s["t"], s["depth"], None, K, SCALE, "agree", **PRM)
    foot = np.concatenate([wb, wm])
    assert scene_ref.records_equal(got["footprints"], foot)
    score = scene_ref.default_score(foot)
    want, wsel = scene_ref.select(np.concatenate([mb, mm]), score, got["group"], foot, 2, min_pixels=20)
    assert scene_ref.records_equal(got["records"], want) and np.array_equal(got["selected"], wsel) and len(wsel) >= 2
    zkey = ref.empty_keys(W, H)
    for slot in wsel.tolist():
        if slot < 3:
            rref.render(zkey, s["Pb"][slot], s["pos"], s["nrm"], K, W, H, slot, **s["sprm"])
        else:
            ref.render(zkey, s["Pm"][slot - 3], s["v"], s["t"], K, W, H, slot)
    w_render = np.concatenate([rref.resolve(zkey, s["Pb"][slot], s["pos"], s["nrm"], s["depth"], None, K, SCALE, slot, **s["sprm"]) if slot < 3
                               else ref.resolve(zkey, s["Pm"][slot - 3], s["v"], s["t"], s["depth"], None, K, SCALE, slot, **PRM) for slot in wsel.tolist()])
    assert got["render"].tobytes() == w_render.tobytes()
    w_lab, w_st = ref.labels(zkey, s["depth"], None, SCALE, **PRM)
    assert np.array_equal(got["labels"], w_lab) and np.array_equal(got["state"], w_st)
    # the default is all points, as before; a mesh object's footprint differs from its points'
    plain = select_scene([eb, em], [s["Pb"], s["Pm"]], min_pixels=20, **s["sprm"])
    same = select_scene([eb, em], [s["Pb"], s["Pm"]], surface=["points", "points"], min_pixels=20, **s["sprm"])
    assert plain["footprints"].tobytes() == same["footprints"].tobytes() and plain["footprints"][3:].tobytes() != got["footprints"][3:].tobytes()
    with pytest.raises(ValueError):
        select_scene([eb, em], [s["Pb"], s["Pm"]], surface=["points"])
    with pytest.raises(ValueError):
        select_scene([eb, em], [s["Pb"], s["Pm"]], surface=["points", "surfels"])
    eb.close(); em.close()
