"""stocs_scene_footprints / stocs_scene_select / select_scene on the GPU against the restatement of their contract (tests/scene_ref.py): every
comparison is array_equal on the downloaded pixel rows and on the records.  Shapes are the smallest at which the kernels can go wrong:
one point at the edges of the splat rule and of the image, two points of one pose on one pixel, models either side of a wavefront, of a
256-point round and of the splat kernel's chunk, frames whose row words straddle image rows and end in padding, the two sizes either
side of the capacity; for the walk, rows uploaded straight from numpy (tests/scene_cases.py), so that it is tested without the renderer."""
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

import render_ref as rref  # noqa: E402
import scene_cases as cases  # noqa: E402
import scene_ref as ref  # noqa: E402
from scene_cases import EPS, K64, K_ROUGH, PRM_ROUGH, SCALE, pose  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
ONES = np.uint32(0xFFFFFFFF)
CHUNK = int(re.search(r"SCENE_CHUNK_POINTS = (\d+)", open(os.path.join(ROOT, "model_matching_amd", "csrc", "scene.hip")).read()).group(1))


def _est(model_pos, model_nrm):
    """a context around a model; the scene plays no part here (a handful of points serves)"""
    from model_matching_amd.estimator import StocsEstimator
    rng = np.random.default_rng(1)
    sp = rng.normal(0, 0.05, (32, 3)).astype(F)
    sn = sp / np.linalg.norm(sp, axis=1, keepdims=True)
    return StocsEstimator(sp, sn, np.ones(32, F), None, np.asarray(model_pos, F).reshape(-1, 3), np.asarray(model_nrm, F).reshape(-1, 3), build_index=False)


def _footprints(est, shape, poses, slot_base, n_slots, claim, **prm):
    """-> (the whole pool (n_slots, Wr), pre-filled with ones through dev_upload; the records)"""
    from model_matching_amd.estimator import scene_row_words
    pool = np.full((n_slots, scene_row_words(shape)), ONES, np.uint32)
    d = est.dev_alloc(pool.nbytes)
    try:
        est.dev_upload(d, pool)
        rec = est.scene_footprints(poses, d, slot_base, n_slots, claim, **prm)
        est.dev_download(d, pool)
    finally:
        est.dev_free(d)
    return pool, rec


class Case:
    """one context + frame; check() writes the poses into slots 1 .. n of a pool of n + 2 slots filled with ones and compares rows and records
    with the restatement, the guard slots with what they held, and every record with the GPU's own explain_poses of that pose alone"""
    def __init__(self, mpos, mnrm, depth, prob, K, scale):
        self.mpos, self.mnrm = np.asarray(mpos, F).reshape(-1, 3), np.asarray(mnrm, F).reshape(-1, 3)
        self.est = _est(self.mpos, self.mnrm)
        self.set_frame(depth, prob, K, scale)

    def set_frame(self, depth, prob, K, scale):
        self.depth, self.prob, self.K, self.scale = depth, prob, K, scale
        self.est.set_frame(depth, prob, K, scale)

    def want(self, poses, claim="agree", **prm):
        return ref.footprints(poses, self.mpos, self.mnrm, self.depth, self.prob, self.K, self.scale, claim, **prm)

    def check(self, poses, claim="agree", explain=True, **prm):
        poses = np.asarray(poses, F).reshape(-1, 16)
        n, npix = len(poses), self.depth.size
        w_rec, w_masks, _ = self.want(poses, claim, **prm)
        pool, rec = _footprints(self.est, self.depth.shape, poses, 1, n + 2, claim, **prm)
        assert (pool[0] == ONES).all() and (pool[-1] == ONES).all()                        # the neighbouring slots are untouched
        assert np.array_equal(pool[1:-1], ref.pack_rows(w_masks)), [h for h in range(n) if not np.array_equal(pool[1 + h], ref.pack_rows(w_masks[h:h + 1])[0])][:5]
        assert ref.records_equal(rec, w_rec), (rec, w_rec)
        assert np.array_equal(rec["footprint"], rec["no_depth"] + rec["agree"] + rec["in_front"] + rec["behind"])
        assert np.array_equal(rec["claimed"], ref.unpack_rows(pool[1:-1], npix).sum(axis=1))
        if explain:
            for h in range(n):
                e = self.est.explain_poses(poses[h:h + 1], **prm)[0]
                assert e["hidden"] == 0 and e["visible"] == e["footprint"]
                assert all(rec[k][h] == e[k] for k in ("footprint", "no_depth", "agree", "in_front", "behind", "on_mask")), (h, rec[h], e)
        return rec, ref.unpack_rows(pool[1:-1], npix).reshape((n,) + self.depth.shape)


@pytest.fixture(scope="module")
def one_point():
    """ONE model point at the origin with normal (0, 0, -1): under the pose [I | t] p = t exactly, q = (0, 0, -1)"""
    depth, prob = cases.flat_frame(64, 48)
    return Case([[0, 0, 0]], [[0, 0, -1]], depth, prob, K64, SCALE)


def test_one_point_splat_radius_and_image_border(one_point):
    c = one_point
    P = pose(t=(0, 0, 1))
    half = float(2.0 ** -6)                                                   # fx * r / z = 0.5 exactly: floor(1.0) = 1
    ulp1 = float(np.nextafter(F(half), F(0)))                                 # one ulp below: the sum rounds to 1.0f: still 1
    below = float(np.nextafter(F(ulp1), F(0)))                                # two ulps below: the sum is 0.99999994f, floor 0
    far = pose(t=(0, 0, float(np.nextafter(F(1), F(2)))))
    for prm, p, foot in ((dict(point_radius=half), P, 9), (dict(point_radius=ulp1), P, 9), (dict(point_radius=below), P, 1), (dict(point_radius=half), far, 1),
                         (dict(point_radius=0.0), P, 1), (dict(point_radius=1.0, max_splat_px=16), P, 33 * 33), (dict(point_radius=1.0, max_splat_px=0), P, 1)):
        rec, m = c.check([p], tolerance=EPS, class_threshold=0.1, **prm)
        assert rec["footprint"][0] == foot, prm
    rec, m = c.check([P], tolerance=EPS, class_threshold=0.1, point_radius=half)
    assert np.array_equal(np.argwhere(m[0]), [[r, q] for r in (23, 24, 25) for q in (31, 32, 33) if (r, q) != (24, 33)])   # the hole has no depth
    prm = dict(tolerance=EPS, class_threshold=0.1, point_radius=half)         # s = 1 at z = 1
    ts = [((-1.0, 0, 1), 6), ((31 / 32, 0, 1), 6), ((0, -24 / 32, 1), 6), ((0, 23 / 32, 1), 6), ((-1.0, -24 / 32, 1), 4), ((31 / 32, 23 / 32, 1), 4),
          ((-33 / 32, 0, 1), 0), ((1.0, 0, 1), 0), ((0, -25 / 32, 1), 0), ((0, 24 / 32, 1), 0)]      # one pixel outside: nothing, though its square would reach in
    rec, m = c.check([pose(t=t) for t, _ in ts], **prm)
    assert rec["footprint"].tolist() == [f for _, f in ts] and m[5, 47, 63] and m[4, 0, 0]


def test_two_points_of_one_pose_on_one_pixel_the_nearer_decides():
    depth, prob = cases.flat_frame(64, 48)
    for order in ([[0, 0, 0], [0, 0, -0.25]], [[0, 0, -0.25], [0, 0, 0]]):    # under [I | (0, 0, 1)]: z = 1 (agrees with the wall) and z = 0.75 (in front of it)
        c = Case(order, [[0, 0, -1], [0, 0, -1]], depth, prob, K64, SCALE)
        rec, m = c.check([pose(t=(0, 0, 1))], tolerance=EPS, class_threshold=0.1, point_radius=0.0)
        assert (rec["footprint"][0], rec["agree"][0], rec["in_front"][0], rec["claimed"][0]) == (1, 0, 1, 0) and not m.any()
    one = Case([[0, 0, 0]], [[0, 0, -1]], depth, prob, K64, SCALE)            # the far point alone agrees
    rec, m = one.check([pose(t=(0, 0, 1))], tolerance=EPS, class_threshold=0.1, point_radius=0.0)
    assert (rec["agree"][0], rec["in_front"][0]) == (1, 0) and m[0, 24, 32]


def test_claims_with_the_class_image_exactly_at_the_threshold(one_point):
    c = one_point
    poses = [pose(t=(0, 0, 1)), pose(t=(-1 / 32, 0, 1)), pose(t=(0.5 / 32, 0, 1)), pose(t=(0, 0, 1.0 + EPS)),
             pose(t=(0, 0, float(np.nextafter(F(1.0 + EPS), F(2.0))))), pose(t=(0, 0, float(np.nextafter(F(1.0 - EPS), F(0.0)))))]
    prm = dict(tolerance=EPS, class_threshold=0.1, point_radius=0.0)
    rec, m = c.check(poses, "agree", **prm)
    assert rec["claimed"].tolist() == [1, 1, 0, 1, 0, 0] and rec["on_mask"].tolist() == [1, 0, 0, 1, 0, 0]
    assert (rec["no_depth"][2], rec["behind"][4], rec["in_front"][5]) == (1, 1, 1) and m[0, 24, 32] and m[1, 24, 31]
    rec, m = c.check(poses, "on_mask", **prm)
    assert rec["claimed"].tolist() == [1, 0, 0, 1, 0, 0] and m[0, 24, 32] and not m[1].any()      # raw 1000 is on the mask, raw 999 is not
    c.set_frame(c.depth, None, K64, SCALE)                                    # no class image: nothing is on the mask
    rec, m = c.check(poses, "on_mask", **prm)
    assert not rec["on_mask"].any() and not rec["claimed"].any() and not m.any() and rec["agree"].tolist() == [1, 1, 0, 1, 0, 0]
    c.set_frame(c.depth, cases.flat_frame(64, 48)[1], K64, SCALE)


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1])
def test_model_sizes_either_side_of_a_wavefront_a_round_and_a_chunk(n):
    depth, prob = cases.rough_frame(64, 48, 3)
    pos, nrm = cases.seeded_model(n, 100 + n)
    case = Case(pos, nrm, depth, prob, K_ROUGH, 1e-4)
    rec, m = case.check(cases.seeded_poses(5, 200 + n, xy=0.15), **PRM_ROUGH)
    assert rec["footprint"].all() and rec["agree"].sum() > 0


@pytest.mark.parametrize("W,H,K", [(1, 1, (1.0, 0.0, 1.0, 0.0)), (5, 7, (6.0, 2.0, 6.0, 3.0)), (33, 3, (30.0, 16.0, 30.0, 1.0)), (128, 1, (100.0, 63.5, 1.0, 0.0))])
def test_frames_whose_row_words_straddle_image_rows_and_end_in_padding(W, H, K):
    depth, prob = cases.rough_frame(W, H, 11)
    depth[depth == 0] = 5000                                                  # (a frame of one pixel must have a depth)
    pos, nrm = cases.seeded_model(65, 12)
    case = Case(pos, nrm, depth, prob, K, 1e-4)
    poses = np.stack([pose(cases.rot((1, 2, 3), 40), (0, 0, 0.5)), pose(t=(0.02, 0, 0.5)), pose(cases.rot((3, 1, 0), 100), (0, 0, 0.45)), pose(t=(0, 0.01, 0.55))])
    for claim in ("agree", "on_mask"):
        rec, m = case.check(poses, claim, point_radius=0.05, max_splat_px=8, tolerance=0.06, class_threshold=0.15)
        assert rec["footprint"].all() and rec["footprint"].max() <= W * H


def test_two_contexts_write_into_one_pool():
    from model_matching_amd.estimator import scene_row_words
    depth, prob = cases.rough_frame(64, 48, 31)
    a = Case(*cases.seeded_model(300, 32), depth, prob, K_ROUGH, 1e-4)
    pos_b, nrm_b = cases.seeded_model(130, 33)
    b = Case((pos_b * F(1.5)).astype(F), nrm_b, depth, cases.rough_frame(64, 48, 36)[1], K_ROUGH, 1e-4)   # its own class image
    Pa, Pb = cases.seeded_poses(5, 34, xy=0.12), cases.seeded_poses(4, 35, xy=0.12)
    pool = np.full((11, scene_row_words(depth.shape)), ONES, np.uint32)
    d = a.est.dev_alloc(pool.nbytes)
    a.est.dev_upload(d, pool)
    rb = b.est.scene_footprints(Pb, d, 6, 11, "on_mask", **PRM_ROUGH)         # the later slots first: the order of the calls plays no part
    ra = a.est.scene_footprints(Pa, d, 1, 11, "on_mask", **PRM_ROUGH)
    a.est.dev_download(d, pool)
    a.est.dev_free(d)
    wa, ma, _ = a.want(Pa, "on_mask", **PRM_ROUGH)
    wb, mb, _ = b.want(Pb, "on_mask", **PRM_ROUGH)
    assert ref.records_equal(ra, wa) and ref.records_equal(rb, wb) and wa["claimed"].sum() > 0 and wb["claimed"].sum() > 0
    assert np.array_equal(pool[1:6], ref.pack_rows(ma)) and np.array_equal(pool[6:10], ref.pack_rows(mb)) and (pool[[0, 10]] == ONES).all()


def test_chunks_batches_and_positions_do_not_change_a_bit(tmp_path):
    """n = 7 under STOCS_SCENE_CHUNK=3 in a child process equals the unchunked call, each pose alone, and the poses reversed"""
    import scene_child as child
    c = cases.chunk_case()
    est = child.make_est(c)
    w_rec, w_masks, _ = ref.footprints(c["poses"], c["pos"], c["nrm"], c["depth"], c["prob"], c["K"], c["scale"], "agree", **c["prm"])
    whole, rec = child.run(est, c, "agree")
    assert np.array_equal(whole, ref.pack_rows(w_masks)) and ref.records_equal(rec, w_rec)
    assert not whole[[2, 5]].any() and not any(rec[2].tolist()) and not any(rec[5].tolist()) and rec["claimed"][[0, 1, 3, 4, 6]].all()
    out = tmp_path / "chunked.npz"
    env = dict(os.environ, STOCS_SCENE_CHUNK="3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scene_child.py"), str(out), "agree"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    assert np.array_equal(got["rows"], whole) and np.array_equal(got["rec"], rec.view(np.int32).reshape(-1, 7))
    for h in range(7):
        row, one = child.run(est, c, "agree", c["poses"][h:h + 1])
        assert np.array_equal(row[0], whole[h]) and one[0] == rec[h]
    rev, rrec = child.run(est, c, "agree", c["poses"][::-1])
    assert np.array_equal(rev[::-1], whole) and np.array_equal(rrec[::-1], rec)


def test_capacity_edge_and_a_second_call_allocates_nothing():
    from model_matching_amd import capi
    L = capi.load()
    pos, nrm = cases.seeded_model(257, 12)
    depth, prob = cases.rough_frame(1024, 512, 11)
    case = Case(pos, nrm, depth, prob, (500.0, 511.5, 500.0, 255.5), 1e-4)
    poses = cases.seeded_poses(3, 13, xy=0.1)
    prm = dict(PRM_ROUGH, max_splat_px=8)
    rec, m = case.check(poses, explain=False, **prm)                          # 2^19 pixels: accepted
    assert rec["footprint"].all()
    d = case.est.dev_alloc(5 * 16384 * 4)
    case.est.scene_footprints(poses, d, 0, 5, **prm)
    a0 = L.stocs_device_alloc_count()
    again = case.est.scene_footprints(poses, d, 0, 5, **prm)
    fewer = case.est.scene_footprints(poses[:2], d, 3, 5, "on_mask", **prm)
    assert L.stocs_device_alloc_count() == a0 and again.tobytes() == rec.tobytes() and fewer["footprint"].tolist() == rec["footprint"][:2].tolist()
    d1, p1 = cases.rough_frame(1024, 513, 11)
    case.set_frame(d1, p1, (500.0, 511.5, 500.0, 256.0), 1e-4)
    q = capi.RenderParams(); L.stocs_default_render_params(C.byref(q))
    P, pP = capi.f32(poses)
    out = (capi.SceneRecord * 3)()
    assert L.stocs_scene_footprints(case.est.h, pP, 3, 0, 5, C.byref(q), 0, d, out) == -4
    case.est.dev_free(d)


def test_footprint_errors():
    from model_matching_amd import capi
    L = capi.load()
    pos, nrm = cases.seeded_model(65, 2)
    est = _est(pos, nrm)
    prm = capi.RenderParams(); L.stocs_default_render_params(C.byref(prm))
    out = (capi.SceneRecord * 2)()
    P, pP = capi.f32(cases.seeded_poses(2, 1))
    rows = est.dev_alloc(4 * ref.row_words(64 * 48) * 4)
    f = lambda h=est.h, pP=pP, n=2, b=0, s=4, q=prm, cl=0, r=rows, o=out: L.stocs_scene_footprints(h, pP, n, b, s, C.byref(q) if q is not None else None, cl, r, o)
    assert f() == -5 and f(n=-1) == -1 and f(n=0) == 0                          # no frame: STOCS_ERR_STATE; n == 0: a no-op whatever the state
    depth, prob = cases.rough_frame(64, 48, 7)
    est.set_frame(depth, prob, K_ROUGH, 1e-4)
    assert f() == 0 and f(b=2) == 0 and f(cl=1) == 0 and f(n=0, r=None) == 0
    assert f(n=-1) == -1 and f(pP=None) == -1 and f(q=None) == -1 and f(r=None) == -1 and f(o=None) == -1 and f(h=None) == -1
    assert f(cl=2) == -1 and f(cl=-1) == -1 and f(b=-1) == -1 and f(b=3) == -1 and f(s=1) == -1
    for k, v in (("point_radius", -1e-3), ("point_radius", float("nan")), ("max_splat_px", -1), ("max_splat_px", 17), ("tolerance", 0.0), ("tolerance", float("inf")),
                 ("class_threshold", float("nan"))):
        q = capi.RenderParams(); L.stocs_default_render_params(C.byref(q)); setattr(q, k, v)
        assert f(q=q) == -1, (k, v)
    with pytest.raises(ValueError):
        est.scene_footprints(P, rows, 0, 4, "behind")
    with pytest.raises(TypeError):
        est.scene_footprints(P, rows, 0, 4, cell_px=2)
    est.dev_free(rows)


# ---- the walk, on rows uploaded straight from numpy ----
@pytest.fixture(scope="module")
def walker():
    return _est(*cases.seeded_model(65, 2))


def _select(est, c):
    rows = ref.pack_rows(c["masks"])
    d = est.dev_alloc(max(rows.nbytes, 16))
    try:
        if rows.size:
            est.dev_upload(d, rows)
        return est.scene_select(d, (1, c["masks"].shape[1]), c["score"], c["group"], c["rec"].astype(ref.RECORD_DTYPE), c["cap"], n_groups=c["n_groups"], **c["params"])
    finally:
        est.dev_free(d)


def _same(got, want):
    return ref.records_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name", sorted(cases.hand_pools()))
def test_hand_built_pools(walker, name):
    c = cases.hand_pools()[name]
    got, want = _select(walker, c), cases.run_ref(c)
    assert _same(got, want), (got, want)
    if name in cases.EXPECT:
        assert got[0]["rank"].tolist() == cases.EXPECT[name][0] and got[0]["reason"].tolist() == cases.EXPECT[name][1]


def test_200_seeded_random_pools(walker):
    reasons = set()
    for seed in range(200):
        c = cases.random_pool(seed)
        got, want = _select(walker, c), cases.run_ref(c)
        assert _same(got, want), (seed, got, want)
        reasons |= set(got[0]["reason"].tolist())
    assert reasons == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("seed", range(3))
def test_the_two_entry_points_of_the_shared_walk_agree(walker, seed):
    """stocs_select_instances_rows and stocs_scene_select on the same sets (scene_cases.walk_pair): rank, own and exclusive per slot and
    the selected lists are equal -- to each other and, the references agreeing on these inputs, to both references"""
    import instances_ref
    rows, c = cases.walk_pair(seed)
    i_want, s_want = instances_ref.select(rows["hit"], rows["counted"], rows["lcp"], **rows["prm"]), cases.run_ref(c)
    assert all(np.array_equal(i_want[0][f], s_want[0][f]) for f in ("rank", "own", "exclusive")) and np.array_equal(i_want[1], s_want[1])
    i_rec, i_sel = walker.select_instances_rows(rows["hit"], rows["counted"], rows["lcp"], rows["nS"], **rows["prm"])
    s_rec, s_sel = _select(walker, c)
    for f in ("rank", "own", "exclusive"):
        assert np.array_equal(i_rec[f], s_rec[f]), (f, i_rec[f], s_rec[f])
    assert np.array_equal(i_sel, s_sel), (i_sel, s_sel)
    assert _same((s_rec, s_sel), s_want)


def test_select_n_0_a_second_call_and_the_errors(walker):
    from model_matching_amd import capi
    L = capi.load()
    est = walker
    tiny = est.dev_alloc(16)
    rec, sel = est.scene_select(tiny, (4, 4), np.zeros(0, F), np.zeros(0, np.int32), np.zeros(0, ref.RECORD_DTYPE))
    est.dev_free(tiny)
    assert len(rec) == 0 and len(sel) == 0
    c = cases.hand_pools()["every_reason"]
    n = len(c["score"])
    rows = ref.pack_rows(c["masks"])
    d = est.dev_alloc(rows.nbytes); est.dev_upload(d, rows)
    call = lambda m: est.scene_select(d, (1, 64), c["score"][:m], c["group"][:m], c["rec"][:m], c["cap"], n_groups=c["n_groups"], **c["params"])
    first = call(n)
    a0 = L.stocs_device_alloc_count()
    again, fewer = call(n), call(n - 2)
    assert L.stocs_device_alloc_count() == a0 and _same(first, again) and _same(first, cases.run_ref(c)) and len(fewer[0]) == n - 2
    prm = capi.SceneParams(); L.stocs_default_scene_params(C.byref(prm)); prm.min_pixels = 2
    sc, psc = capi.f32(c["score"]); gr, pgr = capi.i32(c["group"])
    rc = np.ascontiguousarray(c["rec"], ref.RECORD_DTYPE); prc = rc.ctypes.data_as(C.POINTER(capi.SceneRecord))
    cap, pcap = capi.i32(c["cap"])
    out = (capi.SceneResult * n)(); sel = (C.c_int32 * n)(); ns = C.c_int(-7)
    f = lambda h=est.h, r=d, n=n, W=64, H=1, s=psc, g=pgr, rec=prc, ng=3, cp=pcap, q=prm, o=out, sl=sel, k=ns: \
        L.stocs_scene_select(h, r, n, W, H, s, g, rec, ng, cp, C.byref(q) if q is not None else None, o, sl, C.byref(k) if k is not None else None)
    assert f() == 0 and ns.value == 3 and f(cp=None) == 0
    assert f(n=0) == 0 and ns.value == 0 and f(n=0, r=None, s=None, g=None, rec=None, o=None, sl=None) == 0
    assert f(h=None) == -1 and f(n=-1) == -1 and f(n=16385) == -1 and f(q=None) == -1 and f(k=None) == -1
    assert f(r=None) == -1 and f(s=None) == -1 and f(g=None) == -1 and f(rec=None) == -1 and f(o=None) == -1 and f(sl=None) == -1
    assert f(W=0) == -1 and f(H=0) == -1 and f(ng=0) == -1 and f(ng=1025) == -1 and f(ng=2) == -1      # ng = 2: group id 2 is outside 0 .. 1
    assert f(W=1024, H=513) == -4 and f(W=1024, H=513, n=0) == -4
    for bad in ([0, 5, 5], [1, -1, 5]):
        b, pb = capi.i32(bad)
        assert f(cp=pb) == -1
    g2, pg2 = capi.i32(np.where(np.arange(n) == 1, -1, c["group"]))
    assert f(g=pg2) == -1
    for k in ("footprint", "in_front", "claimed"):
        r2 = rc.copy(); r2[k][n - 1] = -1
        assert f(rec=r2.ctypes.data_as(C.POINTER(capi.SceneRecord))) == -1, k
    for k, v in (("max_selected", 0), ("min_pixels", 0), ("min_exclusive_fraction", 0.0), ("min_exclusive_fraction", 1.5), ("min_exclusive_fraction", float("nan")),
                 ("max_violation_fraction", -0.5), ("max_violation_fraction", 1.5), ("max_violation_fraction", float("nan"))):
        q = capi.SceneParams(); L.stocs_default_scene_params(C.byref(q)); setattr(q, k, v)
        assert f(q=q) == -1, (k, v)
    for k, v in (("min_exclusive_fraction", 1.0), ("max_violation_fraction", 0.0), ("max_violation_fraction", 1.0)):
        q = capi.SceneParams(); L.stocs_default_scene_params(C.byref(q)); setattr(q, k, v)
        assert f(q=q) == 0, (k, v)
    with pytest.raises(TypeError):
        est.scene_select(d, (1, 64), c["score"], c["group"], rc, tolerance=1.0)
    est.dev_free(d)


# ---- end to end ----
def test_select_scene_end_to_end():
    from model_matching_amd.estimator import select_scene
    s = cases.scene_of_two()
    ests = []
    for (pos, nrm), prob in zip(s["models"], s["probs"]):
        e = _est(pos, nrm)
        e.set_frame(s["depth"], prob, s["K"], s["scale"])
        ests.append(e)
    got = select_scene(ests, s["pools"], labels=True, min_pixels=20, **s["prm"])
    foot, masks = [], []
    for (pos, nrm), prob, poses in zip(s["models"], s["probs"], s["pools"]):
        r, m, _ = ref.footprints(poses, pos, nrm, s["depth"], prob, s["K"], s["scale"], **s["prm"])
        foot.append(r); masks.append(m)
    foot, masks = np.concatenate(foot), np.concatenate(masks)
    assert ref.records_equal(got["footprints"], foot)
    score = ref.default_score(foot)
    assert np.array_equal(got["score"].view(np.uint32), score.view(np.uint32)) and got["group"].tolist() == [0, 0, 0, 0, 1, 1] and got["index"].tolist() == [0, 1, 2, 3, 0, 1]
    rec, sel = ref.select(masks, score, got["group"], foot, 2, None, min_pixels=20)
    assert ref.records_equal(got["records"], rec) and np.array_equal(got["selected"], sel)
    assert sorted(sel.tolist()) == [0, 5] and rec["reason"].tolist() == [0, 2, 1, 2, 2, 0]      # the true poses; duplicates 2; the impostors 1 (free space) and 2
    H, W = s["depth"].shape
    zkey = rref.empty_keys(W, H)
    for k in sel.tolist():
        g, i = int(got["group"][k]), int(got["index"][k])
        rref.render(zkey, s["pools"][g][i], s["models"][g][0], s["models"][g][1], s["K"], W, H, k, **s["prm"])
    lab, st = rref.labels(zkey, s["depth"], s["probs"][0], s["scale"], **s["prm"])
    assert np.array_equal(got["labels"], lab) and np.array_equal(got["state"], st) and set(np.unique(lab)) == {-1, 0, 5}
    want = np.concatenate([rref.resolve(zkey, s["pools"][int(got["group"][k])][int(got["index"][k])], *s["models"][int(got["group"][k])], s["depth"],
                                        s["probs"][int(got["group"][k])], s["K"], s["scale"], k, **s["prm"]) for k in sel.tolist()])
    assert rref.records_equal(got["render"], want) and not want["hidden"].any()
    # caps and given scores reach the walk: with the duplicate scored above the true box and one instance per object, the duplicate is taken
    got2 = select_scene(ests, s["pools"], scores_per_object=[[0.5, 0.9, 0.1, 0.1], [0.2, 0.8]], max_per_object=1, min_pixels=20, **s["prm"])
    rec2, sel2 = ref.select(masks, np.array([0.5, 0.9, 0.1, 0.1, 0.2, 0.8], F), got["group"], foot, 2, [1, 1], min_pixels=20)
    assert ref.records_equal(got2["records"], rec2) and np.array_equal(got2["selected"], sel2) and sel2.tolist() == [1, 5] and "labels" not in got2
    with pytest.raises(TypeError):
        select_scene(ests, s["pools"], cell_px=3)


# ---- the driver ----
APP = os.path.join(ROOT, "model_matching_amd", "apps", "stocs_single")
PRE = os.path.join(ROOT, "model_matching_amd", "apps", "model_preprocess")
SCENE_LINE = re.compile(r"^scene (-?\d+): object (\w+) trial (\d+) score (\S+) own (\d+) exclusive (\d+) reason (\d)$")


def _write_two_object_tree(tmp_path):
    """a synthetic scene directory in the reference's layout from the committed data fixture: the bowl's frame, and two objects, a and b, that
    both carry the bowl's model and class image -- two objects that claim the same surface"""
    import shutil
    from PIL import Image
    raw = np.load(os.path.join(ROOT, "tests", "golden", "example_ycb_024_bowl_raw.npz"))
    scene = tmp_path / "scene"; (scene / "probability_maps").mkdir(parents=True)
    Image.fromarray(raw["depth"].astype(np.uint16)).save(scene / "depth.png")
    repo = tmp_path / "repo"
    adir = repo / "models" / "a"; adir.mkdir(parents=True)
    with open(adir / "textured_vertices.ply", "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment VCGLIB generated\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face 0\nproperty list uchar int vertex_indices\nend_header\n" % len(raw["model_raw"]))
        for p in raw["model_raw"]:
            f.write("%.9g %.9g %.9g \n" % (p[0], p[1], p[2]))
    pre = subprocess.run([PRE, "a", "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                          "--model-scale", repr(float(raw["model_scale"]))], capture_output=True, text=True, timeout=300)
    assert pre.returncode == 0, pre.stdout + pre.stderr
    shutil.copytree(adir, repo / "models" / "b")
    for obj in "ab":
        Image.fromarray(raw["prob"].astype(np.uint16)).save(scene / "probability_maps" / (obj + ".png"))
    return raw, scene, repo


def test_driver_scene_select(tmp_path):
    from model_matching_amd import capi
    from model_matching_amd.estimator import select_scene
    raw, scene, repo = _write_two_object_tree(tmp_path)
    K, scale = [float(x) for x in raw["K"]], float(raw["depth_scale"])
    base = [APP, str(scene), "a,b", "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(scale), "--seed", "7", "--trials", "2"]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    assert sorted(os.listdir(scene)) == ["best_pose_candidate_a.txt", "best_pose_candidate_b.txt", "depth.png", "probability_maps"]
    poses_plain = [(scene / ("best_pose_candidate_%s.txt" % o)).read_text() for o in "ab"]
    run = subprocess.run(base + ["--scene-select", "--masks"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    # without the flag: the lines of the run with it minus the scene lines, the same pose files, and neither the selection nor the label image
    timing = re.compile(r"total_microseconds=\d+")
    lines = [timing.sub("", ln) for ln in run.stdout.splitlines()]
    assert [ln for ln in lines if not ln.startswith("scene")] == [timing.sub("", ln) for ln in plain.stdout.splitlines()]
    assert not any(ln.startswith("scene") for ln in plain.stdout.splitlines()) and sum(ln.startswith("scene") for ln in lines) == 5
    assert sorted(os.listdir(scene)) == ["best_pose_candidate_a.txt", "best_pose_candidate_b.txt", "depth.png", "labels_scene.pgm", "probability_maps", "scene_selection.txt"]
    assert [(scene / ("best_pose_candidate_%s.txt" % o)).read_text() for o in "ab"] == poses_plain
    # the Python route from the poses the driver pooled, on the models it worked on
    rows = [ln.split() for ln in (scene / "scene_selection.txt").read_text().splitlines()]
    assert len(rows) == 4 and sorted((r[1], int(r[2])) for r in rows) == [("a", 0), ("a", 1), ("b", 0), ("b", 1)]
    pools = [np.zeros((2, 16), F), np.zeros((2, 16), F)]
    for r in rows:
        M = np.vstack([np.array(r[3:], np.float64).astype(F).reshape(3, 4), [0, 0, 0, 1]]).astype(F)
        pools["ab".index(r[1])][int(r[2])] = M.T.reshape(16)
    L = capi.load()
    ests = []
    for obj in "ab":
        n, hn = C.c_int(), C.c_int()
        mp = str(repo / "models" / obj / "model_search.ply").encode()
        assert L.stocs_ply_read(mp, None, None, 0, C.byref(n), C.byref(hn)) == 0
        mpos = np.zeros((n.value, 3), F); mnrm = np.zeros((n.value, 3), F)
        assert L.stocs_ply_read(mp, mpos.ctypes.data_as(capi._fp), mnrm.ctypes.data_as(capi._fp), n.value, C.byref(n), C.byref(hn)) == 0
        e = _est(mpos, mnrm)
        e.set_frame(raw["depth"], raw["prob"], K, scale)
        ests.append(e)
    want = select_scene(ests, pools, labels=True)
    order = want["selected"].tolist() + [h for h in range(4) if want["records"]["rank"][h] < 0]
    got = [SCENE_LINE.match(ln) for ln in run.stdout.splitlines() if ln.startswith("scene ") and not ln.startswith("scene: ")]
    assert len(got) == 4 and all(got)
    for m, r, h in zip(got, rows, order):
        rec = want["records"][h]
        assert (int(m.group(1)), m.group(2), int(m.group(3))) == (int(rec["rank"]), "ab"[want["group"][h]], int(want["index"][h])) == (int(r[0]), r[1], int(r[2]))
        assert F(float(m.group(4))) == want["score"][h] and (int(m.group(5)), int(m.group(6)), int(m.group(7))) == (int(rec["own"]), int(rec["exclusive"]), int(rec["reason"]))
    assert "scene: hypotheses=4 selected=%d" % len(want["selected"]) in run.stdout.splitlines()
    assert len(want["selected"]) >= 1 and want["footprints"]["footprint"].max() > 1000
    pgm = (scene / "labels_scene.pgm").read_bytes()
    head = b"P5\n640 480\n65535\n"
    assert pgm.startswith(head) and len(pgm) == len(head) + 640 * 480 * 2
    assert np.array_equal(np.frombuffer(pgm[len(head):], ">u2").reshape(480, 640).astype(np.int32), want["labels"] + 1)
    # the flag is refused where it does not apply
    for bad in ([APP, str(scene), "a", "--repo", str(repo), "--trials", "2", "--scene-select"], [APP, str(scene), "a,b", "--repo", str(repo), "--scene-select"],
                [APP, str(scene), "a,b", "--repo", str(repo), "--trials", "2", "--scene-max-per-object", "1"]):
        r = subprocess.run(bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--scene-select needs" in r.stderr
