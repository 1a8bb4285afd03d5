"""stocs_render_poses / stocs_render_resolve / stocs_render_labels / stocs_explain_poses on the GPU against the float32 restatement of their
contract (tests/render_ref.py): every comparison is array_equal on the records, the labels, the states and the downloaded key buffer.
Shapes are the smallest at which the kernels can go wrong: one point at the edges of the splat rule and of the image, models either
side of a wavefront, of a 256-point round and of the splat kernel's chunk, frames whose bitset words straddle rows, a frame of one
pixel, and the two sizes either side of the resolve kernel's capacity."""
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

import render_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
APP = os.path.join(ROOT, "model_matching_amd", "apps", "stocs_single")
PRE = os.path.join(ROOT, "model_matching_amd", "apps", "model_preprocess")
F = np.float32
EPS = float(2.0 ** -7)          # tolerance of the hand-built cases: a representable float
SCALE = float(2.0 ** -10)       # depth unit of the hand-built frames: raw 1024 is exactly 1 m
K64 = (32.0, 32.0, 32.0, 24.0)  # 64 x 48 camera, everything a power of two or a small integer
CHUNK = int(re.search(r"RENDER_CHUNK = (\d+)", open(os.path.join(ROOT, "model_matching_amd", "csrc", "render.hip")).read()).group(1))


def _est(model_pos, model_nrm):
    """a context around a model; the scene plays no part in rendering (a handful of points serves)"""
    from model_matching_amd.estimator import StocsEstimator
    rng = np.random.default_rng(1)
    sp = rng.normal(0, 0.05, (32, 3)).astype(F)
    sn = sp / np.linalg.norm(sp, axis=1, keepdims=True)
    return StocsEstimator(sp, sn, np.ones(32, F), None, np.asarray(model_pos, F).reshape(-1, 3), np.asarray(model_nrm, F).reshape(-1, 3), build_index=False)


def _keys(est, zkey, npix):
    out = np.zeros(npix, np.uint64)
    est.dev_download(zkey, out)
    return out


class Case:
    """one context + frame + a key buffer of its own; check() runs explain_poses AND the three steps and compares both with the restatement"""
    def __init__(self, mpos, mnrm, depth, prob, K, scale):
        self.mpos, self.mnrm, self.depth, self.prob, self.K, self.scale = np.asarray(mpos, F).reshape(-1, 3), np.asarray(mnrm, F).reshape(-1, 3), depth, prob, K, scale
        self.est = _est(self.mpos, self.mnrm)
        self.set_frame(depth, prob, K, scale)

    def set_frame(self, depth, prob, K, scale):
        self.depth, self.prob, self.K, self.scale = depth, prob, K, scale
        self.H, self.W = depth.shape
        self.est.set_frame(depth, prob, K, scale)
        self.zkey = self.est.dev_alloc(self.H * self.W * 8)

    def want(self, poses, **prm):
        return ref.explain(poses, self.mpos, self.mnrm, self.depth, self.prob, self.K, self.scale, **prm)

    def steps(self, poses, id_base=0, **prm):
        self.est.render_poses(poses, self.zkey, id_base, True, **prm)
        rec = self.est.render_resolve(poses, self.zkey, id_base, **prm)
        lab, st = self.est.render_labels(self.zkey, **prm)
        return rec, lab, st, _keys(self.est, self.zkey, self.H * self.W)

    def check(self, poses, **prm):
        poses = np.asarray(poses, F).reshape(-1, 16)
        w_rec, w_lab, w_st, w_key = self.want(poses, **prm)
        rec, lab, st, key = self.steps(poses, **prm)
        assert np.array_equal(key, w_key), np.flatnonzero(key != w_key)[:5]
        bad = [i for i in range(len(poses)) if not ref.records_equal(rec[i], w_rec[i])]
        assert not bad, (bad[:5], rec[bad[:5]], w_rec[bad[:5]])
        assert np.array_equal(lab, w_lab) and np.array_equal(st, w_st)
        e_rec, e_lab, e_st = self.est.explain_poses(poses, labels=True, **prm)     # the single-object form equals the three steps
        assert e_rec.tobytes() == rec.tobytes() and np.array_equal(e_lab, lab) and np.array_equal(e_st, st)
        assert self.est.explain_poses(poses, **prm).tobytes() == rec.tobytes()
        assert np.array_equal(rec["footprint"], rec["visible"] + rec["hidden"])
        assert np.array_equal(rec["visible"], rec["no_depth"] + rec["agree"] + rec["in_front"] + rec["behind"])
        return rec, lab, st


def _pose(R=None, t=(0, 0, 0)):
    P = np.eye(4)
    if R is not None:
        P[:3, :3] = R
    P[:3, 3] = t
    return P.T.reshape(16).astype(F)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def _counts(r):
    return tuple(int(r[c]) for c in ref.COUNTS)


def flat_frame(W, H, raw=1024):
    """a wall at raw depth units with a hole (no depth) at pixel (row 24, col 33), and a class image that is exactly at the 0.1 threshold at
    the centre pixel (raw 1000), just below it one column to the left (999), 1.0 elsewhere"""
    depth = np.full((H, W), raw, np.uint16)
    prob = np.full((H, W), 10000, np.uint16)
    depth[24, 33] = 0
    prob[24, 32] = 1000
    prob[24, 31] = 999
    return depth, prob


@pytest.fixture(scope="module")
def one_point():
    """ONE model point at the origin with normal (0, 0, -1): under the pose [I | t] p = t exactly, q = (0, 0, -1)"""
    depth, prob = flat_frame(64, 48)
    return Case([[0, 0, 0]], [[0, 0, -1]], depth, prob, K64, SCALE)


def test_one_point_splat_radius_at_its_edges(one_point):
    c = one_point
    P = _pose(t=(0, 0, 1))
    half = float(2.0 ** -6)                                                   # fx * r / z = 0.5 exactly: floor(1.0) = 1
    ulp1 = float(np.nextafter(F(half), F(0)))                                 # one ulp below: 0.5 - 2^-25, and the sum rounds to 1.0f: still 1
    below = float(np.nextafter(F(ulp1), F(0)))                                # two ulps below: the sum is 0.99999994f, floor 0
    far = _pose(t=(0, 0, float(np.nextafter(F(1), F(2)))))                    # the same from the depth side
    for prm, pose, foot in ((dict(point_radius=half), P, 9), (dict(point_radius=ulp1), P, 9), (dict(point_radius=below), P, 1), (dict(point_radius=half), far, 1), (dict(point_radius=0.0), P, 1),
                            (dict(point_radius=1.0, max_splat_px=16), P, 33 * 33), (dict(point_radius=1.0, max_splat_px=2), P, 25),
                            (dict(point_radius=1.0, max_splat_px=0), P, 1)):
        rec, lab, st = c.check([pose], tolerance=EPS, class_threshold=0.1, **prm)
        assert rec["footprint"][0] == foot == rec["visible"][0] == (lab == 0).sum(), prm
    rec, lab, st = c.check([P], tolerance=EPS, class_threshold=0.1, point_radius=half)
    assert np.array_equal(np.argwhere(lab == 0), [[r, q] for r in (23, 24, 25) for q in (31, 32, 33)])


def test_splats_are_clipped_at_the_image_border(one_point):
    c = one_point
    prm = dict(tolerance=EPS, class_threshold=0.1, point_radius=float(2.0 ** -6))   # s = 1 at z = 1
    for t, foot in (((-1.0, 0, 1), 6), ((31 / 32, 0, 1), 6), ((0, -24 / 32, 1), 6), ((0, 23 / 32, 1), 6), ((-1.0, -24 / 32, 1), 4), ((31 / 32, 23 / 32, 1), 4),
                    ((-33 / 32, 0, 1), 0), ((1.0, 0, 1), 0), ((0, -25 / 32, 1), 0), ((0, 24 / 32, 1), 0)):     # one pixel outside: nothing, though its square would reach in
        rec, lab, st = c.check([_pose(t=t)], **prm)
        assert rec["footprint"][0] == foot == (lab == 0).sum(), t


def test_two_hypotheses_over_the_same_pixel(one_point):
    c = one_point
    prm = dict(tolerance=EPS, class_threshold=0.1, point_radius=float(2.0 ** -6))
    near, far = _pose(t=(0, 0, 0.75)), _pose(t=(0, 0, 1))
    for poses, winner in (([near, far], 0), ([far, near], 1)):
        rec, lab, st = c.check(poses, **prm)
        assert rec["visible"][winner] == 9 and rec["hidden"][1 - winner] == 9 and rec["visible"][1 - winner] == 0 and set(np.unique(lab)) == {-1, winner}
    rec, lab, st = c.check([far, far], **prm)                                 # equal p_2 bits: the lower id
    assert rec["visible"].tolist() == [9, 0] and rec["hidden"].tolist() == [0, 9]
    npix = c.W * c.H
    for first, second in ((5, 2), (2, 5)):                                    # ... whatever its position among the calls; id_base non-zero
        c.est.render_poses([far], c.zkey, first, True, **prm)
        c.est.render_poses([far], c.zkey, second, False, **prm)
        key = _keys(c.est, c.zkey, npix)
        want = ref.render(ref.render(ref.empty_keys(c.W, c.H), far, c.mpos, c.mnrm, c.K, c.W, c.H, first, **prm), far, c.mpos, c.mnrm, c.K, c.W, c.H, second, **prm)
        assert np.array_equal(key, want) and set((key[key != ref.EMPTY] & np.uint64(0xFFFFFFFF)).tolist()) == {2}
        assert _counts(c.est.render_resolve([far], c.zkey, 2, **prm)[0])[:3] == (9, 9, 0) and _counts(c.est.render_resolve([far], c.zkey, 5, **prm)[0])[:3] == (9, 0, 9)
    # the largest ids: id_base + n == 2^31 - 1 passes, one more is refused
    from model_matching_amd import capi
    top = 2 ** 31 - 1 - 2
    c.est.render_poses([near, far], c.zkey, top, True, **prm)
    key = _keys(c.est, c.zkey, npix)
    assert np.array_equal(key, ref.render(ref.empty_keys(c.W, c.H), [near, far], c.mpos, c.mnrm, c.K, c.W, c.H, top, **prm))
    assert c.est.render_resolve([near, far], c.zkey, top, **prm)["visible"].tolist() == [9, 0]
    lab, _ = c.est.render_labels(c.zkey, **prm)
    assert set(np.unique(lab)) == {-1, top}
    with pytest.raises(capi.StocsError):
        c.est.render_poses([near, far], c.zkey, top + 1, True, **prm)
    with pytest.raises(capi.StocsError):
        c.est.render_resolve([near, far], c.zkey, top + 1, **prm)
    with pytest.raises(capi.StocsError):
        c.est.render_poses([near], c.zkey, -1, True, **prm)


UP = float(np.nextafter(F(1.0 + EPS), F(2.0)))
DN = float(np.nextafter(F(1.0 - EPS), F(0.0)))
# (name, translation, state of the one touched pixel) with point_radius 0, tolerance 2^-7, threshold 0.1 on flat_frame(64, 48)
CLASS_POINTS = [
    ("d = 0, class exactly at the threshold", (0, 0, 1), 2 + 16),
    ("class just below the threshold", (-1 / 32, 0, 1), 2),
    ("raw depth 0", (0.5 / 32, 0, 1), 1),
    ("d = +tolerance: agrees (inclusive)", (0, 0, 1.0 + EPS), 2 + 16),
    ("d = -tolerance: agrees (inclusive)", (0, 0, 1.0 - EPS), 2 + 16),
    ("d one ulp above +tolerance: behind", (0, 0, UP), 4),
    ("d one ulp below -tolerance: in front", (0, 0, DN), 3),
]


def test_classification_at_its_boundaries_from_the_keys_z(one_point):
    c = one_point
    for name, t, state in CLASS_POINTS:
        rec, lab, st = c.check([_pose(t=t)], tolerance=EPS, class_threshold=0.1, point_radius=0.0)
        assert st[lab == 0].tolist() == [state], name
        k = {1: "no_depth", 2: "agree", 3: "in_front", 4: "behind"}[state & 15]
        assert rec[k][0] == 1 and rec["on_mask"][0] == (state >> 4) and rec["visible"][0] == 1, name
    # no class image: on_mask nowhere, the rest stays
    c.set_frame(c.depth, None, K64, SCALE)
    rec, lab, st = c.check([_pose(t=t) for _, t, _ in CLASS_POINTS[3:]], tolerance=EPS, point_radius=0.0)
    assert not rec["on_mask"].any() and not (st & 16).any()
    c.set_frame(c.depth, flat_frame(64, 48)[1], K64, SCALE)


def seeded_model(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    pos = (u * np.array([0.06, 0.04, 0.03])).astype(F)
    nrm = (u / np.array([0.06, 0.04, 0.03])).astype(F)        # not unit: the context normalises
    return pos, nrm


def seeded_poses(n, seed, z=(0.3, 0.9), xy=0.25):
    rng = np.random.default_rng(seed)
    return np.stack([_pose(_rot(rng.normal(size=3), rng.uniform(0, 180)), (rng.uniform(-xy, xy), rng.uniform(-xy, xy), rng.uniform(*z))) for _ in range(n)])


def rough_frame(W, H, seed, raw=(3000, 9000)):
    rng = np.random.default_rng(seed)
    depth = rng.integers(raw[0], raw[1], (H, W)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.15] = 0
    prob = rng.integers(0, 3000, (H, W)).astype(np.uint16)
    return depth, prob


K_ROUGH = (60.0, 31.5, 60.0, 23.5)
PRM_ROUGH = dict(point_radius=0.01, max_splat_px=3, tolerance=0.05, class_threshold=0.15)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_model_sizes_either_side_of_a_wavefront_a_round_and_a_chunk(n):
    depth, prob = rough_frame(64, 48, 3)
    pos, nrm = seeded_model(n, 100 + n)
    case = Case(pos, nrm, depth, prob, K_ROUGH, 1e-4)
    rec, lab, st = case.check(seeded_poses(12, 200 + n, xy=0.15), **PRM_ROUGH)
    if n >= 255:
        assert all(rec[k].sum() > 0 for k in ref.COUNTS), rec


@pytest.mark.parametrize("W,H,K", [(37, 29, (40.0, 18.0, 40.0, 14.0)), (1, 1, (1.0, 0.0, 1.0, 0.0)), (1024, 512, (500.0, 511.5, 500.0, 255.5))])
def test_frame_sizes(W, H, K):
    """37 x 29: bitset words straddle rows; 1 x 1; 1024 x 512 = 2^19 pixels, the largest frame resolve takes"""
    depth, prob = rough_frame(W, H, 11)
    pos, nrm = seeded_model(257, 12)
    case = Case(pos, nrm, depth, prob, K, 1e-4)
    poses = seeded_poses(6, 13, xy=0.1) if W > 1 else np.stack([_pose(_rot((1, 2, 3), 40), (0, 0, 0.5)), _pose(t=(0.3, 0, 0.5)), _pose(_rot((3, 1, 0), 100), (0, 0, 0.4))])
    rec, lab, st = case.check(poses, **dict(PRM_ROUGH, max_splat_px=8))
    assert rec["footprint"].sum() > 0 and rec["hidden"].sum() > 0


def test_camera_640x480_and_batches_of_1_and_65():
    raw = np.load(os.path.join(GOLD, "example_ycb_024_bowl_raw.npz"))
    K = [float(x) for x in raw["K"]]
    pos, nrm = seeded_model(1025, 9)
    case = Case(pos, nrm, raw["depth"], raw["prob"], K, float(raw["depth_scale"]))
    poses = seeded_poses(65, 10, z=(0.5, 1.2))
    poses[20] = np.nan; poses[40] = 0
    rec, lab, st = case.check(poses)                                          # the library's defaults
    assert not any(_counts(rec[20])) and not any(_counts(rec[40])) and rec["footprint"][[19, 21, 39, 41]].all() and not np.isin(lab, (20, 40)).any()
    whole = _keys(case.est, case.zkey, case.W * case.H)
    # the neighbours of the invalid poses are what they are without them
    keep = [i for i in range(65) if i not in (20, 40)]
    case.est.render_poses(poses[0], case.zkey, 0, True)
    for i in keep[:0:-1]:                                                     # the same poses in reverse, one call each, every pose under its own id
        case.est.render_poses(poses[i], case.zkey, i, False)
    assert np.array_equal(_keys(case.est, case.zkey, case.W * case.H), whole)
    assert case.est.render_resolve(poses, case.zkey).tobytes() == rec.tobytes()
    one = case.check(poses[:1])[0]
    assert one["visible"][0] == one["footprint"][0] == rec["footprint"][0]


def test_capacity_one_pixel_above_2_to_the_19():
    """3 x 174 763 = 2^19 + 1 pixels: resolve and explain refuse, render and labels work"""
    from model_matching_amd import capi
    W, H = 3, 174763
    depth, prob = rough_frame(W, H, 21)
    pos, nrm = seeded_model(65, 22)
    case = Case(pos, nrm, depth, prob, (60.0, 1.0, 60.0, 87381.0), 1e-4)
    poses = np.stack([_pose(_rot((1, 0, 0), 20), (0, dy, 0.5)) for dy in (-100.0, 0.0, 0.02, 300.0)])
    prm = dict(PRM_ROUGH, max_splat_px=8)
    case.est.render_poses(poses, case.zkey, 3, True, **prm)
    key = _keys(case.est, case.zkey, W * H)
    want = ref.render(ref.empty_keys(W, H), poses, pos, nrm, case.K, W, H, 3, **prm)
    assert np.array_equal(key, want) and (key != ref.EMPTY).sum() > 20
    lab, st = case.est.render_labels(case.zkey, **prm)
    w_lab, w_st = ref.labels(want, depth, prob, 1e-4, **prm)
    assert np.array_equal(lab, w_lab) and np.array_equal(st, w_st)
    L = capi.load()
    p = capi.RenderParams(); L.stocs_default_render_params(C.byref(p))
    P, pP = capi.f32(poses)
    out = (capi.RenderResult * 4)()
    assert L.stocs_render_resolve(case.est.h, pP, 4, 3, C.byref(p), case.zkey, out) == -4
    assert L.stocs_explain_poses(case.est.h, pP, 4, C.byref(p), out, None, None) == -4


def test_two_contexts_share_one_buffer():
    depth, prob = rough_frame(64, 48, 31)
    a = Case(*seeded_model(300, 32), depth, prob, K_ROUGH, 1e-4)
    pos_b, nrm_b = seeded_model(130, 33)
    pos_b = (pos_b * F(1.5)).astype(F)
    b = Case(pos_b, nrm_b, depth, prob, K_ROUGH, 1e-4)
    Pa, Pb = seeded_poses(5, 34, xy=0.12), seeded_poses(4, 35, xy=0.12)
    z, npix, prm = a.zkey, 64 * 48, PRM_ROUGH
    want = ref.render(ref.empty_keys(64, 48), Pa, a.mpos, a.mnrm, K_ROUGH, 64, 48, 0, **prm)
    only_a = want.copy()
    ref.render(want, Pb, b.mpos, b.mnrm, K_ROUGH, 64, 48, 5, **prm)
    a.est.render_poses(Pa, z, 0, True, **prm)
    assert np.array_equal(_keys(a.est, z, npix), only_a)
    b.est.render_poses(Pb, z, 5, False, **prm)                                # clear = 0 accumulates
    ab = _keys(a.est, z, npix)
    b.est.render_poses(Pb, z, 5, True, **prm)                                 # clear = 1 forgets
    assert np.array_equal(_keys(b.est, z, npix), ref.render(ref.empty_keys(64, 48), Pb, b.mpos, b.mnrm, K_ROUGH, 64, 48, 5, **prm))
    a.est.render_poses(Pa, z, 0, False, **prm)
    ba = _keys(b.est, z, npix)
    assert np.array_equal(ab, want) and np.array_equal(ba, want)
    ra, rb = a.est.render_resolve(Pa, z, 0, **prm), b.est.render_resolve(Pb, z, 5, **prm)
    assert ref.records_equal(ra, ref.resolve(want, Pa, a.mpos, a.mnrm, depth, prob, K_ROUGH, 1e-4, 0, **prm))
    assert ref.records_equal(rb, ref.resolve(want, Pb, b.mpos, b.mnrm, depth, prob, K_ROUGH, 1e-4, 5, **prm))
    assert ra["hidden"].sum() > 0 and rb["hidden"].sum() > 0 and ra["visible"].sum() + rb["visible"].sum() == (want != ref.EMPTY).sum()
    w_lab, w_st = ref.labels(want, depth, prob, 1e-4, **prm)
    for est in (a.est, b.est):
        lab, st = est.render_labels(z, **prm)
        assert np.array_equal(lab, w_lab) and np.array_equal(st, w_st)
    assert lab.max() >= 5


def test_a_second_call_of_the_same_size_allocates_nothing():
    from model_matching_amd import capi
    depth, prob = rough_frame(64, 48, 41)
    case = Case(*seeded_model(257, 42), depth, prob, K_ROUGH, 1e-4)
    poses = seeded_poses(33, 43, xy=0.15)
    first = case.est.explain_poses(poses, labels=True, **PRM_ROUGH)
    L = capi.load()
    a0 = L.stocs_device_alloc_count()
    again = case.est.explain_poses(poses, labels=True, **PRM_ROUGH)
    fewer = case.est.explain_poses(poses[:7], **PRM_ROUGH)
    assert L.stocs_device_alloc_count() == a0
    assert all(np.array_equal(x, y) for x, y in zip(first, again)) and fewer.tobytes() != first[0][:7].tobytes()
    # n == 0: no records, and the all-empty label image when asked
    rec, lab, st = case.est.explain_poses(np.zeros((0, 16), F), labels=True)
    assert len(rec) == 0 and (lab == -1).all() and not st.any() and lab.shape == (48, 64)
    assert len(case.est.explain_poses(np.zeros((0, 16), F))) == 0


def _push(pose16, metres):
    """the pose moved along the view ray through its translation"""
    P = np.asarray(pose16, np.float64).copy()
    t = P[12:15]
    P[12:15] = t + metres * t / np.linalg.norm(t)
    return P.astype(F)


def test_ycb_example_fixture():
    """the 472-point model against its own depth and class image: the winner of a trial batch, the same pose pushed along its view ray either
    way and turned a little, rendered together"""
    from model_matching_amd.estimator import StocsEstimator
    d = np.load(os.path.join(GOLD, "example_ycb_024_bowl.npz"))
    raw = np.load(os.path.join(GOLD, "example_ycb_024_bowl_raw.npz"))
    K, scale = [float(x) for x in raw["K"]], float(raw["depth_scale"])
    est = StocsEstimator(d["scene_pos"], d["scene_nrm"], d["scene_prob"], d["scene_pixel"], d["model_pos"], d["model_nrm"], build_index=True)
    est.set_frame(raw["depth"], raw["prob"], K, scale)
    est.run_trials(list(range(7, 11)), 100, max_per_base=200, post=dict(maximum_pose_count=10))
    hyps = np.concatenate([est.trials_get_hypotheses(t) for t in range(4)])
    win = hyps["pose16"][int(np.argmax(hyps["lcp"]))]
    turned = (np.vstack([np.hstack([_rot((0, 0, 1), 10), np.zeros((3, 1))]), [0, 0, 0, 1]]) @ win.reshape(4, 4).T.astype(np.float64)).T.reshape(16).astype(F)
    poses = np.stack([_push(win, 0.03), win, _push(win, -0.03), turned, win])
    rec, lab, st = est.explain_poses(poses, labels=True)
    w_rec, w_lab, w_st, _ = ref.explain(poses, d["model_pos"], d["model_nrm"], raw["depth"], raw["prob"], K, scale)
    assert ref.records_equal(rec, w_rec) and np.array_equal(lab, w_lab) and np.array_equal(st, w_st)
    assert rec["footprint"][1] > 1000 and rec["visible"][4] == 0 and rec["visible"][2] > rec["visible"][0]   # the repeated winner loses every tie; the nearest pose shows most


def _write_example_tree(tmp_path, name):
    """the reference's directory layout rebuilt from the committed data fixtures (as tests/test_driver_gpu.py does)"""
    from PIL import Image
    raw = np.load(os.path.join(GOLD, "example_%s_raw.npz" % name))
    obj = name.split("_", 1)[1]
    scene = tmp_path / "scene"; (scene / "probability_maps").mkdir(parents=True)
    Image.fromarray(raw["depth"].astype(np.uint16)).save(scene / "depth.png")
    Image.fromarray(raw["prob"].astype(np.uint16)).save(scene / "probability_maps" / (obj + ".png"))
    mdir = tmp_path / "repo" / "models" / obj; mdir.mkdir(parents=True)
    with open(mdir / "textured_vertices.ply", "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment VCGLIB generated\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face 0\nproperty list uchar int vertex_indices\nend_header\n" % len(raw["model_raw"]))
        for p in raw["model_raw"]:
            f.write("%.9g %.9g %.9g \n" % (p[0], p[1], p[2]))
    return raw, obj, scene, tmp_path / "repo"


MASK_LINE = re.compile(r"^mask (\d+): footprint (\d+) visible (\d+) hidden (\d+) agree (\d+) in_front (\d+) behind (\d+) no_depth (\d+) on_mask (\d+)$")


def test_driver_masks(tmp_path):
    from model_matching_amd import capi
    raw, obj, scene, repo = _write_example_tree(tmp_path, "ycb_024_bowl")
    K, scale = [float(x) for x in raw["K"]], float(raw["depth_scale"])
    pre = subprocess.run([PRE, obj, "--repo", str(repo), "--voxel", repr(float(raw["model_voxel"])), "--normal-radius", repr(float(raw["normal_radius"])),
                          "--model-scale", repr(float(raw["model_scale"]))], capture_output=True, text=True, timeout=300)
    assert pre.returncode == 0, pre.stdout + pre.stderr
    runs = {}
    for name, extra in (("plain", []), ("masks", ["--masks"])):
        (tmp_path / name).mkdir()
        r = subprocess.run([APP, str(scene), obj, "--repo", str(repo), "--intrinsics", ",".join(repr(k) for k in K), "--depth-scale", repr(scale), "--seed", "7",
                            "--trials", "4", "--cluster", "1", "--instances", "4", "--out", str(tmp_path / name / "pose.txt")] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[name] = r.stdout.splitlines()
    # without the flag: the lines of the run with it minus the mask lines, and no label image
    timing = re.compile(r"total_microseconds=\d+")
    plain = [timing.sub("", ln) for ln in runs["plain"]]
    flagged = [timing.sub("", ln) for ln in runs["masks"]]
    assert [ln for ln in flagged if not ln.startswith("mask ")] == plain and not any(ln.startswith("mask ") for ln in plain)
    assert sorted(os.listdir(tmp_path / "plain")) == ["pose.txt", "pose_instances_%s.txt" % obj]
    assert sorted(os.listdir(tmp_path / "masks")) == ["labels_%s.pgm" % obj, "pose.txt", "pose_instances_%s.txt" % obj]
    assert (tmp_path / "plain" / ("pose_instances_%s.txt" % obj)).read_text() == (tmp_path / "masks" / ("pose_instances_%s.txt" % obj)).read_text()
    # the Python route from the poses the driver selected, on the model it worked on
    L = capi.load()
    n, hn = C.c_int(), C.c_int()
    mp = str(repo / "models" / obj / "model_search.ply").encode()
    assert L.stocs_ply_read(mp, None, None, 0, C.byref(n), C.byref(hn)) == 0
    mpos = np.zeros((n.value, 3), F); mnrm = np.zeros((n.value, 3), F)
    assert L.stocs_ply_read(mp, mpos.ctypes.data_as(capi._fp), mnrm.ctypes.data_as(capi._fp), n.value, C.byref(n), C.byref(hn)) == 0
    rows = np.array((tmp_path / "masks" / ("pose_instances_%s.txt" % obj)).read_text().split(), np.float64).astype(F).reshape(-1, 12)
    assert len(rows) >= 1
    poses = np.stack([np.vstack([r.reshape(3, 4), [0, 0, 0, 1]]).T.reshape(16) for r in rows]).astype(F)
    est = _est(mpos, mnrm)
    est.set_frame(raw["depth"], raw["prob"], K, scale)
    rec, lab, st = est.explain_poses(poses, labels=True)
    got = [MASK_LINE.match(ln) for ln in runs["masks"] if ln.startswith("mask ")]
    assert len(got) == len(rows) and all(got)
    for i, (m, r) in enumerate(zip(got, rec)):
        assert int(m.group(1)) == i
        assert tuple(int(m.group(2 + j)) for j in range(8)) == tuple(int(r[k]) for k in ("footprint", "visible", "hidden", "agree", "in_front", "behind", "no_depth", "on_mask"))
    pgm = (tmp_path / "masks" / ("labels_%s.pgm" % obj)).read_bytes()
    head = b"P5\n640 480\n65535\n"
    assert pgm.startswith(head) and len(pgm) == len(head) + 640 * 480 * 2
    img = np.frombuffer(pgm[len(head):], ">u2").reshape(480, 640).astype(np.int32)
    assert np.array_equal(img, lab + 1) and rec["footprint"][0] > 0
    # the flag is refused where it does not apply
    bad = subprocess.run([APP, str(scene), obj, "--repo", str(repo), "--trials", "4", "--cluster", "1", "--masks"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--masks needs" in bad.stderr


def test_errors():
    from model_matching_amd import capi
    L = capi.load()
    pos, nrm = seeded_model(65, 2)
    est = _est(pos, nrm)
    prm = capi.RenderParams(); L.stocs_default_render_params(C.byref(prm))
    out = (capi.RenderResult * 2)()
    P, pP = capi.f32(seeded_poses(2, 1))
    lab = np.zeros(64 * 48, np.int32); st = np.zeros(64 * 48, np.uint8)
    pl, ps = lab.ctypes.data_as(capi._ip), st.ctypes.data_as(capi._u8p)
    z = est.dev_alloc(64 * 48 * 8)
    calls = {
        "poses": lambda h=est.h, pP=pP, n=2, b=0, q=prm, z=z: L.stocs_render_poses(h, pP, n, b, C.byref(q) if q is not None else None, z, 1),
        "resolve": lambda h=est.h, pP=pP, n=2, b=0, q=prm, z=z, o=out: L.stocs_render_resolve(h, pP, n, b, C.byref(q) if q is not None else None, z, o),
        "explain": lambda h=est.h, pP=pP, n=2, b=0, q=prm, z=None, o=out: L.stocs_explain_poses(h, pP, n, C.byref(q) if q is not None else None, o, pl, ps),
    }
    for name, f in calls.items():
        assert f() == -5, name                                               # no frame: STOCS_ERR_STATE
        assert f(n=-1) == -1, name
    assert L.stocs_render_labels(est.h, z, C.byref(prm), pl, ps) == -5
    assert calls["poses"](n=0) == 0 and calls["resolve"](n=0) == 0           # n == 0: no-op, whatever the state
    assert L.stocs_explain_poses(est.h, pP, 0, C.byref(prm), out, None, None) == 0
    assert L.stocs_explain_poses(est.h, pP, 0, C.byref(prm), out, pl, ps) == -5   # the label image takes its size from the frame
    depth, prob = rough_frame(64, 48, 7)
    est.set_frame(depth, prob, K_ROUGH, 1e-4)
    for name, f in calls.items():
        assert f() == 0, name
        assert f(n=-1) == -1 and f(pP=None) == -1 and f(q=None) == -1, name
        assert f(b=-1) == -1 or name == "explain"
    assert calls["poses"](z=None) == -1 and calls["resolve"](z=None) == -1 and calls["resolve"](o=None) == -1 and calls["explain"](o=None) == -1
    assert L.stocs_render_labels(est.h, z, C.byref(prm), pl, ps) == 0 and L.stocs_render_labels(est.h, z, C.byref(prm), pl, None) == 0
    assert L.stocs_render_labels(est.h, None, C.byref(prm), pl, ps) == -1 and L.stocs_render_labels(est.h, z, None, pl, ps) == -1
    assert L.stocs_render_labels(est.h, z, C.byref(prm), None, ps) == -1
    bad = [("point_radius", -1e-3), ("point_radius", float("nan")), ("point_radius", float("inf")), ("max_splat_px", -1), ("max_splat_px", 17),
           ("tolerance", 0.0), ("tolerance", -1.0), ("tolerance", float("nan")), ("tolerance", float("inf")), ("class_threshold", float("nan")),
           ("class_threshold", float("inf"))]
    for k, v in bad:
        q = capi.RenderParams(); L.stocs_default_render_params(C.byref(q)); setattr(q, k, v)
        for name, f in calls.items():
            assert f(q=q) == -1, (name, k, v)
        assert L.stocs_render_labels(est.h, z, C.byref(q), pl, ps) == -1, (k, v)
    for k, v in (("point_radius", 0.0), ("max_splat_px", 0), ("max_splat_px", 16)):
        q = capi.RenderParams(); L.stocs_default_render_params(C.byref(q)); setattr(q, k, v)
        assert calls["explain"](q=q) == 0, (k, v)
    with pytest.raises(capi.StocsError):
        est.explain_poses(P, tolerance=0.0)
    with pytest.raises(TypeError):
        est.explain_poses(P, cell_px=2)
    # a new frame of another size is honoured: the label image, the records and the key buffer follow it
    d2, p2 = rough_frame(17, 9, 8)
    est.set_frame(d2, p2, (20.0, 8.0, 20.0, 4.0), 1e-4)
    rec, lab2, st2 = est.explain_poses(P, labels=True)
    w_rec, w_lab, w_st, _ = ref.explain(P, pos, nrm, d2, p2, (20.0, 8.0, 20.0, 4.0), 1e-4)
    assert lab2.shape == (9, 17) and ref.records_equal(rec, w_rec) and np.array_equal(lab2, w_lab) and np.array_equal(st2, w_st)
