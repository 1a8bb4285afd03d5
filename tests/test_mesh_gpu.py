"""stocs_ctx_set_mesh, stocs_render_depth_mesh and stocs_pose_errors_vsd_mesh on the GPU against the float32 numpy restatement of their
contract (tests/mesh_ref.py): z images equal bit for bit, records equal field for field.  Small shapes, chosen at the edges of the triangle
rule, of the kernel's work split (64 triangles per wavefront, 256 per workgroup, a lane's own box up to STOCS_MESH_SMALL_PX pixels, the
workgroup's boxes) and of the chunks of z-buffers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_cases as mc  # noqa: E402
import mesh_ref as ref  # noqa: E402
import vsd_cases as vc  # noqa: E402
import vsd_ref  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SCALE = vc.DEPTH_SCALE
TAUS10 = [F(0.005 * i) for i in range(1, 11)]
K64 = mc.K_EXACT                                # pixel (r, c) looks along (c / 64, r / 64, 1)
GROUP_PX = 8192                                 # mesh.hip: boxes above it go to the whole workgroup


def _est(pos=None, nrm=None):
    """an estimator whose model cloud is (pos, nrm), or a few points that nothing here reads"""
    from model_matching_amd.estimator import StocsEstimator
    rng = np.random.default_rng(1)
    sp = rng.normal(0, 0.05, (32, 3)).astype(F)
    sn = sp / np.linalg.norm(sp, axis=1, keepdims=True)
    if pos is None:
        pos, nrm = sp[:8], sn[:8]
    return StocsEstimator(sp, sn, np.ones(32, F), None, np.asarray(pos, F), np.asarray(nrm, F), build_index=False)


def _same_depth(got, want):
    assert got.dtype == want.dtype == F and got.shape == want.shape
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:4], [(got[tuple(b)], want[tuple(b)]) for b in bad[:4]])


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = [i for i in range(len(got)) if not ref.records_equal(got[i], want[i])]
    assert not bad, (bad[:4], got[bad[0]], want[bad[0]])


def _render(est, v, t, E, K, W, H):
    """the mesh and an empty frame go up, the images come back equal to the restatement's; returns them"""
    est.set_mesh(v, t)
    est.set_frame(vc.flat_frame(W, H, 0), None, K, SCALE)
    got = est.render_depth_mesh(E)
    _same_depth(got, ref.render_depth(E, v, t, K, W, H))
    return got


@pytest.fixture(scope="module")
def est():
    e = _est()
    yield e
    e.close()


def at(c, r, z=1.0):
    """the point at depth z that K64 projects onto column c, row r"""
    return (c / 64.0 * z, r / 64.0 * z, z)


# ---- single triangles ----

SINGLE = {
    "centres on an edge and on the vertices": (at(8, 2), at(8, 12), at(2, 7)),
    "a sliver thinner than a pixel": (at(3.2, 3.3), at(40.7, 30.1), at(40.9, 30.2)),
    "a sliver along a row of centres": (at(3, 9), at(50, 9), at(50, 9.001)),
    "zero area": (at(2, 2), at(12, 2), at(7, 2)),
    "edge-on to the camera": (at(5, 5, 1.0), at(20, 9, 1.0), at(5, 5, 2.0)),
    "a vertex at z = 1e-6f": (at(2, 2), at(12, 2), (0.1, 0.1, float(F(1e-6)))),
    "a vertex just above z = 1e-6f": (at(2, 2), at(12, 2), (1e-7, 1e-7, float(np.nextafter(F(1e-6), F(1))))),
    "a vertex behind the camera": (at(2, 2), at(12, 2), (0.1, 0.1, -0.5)),
    "off the left": (at(-30, 5), at(-8, 5), at(-30, 20)),
    "off the right": (at(70, 5), at(90, 5), at(70, 20)),
    "off the top": (at(5, -30), at(25, -30), at(5, -6)),
    "off the bottom": (at(5, 55), at(25, 55), at(5, 80)),
    "within the box margin of the left edge": (at(-2.5, 5), at(-1.5, 5), at(-2.5, 20)),
    "straddles the left": (at(-9, 5), at(11, 8), at(-4, 30)),
    "straddles the right": (at(55, 5), at(80, 8), at(60, 30)),
    "straddles the top": (at(5, -9), at(25, -4), at(9, 12)),
    "straddles the bottom": (at(5, 40), at(25, 44), at(9, 70)),
    "straddles a corner": (at(50, 40), at(90, 44), at(60, 70)),
    "tilted": (at(4.4, 3.1, 0.7), at(50.2, 9.9, 1.9), at(20.5, 40.3, 1.1)),
}


@pytest.mark.parametrize("name", list(SINGLE))
def test_single_triangles(est, name):
    v, t = mc.triangle(*SINGLE[name])
    z = _render(est, v, t, mc.IDENTITY, K64, 64, 48)[0]
    n = int((z > 0).sum())
    if name in ("zero area", "a vertex at z = 1e-6f", "a vertex behind the camera", "off the left", "off the right", "off the top", "off the bottom",
                "within the box margin of the left edge"):
        assert n == 0
    elif name == "centres on an edge and on the vertices":
        assert np.all(z[2:13, 8] == 1.0) and z[7, 2] == 1.0 and z[1, 8] == 0 and z[7, 1] == 0
    elif not name.startswith("a sliver") and name != "edge-on to the camera":
        assert n > 20


def test_a_repeated_index(est):
    v = np.array([at(2, 2), at(12, 2), at(2, 12)], F)
    for tri in ([0, 1, 1], [2, 2, 2], [0, 0, 1]):
        z = _render(est, v, np.array([tri], np.int32), mc.IDENTITY, K64, 64, 48)[0]
        assert not z.any()


@pytest.mark.parametrize("W, H", [(1, 1), (7, 5), (64, 48), (640, 480)])
def test_a_triangle_that_covers_the_whole_frame(est, W, H):
    """a lane's own box (1, 35 pixels), a wavefront's (3 072) and the workgroup's (307 200)"""
    v, t = mc.triangle(at(-10, -10, 1.0), at(3 * W + 10, -10, 1.5), at(-10, 3 * H + 10, 2.0))
    z = _render(est, v, t, mc.IDENTITY, K64, W, H)[0]
    assert np.all(z > 0)


@pytest.mark.parametrize("second", [(1, 0, 3), (0, 1, 3), (3, 1, 0)])
def test_two_triangles_on_a_shared_edge(est, second):
    """the edge 0-1 through pixel centres, walked by the second triangle in the opposite order and in the same: its pixels are hit
    through both, and no pixel of the quad is empty"""
    v = np.array([at(8, 2), at(8, 12), at(2, 7), at(14, 7)], F)
    z = _render(est, v, np.array([(0, 1, 2), second], np.int32), mc.IDENTITY, K64, 64, 48)[0]
    assert np.all(z[2:13, 8] == 1.0) and np.all(z[7, 2:15] == 1.0)
    for tri in ((0, 1, 2), second):
        assert np.all(_render(est, v, np.array([tri], np.int32), mc.IDENTITY, K64, 64, 48)[0][2:13, 8] == 1.0)


@pytest.mark.parametrize("dz", [0.0, 2.0 ** -23])
def test_equal_and_adjacent_depths_on_one_pixel(est, dz):
    """two frontal triangles over the same pixels at equal z and one ulp apart: the minimum is the nearer one's bits whatever the order"""
    tri = lambda z: [at(4, 4, z), at(30, 4, z), at(4, 30, z)]
    for za, zb in ((1.0, 1.0 + dz), (1.0 + dz, 1.0)):
        v = np.array(tri(za) + tri(zb), F)
        z = _render(est, v, np.array([(0, 1, 2), (3, 4, 5)], np.int32), mc.IDENTITY, K64, 64, 48)[0]
        assert z[10, 10] == 1.0 and set(np.unique(z[z > 0]).tolist()) == {1.0}


# ---- counts, box sizes, forms ----

@pytest.mark.parametrize("nt", [1, 63, 64, 65, 255, 256, 257])
def test_every_triangle_count(est, nt):
    """either side of a wavefront's 64 triangles and of a workgroup's 256"""
    v, t = mc.ellipsoid(2)
    W, H = 37, 29
    E = mc.random_poses(2, 300 + nt, z=0.8, spread=0.01)
    z = _render(est, v, t[:nt], E, vc.small_camera(W, H), W, H)
    assert nt < 63 or (z[0].any() and z[1].any())      # a single level-2 triangle is smaller than a pixel here


def _factors(area):
    """(w, h) with w * h == area, as square as they come (a triangle needs three pixels of a box's width to cover a centre)"""
    return next((w, area // w) for w in range(int(area ** 0.5), 3, -1) if area % w == 0)


@pytest.mark.parametrize("off", [-1, 0, 1])
def test_boxes_at_the_small_box_limit(est, off):
    """70 separate triangles whose clamped boxes hold STOCS_MESH_SMALL_PX - 1, that many and one more pixels"""
    from model_matching_amd import capi
    small = capi.load().stocs_mesh_small_px()
    w, h = _factors(small + off)
    W, H = 160, 128
    v, t = mc.grid_of_small_triangles(70, w, h, K64, W)
    g = ref.setup(mc.IDENTITY, v, t, K64, W, H)
    assert g["live"].all() and np.all((g["c_hi"] - g["c_lo"] + 1) * (g["r_hi"] - g["r_lo"] + 1) == small + off)
    z = _render(est, v, t, mc.IDENTITY, K64, W, H)[0]
    assert (z > 0).sum() >= 70


@pytest.fixture(scope="module")
def forms_want():
    """the level-3 Cm mesh on 160 x 120 and a box that fills a third of 256 x 192, three poses each: meshes, cameras and the
    restatement's images, computed once (read-only)"""
    out = {}
    W, H = 160, 120
    v, t = mc.cm_mesh(3)
    E = mc.random_poses(3, 11, z=0.8, spread=0.01)
    out["cm3"] = dict(v=v, t=t, E=E, K=vc.small_camera(W, H), W=W, H=H)
    W, H = 256, 192
    v, t = mc.box(0.3, 0.2, 0.1)
    E = mc.random_poses(3, 12, z=0.8, spread=0.01)
    out["box"] = dict(v=v, t=t, E=E, K=vc.small_camera(W, H), W=W, H=H)
    for g in out.values():
        g["want"] = ref.render_depth(g["E"], g["v"], g["t"], g["K"], g["W"], g["H"])
        g["want"].setflags(write=False)
    s = ref.setup(out["box"]["E"][0], out["box"]["v"], out["box"]["t"], out["box"]["K"], 256, 192)
    assert ((s["c_hi"] - s["c_lo"] + 1) * (s["r_hi"] - s["r_lo"] + 1))[s["live"]].max() > GROUP_PX      # the workgroup's path runs
    return out


@pytest.mark.parametrize("form", [a | b | c for a in (0, 1, 2) for b in (0, 4, 8) for c in (0, 16)])
@pytest.mark.parametrize("which", ["cm3", "box"])
def test_every_kernel_form_gives_the_same_image(est, forms_want, which, form, monkeypatch):
    """STOCS_MESH_FORM: lanes walk their own boxes (1), none does (2) or the box size decides; the atomic minimum behind a read of the
    stored depth (4), blind (8) or as the call's size decides; the largest boxes to the workgroup or to one wavefront (16)"""
    monkeypatch.setenv("STOCS_MESH_FORM", str(form))
    g = forms_want[which]
    est.set_mesh(g["v"], g["t"])
    est.set_frame(vc.flat_frame(g["W"], g["H"], 0), None, g["K"], SCALE)
    _same_depth(est.render_depth_mesh(g["E"]), g["want"])


def test_reversed_winding_gives_the_same_image(est, forms_want):
    """(i0, i2, i1) for every triangle, and for every second one alone: the library's image does not change by a bit"""
    g = forms_want["cm3"]
    est.set_frame(vc.flat_frame(g["W"], g["H"], 0), None, g["K"], SCALE)
    half = g["t"].copy(); half[::2] = half[::2][:, [0, 2, 1]]
    for t in (g["t"][:, [0, 2, 1]], half):
        est.set_mesh(g["v"], t)
        _same_depth(est.render_depth_mesh(g["E"]), g["want"])


# ---- records ----

@pytest.fixture(scope="module")
def rec(forms_want):
    """five estimates of the level-3 Cm mesh against one ground truth on 160 x 120, a frame that shows the ground truth in front of a
    wall, the restatement's z-buffers and records (read-only)"""
    g = forms_want["cm3"]
    W, H, K, v, t = g["W"], g["H"], g["K"], g["v"], g["t"]
    E = mc.random_poses(5, 21, z=0.8, spread=0.004)
    G = E[0].copy()
    off = vc.pose16(vc.translation(3.0, 0.0, 0.8))          # off the frame
    E = np.concatenate([E, off[None]])
    zG = ref.render_bits(G, v, t, K, W, H)
    frame = vc.raw_from_depth(np.where(zG != ref.EMPTY, ref.bits_to_depth(zG, W, H).reshape(-1), 1.0).reshape(H, W))
    frame.setflags(write=False)
    want = ref.pose_errors_vsd_mesh(E, G, v, t, frame, K, SCALE, TAUS10)
    want.setflags(write=False)
    return dict(W=W, H=H, K=K, v=v, t=t, E=E, G=G, zG=zG, frame=frame, want=want)


def _call(est, rec, E, G, taus=TAUS10, **prm):
    est.set_mesh(rec["v"], rec["t"])
    est.set_frame(rec.get("frame2", rec["frame"]), None, rec["K"], SCALE)
    return est.pose_errors_vsd_mesh(E, G, taus, **prm)


def test_records_with_one_and_with_n_ground_truths(est, rec):
    n = len(rec["E"])
    one = _call(est, rec, rec["E"], rec["G"])
    each = _call(est, rec, rec["E"], np.tile(rec["G"], (n, 1)))
    _same(one, rec["want"])
    _same(each, rec["want"])
    assert np.all(one["e"][0] == 0) and one["uni"][0] == one["inter"][0] == one["px_gt"][0] > 500 and one["valid"].all()     # estimate == ground truth
    assert one["px_est"][-1] == 0 and np.all(one["e"][-1][:10] == 1) and one["valid"][-1] == 1                                  # off the frame
    assert one["px_est"][1] > 500 and 0 < one["e"][1][0] <= 1
    for i in (1, 5):
        _same(_call(est, rec, rec["E"][i], rec["G"]), rec["want"][i:i + 1])          # a record does not depend on its batch


@pytest.mark.parametrize("chunk", ["1", "2", "3"])
def test_chunk_edges_change_nothing(est, rec, chunk, monkeypatch):
    monkeypatch.setenv("STOCS_VSD_CHUNK", chunk)
    _same(_call(est, rec, rec["E"][:5], rec["G"]), rec["want"][:5])
    _same(_call(est, rec, rec["E"][:5], np.tile(rec["G"], (5, 1))), rec["want"][:5])
    _same_depth(est.render_depth_mesh(rec["E"][:5]), ref.render_depth(rec["E"][:5], rec["v"], rec["t"], rec["K"], rec["W"], rec["H"]))


def test_invalid_poses_render_nothing_and_score_one(est, rec):
    E = np.stack([rec["E"][1]] * 6)
    E[1, 14] = np.nan; E[2, 0] = np.inf; E[3] = 0; E[4, 15] = np.nan; E[4, 3] = np.inf      # entries 3, 7, 11, 15 are not read
    G = np.stack([rec["G"]] * 6)
    G[5, 12] = -np.inf
    got = _call(est, rec, E, G)
    _same(got, ref.pose_errors_vsd_mesh(E, G, rec["v"], rec["t"], rec["frame"], rec["K"], SCALE, TAUS10))
    assert got["valid"].tolist() == [1, 0, 0, 0, 1, 0]
    assert got["px_est"][[1, 2, 3]].tolist() == [0, 0, 0] and got["px_gt"][5] == 0 and got["px_est"][4] == got["px_est"][0] > 0
    assert np.all(got["e"][[1, 2, 3, 5]][:, :10] == 1)
    z = est.render_depth_mesh(E)
    assert not z[1].any() and not z[2].any() and not z[3].any() and z[4].any()


def test_a_difference_equal_to_tau_counts_as_far(est, rec):
    zE = ref.render_bits(rec["E"][1], rec["v"], rec["t"], rec["K"], rec["W"], rec["H"])
    _, m = ref.compare(zE, rec["zG"], rec["frame"], rec["K"], SCALE, TAUS10)
    dd = np.sort(m["dd"][m["inter"]])
    assert len(dd) > 20
    t = dd[len(dd) // 2]
    assert t > 0
    taus = [np.nextafter(t, F(0)), t, np.nextafter(t, F(np.inf))]
    got = _call(est, rec, rec["E"][1], rec["G"], taus)
    _same(got, ref.pose_errors_vsd_mesh(rec["E"][1], rec["G"], rec["v"], rec["t"], rec["frame"], rec["K"], SCALE, taus))
    n_eq = int((dd == t).sum())
    assert got["far"][0][0] == got["far"][0][1] == got["far"][0][2] + n_eq and n_eq >= 1


def test_a_depth_exactly_delta_behind_the_frame_is_visible(est, rec):
    frame = rec["frame"].copy()
    zE = ref.render_bits(rec["E"][2], rec["v"], rec["t"], rec["K"], rec["W"], rec["H"])
    _, m = ref.compare(zE, rec["zG"], frame, rec["K"], SCALE, TAUS10)
    px = int(np.flatnonzero(m["pe"] & ~m["pg"])[3])        # an estimate-only pixel
    k = ref.pixel_k(rec["K"], rec["W"], rec["H"])[px]
    frame.reshape(-1)[px] = int(round((float(m["dE"][px]) - 0.004) / float(k) / SCALE))
    _, m = ref.compare(zE, rec["zG"], frame, rec["K"], SCALE, TAUS10)
    delta = F(m["dE"][px] - m["dS"][px])
    assert 0.003 < delta < 0.005
    vis = []
    r2 = dict(rec); r2["frame2"] = frame
    for d in (delta, np.nextafter(delta, F(0))):
        got = _call(est, r2, rec["E"][2], rec["G"], delta=float(d))
        _same(got, ref.pose_errors_vsd_mesh(rec["E"][2], rec["G"], rec["v"], rec["t"], frame, rec["K"], SCALE, TAUS10, delta=float(d)))
        _, md = ref.compare(zE, rec["zG"], frame, rec["K"], SCALE, TAUS10, delta=float(d))
        assert bool(md["visE"][px]) == (d == delta)
        vis.append(int(got["vis_est"][0]))
    assert vis[0] >= vis[1] + 1


def test_surfel_parameters_are_ignored(est, rec):
    from model_matching_amd import capi
    L = capi.load()
    est.set_mesh(rec["v"], rec["t"])
    est.set_frame(rec["frame"], None, rec["K"], SCALE)
    P, pP = capi.f32(rec["E"][:2]); G, pG = capi.f32(rec["G"])
    prm = capi.VsdParams(); L.stocs_default_vsd_params(C.byref(prm)); prm.n_tau = 10
    for i, t in enumerate(TAUS10):
        prm.tau[i] = float(t)
    prm.surfel_radius = float("nan"); prm.max_splat_px = -7
    out = (capi.VsdRecord * 2)()
    assert L.stocs_pose_errors_vsd_mesh(est.h, pP, 2, pG, 1, C.byref(prm), out) == 0
    _same(np.frombuffer(out, dtype=ref.DTYPE, count=2), rec["want"][:2])
    with pytest.raises(TypeError):
        est.pose_errors_vsd_mesh(rec["E"][:2], rec["G"], TAUS10, surfel_radius=0.01)


def test_call_timing_names_the_steps(est, rec):
    _call(est, rec, rec["E"][:3], rec["G"])
    steps = est.last_mesh_call_timing()
    assert [s[0] for s in steps[:3]] == ["stage and enqueue", "wait for the device", "records"] and all(s[1] >= 0 for s in steps)


# ---- state, errors, the surfel path ----

def test_state_and_argument_errors_in_the_documented_order(rec):
    from model_matching_amd import capi
    L = capi.load()
    pos, nrm = vc.ball_model(8, 3)
    e = _est(pos, nrm)
    P, pP = capi.f32(vc.ball_poses(2, 4))
    prm = capi.VsdParams(); L.stocs_default_vsd_params(C.byref(prm)); prm.n_tau = 1; prm.tau[0] = 0.01
    out = (capi.VsdRecord * 2)()
    D = np.zeros((2, 4, 4), F)
    pD = D.ctypes.data_as(capi._fp)
    STATE = L.stocs_depth_check_poses(e.h, pP, 1, C.byref(capi.DepthParams(0.01, 0.1, 0, 8, 0.01)), (capi.DepthResult * 1)())
    assert STATE not in (0, -1)
    v, t = mc.ellipsoid(0)
    vp, tp = v.ctypes.data_as(capi._fp), t.ctypes.data_as(capi._ip)
    assert e.mesh_info() == (0, 0)
    # no mesh comes before no frame
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, 2, pP, 1, C.byref(prm), out) == STATE and b"no mesh" in L.stocs_last_error()
    assert L.stocs_render_depth_mesh(e.h, pP, 2, pD) == STATE and b"no mesh" in L.stocs_last_error()
    # bad meshes leave no mesh behind
    bad = t.copy(); bad[3, 2] = len(v)
    assert L.stocs_ctx_set_mesh(e.h, vp, len(v), bad.ctypes.data_as(capi._ip), len(t)) == -1 and e.mesh_info() == (0, 0)
    nanv = v.copy(); nanv[1, 1] = np.nan
    assert L.stocs_ctx_set_mesh(e.h, nanv.ctypes.data_as(capi._fp), len(v), tp, len(t)) == -1
    assert L.stocs_ctx_set_mesh(e.h, None, len(v), tp, len(t)) == -1 and L.stocs_ctx_set_mesh(e.h, vp, len(v), None, len(t)) == -1
    assert L.stocs_ctx_set_mesh(e.h, vp, -1, tp, len(t)) == -1
    assert L.stocs_ctx_set_mesh(e.h, vp, 2 ** 24 + 1, tp, len(t)) not in (0, -1, STATE)
    e.set_mesh(v, t)
    assert e.mesh_info() == (len(v), len(t))
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, 2, pP, 1, C.byref(prm), out) == STATE and b"no frame" in L.stocs_last_error()
    assert L.stocs_render_depth_mesh(e.h, pP, 2, pD) == STATE
    e.set_frame(vc.flat_frame(4, 4, 0.8), None, vc.small_camera(4, 4), SCALE)
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, 2, pP, 1, C.byref(prm), out) == 0
    assert L.stocs_render_depth_mesh(e.h, pP, 2, pD) == 0
    # (a frame whose width * height differs from what was uploaded is the third STOCS_ERR_STATE of check_frame; stocs_ctx_set_frame sets
    # both together, so no call sequence reaches it)
    # the argument checks, in the order of stocs_pose_errors_vsd
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, 0, None, 0, None, None) == 0        # n == 0 looks at nothing else
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, -1, pP, 1, C.byref(prm), out) == -1
    assert L.stocs_pose_errors_vsd_mesh(e.h, None, 2, pP, 1, C.byref(prm), out) == -1
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, 2, None, 1, C.byref(prm), out) == -1
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, 2, pP, 1, None, out) == -1
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, 2, pP, 1, C.byref(prm), None) == -1
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, 2, pP, 0, C.byref(prm), out) == -1
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, 2, pP, 3, C.byref(prm), out) == -1
    prm.n_tau = 0
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, 2, pP, 1, C.byref(prm), out) == -1
    prm.n_tau = 1; prm.delta = 0.0
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, 2, pP, 1, C.byref(prm), out) == -1
    prm.delta = 0.015
    assert L.stocs_render_depth_mesh(e.h, pP, -1, pD) == -1 and L.stocs_render_depth_mesh(e.h, None, 2, pD) == -1 and L.stocs_render_depth_mesh(e.h, pP, 2, None) == -1
    assert L.stocs_render_depth_mesh(e.h, None, 0, None) == 0
    # nt == 0 drops the mesh, whatever else is passed
    assert L.stocs_ctx_set_mesh(e.h, None, 0, None, 0) == 0 and e.mesh_info() == (0, 0)
    assert L.stocs_pose_errors_vsd_mesh(e.h, pP, 2, pP, 1, C.byref(prm), out) == STATE and b"no mesh" in L.stocs_last_error()
    e.close()


def test_second_call_allocates_nothing_and_meshes_replace_each_other(est, rec):
    from model_matching_amd import capi
    L = capi.load()
    first = _call(est, rec, rec["E"], rec["G"])
    z1 = est.render_depth_mesh(rec["E"][:3])
    v0, t0 = mc.ellipsoid(1)
    a0 = L.stocs_device_alloc_count()
    again = _call(est, rec, rec["E"], rec["G"])              # sets the same mesh again
    z2 = est.render_depth_mesh(rec["E"][:3])
    est.set_mesh(v0, t0)                                     # a smaller mesh in between
    z_small = est.render_depth_mesh(rec["E"][:3])
    fewer = _call(est, rec, rec["E"][:4], np.tile(rec["G"], (4, 1)))
    assert L.stocs_device_alloc_count() == a0
    assert again.tobytes() == first.tobytes() and z1.tobytes() == z2.tobytes()
    _same(fewer, rec["want"][:4])
    _same_depth(z_small, ref.render_depth(rec["E"][:3], v0, t0, rec["K"], rec["W"], rec["H"]))


def test_the_surfel_path_is_left_alone(rec):
    """after mesh calls on the same context, stocs_render_depth and stocs_pose_errors_vsd (surfels) still equal vsd_ref"""
    pos, nrm = vc.ball_model(257, 7)
    e = _est(pos, nrm)
    W, H = 64, 48
    K = vc.small_camera(W, H)
    E = vc.ball_poses(4, 8)
    zG = vsd_ref.render_depth(E[:1], pos, nrm, K, W, H, surfel_radius=0.01)[0]
    frame = vc.raw_from_depth(np.where(zG > 0, zG, 1.0))
    e.set_frame(frame, None, K, SCALE)
    e.set_mesh(rec["v"], rec["t"])
    mesh_first = e.pose_errors_vsd_mesh(E, E[0], TAUS10)
    _same(mesh_first, ref.pose_errors_vsd_mesh(E, E[0], rec["v"], rec["t"], frame, K, SCALE, TAUS10))
    _same_depth(e.render_depth(E, surfel_radius=0.01), vsd_ref.render_depth(E, pos, nrm, K, W, H, surfel_radius=0.01))
    _same(e.pose_errors_vsd(E, E[0], TAUS10, surfel_radius=0.01), vsd_ref.pose_errors_vsd(E, E[0], pos, nrm, frame, K, SCALE, TAUS10, surfel_radius=0.01))
    _same(e.pose_errors_vsd_mesh(E, E[0], TAUS10), mesh_first)
    e.close()
