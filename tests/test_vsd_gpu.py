"""stocs_render_depth and stocs_pose_errors_vsd on the GPU against the float32 numpy restatement of their contract (tests/vsd_ref.py):
z images equal bit for bit, records equal field for field.  Small shapes, chosen at the edges of the surfel rule, of the compare and of
the kernel's work split (64 points per wavefront, STOCS_VSD_POINTS = 256 per workgroup, chunks of z-buffers)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depth_check_ref as dref  # noqa: E402
import vsd_cases as vc  # noqa: E402
import vsd_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SCALE = vc.DEPTH_SCALE
TAUS10 = [F(0.005 * i) for i in range(1, 11)]
K_EXACT = (128.0, 32.0, 128.0, 24.0)          # 64 x 48: powers of two and a principal point on a pixel, so that a ray's numbers are exact


def _est(pos, nrm):
    from model_matching_amd.estimator import StocsEstimator
    m = np.asarray(pos, F).reshape(-1, 3)
    k = np.asarray(nrm, F).reshape(-1, 3)
    rng = np.random.default_rng(1)
    sp = rng.normal(0, 0.05, (32, 3)).astype(F)
    sn = sp / np.linalg.norm(sp, axis=1, keepdims=True)
    return StocsEstimator(sp, sn, np.ones(32, F), None, m, k, build_index=False)


def _same_depth(got, want):
    assert got.dtype == want.dtype == F and got.shape == want.shape
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:4], [(got[tuple(b)], want[tuple(b)]) for b in bad[:4]])


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = [i for i in range(len(got)) if not ref.records_equal(got[i], want[i])]
    assert not bad, (bad[:4], got[bad[0]], want[bad[0]])


def _check(est, pos, nrm, E, G, frame, K, taus=TAUS10, **prm):
    """the frame goes up, then both entry points against the restatement; returns the library's records"""
    H, W = frame.shape
    est.set_frame(frame, None, K, SCALE)
    E = np.asarray(E, F).reshape(-1, 16)
    rp = {k: v for k, v in prm.items() if k != "delta"}
    _same_depth(est.render_depth(E, **rp), ref.render_depth(E, pos, nrm, K, W, H, **rp))
    got = est.pose_errors_vsd(E, G, taus, **prm)
    _same(got, ref.pose_errors_vsd(E, G, pos, nrm, frame, K, SCALE, taus, **prm))
    return got


def _frontal(x, y, z):
    return vc.pose16(vc.translation(x, y, z))


# ---- one surfel ----

@pytest.fixture(scope="module")
def disc():
    """one model point at the origin whose normal looks down -z: under a pure translation a disc that faces the camera (read-only)"""
    pos, nrm = vc.one_surfel((0, 0, 0), (0, 0, -1))
    est = _est(pos, nrm)
    yield est, pos, nrm
    est.close()


@pytest.mark.parametrize("radius, cap, s", [(0.002, 16, 0), (0.01, 16, 1), (0.2, 16, 16), (0.2, 3, 3), (0.2, 0, 0)])
def test_square_half_width_zero_one_and_at_the_cap(disc, radius, cap, s):
    est, pos, nrm = disc
    frame = vc.flat_frame(64, 48, 0)
    P = _frontal(0, 0, 1.0)                                # projects onto pixel (24, 32) exactly
    assert int(min(np.floor(F(128.0) * F(radius) / F(1.0) + F(0.5)), cap)) == s
    _check(est, pos, nrm, P, P, frame, K_EXACT, surfel_radius=radius, max_splat_px=cap)
    z = est.render_depth(P, surfel_radius=radius, max_splat_px=cap)[0]
    rows, cols = np.nonzero(z)
    assert z[24, 32] == 1.0 and rows.max() - 24 == s and 32 - cols.min() == s      # the disc is wider than its square in every case


def test_a_pixel_exactly_on_the_rim(disc):
    """the disc at z = 1 seen through fx = 128: pixel (24, 35) has ex = 3 / 128 exactly, so with surfel_radius = 3 / 128 its squared
    distance equals r^2 (hit), one ulp less misses it, one ulp more hits it"""
    est, pos, nrm = disc
    est.set_frame(vc.flat_frame(64, 48, 0), None, K_EXACT, SCALE)
    P = _frontal(0, 0, 1.0)
    r = F(3.0 / 128.0)
    for radius, hit in ((r, True), (np.nextafter(r, F(0)), False), (np.nextafter(r, F(1)), True)):
        want = ref.render_depth(P, pos, nrm, K_EXACT, 64, 48, surfel_radius=radius)
        assert (want[0, 24, 35] == 1.0) == hit and (want[0, 24, 29] == 1.0) == hit and want[0, 24, 34] == 1.0 and want[0, 24, 36] == 0.0
        _same_depth(est.render_depth(P, surfel_radius=radius), want)


def test_discs_seen_edge_on(disc):
    """the disc turned about y until the camera sees it edge-on: dn near 0 on either side, dn >= 0 for the pixels beyond the plane"""
    est, pos, nrm = disc
    E = []
    for deg in (60.0, 85.0, 89.0, 89.9, 89.99, 90.0, 90.01, 90.1, 91.0, 95.0, 120.0):
        for x in (-0.1, 0.0, 0.1):
            T = vc.translation(x, 0.01, 0.8)
            T[:3, :3] = vc.rot((0, 1, 0), deg)
            E.append(vc.pose16(T))
    E = np.stack(E)
    got = _check(est, pos, nrm, E, E[0], vc.flat_frame(64, 48, 0), K_EXACT, surfel_radius=0.03)
    assert (got["px_est"] > 0).any() and (got["px_est"] == 0).any()


def test_discs_clipped_at_every_border(disc):
    est, pos, nrm = disc
    z = 0.8
    at = lambda col, row: _frontal((col - 32.0) / 128.0 * z, (row - 24.0) / 128.0 * z, z)
    E = np.stack([at(c, r) for c in (0, 1, 31, 62, 63) for r in (0, 1, 23, 46, 47)] + [at(-0.4, 10), at(63.4, 10), at(10, -0.4), at(10, 47.4), at(-0.6, 10), at(64, 10)])
    got = _check(est, pos, nrm, E, E[12], vc.flat_frame(64, 48, 0), K_EXACT, surfel_radius=0.03)      # s = 5
    assert (got["px_est"][:25] > 0).all() and got["px_est"][0] < got["px_est"][12]
    assert got["px_est"][-2:].tolist() == [0, 0]           # projected outside the image: not in_image, nothing rendered


@pytest.mark.parametrize("dz", [0.0, 2.0 ** -23])
def test_two_surfels_over_one_pixel(dz):
    """two frontal discs over the same pixels at equal z and one ulp apart: the minimum is the nearer one's bits whatever the order"""
    pos = np.array([(0, 0, dz), (0.004, 0, 0), (0.008, 0, dz)], F)
    nrm = np.tile(np.array((0, 0, -1), F), (3, 1))
    est = _est(pos, nrm)
    P = _frontal(0, 0, 1.0)
    _check(est, pos, nrm, P, P, vc.flat_frame(64, 48, 0), K_EXACT, surfel_radius=0.02)
    z = est.render_depth(P, surfel_radius=0.02)[0]
    est.close()
    assert z[24, 32] == 1.0 and set(np.unique(z[z > 0]).tolist()) == ({1.0} if dz == 0 else {1.0, float(F(1.0) + F(dz))})


# ---- model sizes, frames ----

@pytest.mark.parametrize("M", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_every_model_size(M):
    """either side of a wavefront's 64 points and of a workgroup's STOCS_VSD_POINTS = 256, and several workgroups"""
    pos, nrm = vc.ball_model(M, 100 + M)
    est = _est(pos, nrm)
    W, H = 37, 29
    K = vc.small_camera(W, H)
    E = vc.ball_poses(3, 200 + M)
    zG = ref.render_depth(E[:1], pos, nrm, K, W, H, surfel_radius=0.02)[0]
    frame = vc.raw_from_depth(np.where(zG > 0, zG, 1.2))
    got = _check(est, pos, nrm, E, E[0], frame, K, surfel_radius=0.02)
    est.close()
    assert got["px_gt"][0] > 0 and np.all(got["e"][0] == 0)


@pytest.fixture(scope="module")
def ball():
    """a ball of 257 points, 65 poses of it, an estimator (read-only)"""
    pos, nrm = vc.ball_model(257, 7)
    est = _est(pos, nrm)
    E = vc.ball_poses(65, 8)
    yield dict(est=est, pos=pos, nrm=nrm, E=E)
    est.close()


@pytest.mark.parametrize("W, H, K", [(1, 1, (2.0, 0.02, 2.0, -0.03)), (37, 29, None), (64, 48, None)])
def test_frames(ball, W, H, K):
    K = K or vc.small_camera(W, H)
    rng = np.random.default_rng(W)
    E, G = ball["E"][:4], ball["E"][4:8]
    zG = ref.render_depth(G[:1], ball["pos"], ball["nrm"], K, W, H, surfel_radius=0.01)[0]
    frame = vc.raw_from_depth(np.where(zG > 0, zG, 0.9) + rng.normal(0, 0.01, (H, W)))      # some pixels occlude, some are behind
    frame[rng.random((H, W)) < 0.1] = 0
    got = _check(ball["est"], ball["pos"], ball["nrm"], E, G, frame, K, surfel_radius=0.01)
    assert got["px_est"].all() and got["px_gt"].all()


def test_cm_at_vga_against_itself():
    pos, nrm = vc.cm_model()
    est = _est(pos, nrm)
    P = vc.cm_pose()
    z = ref.render_depth(P, pos, nrm, vc.YCB_K, 640, 480)[0]
    frame = vc.raw_from_depth(np.where(z > 0, z, 1.5))
    got = _check(est, pos, nrm, P, P, frame, vc.YCB_K, None)      # taus None: BOP's, from the model's diameter
    est.close()
    assert got["uni"][0] == got["inter"][0] == got["px_gt"][0] > 30000 and np.all(got["e"][0] == 0) and got["valid"][0] == 1


# ---- the compare's edges ----

@pytest.fixture(scope="module")
def edge(ball):
    """an estimate beside its ground truth on 64 x 48, a frame that shows the ground truth in front of a wall, the restatement's masks"""
    W, H = 64, 48
    K = vc.small_camera(W, H)
    E, G = ball["E"][0], ball["E"][1]
    kn = dref.unit_normals(ball["nrm"])
    zE = ref.render_bits(E, ball["pos"], kn, K, W, H, surfel_radius=0.01)
    zG = ref.render_bits(G, ball["pos"], kn, K, W, H, surfel_radius=0.01)
    frame = vc.raw_from_depth(np.where(zG != ref.EMPTY, ref.bits_to_depth(zG, W, H).reshape(-1), 1.0).reshape(H, W))
    frame.setflags(write=False)
    return dict(W=W, H=H, K=K, E=E, G=G, zE=zE, zG=zG, frame=frame)


def test_a_difference_equal_to_tau_counts_as_far(ball, edge):
    _, m = ref.compare(edge["zE"], edge["zG"], edge["frame"], edge["K"], SCALE, TAUS10)
    dd = np.sort(m["dd"][m["inter"]])
    assert len(dd) > 20
    t = dd[len(dd) // 2]                                   # the difference at one pixel, as a tau
    assert t > 0
    taus = [np.nextafter(t, F(0)), t, np.nextafter(t, F(np.inf))]
    got = _check(ball["est"], ball["pos"], ball["nrm"], edge["E"], edge["G"], edge["frame"], edge["K"], taus, surfel_radius=0.01)
    n_eq = int((dd == t).sum())
    assert got["far"][0][0] == got["far"][0][1] == got["far"][0][2] + n_eq and n_eq >= 1


def test_a_depth_exactly_delta_behind_the_frame_is_visible(ball, edge):
    """the frame's raw value at one pixel of the estimate is chosen from the restatement's dE so that dE - dS is a few millimetres; that
    difference itself is then the delta: the pixel is visible at it and hidden one ulp below"""
    frame = edge["frame"].copy()
    _, m = ref.compare(edge["zE"], edge["zG"], frame, edge["K"], SCALE, TAUS10)
    px = int(np.flatnonzero(m["pe"] & ~m["pg"])[3])        # an estimate-only pixel
    k = ref.pixel_k(edge["K"], edge["W"], edge["H"])[px]
    frame.reshape(-1)[px] = int(round((float(m["dE"][px]) - 0.004) / float(k) / SCALE))
    _, m = ref.compare(edge["zE"], edge["zG"], frame, edge["K"], SCALE, TAUS10)
    delta = F(m["dE"][px] - m["dS"][px])
    assert 0.003 < delta < 0.005
    vis = []
    for d in (delta, np.nextafter(delta, F(0))):
        got = _check(ball["est"], ball["pos"], ball["nrm"], edge["E"], edge["G"], frame, edge["K"], delta=float(d), surfel_radius=0.01)
        _, md = ref.compare(edge["zE"], edge["zG"], frame, edge["K"], SCALE, TAUS10, delta=float(d))
        assert bool(md["visE"][px]) == (d == delta)
        vis.append(int(got["vis_est"][0]))
    assert vis[0] >= vis[1] + 1


def test_pixels_without_a_measurement(ball, edge):
    frame = edge["frame"].copy()
    frame[:, ::2] = 0
    got = _check(ball["est"], ball["pos"], ball["nrm"], edge["E"], edge["G"], frame, edge["K"], surfel_radius=0.01)
    frame[:] = 0
    all0 = _check(ball["est"], ball["pos"], ball["nrm"], edge["E"], edge["G"], frame, edge["K"], surfel_radius=0.01)
    assert all0["vis_est"][0] == all0["px_est"][0] == got["px_est"][0] and all0["vis_gt"][0] == all0["px_gt"][0]


@pytest.mark.parametrize("n_tau", [1, 16])
def test_one_tau_and_sixteen(ball, edge, n_tau):
    taus = [F(0.0005 * (i + 1)) for i in range(n_tau)]
    got = _check(ball["est"], ball["pos"], ball["nrm"], edge["E"], edge["G"], edge["frame"], edge["K"], taus, surfel_radius=0.01)
    assert np.all(np.diff(got["far"][0][:n_tau]) <= 0) and np.all(got["far"][0][n_tau:] == 0) and np.all(got["e"][0][n_tau:] == 0)
    assert got["far"][0][0] > 0


# ---- batches, chunks, invalid poses ----

@pytest.fixture(scope="module")
def batch(ball, edge):
    """65 estimates against one ground truth on the edge frame: the restatement's records, computed once (read-only)"""
    want = ref.pose_errors_vsd(ball["E"], edge["G"], ball["pos"], ball["nrm"], edge["frame"], edge["K"], SCALE, TAUS10, surfel_radius=0.01)
    want.setflags(write=False)
    return want


def _call(ball, edge, E, G):
    ball["est"].set_frame(edge["frame"], None, edge["K"], SCALE)
    return ball["est"].pose_errors_vsd(E, G, TAUS10, surfel_radius=0.01)


@pytest.mark.parametrize("n", [1, 2, 65])
def test_batches_with_one_and_with_n_ground_truths(ball, edge, batch, n):
    one = _call(ball, edge, ball["E"][:n], edge["G"])
    each = _call(ball, edge, ball["E"][:n], np.tile(edge["G"], (n, 1)))
    _same(one, batch[:n])
    _same(each, batch[:n])


def test_a_record_does_not_depend_on_its_batch(ball, edge, batch):
    for i in (0, 31, 64):
        _same(_call(ball, edge, ball["E"][i], edge["G"]), batch[i:i + 1])
    rev = _call(ball, edge, ball["E"][::-1], edge["G"])
    _same(rev, batch[::-1])


@pytest.mark.parametrize("chunk", ["1", "2", "3", "7", "64"])
def test_chunk_edges_change_nothing(ball, edge, batch, chunk, monkeypatch):
    """STOCS_VSD_CHUNK=<poses>: chunk edges inside the batch; with one ground truth every chunk after the first compares against a
    buffer rendered before it, with n ground truths an odd size is rounded down to whole pairs (1: one pair)"""
    monkeypatch.setenv("STOCS_VSD_CHUNK", chunk)
    n = 9
    _same(_call(ball, edge, ball["E"][:n], edge["G"]), batch[:n])
    _same(_call(ball, edge, ball["E"][:n], np.tile(edge["G"], (n, 1))), batch[:n])
    want = ref.render_depth(ball["E"][:5], ball["pos"], ball["nrm"], edge["K"], edge["W"], edge["H"], surfel_radius=0.01)
    _same_depth(ball["est"].render_depth(ball["E"][:5], surfel_radius=0.01), want)


@pytest.mark.parametrize("form", ["0", "1", "2", "3", "4", "5"])
def test_every_kernel_form_gives_the_same_records(ball, edge, batch, form, monkeypatch):
    """STOCS_VSD_FORM: the compare over the pair's bounding rectangle (0) or whole frames (1), the atomic minimum behind a read of the
    stored depth (4), blind (2) or as the call's size decides (0); with poses that render nothing on either side of a pair"""
    monkeypatch.setenv("STOCS_VSD_FORM", form)
    _same(_call(ball, edge, ball["E"][:9], edge["G"]), batch[:9])
    E = np.stack([ball["E"][0], np.zeros(16, F), ball["E"][2], np.zeros(16, F)])
    G = np.stack([edge["G"], edge["G"], np.full(16, np.nan, F), np.zeros(16, F)])
    got = _check(ball["est"], ball["pos"], ball["nrm"], E, G, edge["frame"], edge["K"], surfel_radius=0.01)
    assert got["uni"][3] == 0 and got["px_est"][2] > 0 and got["px_gt"][2] == 0 and np.all(got["e"][3][:10] == 1)


def test_invalid_poses_render_nothing_and_score_one(ball, edge):
    E = np.stack([ball["E"][0]] * 6)
    E[1, 14] = np.nan; E[2, 0] = np.inf; E[3] = 0; E[4, 15] = np.nan; E[4, 3] = np.inf      # entries 3, 7, 11, 15 are not read
    G = np.stack([edge["G"]] * 6)
    G[5, 12] = -np.inf
    got = _check(ball["est"], ball["pos"], ball["nrm"], E, G, edge["frame"], edge["K"], surfel_radius=0.01)
    assert got["valid"].tolist() == [1, 0, 0, 0, 1, 0]
    assert got["px_est"][[1, 2, 3]].tolist() == [0, 0, 0] and got["px_gt"][5] == 0 and got["px_est"][4] == got["px_est"][0] > 0
    assert np.all(got["e"][[1, 2, 3, 5]][:, :10] == 1)


def test_second_call_allocates_nothing(ball, edge, batch):
    from model_matching_amd import capi
    L = capi.load()
    first = _call(ball, edge, ball["E"], edge["G"])
    z1 = ball["est"].render_depth(ball["E"][:8], surfel_radius=0.01)
    a0 = L.stocs_device_alloc_count()
    again = _call(ball, edge, ball["E"], edge["G"])
    fewer = _call(ball, edge, ball["E"][:5], np.tile(edge["G"], (5, 1)))
    z2 = ball["est"].render_depth(ball["E"][:8], surfel_radius=0.01)
    assert L.stocs_device_alloc_count() == a0
    assert again.tobytes() == first.tobytes() and z1.tobytes() == z2.tobytes()
    _same(fewer, batch[:5])


def test_call_timing_names_the_steps(ball, edge):
    _call(ball, edge, ball["E"][:3], edge["G"])
    from model_matching_amd import capi
    L = capi.load()
    labels = (C.c_char_p * 18)(); ms = (C.c_double * 18)(); n = C.c_int(0)
    assert L.stocs_last_call_timing(ball["est"].h, 7, labels, ms, 18, C.byref(n)) == 0
    names = [labels[i].decode() for i in range(n.value)]
    assert names[:3] == ["stage and enqueue", "wait for the device", "records"] and all(ms[i] >= 0 for i in range(n.value))
    assert L.stocs_last_call_timing(ball["est"].h, 8, labels, ms, 18, C.byref(n)) == -1


def test_state_and_argument_errors():
    from model_matching_amd import capi
    L = capi.load()
    pos, nrm = vc.ball_model(8, 3)
    est = _est(pos, nrm)
    P, pP = capi.f32(vc.ball_poses(2, 4))
    prm = capi.VsdParams(); L.stocs_default_vsd_params(C.byref(prm)); prm.n_tau = 1; prm.tau[0] = 0.01
    out = (capi.VsdRecord * 2)()
    D = np.zeros((2, 4, 4), F)
    STATE = L.stocs_depth_check_poses(est.h, pP, 1, C.byref(capi.DepthParams(0.01, 0.1, 0, 8, 0.01)), (capi.DepthResult * 1)())
    assert STATE != 0 and STATE != -1                       # the depth check's own answer without a frame: STOCS_ERR_STATE
    assert L.stocs_pose_errors_vsd(est.h, pP, 2, pP, 1, C.byref(prm), out) == STATE and b"no frame" in L.stocs_last_error()
    assert L.stocs_render_depth(est.h, pP, 2, C.byref(prm), D.ctypes.data_as(capi._fp)) == STATE
    est.set_frame(vc.flat_frame(4, 4, 0.8), None, vc.small_camera(4, 4), SCALE)
    assert L.stocs_pose_errors_vsd(est.h, pP, 2, pP, 1, C.byref(prm), out) == 0
    assert L.stocs_pose_errors_vsd(est.h, pP, 0, None, 0, None, None) == 0        # n == 0 looks at nothing else
    assert L.stocs_pose_errors_vsd(est.h, pP, -1, pP, 1, C.byref(prm), out) == -1
    assert L.stocs_pose_errors_vsd(est.h, None, 2, pP, 1, C.byref(prm), out) == -1
    assert L.stocs_pose_errors_vsd(est.h, pP, 2, None, 1, C.byref(prm), out) == -1
    assert L.stocs_pose_errors_vsd(est.h, pP, 2, pP, 1, None, out) == -1
    assert L.stocs_pose_errors_vsd(est.h, pP, 2, pP, 1, C.byref(prm), None) == -1
    assert L.stocs_pose_errors_vsd(est.h, pP, 2, pP, 0, C.byref(prm), out) == -1
    assert L.stocs_pose_errors_vsd(est.h, pP, 2, pP, 3, C.byref(prm), out) == -1
    prm.n_tau = 0
    assert L.stocs_pose_errors_vsd(est.h, pP, 2, pP, 1, C.byref(prm), out) == -1
    assert L.stocs_render_depth(est.h, pP, 2, C.byref(prm), D.ctypes.data_as(capi._fp)) == 0      # the renderer reads no tau
    prm.surfel_radius = 0.0
    assert L.stocs_render_depth(est.h, pP, 2, C.byref(prm), D.ctypes.data_as(capi._fp)) == -1
    assert L.stocs_render_depth(est.h, pP, 2, None, D.ctypes.data_as(capi._fp)) == -1
    assert L.stocs_render_depth(est.h, pP, 2, C.byref(prm), None) == -1
    assert L.stocs_render_depth(est.h, pP, -1, C.byref(prm), None) == -1
    with pytest.raises(TypeError):
        est.pose_errors_vsd(P, P[0], [0.01], tolerance=0.1)
    est.close()
