"""Scene ingest and model preprocessing (ingest.hip) against the numpy restatement (oracle/ingest_oracle.py) at their edges: frame
sizes either side of the own leaf sort's 65 536-point start, far and saturated depths, empty and nearly empty frames, depth steps at
the gradient normals' 50-unit test, grazing planes, off-centre and anisotropic cameras, leaf sizes whose leaves outgrow
centroid_kernel, class-threshold equality, several objects per frame, and models that take the own sort, the long-leaf kernel with
normals and 64-bit leaf keys.  Every case is built here from the committed raw frames and models or from seeded synthesis; which
branch of ingest.hip each one reaches is computed on the host from its inputs and asserted (test_the_cases_reach_every_branch)."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LONG_LEAF = 192          # STOCS_LONG_LEAF in ingest.hip: longer leaves go to centroid_long_kernel
OWN_SORT_MIN = 65536     # voxel_grid_device: the library's own leaf sort from this many points on (32-bit keys)


@functools.lru_cache(maxsize=None)
def _raw(name):
    r = np.load(os.path.join(GOLD, "example_%s_raw.npz" % name))
    return {k: r[k] for k in r.files}


FRAMES = {"lm": "linemod_obj_06", "pd": "packed_dove", "ycb": "ycb_024_bowl"}


def _synthetic(kind):
    H, W = 120, 160
    jj = np.arange(W)[None, :].repeat(H, 0)
    if kind == "steps":    # vertical bands at 800 + k * step for the four steps either side of the bilateral test
        d = np.full((H, W), 800, np.int64)
        for b, step in enumerate((49, 50, -49, -50)):
            d[:, 20 + 35 * b:20 + 35 * b + 17] += step
        d[40:80, :] += (jj[40:80] // 7) * 49          # and a staircase of 49-unit steps
    elif kind == "grazing":  # a plane seen at 80-85 degrees: depth rises 9 raw units (mm) per column, a column is 0.8-3 mm wide
        d = 500 + 9 * jj + (np.arange(H)[:, None] // 3)
        return d.astype(np.uint16), np.full((H, W), 10000, np.uint16), np.array([600.0, 80.0, 600.0, 60.0])
    else:
        raise ValueError(kind)
    return d.astype(np.uint16), np.full((H, W), 10000, np.uint16), np.array([200.0, 80.0, 200.0, 60.0])


def _corner_patches(d, v):
    d = d.copy()
    d[:20, :20] = v
    d[-20:, -20:] = v
    return d


def _case_inputs(c):
    """(depth u16, prob u16, K, depth_scale, voxel, threshold) of a scene case (a dict, see SCENE_CASES)."""
    if c["frame"] in FRAMES:
        r = _raw(FRAMES[c["frame"]])
        depth, prob, K, scale = r["depth"].copy(), r["prob"].copy(), r["K"].astype(np.float64).copy(), float(r["depth_scale"])
    else:
        depth, prob, K = _synthetic(c["frame"])
        scale = 0.001
    if "crop" in c:
        r0, c0, h, w = c["crop"]
        depth, prob = depth[r0:r0 + h, c0:c0 + w].copy(), prob[r0:r0 + h, c0:c0 + w].copy()
        K[1] -= c0; K[3] -= r0
    if "up" in c:                      # nearest-neighbour upscale, intrinsics scaled to match
        h, w = c["up"]
        h0, w0 = depth.shape
        ri = (np.arange(h) * h0) // h; ci = (np.arange(w) * w0) // w
        depth, prob = depth[ri][:, ci].copy(), prob[ri][:, ci].copy()
        K = np.array([K[0] * w / w0, K[1] * w / w0, K[2] * h / h0, K[3] * h / h0])
    e = c.get("edit")
    if e is not None:
        kind, v = e
        if kind == "far":
            depth = _corner_patches(depth, v)
        elif kind == "zero":
            depth[:] = 0
        elif kind == "one":
            keep = depth[v]; depth[:] = 0; depth[v] = keep if keep else 700
        elif kind == "salt":
            depth[np.random.default_rng(v).random(depth.shape) < 0.1] = 0
        elif kind == "prob":          # 999 / 1000 / 1001 in a checkerboard of 3-pixel stripes, around threshold 0.1
            prob = (999 + ((np.arange(depth.size).reshape(depth.shape) // 3) % 3)).astype(np.uint16)
        elif kind == "prob_full":
            prob[:] = 10000
        else:
            raise ValueError(kind)
    if "scale" in c:
        scale = c["scale"]
    if "K" in c:
        K = np.array(c["K"](K), np.float64)
    return depth, prob, [float(x) for x in K], scale, c.get("voxel", 0.005), c.get("thr", 0.10)


SCENE_CASES = [
    # frame sizes (crops of the real frames; rows x columns)
    dict(frame="lm", crop=(88, 385, 11, 13)),
    dict(frame="pd", crop=(230, 470, 97, 61)),
    dict(frame="ycb", crop=(100, 200, 255, 257)),
    dict(frame="lm", crop=(0, 260, 256, 256)),
    dict(frame="pd", crop=(150, 380, 257, 256)),
    dict(frame="lm", voxel=0.02),
    dict(frame="lm", up=(720, 1280)),
    dict(frame="ycb", up=(1080, 1920)),
    # depth content
    dict(frame="lm", edit=("far", 4000)),
    dict(frame="lm", edit=("far", 10000)),
    dict(frame="lm", edit=("far", 20000)),
    dict(frame="lm", edit=("far", 65535)),
    dict(frame="ycb", edit=("far", 65535), scale=0.0001),
    dict(frame="pd", crop=(230, 470, 97, 61), edit=("zero", 0)),
    dict(frame="lm", crop=(150, 250, 64, 80), edit=("one", (30, 40))),
    dict(frame="ycb", edit=("salt", 7)),
    dict(frame="steps"),
    dict(frame="grazing"),
    # camera
    dict(frame="lm", scale=0.000125),
    dict(frame="lm", crop=(0, 260, 256, 256), scale=0.0001),
    dict(frame="pd", scale=0.001),
    dict(frame="lm", K=lambda K: [K[0], -40.0, K[2], 600.0]),
    dict(frame="lm", crop=(0, 260, 256, 256), K=lambda K: [K[0], K[1] + 37.3, K[2] * 0.8, K[3] - 21.6]),
    dict(frame="ycb", K=lambda K: [K[0] * 1.3, K[1], K[2] * 0.7, K[3]]),
    # leaf size
    dict(frame="ycb", voxel=0.002),
    dict(frame="pd", voxel=0.01),
    dict(frame="pd", voxel=0.02),
    # class probability
    dict(frame="lm", edit=("prob", 0)),
    dict(frame="ycb", crop=(100, 200, 255, 257), thr=0.0),
    dict(frame="ycb", crop=(100, 200, 255, 257), thr=1.0),
    dict(frame="pd", edit=("prob_full", 0), thr=1.0),
]


def _case_id(c):
    parts = [c["frame"]]
    for k in ("crop", "up", "edit", "scale", "voxel", "thr"):
        if k in c:
            parts.append("%s=%s" % (k, c[k]))
    if "K" in c:
        parts.append("K=custom")
    return ",".join(str(p).replace(" ", "") for p in parts)


def _describe(c, method):
    depth, prob, K, scale, voxel, thr = _case_inputs(c)
    return "case %s: %dx%d, depth_scale %g, K %s, voxel %g, threshold %g, normal_method %d" % (
        _case_id(c), depth.shape[0], depth.shape[1], scale, ["%.4f" % k for k in K], voxel, thr, method)


@functools.lru_cache(maxsize=None)
def _oracle_scene(ci, method):
    from oracle.ingest_oracle import ingest_scene as ref
    depth, prob, K, scale, voxel, thr = _case_inputs(SCENE_CASES[ci])
    return ref(depth, prob, K, scale, voxel, thr, normal_method=method)


@functools.lru_cache(maxsize=None)
def _plane_fit_detail(ci):
    """The oracle's plane-fit smallest eigenvalue per pixel, and the back-projected points (for the excusals)."""
    from oracle.ingest_oracle import depth_normals
    depth, prob, K, scale, voxel, thr = _case_inputs(SCENE_CASES[ci])
    P = _backproject(depth, K, scale)
    return depth_normals(P, P[..., 2] > 0)[1], P


def _backproject(depth, K, scale):
    fx, cx, fy, cy = (np.float32(v) for v in K)
    d = depth.astype(np.float32) * np.float32(scale)
    H, W = d.shape
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    return np.stack([(jj - np.float64(cx)) * d / np.float64(fx), (ii - np.float64(cy)) * d / np.float64(fy), d], axis=-1).astype(np.float32)


def _window_cov(P, row, col):
    H, W, _ = P.shape
    q = P[max(0, row - 2):row + 3, max(0, col - 2):col + 3].reshape(-1, 3).astype(np.float64)
    q = q[q[:, 2] > 0]
    m = q.mean(0)
    return (q.T @ q) / len(q) - np.outer(m, m)


def _keys(pos, pix):
    return [(a.tobytes(), tuple(b)) for a, b in zip(np.ascontiguousarray(pos), pix.tolist())]


def _compare_scene(what, got, ref, method, detail=None):
    """The bars of test_ingest_gpu.py: the same points in the same order, positions / probabilities / pixels bit for bit, gradient normals
    within 2e-6, plane-fit normals within 1e-6.  Plane-fit only, each checked: a point whose pixel's smallest eigenvalue is within
    rounding of the 1e-5 cut may be on one side only; a normal whose window has two smallest eigenvalues within 1e-12 must be unit length,
    in that null space and face the camera; one whose n . p is within rounding of 0 may come out negated.  Returns the excusal count."""
    pos, nrm, prob, pix = got
    rpos, rnrm, rprob, rpix = ref
    excused = 0
    if len(pos) != len(rpos) or not np.array_equal(pix, rpix) or not np.array_equal(pos, rpos):
        assert method == 1, "%s: the clouds differ (%d points against the oracle's %d)" % (what, len(pos), len(rpos))
        w0, P = detail
        gk, rk = _keys(pos, pix), _keys(rpos, rpix)
        gs, rs = set(gk), set(rk)
        for k in gs ^ rs:
            row, col = k[1]
            assert abs(w0[row, col] - 1e-5) < 1e-12, "%s: point at pixel %s only on one side; smallest eigenvalue %.17g is not at the cut" % (
                what, k[1], w0[row, col])
            excused += 1
        gi = [i for i, k in enumerate(gk) if k in rs]
        ri = [i for i, k in enumerate(rk) if k in gs]
        assert [gk[i] for i in gi] == [rk[i] for i in ri], "%s: the common points are in another order" % what
        pos, nrm, prob, pix = pos[gi], nrm[gi], prob[gi], pix[gi]
        rpos, rnrm, rprob, rpix = rpos[ri], rnrm[ri], rprob[ri], rpix[ri]
    assert np.array_equal(pos, rpos), what
    assert np.array_equal(prob, rprob) and np.array_equal(pix, rpix), what
    if len(pos) == 0:
        return excused
    err = np.abs(nrm.astype(np.float64) - rnrm.astype(np.float64)).max(1)
    tol = 2e-6 if method == 0 else 1e-6
    bad = np.flatnonzero(~(err < tol))
    if len(bad):
        assert method == 1, "%s: %d gradient normals off by up to %.3g (first at pixel %s)" % (what, len(bad), err.max(), pix[bad[0]].tolist())
        w0, P = detail
        for i in bad:
            row, col = pix[i]
            p = P[row, col].astype(np.float64)
            n, rn = nrm[i].astype(np.float64), rnrm[i].astype(np.float64)
            C = _window_cov(P, row, col)
            w = np.linalg.eigvalsh(C)
            if w[1] - w[0] < 1e-12:
                assert abs(np.linalg.norm(n) - 1) < 1e-5 and n @ C @ n <= w[1] + 1e-12 and n @ p <= 0, \
                    "%s: degenerate window at pixel %s: the normal %s is not a unit null vector facing the camera" % (what, (row, col), n)
            else:
                assert abs(rn @ p) <= 1e-6 * np.linalg.norm(p) and np.abs(n + rn).max() < tol, \
                    "%s: normal at pixel %s off by %.3g (eigenvalues %s, n.p %.3g)" % (what, (row, col), err[i], w, rn @ p)
            excused += 1
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-5, what
    assert pos[:, 2].min() > 0 and pos[:, 2].max() <= 2.0, what
    return excused


def _excusal_bound(n):
    return 2 + n // 5000


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("ci", range(len(SCENE_CASES)), ids=[_case_id(c) for c in SCENE_CASES])
def test_scene_ingest_edges_equal_the_restatement(ci, method):
    from model_matching_amd.estimator import ingest_scene
    c = SCENE_CASES[ci]
    depth, prob, K, scale, voxel, thr = _case_inputs(c)
    what = _describe(c, method)
    got = ingest_scene(depth, prob, K, scale, voxel, thr, normal_method=method)
    ref = _oracle_scene(ci, method)
    n_exc = _compare_scene(what, got, ref, method, _plane_fit_detail(ci) if method == 1 else None)
    assert n_exc <= _excusal_bound(len(ref[0])), "%s: %d excusals" % (what, n_exc)
    assert (got[2] >= np.float32(thr)).all(), what
    if c.get("crop", (0, 0, 0, 0))[2:] == (11, 13) and method == 0:
        assert len(got[0]) == 0, what      # no pixel of an 11 x 13 frame has a gradient normal
    if c.get("edit", ("",))[0] in ("zero", "one"):
        assert len(got[0]) == 0, what      # no leaf with 11 neighbours
    if c["frame"] in ("steps", "grazing") or c.get("edit", ("",))[0] == "far" or c.get("up") or c.get("K"):
        assert len(got[0]) > 100, what     # these cases must not be vacuous


def test_far_depths_leave_the_near_cloud_unchanged():
    """Far background and saturated depths (up to 65.5 m) are accepted.  They cannot change the near cloud: the frame with raw 65 535 in two
    corner patches gives exactly the points of the frame whose patches are 0, except those whose pixel normal sees the patch."""
    from model_matching_amd.estimator import ingest_scene
    r = _raw("linemod_obj_06")
    K = [float(x) for x in r["K"]]
    a = ingest_scene(_corner_patches(r["depth"], 65535), r["prob"], K, 0.001)
    b = ingest_scene(_corner_patches(r["depth"], 0), r["prob"], K, 0.001)
    assert len(a[0]) > 1000
    near = lambda px: (((px[:, 0] < 31) & (px[:, 1] < 31)) | ((px[:, 0] >= 480 - 31) & (px[:, 1] >= 640 - 31)))
    ka, kb = set(_keys(a[0][~near(a[3])], a[3][~near(a[3])])), set(_keys(b[0][~near(b[3])], b[3][~near(b[3])]))
    assert ka == kb


def test_absurd_intrinsics_are_refused():
    """The outlier-removal grid spans the part of the frame with z <= 2 m; a focal length of half a pixel makes that 2.5 km wide, over 2^28
    cells: STOCS_ERR_INVALID (include/stocs_hip.h)."""
    from model_matching_amd import capi
    from model_matching_amd.estimator import ingest_scene
    r = _raw("linemod_obj_06")
    with pytest.raises(capi.StocsError) as e:
        ingest_scene(r["depth"], r["prob"], [0.5, 325.0, 0.5, 242.0], 0.001)
    assert e.value.code == capi.ERR_INVALID and "outlier-removal grid" in str(e.value)


MULTI_CASES = [(1, 5), (3, 9), (3, 11), (64, 1)]   # (number of maps, scene case)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("n_maps,ci", MULTI_CASES)
def test_multi_object_ingest_edges(n_maps, ci, method):
    from model_matching_amd.estimator import ingest_scene, ingest_scene_multi
    from oracle.ingest_oracle import ingest_scene as ref
    c = SCENE_CASES[ci]
    depth, prob, K, scale, voxel, thr = _case_inputs(c)
    rng = np.random.default_rng(100 + n_maps)
    probs = [prob] + [np.roll(prob, int(rng.integers(-40, 40)), axis=int(rng.integers(0, 2))) for _ in range(n_maps - 1)]
    if n_maps > 2:
        probs[1] = np.full_like(prob, 1000)            # exactly at the default threshold
        probs[2] = rng.integers(0, 10001, prob.shape).astype(np.uint16)
    thrs = [thr] + [float(x) for x in rng.choice([0.0, 0.1, 0.35, 1.0], n_maps - 1)]
    outs = ingest_scene_multi(depth, np.stack(probs), K, scale, voxel, thrs, normal_method=method)
    assert len(outs) == n_maps
    detail = None
    if method == 1:
        detail = _plane_fit_detail(ci)
    for k in range(n_maps):
        what = "%s, object %d of %d (threshold %g)" % (_describe(c, method), k, n_maps, thrs[k])
        one = ingest_scene(depth, probs[k], K, scale, voxel, thrs[k], normal_method=method)
        assert all(np.array_equal(x, y) for x, y in zip(outs[k], one)), what
        if k < 4 or k % 16 == 0:
            r = _oracle_scene(ci, method) if k == 0 else ref(depth, probs[k], K, scale, voxel, thrs[k], normal_method=method)
            assert _compare_scene(what, outs[k], r, method, detail) <= _excusal_bound(len(r[0])), what


def test_rocprim_leaf_sort_equals_the_own_sort(monkeypatch):
    """STOCS_SORT=rocprim: the leaves of a >= 65 536-pixel frame sorted by rocPRIM instead of sort32.hip, bit for bit the same cloud."""
    from model_matching_amd.estimator import ingest_scene
    for ci in (4, 7):
        depth, prob, K, scale, voxel, thr = _case_inputs(SCENE_CASES[ci])
        assert depth.size >= OWN_SORT_MIN
        a = ingest_scene(depth, prob, K, scale, voxel, thr)
        monkeypatch.setenv("STOCS_SORT", "rocprim")
        b = ingest_scene(depth, prob, K, scale, voxel, thr)
        monkeypatch.delenv("STOCS_SORT")
        assert len(a[0]) > 1000 and all(np.array_equal(x, y) for x, y in zip(a, b)), _case_id(SCENE_CASES[ci])


# ---- models
def _sphere(n, radius, seed):
    """n points of a Fibonacci lattice on a sphere (spacing ~ radius * sqrt(4 pi / n)), jittered a little, off the origin."""
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n); th = np.pi * (1 + 5 ** 0.5) * i
    p = radius * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)
    p += np.random.default_rng(seed).normal(0, radius * 1e-3, p.shape)
    return (p + np.array([0.011, -0.007, 0.004])).astype(np.float32)


def _one_leaf_patch():
    """22 500 points of a gently curved 7.5 mm patch inside one 1 cm leaf: more than the 63 x 256 that centroid_long_kernel's workgroups
    but one take in their first stride, so every workgroup holds a share of the leaf."""
    g = np.arange(150) * 5e-5 + 0.0012
    x, y = np.meshgrid(g, g)
    z = 0.0051 + 20.0 * (x - 0.005) ** 2
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)


MODEL_CASES = [
    ("isolated points", lambda: np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float32), 0.01, 0.005, 1.0),
    ("sphere 65 535", lambda: _sphere(65535, 0.05, 1), 0.002, 0.005, 1.0),
    ("sphere 65 536", lambda: _sphere(65536, 0.05, 2), 0.002, 0.005, 1.0),
    ("sphere 65 537", lambda: _sphere(65537, 0.05, 3), 0.002, 0.005, 1.0),
    ("dense sphere 150 000", lambda: _sphere(150000, 0.03, 4), 0.001, 0.01, 1.0),
    ("one leaf of 22 500 points", _one_leaf_patch, 0.0002, 0.01, 1.0),
    ("linemod model (mm), leaf 0.05 mm", lambda: _raw("linemod_obj_06")["model_raw"], 10.0, 0.05, 0.001),
    ("ycb model, scale 0.001", lambda: _raw("ycb_024_bowl")["model_raw"], 0.01, 0.005, 0.001),
]


@functools.lru_cache(maxsize=None)
def _oracle_model(mi):
    from oracle.ingest_oracle import preprocess_model as ref
    name, make, rad, voxel, scale = MODEL_CASES[mi]
    return ref(make(), rad, voxel, scale)


@pytest.mark.parametrize("mi", range(len(MODEL_CASES)), ids=[m[0].replace(" ", "_") for m in MODEL_CASES])
def test_model_preprocess_edges_equal_the_restatement(mi):
    from model_matching_amd.estimator import preprocess_model
    name, make, rad, voxel, scale = MODEL_CASES[mi]
    what = "model case %s: normal radius %g, voxel %g, model_scale %g" % (name, rad, voxel, scale)
    pos, nrm = preprocess_model(make(), rad, voxel, scale)
    rpos, rnrm = _oracle_model(mi)
    assert len(pos) == len(rpos), what
    if mi == 0:
        assert len(pos) == 0, what
        return
    assert np.abs(pos - rpos).max() <= 1e-7 * max(1.0, np.abs(pos).max()) * 10, what
    ang = np.degrees(np.arccos(np.clip((nrm * rnrm).sum(1), -1, 1)))
    assert np.percentile(ang, 99) < 0.05 and (ang < 1.0).mean() > 0.995, what


# ---- coverage: computed on the host from the inputs
def _leaf_stats(points, leaf):
    """(cells of the leaf grid, points per leaf) as voxel_grid_device sees them."""
    ijk = np.floor(np.asarray(points, np.float32).astype(np.float64) * (1.0 / np.float64(np.float32(leaf)))).astype(np.int64)
    dims = ijk.max(0) - ijk.min(0) + 1
    _, cnt = np.unique(ijk, axis=0, return_counts=True)
    return float(np.prod(dims.astype(np.float64))), cnt


def _old_ror_cells(points, leaf):
    """Cells of the outlier-removal grid as it was built before far depths were accepted: over the box of every leaf."""
    ijk = np.floor(np.asarray(points, np.float32).astype(np.float64) * (1.0 / np.float64(np.float32(leaf)))).astype(np.int64)
    lo, hi = (ijk.min(0) - 1.0) * float(np.float32(leaf)), (ijk.max(0) + 2.0) * float(np.float32(leaf))
    r = 2.0 * float(np.float32(leaf)) + 0.005
    return float(np.prod(np.floor((hi - lo) / r) + 1))


def _model_with_normals(mi):
    """The raw points that get a normal (at least 3 neighbours within the radius): what the model's voxel grid sorts."""
    from scipy.spatial import cKDTree
    name, make, rad, voxel, scale = MODEL_CASES[mi]
    p = np.asarray(make(), np.float32).astype(np.float64)
    k = cKDTree(p).query_ball_point(p, float(np.float32(rad)), return_length=True)
    return p[k >= 3].astype(np.float32)


def test_the_cases_reach_every_branch():
    frames = []
    for c in SCENE_CASES:
        depth, prob, K, scale, voxel, thr = _case_inputs(c)
        P = _backproject(depth, K, scale).reshape(-1, 3)
        cells, cnt = _leaf_stats(P, voxel)
        frames.append((len(P), cells, int((cnt > LONG_LEAF).sum()), _old_ror_cells(P, voxel)))
    npx = [f[0] for f in frames]
    assert min(npx) < OWN_SORT_MIN and any(n == OWN_SORT_MIN for n in npx) and any(n == OWN_SORT_MIN - 1 for n in npx)   # rocPRIM / own sort
    assert any(f[1] > 2.0 ** 32 for f in frames)                       # 64-bit leaf keys in a frame
    assert any(f[2] >= 2 for f in frames)                              # several queued leaves in centroid_long_kernel
    assert any(f[3] > 2.0 ** 28 for f in frames)                       # refused before far depths were accepted
    assert sum(f[3] > 2.0 ** 28 for f in frames) >= 3
    models = []
    for mi in range(1, len(MODEL_CASES)):
        q = _model_with_normals(mi)
        cells, cnt = _leaf_stats(q, MODEL_CASES[mi][3])
        models.append((len(q), cells, int((cnt > LONG_LEAF).sum()), int(cnt.max())))
    nk = [m[0] for m in models]
    assert any(n < OWN_SORT_MIN for n in nk) and any(n >= OWN_SORT_MIN for n in nk)   # rocPRIM / own sort with the normals as extra
    assert any(n == OWN_SORT_MIN - 1 for n in nk) and any(n == OWN_SORT_MIN for n in nk)
    assert any(m[2] >= 1 for m in models)                              # long leaves with normals
    assert any(m[3] > 63 * 256 for m in models)                        # a leaf shared by all 64 workgroups of centroid_long_kernel
    assert any(m[1] > 2.0 ** 32 for m in models)                       # 64-bit leaf keys in a model
