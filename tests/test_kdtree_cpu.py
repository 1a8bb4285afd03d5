"""The reference-order kd-tree of the exact_ties option (csrc/kdtree.h, stocs_kdtree_nn_host) against the oracle's restatement of
the reference's KdTree (orc_nn): the same scene index for every query, exact distance ties included (divergence Q11).

Both trees see identical floats: the product's tree is built over Oracle.scene_centred(), the positions the oracle's own tree
holds.  Lattices with spacing 2^-9, symmetric about the origin, have an exactly zero sequential float centroid, so centring keeps
their ties exact.  No device is needed.  tests/test_ref_accel_cpu.py holds both trees to the reference's own kdtree.h."""
import numpy as np
import pytest

H = 2.0 ** -9


def _oracle(pos):
    from oracle import pyoracle
    pos = np.asarray(pos, np.float32)
    n = len(pos)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    mp = np.array([[0, 0, 0], [H, 0, 0], [0, H, 0], [0, 0, H]], np.float32)
    mn = np.tile(np.array([0, 0, 1], np.float32), (4, 1))
    return pyoracle.Oracle(pos, nrm, np.full(n, 0.5, np.float32), None, mp, mn, build_index=False)


def _check(pos, queries, sqdists, min_ties=0):
    """product tree == oracle tree on every (query, sqdist); returns the number of tied queries (orc_nn_brute)"""
    from model_matching_amd.estimator import kdtree_nn_host
    orc = _oracle(pos)
    sc = orc.scene_centred()
    queries = np.asarray(queries, np.float32).reshape(-1, 3)
    n_tied = 0
    for sq in sqdists:
        got = kdtree_nn_host(sc, queries, sq)
        for q, g in zip(queries, got):
            ref = orc.nn(q, sq)
            assert g == ref, (q.tolist(), float(sq), int(g), ref)
            _, t = orc.nn_brute(q, sq)
            n_tied += t > 0
    assert n_tied >= min_ties, n_tied
    return n_tied


def _lattice(k, rng, dup=1):
    r = np.arange(-k, k + 1, dtype=np.float32) * np.float32(H)
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    g = np.repeat(g, dup, axis=0)
    return g[rng.permutation(len(g))]


def _tie_queries(k, rng, m):
    """edge (2-way), face (4-way) and body (8-way) midpoints of the lattice cells, plus lattice points and a few outside the box"""
    c = rng.integers(-k, k, size=(m, 3)).astype(np.float32) * np.float32(H)
    half = np.float32(H / 2)
    e = c.copy(); e[:, 0] += half
    f = c.copy(); f[:, 0] += half; f[:, 1] += half
    b = c + half
    out = np.float32((k + 1) * H) * np.array([[1, 0, 0], [0, -1, 0], [1, 1, 1], [-1, -1, 0.5]], np.float32)
    return np.concatenate([e, f, b, c, out]).astype(np.float32)


def test_symmetric_lattice_ties():
    rng = np.random.default_rng(11)
    pos = _lattice(7, rng)                       # 15^3 = 3 375 points in a random index order
    orc = _oracle(pos)
    assert np.array_equal(orc.scene_centred(), pos)   # the centroid is exactly zero: ties survive centring
    q = _tie_queries(7, rng, 120)
    _check(pos, q, [np.float32(H * H), np.float32((1.5 * H) ** 2), np.float32(4 * H * H)], min_ties=300)


def test_duplicated_points():
    rng = np.random.default_rng(12)
    pos = _lattice(4, rng, dup=3)                # every point three times
    q = np.concatenate([_tie_queries(4, rng, 60), pos[:80]])
    _check(pos, q, [np.float32(H * H), np.float32(0.0), np.float32(9 * H * H)], min_ties=200)


def test_all_points_identical():
    pos = np.zeros((300, 3), np.float32)        # every split degenerate: the tree runs to depth 32
    q = np.array([[0, 0, 0], [H, 0, 0], [0, 0, -H], [1, 1, 1]], np.float32)
    _check(pos, q, [np.float32(0.0), np.float32(H * H), np.float32(4 * H * H)], min_ties=3)


@pytest.mark.parametrize("shape", ["planar", "collinear"])
def test_degenerate_axes(shape):
    rng = np.random.default_rng(13)
    pos = _lattice(7, rng)
    if shape == "planar":
        pos = pos[pos[:, 2] == 0]
    else:
        pos = pos[(pos[:, 1] == 0) & (pos[:, 2] == 0)]
        pos = np.repeat(pos, 7, axis=0)[rng.permutation(7 * len(pos))]
    q = _tie_queries(7, rng, 80)
    if shape == "planar":
        q[:, 2] = np.where(rng.random(len(q)) < 0.5, 0.0, q[:, 2])
    else:
        q[:, 1:] = np.where(rng.random((len(q), 1)) < 0.5, 0.0, q[:, 1:])
    _check(pos, q, [np.float32(H * H), np.float32(4 * H * H)], min_ties=20)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 20000])
def test_sizes(n):
    rng = np.random.default_rng(100 + n)
    k = 3 if n < 1000 else 14
    pts = rng.integers(-k, k + 1, size=(n, 3)).astype(np.float32) * np.float32(H)
    pts = np.concatenate([pts, -pts])[:n] if n > 1 else np.zeros((1, 3), np.float32)   # (a symmetric set: zero centroid)
    if n % 2 == 1 and n > 1:
        pts[-1] = 0.0
    q = _tie_queries(k, rng, 40 if n < 1000 else 300)
    _check(pts, q, [np.float32(H * H), np.float32(4 * H * H)], min_ties=0 if n < 64 else (5 if n < 1000 else 100))


def test_split_planes_and_outside():
    """queries exactly on the split planes of the tree (the box midpoints of the nodes) and far outside the box"""
    rng = np.random.default_rng(14)
    pos = rng.standard_normal((5000, 3)).astype(np.float32) * np.float32(0.05)
    orc = _oracle(pos)
    sc = orc.scene_centred()
    mn, mx = sc.min(0), sc.max(0)
    ctr = mn + (mx - mn) / np.float32(2)
    q = rng.standard_normal((200, 3)).astype(np.float32) * np.float32(0.05)
    for a in range(3):
        q[a * 40:(a + 1) * 40, a] = ctr[a]              # on the root's candidate split planes
    q[150:160] = sc[rng.integers(0, len(sc), 10)]       # on scene points (splits of deeper nodes pass close to them)
    q[160:170] = mx + np.float32(0.01)
    q[170:180] = mn - np.float32(1.0)
    _check(pos, q, [np.float32(1e-4), np.float32(0.0), np.float32(0.04)])


def test_inclusive_bound():
    """sqdist equal to a point's squared distance, evaluated as both trees evaluate it: that point is within the radius"""
    rng = np.random.default_rng(15)
    pos = rng.standard_normal((3000, 3)).astype(np.float32) * np.float32(0.05)
    orc = _oracle(pos)
    sc = orc.scene_centred()
    from model_matching_amd.estimator import kdtree_nn_host
    n_found = 0
    for _ in range(150):
        q = sc[rng.integers(0, len(sc))] + rng.standard_normal(3).astype(np.float32) * np.float32(0.004)
        j = int(rng.integers(0, len(sc)))
        d = q - sc[j]
        sq = np.float32(d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]))
        # the nearest point's own squared distance: the bound is then met exactly by the answer
        dd = sc - q
        all_d = dd[:, 0] * dd[:, 0] + (dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2])
        sq_near = np.float32(all_d.min())
        for s in (sq, sq_near):
            g = kdtree_nn_host(sc, q[None], s)[0]
            assert g == orc.nn(q, s), (q.tolist(), float(s))
        n_found += kdtree_nn_host(sc, q[None], sq_near)[0] >= 0
    assert n_found == 150
