"""The reference's own kd-tree and normal-set headers (compiled unchanged into oracle/_ref/libref_accel.so, oracle/ref_accel.cpp) against
the oracle's restatement of them, and for the kd-tree also against the product's host tree (csrc/kdtree.h, stocs_kdtree_nn_host).  This
is what pins oracle/stocs_oracle.cpp, the file every GPU parity test compares with, to something the reference holds.

kd-tree: reference header, orc_nn and kdtree_nn_host answer every (query, sqdist) over identical floats (Oracle.scene_centred()) with
the same index -- no allowance, ties and the exact radius included.  Normal set: position cell, normal cell, _nepsilon, the power-of-two
correction of epsilon and the order inside a cell, reference against oracle.

No device is needed.  Without the library the tests FAIL where the reference tree is present (oracle/Makefile should have built it) and
skip only where neither exists."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grid_ref  # noqa: E402

F = np.float32
H = 2.0 ** -9
EPS_LIST = [0.03, 0.0625, 0.01, 0.1, 0.5]


@pytest.fixture(scope="module")
def ref(oracle_lib):
    from oracle import pyref
    if not pyref.available():
        if pyref.reference_present():
            pytest.fail("the reference tree is at %s but %s is missing: `make -C oracle` builds it" % (pyref.reference_dir(), pyref.SO))
        pytest.skip("neither the reference tree (%s) nor %s exists" % (pyref.reference_dir(), pyref.SO))
    return pyref.RefAccel()


# ------------------------------------------------------------------------------------------------------------------------------------
# kd-tree
# ------------------------------------------------------------------------------------------------------------------------------------
def _oracle(pos):
    from oracle import pyoracle
    pos = np.asarray(pos, F)
    n = len(pos)
    nrm = np.tile(np.array([0, 0, 1], F), (n, 1))
    mp = np.array([[0, 0, 0], [H, 0, 0], [0, H, 0], [0, 0, H]], F)
    return pyoracle.Oracle(pos, nrm, np.full(n, 0.5, F), None, mp, nrm[:4].copy(), build_index=False)


class Three:
    """the three trees over the same floats"""

    def __init__(self, ref, orc):
        self.orc = orc
        self.sc = orc.scene_centred()
        self.tree = ref.kdtree(self.sc)

    def check(self, queries, sqdist, what=""):
        """reference == oracle == product on every query; returns the reference's answers"""
        from model_matching_amd.estimator import kdtree_nn_host
        q = np.ascontiguousarray(np.asarray(queries, F).reshape(-1, 3))
        sq = F(sqdist)
        r = self.tree.nn(q, sq)
        o = np.array([self.orc.nn(row, sq) for row in q], np.int32)
        p = kdtree_nn_host(self.sc, q, sq)
        assert r.min() >= -1 and r.max() < len(self.sc)
        bad = np.nonzero(r != o)[0]
        assert len(bad) == 0, "%s sqdist %r: oracle differs from the reference header at %d of %d queries, first %s: ref %d oracle %d" % (
            what, float(sq), len(bad), len(q), q[bad[0]].tolist(), r[bad[0]], o[bad[0]])
        bad = np.nonzero(r != p)[0]
        assert len(bad) == 0, "%s sqdist %r: product tree differs from the reference header at %d of %d queries, first %s: ref %d product %d" % (
            what, float(sq), len(bad), len(q), q[bad[0]].tolist(), r[bad[0]], p[bad[0]])
        return r

    def n_tied(self, queries, sqdist):
        return sum(self.orc.nn_brute(row, F(sqdist))[1] > 0 for row in np.asarray(queries, F).reshape(-1, 3))


def _lattice(k, rng, dup):
    r = np.arange(-k, k + 1, dtype=F) * F(H)
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    g = np.repeat(g, dup, axis=0)
    return g[rng.permutation(len(g))]


def _tie_queries(k, rng, m):
    """m each of: edge (2-way), face (4-way) and body (8-way) midpoints of lattice cells, and lattice points"""
    c = rng.integers(-k, k, size=(m, 3)).astype(F) * F(H)
    half = F(H / 2)
    e = c.copy(); e[:, 0] += half
    f = c.copy(); f[:, 0] += half; f[:, 1] += half
    b = c + half
    return np.concatenate([e, f, b, c]).astype(F)


@pytest.mark.parametrize("k,dup", [(7, 1), (4, 3), (2, 70)], ids=["hw7x1", "hw4x3", "hw2x70"])
def test_tie_lattices(ref, k, dup):
    """Lattices symmetric about the origin (spacing 2^-9: the float centroid is exactly zero, so centring keeps every tie exact), in a
    shuffled index order.  70 copies per site are more than the 64 points of a leaf: no split separates them, the depth limit ends the
    recursion.  600 queries x 4 radii = 2 400; at least 1 000 of them are exact ties by the brute force (every midpoint query at the
    three positive radii is one: 1 350, and with copies every lattice-point query too: 1 950)."""
    rng = np.random.default_rng(1000 + 10 * k + dup)
    pos = _lattice(k, rng, dup)
    assert len(pos) == (2 * k + 1) ** 3 * dup
    t = Three(ref, _oracle(pos))
    assert np.array_equal(t.sc, pos)
    q = _tie_queries(k, rng, 150)
    n_q = n_tied = 0
    for sq in (F(H * H), F(0.75 * H * H), F(4 * H * H), F(0.0)):
        r = t.check(q, sq, "lattice %d x %d" % (k, dup))
        n_q += len(q)
        n_tied += t.n_tied(q, sq)
        if sq == 0:
            # the walk tests the root with a strict `<` (kdtree.h:416: 0 < 0 fails), so radius 0 finds nothing -- not even the
            # lattice-point queries that coincide with scene points, which the brute force's `<=` does find
            assert np.all(r == -1)
            assert all(t.orc.nn_brute(row, sq)[0] >= 0 for row in q[450:])
        else:
            assert np.all(r >= 0)
    assert n_q == 2400
    assert n_tied >= 1000, n_tied


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 129, 5000])
def test_leaf_capacity_edges(ref, n):
    """random clouds around the 64 points of a leaf; the root is split even when it holds one point"""
    rng = np.random.default_rng(2000 + n)
    pos = (rng.standard_normal((n, 3)) * 0.05).astype(F)
    t = Three(ref, _oracle(pos))
    q = np.concatenate([t.sc[rng.integers(0, n, 60)] + (rng.standard_normal((60, 3)) * 0.004).astype(F),
                        t.sc[:min(n, 40)], (rng.standard_normal((40, 3)) * 0.08).astype(F)]).astype(F)
    found = 0
    for sq in (F(1e-4), F(2.5e-5), F(0.04), F(0.0)):
        found += int((t.check(q, sq, "n = %d" % n) >= 0).sum())
    assert found > 0


def _degenerate(shape, rng):
    if shape == "collinear":
        x = np.arange(-40, 41, dtype=F) * F(H)
        pos = np.zeros((len(x) * 5, 3), F)
        pos[:, 0] = np.repeat(x, 5)                                       # five copies per site on the x axis
        q = np.zeros((160, 3), F)
        q[:, 0] = rng.integers(-82, 83, 160).astype(F) * F(H / 2)         # sites and midpoints
        q[80:, 1:] = rng.integers(-1, 2, (80, 2)).astype(F) * F(H / 2)
    elif shape == "planar":
        r = np.arange(-9, 10, dtype=F) * F(H)
        pos = np.stack(np.meshgrid(r, r, [F(0)], indexing="ij"), -1).reshape(-1, 3).astype(F)   # zero extent in z
        q = np.zeros((200, 3), F)
        q[:, :2] = rng.integers(-19, 20, (200, 2)).astype(F) * F(H / 2)
        q[100:, 2] = rng.integers(-1, 2, 100).astype(F) * F(H / 2)
    elif shape == "coincident":
        pos = np.zeros((200, 3), F)                                       # every split degenerate: the tree runs to depth 32
        q = np.array([[0, 0, 0], [H, 0, 0], [0, 0, -H], [0, H / 2, 0], [1, 1, 1]], F)
    else:                                                                 # two clusters, 10^3 cells of size sqrt(sqdist) = H apart
        a = (rng.integers(-6, 7, (600, 3)).astype(F) * F(H))
        a = np.concatenate([a, -a])                                       # symmetric, so both clusters keep lattice coordinates
        off = np.array([1000 * H, 0, 0], F)
        pos = np.concatenate([a - off / 2, a + off / 2]).astype(F)
        q = np.concatenate([pos[rng.integers(0, len(pos), 100)] + F(H / 2), np.zeros((4, 3), F), pos[:40]]).astype(F)
    return pos[rng.permutation(len(pos))], q


@pytest.mark.parametrize("shape", ["collinear", "planar", "coincident", "far_clusters"])
def test_degenerate_clouds(ref, shape):
    rng = np.random.default_rng(31)
    pos, q = _degenerate(shape, rng)
    t = Three(ref, _oracle(pos))
    assert np.array_equal(t.sc, pos)          # symmetric about the origin: centring changes nothing, ties stay exact
    found = 0
    for sq in (F(H * H), F(0.25 * H * H), F(4 * H * H)):
        found += int((t.check(q, sq, shape) >= 0).sum())
    assert found > 0
    assert t.n_tied(q, F(H * H)) > 0


def test_radius_exactly_met(ref):
    """sqdist equal to the nearest point's own d2 (in the float order of the trees, grid_ref.d2_f32), one float below and one above.  The
    leaf test is `<=`, the node test `<`: a point exactly at the radius is found unless a split plane on the way to its leaf lies at
    that same distance.  The reference decides; below the radius nothing is in range, above it the nearest point must be found."""
    rng = np.random.default_rng(15)
    pos = (rng.standard_normal((3000, 3)) * 0.05).astype(F)
    t = Three(ref, _oracle(pos))
    q = (t.sc[rng.integers(0, len(t.sc), 200)] + (rng.standard_normal((200, 3)) * 0.004).astype(F)).astype(F)
    d2 = grid_ref.d2_f32(q, t.sc)
    near = d2.min(1)
    n_on = 0
    for i in range(len(q)):
        s = F(near[i])
        below, above = np.nextafter(s, F(0)), np.nextafter(s, F(np.inf))
        assert t.check(q[i], below, "below")[0] == -1
        n_on += t.check(q[i], s, "on")[0] >= 0
        hit = t.check(q[i], above, "above")[0]
        assert hit >= 0 and d2[i, hit] == s
    print("found exactly at the radius: %d of %d" % (n_on, len(q)))


def test_radius_met_on_a_split_plane(ref):
    """The other side of the same rule, which random clouds do not reach.  Three slabs of lattice points at x = -4H, 0, 4H (y, z over
    -7H..7H).  Once y and z are halved, x is the widest axis and the split plane lies at x = 0, ON the middle slab, whose points go
    to the right child (`>=`).  A query at (-H, y, z) has exactly one point within sqdist = H^2, (0, y, z), exactly at the radius and
    behind that plane; the plane's own H^2 is not < the radius, so the subtree is never opened and the answer is "none".  The mirrored
    query (+H, y, z) starts on the slab's side and finds it.  One float above the radius both do, one float below neither."""
    rng = np.random.default_rng(17)
    r = np.arange(-7, 8, dtype=F) * F(H)
    g = np.stack(np.meshgrid(np.array([-4, 0, 4], F) * F(H), r, r, indexing="ij"), -1).reshape(-1, 3).astype(F)
    pos = g[rng.permutation(len(g))]
    t = Three(ref, _oracle(pos))
    assert np.array_equal(t.sc, pos)
    yz = np.stack(np.meshgrid(r, r, indexing="ij"), -1).reshape(-1, 2)
    left = np.concatenate([np.full((len(yz), 1), -H, F), yz], 1).astype(F)
    right = left * np.array([-1, 1, 1], F)
    sq = F(H * H)
    for q in (left, right):
        assert all(t.orc.nn_brute(row, sq) == (t.orc.nn_brute(row, sq)[0], 0) and t.orc.nn_brute(row, sq)[0] >= 0 for row in q)   # one point, no tie
        assert np.all(t.check(q, np.nextafter(sq, F(0)), "below") == -1)
        assert np.all(t.check(q, np.nextafter(sq, F(1)), "above") >= 0)
    on_left, on_right = t.check(left, sq, "left of the plane"), t.check(right, sq, "right of the plane")
    assert np.all(on_left == -1), int((on_left >= 0).sum())
    assert np.all(on_right >= 0), int((on_right < 0).sum())


@pytest.mark.parametrize("name", ["tiny", "small", "dense"])
def test_synth_workloads(ref, oracle_lib, name):
    """the queries LCP verification asks: every model point under 12 candidate transforms, at the workload's squared epsilon"""
    from model_matching_amd import synth
    m, s, k = synth.workload(name)
    orc = oracle_lib.Oracle(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    cs, cm = orc.centroids()
    T = synth.make_candidates(synth.centred_gt(s.T_gt, cs.astype(np.float64), cm.astype(np.float64)), k)[:12]
    t = Three(ref, orc)
    mc = orc.model_centred()
    q = np.concatenate([grid_ref.transform(T[c], mc) for c in range(len(T))])
    r = t.check(q, grid_ref.sq_eps(orc.prm.distance_threshold), name)
    assert (r >= 0).sum() > 0


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_host_trees_stand_alone(tmp_path, flags):
    """tests/cpp/kdtree_ref_check.cpp: the product's host tree (csrc/kdtree.h, kdtree.hip's construction) and the reference's header in
    one stand-alone program over the coincident and the collinear cloud, built with g++ against the HIP headers (no HIP library, no
    device), once plainly and once under the address and undefined-behaviour sanitizers.  Nothing is preloaded.  The program is
    compiled against the reference tree itself, so it runs only where that tree is."""
    import subprocess
    from oracle import pyref
    if not pyref.reference_present():
        pytest.skip("the reference tree (%s) is not here: kdtree_ref_check.cpp compiles against its headers" % pyref.reference_dir())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "kdtree_ref_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-deprecated-declarations", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(root, "oracle", "eigen_standin"),
                           "-I" + os.path.join(pyref.reference_dir(), "include"), "-I" + os.path.join(root, "model_matching_amd", "csrc"),
                           *flags, "-o", exe, os.path.join(root, "tests", "cpp", "kdtree_ref_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "kdtree_ref_check: ok" in r.stdout and " 0 differ" in r.stdout


# ------------------------------------------------------------------------------------------------------------------------------------
# normal set
# ------------------------------------------------------------------------------------------------------------------------------------
def _key(v):
    """floats as ordered integers, so that a bisection crosses zero too"""
    i = np.asarray(v, F).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7FFFFFFF))


def _val(j):
    j = np.asarray(j, np.int64)
    return np.where(j >= 0, j, ((-j) | 0x80000000) - (1 << 32)).astype(np.int32).view(F)


def _faces(coord, ks, lo, hi):
    """per k of ks, the smallest float x in (lo, hi] with coord(x) >= k (coord monotone, vectorised over rows), by bisection over floats,
    as grid_ref.face_float finds the grid's faces"""
    ks = np.asarray(ks, np.int64)
    a = np.full(len(ks), int(_key(F(lo))), np.int64); b = np.full(len(ks), int(_key(F(hi))), np.int64)
    assert np.all(coord(_val(a)) < ks) and np.all(coord(_val(b)) >= ks)
    while np.any(b - a > 1):
        mid = (a + b) // 2
        up = coord(_val(mid)) >= ks
        b = np.where(up, mid, b); a = np.where(up, a, mid)
    return _val(b)


def _around(x):
    """the floats below, on and above each x"""
    k = _key(x)
    return np.concatenate([_val(k - 1), _val(k), _val(k + 1)]).astype(F)


def _compare_normals(ref, oracle_lib, n):
    n = np.ascontiguousarray(n, F)
    r = ref.index_normal_rows(n)
    o = np.array([oracle_lib.index_normal(row) for row in n], np.int32)
    bad = np.nonzero(r != o)[0]
    assert len(bad) == 0, (len(bad), n[bad[0]].tolist(), int(r[bad[0]]), int(o[bad[0]]))
    return r


def test_normal_cells(ref, oracle_lib):
    rng = np.random.default_rng(41)
    unit = oracle_lib.normalize_rows(rng.standard_normal((20000, 3)).astype(F))
    r = _compare_normals(ref, oracle_lib, unit)
    assert r.min() >= 0 and r.max() < 343 and len(np.unique(r)) > 150
    axes = np.concatenate([np.eye(3, dtype=F), -np.eye(3, dtype=F)])      # -1 and +1 exactly: cells 0 and 6 of the axis
    r = _compare_normals(ref, oracle_lib, axes)
    assert sorted(r.tolist()) == sorted([6 + 3 * 7 + 3 * 49, 3 + 6 * 7 + 3 * 49, 3 + 3 * 7 + 6 * 49, 0 + 3 * 7 + 3 * 49, 3 + 0 * 7 + 3 * 49, 3 + 3 * 7 + 0 * 49])
    # zero and non-unit vectors: the index is plain integer arithmetic on truncated coordinates, outside 0..342 too
    odd = np.concatenate([np.zeros((1, 3), F), unit[:200] * F(0.5), unit[:200] * F(1.5), unit[:200] * F(3.0),
                          np.array([[2, -2, 0.3], [1, 1, 1], [-1, -1, -1], [1e-30, -1e-30, 0], [-0.0, 0.0, -0.0]], F)])
    _compare_normals(ref, oracle_lib, odd)


def test_nepsilon_is_double_arithmetic_cast_to_float(ref):
    """normalset.h:86: Scalar(1.)/Scalar(_ngSize) + 0.00001 -- a float quotient, a double sum, stored as a float"""
    want = F(np.float64(F(1.0) / F(7.0)) + 0.00001)
    assert F(ref.nepsilon()) == want


def test_normal_cell_faces(ref, oracle_lib):
    """For each of the 7 faces per axis (the lower faces of cells 1..6 and the upper face of cell 6, just above +1): the floats below, on
    and above it, on that axis with every other pair of fixed coordinates below.  This is where a restated _nepsilon would show."""
    n_checked = 0
    for axis in range(3):
        for other in (F(0.0), F(-0.93), F(0.37)):
            base = np.full(3, other, F)

            def rows(x):
                v = np.tile(base, (len(x), 1)); v[:, axis] = x
                return v

            def coord(x):
                idx = ref.index_normal_rows(rows(x)).astype(np.int64)
                v = np.zeros(3, F); v[:] = other; v[axis] = F(-1.0)     # coordinate 0 on `axis`: what the other two contribute
                return (idx - ref.index_normal(v)) // 7 ** axis
            faces = _faces(coord, np.arange(1, 8), -1.0, 1.5)
            assert np.all(np.diff(faces) > 0) and faces[-1] > 1.0 and faces[-2] < 1.0
            x = _around(faces)
            got = _compare_normals(ref, oracle_lib, rows(x))
            c = coord(x)
            assert np.array_equal(c[:7] + 1, c[7:14]) and np.array_equal(c[7:14], c[14:]) and np.array_equal(c[7:14], np.arange(1, 8))
            n_checked += len(got)
    assert n_checked == 3 * 3 * 21


@pytest.mark.parametrize("eps", EPS_LIST)
def test_position_cells_and_epsilon_correction(ref, oracle_lib, eps):
    eg, cell = ref.nset_params(eps)
    depth_o, eg_o, cell_o = oracle_lib.normalset_params(eps)
    assert (eg, F(cell)) == (eg_o, F(cell_o)) and eg == 2 ** depth_o
    # the corrected epsilon is the power of two at or above eps (normalset.h:117-119: the depth is truncated)
    assert F(cell) == F(1.0) / F(eg) and cell >= F(eps) > cell / 2
    rng = np.random.default_rng(43)
    p = rng.random((4000, 3)).astype(F)
    r = ref.index_pos_rows(eps, p)
    o = np.array([oracle_lib.index_pos(eps, row) for row in p], np.int32)
    assert np.array_equal(r, o)
    assert r.min() >= 0 and r.max() < eg ** 3
    # every inner face per axis, and the outer ones (0 and 1): the floats below, on and above
    for axis in range(3):
        base = np.array([0.31, 0.62, 0.93], F)

        def rows(x):
            v = np.tile(base, (len(x), 1)); v[:, axis] = x
            return v

        def coord(x):
            v = base.copy(); v[axis] = 0.0
            return (ref.index_pos_rows(eps, rows(x)).astype(np.int64) - ref.index_pos(eps, v)) // eg ** axis
        faces = _faces(coord, np.arange(1, eg + 1), 0.0, 1.25)
        assert np.array_equal(faces, (np.arange(1, eg + 1) / eg).astype(F))       # a power-of-two cell: the faces are exact
        x = np.concatenate([_around(faces), _around(np.zeros(1, F))])
        r = ref.index_pos_rows(eps, rows(x))
        o = np.array([oracle_lib.index_pos(eps, row) for row in rows(x)], np.int32)
        assert np.array_equal(r, o), (axis, np.nonzero(r != o)[0][:4])


def test_order_inside_a_cell(ref, oracle_lib):
    """300 elements into three cells, in a shuffled assignment: getNeighbors(p, n) returns a cell's ids in insertion order, and
    getNeighbors(p) the normal cells of a position cell in index order.  This is the property the stable sort of the congruent phase
    (csrc/sort32.hip, tests/test_sort_gpu.py) stands in for; the oracle's lists are held to the same order."""
    eps = 0.0625
    rng = np.random.default_rng(47)
    pc = np.array([[0.40, 0.40, 0.40], [0.40, 0.40, 0.40], [0.80, 0.15, 0.55]], F)     # two cells share a position cell
    # (unit normals whose components sit near the middle of their normal cells: 0.30 -> coordinate 4.6, 0.90 -> 6.7, -0.90 -> 0.3)
    nc = oracle_lib.normalize_rows(np.array([[0.857, 0.286, 0.286], [-0.286, 0.286, -0.857], [0.286, -0.857, 0.286]], F))
    which = rng.integers(0, 3, 300)
    pos = (pc[which] + (rng.random((300, 3)) * 0.01).astype(F)).astype(F)
    nrm = oracle_lib.normalize_rows((nc[which] + (rng.standard_normal((300, 3)) * 0.01).astype(F)).astype(F))
    ns = ref.normalset(eps, pos, nrm)
    assert ns.n_added == 300
    # the jitter keeps every element in its cell
    for c in range(3):
        assert len(set(ref.index_pos_rows(eps, pos[which == c]).tolist())) == 1 and len(set(ref.index_normal_rows(nrm[which == c]).tolist())) == 1
    assert ref.index_normal(nc[0]) > ref.index_normal(nc[1])          # cell 0 has the larger normal index of the shared position cell
    for c in range(3):
        want = np.nonzero(which == c)[0].astype(np.uint32)            # increasing id = insertion order
        got = ns.cell(pc[c] + F(0.005), nc[c])
        assert np.array_equal(got, want), c
        assert np.array_equal(oracle_lib.nset_cell(eps, pos, nrm, pc[c] + F(0.005), nc[c]), want), c
    whole = np.concatenate([np.nonzero(which == 1)[0], np.nonzero(which == 0)[0]]).astype(np.uint32)   # normal cells in index order
    assert np.array_equal(ns.cell(pc[0] + F(0.005)), whole)
    assert np.array_equal(oracle_lib.nset_cell(eps, pos, nrm, pc[0] + F(0.005)), whole)
    assert len(ns.cell(np.array([0.1, 0.1, 0.1], F))) == 0 and len(oracle_lib.nset_cell(eps, pos, nrm, np.array([0.1, 0.1, 0.1], F))) == 0
    ns.close()
