"""The cases of tests/ppf_index_cases.py checked with the CPU oracle alone: every condition the GPU tests of
tests/test_ppf_index_edges_gpu.py rely on, so that a family cannot stop holding what it is named for unnoticed.  These are conditions
on the inputs and on the oracle's two index forms, not on the code under test.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import ppf_index_cases as pc

_REF = {}


def _ref(oracle_lib, fam, tr, rot):
    k = (fam, tr, rot)
    if k not in _REF:
        pos, nrm = pc.FAMILIES[fam]()
        _REF[k] = (pos, nrm) + pc.reference_keys(pos, nrm, tr, rot, oracle_lib)
    return _REF[k]


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    _REF.clear()


def test_the_table_holds_what_the_issue_lists():
    want = {(f, d) for f in ("lattice", "collinear", "sphere") for d in [(5, 5), (4, 6), (10, 10), (20, 30), (7, 45), (5, 180), (1, 1)]}
    want |= {("bin_edges", d) for d in [(3, 2), (4, 6), (5, 5), (10, 10)]} | {("far_corners", d) for d in [(5, 5), (10, 10), (20, 30)]}
    assert set(pc.TABLE) == want and len(pc.TABLE) == len(want)
    assert pc.LOOKUP_CAP == 1500
    for fam, make in pc.FAMILIES.items():
        pos, nrm = make()
        pos2, nrm2 = make()
        assert pos.dtype == nrm.dtype == np.float32 and pos.shape == nrm.shape and len(pos) <= 64, fam
        assert pos.tobytes() == pos2.tobytes() and nrm.tobytes() == nrm2.tobytes(), fam          # deterministic
    assert len(pc.lattice()[0]) == 50 and len(pc.collinear()[0]) == 40 and len(pc.sphere()[0]) == 64 and len(pc.far_corners()[0]) == 24
    assert [len(pc.tiny_M(m)[0]) for m in range(4)] == [0, 1, 2, 3]
    pos, nrm = pc.nan_normal()
    assert np.isnan(nrm[pc.NAN_ID]).all() and np.isfinite(np.delete(nrm, pc.NAN_ID, 0)).all() and np.isfinite(pos).all()
    pos, nrm = pc.stride()
    assert len(pos) == 2049 and len(pos) ** 2 > 16384 * 256 >= 2048 ** 2


def _calls(oracle_lib):
    """the oracle's index calls with plain addresses as arguments: a loop over 10^5 keys costs no array conversion per key"""
    oracle_lib.lib()
    L = C.CDLL(oracle_lib.lib()._name)
    for name in ("orc_index_lit_lookup", "orc_index_lookup"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        getattr(L, name).restype = C.c_int64
    L.orc_index_exists.argtypes = [C.c_void_p, C.c_void_p]
    L.orc_index_exists.restype = C.c_int
    return L


@pytest.mark.parametrize("fam,disc", pc.TABLE, ids=["%s-%d-%d" % (f, d[0], d[1]) for f, d in pc.TABLE])
def test_reference_keys_are_the_literal_map_and_both_oracle_forms_agree(oracle_lib, fam, disc):
    tr, rot = disc
    pos, nrm, keys, F, pairs = _ref(oracle_lib, fam, tr, rot)
    nn = oracle_lib.normalize_rows(nrm)
    lit = oracle_lib.Index(pos, nn, tr, rot, literal=True)
    qry = oracle_lib.Index(pos, nn, tr, rot)
    M = len(pos)
    assert len(keys) == lit.num_keys() > 0
    assert sum(len(v) for v in pairs.values()) == M * (M - 1) == qry.num_pairs()
    L = _calls(oracle_lib)
    sh = pc.shell(keys, tr, rot)
    assert len(sh) > len(keys)
    inside = set(pc.pack_keys(keys).tolist())
    # on every key and on the whole shell: the literal map and the query form hold the same number of pairs, and a key is there
    # exactly when reference_keys has it
    allk = np.ascontiguousarray(pc.unique_keys(np.concatenate([keys, sh])))
    packed = pc.pack_keys(allk).tolist()
    base = allk.ctypes.data
    for i in range(len(allk)):
        a = L.orc_index_lit_lookup(lit.h, base + 16 * i, None, 0)
        b = L.orc_index_lookup(qry.h, base + 16 * i, None, 0)
        assert a == b and (a > 0) == bool(L.orc_index_exists(qry.h, base + 16 * i)) == (packed[i] in inside), allk[i]
    # content and order of the lookups: on every reference key of the coarse cases, else on an evenly strided 3000 of them
    some = keys[::max(1, -(-len(keys) // 3000))]
    for k in some:
        a, b = lit.lookup(k), qry.lookup(k)
        assert len(a) > 0 and a.shape == b.shape and (a == b).all(), k
        f = tuple(int(v) for v in k)
        if f in pairs:                                              # a key that is itself a feature holds that feature's pairs
            assert set(pairs[f]) <= set(map(tuple, a.tolist())), k
    # the border keys really are there, and every one of them is looked up
    b = pc.border(allk, tr, rot)
    lk = pc.lookup_keys(keys, allk, tr, rot)
    assert len(b) > 0 and len(lk) >= min(len(allk), pc.LOOKUP_CAP) and set(pc.pack_keys(b).tolist()) <= set(pc.pack_keys(lk).tolist())


def test_host_feature_equals_oracle_on_every_pair(oracle_lib):
    """csrc/stocs_math.h's ppf_compute (its own double atan2, plain IEEE operations, so host == device) against the oracle's glibc
    form on every ordered pair of every family, at the raw (1,1) discretisation and at (5,5)"""
    from model_matching_amd import capi
    L = capi.load()
    out = np.zeros(4, np.int32)
    for fam, make in pc.FAMILIES.items():
        pos, nrm = make()
        nn = oracle_lib.normalize_rows(nrm)
        for tr, rot in ((1, 1), (5, 5)):
            F = _ref(oracle_lib, fam, tr, rot)[3]
            for i in range(len(pos)):
                for j in range(len(pos)):
                    if i == j:
                        continue
                    a, pa = capi.f32(pos[i]); b, pb = capi.f32(nn[i]); c, pcc = capi.f32(pos[j]); d, pd = capi.f32(nn[j])
                    assert L.stocs_ppf_compute_host(pa, pb, pcc, pd, tr, rot, out.ctypes.data_as(capi._ip)) == 0
                    assert (out == F[i, j]).all(), (fam, tr, rot, i, j, out, F[i, j])


def test_lattice_holds_exact_angles_short_distances_and_coincident_points(oracle_lib):
    pos, nrm, keys, F, pairs = _ref(oracle_lib, "lattice", 5, 5)
    feats = list(pairs)
    n180 = sum(1 for f in feats if 180 in f[1:])
    n0 = sum(1 for f in feats if 0 in f[1:])
    short = sum(len(v) for f, v in pairs.items() if f[0] <= 5)
    coincident = [(i, j) for i in range(len(pos)) for j in range(len(pos)) if i != j and (pos[i] == pos[j]).all()]
    print("lattice (5,5): %d features with 180, %d with 0, %d pairs with F0 <= 5, %d coincident, %d keys" % (n180, n0, short, len(coincident), len(keys)))
    assert n180 >= 40 and n0 >= 100 and short >= 200 and len(coincident) == 6
    for i, j in coincident:
        assert F[i, j][0] == 0 and F[i, j][1] == 0 and F[i, j][2] == 0          # u = 0: atan2(0, 0) is taken as 0
    # every exact angle is there, and so is the zero normal (atan2(0,0) = 0 against everything)
    angles = {int(a) for f in feats for a in f[1:]}
    assert {0, 45, 90, 135, 180} <= angles
    zero = [i for i in range(len(pos)) if not nrm[i].any()]
    # the zero normal: norm(cross) = +0 and dot = +-0, so the angle is atan2(0, +0) = 0 or atan2(0, -0) = 180, by the signs of the other vector
    za = np.array([F[z, j][[1, 3]] for z in zero for j in range(len(pos)) if j != z]).ravel()
    assert len(zero) >= 3 and set(za.tolist()) == {0, 180}
    # equal distances: many pairs share one raw distance
    raw = _ref(oracle_lib, "lattice", 1, 1)[3]
    d = raw[..., 0][~np.eye(len(pos), dtype=bool)]
    assert np.bincount(d).max() >= 200


def test_collinear_normals_are_parallel_antiparallel_and_perpendicular(oracle_lib):
    pos, nrm, keys, F, pairs = _ref(oracle_lib, "collinear", 5, 5)
    a = F[..., 1][~np.eye(len(pos), dtype=bool)]
    assert set(np.unique(a).tolist()) <= {0, 90, 180} and {0, 90, 180} <= set(np.unique(a).tolist())
    t = np.linalg.norm(pos.astype(np.float64), axis=1)
    assert (np.diff(t) > 0).all() and len(np.unique(np.round(np.diff(t), 6))) >= 8            # uneven spacing


def _box_diag_mm(pos):
    """(int)(diag*1000) as build_ppf_index takes it: float min/max and squared norm, double square root"""
    d = (pos.max(0) - pos.min(0)).astype(np.float32)
    s = np.float32(d[0] * d[0]) + (np.float32(d[1] * d[1]) + np.float32(d[2] * d[2]))
    return int(math.sqrt(float(np.float32(s))) * 1000.0)


@pytest.mark.parametrize("disc", pc.DISCS_FAR)
def test_far_corners_reaches_the_top_distance_bin(oracle_lib, disc):
    tr, rot = disc
    pos, nrm, keys, F, pairs = _ref(oracle_lib, "far_corners", tr, rot)
    top = _box_diag_mm(pos) // tr + 1
    bins = F[..., 0][~np.eye(len(pos), dtype=bool)] // tr
    print("far_corners tr=%d: diag %d mm, top bin %d, pairs in it %d" % (tr, _box_diag_mm(pos), top, int((bins == top).sum())))
    assert bins.max() == top and (bins == top).sum() >= 2
    assert (pos[0] == pos.min(0)).all() and (pos[12] == pos.max(0)).all()          # the exact corners


def _edges_and_ties(values, d):
    """rounding edges v of closest_bin (v - 1 goes down, v goes up: v % d == ceil(d/2)) with both sides present, and exact half-bin
    ties present (2 (v % d) == d; an odd d has none: no integer lies on its half bin)"""
    have = set(int(v) for v in values)
    edges = [v for v in have if v % d == (d + 1) // 2 and v - 1 in have]
    ties = [v for v in have if 2 * (v % d) == d]
    return edges, ties


def test_bin_edges_hits_both_sides_of_the_rounding_edges_and_the_ties(oracle_lib):
    pos, nrm, keys, raw, pairs = _ref(oracle_lib, "bin_edges", 1, 1)          # at (1,1) the feature is the raw truncated value
    off = ~np.eye(len(pos), dtype=bool)
    dist = raw[..., 0][off]
    ang = raw[..., 1:][off].ravel()
    for tr in pc.BIN_EDGE_TR:
        e, t = _edges_and_ties(dist, tr)
        print("bin_edges tr=%d: %d edges with both sides, %d ties" % (tr, len(e), len(t)))
        assert len(e) >= 3 and (len(t) >= 2 if tr % 2 == 0 else len(t) == 0), tr
        for v in e:                                               # and the two sides really land in different bins
            assert oracle_lib.closest_bin(v - 1, tr) + tr == oracle_lib.closest_bin(v, tr)
    for rot in pc.BIN_EDGE_ROT:
        e, t = _edges_and_ties(ang, rot)
        print("bin_edges rot=%d: %d edges with both sides, %d ties" % (rot, len(e), len(t)))
        assert len(e) >= 3 and (len(t) >= 2 if rot % 2 == 0 else len(t) == 0), rot
    # the constructed distances themselves: k - 0.02 mm truncates to k - 1, k + 0.02 mm to k
    nominal, _ = pc.bin_edges_nominal()
    for j in range(1, len(pos)):
        if nominal[j] % 100:
            assert raw[0, j, 0] == raw[j, 0, 0] == nominal[j] // 100, j


def _features_f64(pos, nn):
    """the raw features of every ordered pair in float64 throughout (from the same float32 inputs)"""
    p, n = pos.astype(np.float64), nn.astype(np.float64)
    u = p[:, None, :] - p[None, :, :]

    def ang(a, b):
        return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1)))
    n1 = np.broadcast_to(n[:, None, :], u.shape)
    n2 = np.broadcast_to(n[None, :, :], u.shape)
    return np.stack([np.linalg.norm(u, axis=-1) * 1000.0, ang(n1, u), ang(n2, u), ang(n1, n2)], -1)


def test_bin_edges_does_not_rest_on_float_luck(oracle_lib):
    """every pair that is not a constructed exact tie -- a nominal distance of whole millimetres -- has the same raw features in
    float64 as in the reference's float arithmetic, hence the same bins at every discretisation"""
    pos, nrm, keys, raw, pairs = _ref(oracle_lib, "bin_edges", 1, 1)
    exact = _features_f64(pos, oracle_lib.normalize_rows(nrm))
    nominal, _ = pc.bin_edges_nominal()
    M = len(pos)
    checked = ties = 0
    for i in range(M):
        for j in range(M):
            if i == j:
                continue
            want = np.floor(exact[i, j]).astype(np.int64)
            if abs(int(nominal[i]) - int(nominal[j])) % 100 == 0:
                ties += 1
                assert (raw[i, j, 1:] == want[1:]).all(), (i, j)          # the angles of a distance tie are no tie
                assert abs(int(raw[i, j, 0]) - int(round(exact[i, j, 0]))) <= 1
                continue
            assert (raw[i, j] == want).all(), (i, j, raw[i, j], exact[i, j])
            frac = exact[i, j] - want
            # no feature sits within float error of a whole number, unless it is one exactly (point 0's normal lies along the axis)
            m = np.minimum(frac, 1 - frac)
            assert ((m[1:] > 1e-4) | (m[1:] == 0)).all() and m[0] > 1e-2, (i, j, exact[i, j])
            checked += 1
    assert checked > 800 and ties > 100
