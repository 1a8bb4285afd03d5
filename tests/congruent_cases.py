"""Small models that put the congruent-set join (csrc/congruent.hip, csrc/congruent_lists.h) on its edges: intersection points exactly
on position-cell faces, pair directions exactly along the axes (the anti-parallel branch of quat_from_z, direction-cell coordinates 0
and 6), position cells at the ends of the table, P runs whose lengths sit on the thresholds of join_count_kernel, and degenerate clouds.

Every model is point-mirrored and interleaved (p, -p, p', -p', ...): the sequential float centroid sum returns to exactly zero after
every pair, so centring changes nothing, the bounding box is symmetric and its centre is exactly zero.  Two anchor points +-(a, a, a)
with 2 a = fl(0.999) fix the extent: ratio = fl(0.999 + 0.001) = 1 exactly, so a model coordinate p has the unit coordinate p + 0.5,
the normalised epsilon is 0.005, the position grid has 128^3 cells of 1/128 (normalset.h:117-119), and a dyadic model coordinate
gives a dyadic unit coordinate.  The scene is the same points in the same order, moved by a signed axis permutation or an exact
(dyadic) translation; bases are scene indices with dyadic invariants.

A case is a dict: name, mpos, mnrm, spos, snrm, sprob, spix, ids (n x 4), inv (n x 2), runs (the P run lengths that must occur in a
cell some Q entry queries), expect_quads (per base: the number of quads the case was built to have; 0 where it was built to have none).  analyse() computes, from the
oracle's index alone, what a case reaches; test_congruent_cases_cpu.py asserts it, test_congruent_edges_gpu.py runs the join on it."""
import functools

import numpy as np

F = np.float32
A_ANCHOR = F(0.999) / F(2)
EG = 128
INVS = (F(0.0), F(0.25), F(0.5), F(1.0))


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def mirror(a):
    a = np.asarray(a, F)
    out = np.empty((2 * len(a), 3), F)
    out[0::2] = a
    out[1::2] = -a
    return out


ROT_Z90 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)          # (x, y, z) -> (-y, x, z): a signed axis permutation
MIRROR_XZ = np.array([[0, 0, 1], [0, -1, 0], [1, 0, 0]], F)        # (x, y, z) -> (z, -y, x)


def assemble(name, pts, nrm, ids, inv, motion, runs=(), expect_quads=None):
    """pts / nrm: the half model (its mirror image is interleaved, the anchors appended); ids index the HALF model's points (2 i in the
    full one) unless given as pairs (i, mirrored)."""
    a = A_ANCHOR
    mpos = mirror(np.concatenate([np.asarray(pts, F).reshape(-1, 3), [[a, a, a]]]))
    mnrm = mirror(np.concatenate([np.asarray(nrm, F).reshape(-1, 3), [[0, 0, 1]]]))
    assert len(mpos) <= 65535 and np.abs(mpos).max() == a
    if isinstance(motion, np.ndarray) and motion.shape == (3, 3):
        spos, snrm = (mpos @ motion.T).astype(F), (mnrm @ motion.T).astype(F)
        assert np.array_equal(np.sort(np.abs(spos), 1), np.sort(np.abs(mpos), 1))       # exact: a permutation of the coordinates and signs
    else:
        spos, snrm = (mpos + np.asarray(motion, F)).astype(F), mnrm.copy()
        assert np.array_equal((spos - np.asarray(motion, F)).astype(F)[:-2], mpos[:-2])   # exact translation (of all but the anchors, which no base uses)
    ids = np.asarray(ids, np.int32).reshape(-1, 4)
    return dict(name=name, mpos=mpos, mnrm=mnrm, spos=spos, snrm=snrm, sprob=np.ones(len(spos), F), spix=np.zeros((len(spos), 2), np.int32),
                ids=ids, inv=np.asarray(inv, F).reshape(-1, 2), runs=tuple(runs), expect_quads=expect_quads)


# ---- lattice ----
DIRS18 = _unit([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0],
                [1, 0, 1], [1, 0, -1], [-1, 0, 1], [-1, 0, -1], [0, 1, 1], [0, 1, -1], [0, -1, 1], [0, -1, -1]])


def _lattice_points():
    """6 x 6 x 6 points, spacing 1/16 = 8 position cells.  x: +-{1, 3, 5}/32 -- every x is on a cell face (128 x = 64 +- 4 k) and so is
    every quarter point and midpoint; y: the same pushed outwards by 1/512 (a quarter cell), z: by 1/1024 -- on a face only where a
    mirrored pair's midpoint cancels the push.  -> the half with x > 0 (108 points; the other half is its mirror image)"""
    c = np.array([1, 3, 5], np.float64) / 32
    xs = np.concatenate([-c[::-1], c])
    ys = np.concatenate([-(c[::-1] + 1 / 512), c + 1 / 512])
    zs = np.concatenate([-(c[::-1] + 1 / 1024), c + 1 / 1024])
    g = np.array([(x, y, z) for x in xs if x > 0 for y in ys for z in zs])
    assert np.array_equal(g.astype(F).astype(np.float64), g)
    return g.astype(F)


def lattice():
    pts = _lattice_points()
    nrm = DIRS18[(np.arange(len(pts)) * 7) % 18]
    idx = {tuple(np.round(p * 1024).astype(int)): i for i, p in enumerate(pts)}

    def at(ix, iy, iz):                       # lattice steps 0..5 per axis -> model id (a point with x < 0 is the mirror image of one with x > 0)
        c = (np.array([-5, -3, -1, 1, 3, 5]) * 32, np.array([-162, -98, -34, 34, 98, 162]), np.array([-161, -97, -33, 33, 97, 161]))
        x, y, z = c[0][ix], c[1][iy], c[2][iz]
        return 2 * idx[(x, y, z)] if x > 0 else 2 * idx[(-x, -y, -z)] + 1
    ids, inv = [], []
    # pairs along the axes in both senses (Q directions exactly +-x, +-y, +-z), every dyadic invariant
    # (each base's two segments cross at the point its invariants name, so the base itself is one of its quads)
    ids.append([at(3, 3, 4), at(5, 3, 4), at(4, 3, 5), at(4, 3, 3)]); inv.append([0.5, 0.5])       # P along +x, Q along -z, crossing at a lattice point
    ids.append([at(4, 3, 4), at(4, 5, 4), at(4, 4, 3), at(4, 4, 5)]); inv.append([0.5, 0.5])       # P along +y, Q along +z
    ids.append([at(4, 1, 5), at(4, 1, 3), at(5, 1, 4), at(1, 1, 4)]); inv.append([0.5, 0.25])      # P along -z, Q along -x over four spacings, its quarter point
    ids.append([at(5, 5, 2), at(3, 5, 2), at(3, 5, 2), at(3, 3, 2)]); inv.append([1.0, 0.0])       # P along -x ends where Q along -y starts
    ids.append([at(3, 2, 3), at(3, 2, 5), at(1, 2, 3), at(3, 2, 3)]); inv.append([0.0, 1.0])       # P along +z starts where Q along +x ends
    ids.append([at(0, 0, 1), at(4, 0, 1), at(1, 0, 0), at(1, 0, 2)]); inv.append([0.25, 0.5])      # x < 0: the quarter point of four spacings, Q along +z
    ids.append([at(0, 2, 3), at(1, 3, 3), at(0, 3, 3), at(1, 2, 3)]); inv.append([0.5, 0.5])       # two face diagonals crossing at their midpoints
    ids.append([at(0, 1, 1), at(1, 2, 2), at(1, 1, 2), at(0, 2, 1)]); inv.append([0.5, 0.5])       # two space diagonals of one lattice cube
    ids.append([at(0, 2, 2), at(0, 3, 3), at(0, 3, 2), at(0, 2, 3)]); inv.append([0.5, 0.5])       # mirrored y and z: a midpoint on a face of all three axes
    return assemble("lattice", pts, nrm, ids, inv, ROT_Z90, expect_quads=(7, 24, 14, 8, 8, 8, 4, 8, 6))


# ---- clusters ----
DELTA = 2.0 ** -16          # spacing inside a cluster: 16 points across are 0.03 of a position cell


def _cluster(centre, n):
    k = np.arange(n)
    off = np.stack([(k % 16) * DELTA, (k // 16) * DELTA, ((k * 5) % 7) * DELTA], -1)
    centre = np.round(np.asarray(centre, np.float64) / DELTA) * DELTA          # every coordinate a multiple of 2^-16: translations by 2^-4 are exact
    return (centre[None, :] + off - np.round(off.mean(0) / DELTA) * DELTA).astype(F)


def _cluster_group(cell, u, v, d_ab, d_cd, na, nb, nc, nd, inv1, inv2):
    """Clusters A, B (|B - A| = d_ab along u) and C, D (d_cd along v) whose segments cross at the centre X of position cell `cell`:
    X = A + inv1 (B - A) = C + inv2 (D - C)."""
    X = (np.asarray(cell, np.float64) + 0.5) / EG - 0.5
    u, v = np.asarray(u, np.float64) / np.linalg.norm(u), np.asarray(v, np.float64) / np.linalg.norm(v)
    A, B = X - inv1 * d_ab * u, X + (1 - inv1) * d_ab * u
    Cc, D = X - inv2 * d_cd * v, X + (1 - inv2) * d_cd * v
    pts = [_cluster(A, na), _cluster(B, nb), _cluster(Cc, nc), _cluster(D, nd)]
    w = np.cross(u, v)
    nrm = [np.tile(_unit(n), (len(p), 1)) for n, p in zip((w + 0.3 * u, w - 0.4 * u, w + 0.5 * v, w - 0.2 * v), pts)]
    return pts, nrm


GROUPS = (  # (|A|, |B|), position cell, direction of A -> B, of C -> D, |AB|, |CD| in metres
    ((7, 9), (20, 30, 40), (0.60, 0.64, 0.48), (0.64, -0.60, 0.30), 0.040, 0.050),
    ((8, 8), (100, 30, 50), (0.10, 0.70, 0.70), (0.29, 0.03, 0.55), 0.060, 0.070),
    ((5, 13), (30, 100, 60), (0.80, 0.10, 0.59), (-0.10, 0.90, 0.40), 0.080, 0.090),
    ((15, 17), (90, 90, 30), (0.30, -0.50, 0.81), (0.70, 0.65, 0.20), 0.100, 0.110),
    ((16, 16), (40, 60, 100), (-0.60, 0.50, 0.62), (0.55, 0.80, 0.10), 0.120, 0.130),
    ((13, 20), (64, 64, 64), (0.45, 0.45, 0.77), (-0.51, -1.65, 0.17), 0.140, 0.150),
)


def clusters():
    """P runs of 63, 64, 65 (JOIN_RUN_MIN = 64) and 255, 256, 260 (the 256-entry stride of the histogram loop): all |A| x |B| pairs of a
    group land in ONE position cell (inv1 = 0.25: the reversed pairs land elsewhere), in one direction cell, and the group's 3 x 4 Q
    pairs (and their reverses, inv2 = 0.5) query it."""
    pts, nrm, ids, inv, runs, start = [], [], [], [], [], 0
    for (na, nb), cell, u, v, dab, dcd in GROUPS:
        p, n = _cluster_group(cell, u, v, dab, dcd, na, nb, 3, 4, 0.25, 0.5)
        first = np.cumsum([0] + [len(x) for x in p])[:4] + start
        ids.append(2 * first); inv.append([0.25, 0.5])
        runs.append(na * nb)
        pts += p; nrm += n
        start += sum(len(x) for x in p)
    return assemble("clusters", np.concatenate(pts), np.concatenate(nrm), ids, inv, np.array([0.25, -0.125, 0.0625], F), runs=runs,
                    expect_quads=tuple(24 * r for r in runs))       # every one of the 24 Q entries matches the whole run


GROUPS_64K = (
    ((255, 257), (30, 40, 90), (0.60, 0.64, 0.48), (0.64, -0.60, 0.30), 0.100, 0.110),
    ((256, 256), (90, 80, 40), (0.30, -0.50, 0.81), (0.70, 0.65, 0.20), 0.120, 0.130),
)


def clusters_64k():
    """P runs of 65 535 and 65 536 entries: either side of the (hi - lo) < 65536 guard of join_count_kernel's histogram path, and -- every
    entry of a run sits in ONE direction cell -- a 16-bit histogram counter at 65 535.  3 x 4 Q pairs (and their reverses) query each run.
    Oracle time on the CPU that built this case: index 0.5 s, find_congruent + find_congruent_seq of both bases 5 s."""
    pts, nrm, ids, inv, runs, start = [], [], [], [], [], 0
    for (na, nb), cell, u, v, dab, dcd in GROUPS_64K:
        p, n = _cluster_group(cell, u, v, dab, dcd, na, nb, 3, 4, 0.25, 0.5)
        first = np.cumsum([0] + [len(x) for x in p])[:4] + start
        ids.append(2 * first); inv.append([0.25, 0.5])
        runs.append(na * nb)
        pts += p; nrm += n
        start += sum(len(x) for x in p)
    return assemble("clusters_64k", np.concatenate(pts), np.concatenate(nrm), ids, inv, np.array([-0.125, 0.25, 0.0625], F), runs=runs,
                    expect_quads=tuple(24 * r for r in runs))


# ---- borders ----
def borders():
    """Intersection points in the first and the last position cell of every axis (cells 0 and 127: the anchors' own cells, unit coordinates
    0.0005 and 0.9995, and clusters beside them), pair directions exactly along the axes there (direction-cell coordinates 0 and 6)."""
    a = float(A_ANCHOR)
    s = 2.0 ** -9                       # a quarter cell
    pts, nrm, ids, inv = [], [], [], []
    # per axis: two points in the last cell on that axis (the mirror images are in the first), joined along each of the other two axes
    for ax in range(3):
        o1, o2 = (ax + 1) % 3, (ax + 2) % 3
        base = np.zeros(3); base[ax] = a - s
        for k, (du, dv) in enumerate(((0.0625, 0.0), (-0.0625, 0.0), (0.0, 0.0625), (0.0, -0.0625), (0.125, 0.0), (0.0, 0.125), (0.0, 0.0))):
            p = base.copy(); p[o1] += du; p[o2] += dv
            pts.append(p); nrm.append(DIRS18[(3 * ax + k) % 18])
    pts, nrm = np.array(pts), np.array(nrm)
    for ax in range(3):
        g = 7 * ax
        # P pair along +o1 ... -o1 through the cell's point, Q pair along +o2 ... -o2: both cross at `base`
        ids.append([2 * (g + 1), 2 * (g + 0), 2 * (g + 3), 2 * (g + 2)]); inv.append([0.5, 0.5])
        ids.append([2 * (g + 1) + 1, 2 * (g + 0) + 1, 2 * (g + 2) + 1, 2 * (g + 3) + 1]); inv.append([0.5, 0.5])     # the mirror images: first cell
        ids.append([2 * (g + 6), 2 * (g + 0), 2 * (g + 6), 2 * (g + 2)]); inv.append([0.0, 0.0])                       # invariant 0: both pairs start at the cell's point
        ids.append([2 * (g + 1) + 1, 2 * (g + 6) + 1, 2 * (g + 3) + 1, 2 * (g + 6) + 1]); inv.append([1.0, 1.0])       # invariant 1: both end there, first cell
    return assemble("borders", pts, nrm, ids, inv, MIRROR_XZ, expect_quads=(16, 16, 2, 2) + (2, 2, 2, 2) + (4, 4, 4, 4))


# ---- degenerate ----
def degenerate_coincident():
    """Every point of a 3 x 3 x 3 lattice twice (one of them three times), same normal: coincident model points -- pairs of distance zero are
    not indexed, every other pair occurs several times over."""
    c = np.array([1, 3, 5], np.float64) / 32
    g = np.array([(x, y + 1 / 512, z + 1 / 1024) for x in c for y in c for z in c])
    pts = np.concatenate([g, g, g[:1]])
    nrm = np.concatenate([DIRS18[(np.arange(27) * 5) % 18]] * 2 + [DIRS18[:1]])
    # point (ix, iy, iz) is 9 ix + 3 iy + iz, its copy 27 more, the third copy of point 0 is 54
    ids = [[2 * 4, 2 * 22, 2 * 10, 2 * 16],                 # P along +x and Q along +y through point 13, midpoints
           [2 * (4 + 27), 2 * 22, 2 * 10, 2 * (16 + 27)],   # the same through the copies
           [2 * 4, 2 * 22, 2 * 4, 2 * 22],                  # the same pair twice: cos alpha = 1, no cone samples, no quads (Q9)
           [2 * 4, 2 * 13, 2 * 13, 2 * 4],                  # a pair and its reverse, invariants 0 and 1: cos alpha = -1
           [2 * 54, 2 * 18, 2 * 6, 2 * 27]]                 # the point that exists three times: P starts at it, Q ends at it
    inv = [[0.5, 0.5], [0.5, 0.5], [0.5, 0.5], [0.0, 1.0], [0.0, 1.0]]
    return assemble("degenerate_coincident", pts, nrm, ids, inv, ROT_Z90, expect_quads=(64, 64, 0, 232, 72))


def degenerate_planar():
    c = np.array([1, 3, 5], np.float64) / 32
    xs = np.concatenate([-c[::-1], c])
    g = np.array([(x, y, 0.0) for x in c for y in xs] + [(0.0, y, 0.0) for y in c])
    nrm = DIRS18[(np.arange(len(g)) * 7 + 4) % 18]
    # point (ix, iy) is 6 ix + iy
    ids = [[2 * 2, 2 * 14, 2 * 7, 2 * 9],                   # P along +x, Q along +y, crossing at point 8
           [0, 2 * 7, 2 * 1, 2 * 6],                        # the diagonals of one lattice square
           [0, 2 * 6, 0, 2 * 6],                            # the same pair twice
           [2 * 2, 2 * 8, 2 * 8, 2 * 9]]                    # P ends where Q starts
    inv = [[0.5, 0.5], [0.5, 0.5], [1.0, 0.0], [1.0, 0.0]]
    return assemble("degenerate_planar", g, nrm, ids, inv, MIRROR_XZ, expect_quads=(2, 4, 0, 2))


def degenerate_collinear():
    """Twelve points on the x axis: every pair direction is exactly +-x, and a base's two pairs are parallel (cos alpha = 1: no cone samples,
    no quads, Q9) or opposed (cos alpha = -1: 56 samples at sin(pi))."""
    x = np.array([1, 2, 3, 5, 8, 13], np.float64) / 32
    g = np.stack([x, np.zeros(6), np.zeros(6)], -1)
    nrm = DIRS18[[2, 4, 2, 4, 14, 2]]
    ids = [[2 * 1, 2 * 4, 2 * 4, 2 * 1],                    # a pair and its reverse, midpoints
           [2 * 1, 2 * 4, 2 * 4, 2 * 1],                    # ... invariants 0 and 1
           [0, 2 * 2, 2 * 3, 2 * 1],                        # opposed pairs of different lengths
           [0, 2 * 2, 0, 2 * 2]]                            # the same pair twice: parallel, no samples
    inv = [[0.5, 0.5], [0.0, 1.0], [0.5, 0.5], [0.0, 1.0]]
    return assemble("degenerate_collinear", g, nrm, ids, inv, np.array([0.5, 0.0, -0.25], F), expect_quads=(4, 4, 0, 0))


BUILDERS = {"lattice": lattice, "clusters": clusters, "clusters_64k": clusters_64k, "borders": borders, "degenerate_coincident": degenerate_coincident,
            "degenerate_planar": degenerate_planar, "degenerate_collinear": degenerate_collinear}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def build(name):
    return BUILDERS[name]()


def make_oracle(pyoracle, case):
    return pyoracle.Oracle(case["spos"], case["snrm"], case["sprob"], case["spix"], case["mpos"], case["mnrm"], build_index=True)


def analyse(pyoracle, orc, case, index_pos_rows=None, index_normal_rows=None):
    """What the join of every base of a case meets, from the oracle's index and the cell functions alone (the reference's own where
    given, else numpy restatements of normalset.h:97-104): per base a dict with the P / Q pair lists, their intersection points (unit
    cube, float32), position cells, direction cells, directions, the P run length of every position cell, and the cells some Q entry queries."""
    mpos = orc.model_centred()
    assert np.array_equal(mpos, case["mpos"])                 # centring changed nothing
    unit = (mpos / F(1.0) + F(0.5)).astype(F)
    spos, snrm = orc.scene_centred(), pyoracle.normalize_rows(case["snrm"])
    neps = F(np.float64(F(1.0) / F(7.0)) + 0.00001)

    def pos_cells(p):
        if index_pos_rows is not None:
            return index_pos_rows(0.005, p).astype(np.int64)
        c = (p / F(1.0 / EG)).astype(np.int64)
        return c[:, 2] * EG * EG + c[:, 1] * EG + c[:, 0]

    def dir_cells(d):
        if index_normal_rows is not None:
            return index_normal_rows(d).astype(np.int64)
        c = ((d / F(2.0) + F(0.5)) / neps).astype(np.int64)
        return c[:, 2] * 49 + c[:, 1] * 7 + c[:, 0]

    def side(pairs, inv):
        p1, p2 = unit[pairs[:, 0]], unit[pairs[:, 1]]
        x = (p1 + F(inv) * (p2 - p1)).astype(F)
        d = p2 - p1
        z = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.where((z > 0)[:, None], d / np.sqrt(z)[:, None], d).astype(F)
        return dict(pairs=pairs, x=x, dir=d, cell=pos_cells(x), dcell=dir_cells(d))
    out = []
    for ids, inv in zip(case["ids"], case["inv"]):
        K = [pyoracle.ppf_compute(spos[ids[2 * j]], snrm[ids[2 * j]], spos[ids[2 * j + 1]], snrm[ids[2 * j + 1]]) for j in (0, 1)]
        P, Q = (orc.index_lookup(k).reshape(-1, 2) for k in K)
        rec = dict(K=K, P=side(P, inv[0]), Q=side(Q, inv[1]))
        if len(P) == 0 or len(Q) == 0:                       # stocs.cpp:788: neither list is used
            rec["runs"], rec["queried"] = {}, set()
        else:
            cells, counts = np.unique(rec["P"]["cell"], return_counts=True)
            rec["runs"] = dict(zip(cells.tolist(), counts.tolist()))
            rec["queried"] = set(rec["Q"]["cell"].tolist())
        out.append(rec)
    return out
