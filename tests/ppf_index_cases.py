"""Model clouds and key sets for the edge tests of the PPF index (csrc/ppf_index.hip): pure numpy, no GPU.

The families put pairs ON the rules a generic model never meets -- exact 0/45/90/135/180 degree angles, coincident points, a zero
normal, integer-millimetre distances, the rounding edges and half-bin ties of `ppf_closest_bin`, the top distance bin of the
bounding-box bound -- and `reference_keys` / `shell` / `border` name the keys the device index is then asked for.
tests/test_ppf_index_cases_cpu.py checks, with the CPU oracle alone, that the families hold what they are named for;
tests/test_ppf_index_edges_gpu.py holds the device index to the oracle's literal map (`Index(literal=True)`) on them."""
import numpy as np

# (tr, rot) per family in the GPU edge test
DISCS_GENERAL = [(5, 5), (4, 6), (10, 10), (20, 30), (7, 45), (5, 180), (1, 1)]
DISCS_BIN_EDGES = [(3, 2), (4, 6), (5, 5), (10, 10)]
DISCS_FAR = [(5, 5), (10, 10), (20, 30)]
TABLE = ([(f, d) for f in ("lattice", "collinear", "sphere") for d in DISCS_GENERAL] + [("bin_edges", d) for d in DISCS_BIN_EDGES] +
         [("far_corners", d) for d in DISCS_FAR])
COARSE = {(10, 10), (20, 30), (7, 45), (5, 180)}          # save/load round trip on these
LOOKUP_CAP = 1500

_F32 = np.float32


def _pack(pos, nrm):
    return np.ascontiguousarray(pos, _F32), np.ascontiguousarray(nrm, _F32)


# ---------------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------------
LATTICE_DIRS = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1),
                         (-1, 1, 0), (1, -1, -1), (0, 0, 0)], _F32)


def lattice():
    """48 points on a 4 x 4 x 3 lattice of step 2^-7 m (exact in float), normals cycling through 13 directions (the axes, face and
    space diagonals, the zero vector), plus two exact copies of lattice point 5: one with another normal, one with the same."""
    step = 2.0 ** -7
    pts = [(x * step, y * step, z * step) for x in range(4) for y in range(4) for z in range(3)]
    nrm = [LATTICE_DIRS[i % 13] for i in range(48)]
    pts += [pts[5], pts[5]]
    nrm += [LATTICE_DIRS[(5 + 4) % 13], LATTICE_DIRS[5]]
    return _pack(pts, nrm)


def collinear():
    """40 points on a line along (1,1,1)/sqrt3 at uneven spacing; normals parallel, antiparallel and perpendicular to the line."""
    d = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    t = np.cumsum(0.0006 + 0.00044 * ((np.arange(40) * 7) % 5) + 0.00015 * ((np.arange(40) * 3) % 4))
    pos = t[:, None] * d[None, :]
    perp = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    perp2 = np.cross(d, perp)
    choice = [d, -d, perp, perp2]
    nrm = [choice[i % 4] for i in range(40)]
    return _pack(pos, nrm)


BIN_EDGE_TR = (3, 4, 5, 10)
BIN_EDGE_ROT = (2, 5, 6, 10)
# integer millimetres k with trunc = k-1 / k on the two sides of a rounding edge of closest_bin (k % d == ceil(d/2); for an even d that
# k is the exact half-bin tie): 14, 26, 38 for tr 3 and 4 (38 also for 5), 13, 23 for tr 5 (23 also for 3), 15, 25, 35 for tr 10;
# 6, 8, 10, 20 put keys next to the literal `K0 <= 5` at every tr
BIN_EDGE_MM = (14, 26, 38, 13, 23, 15, 25, 35, 6, 8, 10, 20)
# whole degrees n with trunc = n-1 / n on the two sides: 15, 45, 75, 135, 165 are edges and ties of rot 2, 6 and 10, 3, 33, 63, 93 edges
# of rot 5 (and of 2 and 6)
BIN_EDGE_DEG = (15, 45, 75, 135, 165, 3, 33, 63, 93)


def bin_edges_nominal():
    """(distance of every point from point 0 in hundredths of a millimetre, its normal's angle to the x axis in thousandths of a degree)"""
    dist = [0] + [100 * k + o for k in BIN_EDGE_MM for o in (-2, 0, 2)]
    ang_all = [1000 * n + o for n in BIN_EDGE_DEG for o in (-1, 1)]
    ang = [0] + [ang_all[i % len(ang_all)] for i in range(len(dist) - 1)]
    return np.array(dist, np.int64), np.array(ang, np.int64)


def bin_edges():
    """Point 0 at the origin with normal +x, the others on the x axis at k mm and k +- 0.02 mm, their normals at n degrees +- 1e-3
    degrees to the axis (float64, then rounded to float), each turned about the axis by its own generic angle."""
    dist, ang = bin_edges_nominal()
    x = dist.astype(np.float64) * 1e-5
    th = np.deg2rad(ang.astype(np.float64) * 1e-3)
    ph = 0.7548776662466927 * 2.0 * np.pi * np.arange(len(dist))     # a generic turn per point: no two normals in one plane
    pos = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    nrm = np.stack([np.cos(th), np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph)], 1)
    nrm[0] = (1.0, 0.0, 0.0)
    return _pack(pos, nrm)


# The side of the box.  The top distance bin (int)(diag*1000)/tr + 1 is reached only when the diagonal in whole millimetres rounds UP
# in closest_bin, i.e. (int)(diag*1000) % tr >= tr/2.  A 0.7 m cube has a 1212.4 mm diagonal: 1212 rounds down at tr = 5 and 10 and no
# pair can sit in the top bin.  0.7035 m gives 1218.4 mm, which rounds up at tr = 5, 10 and 20 alike.
FAR_SIDE = 0.7035


def far_corners():
    """Two clusters of 12 points at opposite corners of a FAR_SIDE^3 m box, the two exact corners included: the largest pair distance
    is the bounding-box diagonal."""
    rng = np.random.default_rng(11)
    a = rng.uniform(0.0, 0.02, (12, 3))
    b = FAR_SIDE - rng.uniform(0.0, 0.02, (12, 3))
    a[0] = 0.0
    b[0] = FAR_SIDE
    nrm = rng.normal(size=(24, 3))
    return _pack(np.concatenate([a, b]), nrm)


def _sphere(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    nrm = d + 0.15 * rng.normal(size=(n, 3))
    return _pack(0.05 * d, nrm)


def sphere():
    """64 random points on a 5 cm sphere with noisy outward normals: the generic control."""
    return _sphere(64, 3)


def tiny_M(m):
    """the first m (0..3) points of `sphere`"""
    pos, nrm = sphere()
    return pos[:m].copy(), nrm[:m].copy()


NAN_ID = 17


def nan_normal():
    """`sphere` with the normal of point NAN_ID set to NaN"""
    pos, nrm = sphere()
    nrm = nrm.copy()
    nrm[NAN_ID] = np.nan
    return pos, nrm


STRIDE_M = 2049


def stride():
    """2 049 points of the `sphere` kind: M^2 = 4 198 401 pairs, just over the 16 384 x 256 threads of one turn of the build's loop"""
    return _sphere(STRIDE_M, 5)


FAMILIES = {"lattice": lattice, "collinear": collinear, "bin_edges": bin_edges, "far_corners": far_corners, "sphere": sphere}


# ---------------------------------------------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------------------------------------------
_OFF0, _OFFA = 1 << 20, 1 << 11          # K0 in (-2^20, 2^20), angles in (-2048, 2048)


def pack_keys(k4):
    k = np.asarray(k4, np.int64).reshape(-1, 4)
    assert (np.abs(k[:, 0]) < _OFF0).all() and (np.abs(k[:, 1:]) < _OFFA).all()
    return ((k[:, 0] + _OFF0) << 36) | ((k[:, 1] + _OFFA) << 24) | ((k[:, 2] + _OFFA) << 12) | (k[:, 3] + _OFFA)


def unpack_keys(p):
    p = np.asarray(p, np.int64)
    return np.stack([(p >> 36) - _OFF0, ((p >> 24) & 0xFFF) - _OFFA, ((p >> 12) & 0xFFF) - _OFFA, (p & 0xFFF) - _OFFA], 1).astype(np.int32)


def unique_keys(k4):
    """the distinct rows of an (n,4) key array, in lexicographic order"""
    return unpack_keys(np.unique(pack_keys(k4)))


def features(pos, nrm, tr, rot, oracle_lib):
    """(M,M,4) int32: the oracle's feature of every ordered pair (id1,id2) on normalize_rows(nrm); the diagonal is unused (-1)"""
    M = len(pos)
    nn = oracle_lib.normalize_rows(nrm) if M else np.zeros((0, 3), _F32)
    F = np.full((M, M, 4), -1, np.int32)
    for i in range(M):
        for j in range(M):
            if i != j:
                F[i, j] = oracle_lib.ppf_compute(pos[i], nn[i], pos[j], nn[j], tr, rot)
    return F


_OFFS = np.array([(a, b, c, d) for a in (-1, 0) for b in (-2, -1, 0, 1) for c in (-2, -1, 0, 1) for d in (-2, -1, 0, 1)], np.int64)


def expand(feats, tr, rot):
    """the 128 offset keys of every feature under the reference's rule (rgbd.cpp:130-137: p1 <= 5 or a negative angle is skipped)"""
    f = np.asarray(feats, np.int64).reshape(-1, 4)
    k = (f[:, None, :] + _OFFS[None, :, :] * np.array([tr, rot, rot, rot], np.int64)).reshape(-1, 4)
    return k[(k[:, 0] > 5) & (k[:, 1:] >= 0).all(1)]


def reference_keys(pos, nrm, tr, rot, oracle_lib):
    """(keys, feats, pairs): the distinct keys of the reference's map as a sorted (n,4) array, the (M,M,4) features, and a dict from
    feature tuple to its ordered pairs in insertion order"""
    F = features(pos, nrm, tr, rot, oracle_lib)
    M = len(pos)
    pairs = {}
    for i in range(M):
        for j in range(M):
            if i != j:
                pairs.setdefault(tuple(int(v) for v in F[i, j]), []).append((i, j))
    valid = np.array([f for f in pairs if min(f) >= 0], np.int64).reshape(-1, 4)
    keys = unique_keys(expand(valid, tr, rot)) if len(valid) else np.zeros((0, 4), np.int32)
    return keys, F, pairs


def shell(keys, tr, rot):
    """Keys around the key set: every key one step out in each component, both ways (this yields the negative angles below 0 and the
    angle 180 + rot above 180); off-grid variants (a component + 1); the keys of the two lowest populated distances moved to K0 in
    {0, tr, 5, the first multiple of tr above 5}; an explicit negative angle and an explicit 180 + rot on the keys that touch those
    borders; the keys of the top distance moved to K0 + tr and K0 + 2 tr."""
    k = np.asarray(keys, np.int64).reshape(-1, 4)
    if not len(k):
        return np.array([(0, 0, 0, 0), (tr, 0, 0, 0), (5, 0, 0, 0), ((5 // tr + 1) * tr, 0, 0, 0), ((5 // tr + 1) * tr, -rot, 0, 0),
                         ((5 // tr + 1) * tr, 180 + rot, 0, 0)], np.int32)
    step = np.array([tr, rot, rot, rot], np.int64)
    out = []
    for c in range(4):
        e = np.zeros(4, np.int64)
        e[c] = 1
        out += [k + e * step, k - e * step, k + e]
    d0 = np.unique(k[:, 0])
    low = k[k[:, 0] <= d0[min(1, len(d0) - 1)]]
    for v in (0, tr, 5, (5 // tr + 1) * tr):
        m = low.copy()
        m[:, 0] = v
        out.append(m)
    for c in (1, 2, 3):
        m = k[k[:, c] == 0].copy()
        m[:, c] = -rot
        out.append(m)
        m = k[k[:, c] >= 180 - rot].copy()
        m[:, c] = 180 + rot
        out.append(m)
    top = k[k[:, 0] == d0[-1]]
    for s in (1, 2):
        m = top.copy()
        m[:, 0] += s * tr
        out.append(m)
    return unique_keys(np.concatenate(out))


def border(keys, tr, rot):
    """the keys with an angle component in {0, rot, 180 - rot, 180} or a K0 in the lowest or the top two populated distance bins"""
    k = np.asarray(keys, np.int64).reshape(-1, 4)
    if not len(k):
        return k.astype(np.int32)
    d0 = np.unique(k[:, 0])
    sel = np.isin(k[:, 1:], (0, rot, 180 - rot, 180)).any(1) | np.isin(k[:, 0], (d0[0], d0[-1], d0[max(len(d0) - 2, 0)]))
    return k[sel].astype(np.int32)


def in_key_space(keys):
    """The device's key space holds angles 0..180 only.  The reference's map also holds keys with a component of 180 + rot (the + rot
    offset of a feature at 180); no feature ever equals such a key, so nothing can look it up, and the device answers it as absent
    (deliberate divergences)."""
    k = np.asarray(keys).reshape(-1, 4)
    return (k[:, 1:] <= 180).all(1)


def _strided(packed, n):
    return packed if len(packed) <= n else packed[np.unique(np.linspace(0, len(packed) - 1, n).astype(np.int64))]


def lookup_keys(keys, keys_all, tr, rot, cap=LOOKUP_CAP):
    """The keys whose lookups are compared, of `keys_all` = reference keys | shell: all of them up to `cap`; else all of `border`
    (never dropped) plus an evenly strided sample of the sorted rest -- `cap` of the remaining reference keys (every one a non-empty
    lookup) and `cap` of the remaining shell (almost all empty).  The cap exists only for time: see DESIGN.md for the measured cost."""
    k = unique_keys(keys_all)
    if len(k) <= cap:
        return k
    b = pack_keys(border(k, tr, rot))
    rest = np.setdiff1d(pack_keys(k), b)
    rest_ref = np.intersect1d(rest, pack_keys(keys)) if len(keys) else rest[:0]
    rest_shell = np.setdiff1d(rest, rest_ref)
    return unpack_keys(np.unique(np.concatenate([b, _strided(rest_ref, cap), _strided(rest_shell, cap)])))
