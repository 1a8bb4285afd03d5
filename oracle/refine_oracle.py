"""Plain reference of the refinement's first evaluation (stocs_refine_detail / stocs_refine_poses, csrc/refine.hip) and the cases that
pin it at its edges.  numpy only: brute force over all model points in float64 on the float32 values the context holds.

Per source point: the model indices at the minimum squared distance d1, the next distinct distance d2 and a class --
    TIE    two or more indices at d1: the expected match is the lowest index;
    CLEAR  d2 > d1 (1 + 2^-20): the expected match is the argmin;
    AMBIG  otherwise: any index whose distance is <= d1 (1 + 2^-20) is accepted.
The margin: the kernel forms d^2 from three float subtractions and two fmas, a relative error below 2^-22; 2^-20 sits two bits above.
The threshold works the same way with D2 = float64(float32(dist))^2 (see expected()).

Constructed cases are seeded, point-symmetric (both centroids exactly 0) and dyadic where ties and thresholds are meant to be exact."""
import math
from fractions import Fraction

import numpy as np

F = np.float32
MARGIN = 2.0 ** -20
TIE, CLEAR, AMBIG = 0, 1, 2
LDS_BYTES = 48 << 10
OCTANT_DENSITY = 32
MAX_CELLS = 1 << 18


# ---------------------------------------------------------------- what the context holds
def centre(cloud):
    """centroid_shift as the context does it: sequential float sums, one division, one subtraction -> (centred float32, centroid)"""
    p = np.ascontiguousarray(cloud, F)
    c = (np.cumsum(p, axis=0, dtype=F)[-1] / F(len(p))).astype(F)
    return (p - c).astype(F), c


def identity_hyp(t=(0.0, 0.0, 0.0)):
    """column-major [I | t], centred model -> centred scene"""
    T = np.eye(4, dtype=F).T.reshape(16).copy()
    T[12:15] = np.asarray(t, F)
    return T


def source_points(scene_c, T16, src_idx=None):
    """the source in the model frame as the kernel sees it at U = I, for a hypothesis [I | t]: float(x - t), one rounding"""
    T = np.asarray(T16, F).reshape(4, 4).T
    assert np.array_equal(T[:3, :3], np.eye(3, dtype=F)), "exact source only for [I | t]"
    x = scene_c if src_idx is None else scene_c[np.asarray(src_idx, np.int64)]
    return (x.astype(np.float64) - T[:3, 3].astype(np.float64)).astype(F)


# ---------------------------------------------------------------- the grid, as build_refine_grid computes it
def predict_grid(model_c, dist):
    m = np.ascontiguousarray(model_c, F)
    d = F(dist)
    mn, mx = m.min(0), m.max(0)
    h = F(d * F(1.001))
    raised = 0
    while True:
        inv_h = F(1.0) / h
        n3 = [int(np.floor(F(F(mx[k] - mn[k]) * inv_h))) + 1 for k in range(3)]
        cells = n3[0] * n3[1] * n3[2]
        if cells <= MAX_CELLS:
            break
        h = F(h * F(1.25))
        raised += 1
    nM = len(m)
    return dict(o=mn, h=h, inv_h=F(1.0) / h, n3=n3, cells=cells, raised=raised, lo=(mn - d).astype(F), hi=(mx + d).astype(F),
                lds=nM * 16 + (8 * cells + 1) * 4 <= LDS_BYTES, octants=nM >= OCTANT_DENSITY * cells)


def cell_units(g, x, k):
    """(x - o) * inv_h along axis k in float, as the kernels form it"""
    return F(F(F(x) - g["o"][k]) * g["inv_h"])


def face_floats(g, k, face, half=False):
    """the largest float whose cell coordinate along axis k is below `face` (+ 0.5 with half) and the smallest one at or above it"""
    target = F(face + (0.5 if half else 0.0))
    x = F(np.float64(g["o"][k]) + np.float64(target) * np.float64(g["h"]))
    while cell_units(g, x, k) >= target:
        x = np.nextafter(x, F(-np.inf))
    while cell_units(g, np.nextafter(x, F(np.inf)), k) < target:
        x = np.nextafter(x, F(np.inf))
    return x, np.nextafter(x, F(np.inf))


def in_box(g, s):
    return ((s >= g["lo"]) & (s <= g["hi"])).all(1)


# ---------------------------------------------------------------- brute force
def classify(src, model_c, block=2048):
    """-> dict: d1, d2 (inf: no second distance), low (lowest index at d1), ntie (indices at d1), cls"""
    s = np.asarray(src, F).astype(np.float64)
    m = np.asarray(model_c, F).astype(np.float64)
    n = len(s)
    d1 = np.zeros(n); d2 = np.full(n, np.inf); low = np.zeros(n, np.int64); ntie = np.zeros(n, np.int64)
    for a in range(0, n, block):
        b = min(n, a + block)
        D = ((s[a:b, None, :] - m[None, :, :]) ** 2).sum(2)
        mnv = D.min(1)
        eq = D == mnv[:, None]
        d1[a:b] = mnv
        low[a:b] = eq.argmax(1)
        ntie[a:b] = eq.sum(1)
        d2[a:b] = np.where(eq, np.inf, D).min(1)
    cls = np.where(ntie >= 2, TIE, np.where(d2 > d1 * (1.0 + MARGIN), CLEAR, AMBIG))
    return dict(d1=d1, d2=d2, low=low, ntie=ntie, cls=cls)


def dist2(src, model_c, idx):
    s = np.asarray(src, F).astype(np.float64)
    t = np.asarray(model_c, F).astype(np.float64)[idx]
    return ((s - t) ** 2).sum(1)


def check_detail(src, model_c, dist, grid, match, counted, exact_threshold, cl=None):
    """every way the kernel's (match, counted) may contradict the classes -> list of (i, reason); empty: all is well.
    D2 = float64(float32(dist))^2 decides `counted` (ambiguous within D2 2^-20 unless exact_threshold); the walk starts at
    F2 = float32(D2 (1 + 1e-5)): a nearest point beyond F2 (1 + 2^-20), or a source outside the widened box, must give -1, one
    within F2 (1 - 2^-20) inside the box must be found."""
    cl = cl or classify(src, model_c)
    D2 = float(F(dist)) ** 2
    F2 = float(F(D2 * (1.0 + 1e-5)))
    inside = in_box(grid, np.asarray(src, F))
    bad = []
    match = np.asarray(match, np.int64)
    has = match >= 0
    dm = np.full(len(match), np.inf)
    if has.any():
        dm[has] = dist2(np.asarray(src)[has], model_c, match[has])
    for i in range(len(match)):
        d1 = cl["d1"][i]
        if not has[i]:
            if counted[i]:
                bad.append((i, "counted without a match"))
            if inside[i] and d1 <= F2 * (1.0 - MARGIN):
                bad.append((i, "no match though the nearest point is inside the search bound"))
            continue
        if not inside[i]:
            bad.append((i, "match outside the widened box"))
        if d1 > F2 * (1.0 + MARGIN):
            bad.append((i, "match beyond the search bound"))
        c = cl["cls"][i]
        if c != AMBIG and match[i] != cl["low"][i]:
            bad.append((i, "tie broken to %d, lowest index is %d" % (match[i], cl["low"][i]) if c == TIE else "match %d, nearest is %d" % (match[i], cl["low"][i])))
        if c == AMBIG and dm[i] > d1 * (1.0 + MARGIN):
            bad.append((i, "match %d is not among the nearest" % match[i]))
        want = dm[i] <= D2
        if bool(counted[i]) != want and (exact_threshold or abs(dm[i] - D2) > D2 * MARGIN):
            bad.append((i, "counted %d at d^2 = %.17g against %.17g" % (counted[i], dm[i], D2)))
    return bad


def ambiguous_share(src, model_c, dist, exact_threshold, cl=None):
    cl = cl or classify(src, model_c)
    D2 = float(F(dist)) ** 2
    amb = cl["cls"] == AMBIG
    if not exact_threshold:
        amb = amb | (np.abs(cl["d1"] - D2) <= D2 * MARGIN)
    return float(amb.mean()) if len(amb) else 0.0


# ---------------------------------------------------------------- sums and the one-iteration pose
def _rows(s, t, n):
    """per pair: a = [s x n, n], b = (t - s) . n and the sums of the absolute elementary products behind them"""
    a = np.concatenate([np.cross(s, n), n], axis=1)
    b = ((t - s) * n).sum(1)
    an = np.abs(n)
    ma = np.concatenate([np.stack([np.abs(s[:, 1] * n[:, 2]) + np.abs(s[:, 2] * n[:, 1]), np.abs(s[:, 2] * n[:, 0]) + np.abs(s[:, 0] * n[:, 2]),
                                   np.abs(s[:, 0] * n[:, 1]) + np.abs(s[:, 1] * n[:, 0])], 1), an], axis=1)
    mb = (np.abs(t - s) * an).sum(1)
    return a, b, ma, mb


def exact_sums(src, model_c, model_n, match, counted, use_fractions=None):
    """-> (sums28 as float64 of the exact value, bound28): A^T A upper triangle row by row | A^T b | count over the counted pairs, from
    the float64 images of s, t, n.  Exact rational arithmetic up to 300 pairs; beyond, longdouble products split into two doubles and
    math.fsum (an error of 2^-63 per product, far inside the bound).  bound = (n + 8) 2^-53 sum |elementary products|: one rounding
    per difference, product and addition of the device's double arithmetic, whatever the order of the sum."""
    sel = np.nonzero(np.asarray(counted) != 0)[0]
    n = len(sel)
    out = np.zeros(28); mag = np.zeros(28)
    out[27] = n
    if n == 0:
        return out, mag
    s = np.asarray(src, F)[sel].astype(np.float64)
    idx = np.asarray(match, np.int64)[sel]
    t = np.asarray(model_c, F)[idx].astype(np.float64)
    nn = np.asarray(model_n, F)[idx].astype(np.float64)
    a, b, ma, mb = _rows(s, t, nn)
    if use_fractions is None:
        use_fractions = n <= 300
    if use_fractions:
        fr = lambda v: [Fraction(float(x)) for x in v]
        A, B = [], []
        for i in range(n):
            S, T_, N = fr(s[i]), fr(t[i]), fr(nn[i])
            A.append([S[1] * N[2] - S[2] * N[1], S[2] * N[0] - S[0] * N[2], S[0] * N[1] - S[1] * N[0], N[0], N[1], N[2]])
            B.append(sum((T_[k] - S[k]) * N[k] for k in range(3)))
    else:
        L = np.longdouble
        sl, tl, nl = s.astype(L), t.astype(L), nn.astype(L)
        al = np.concatenate([np.cross(sl, nl), nl], axis=1)
        bl = ((tl - sl) * nl).sum(1)

    def total(u, v):
        if use_fractions:
            return float(sum(x * y for x, y in zip(u, v)))
        p = u * v
        hi = p.astype(np.float64)
        lo = (p - hi.astype(np.longdouble)).astype(np.float64)
        return math.fsum(list(hi) + list(lo))
    k = 0
    for r in range(6):
        for c in range(r, 6):
            out[k] = total([x[r] for x in A], [x[c] for x in A]) if use_fractions else total(al[:, r], al[:, c])
            mag[k] = (ma[:, r] * ma[:, c]).sum()
            k += 1
    for r in range(6):
        out[21 + r] = total([x[r] for x in A], B) if use_fractions else total(al[:, r], bl)
        mag[21 + r] = (ma[:, r] * mb).sum()
    return out, (n + 8) * 2.0 ** -53 * mag


def _solve(A, b):
    """Gaussian elimination with partial pivoting in the dtype of A (numpy has no longdouble solve)"""
    A = A.copy(); b = b.copy(); n = len(b)
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]] = A[[p, c]]; b[[c, p]] = b[[p, c]]
        for r in range(c + 1, n):
            f = A[r, c] / A[c, c]
            A[r, c:] -= f * A[c, c:]
            b[r] -= f * b[c]
    x = np.zeros(n, A.dtype)
    for r in range(n - 1, -1, -1):
        x[r] = (b[r] - (A[r, r + 1:] * x[r + 1:]).sum()) / A[r, r]
    return x


def one_iteration(T16, src, model_c, model_n, match, counted, dtype=np.float64):
    """T U^-1 after one update from the kernel's OWN correspondences (no tie ambiguity left), in `dtype` -> (4x4, cond(A^T A))"""
    sel = np.nonzero(np.asarray(counted) != 0)[0]
    idx = np.asarray(match, np.int64)[sel]
    s = np.asarray(src, F)[sel].astype(dtype)
    t = np.asarray(model_c, F)[idx].astype(dtype)
    n = np.asarray(model_n, F)[idx].astype(dtype)
    A = np.concatenate([np.cross(s, n), n], axis=1)
    b = ((t - s) * n).sum(1)
    AtA, Atb = A.T @ A, A.T @ b
    x = _solve(AtA, Atb)
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    U = np.eye(4, dtype=dtype)
    U[:3, :3] = np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa], [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                          [-sb, cb * sa, cb * ca]], dtype)
    U[:3, 3] = x[3:]
    Ui = np.eye(4, dtype=dtype)
    Ui[:3, :3] = U[:3, :3].T
    Ui[:3, 3] = -(U[:3, :3].T @ U[:3, 3])
    T = np.asarray(T16, F).reshape(4, 4).T.astype(dtype)
    return T @ Ui, float(np.linalg.cond(AtA.astype(np.float64)))


def pose_tolerance(T_ref, cond):
    """per entry: 4 float32 ulps of the entry (the rounding of T U^-1 to float) + cond(A^T A) 2^-50"""
    ref = np.asarray(T_ref, np.float64)[:3, :]
    return 4.0 * np.spacing(np.abs(ref).astype(F)).astype(np.float64) + cond * 2.0 ** -50


def scaled_hyp(T16, scale=1.25):
    """the hypothesis with its linear part scaled: invertible, not rigid"""
    T = np.asarray(T16, F).copy()
    T[[0, 1, 2, 4, 5, 6, 8, 9, 10]] *= F(scale)
    return T


def source_general(scene_c, T16, src_idx=None):
    """the source for any invertible hypothesis: T^-1 x in float64, rounded to float (the general inverse)"""
    T = np.asarray(T16, F).reshape(4, 4).T.astype(np.float64)
    Ti = np.linalg.inv(T)
    x = scene_c if src_idx is None else scene_c[np.asarray(src_idx, np.int64)]
    return (x.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(F)


# ---------------------------------------------------------------- cases
class Case:
    """model / scene: raw clouds handed to the estimator; T16: the hypothesis; exact: thresholds and ties are bitwise (dyadic
    construction, centroids exactly 0); expect: what the grid prediction must say; unit: metres (1) or millimetres (1000)"""

    def __init__(self, family, name, model, scene, dist, model_nrm=None, T16=None, src_idx=None, exact=True, expect=None, unit=1.0, seed=0):
        self.family, self.name, self.dist, self.exact, self.unit = family, name, float(F(dist)), exact, unit
        self.model = np.ascontiguousarray(model, F)
        self.scene = np.ascontiguousarray(scene, F)
        rng = np.random.default_rng(seed + 977)
        if model_nrm is None:
            v = rng.normal(size=(len(self.model), 3))
            model_nrm = v / np.linalg.norm(v, axis=1)[:, None]
        self.model_nrm = np.ascontiguousarray(model_nrm, F)
        self.T16 = identity_hyp() if T16 is None else np.asarray(T16, F)
        self.src_idx = None if src_idx is None else np.asarray(src_idx, np.int32)
        self.expect = expect or {}

    @property
    def id(self):
        return "%s-%s" % (self.family, self.name)

    def estimator_inputs(self):
        n = len(self.scene)
        nrm = np.tile(np.array([0.0, 0.0, 1.0], F), (n, 1))
        pix = np.stack([np.arange(n) // 640 % 480, np.arange(n) % 640], 1).astype(np.int32)
        return self.scene, nrm, np.ones(n, F), pix, self.model, self.model_nrm

    def unit_normals(self):
        """normalized3 of the context, in float"""
        n = self.model_nrm
        z = np.sqrt((n[:, 0] * n[:, 0] + (n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])).astype(F)).astype(F)   # dot3's order
        return (n / z[:, None]).astype(F)

    def held(self):
        """(scene_c, model_c, source) as the context holds them"""
        sc, _ = centre(self.scene)
        mc, _ = centre(self.model)
        return sc, mc, source_points(sc, self.T16, self.src_idx)


def _sym(p, rng=None, pairs=False):
    """point-symmetric cloud: p and -p.  pairs: (p_i, -p_i) adjacent, so the sequential centroid sum is exactly 0 for any floats;
    else a seeded shuffle (dyadic coordinates: every partial sum is exact)"""
    p = np.asarray(p, np.float64)
    if pairs:
        q = np.empty((2 * len(p), 3)); q[0::2] = p; q[1::2] = -p
        return q
    q = np.concatenate([p, -p])
    return q[rng.permutation(len(q))] if rng is not None else q


def _lattice(k, a):
    g = np.arange(-k, k + 1)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float64) * a


def lattice_ties(unit=1.0, seed=1):
    """lattice model, sources at lattice points and edge / face / body centres: 1-, 2-, 4- and 8-way ties, index order scrambled"""
    rng = np.random.default_rng(seed)
    a = 2.0 ** -6 * unit
    lat = _lattice(4, a)
    model = lat[rng.permutation(len(lat))]                     # symmetric as a set; dyadic: any order sums exactly
    inner = lat[(np.abs(lat) < 4 * a).all(1)]
    src = inner[rng.integers(0, len(inner), 600)] + rng.integers(0, 2, (600, 3)) * (a / 2)
    fam = "lattice_ties" if unit == 1.0 else "millimetres"
    return Case(fam, "step2^-6", model, _sym(src, rng), 2.0 ** -5 * unit, unit=unit, seed=seed, expect=dict(ties={2, 4, 8}))


def duplicates(seed=2):
    """every lattice point three times at scattered indices; sources on the points and between them"""
    rng = np.random.default_rng(seed)
    a = 2.0 ** -6
    lat = _lattice(2, a)
    model = np.concatenate([lat, lat, lat])[rng.permutation(3 * len(lat))]
    src = lat[rng.integers(0, len(lat), 300)] + rng.integers(-1, 2, (300, 3)) * (a / 4)
    return Case("duplicates", "x3", model, _sym(src, rng), 2.0 ** -5, seed=seed, expect=dict(ties={3}))


CORNER = 0.05859375   # 15 * 2^-8: the dyadic corner that pins the box of the random dyadic models (4 cells per axis at d = 2^-5)


def _dyadic_cloud(rng, n, extent, bits=12):
    q = 2.0 ** -bits
    return rng.integers(-int(extent / q), int(extent / q) + 1, (n, 3)) * q


def cell_faces(n_half, seed=3):
    """sources exactly on cell faces, cell corners and octant mid-planes of the predicted grid (both neighbouring floats each), the
    other coordinates seeded; a dyadic random model, dense (octants tested) or sparse (whole cells)"""
    rng = np.random.default_rng(seed)
    dist = 2.0 ** -5
    q = _dyadic_cloud(rng, n_half - 1, 0.05)
    model = _sym(np.concatenate([q, [[CORNER, CORNER, CORNER]]]), rng)           # the box is pinned by its corners
    g = predict_grid(centre(model)[0], dist)
    src = []
    for k in range(3):
        for face in range(0, g["n3"][k] + 1):
            for half in (False, True):
                if half and face == g["n3"][k]:
                    continue
                for x in face_floats(g, k, face, half):
                    for _ in range(6):
                        p = rng.uniform(-0.06, 0.06, 3).astype(F)
                        p[k] = x
                        src.append(p)
    for cx in range(g["n3"][0] + 1):                                        # cell corners
        for cy in range(g["n3"][1] + 1):
            for cz in range(g["n3"][2] + 1):
                side = rng.integers(0, 2, 3)
                src.append([face_floats(g, k, f)[side[k]] for k, f in enumerate((cx, cy, cz))])
    src = np.array(src, F)
    return Case("cell_faces", "octants" if g["octants"] else "cells", model, _sym(src, pairs=True), dist, exact=False, seed=seed,
                expect=dict(octants=n_half * 2 >= OCTANT_DENSITY * g["cells"]))


def margin_u(g):
    """refine_args: the slack of the box distances in cell units"""
    return F(F(1e-3) + F(F(1e-6) * F(max(g["n3"]))))


def box_bound(g, s, lo, size, margin):
    """the walk's lower bound on the squared distance from source s to the box [lo, lo + size]^3 (cell units: a cell has size 1, an
    octant 0.5), in float as refine_accumulate_kernel forms it: h^2 sum(max(max(lo - u, u - hi) - margin, 0)^2)"""
    gs = []
    for k in range(3):
        u = cell_units(g, s[k], k)
        a, b = F(lo[k]), F(F(lo[k]) + F(size))
        gs.append(max(F(max(F(a - u), F(u - b)) - F(margin)), F(0.0)))
    return F(F(g["h"] * g["h"]) * F(F(F(gs[0] * gs[0]) + F(gs[1] * gs[1])) + F(gs[2] * gs[2])))


def prune_margin(n_cloud, seed=8):
    """the box prune at float equality, found by search over floats: a source s in a cell's interior, a model point p of its own cell
    (own octant) at distance r along one axis, and a model point q of LOWER index at the same distance r along another axis, where q
    is the first float beyond a cell face (or an octant mid-plane) -- the very edge of its box.  r is dyadic and s = q -+ r is exact,
    so d^2(p) = d^2(q) = r^2 bit for bit: q must win.  Kept are the instances where the box distance WITHOUT the margin rounds to
    more than r^2 in float: a walk without margin_u prunes q's box and answers p.  With the margin the bound lies below r^2 by
    about 2e-3 r h, a thousand times the rounding: the comparison is then never at equality for a box that holds a nearest point.
    Dense model (n_cloud large): octants are tested, both prunes are met; sparse: the cell prune alone."""
    rng = np.random.default_rng(seed)
    dist = 2.0 ** -5
    cloud = np.concatenate([_dyadic_cloud(rng, n_cloud, 0.05), [[CORNER, CORNER, CORNER]]])
    g = predict_grid(_sym(cloud).astype(F), dist)            # the box is pinned by the corners, whatever is added inside
    assert g["n3"] == [4, 4, 4]
    dense = 2 * n_cloud >= OCTANT_DENSITY * g["cells"]
    cell_of = lambda p: [int(np.floor(cell_units(g, p[k], k))) for k in range(3)]
    oct_of = lambda x: [int(cell_units(g, x[a], a) - F(cell_of(x)[a]) >= F(0.5)) for a in range(3)]
    S, P, Q, R, kinds = [], [], [], [], []
    for k in range(3):
        for half in ((False, True) if dense else (False,)):
            for face in range(1, 4) if not half else range(0, 4):
                below, above = face_floats(g, k, face, half)
                for side in ((1,) if half else (1, -1)):           # q above the plane, s below it -- or the reverse (cell faces only:
                    for r in (2.0 ** -6, 2.0 ** -7, 3 * 2.0 ** -9, 2.0 ** -8, 5 * 2.0 ** -10):   # an octant across a mid-plane is walked AFTER the source's only when above)
                        if half and r > 2.0 ** -7:
                            continue
                        j = (k + 1 + int(rng.integers(0, 2))) % 3
                        q = np.zeros(3, F)
                        q[k] = above if side > 0 else below
                        cq = face if side > 0 else face - 1          # q's cell along k
                        cs = (face - 1 if side > 0 else face) if not half else face
                        for a in range(3):
                            if a != k:                               # the other coordinates: a dyadic point well inside a cell's lower octant
                                c = int(rng.integers(0, 4))
                                q[a] = F(np.round((np.float64(g["o"][a]) + (c + 0.12) * np.float64(g["h"])) * 4096) / 4096)
                        s = q.copy(); s[k] = F(q[k] - F(side * r))
                        p = s.copy(); p[j] = F(s[j] + F(r))
                        if np.float64(s[k]) != np.float64(q[k]) - side * r:
                            continue                                 # s = q -+ r must be exact
                        if cell_of(s) != cell_of(p) or oct_of(s) != oct_of(p) or cell_of(s)[k] != cs or cell_of(q)[k] != cq:
                            continue
                        if half and (oct_of(q)[k], oct_of(s)[k]) != (1, 0):
                            continue
                        lo = [float(c) for c in cell_of(q)]
                        size = 1.0
                        if half:
                            lo = [c + 0.5 * o for c, o in zip(lo, oct_of(q))]; size = 0.5
                        r2 = F(r * r)
                        if not (box_bound(g, s, lo, size, 0.0) > r2 and box_bound(g, s, lo, size, margin_u(g)) < r2):
                            continue
                        # no instance (or its mirror image) comes near another's source
                        if any(np.linalg.norm(np.float64(x) - sg * np.float64(y)) < 1.5 * 2.0 ** -6 for sg in (1, -1) for x in (s, p, q) for y in S) or \
                           any(np.linalg.norm(np.float64(s) - sg * np.float64(y)) < 1.5 * 2.0 ** -6 for sg in (1, -1) for y in P + Q):
                            continue
                        S.append(s); P.append(p); Q.append(q); R.append(r); kinds.append(("mid-plane" if half else "face", k))
    S64 = np.array(S, np.float64)
    both = np.concatenate([S64, -S64])
    reach = 1.25 * np.array(R + R)
    keep = np.array([(np.linalg.norm(both - c, axis=1) > reach).all() for c in cloud[:-1]])                # p and q alone are within r of s
    model = _sym(np.concatenate([np.array(Q, np.float64), np.array(P, np.float64), cloud[:-1][keep], cloud[-1:]]), pairs=True)   # every q before every p
    case = Case("prune_margin", "octants" if dense else "cells", model, _sym(S64, pairs=True), dist, seed=seed,
                expect=dict(octants=dense, cells=64))
    case.instances = [dict(s=s, p=p, q=q, r=r, kind=kd) for s, p, q, r, kd in zip(S, P, Q, R, kinds)]
    return case


def box_and_threshold(seed=4):
    """a sparse lattice (step 4 d): sources exactly d from their only neighbour along an axis (counted), one float farther (found,
    not counted), one float nearer, at 2 d (none); at the lattice's outer faces the first ones lie exactly on the widened box and
    the second ones one float outside it (none)"""
    d = 2.0 ** -5
    lat = _lattice(1, 4 * d)
    rng = np.random.default_rng(seed)
    model = lat[rng.permutation(len(lat))]
    src = []
    for p in lat:
        for k in range(3):
            for sgn in (-1.0, 1.0):
                for kind in range(4):
                    s = p.astype(F).copy()
                    x = F(p[k] + sgn * d)
                    if kind == 1:
                        x = np.nextafter(x, F(sgn * np.inf))
                    elif kind == 2:
                        x = np.nextafter(x, F(-sgn * np.inf))
                    elif kind == 3:
                        x = F(p[k] + sgn * 2 * d)
                    s[k] = x
                    src.append(s)
    return Case("box_and_threshold", "lattice4d", model, _sym(np.array(src, F), pairs=True), d, seed=seed)


def grid_shapes(seed=5):
    rng = np.random.default_rng(seed)
    a = 2.0 ** -6
    out = []
    near = lambda pts, n, r: pts[rng.integers(0, len(pts), n)] + rng.integers(-4, 5, (n, 3)) * (r / 4)
    one = np.zeros((1, 3))
    out.append(Case("grid_shapes", "single_point", one, _sym(near(one, 40, 2.0 ** -5), rng), 2.0 ** -5, seed=seed, expect=dict(cells=1)))
    g = np.arange(-20, 21)[:, None] * a
    line = np.concatenate([g, 0 * g, 0 * g], 1)
    out.append(Case("grid_shapes", "collinear", line[rng.permutation(len(line))], _sym(near(line, 200, 2.0 ** -5), rng), 2.0 ** -5, seed=seed,
                    expect=dict(thin=(1, 2))))
    gg = np.stack(np.meshgrid(np.arange(-8, 9), np.arange(-8, 9), indexing="ij"), -1).reshape(-1, 2) * a
    plane = np.concatenate([gg, np.zeros((len(gg), 1))], 1)
    out.append(Case("grid_shapes", "planar", plane[rng.permutation(len(plane))], _sym(near(plane, 300, 2.0 ** -5), rng), 2.0 ** -5, seed=seed,
                    expect=dict(thin=(2,))))
    lat = _lattice(2, a)
    out.append(Case("grid_shapes", "one_cell", lat[rng.permutation(len(lat))], _sym(near(lat, 300, 2.0 ** -4), rng), 1.0, seed=seed, expect=dict(cells=1)))
    big = _lattice(4, 2.0 ** -5)                                            # extent 0.25 against d = 2^-9: 128^3 cells at h = 1.001 d
    out.append(Case("grid_shapes", "cell_cap", big[rng.permutation(len(big))], _sym(near(big, 400, 2.0 ** -9), rng), 2.0 ** -9, seed=seed,
                    expect=dict(raised=True)))
    return out


def budget_pairs(seed=6):
    """pairs of models that differ by late duplicates of two of their points only (so every match is the same) and sit either side of
    the LDS budget (nM 16 + (8 cells + 1) 4 against 48 KiB) and of nM = 32 cells; one shared source"""
    rng = np.random.default_rng(seed)
    dist = 2.0 ** -5
    q = np.concatenate([_dyadic_cloud(rng, 1471, 0.05), [[CORNER, CORNER, CORNER]]])
    src = _sym(_dyadic_cloud(rng, 500, 0.07), rng)
    out = []
    for fam, n_half in (("lds_budget", 1471), ("octant_switch", 1023)):
        base = _sym(np.concatenate([q[:n_half - 1], q[-1:]]), rng)
        more = np.concatenate([base, base[:1], -base[:1]])
        g = predict_grid(base.astype(F), dist)
        key = "lds" if fam == "lds_budget" else "octants"
        out.append(Case(fam, "below", base, src, dist, seed=seed, expect={key: fam == "lds_budget", "cells": g["cells"]}))
        out.append(Case(fam, "above", more, src, dist, seed=seed, expect={key: fam != "lds_budget", "cells": g["cells"]}))
    return out


N_SRC = (0, 1, 63, 64, 255, 256, 257, 65537)


def source_sizes(seed=7):
    """n_src over the chunk tails, src_idx unsorted and with repeats (0: a non-NULL, empty index array)"""
    base = lattice_ties(seed=seed)
    rng = np.random.default_rng(seed)
    out = []
    for n in N_SRC:
        c = Case("n_src", str(n), base.model, base.scene, base.dist, model_nrm=base.model_nrm, src_idx=rng.integers(0, len(base.scene), n), seed=seed)
        out.append(c)
    return out


def random_clouds():
    """uniform, clustered and surface-like clouds at several densities and distances; centroids are whatever they are, the hypothesis
    [I | cm - cs] puts the scene back on the model"""
    out = []
    for kind, n_m, n_s, dist, seed in (("uniform", 800, 3000, 0.02, 11), ("uniform", 6000, 3000, 0.035, 12), ("clustered", 3000, 3000, 0.01, 13),
                                       ("clustered", 5000, 2000, 0.035, 14), ("surface", 2500, 4000, 0.035, 15), ("surface", 5000, 3000, 0.005, 16)):
        rng = np.random.default_rng(seed)
        if kind == "uniform":
            m = rng.uniform(-0.1, 0.1, (n_m, 3)) + [0.3, -0.2, 0.9]
        elif kind == "clustered":
            cen = rng.uniform(-0.1, 0.1, (12, 3))
            m = cen[rng.integers(0, 12, n_m)] + rng.normal(0, 0.004, (n_m, 3)) + [0.1, 0.0, 0.5]
        else:
            v = rng.normal(size=(n_m, 3)); v /= np.linalg.norm(v, axis=1)[:, None]
            m = v * [0.09, 0.06, 0.04] + [0.0, 0.1, 0.7]
        m = m.astype(F)
        nrm = None
        if kind == "surface":
            v = (m.astype(np.float64) - [0.0, 0.1, 0.7]) / np.array([0.09, 0.06, 0.04]) ** 2
            nrm = v / np.linalg.norm(v, axis=1)[:, None]
        s = np.concatenate([m[rng.integers(0, n_m, n_s - n_s // 5)] + rng.normal(0, dist / 2, (n_s - n_s // 5, 3)),
                            rng.uniform(m.min(0) - 2 * dist, m.max(0) + 2 * dist, (n_s // 5, 3))]).astype(F)
        _, cm = centre(m)
        _, cs = centre(s)
        T = identity_hyp((cm.astype(np.float64) - cs.astype(np.float64)).astype(F))
        out.append(Case("random_" + kind, "%d_%g" % (n_m, dist), m, s, dist, model_nrm=nrm, T16=T, exact=False, seed=seed))
    return out


def constructed_cases():
    return ([lattice_ties(), duplicates(), cell_faces(1300), cell_faces(300), prune_margin(1700), prune_margin(300), box_and_threshold()] + grid_shapes() + budget_pairs() + [lattice_ties(unit=1000.0)]
            + source_sizes())


def all_cases():
    return constructed_cases() + random_clouds()


def expected_detail(src, model_c, dist, grid, cl=None):
    """the reference's own (match, counted): lowest index at the minimum, found when inside the box and within the search bound,
    counted on d1 <= D2 -- what the kernel must give wherever nothing is ambiguous"""
    cl = cl or classify(src, model_c)
    D2 = float(F(dist)) ** 2
    F2 = float(F(D2 * (1.0 + 1e-5)))
    found = in_box(grid, np.asarray(src, F)) & (cl["d1"] <= F2)
    match = np.where(found, cl["low"], -1).astype(np.int32)
    return match, (found & (cl["d1"] <= D2)).astype(np.uint8)


POSE_FAMILIES = ("lattice_ties", "random_uniform", "random_clustered", "random_surface")
