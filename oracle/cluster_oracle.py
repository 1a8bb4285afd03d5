"""Plain float64 reference of the pose clustering (csrc/cluster.hip: stocs_cluster_poses on the host, trial_cluster_kernel on the
device) and the cases that pin it at its edges.  Not a port of csrc/pose_diff.h: written from the definition.

The definition.  A pose is a column-major 4x4, rotation R and translation t.  For a pair (test, base):
  translation error  |t_base - t_test|, Euclidean;
  rotation error     D = R_test^-1 . R_base (numpy.linalg); its ZYX Euler angles read off the matrix -- roll = atan2(D21, D22),
                     pitch = asin(-D20), yaw = atan2(D10, D00) -- in degrees, absolute value; per axis d the fold of sym[d]:
                     90: e = |e - 90|, e = min(e, 90 - e);  180: e = min(e, 180 - e);  360: e = 0;  anything else: none;
                     the maximum over the three axes.
The greedy run of one trial: the survivors are the candidates with lcp > float32(fraction * best) -- the FLOAT product, that is the
contract; a NaN score never survives.  They are taken by descending score, the lowest index first among equal scores.  A survivor
is dropped when some kept one is within BOTH thresholds of it (rotation error of (test = survivor, base = kept) < min_angle and
translation error < min_distance, both strict).  The run stops once more than `count` are kept.

Outside the definition.  A pose with a NaN entry or a singular rotation has no inverse or no angles: its rotation error with
anything is NaN, and NaN is never `<`, so such a pose neither drops nor is dropped (class exact: the float routine gives NaN too,
0 * inf and NaN propagate).  A D that is not orthonormal (a scaled pose against a plain one, a zero matrix as base) has no Euler
angles: the rotation test of that pair is undefined here, and the pair is decided only if the translation test alone decides it.

How a pair decision is classed.  The library decides in float32 (pose_diff.h); this reference in float64.  Per pair:
  exact      float and double agree by construction: the translation differences are float32 numbers and the square root of their
             sum of squares is exact and a float32 number (Pythagorean lattices; checked in integers); a rotation error that is 0
             on both sides (every axis sym 360); NaN errors; both rotations signed permutation matrices (hinverse and hmul are
             exact on 0 / +-1, so D is exact and its angles are multiples of 90 degrees; see PERM_TOL below);
  clear      the float64 value is further from the threshold than the bound below on what float32 evaluation can move it (or the
             other test decides the pair alone: both must hold to drop);
  ambiguous  neither.  A case with an ambiguous pair is compared with the float twins only.

The bound (u = 2^-24, first order, constants rounded up; orthonormal input, |entries| <= 1; a common scale factor of a pose
cancels in every relative error, so k.R against k.R is covered).
  hinverse   a cofactor ab - cd: two products and a difference, |err| <= 2u (|ab| + |cd| <= 1).  det = sum of three a.c: 2u.sqrt(3)
             from the cofactors + 3u from its own operations < 6.5u; 1 / det: 7.5u; entry c / det: 2u + 7.5u + u = 10.5u.
  hmul       D_ij = sum_k A_ik B_kj: 10.5u . sum_k |B_kj| <= 10.5u.sqrt(3) from A, 3u from the three operations: eps_D = 22u.  The
             float64 D itself is orthonormal only as far as the float32 input is; eta = max |D^T D - I| is measured per pair and
             added (the quaternion route and the matrix route read different entries of D): eps_D = 22u + eta.
  quaternion Both branches of mat_to_quat divide by s = sqrt(1 + d_i - d_j - d_k) (or sqrt(1 + trace)) with s^2 = 4 q_max^2 >= 1.
             err(s^2) <= 3 eps_D + 12u, err(s) <= 1.5 eps_D + 8u; the large component 0.5 s: 0.75 eps_D + 5u; the others
             (D_ab +- D_ba) . 0.5 / s: numerator 2 eps_D + 2u times 0.5, plus |numerator| <= 2 times err(0.5 / s) <= 0.75 eps_D + 5u,
             plus u: eps_q = 2.5 eps_D + 12u.
  sines      sinr = 2 (wx + yz) and the like: each product moves by eps_q (|a| + |b|), the sum of |q_i| is <= 2, three roundings:
             4 eps_q + 6u; the cosines 1 - 2 (x^2 + y^2): 4 sqrt(2) eps_q + 6u.  eps_e = 6 eps_q + 6u covers all five.
  atan2      a point at distance h = hypot(sin, cos) from the origin moved by at most sqrt(2) eps_e turns by at most
             asin(sqrt(2) eps_e / h) <= 1.01 sqrt(2) eps_e / h while that ratio is below 0.1, unbounded otherwise.  For a rotation
             h = cos(pitch) for roll and yaw alike: the bound grows towards gimbal lock.
  asin       mean value theorem: eps_e / sqrt(1 - (|sinp| + eps_e)^2), unbounded when |sinp| + eps_e >= 1 (there the float routine
             may also take its |sinp| >= 1 branch).
  degrees    the angle is rounded to float, scaled and rounded again, folded by at most two float subtractions of values <= 180:
             8u . 180 degrees in all (libm's atan2 / asin in double add nothing at this scale).  Folds, |.| and the maximum are
             1-Lipschitz: the bound of the result is the largest of the three axes' bounds (0 on an axis with sym 360).
  translation the three float differences are rounded (u each, relative), the rest is double, the result rounded to float:
             3u . distance.
PERM_TOL.  Signed permutation matrices: D is exact, every quaternion component is one exact value through a square root, a
division and a product (<= 4u), so every sine and cosine is within 16u of 0 or +-1.  Away from gimbal lock the general bound
applies with eps_D = 0.  At |D20| = 1 the float sinp may fall short of 1 by 16u, asin by sqrt(2 . 16u) rad = 0.079 degrees, while
roll and yaw are atan2 of two roundings and may be anything: the pair's error is only known to be >= 90 - 0.08 degrees whatever
they are (and only if axis 1 has no fold).  Such a pair is exact when min_angle <= 89.9, undefined otherwise.
The CPU test (tests/test_cluster_cases_cpu.py) holds the bound against the host twin on every pair the cases meet; the largest
ratio |twin - float64| / bound it finds is recorded in profiles/cluster_edges.md (rotation 0.020, translation 0.332 over 98799 distinct pairs).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

U = 2.0 ** -24
CLEAR, EXACT, AMBIGUOUS = 0, 1, 2
CLASS_NAMES = ("clear", "exact", "ambiguous")
LDS_SURVIVORS = 2048          # csrc/cluster.hip CLUSTER_LDS: at most this many survivors and the later rounds walk the LDS list
PERM_TOL_DEG = 0.08
DEG = 180.0 / math.pi


@dataclass
class Case:
    name: str
    family: str
    poses: np.ndarray            # (N, 16) float32, camera frame, column-major
    lcp: np.ndarray              # (N,) float32
    off: np.ndarray              # (n_trials + 1,) int32
    best: np.ndarray             # (n_trials,) float32
    fraction: float = 0.0
    count: int = 100
    min_distance: float = 0.02
    min_angle: float = 15.0
    sym: tuple = (0.0, 0.0, 0.0)
    built_ambiguous: bool = False     # the case is meant to be ambiguous (the two near-gimbal cases)
    note: dict = field(default_factory=dict)

    @property
    def n_trials(self):
        return len(self.off) - 1

    def trial(self, t):
        a, b = int(self.off[t]), int(self.off[t + 1])
        return self.poses[a:b], self.lcp[a:b]


# ---------------------------------------------------------------- the reference

class _Prep:
    """float64 views of one trial's poses"""

    def __init__(self, P):
        P = np.asarray(P, np.float32).reshape(-1, 16)
        M = P.astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)      # M[n, r, c] = p[c * 4 + r]
        self.P32 = P
        self.R = np.ascontiguousarray(M[:, :3, :3])
        self.t = np.ascontiguousarray(M[:, :3, 3])
        n = len(P)
        fin = np.isfinite(self.R).reshape(n, -1).all(1) if n else np.zeros(0, bool)
        det = np.zeros(n)
        if fin.any():
            det[fin] = np.linalg.det(self.R[fin])
        ok = fin & (det != 0)
        self.Rinv = np.full((n, 3, 3), np.nan)
        if ok.any():
            self.Rinv[ok] = np.linalg.inv(self.R[ok])
        self.perm = np.zeros(n, bool)
        for i in np.flatnonzero(ok):
            R = self.R[i]
            self.perm[i] = bool(np.isin(R, (-1.0, 0.0, 1.0)).all() and np.array_equal(R.T @ R, np.eye(3)))


def _exact_distance(dt):
    """dt: float64 differences of float32 translations (exact).  True when each is a float32 number and sqrt(sum of squares) is exact and a
    float32 number -- in integers."""
    if not np.isfinite(dt).all() or not np.array_equal(dt.astype(np.float32).astype(np.float64), dt):
        return False
    k = [int(round(math.ldexp(float(v), 80))) for v in dt]
    if any(math.ldexp(float(x), -80) != float(v) for x, v in zip(k, dt)):
        return False
    ss = sum(x * x for x in k)
    r = math.isqrt(ss)
    if r * r != ss:
        return False
    d = math.ldexp(float(r), -80)
    return int(round(math.ldexp(d, 80))) == r and float(np.float32(d)) == d


def pair_eval(prep, tests, base, min_distance, min_angle, sym):
    """The pairs (test = each of `tests`, base) of one trial.  -> dict of arrays over the tests: te, re (float64 errors; re NaN where
    it is NaN by rule or undefined), bt, br (bounds), lower_only (the float rotation error is only known to be >= re - br), drop (the
    float64 decision), cls."""
    tests = np.asarray(tests, np.int64)
    m = len(tests)
    min_d, min_a = float(np.float32(min_distance)), float(np.float32(min_angle))
    dt = prep.t[base][None, :] - prep.t[tests]
    with np.errstate(invalid="ignore", over="ignore"):
        te = np.sqrt((dt * dt).sum(1))
    bt = 3 * U * np.where(np.isfinite(te), te, 0.0)
    # translation: +1 clearly not near, -1 clearly near, 0 undecided
    t_dec = np.where(~np.isfinite(te) | (te - bt >= min_d), 1, np.where(te + bt < min_d, -1, 0))
    t_exact = ~np.isfinite(te)
    for k in np.flatnonzero(t_dec == 0):
        if _exact_distance(dt[k]):
            t_exact[k] = True
            t_dec[k] = -1 if te[k] < min_d else 1
    # rotation
    with np.errstate(invalid="ignore", over="ignore"):
        D = prep.Rinv[tests] @ prep.R[base][None]
        nan_rule = ~np.isfinite(D).reshape(m, -1).all(1)
        Ds = np.where(nan_rule[:, None, None], np.eye(3)[None], D)
        eta = np.abs(Ds.transpose(0, 2, 1) @ Ds - np.eye(3)[None]).reshape(m, -1).max(1)
        undefined = ~nan_rule & (eta > 1e-3)
        Ds = np.where(undefined[:, None, None], np.eye(3)[None], Ds)
        eta = np.where(undefined, 0.0, eta)
        sinp = np.clip(-Ds[:, 2, 0], -1.0, 1.0)
        ang = np.stack([np.arctan2(Ds[:, 2, 1], Ds[:, 2, 2]), np.arcsin(sinp), np.arctan2(Ds[:, 1, 0], Ds[:, 0, 0])], 1) * DEG
        both_perm = prep.perm[tests] & prep.perm[base]
        eps_d = np.where(both_perm, 0.0, 22 * U + eta)
        eps_q = np.where(both_perm, 4 * U, 2.5 * eps_d + 12 * U)
        eps_e = np.where(both_perm, 16 * U, 6 * eps_q + 6 * U)
        h = np.stack([np.hypot(Ds[:, 2, 1], Ds[:, 2, 2]), np.zeros(m), np.hypot(Ds[:, 1, 0], Ds[:, 0, 0])], 1)
        ratio = math.sqrt(2.0) * eps_e[:, None] / np.maximum(h, 1e-300)
        b_atan = np.where(ratio < 0.1, 1.01 * ratio, np.inf)
        room = 1.0 - (np.abs(sinp) + eps_e) ** 2
        b_asin = np.where(room > 0, eps_e / np.sqrt(np.maximum(room, 1e-300)), np.inf)
        b_ax = np.stack([b_atan[:, 0], b_asin, b_atan[:, 2]], 1) * DEG + 8 * U * 180.0
    e = np.abs(ang)
    for d in range(3):
        s = float(np.float32(sym[d]))
        if s == 90:
            e[:, d] = np.abs(e[:, d] - 90); e[:, d] = np.minimum(e[:, d], 90 - e[:, d])
        elif s == 180:
            e[:, d] = np.minimum(e[:, d], 180 - e[:, d])
        elif s == 360:
            e[:, d] = 0.0; b_ax[:, d] = 0.0
    re = e.max(1)
    br = b_ax.max(1)
    lower_only = np.zeros(m, bool)
    gimbal_perm = both_perm & ~nan_rule & ~undefined & (np.abs(Ds[:, 2, 0]) == 1.0)
    if gimbal_perm.any():
        fold1 = float(np.float32(sym[1])) in (90.0, 180.0, 360.0)
        for k in np.flatnonzero(gimbal_perm):
            if fold1:
                undefined[k] = True
            else:
                re[k] = max(re[k], 90.0); br[k] = PERM_TOL_DEG; lower_only[k] = True
    re = np.where(nan_rule | undefined, np.nan, re)
    br = np.where(nan_rule | undefined, 0.0, br)
    all360 = all(float(np.float32(s)) == 360 for s in sym)
    with np.errstate(invalid="ignore"):
        r_dec = np.where(nan_rule, 1, np.where(undefined, 0, np.where(re - br >= min_a, 1, np.where(~lower_only & (re + br < min_a), -1, 0))))
    r_exact = nan_rule | (both_perm & ~undefined) | (all360 & ~undefined & ~nan_rule)
    with np.errstate(invalid="ignore"):
        drop = (te < min_d) & (re < min_a)
    # both tests must hold to drop: a test that clearly fails decides the pair alone
    cls = np.where(t_dec == 1, np.where(t_exact, EXACT, CLEAR),
                   np.where(r_dec == 1, np.where(r_exact, EXACT, CLEAR),
                            np.where((t_dec == -1) & (r_dec == -1), np.where(t_exact | r_exact, EXACT, CLEAR), AMBIGUOUS)))
    return dict(te=te, re=re, bt=bt, br=br, lower_only=lower_only, drop=drop, cls=cls, undefined=undefined, nan_rule=nan_rule)


def cluster_trial(poses, lcp, fraction, best, count, min_distance, min_angle, sym, pairs=None):
    """The float64 greedy run of one trial -> (kept indices int32, survivors of round 0, class counts [clear, exact, ambiguous]).
    pairs: a list that receives (test, base, te, re, bt, br, lower_only) of every pair met."""
    prep = _Prep(poses)
    lcp = np.asarray(lcp, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        thr = np.float32(fraction) * np.float32(best)
        alive = lcp > thr
    n0 = int(alive.sum())
    kept, classes = [], [0, 0, 0]
    while alive.any():
        idx = np.flatnonzero(alive)
        j = int(idx[np.argmax(lcp[idx])])          # the first maximum: highest score, lowest index
        kept.append(j)
        alive[j] = False
        if len(kept) > count:                      # sic: size > count
            break
        tests = np.flatnonzero(alive)
        if not len(tests):
            break
        ev = pair_eval(prep, tests, j, min_distance, min_angle, sym)
        alive[tests[ev["drop"]]] = False
        for c in range(3):
            classes[c] += int((ev["cls"] == c).sum())
        if pairs is not None:
            for k in range(len(tests)):
                pairs.append((int(tests[k]), j, float(ev["te"][k]), float(ev["re"][k]), float(ev["bt"][k]), float(ev["br"][k]), bool(ev["lower_only"][k])))
    return np.asarray(kept, np.int32), n0, classes


def cluster_case(case, pairs=None):
    """Every trial of a case -> (list of kept arrays, survivors per trial, class counts over the case).  pairs: receives (trial, test, base, ...)."""
    kept, surv, classes = [], [], [0, 0, 0]
    for t in range(case.n_trials):
        P, l = case.trial(t)
        pp = [] if pairs is not None else None
        k, n0, c = cluster_trial(P, l, case.fraction, case.best[t], case.count, case.min_distance, case.min_angle, case.sym, pp)
        kept.append(k); surv.append(n0)
        for i in range(3):
            classes[i] += c[i]
        if pairs is not None:
            pairs.extend((t,) + p for p in pp)
    return kept, surv, classes


def diff_trace32(test16, base16):
    """trace and diagonal of D as the float routine forms it (cofactor inverse, products in its order, all float32): which branch of the
    quaternion conversion a pair takes.  -> (trace, i) with i the branch index of `t <= 0`, or -1 for `t > 0`."""
    f = np.float32
    a = np.asarray(test16, f).reshape(4, 4).T[:3, :3]
    b = np.asarray(base16, f).reshape(4, 4).T[:3, :3]
    c00 = a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]; c01 = a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2]; c02 = a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]
    inv = f(1.0) / (a[0, 0] * c00 + (a[0, 1] * c01 + a[0, 2] * c02))
    r = np.zeros((3, 3), f)
    r[0, 0] = c00 * inv; r[1, 0] = c01 * inv; r[2, 0] = c02 * inv
    r[0, 1] = (a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2]) * inv; r[1, 1] = (a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0]) * inv; r[2, 1] = (a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1]) * inv
    r[0, 2] = (a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]) * inv; r[1, 2] = (a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]) * inv; r[2, 2] = (a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]) * inv
    d = [r[i, 0] * b[0, i] + (r[i, 1] * b[1, i] + r[i, 2] * b[2, i]) for i in range(3)]
    t = d[0] + d[1] + d[2]
    if t > 0:
        return float(t), -1
    i = 0
    if d[1] > d[0]:
        i = 1
    if d[2] > d[i]:
        i = 2
    return float(t), i


# ---------------------------------------------------------------- building blocks of the cases

def rot(axis, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)
    if axis == 1:
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def rand_rot(rs):
    q = rs.normal(size=4); q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def pose(R, t):
    p = np.zeros(16, np.float64)
    for c in range(3):
        p[c * 4:c * 4 + 3] = np.asarray(R)[:, c]
    p[12:15] = t; p[15] = 1.0
    return p.astype(np.float32)


def best_of(lcp):
    """a trial's best score as the batch's arg-max leaves it: the largest positive score, 0 when there is none"""
    l = np.asarray(lcp, np.float32)
    l = l[l > 0]
    return np.float32(l.max()) if len(l) else np.float32(0)


def single(name, family, P, lcp, **kw):
    P = np.asarray(P, np.float32).reshape(-1, 16); lcp = np.asarray(lcp, np.float32).reshape(-1)
    best = kw.pop("best", None)
    best = np.asarray([best_of(lcp) if best is None else best], np.float32)
    return Case(name, family, P, lcp, np.asarray([0, len(lcp)], np.int32), best, **kw)


def batch(name, family, trials, **kw):
    """trials: list of (P, lcp)"""
    P = np.concatenate([np.asarray(p, np.float32).reshape(-1, 16) for p, _ in trials] + [np.zeros((0, 16), np.float32)])
    l = np.concatenate([np.asarray(s, np.float32).reshape(-1) for _, s in trials] + [np.zeros(0, np.float32)])
    off = np.concatenate([[0], np.cumsum([len(np.asarray(s).reshape(-1)) for _, s in trials])]).astype(np.int32)
    best = np.asarray([best_of(s) for _, s in trials], np.float32)
    return Case(name, family, P, l, off, best, **kw)


def grouped(rs, n, groups=12):
    """n poses drawn from `groups` far-apart places with four variants each: the place's pose; the same turned by 40 degrees (near in
    translation only); the same moved by 0.05 (near in rotation only); the same turned by 5 degrees and moved by 0.005 (near in both: it
    merges with the first, whichever scores higher).  At most 3 * groups clusters, and few distinct poses however large n is."""
    pool = []
    for g in range(groups):
        R = rand_rot(rs)
        c = np.array([g % 4, (g // 4) % 4, g // 16], np.float64) * 0.5 + 1.0
        pool += [pose(R, c), pose(R @ rot(0, 40.0), c), pose(R, c + [0.05, 0, 0]), pose(R @ rot(2, 5.0), c + [0.005, 0, 0])]
    pool = np.asarray(pool, np.float32)
    return pool[rs.randint(0, len(pool), size=n)] if n else np.zeros((0, 16), np.float32)


def grid_scores(rs, n, lo=1, hi=97):
    return (rs.randint(lo, hi + 1, size=n).astype(np.float32) / np.float32(97)).astype(np.float32)


# ---------------------------------------------------------------- the families

def fam_sizes():
    out = []
    for n in (0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 1280):
        rs = np.random.RandomState(1000 + n)
        out.append(single("sizes_n%d" % n, "sizes", grouped(rs, n), grid_scores(rs, n), fraction=0.0, count=40))
    return out


def fam_lds():
    out = []
    for S in (LDS_SURVIVORS - 1, LDS_SURVIVORS, LDS_SURVIVORS + 1):
        rs = np.random.RandomState(2000 + S)
        out.append(single("lds_%d_of_%d" % (S, S), "lds", grouped(rs, S), grid_scores(rs, S), fraction=0.0, count=40, note={"survivors": S}))
        n = 4608
        l = grid_scores(rs, n, 0, 48)                       # <= 48/97 < 0.5: out
        l[rs.randint(0, n, 200)] = np.float32(0.5)          # exactly the threshold: out
        pos = np.sort(rs.choice(n, S, replace=False))
        l[pos] = grid_scores(rs, S, 49, 97)                 # >= 49/97 > 0.5: in
        l[pos[S // 2]] = np.float32(1.0)
        out.append(single("lds_%d_of_%d" % (S, n), "lds", grouped(rs, n), l, fraction=0.5, count=40, note={"survivors": S}))
    rs = np.random.RandomState(2999)
    n, S = 4608, LDS_SURVIVORS + 1
    l = grid_scores(rs, n, 0, 48)
    pos = np.sort(np.concatenate([rs.choice(n - 64, S - 64, replace=False), np.arange(n - 64, n)]))
    l[pos] = grid_scores(rs, S, 49, 90)
    l[n - 64:] = grid_scores(rs, 64, 96, 97)                # the last survivors a first pass appends are the best ones
    l[n - 1] = np.float32(1.0)
    out.append(single("lds_%d_of_%d_top_last" % (S, n), "lds", grouped(rs, n), l, fraction=0.5, count=40, note={"survivors": S}))
    return out


def fam_ties():
    rs = np.random.RandomState(3000)
    n = 300
    out = [single("ties_all_equal", "ties", grouped(rs, n), np.full(n, 0.5, np.float32), fraction=0.0, count=40)]
    out.append(single("ties_blocks", "ties", grouped(rs, n), ((np.arange(n) // 16 % 7 + 1) / 97.0).astype(np.float32), fraction=0.0, count=40))
    l = np.full(n, 1.0, np.float32)
    l[::3] = np.float32(0.3)                                 # index 0 and every third: out, next to the equal best ones
    out.append(single("ties_next_to_non_survivors", "ties", grouped(rs, n), l, fraction=0.5, count=40))
    return out


def _far_line(k, R=None):
    R = np.eye(3) if R is None else R
    return [pose(R, [1.0 + 0.5 * i, 2.0, 3.0]) for i in range(k)]


def fam_thresholds():
    out = []
    R = rand_rot(np.random.RandomState(4000))
    for nm, v in (("345", np.array([3, 4, 0]) / 256.0), ("236", np.array([2, 3, 6]) / 512.0)):
        d = float(np.linalg.norm(v))
        P = [pose(R, [0.5, 0.25, 1.0]), pose(R, np.array([0.5, 0.25, 1.0]) + v)]
        out.append(single("thr_distance_equal_" + nm, "thresholds", P, [0.9, 0.8], min_distance=d, note={"kept": 2}))
        out.append(single("thr_distance_below_" + nm, "thresholds", P, [0.9, 0.8], min_distance=float(np.nextafter(np.float32(d), np.float32(1))), note={"kept": 1}))
    fr, be = np.float32(0.8), np.float32(0.75)
    thr = fr * be
    l = np.asarray([be, thr, np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(0))], np.float32)
    out.append(single("thr_lcp_equal_and_above", "thresholds", _far_line(4), l, fraction=float(fr), note={"kept": 2}))
    out.append(single("thr_best_zero", "thresholds", _far_line(4), np.zeros(4, np.float32), fraction=0.8, note={"kept": 0}))
    out.append(single("thr_fraction_0", "thresholds", _far_line(4), [0.0, 0.5, 0.0, 0.25], fraction=0.0, note={"kept": 2}))
    out.append(single("thr_fraction_1", "thresholds", _far_line(4), [0.1, 0.5, 0.5, 0.25], fraction=1.0, note={"kept": 0}))
    out.append(single("thr_fraction_negative_zero_scores", "thresholds", _far_line(4), np.zeros(4, np.float32), fraction=-1.0, note={"kept": 0}))
    out.append(single("thr_fraction_negative", "thresholds", _far_line(4), [0.0, 0.5, 0.0, 0.25], fraction=-1.0, note={"kept": 4}))
    out.append(single("thr_fraction_inf", "thresholds", _far_line(4), [0.1, 0.5, 0.5, 0.25], fraction=float("inf"), note={"kept": 0}))
    out.append(single("thr_fraction_inf_best_zero", "thresholds", _far_line(4), np.zeros(4, np.float32), fraction=float("inf"), note={"kept": 0}))
    return out


def fam_both():
    R = rand_rot(np.random.RandomState(5000))
    t = np.array([0.3, 0.2, 0.9])
    return [single("both_near_t_far_r", "both", [pose(R, t), pose(R @ rot(1, 30.0), t + [0.004, 0, 0])], [0.9, 0.8], note={"kept": 2}),
            single("both_far_t_near_r", "both", [pose(R, t), pose(R @ rot(1, 3.0), t + [0.04, 0, 0])], [0.9, 0.8], note={"kept": 2}),
            single("both_near", "both", [pose(R, t), pose(R @ rot(1, 3.0), t + [0.004, 0, 0])], [0.9, 0.8], note={"kept": 1})]


def fam_chains():
    R = rand_rot(np.random.RandomState(6000))
    t = np.array([0.3, 0.2, 0.9])
    T = [pose(R, t), pose(R, t + [0.015, 0, 0]), pose(R, t + [0.03, 0, 0])]
    A = [pose(R, t), pose(R @ rot(2, 10.0), t), pose(R @ rot(2, 20.0), t)]
    out = []
    for nm, P in (("translation", T), ("rotation", A)):
        out.append(single("chain_%s_abc" % nm, "chains", P, [0.9, 0.8, 0.7], note={"kept_list": [0, 2]}))
        out.append(single("chain_%s_bac" % nm, "chains", P, [0.8, 0.9, 0.7], note={"kept_list": [1]}))
        out.append(single("chain_%s_cba" % nm, "chains", P, [0.7, 0.8, 0.9], note={"kept_list": [2, 0]}))
    return out


def _euler_err(D):
    return float(np.abs([math.atan2(D[2, 1], D[2, 2]), math.asin(max(-1.0, min(1.0, -D[2, 0]))), math.atan2(D[1, 0], D[0, 0])]).max() * DEG)


def fam_argument_order():
    """relative rotations D whose error is clearly below min_angle while that of D^T is clearly above: found by a seeded search"""
    rs = np.random.RandomState(7000)
    found = []
    for _ in range(200000):
        D = rot(2, rs.uniform(-20, 20)) @ rot(1, rs.uniform(-60, 60)) @ rot(0, rs.uniform(-20, 20))
        if _euler_err(D) < 14.0 and _euler_err(D.T) > 16.0:      # a degree from min_angle = 15 on either side
            found.append(D)
            if len(found) == 3:
                break
    assert len(found) == 3
    out = []
    t = np.array([0.3, 0.2, 0.9])
    for k, D in enumerate(found):
        Ra = rand_rot(rs)
        Rb = Ra @ D                                          # (test = a, base = b): Ra^-1 Rb = D, below;  (test = b, base = a): D^T, above
        out.append(single("order_%d_b_kept_a_dropped" % k, "order", [pose(Ra, t), pose(Rb, t)], [0.8, 0.9], note={"kept_list": [1]}))
        out.append(single("order_%d_a_kept_b_stays" % k, "order", [pose(Ra, t), pose(Rb, t)], [0.9, 0.8], note={"kept_list": [0, 1]}))
    return out


def fam_quaternion():
    out = []
    R0 = rand_rot(np.random.RandomState(8000))
    t = np.array([0.3, 0.2, 0.9])
    for ax in range(3):
        for dl in (-0.5, 0.5):
            P = [pose(R0, t), pose(R0 @ rot(ax, 180.0 + dl), t)]
            sym = [0.0, 0.0, 0.0]
            out.append(single("quat_axis%d_%+.1f" % (ax, dl), "quaternion", P, [0.9, 0.8], note={"kept": 2, "branch": ax}))
            sym[ax] = 180.0
            if ax != 1:     # (about y the half turn shows as roll = yaw = 180: folding axis 1 alone changes nothing)
                out.append(single("quat_axis%d_%+.1f_sym180" % (ax, dl), "quaternion", P, [0.9, 0.8], sym=tuple(sym), note={"kept": 1, "branch": ax}))
    cyc = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64)      # 120 degrees about (1, 1, 1): trace exactly 0
    out.append(single("quat_trace_zero", "quaternion", [pose(np.eye(3), t), pose(cyc, t)], [0.9, 0.8], note={"kept": 2, "branch": 0, "trace": 0.0}))
    return out


def fam_gimbal():
    out = []
    t = np.array([0.3, 0.2, 0.9])
    for sg in (1, -1):
        Ry = np.array([[0, 0, sg], [0, 1, 0], [-sg, 0, 0]], np.float64)
        out.append(single("gimbal_exact_%+d" % sg, "gimbal", [pose(np.eye(3), t), pose(Ry, t)], [0.9, 0.8], note={"kept": 2}))
    R0 = rand_rot(np.random.RandomState(9000))
    for dl in (-1e-3, 1e-3):
        out.append(single("gimbal_near_%+.0e" % dl, "gimbal", [pose(R0, t), pose(R0 @ rot(1, 90.0 + dl), t)], [0.9, 0.8], built_ambiguous=True))
    return out


SYM_ANGLES = (10.0, 20.0, 50.0, 80.0, 130.0, 160.0)     # every difference is a multiple of 10 and none is 90: 5 degrees from every fold's threshold


def fam_sym():
    out = []
    t = np.array([0.3, 0.2, 0.9])
    for sym in ((90.0, 0.0, 0.0), (0.0, 180.0, 0.0), (0.0, 0.0, 360.0), (90.0, 180.0, 360.0), (45.0, 0.0, 0.0)):
        for ax in range(3):
            P = [pose(np.eye(3), t)] + [pose(rot(ax, a), t) for a in SYM_ANGLES]
            l = [0.9] + [0.8 - 0.01 * k for k in range(len(SYM_ANGLES))]
            out.append(single("sym_%g_%g_%g_axis%d" % (sym + (ax,)), "sym", P, l, sym=sym))
    return out


def fam_count():
    rs = np.random.RandomState(10000)
    n = 30
    P, l = grouped(rs, n, groups=3), grid_scores(rs, n)
    return [single("count_%d" % c, "count", P, l, count=c) for c in (0, 1, n - 1, n, n + 1, 100000)]


def fam_degenerate():
    out = []
    R0 = rand_rot(np.random.RandomState(11000))
    far = np.array([5.0, 5.0, 5.0])
    bad = {"nan": np.full(16, np.nan, np.float32), "zero": np.zeros(16, np.float32), "scaled": pose(2.0 * R0, far)}
    good = _far_line(6, R0) + [pose(R0 @ rot(2, 4.0), [1.0, 2.0, 3.003])]     # the last one merges with the first
    base_scores = [0.9, 0.85, 0.8, 0.75, 0.7, 0.65, 0.6]
    for kind, b in bad.items():
        for where, sc in (("top", [0.95]), ("second", [0.87]), ("pair", [0.87, 0.86])):
            P = list(good) + [b] * len(sc)
            out.append(single("degenerate_%s_%s" % (kind, where), "degenerate", P, base_scores + sc))
            P = [b] * len(sc) + list(good)                    # the same at the lowest indices
            out.append(single("degenerate_%s_%s_first" % (kind, where), "degenerate", P, sc + base_scores))
    l = np.asarray(base_scores, np.float32); l[[1, 4]] = np.nan
    out.append(single("degenerate_nan_scores", "degenerate", good, l, fraction=0.5))
    return out


def fam_batch():
    sizes = (0, 1, 300, 0, 2600, LDS_SURVIVORS, 5)
    trials = []
    for k, n in enumerate(sizes):
        rs = np.random.RandomState(12000 + k)
        trials.append((grouped(rs, n), grid_scores(rs, n)))
    return [batch("batch_forward", "batch", trials, fraction=0.0, count=40), batch("batch_reverse", "batch", trials[::-1], fraction=0.0, count=40)]


def fam_random():
    out = []
    side = 0.02 * (4 * math.pi) ** (1.0 / 3.0)       # a ball of radius min_distance holds a third of the box
    for k in range(64):
        rs = np.random.RandomState(13000 + k)
        n = int(rs.randint(1, 601))
        P = [pose(rand_rot(rs), rs.uniform(0, side, 3) + 1.0) for _ in range(n)]
        out.append(single("random_%02d" % k, "random", P, grid_scores(rs, n), fraction=float(rs.choice([0.0, 0.5, 0.8])), count=int(rs.randint(0, 13)),
                          min_angle=float(rs.choice([15.0, 30.0])), sym=tuple(rs.choice([0.0, 180.0, 360.0], 3).tolist()) if k % 4 == 3 else (0.0, 0.0, 0.0)))
    return out


FAMILIES = {"sizes": fam_sizes, "lds": fam_lds, "ties": fam_ties, "thresholds": fam_thresholds, "both": fam_both, "chains": fam_chains,
            "order": fam_argument_order, "quaternion": fam_quaternion, "gimbal": fam_gimbal, "sym": fam_sym, "count": fam_count,
            "degenerate": fam_degenerate, "batch": fam_batch, "random": fam_random}

_CACHE = {}


def cases(family=None):
    """the cases of one family (all families: None), built once"""
    if family is None:
        return [c for f in FAMILIES for c in cases(f)]
    if family not in _CACHE:
        _CACHE[family] = FAMILIES[family]()
    return _CACHE[family]


_REF = {}


def reference(case):
    """cluster_case(case) with its pairs, computed once per case and shared: (kept, survivors, classes, pairs)"""
    if case.name not in _REF:
        pairs = []
        kept, surv, classes = cluster_case(case, pairs)
        _REF[case.name] = (kept, surv, classes, pairs)
    return _REF[case.name]
