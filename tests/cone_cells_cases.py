"""Inputs and CPU references for the cone colouring of the congruent join (csrc/cone_cells.h), used by test_cone_cells_gpu.py.

Two sets of 4 096 cone queries (normal, cos alpha):
  random       the recipe of test_abi_cpu.py's host test (a quarter near the anti-parallel case, cos alpha uniform in (-1, 1)) plus the
               branch points of quat_from_z and of the cone table by hand;
  adversarial  normals found by bisection in float64 at which some sample's cell coordinate sits on an integer k (every k in 1..6 on every
               axis), and at offsets that move the coordinate by about +-1e-6 .. +-1e-4 cell units across it.
The references: the cone fields of a query from libm's float functions (the calls fill_cone_table and cone_trig make), the cell
coordinates t = (normalize(M(q) d) / 2 + 0.5) / nepsilon in float64, and cone_cell_exact's float32 operations restated in numpy."""
import ctypes as C
import ctypes.util

import numpy as np

F = np.float32
MAX_CONE = 64
MARGIN = float(F(5e-5))                                      # STOCS_CONE_MARGIN
NEPS = F(np.float64(F(1.0) / F(7.0)) + 0.00001)              # normalset.h:86, as congruent.hip computes it
N_QUERIES = 4096
# (the offsets within 2e-5 outnumber the others: more than half of the queries must end up that close to a boundary)
OFFSETS = (0.0, 1e-6, -1e-6, 2e-6, -2e-6, 5e-6, -5e-6, 1e-5, -1e-5, 1.5e-5, -1.5e-5, 4e-5, -4e-5, 5e-5, -5e-5, 6e-5, -6e-5, 1e-4, -1e-4)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in ("acosf", "atanf", "sinf", "cosf", "ceilf"):
    getattr(_libm, _f).restype = C.c_float
    getattr(_libm, _f).argtypes = [C.c_float]


def _trig_table():
    t = np.zeros((MAX_CONE + 1, MAX_CONE, 2), F)
    for nb in range(1, MAX_CONE + 1):
        step = F(np.float64(F(2.0)) * np.pi / np.float64(F(nb)))
        for a in range(nb):
            theta = F(F(a) * step)
            t[nb, a] = (_libm.cosf(theta), _libm.sinf(theta))
    return t


TRIG = _trig_table()


def cone_fields(cos_alpha):
    """-> (nb, sin_alpha) per query: fill_cone_table of congruent.hip (normalset.hpp:178-190), libm's float functions."""
    nb, sa = np.zeros(len(cos_alpha), np.int32), np.zeros(len(cos_alpha), F)
    for i, ca in enumerate(np.asarray(cos_alpha, F)):
        alpha = F(_libm.acosf(ca))
        perimeter = F(np.float64(F(2.0)) * np.pi * np.float64(F(_libm.atanf(alpha))))
        sa[i] = _libm.sinf(alpha)
        if alpha == alpha:
            n = int(2 * _libm.ceilf(F(F(perimeter * F(7.0)) / F(2.0))))
            nb[i] = n if n <= MAX_CONE else 0
    return nb, sa


def samples(cos_alpha, nb, sa):
    """-> d[n, 64, 3] float32 (sin_alpha * table entry, cos alpha), valid[n, 64]"""
    n = len(nb)
    d = np.zeros((n, MAX_CONE, 3), F)
    tr = TRIG[nb]                                            # n x 64 x 2
    d[:, :, 0] = sa[:, None] * tr[:, :, 0]
    d[:, :, 1] = sa[:, None] * tr[:, :, 1]
    d[:, :, 2] = np.asarray(cos_alpha, F)[:, None]
    return d, np.arange(MAX_CONE)[None, :] < nb[:, None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def t_float64(q, d):
    """Cell coordinates of the samples d[n, 64, 3] under the quaternions q[n, 4], in float64 from the float32 values."""
    q, d = np.asarray(q, np.float64), np.asarray(d, np.float64)
    qv, w = q[:, None, :3], q[:, None, 3:4]
    uv = 2.0 * _cross(qv, d)
    v = d + w * uv + _cross(qv, uv)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (v / np.linalg.norm(v, axis=-1, keepdims=True) / 2.0 + 0.5) / np.float64(NEPS)


def t_exact_float32(q, d):
    """cone_cell_exact before its truncation, float32 operation for operation: quat_rot, normalized3 (dot3: x x + (y y + z z)),
    index_normal's (n / 2 + 0.5) / nepsilon.  numpy's float32 +, -, *, / and sqrt are the IEEE operations the device performs."""
    q, d = np.asarray(q, F), np.asarray(d, F)
    qv, w = np.broadcast_to(q[:, None, :3], d.shape), q[:, None, 3:4]
    uv = _cross(qv, d)
    uv = uv + uv
    v = (d + w * uv) + _cross(qv, uv)
    z = v[..., 0] * v[..., 0] + (v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(z)[..., None]
        dirn = np.where((z > 0)[..., None], v / r, v)
        out = (dirn / F(2.0) + F(0.5)) / NEPS
    assert out.dtype == F
    return out


def cell_ids(t):
    """index_normal's truncation and cone_cell_exact's range test: -1 outside 0..342 or not finite"""
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(t).all(-1) & (np.abs(t) < 1e6).all(-1)
        c = np.trunc(np.where(ok[..., None], t, 0)).astype(np.int64)
    cid = c[..., 2] * 49 + (c[..., 1] * 7 + c[..., 0])
    return np.where(ok & (cid >= 0) & (cid < 343), cid, -1).astype(np.int32)


def quat_float64(n):
    """quat_from_z's general branch in float64 (setFromTwoVectors(z, n)); the caller keeps n away from -z"""
    v1 = n / np.linalg.norm(n, axis=-1, keepdims=True)
    c = v1[..., 2]
    assert (c > -0.999).all()
    s = np.sqrt((1.0 + c) * 2.0)
    return np.stack([-v1[..., 1] / s, v1[..., 0] / s, np.zeros_like(c), s * 0.5], -1)       # z x v1 = (-y, x, 0)


def quat_float32(nrm):
    """quat_from_z in float32, operation for operation, both branches -> q[n, 4], branch[n] (True: the near-anti-parallel branch)"""
    n = np.asarray(nrm, F)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = n[:, 0] * n[:, 0] + (n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        v1 = np.where((z > 0)[:, None], n / np.sqrt(z)[:, None], n)
        c = v1[:, 0] * F(0) + (v1[:, 1] * F(0) + v1[:, 2] * F(1))
        x = np.stack([F(0) * v1[:, 2] - F(1) * v1[:, 1], F(1) * v1[:, 0] - F(0) * v1[:, 2], F(0) * v1[:, 1] - F(0) * v1[:, 0]], -1)
        s = np.sqrt((F(1) + c) * F(2))
        general = np.concatenate([x * (F(1) / s)[:, None], (s * F(0.5))[:, None]], 1)
        branch = c < F(F(-1.0) + F(1e-5))
        cb = np.where(c > F(-1), c, F(-1))
        w2 = (F(1) + cb) * F(0.5)
        sb = np.sqrt(F(1) - w2)
        x2 = x[:, 0] * x[:, 0] + (x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
        ax = np.where((x2 > 0)[:, None], x / np.sqrt(x2)[:, None], np.array([1, 0, 0], F)[None, :])
        near = np.concatenate([ax * sb[:, None], np.sqrt(w2)[:, None]], 1)
    out = np.where(branch[:, None], near, general)
    assert out.dtype == F
    return out, branch


def _c_of(n):
    """c = dot(normalized3(n), z) as quat_from_z computes it in float32"""
    n = np.asarray(n, F)
    z = n[0] * n[0] + (n[1] * n[1] + n[2] * n[2])
    v = n / np.sqrt(z)
    return F(v[0] * F(0) + (v[1] * F(0) + v[2] * F(1)))


def threshold_normals():
    """Unit normals whose c is the float just below, equal to and just above the branch point -1 + 1e-5 of quat_from_z"""
    thr = F(F(-1.0) + F(1e-5))
    want = {"below": np.nextafter(thr, F(-2)), "at": thr, "above": np.nextafter(thr, F(0))}
    found = {}
    for steps in range(-16, 17):
        z = thr
        for _ in range(abs(steps)):
            z = np.nextafter(z, F(-2) if steps < 0 else F(0))
        for x in (F(np.sqrt(1.0 - float(z) ** 2)), ):
            for n in (np.array([x, 0, z], F), np.array([0, x, z], F), np.array([x * F(0.6), x * F(0.8), z], F)):
                c = _c_of(n)
                for k, v in want.items():
                    if c == v and k not in found:
                        found[k] = n
    assert set(found) == set(want), found.keys()
    return found


def random_queries(seed=20261004):
    """-> normals[4096, 3], cos_alpha[4096], special{name: index}"""
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(N_QUERIES, 3)).astype(F)
    for i in range(0, N_QUERIES, 4):
        nrm[i, :2] *= F(10.0 ** rng.uniform(-6, -1))
        nrm[i, 2] = -abs(nrm[i, 2])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(F)
    ca = rng.uniform(-1, 1, N_QUERIES).astype(F)
    special, k = {}, 1                                        # by hand, on slots that are not the near-anti-parallel ones

    def put(name, n, c=None):
        nonlocal k
        while k % 4 == 0:
            k += 1
        nrm[k] = n
        if c is not None:
            ca[k] = c
        special[name] = k
        k += 1
    thr = threshold_normals()
    for c in (0.3, -0.6):
        put("minus_z_%g" % c, (0, 0, -1), c); put("plus_z_%g" % c, (0, 0, 1), c)
        put("c_below_%g" % c, thr["below"], c); put("c_at_%g" % c, thr["at"], c); put("c_above_%g" % c, thr["above"], c)
        put("zero_%g" % c, (0, 0, 0), c)
    put("nan_x", (np.nan, 0.5, 0.5), 0.99); put("nan_all", (np.nan, np.nan, np.nan), 0.99)
    one = F(1.0)
    for name, c in (("cos_1", one), ("cos_below_1", np.nextafter(one, F(0))), ("cos_minus_1", -one), ("cos_above_1", np.nextafter(one, F(2)))):
        put(name, nrm[k], c)
        put(name + "_minus_z", (0, 0, -1), c)
    return nrm, ca, special


def _coord(n0, n1, theta, ca, d):
    """float64 cell coordinates [64, 3] of the samples d of one query at n(theta)"""
    n = (1.0 - theta) * n0 + theta * n1
    return t_float64(quat_float64(n[None, :]), d[None])[0]


def adversarial_queries(seed=20261021):
    """-> normals[4096, 3] float32, cos_alpha[4096] float32, target[4096, 3] = (axis, k, offset index) of the crossing a query was built on"""
    rng = np.random.default_rng(seed)
    per = len(OFFSETS)
    n_cross = N_QUERIES // per                                # 215 crossings x 19 offsets = 4 085, the rest repeats the first query
    nrm, ca_out, target = np.zeros((N_QUERIES, 3), F), np.zeros(N_QUERIES, F), np.zeros((N_QUERIES, 3), np.int32)
    grid = np.linspace(0.0, 1.0, 33)
    done = 0
    while done < n_cross:
        axis, k = done % 3, 1 + (done // 3) % 6
        n0, n1 = rng.normal(size=3), rng.normal(size=3)
        n0 /= np.linalg.norm(n0); n1 /= np.linalg.norm(n1)
        path = (1.0 - grid)[:, None] * n0 + grid[:, None] * n1
        if n0 @ n1 < -0.5 or (path[:, 2] / np.linalg.norm(path, axis=1)).min() < -0.9:      # a walk that stays clear of 0 and of -z
            continue
        ca = F(rng.uniform(-0.95, 0.95))
        nb, sa = cone_fields([ca])
        d, _ = samples([ca], nb, sa)
        d = d[0].astype(np.float64)
        g = np.stack([_coord(n0, n1, th, ca, d)[: nb[0], axis] - k for th in grid])        # 33 x nb
        flips = np.argwhere(np.sign(g[:-1]) * np.sign(g[1:]) < 0)
        if not len(flips):
            continue
        j, a = flips[rng.integers(len(flips))]
        f = lambda th: _coord(n0, n1, th, ca, d)[a, axis] - k
        lo, hi = grid[j], grid[j + 1]
        flo = f(lo)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            fm = f(mid)
            if (fm < 0) == (flo < 0):
                lo, flo = mid, fm
            else:
                hi = mid
        th0 = 0.5 * (lo + hi)
        slope = (f(th0 + 1e-6) - f(th0 - 1e-6)) / 2e-6
        if abs(slope) < 0.05:                                 # a grazing crossing: the offsets would leave the linear range
            continue
        for o, off in enumerate(OFFSETS):
            i = done * per + o
            n = (1.0 - (th0 + off / slope)) * n0 + (th0 + off / slope) * n1
            nrm[i] = (n / np.linalg.norm(n)).astype(F)
            ca_out[i] = ca
            target[i] = (axis, k, o)
        done += 1
    nrm[n_cross * per:] = nrm[0]; ca_out[n_cross * per:] = ca_out[0]; target[n_cross * per:] = target[0]
    return nrm, ca_out, target


def adversarial_condition(nrm, ca):
    """What the adversarial set must reach, from its float32 inputs in float64: -> (share of queries with a sample coordinate within 2e-5 of
    an integer, the set of (axis, k) on which such a coordinate occurs, dist[n, 64] = every sample's distance to its nearest cell
    boundary (inf beyond a query's samples))"""
    nb, sa = cone_fields(ca)
    d, valid = samples(ca, nb, sa)
    t = t_float64(quat_float64(nrm.astype(np.float64)), d)
    near = np.rint(t)
    dist = np.where(valid[..., None], np.abs(t - near), np.inf)
    close = dist < 2e-5
    reached = {(int(ax), int(k)) for ax, k in zip(np.nonzero(close)[2], near[close])}
    return float(close.any(axis=(1, 2)).mean()), reached, dist.min(-1)
