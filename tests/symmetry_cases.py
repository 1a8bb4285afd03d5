"""Seeded cases for the symmetry tests (tests/test_symmetry_cases_cpu.py checks that each holds what it is named for, without a GPU;
tests/test_symmetry_gpu.py runs the library on them).
A kernel case is dict(model (M, 3), normals (M, 3), transforms (K, 16) column-major in the model frame, reach, cos_normal).
A search case is dict(model, normals, tol (metres, or 0: a tenth of the diameter), expect = [(axis, order)], K, sym3, flags, center).
The sizes come from the constants the header names for the kernel."""
import math
import os
import re

import numpy as np

import pose_error_cases as pc
import symmetry_ref as ref

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COS30 = ref.COS30


def kernel_sizes():
    """STOCS_SYMMETRY_THREADS / _MAX_LAUNCH / _GRID_SPAN of include/stocs_hip.h"""
    txt = open(os.path.join(ROOT, "include", "stocs_hip.h")).read()
    return {k: int(re.search(r"#define\s+STOCS_SYMMETRY_%s\s+(\d+)" % k, txt).group(1)) for k in ("THREADS", "MAX_LAUNCH", "GRID_SPAN")}


def model_sizes():
    """the issue's list and one below / at / one above the workgroup's size (a lane's stride)"""
    t = kernel_sizes()["THREADS"]
    return sorted({1, 2, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1})


def launch_counts():
    """transform counts about the launch limit"""
    n = kernel_sizes()["MAX_LAUNCH"]
    return [n - 1, n, n + 1]


def normals_for(model, seed=0, unit=True):
    """roughly radial normals, disturbed; unit = False leaves them at lengths of 0.5 .. 2 (the context normalises)"""
    m = np.asarray(model, np.float64).reshape(-1, 3)
    rng = np.random.default_rng(77 + seed)
    n = m - m.mean(0) + rng.normal(0, 0.01, m.shape)
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-12)
    if not unit:
        n *= rng.uniform(0.5, 2.0, (len(m), 1))
    return n.astype(F)


def small_motion(rng, deg, shift):
    D = np.eye(4)
    D[:3, :3] = pc.rot(rng.normal(size=3), rng.uniform(0, deg))
    D[:3, 3] = rng.normal(0, shift, 3)
    return D.T.reshape(16).astype(F)


def random_case(M, K, seed, reach=0.01, unit=True):
    """the identity, then motions from a fraction of the reach to several: some points stay matched, some go far"""
    rng = np.random.default_rng(seed)
    model = pc.random_model(M, seed)
    T = [ref.IDENTITY] + [small_motion(rng, 3.0 * (1 + k % 5), reach * 0.3 * (k % 4)) for k in range(K - 1)]
    return dict(model=model, normals=normals_for(model, seed, unit), transforms=np.stack(T[:K]), reach=F(reach), cos_normal=F(COS30))


def translation(t):
    return pc.pose(None, t)


def face_lattice(flip=False, nx=None, h=2.0 ** -6):
    """nx x 2 x 2 lattice of spacing h, nx = GRID_SPAN + 1: the box is GRID_SPAN h long, so for every reach <= 64 / 65 h the cell edge is h
    and every point sits on a cell corner.  flip: the index order reversed (the lowest index then lies in the cell visited last)"""
    nx = nx or kernel_sizes()["GRID_SPAN"] + 1
    z, y, x = np.meshgrid(np.arange(2), np.arange(2), np.arange(nx), indexing="ij")
    m = (np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1) * h).astype(F)
    return m[::-1].copy() if flip else m


def lattice_case(flip):
    """on the faces (shifts by whole spacings: D = 0), ties of 2, 4 and 8 targets in as many cells (three_way_case has the tie of three) (shifts by half a spacing along 1, 2,
    3 axes) at a reach of 7 / 8 h, and the 2-way tie exactly at the reach (h / 2: D == reach * reach), one ulp below and one above it"""
    h = 2.0 ** -6
    m = face_lattice(flip)
    nrm = np.tile(np.array([0, 0, 1], F), (len(m), 1))
    T = np.stack([ref.IDENTITY, translation((h, 0, 0)), translation((-3 * h, h, 0)), translation((h / 2, 0, 0)), translation((h / 2, h / 2, 0)),
                  translation((h / 2, h / 2, h / 2)), translation((-h / 2, 0, -h / 2))])
    return dict(model=m, normals=nrm, transforms=T, h=F(h), cos_normal=F(COS30),
                reaches=dict(wide=F(0.875 * h), at=F(h / 2), below=np.nextafter(F(h / 2), F(0)), above=np.nextafter(F(h / 2), F(1))))


def three_way_case(lowest_last=True, s=2.0 ** -6):
    """exactly three targets equidistant from one query, in three different cells, none of them the query's own: with c = 1.5 s (1, 1, 1)
    the targets are c + a e_x, c + a e_y, c + a e_z, a = 0.75 s, every D = a * a exactly.  Two anchors span a box of GRID_SPAN s along x,
    so at the reach of 7 / 8 s the cell edge is s: c lies in cell (1, 1, 1) and the targets in (2, 1, 1), (1, 2, 1), (1, 1, 2).  The
    query is point 3 under the one translation.  lowest_last: the lowest index is the target along z, whose cell a walk in ascending
    z, y, x meets last; otherwise the one along x, met first"""
    span = kernel_sizes()["GRID_SPAN"]
    c, a = np.array([1.5, 1.5, 1.5]) * s, 0.75 * s
    tx, ty, tz = c + (a, 0, 0), c + (0, a, 0), c + (0, 0, a)
    src = c + (4 * s, 0, 0)
    first3 = [tz, ty, tx] if lowest_last else [tx, ty, tz]
    m = np.array(first3 + [src, (0, 0, 0), (span * s, 0, 0)]).astype(F)
    nrm = np.tile(np.array([0, 0, 1], F), (len(m), 1))
    return dict(model=m, normals=nrm, transforms=np.stack([translation((-4 * s, 0, 0)), ref.IDENTITY]), reach=F(0.875 * s), cos_normal=F(COS30), s=F(s),
                query=3, a=F(a), lowest_last=lowest_last)


def duplicates_case(M=130, seed=3):
    half = pc.random_model(M // 2, seed)
    model = np.concatenate([half, half])
    rng = np.random.default_rng(seed)
    return dict(model=model, normals=normals_for(model, seed), transforms=np.stack([ref.IDENTITY, small_motion(rng, 2.0, 0.002)]), reach=F(0.01),
                cos_normal=F(COS30))


def outside_case(M=200, seed=4):
    """transform 0 throws every point far outside the grid's box (all far); 1 shifts the cloud by half its length along x (about half of the
    points land inside the box); 2 by a little more than its whole length plus the reach (the cells just outside the box)"""
    model = pc.random_model(M, seed)
    ext = float(model[:, 0].max() - model[:, 0].min())
    T = np.stack([translation((10.0, -7.0, 3.0)), translation((ext / 2, 0, 0)), translation((ext + 0.0101, 0, 0)), translation((1e30, 0, 0))])
    return dict(model=model, normals=normals_for(model, seed), transforms=T, reach=F(0.01), cos_normal=F(COS30))


def bad_normals_case(M=63, seed=5):
    """normal 5 is NaN, normal 9 is zero: under the identity both points are matched (to themselves) and both count as bad"""
    model = pc.random_model(M, seed)
    n = normals_for(model, seed, unit=False)
    n[5] = np.nan
    n[9] = 0
    rng = np.random.default_rng(seed)
    return dict(model=model, normals=n, transforms=np.stack([ref.IDENTITY, small_motion(rng, 2.0, 0.001)]), reach=F(0.01), cos_normal=F(COS30))


def nan_point_case(M=63, at=17, seed=7):
    """one model point is NaN (below 64 points a context takes such a model): it is far under every transform and nobody's neighbour"""
    c = random_case(M, 3, seed)
    c["model"][at] = np.nan
    c["at"] = at
    return c


def span_case(k, M=150, seed=8):
    """the reach at which the box is k cells of 65 / 64 reach long: below GRID_SPAN the reach sets the cell edge, above it the box does"""
    model = pc.random_model(M, seed)
    ext = float((model.max(0).astype(np.float64) - model.min(0).astype(np.float64)).max())
    rng = np.random.default_rng(seed)
    reach = F(ext / k * 64.0 / 65.0)
    T = np.stack([ref.IDENTITY] + [small_motion(rng, 1.0, float(reach) * 0.5) for _ in range(3)])
    return dict(model=model, normals=normals_for(model, seed), transforms=T, reach=reach, cos_normal=F(COS30))


def kernel_cases():
    """name -> case with one reach"""
    out = {}
    for M in model_sizes():
        out["random_M%d" % M] = random_case(M, 5, 100 + M, unit=(M % 2 == 0))
    for flip in (False, True):
        c = lattice_case(flip)
        for name, r in c["reaches"].items():
            d = dict(c); d["reach"] = r
            out["lattice_%s_%s" % ("flipped" if flip else "plain", name)] = d
    out["three_way_lowest_last"] = three_way_case(True)
    out["three_way_lowest_first"] = three_way_case(False)
    out["duplicates"] = duplicates_case()
    out["outside"] = outside_case()
    out["bad_normals"] = bad_normals_case()
    out["nan_point"] = nan_point_case()
    span = kernel_sizes()["GRID_SPAN"]
    for k in (span - 1, span, span + 1):
        out["span_%d" % k] = span_case(k)
    out["millimetres"] = dict(random_case(300, 4, 9), reach=F(10.0))
    out["millimetres"]["model"] = (out["millimetres"]["model"].astype(np.float64) * 1000).astype(F)
    out["millimetres"]["transforms"][:, 12:15] *= F(1000)
    return out


# ---- search cases: a seeded generator cloud replicated by a group in float64, rounded once ----
def blade(n, seed, length=0.06, width=0.08, lift=0.35):
    """n points and normals of a thin curved blade along +x in its own frame: radius 0.012 .. length, azimuth within +-width / 2 radians,
    height lift r + a ripple (no mirror, no perpendicular half turn maps it onto itself)"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.012, length, n)
    phi = rng.uniform(-width / 2, width / 2, n)
    z = lift * r + 0.004 * np.sin(90.0 * r)
    p = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    nrm = np.stack([-lift * np.cos(phi), -lift * np.sin(phi), np.ones(n)], axis=1) + rng.normal(0, 0.05, (n, 3))
    return p, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def frame_of(axis):
    """a rotation that takes z to axis"""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    u = np.cross(a, [1.0, 0.0, 0.0]); u /= np.linalg.norm(u)
    return np.stack([u, np.cross(a, u), a], axis=1)


def replicate(p, n, rotations, frame=None, centre=(0, 0, 0)):
    """the orbit of the cloud under 3x3 rotations of its own frame, then into the model frame; float64 until the end"""
    P = np.concatenate([p @ R.T for R in rotations]); N = np.concatenate([n @ R.T for R in rotations])
    if frame is not None:
        P, N = P @ frame.T, N @ frame.T
    return (P + np.asarray(centre, np.float64)).astype(F), N.astype(F)


def c4_z(n=45, seed=21):
    """C4 about z by EXACT quarter turns: the generator cloud is rounded first, its copies permute and negate the rounded coordinates"""
    p, nrm = blade(n, seed, length=0.08, width=0.05, lift=0.8)
    p, nrm = p.astype(F), nrm.astype(F)
    turn = lambda v: np.stack([-v[:, 1], v[:, 0], v[:, 2]], axis=1)
    P, N = [p], [nrm]
    for _ in range(3):
        P.append(turn(P[-1])); N.append(turn(N[-1]))
    return dict(model=np.concatenate(P), normals=np.concatenate(N), tol=0.004, expect=[((0, 0, 1), 4)], K=4, sym3=(0, 0, 90), flags=0,
                false_axes=[(1, 0, 0), (0, 1, 0)])


C3_AXIS = (0.3, -0.5, 0.81)


def c3_tilted(n=60, seed=22):
    """C3 about an axis off the lattice and off the origin"""
    p, nrm = blade(n, seed, length=0.07, lift=0.8)
    model, normals = replicate(p, nrm, [pc.rot((0, 0, 1), 120.0 * k) for k in range(3)], frame_of(C3_AXIS), (0.01, -0.02, 0.03))
    return dict(model=model, normals=normals, tol=0.004, expect=[(C3_AXIS, 3)], K=3, sym3=(0, 0, 0), flags=ref.INEXACT,
                false_axes=[(1, 0, 0), (0, 1, 0), (0, 0, 1)])


def d2(n=70, seed=23):
    """D2: three perpendicular half turns about the coordinate axes; one compact lump per orbit point"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = np.array([0.05, 0.028, 0.012]) + d * np.array([0.009, 0.007, 0.005]) * rng.uniform(0.5, 1.0, (n, 1))
    nrm = d + rng.normal(0, 0.05, (n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    model, normals = replicate(p, nrm, [np.diag(s) for s in ((1.0, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))])
    return dict(model=model, normals=normals, tol=0.006, expect=[((1, 0, 0), 2), ((0, 1, 0), 2), ((0, 0, 1), 2)], K=4, sym3=(180, 180, 180), flags=0,
                false_axes=[])


def revolution(rings=8, per_ring=60, seed=24):
    """a vase about z: rings of 60 points, so that every order 2 .. 6 maps it onto itself exactly (continuous by the search's definition);
    the profile has no mirror in z, so no perpendicular axis"""
    rng = np.random.default_rng(seed)
    P, N = [], []
    for k in range(rings):
        z = -0.04 + 0.011 * k
        rho = 0.018 + 0.032 * (k / (rings - 1.0)) ** 2
        a = 2 * np.pi * (np.arange(per_ring) / per_ring) + rng.uniform(0, 2 * np.pi)
        P.append(np.stack([rho * np.cos(a), rho * np.sin(a), np.full(per_ring, z)], axis=1))
        N.append(np.stack([np.cos(a), np.sin(a), np.full(per_ring, -0.5)], axis=1) / math.sqrt(1.25))
    return dict(model=np.concatenate(P).astype(F), normals=np.concatenate(N).astype(F), tol=0.004, expect=[((0, 0, 1), 0)], K=72, sym3=(0, 0, 360), flags=0,
                false_axes=[(1, 0, 0), (0, 1, 0)])


def blob(M=300, seed=25):
    """a seeded bumpy ellipsoid shell with no symmetry"""
    model = pc.random_model(M, seed)
    return dict(model=model, normals=normals_for(model, seed), tol=0.003, expect=[], K=1, sym3=(0, 0, 0), flags=ref.NOTHING, false_axes=[(1, 0, 0), (0, 1, 0), (0, 0, 1)])


SEARCH_CASES = dict(c4_z=c4_z, c3_tilted=c3_tilted, d2=d2, revolution=revolution, blob=blob)
_CACHE = {}


def search_case(name):
    """the case with its resolved tolerance (float32) and centre, built once per process"""
    if name not in _CACHE:
        c = SEARCH_CASES[name]()
        import pose_error_ref as base
        c["diameter"] = base.diameter(c["model"])
        c["tol_resolved"] = F(c["tol"]) if c["tol"] > 0 else F(0.1) * c["diameter"]
        c["center"] = ref.centroid(c["model"])
        _CACHE[name] = c
    return _CACHE[name]


def search_restated(name):
    """what the restated search returns on float64 scores, once per process -> (axes, set, sym3, flags)"""
    key = ("found", name)
    if key not in _CACHE:
        c = search_case(name)
        score = ref.scorer64(c["model"], c["normals"], float(c["tol_resolved"]), COS30)
        _CACHE[key] = ref.find(score, len(c["model"]), c["tol_resolved"], c["center"])
    return _CACHE[key]


def axis_bound_deg(n_axes=2048, rounds=4):
    """twice the last round's cone spacing, lattice spacing / 2^rounds: derived from the search's parameters"""
    return math.degrees(2.0 * ref.lattice_spacing(n_axes) / 2 ** rounds)


def angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return math.degrees(math.acos(min(1.0, abs(float(a @ b)) / (np.linalg.norm(a) * np.linalg.norm(b)))))
