"""Small scenes and models that put the scene grid (grid.hip) and the scan kernels (lcp.hip) on their edges: queries on the cell,
sub-cell, brick and outer faces AS THE KERNELS COMPUTE THEM, scene points a few float steps inside and outside epsilon, exact ties,
lists at their padding / group / re-read lengths, degenerate clouds, scenes whose extent strains the float cell computation, and
scenes on either side of the build's thresholds.  The model's points are the queries.

Both clouds are point-mirrored and interleaved (p, -p, p', -p', ...): the sequential float centroid sum of ctx.hip returns to exactly
zero after every pair, so centring changes nothing and a query built here is the query the kernel sees (asserted in assemble()).
Scene normals are +-z, model normals are the axis that a case's designed transform turns into +-z, and the general transforms tilt
by five degrees only: every normal product is ~0, ~0.09, ~0.996 or 1 -- far from cos 30.

A case is a dict: name, eps, spos, snrm, sprob, spix, mpos, mnrm, T (n x 16, column-major), intent (transform, model index, div,
axis, sub, expected floor of (q - o) * inv_h * sub), min_hits / min_misses (32 unless the scene is one or two points), divs (the cell
edges the GPU matrix builds it at), box (the half-extent that fixes the grid's geometry whatever else the scene holds)."""
import functools
import math

import numpy as np

import grid_ref as ref

F = ref.F
EPS_DEFAULT = F(0.005)
EPS_POW2 = F(2.0 ** -8)


def mirror(a):
    a = np.asarray(a, F)
    out = np.empty((2 * len(a), a.shape[1]), F)
    out[0::2] = a
    out[1::2] = -a
    return out


def T16(R, t):
    T = np.zeros(16, F)
    R = np.asarray(R, np.float64)
    for col in range(3):
        for row in range(3):
            T[4 * col + row] = F(R[row, col])
    T[12:15] = np.asarray(t, F)
    T[15] = 1
    return T


RZ90 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])
RX90 = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]])
DESIGNED = [(np.eye(3, dtype=int), np.zeros(3)), (RZ90, np.array([3, -2, 1]) * 2.0 ** -10), (RX90, np.array([-1, 2, 2]) * 2.0 ** -10)]


def general_transforms(rng, eps, n=3):
    out = []
    for _ in range(n):
        a, b = rng.uniform(0, 2 * math.pi), math.radians(5.0)
        Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
        Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
        out.append(T16(Rz @ Rx, rng.uniform(-0.5, 0.5, 3) * float(eps)))
    # and one that barely moves anything: the designed queries leave their faces by a few float steps
    b = 1e-4
    out.append(T16(np.array([[math.cos(b), -math.sin(b), 0], [math.sin(b), math.cos(b), 0], [0, 0, 1]]), rng.uniform(-1e-3, 1e-3, 3) * float(eps)))
    return out


def box_geoms(box, eps, divs=(1, 2, 3, 4)):
    """The grid's geometry at every cell edge, from the two anchor points +-box alone."""
    return {d: ref.geometry(np.array([box, -np.asarray(box)], F), eps, d) for d in divs}


def ulps(d2, s2):
    return np.asarray(d2, F).view(np.int32).astype(np.int64) - int(np.asarray(s2, F).view(np.int32))


def partner(rng, q, dirn, eps, want, n=8000, spread=5e-5, tries=8):
    """A float32 scene point about eps from q along dirn whose kernel-order d2 is: want = 'in' -> the largest found <= fl(eps*eps),
    'out' -> the smallest found above it, an int -> exactly that many float steps from it.  -> (point, float steps from fl(eps*eps))"""
    e, s2 = float(F(eps)), ref.sq_eps(eps)
    q = np.asarray(q, F)
    dirn = np.asarray(dirn, np.float64) / np.linalg.norm(dirn)
    w = max(spread * e, (4.0 if isinstance(want, str) else 64.0) * float(np.spacing(F(np.abs(q).max() + e))))   # room to choose among floats
    for _ in range(tries):
        cand = (q.astype(np.float64) + dirn * e + rng.uniform(-w, w, (n, 3))).astype(F)
        u = ulps(ref.d2_f32(q[None], cand)[0], s2)
        if want == "in":
            ok, key = u <= 0, -u
        elif want == "out":
            ok, key = u >= 1, u
        else:
            ok, key = u == want, np.zeros_like(u)
        if ok.any():
            i = int(np.argmin(np.where(ok, key, np.iinfo(np.int64).max)))
            return cand[i], int(u[i])
    raise AssertionError("no partner found (%s)" % (want,))


def lattice_sites(rng, lo, hi, step):
    ax = [np.arange(lo[k], hi[k] + 1e-12, step) for k in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    g = g + rng.uniform(-0.2, 0.2, g.shape) * step * 0.5
    return list(g[rng.permutation(len(g))])


def step_float(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf if k > 0 else -np.inf))
    return x


def face_probes(rng, eps, geoms, sites, box, pure_axis=False):
    """Queries on the kernel's cell / sub-cell / brick faces (one float below, on, one float above), each with a scene point across
    the face just inside or just outside epsilon.  -> (scene points, queries, q_intent (query, div, axis, sub, expected), steps)"""
    e = float(F(eps))
    S, Q, intent, steps, worst = [], [], [], [], []
    for d, g in geoms.items():
        kinds = [("cell", 1, 0), ("brick", 1, 0)] + ([("sub", 4, j) for j in (1, 2, 3)] if d == 1 else [])
        for axis in range(3):
            for kind, sub, j in kinds:
                for off in (-1, 0, 1):
                    for want in ("in", "out"):
                        if kind == "brick":      # the free site nearest to a brick face on this axis
                            u = [(c[axis] - g["o"][axis]) / (8 * g["h64"]) for c in sites]
                            c = sites.pop(int(np.argmin([abs(v - round(v)) for v in u])))
                            k = 8 * int(round((c[axis] - g["o"][axis]) / (8 * g["h64"])))
                        else:
                            c = sites.pop()
                            k = int(math.floor((c[axis] - g["o"][axis]) / g["h64"])) * sub + (j if sub == 4 else 1)
                        q = np.asarray(c, F).copy()
                        q[axis] = step_float(ref.face_float(g, axis, k, sub), off)
                        if abs(float(q[axis])) > box[axis] - 1.5 * e:       # (a thin scene: no room for a point across this face)
                            continue
                        side = 1.0 if off < 0 else -1.0        # the scene point lies across the face
                        dirn = np.zeros(3); dirn[axis] = side
                        if not pure_axis:
                            dirn[(axis + 1) % 3], dirn[(axis + 2) % 3] = 0.03, -0.02
                        p, u = partner(rng, q, dirn, eps, want)
                        intent.append((len(Q), d, axis, sub, k - 1 if off < 0 else k))
                        Q.append(q); S.append(p); steps.append(u)
    if pure_axis:
        # The faces where the kernels' float face lies farthest from the build's (float origin + k h in double): a query on the
        # kernels' face float is then that far inside the NEIGHBOURING cell's box, and a scene point at epsilon behind it is that
        # much farther than epsilon from the box of the cell the kernels look in.  Three per sign, axis and cell edge, chosen among
        # the faces within two cells of 60 free sites
        for d, g in geoms.items():
            for axis in (0, 1):
                cand = []
                for si in range(min(len(sites), 60)):
                    k0 = int(math.floor((sites[si][axis] - g["o"][axis]) / g["h64"]))
                    for k in range(k0 - 1, k0 + 3):
                        qf = ref.face_float(g, axis, k)
                        cand.append((float(g["origin"][axis]) + k * g["h64"] - float(qf), si, k, qf))
                cand.sort(key=lambda t: t[0])
                chosen, used = [], set()
                for group in ([t for t in cand[::-1] if t[0] > 0], [t for t in cand if t[0] < 0]):
                    for t in [t for t in group][:60]:
                        if t[1] not in used and sum(1 for c in chosen if (c[0] > 0) == (t[0] > 0)) < 3:
                            chosen.append(t); used.add(t[1])
                for delta, si, k, qf in chosen:
                    for want in ("in", "out"):
                        q = np.asarray(sites[si], F).copy()
                        q[1 - axis] += F((0.0 if want == "in" else 2.5) * e)            # (the two share a site, 2.5 epsilons apart)
                        q[axis] = qf if delta > 0 else step_float(qf, -1)
                        dirn = np.zeros(3); dirn[axis] = -1.0 if delta > 0 else 1.0
                        p, u = partner(rng, q, dirn, eps, want)
                        intent.append((len(Q), d, axis, 1, k if delta > 0 else k - 1))
                        Q.append(q); S.append(p); steps.append(u); worst.append(delta / e)
                for si in sorted(used, reverse=True):
                    sites.pop(si)
    return S, Q, intent, steps, worst


def outer_probes(rng, geoms, lo, hi):
    """Queries on the grid's outer faces and one cell outside them, per axis and at the corners.  No scene point can be near: the
    grid is padded beyond the scene's box by more than epsilon."""
    Q, intent = [], []
    for d, g in geoms.items():
        n = g["cells"]
        for axis in range(3):
            for k in (0, n[axis], -1, n[axis] + 1):
                for off in (-1, 0, 1):
                    q = rng.uniform(lo, hi).astype(F)
                    q[axis] = step_float(ref.face_float(g, axis, k), off)
                    intent.append((len(Q), d, axis, 1, k - 1 if off < 0 else k))
                    Q.append(q)
        for corner in range(8):
            for off in (-1, 0):
                ks = [n[a] if (corner >> a) & 1 else 0 for a in range(3)]
                q = np.array([step_float(ref.face_float(g, a, ks[a]), off) for a in range(3)], F)
                for a in range(3):
                    intent.append((len(Q), d, a, 1, ks[a] + off))
                Q.append(q)
    return Q, intent


def shell_queries(rng, pts, eps, n, lo=0.5, hi=1.5):
    pts = np.asarray(pts, np.float64)
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1)[:, None]
    return list((pts[rng.integers(0, len(pts), n)] + v * rng.uniform(lo, hi, (n, 1)) * float(eps)).astype(F))


def assemble(name, eps, rng, box, s_half, Q, q_intent=(), designed=DESIGNED, general=True, **meta):
    """Mirror both clouds, derive the model from the queries and the designed transforms, and check what the docstring promises."""
    box = np.asarray(box, np.float64)
    s_half = np.concatenate([np.asarray([box], F), np.asarray(s_half, F).reshape(-1, 3)])
    assert np.all(np.abs(s_half) <= box.astype(F)), name
    spos = mirror(s_half)
    nS = len(spos)
    snrm = np.zeros((nS, 3), F); snrm[:, 2] = rng.choice([-1.0, 1.0], nS)
    sprob = rng.uniform(0.2, 1.0, nS).astype(F)
    spix = np.stack([np.arange(nS) // 640, np.arange(nS) % 640], 1).astype(np.int32)
    Q = np.asarray(Q, F).reshape(-1, 3)
    nQ = len(Q)
    m_half, n_half = [], []
    sign = rng.choice([-1.0, 1.0], nQ)
    for R, t in designed:
        m_half.append(((Q - np.asarray(t, F)).astype(F) @ R.astype(F)).astype(F))
        n_half.append(np.stack([np.zeros(nQ), np.zeros(nQ), sign], 1).astype(F) @ R.astype(F))
    mpos = mirror(np.concatenate(m_half))
    mnrm = np.repeat(np.concatenate(n_half).astype(F), 2, axis=0)
    T = [T16(R, t) for R, t in designed] + (general_transforms(rng, eps) if general else [])
    case = dict(name=name, eps=F(eps), spos=spos, snrm=snrm, sprob=sprob, spix=spix, mpos=mpos, mnrm=mnrm, T=np.asarray(T, F),
                box=box, min_hits=32, min_misses=32, divs=(1, 2, 3, 4), n_queries=nQ)
    case.update(meta)
    # centring is the identity on both clouds
    for cloud in (spos, mpos):
        c, cen = ref.centre(cloud)
        assert np.all(cen == 0) and np.array_equal(c, cloud), name
    # the designed transforms put the model's subsets back on the queries, exactly, wherever the float subtraction of the lattice
    # translation was exact; the intent follows those
    intent, exact = [], []
    for j in range(len(designed)):
        idx = 2 * (j * nQ + np.arange(nQ))
        back = ref.transform(T[j], mpos[idx])
        same = np.all(back == Q, axis=1)
        exact.append(float(same.mean()) if nQ else 1.0)
        intent += [(j, int(idx[qi]), d, axis, sub, k) for qi, d, axis, sub, k in q_intent if same[qi]]
    assert exact[0] == 1.0 and (not len(q_intent) or min(exact) > 0.6), (name, exact)
    case["intent"] = intent
    return case


def _faces(name, eps, seed):
    rng = np.random.default_rng(seed)
    e = float(F(eps))
    box = np.array([64.0, 64.0, 46.0]) * e
    geoms = box_geoms(box, eps)
    sites = lattice_sites(rng, 6 * e * np.ones(3), box - 6 * e, 6 * e)
    S, Q, intent, steps, _ = face_probes(rng, eps, geoms, sites, box)
    Qo, into = outer_probes(rng, geoms, -box, box)
    intent += [(qi + len(Q), d, a, s, k) for qi, d, a, s, k in into]
    return assemble(name, eps, rng, box, S, Q + Qo, intent, partner_steps=steps)


def _radius(name, eps, seed):
    rng = np.random.default_rng(seed)
    e = float(F(eps))
    box = np.array([70.0, 70.0, 70.0]) * e
    # sites that stay four epsilons apart in every coordinate plane (one coordinate of a query is moved next to zero below): lattice
    # indices (b + 2c mod 15, b, c) -- any two of the three determine the third
    sites = [(np.array([(b + 2 * c) % 15, b, c]) * 4.0 + 6.0 + rng.uniform(-0.4, 0.4, 3)) * e for b in range(15) for c in range(15)]
    sites = [sites[i] for i in rng.permutation(len(sites))]
    dirs = [v for v in np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3) if np.any(v)]
    S, Q, steps = [], [], []
    for v in dirs:
        for want in (-1, 0, 1, -1, 0, 1):
            # q - p is a multiple of p's float spacing, so at a site's coordinates d2 moves in steps of a dozen floats whatever q is.
            # One coordinate of the query goes next to zero (the mirror images are an octant away), where the floats are 16 times
            # denser, and the search window is wide enough for the other two offsets to fill what is left
            q = np.asarray(sites.pop(), F)
            q[int(np.nonzero(v)[0][0])] = F(rng.uniform(-0.1, 0.1) * e)
            p, u = partner(rng, q, v, eps, want, n=20000, spread=5e-4, tries=64)
            S.append(p); Q.append(q); steps.append(u)
    # along the axes the offset that IS epsilon: d2 = fl(eps*eps) by the same float product that makes the threshold
    for a in range(3):
        for sgn in (-1.0, 1.0):
            for off in (-1, 0, 1):
                q = np.asarray(sites.pop(), F); q[a] = 0
                p = q.copy(); p[a] = F(sgn) * step_float(F(eps), off)
                S.append(p); Q.append(q)
                steps.append(int(ulps(ref.d2_f32(q[None], p[None])[0], ref.sq_eps(eps))[0]))
                assert off != 0 or steps[-1] == 0
    return assemble(name, eps, rng, box, S, Q, partner_steps=steps)


def _ties(seed=3):
    rng = np.random.default_rng(seed)
    eps, a, u = EPS_DEFAULT, 2.0 ** -10, 2.0 ** -10
    box = np.array([0.25, 0.25, 0.25])
    S, Q = [], []
    site = lambda: (rng.integers(16, 200, 3) * u).astype(np.float64)       # lattice sites: c +- a is exact in float
    used = set()
    for corners in ([(1, 0, 0), (-1, 0, 0)], [(x, y, 0) for x in (-1, 1) for y in (-1, 1)], [(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]):
        for _ in range(12):
            c = site()
            while any(np.abs(c - o).max() < 8 * u for o in used):
                c = site()
            used.add(tuple(c))
            pts = [c + a * np.array(k) for k in corners]
            for i in rng.permutation(len(pts)):
                S.append(pts[i])
            Q.append(c)
            Q.append(c + np.array([8 * a, 0, 0]))                        # the same group from outside epsilon
    for _ in range(12):                                                    # exact duplicates: the last copy wins
        c = site()
        while any(np.abs(c - o).max() < 8 * u for o in used):
            c = site()
        used.add(tuple(c))
        S += [c, c + a * np.array([0, 2, 0]), c, c]
        Q += [c, c + a * np.array([1, 0, 0]), c + a * np.array([0, 9, 0])]
    return assemble("ties", eps, rng, box, S, Q)


LIST_LENGTHS = (7, 8, 9, 15, 16, 17, 63, 64, 65, 129)


def _clusters(rng, eps, centres, per_cluster=40):
    e = float(F(eps))
    S, Q = [], []
    for c, N in zip(centres, LIST_LENGTHS):
        pts = c + rng.integers(-2048, 2049, (N, 3)) * (e / 16 / 2048)
        dup = rng.integers(0, N, N // 4)
        pts[rng.integers(0, N, N // 4)] = pts[dup]                           # exact duplicates among them
        S += list(pts)
        Q += shell_queries(rng, c[None], eps, per_cluster, 0.2, 1.6) + list(pts[rng.integers(0, N, 4)].astype(F))
    return S, Q


def _lists(sparse, seed=4):
    """Ten clusters of 7 ... 129 points, each alone in its neighbourhood and inside one cell at every cell edge: the list of that cell
    (and of its nearest neighbours) holds exactly the cluster.  sparse: 600 lone points besides, so that the average list is short
    (prune group of 16 lanes)."""
    rng = np.random.default_rng(seed)
    eps = EPS_DEFAULT
    e = float(eps)
    box = np.array([70.0, 70.0, 30.0]) * e
    g1 = box_geoms(box, eps, (1,))[1]
    centres = []
    for i in range(len(LIST_LENGTHS)):
        c = np.array([8 + 12 * (i % 5), 8 + 12 * (i // 5), 10.0]) * e
        k = np.floor((c - g1["o"]) / g1["h64"])
        # the faces of the eps/2, eps/3 and eps/4 grids lie on multiples of eps/12 from the eps grid's origin, the nearest ones to
        # an eighth of a cell at 0 and 1/4: a cluster of half-width eps/16 around it crosses none of them
        centres.append(g1["o"] + (k + 0.125) * g1["h64"])
    S, Q = _clusters(rng, eps, centres)
    if sparse:
        lone = lattice_sites(rng, np.array([4.0, 32.0, 4.0]) * e, box - 4 * e, 3.5 * e)[:600]
        S += lone
        Q += shell_queries(rng, np.asarray(lone), eps, 300)
    case = assemble("lists_sparse" if sparse else "lists", eps, rng, box, S, Q, cluster_centres=np.asarray(centres))
    return case


def _cloud(name, eps, rng, box, s_half, n_q=400, extra_q=(), **meta):
    s_half = np.asarray(s_half, np.float64).reshape(-1, 3)
    Q = shell_queries(rng, s_half, eps, n_q) + list(extra_q)
    return assemble(name, eps, rng, box, s_half, Q, **meta)


def _one_point():
    """nS = 1: the centred scene is the origin.  (No mirror image, no anchor: the one cloud that centring does move.)"""
    rng = np.random.default_rng(5)
    eps = EPS_DEFAULT
    spos = np.array([[0.1, 0.2, 0.3]], F)
    Q = shell_queries(rng, np.zeros((1, 3)), eps, 24, 0.2, 1.8)
    case = assemble("one_point", eps, rng, np.zeros(3), np.zeros((0, 3)), Q, min_hits=6, min_misses=6)
    case.update(spos=spos, snrm=case["snrm"][:1], sprob=case["sprob"][:1], spix=case["spix"][:1], box=None)
    return case


def _two_points():
    rng = np.random.default_rng(6)
    eps = EPS_DEFAULT
    box = np.array([0.6, 0.0, 0.0]) * float(eps)
    Q = shell_queries(rng, np.array([box, -box]), eps, 48, 0.2, 1.8) + [np.zeros(3, F)]       # the origin: a tie, the larger index wins
    return assemble("two_points", eps, rng, box, np.zeros((0, 3)), Q, min_hits=10, min_misses=10)


def _collinear():
    rng = np.random.default_rng(7)
    e = float(EPS_DEFAULT)
    x = np.arange(1, 120) * 0.4 * e
    pts = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    return _cloud("collinear", EPS_DEFAULT, rng, np.array([48.0 * e, 0, 0]), pts)


def _planar():
    rng = np.random.default_rng(8)
    e = float(EPS_DEFAULT)
    g = np.stack(np.meshgrid(np.arange(-20, 21), np.arange(1, 21), indexing="ij"), -1).reshape(-1, 2) * 0.5 * e
    pts = np.concatenate([g, np.zeros((len(g), 1))], 1)
    return _cloud("planar", EPS_DEFAULT, rng, np.array([10.5 * e, 10.5 * e, 0]), pts)


def _one_cell():
    rng = np.random.default_rng(9)
    e = float(EPS_DEFAULT)
    box = np.array([0.2, 0.2, 0.2]) * e
    pts = rng.uniform(-0.2, 0.2, (40, 3)) * e
    return _cloud("one_cell", EPS_DEFAULT, rng, box, pts)


def _two_clusters():
    """Two clusters 80 cells apart (the second is the mirror image of the first), empty bricks between them and queries inside those."""
    rng = np.random.default_rng(10)
    e = float(EPS_DEFAULT)
    c = np.array([40.0, 3.0, -2.0]) * e
    pts = c + rng.uniform(-1.5, 1.5, (150, 3)) * e
    box = np.abs(c) + 1.5 * e
    gap = [np.array([x, y, z], F) * F(e) for x in np.linspace(-30, 30, 13) for y in (-3.0, 0.0, 3.0) for z in (-2.0, 2.0)]
    return _cloud("two_clusters", EPS_DEFAULT, rng, box, pts, extra_q=gap)


def extent_ratio_max():
    """Extent over epsilon at which the flat scene's top table at cell edge eps holds about 30 M bricks: (ratio / 8)^2 bricks in each of
    the two layers that five epsilons of thickness plus the padding need."""
    return 8 * int(math.sqrt(15.0e6)) - 16


def _extent(name, ratio, divs, seed, rod=False):
    """A flat scene `ratio` epsilons wide with the face probes at the corner farthest from the grid's origin, where the float offset
    (q - o) is largest and its rounding coarsest.  Scene points lie across the faces along the axis alone: nothing but the distance
    along that axis decides whether the neighbouring cell's list holds them."""
    rng = np.random.default_rng(seed)
    eps = F(0.001)
    e = float(eps)
    box = np.array([ratio / 2.0, 120.0 if rod else ratio / 2.0, 2.5]) * e      # rod: long in x only, so the top table stays small
    geoms = box_geoms(box, eps, divs)
    lo = np.array([box[0] - 100 * e, box[1] - 100 * e, -0.5 * e])
    hi = np.array([box[0] - 6 * e, box[1] - 6 * e, 0.5 * e])
    sites = lattice_sites(rng, lo, hi, 6 * e)
    S, Q, intent, steps, worst = face_probes(rng, eps, geoms, sites, box, pure_axis=True)
    # (the lattice translations stay in the plane: a z offset of 2^-10 would be larger than the probes' own z and cost them float digits)
    designed = [(R, t * np.array([1, 1, 0])) for R, t in DESIGNED]
    return assemble(name, eps, rng, box, S, Q, intent, designed=designed, divs=divs, partner_steps=steps, general=False,
                    worst_face_offsets=np.asarray(worst))


def _sort_threshold(above, seed=12):
    """Lone points whose (cell, point) incidences at cell edge eps add up to just below / just above 65 536 -- the size from which the
    build sorts them with the library's own sort.  The count is restated on the CPU (grid_ref.incidences)."""
    rng = np.random.default_rng(seed)
    eps = EPS_DEFAULT
    e = float(eps)
    box = np.array([70.0, 70.0, 24.0]) * e
    g1 = box_geoms(box, eps, (1,))[1]
    lone = np.asarray(lattice_sites(rng, 4 * e * np.ones(3), box - 4 * e, 3.2 * e)[:1800])
    full = mirror(np.concatenate([[box], lone]))
    cum = np.cumsum(ref.incidences(full, g1)["per_point"])
    n_lo = int(np.searchsorted(cum, 65536, side="left"))          # the first n_lo points stay below
    n_lo -= n_lo % 2
    n = n_lo if not above else n_lo + 2 * (1 + int(cum[n_lo + 1] < 65536))
    assert n_lo > 1000 and (cum[n - 1] >= 65536) == above and abs(int(cum[n - 1]) - 65536) < 200, (n_lo, cum[n - 1])
    half = lone[: n // 2 - 1]
    Q = shell_queries(rng, half, eps, 300)
    return assemble("sort_above" if above else "sort_below", eps, rng, box, half, Q, divs=(1,), general=False, n_incidences_div1=int(cum[n - 1]))


BUILDERS = {
    "faces": lambda: _faces("faces", EPS_DEFAULT, 1),
    "faces_pow2": lambda: _faces("faces_pow2", EPS_POW2, 2),
    "radius": lambda: _radius("radius", EPS_DEFAULT, 13),
    "radius_pow2": lambda: _radius("radius_pow2", EPS_POW2, 14),
    "ties": _ties,
    "lists": lambda: _lists(False),
    "lists_sparse": lambda: _lists(True),
    "one_point": _one_point,
    "two_points": _two_points,
    "collinear": _collinear,
    "planar": _planar,
    "one_cell": _one_cell,
    "two_clusters": _two_clusters,
    "extent_500": lambda: _extent("extent_500", 500, (1, 2, 3, 4), 20),
    "extent_4000": lambda: _extent("extent_4000", 4000, (1, 2, 4), 21),
    "extent_max": lambda: _extent("extent_max", extent_ratio_max(), (1,), 22),
    "extent_rod": lambda: _extent("extent_rod", 2 ** 18, (1, 2, 4), 23, rod=True),
    "sort_below": lambda: _sort_threshold(False),
    "sort_above": lambda: _sort_threshold(True),
}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def build(name):
    return BUILDERS[name]()


def coincident(n, eps=EPS_DEFAULT):
    """n coincident scene points (the centred scene is n copies of the origin) and a small model around them."""
    rng = np.random.default_rng(30)
    spos = np.tile(np.array([[0.25, 0.5, 0.75]], F), (n, 1))        # sums of these stay exact in float up to 2^16 terms
    Q = shell_queries(rng, np.zeros((1, 3)), eps, 32, 0.2, 1.8)
    case = assemble("coincident_%d" % n, eps, rng, np.zeros(3), np.zeros((0, 3)), Q, general=False)
    nS = n
    snrm = np.zeros((nS, 3), F); snrm[:, 2] = 1
    case.update(spos=spos, snrm=snrm, sprob=rng.uniform(0.2, 1.0, nS).astype(F),
                spix=np.stack([np.arange(nS) // 640, np.arange(nS) % 640], 1).astype(np.int32), box=None)
    return case
