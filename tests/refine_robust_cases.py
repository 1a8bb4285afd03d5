"""Seeded cases of the robust refinement's select and gate (csrc/refine_robust.h), built so that every rank word is known bit for bit.

Construction: the model is a dyadic lattice of step 4 d (d = 2^-5, the correspondence distance), so a source point placed at a small
dyadic offset (dx along one axis, dy along another) from a lattice point has that point as its only neighbour, and its float squared
distance fma(dz, dz, fma(dy, dy, dx dx)) = dx^2 + dy^2 is exact: the rank word is float32(dx^2 + dy^2)'s bit pattern.  Scenes are
point-symmetric in adjacent pairs (p, -p): both centroids are exactly 0 and the hypothesis is [I | 0].  A pair shares its level, so
every level holds an even number of scene points; odd counts come from src_idx."""
import numpy as np

from oracle import refine_oracle as ro

F = np.float32
D = 2.0 ** -5
NOT_CANDIDATE = 0xFFFFFFFF
FAR = "far"          # 2 d from the lattice point: no match
BEYOND = "beyond"    # one float past d: found by the walk, fails the double test -- a match that is no candidate

# offsets (dx, dy) whose words differ in ONE byte only, per byte 3 (top) .. 0
BYTE_PAIRS = {3: ((2.0 ** -6, 0.0), (2.0 ** -7, 0.0)),
              2: ((2.0 ** -6, 0.0), (1.125 * 2.0 ** -6, 0.0)),
              1: ((2.0 ** -6, 2.0 ** -10), (2.0 ** -6, 2.0 ** -11)),
              0: ((2.0 ** -6, 2.0 ** -14), (2.0 ** -6, 2.0 ** -15))}
COINCIDENT = (0.0, 0.0)      # word 0
AT_THRESHOLD = (D, 0.0)      # d^2 == (double)d (double)d: the largest word that is still a candidate


def word_of(off):
    """the rank word of an offset: exact by construction"""
    v = off[0] * off[0] + off[1] * off[1]
    assert float(F(v)) == v, off
    return int(np.array([v], F).view(np.uint32)[0])


class RCase(ro.Case):
    """ro.Case with scene normals of its own, the expected rank word per scene point and the level of each scene point"""

    def __init__(self, *a, scene_nrm=None, words=None, level=None, **kw):
        super().__init__(*a, **kw)
        n = len(self.scene)
        self.scene_nrm = np.tile(np.array([0.0, 0.0, 1.0], F), (n, 1)) if scene_nrm is None else np.ascontiguousarray(scene_nrm, F)
        self.words = None if words is None else np.asarray(words, np.uint32)
        self.level = None if level is None else np.asarray(level, np.int64)

    def estimator_inputs(self):
        sp, _, pr, px, mp, mn = super().estimator_inputs()
        return sp, self.scene_nrm, pr, px, mp, mn

    def source_words(self):
        return self.words if self.src_idx is None else self.words[self.src_idx]


def built(name, offsets, seed=0, src_idx=None, model_nrm=None, scene_nrm_fn=None, family="cut"):
    """offsets: one entry per scene PAIR -- (dx, dy), FAR or BEYOND.  Scene points 2 i and 2 i + 1 are the pair of entry i."""
    rng = np.random.default_rng(1000 + seed)
    lat = ro._lattice(1, 4 * D)
    model = lat[rng.permutation(len(lat))]
    P, words, level = [], [], []
    levels = {}
    for off in offsets:
        L = lat[rng.integers(0, len(lat))]
        a = int(rng.integers(0, 3)); b = (a + 1 + int(rng.integers(0, 2))) % 3
        sa, sb = rng.choice([-1.0, 1.0], 2)
        p = L.copy()
        if off == FAR:
            p[a] += sa * 2 * D; w = NOT_CANDIDATE
        elif off == BEYOND:
            p[a] = float(np.nextafter(F(L[a] + sa * D), F(sa * np.inf))); w = NOT_CANDIDATE
        else:
            p[a] += sa * off[0]; p[b] += sb * off[1]; w = word_of(off)
        assert np.array_equal(p.astype(F).astype(np.float64), p)
        P.append(p); words += [w, w]
        lv = levels.setdefault(w, len(levels)); level += [lv, lv]
    scene = ro._sym(np.array(P), pairs=True)
    nrm = None if scene_nrm_fn is None else scene_nrm_fn(rng, len(scene))
    return RCase(family, name, model, scene, D, model_nrm=model_nrm, src_idx=src_idx, seed=seed, scene_nrm=nrm, words=words, level=level)


def _shuffled(rng, groups):
    out = [o for o, n in groups for _ in range(n)]
    return [out[i] for i in rng.permutation(len(out))]


def one_level(seed=1):
    """every candidate at one distance: the cut is by position alone"""
    rng = np.random.default_rng(seed)
    return built("one_level", _shuffled(rng, [((2.0 ** -7, 0.0), 60), (FAR, 20), (BEYOND, 10)]), seed)


NEAR_PAIRS, FAR_PAIRS = 40, 50


def two_levels(seed=2):
    rng = np.random.default_rng(seed)
    return built("two_levels", _shuffled(rng, [((2.0 ** -7, 0.0), NEAR_PAIRS), ((2.0 ** -6, 0.0), FAR_PAIRS), (FAR, 15), (BEYOND, 5)]), seed)


def two_levels_ks():
    """cut between the levels, inside the nearer tie group, inside the farther one, and at the very ends"""
    na, nb = 2 * NEAR_PAIRS, 2 * FAR_PAIRS
    return [na, na // 2, na - 1, na + 1, na + nb // 2, na + nb - 1, na + nb, 1]


def byte_levels(seed=3):
    """all eight offsets of BYTE_PAIRS, distance 0 and the threshold itself, four pairs each, shuffled"""
    rng = np.random.default_rng(seed)
    offs = sorted({o for pair in BYTE_PAIRS.values() for o in pair} | {COINCIDENT, AT_THRESHOLD})
    return built("byte_levels", _shuffled(rng, [(o, 4) for o in offs] + [(FAR, 6), (BEYOND, 6)]), seed)


def few_candidates():
    """n_cand = 0 .. 7 through src_idx over one scene: j candidates (distinct levels and a repeated one) among non-candidates"""
    base = two_levels(seed=4)
    w = base.words
    cand = np.nonzero(w != NOT_CANDIDATE)[0]
    non = np.nonzero(w == NOT_CANDIDATE)[0]
    rng = np.random.default_rng(44)
    out = []
    for j in range(8):
        idx = np.concatenate([rng.choice(cand, j, replace=False), rng.choice(non, 9, replace=False)]).astype(np.int32)
        idx = idx[rng.permutation(len(idx))]
        out.append(RCase("cut", "n_cand_%d" % j, base.model, base.scene, D, model_nrm=base.model_nrm, src_idx=idx, seed=4, words=base.words, level=base.level))
    return out


SIZES = (1, 255, 256, 257, 1025)


def source_sizes():
    base = two_levels(seed=5)
    rng = np.random.default_rng(55)
    return [RCase("cut", "n_src_%d" % n, base.model, base.scene, D, model_nrm=base.model_nrm, src_idx=rng.integers(0, len(base.scene), n).astype(np.int32), seed=5,
                  words=base.words, level=base.level) for n in SIZES]


def last_chunk():
    """600 source positions, every candidate among the last 88 (the third chunk of 256)"""
    base = two_levels(seed=6)
    rng = np.random.default_rng(66)
    cand = np.nonzero(base.words != NOT_CANDIDATE)[0]
    non = np.nonzero(base.words == NOT_CANDIDATE)[0]
    idx = np.concatenate([rng.choice(non, 512), rng.choice(cand, 88)]).astype(np.int32)
    return RCase("cut", "last_chunk", base.model, base.scene, D, model_nrm=base.model_nrm, src_idx=idx, seed=6, words=base.words, level=base.level)


def repeated_point():
    """src_idx names one candidate scene point twice (positions 3 and 40) among distinct others: equal words, the lower position first"""
    base = one_level(seed=7)
    cand = np.nonzero(base.words != NOT_CANDIDATE)[0]
    idx = np.concatenate([cand[:3], cand[10:11], cand[3:10], cand[11:40], cand[10:11], cand[40:60]]).astype(np.int32)
    c = RCase("cut", "repeated_point", base.model, base.scene, D, model_nrm=base.model_nrm, src_idx=idx, seed=7, words=base.words, level=base.level)
    c.twice = (3, 40)
    return c


def cut_cases():
    return [one_level(), two_levels(), byte_levels()] + few_candidates() + source_sizes() + [last_chunk(), repeated_point()]


def ks_for(case):
    """the kept counts a case is cut at"""
    n_cand = int((case.source_words() != NOT_CANDIDATE).sum())
    if case.name == "two_levels":
        ks = two_levels_ks()
    elif case.name == "byte_levels":
        ks = list(range(1, n_cand + 1, 3)) + [n_cand]
    else:
        ks = [n_cand, (3 * n_cand) // 4, n_cand // 2, 6, 5, 1]
    return sorted({k for k in ks if 1 <= k <= n_cand})


# ---------------------------------------------------------------- the gate
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)


def gate_exact(seed=8):
    """axis-aligned model and scene normals under [I | 0]: c is exactly -1, 0 or 1"""
    rng = np.random.default_rng(seed)
    mn = AXES[rng.integers(0, 6, 27)]
    return built("axis_normals", _shuffled(rng, [((2.0 ** -7, 0.0), 50), ((2.0 ** -6, 2.0 ** -10), 50), (FAR, 10), (BEYOND, 10)]), seed, model_nrm=mn,
                 scene_nrm_fn=lambda r, n: AXES[r.integers(0, 6, n)], family="gate")


GATE_MIN_COS = (-1.0, 0.0, 1.0)


def gate_random(seed=15):
    """oracle/refine_oracle.py's random surface cloud (2 500 x 4 000, 3.5 cm) with seeded unit scene normals"""
    base = next(c for c in ro.random_clouds() if c.id == "random_surface-2500_0.035")
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(len(base.scene), 3))
    return RCase("gate", "random_surface", base.model, base.scene, base.dist, model_nrm=base.model_nrm, T16=base.T16, exact=False, seed=15,
                 scene_nrm=v / np.linalg.norm(v, axis=1)[:, None])


# ---------------------------------------------------------------- the end-to-end hypotheses
TABLE_SEED = 5


def table_hypotheses(Tgt, n=6, seed=TABLE_SEED, max_deg=2.0, move=0.004):
    """n centred hypotheses: the ground truth turned by up to max_deg about a random axis (about the model origin) and moved by
    `move` in a random direction -> (n, 16) float32, column-major"""
    from model_matching_amd.synth import _rot_axis_angle
    rng = np.random.default_rng(seed)
    T0 = np.asarray(Tgt, np.float64)
    out = np.zeros((n, 16), F)
    for i in range(n):
        dR = _rot_axis_angle(rng.normal(size=3), np.deg2rad(max_deg) * rng.uniform(0, 1))
        d = rng.normal(size=3)
        T = np.eye(4)
        T[:3, :3] = T0[:3, :3] @ dR
        T[:3, 3] = T0[:3, 3] + d / np.linalg.norm(d) * move
        out[i] = T.T.reshape(16).astype(F)
    return out
