#!/usr/bin/env python3
"""Census (CPU only) of a normal-cone test on the 16-point sub-patches of lcp_coopq_kernel's shared-list forms: of the sub-patches
that the sphere test (lcp_patch_dead) leaves alive, how many could be ruled out because NO scene normal near them can pass the
normal test against ANY of their rotated model normals -- before they are walked, looked up and gated point by point.
  model side   per sub-patch the cone of its normals: axis a_m = the normalised mean, kept as float32, half-angle beta = the largest
               angle of a member against that float axis (float64); no test above 45 degrees
  scene side   per cell of the patch test's field (cell = epsilon, the same cells as SceneGrid::d_dist) the cone of the normals of
               every scene point within a reach R of the cell's centre: axis = the normalised sum, half-angle delta = the largest
               deviation.  Two codings: "fine" (axis as it is, sin(delta + 0.5 degrees) rounded up to 1/256) and "cell word" (the
               coding of normal_cone.h: octahedral axis of 6 bits a coordinate, sin(delta) rounded up to 1/16, the deviation
               measured against the axis as decoded)
  the test     a live sub-patch with sphere (c, r) under x -> A x + t lands in the cell of A c + t, e = |A c + t - cell centre|.
               It can be tested when s r + epsilon + e <= R (s = linear_norm_bound of A: every scene point that a point of the
               sub-patch can have within epsilon is then inside the reach).  With X the support of the scene cone at v = A a_m
               (the `bound` of cone_rules_out) every (A n_m) . n_s <= X cos(beta) + s sin(beta); below dot_lo it is ruled out.
The model order and the sub-patch spheres are the library's own (stocs_model_subpatches: host code, no device), the field is
restated from grid.hip as in tools/walk_census.py, which this census shares its Field and patch_dead with.  The truth -- which
sub-patches hold a COUNTED point: nearest scene point within epsilon, normals within lcp_normal_angle -- comes from a kd-tree in
float64, so a sub-patch "wrongly ruled out" is one that is ruled out and holds a counted point (must be 0).
"ideal" is the same bound with the cone of the exact ball of radius s r + epsilon around A c + t instead of a cell's reach.
usage: python tools/patch_normal_census.py [Cm|Cm_asym|small] [poses]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("STOCS_PIN_BLAS", "1")
from model_matching_amd import synth  # noqa: E402
from walk_census import EPS, Field, library_subpatches, patch_dead  # noqa: E402

DOT_LO = float(np.cos(np.deg2rad(30.0)))
BETA_MAX = np.deg2rad(45.0)
NO_CONE_SIN = 15.0 / 16.0     # wider cones: class "no cone" (normal_cone.h keeps the same limit)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def model_cones(nrm_sorted, nsub):
    """(axis float32 -> float64, beta) per sub-patch from the exact normals in patch order"""
    ax = np.zeros((nsub, 3)); beta = np.zeros(nsub)
    for q in range(nsub):
        n = nrm_sorted[16 * q:16 * q + 16]
        a = unit(n.sum(0)).astype(np.float32).astype(np.float64)
        ax[q] = a
        beta[q] = np.arccos(np.clip((n @ a) / np.linalg.norm(a), -1.0, 1.0)).max()
    return ax, beta


def oct_decode(u, v):
    x = u * (2.0 / 63.0) - 1.0; y = v * (2.0 / 63.0) - 1.0
    z = 1.0 - abs(x) - abs(y)
    t = max(-z, 0.0)
    x += -t if x >= 0 else t
    y += -t if y >= 0 else t
    return np.array([x, y, z])


def oct_encode(a):
    a = a / np.abs(a).sum()
    x, y = a[0], a[1]
    if a[2] < 0:
        x, y = (1 - abs(a[1])) * (1 if a[0] >= 0 else -1), (1 - abs(a[0])) * (1 if a[1] >= 0 else -1)
    return int(np.clip(np.rint((x + 1) * 31.5), 0, 63)), int(np.clip(np.rint((y + 1) * 31.5), 0, 63))


class ConeField:
    """per cell of F and reach R: (axis, sin delta) under both codings, computed lazily; sin delta = 2: no cone"""

    def __init__(self, F, sp, sn, R):
        self.F, self.sp, self.sn, self.R = F, sp, sn, R
        self.cache = {}

    def cell(self, c):
        key = (int(c[0]), int(c[1]), int(c[2]))
        if key not in self.cache:
            ctr = self.F.o + (np.asarray(c) + 0.5) * self.F.g
            idx = self.F.tree.query_ball_point(ctr, self.R)
            self.cache[key] = self.cone(self.sn[idx]) if len(idx) else None   # None: nothing within reach -- everything is ruled out
        return self.cache[key]

    @staticmethod
    def cone(n):
        s = n.sum(0)
        if not np.linalg.norm(s) > 1e-6:
            return (np.zeros(3), 2.0, np.zeros(3), 2.0)
        a = unit(s)
        d = np.arccos(np.clip(n @ a, -1.0, 1.0)).max()
        sf = np.ceil(np.sin(min(d + np.deg2rad(0.5), np.pi / 2)) * 256.0) / 256.0
        fine = (a, sf if (d + np.deg2rad(0.5) < np.pi / 2 and sf <= NO_CONE_SIN) else 2.0)
        ac = unit(oct_decode(*oct_encode(a)))
        dc = np.arccos(np.clip(n @ ac, -1.0, 1.0)).max()
        sc = np.ceil(np.sin(min(dc, np.pi / 2)) * 16.0) / 16.0
        coarse = (ac, sc if (dc < np.pi / 2 and sc <= NO_CONE_SIN) else 2.0)
        return fine + coarse


def support(v, a, sd):
    """max v . n over unit n within asin(sd) of the unit axis a"""
    va = v @ a
    vp = np.sqrt(max(v @ v - va * va, 0.0))
    cd = np.sqrt(1.0 - sd * sd)
    return np.linalg.norm(v) if vp * cd <= va * sd else va * cd + vp * sd


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "Cm"
    nposes = int(sys.argv[2]) if len(sys.argv) > 2 else 96
    m, s, k = synth.workload(name)
    cs = s.pos.astype(np.float64).mean(0); cm = m.pos.astype(np.float64).mean(0)
    sp = (s.pos - cs.astype(np.float32)).astype(np.float64)
    sn = unit(s.nrm.astype(np.float64))
    T = synth.make_candidates(synth.centred_gt(s.T_gt, cs, cm), k)
    perm, pat, sub = library_subpatches(m.pos)
    M = len(m.pos); nsub = (M + 15) // 16
    mp = (m.pos - m.pos.mean(0, dtype=np.float32))[perm].astype(np.float64)
    mn = unit(m.nrm.astype(np.float64))[perm]
    ax_m, beta = model_cones(mn, nsub)
    F = Field(sp, pat[:, 3])
    rs = np.sort(sub[:, 3])
    q = lambda f: rs[int((len(rs) - 1) * f)]
    half_diag = 0.5 * np.sqrt(3.0) * F.g
    rules = [("20 mm", 0.020)] + [("q%02d" % int(100 * f), q(f) + EPS + half_diag) for f in (0.5, 0.65, 0.8, 0.9, 0.95, 1.0)]
    print("# tools/patch_normal_census.py %s %d: %d model points, %d sub-patches; field cell %.1f mm; %d scene points" %
          (name, nposes, M, nsub, F.g * 1e3, len(sp)))
    print("sub-patch radius mm: median %.2f  q80 %.2f  q90 %.2f  q95 %.2f  max %.2f" % tuple(1e3 * np.array([q(.5), q(.8), q(.9), q(.95), q(1.0)])))
    bd = np.rad2deg(beta)
    print("model cone half-angle beta, degrees: median %.1f  q90 %.1f  max %.1f; above 45: %d of %d" % (np.median(bd), np.sort(bd)[int(.9 * (nsub - 1))], bd.max(), int((beta > BETA_MAX).sum()), nsub))
    sel = np.random.default_rng(0).choice(k, nposes, replace=False)
    fields = [ConeField(F, sp, sn, R) for _, R in rules]
    # counters per rule: [ruled out fine, wrong fine, ruled out cell word, wrong cell word, not testable]
    cnt = np.zeros((len(rules), 5)); live_total = 0; empty_total = 0; ideal = 0; ideal_wrong = 0; pts_nb = 0; pts_cnt = 0; pts_in_ruled = np.zeros(len(rules))
    for ci in sel:
        Mx = T[ci].reshape(4, 4).T.astype(np.float64)
        A, t = Mx[:3, :3], Mx[:3, 3]
        G = A.T @ A; ag = np.abs(G)
        sn_b = np.sqrt(max(G[0, 0] + ag[0, 1] + ag[0, 2], G[1, 1] + ag[0, 1] + ag[1, 2], G[2, 2] + ag[0, 2] + ag[1, 2])) * 1.00001
        live = ~patch_dead(F, sub, A, t)
        # the truth: counted points
        x = mp @ A.T + t
        d, j = F.tree.query(x, distance_upper_bound=EPS)
        has = np.isfinite(d)
        dots = np.zeros(M); dots[has] = np.einsum("ij,ij->i", mn[has] @ A.T, sn[j[has]])
        counted = has & (dots >= DOT_LO)
        pts_nb += has.sum(); pts_cnt += counted.sum()
        sub_counted = np.array([counted[16 * q_:16 * q_ + 16].any() for q_ in range(nsub)])
        sub_nb = np.array([has[16 * q_:16 * q_ + 16].sum() for q_ in range(nsub)])
        assert not (sub_counted & ~live).any(), "the sphere test itself ruled out a counted point"
        c = sub[:, :3] @ A.T + t
        f = np.floor((c - F.o) / F.g).astype(np.int64)
        e = np.linalg.norm(c - (F.o + (f + 0.5) * F.g), axis=1)
        for q_ in np.nonzero(live)[0]:
            live_total += 1
            empty_total += not sub_counted[q_]
            v = A @ ax_m[q_]
            testable_m = beta[q_] <= BETA_MAX
            # ideal: the normals of the exact ball
            idx = F.tree.query_ball_point(c[q_], sn_b * sub[q_, 3] + EPS)
            if testable_m:
                if not len(idx):
                    ideal += 1; ideal_wrong += sub_counted[q_]
                else:
                    co = ConeField.cone(sn[idx])
                    if co[1] < 2.0 and support(v, co[0], co[1]) * np.cos(beta[q_]) + sn_b * np.sin(beta[q_]) < DOT_LO:
                        ideal += 1; ideal_wrong += sub_counted[q_]
            for ri, (_, R) in enumerate(rules):
                if not testable_m or sn_b * sub[q_, 3] + EPS + e[q_] + 1e-5 > R:
                    cnt[ri, 4] += 1
                    continue
                co = fields[ri].cell(f[q_])
                for kk in range(2):
                    out = co is None or (co[2 * kk + 1] < 2.0 and support(v, co[2 * kk], co[2 * kk + 1]) * np.cos(beta[q_]) + sn_b * np.sin(beta[q_]) < DOT_LO)
                    if out:
                        cnt[ri, 2 * kk] += 1; cnt[ri, 2 * kk + 1] += sub_counted[q_]
                        if kk == 0: pts_in_ruled[ri] += sub_nb[q_]
    n = float(nposes)
    print("live sub-patches per pose %.1f; without a counted point %.1f %%; points with a neighbour %.0f, counted %.0f per pose" %
          (live_total / n, 100.0 * empty_total / live_total, pts_nb / n, pts_cnt / n))
    print("ideal (exact ball of radius s r + eps, cone of its normals): ruled out %.1f %% of live, wrongly %d" % (100.0 * ideal / live_total, ideal_wrong))
    print("%-6s %8s | %-22s | %-22s | %s" % ("reach", "R mm", "fine: out %, wrong", "cell word: out %, wrong", "not testable %, neighbours in ruled-out %"))
    for ri, (nm, R) in enumerate(rules):
        print("%-6s %8.2f | %10.1f %10d | %10.1f %10d | %10.1f %10.1f" % (nm, R * 1e3, 100.0 * cnt[ri, 0] / live_total, cnt[ri, 1], 100.0 * cnt[ri, 2] / live_total, cnt[ri, 3],
                                                                 100.0 * cnt[ri, 4] / live_total, 100.0 * pts_in_ruled[ri] / max(pts_nb, 1)))


if __name__ == "__main__":
    main()
