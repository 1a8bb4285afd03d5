#!/usr/bin/env python3
"""Census (CPU only) of the sub-patch walk of lcp_coopq_kernel's SPLIT, CU = 16 forms: what the mapping of live sub-patches to the four
wavefronts of a candidate costs, per pose, under the per-wave rings (wave w owns the 64-point steps w, w + 4, ... and walks the live
sub-patches of those) and under one workgroup-wide list dealt round-robin (step s = entries 4s .. 4s + 3 -> wave s & 3):
  * wave-steps of the whole candidate and of its LONGEST wave (the workgroup lives as long as that one),
  * partial steps (fewer than four sub-patches),
  * patch-test windows (64 sub-patches per ballot), in all and on the longest wave.
The model order and the sub-patch spheres are the library's own (stocs_model_patch_order / stocs_model_subpatches: host code, no device);
the scene's distance field is restated from grid.hip (prepare_cull_field, dist_splat_kernel: cell = epsilon, value = distance from the
cell centre to the nearest scene point, shortened by its rounding margin, capped) with a kd-tree, and lcp_patch_dead from lcp.hip in
float64.  It is an upper bound of what the walk can gain: the verify trips (process) are not counted.
usage: python tools/walk_census.py [Cm|C5|small] [poses]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("STOCS_PIN_BLAS", "1")
from model_matching_amd import capi, synth  # noqa: E402
from scipy.spatial import cKDTree  # noqa: E402

EPS = 0.005


def library_subpatches(pos):
    """the walk order, the 64-point patch spheres and the 16-point sub-patch spheres as the context computes them"""
    L = capi.load()
    n = len(pos)
    pos = np.ascontiguousarray(pos, np.float32)
    perm = np.zeros(n, np.int32); pat = np.zeros(((n + 63) // 64, 4), np.float32); sub = np.zeros(((n + 15) // 16, 4), np.float32)
    assert L.stocs_model_patch_order(pos.ctypes.data_as(capi._fp), n, perm.ctypes.data_as(capi._ip), pat.ctypes.data_as(capi._fp)) == 0
    assert L.stocs_model_subpatches(pos.ctypes.data_as(capi._fp), n, perm.ctypes.data_as(capi._ip), sub.ctypes.data_as(capi._fp)) == 0
    return perm, pat.astype(np.float64), sub.astype(np.float64)


class Field:
    """SceneGrid::d_dist restated: values are looked up lazily, per cell, from a kd-tree of the centred scene"""

    def __init__(self, sp, patch_radii):
        r = np.sort(patch_radii)
        r_ref = r[int((len(r) - 1) * 0.8)]
        self.g = EPS
        self.cap = min(r_ref, 8.0 * EPS) + EPS + self.g
        self.o = sp.min(0) - self.cap - self.g
        self.n = np.floor((sp.max(0) + self.cap + self.g - self.o) / self.g).astype(np.int64) + 1
        self.tree = cKDTree(sp)
        self.cache = {}

    def values(self, cells):
        keys = (cells[:, 2] * self.n[1] + cells[:, 1]) * self.n[0] + cells[:, 0]
        new = np.array([k for k in np.unique(keys) if k not in self.cache], np.int64)
        if len(new):
            c = np.stack([new % self.n[0], (new // self.n[0]) % self.n[1], new // (self.n[0] * self.n[1])], axis=1)
            d, _ = self.tree.query(self.o + (c + 0.5) * self.g, distance_upper_bound=self.cap)
            v = np.where(np.isfinite(d), np.maximum(d * (1.0 - 2.0e-6) - 1.0e-6, 0.0), self.cap)
            self.cache.update(zip(new.tolist(), np.minimum(v, self.cap).tolist()))
        return np.array([self.cache[k] for k in keys.tolist()])


def patch_dead(F, spheres, A, t):
    """lcp_patch_dead for every sphere under x -> A x + t"""
    G = A.T @ A
    ag = np.abs(G)
    rho = max(G[0, 0] + ag[0, 1] + ag[0, 2], G[1, 1] + ag[0, 1] + ag[1, 2], G[2, 2] + ag[0, 2] + ag[1, 2])
    sn = np.sqrt(rho) * 1.00001
    c = spheres[:, :3] @ A.T + t
    mag = np.abs(c).sum(1)
    need = (sn * spheres[:, 3] + EPS * 1.002) + (4.0e-6 + 4.0e-6 * mag)
    f = np.floor((c - F.o) / F.g)
    inside = np.all((f >= 1) & (f < F.n - 1), axis=1)
    dead = np.full(len(spheres), F.cap) > need
    if inside.any():
        fi = f[inside].astype(np.int64)
        e = np.linalg.norm(c[inside] - (F.o + (fi + 0.5) * F.g), axis=1)
        dead[inside] = F.values(fi) - e > need[inside]
    return dead & (mag < 1.0e18)


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "Cm"
    nposes = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    m, s, k = synth.workload(name)
    cs = s.pos.astype(np.float64).mean(0); cm = m.pos.astype(np.float64).mean(0)
    sp = (s.pos - cs.astype(np.float32)).astype(np.float64)
    T = synth.make_candidates(synth.centred_gt(s.T_gt, cs, cm), k)      # the bench batch (rank 0's seed)
    perm, pat, sub = library_subpatches(m.pos)
    M = len(m.pos); nsteps = (M + 63) // 64; nsub = (M + 15) // 16
    F = Field(sp, pat[:, 3])
    owner = (np.arange(nsub) >> 2) & 3                                  # today: wave w owns steps w, w + 4, ...
    sel = np.random.default_rng(0).choice(k, nposes, replace=False)
    rows = []
    for ci in sel:
        Mx = T[ci].reshape(4, 4).T.astype(np.float64)
        live = ~patch_dead(F, sub, Mx[:3, :3], Mx[:3, 3])
        Lw = np.array([live[owner == w].sum() for w in range(4)])
        L = int(live.sum())
        steps_now = (Lw + 3) // 4
        steps_new = (L + 3) // 4
        rows.append((L, steps_now.sum(), steps_now.max(), int((Lw % 4 != 0).sum()), steps_new, (steps_new + 3) // 4, int(L % 4 != 0)))
    r = np.array(rows, np.float64)
    win_now = [(4 * ((nsteps - w + 3) // 4) + 63) // 64 for w in range(4)]
    win_new = (nsub + 63) // 64
    print("# tools/walk_census.py %s %d: %d model points, %d steps, %d sub-patches; field cell %.1f mm, cap %.1f mm" %
          (name, nposes, M, nsteps, nsub, F.g * 1e3, F.cap * 1e3))
    print("live sub-patches per pose           mean %.1f  min %d  max %d" % (r[:, 0].mean(), r[:, 0].min(), r[:, 0].max()))
    print("wave-steps per pose                 per-wave rings %.2f   shared list %.2f" % (r[:, 1].mean(), r[:, 4].mean()))
    print("steps of the longest wave           per-wave rings %.2f   shared list %.2f   (ratio %.3f)" %
          (r[:, 2].mean(), r[:, 5].mean(), r[:, 5].mean() / r[:, 2].mean()))
    print("  longest wave - mean wave (rings)  mean %.2f steps, max %.2f" % ((r[:, 2] - r[:, 1] / 4).mean(), (r[:, 2] - r[:, 1] / 4).max()))
    print("partial steps per pose              per-wave rings %.2f   shared list %.2f" % (r[:, 3].mean(), r[:, 6].mean()))
    print("patch-test windows per pose         per-wave rings %d (longest wave %d)   shared list %d (longest wave %d)" %
          (sum(win_now), max(win_now), win_new, (win_new + 3) // 4))


if __name__ == "__main__":
    main()
