#!/usr/bin/env python3
"""CPU census of the octant lines of the scene grid (model_matching_amd/csrc/octant_lists.h, grid.hip): how long the list is that a
query reads, today and with one line per octant.

A restatement in float64, no GPU: the grid of grid.hip at cell edge epsilon (float origin, every scene point within r of the cell box
in the cell's dilated list, 4x4x4 sub-cell masks from tools/gate_census.py), the dominance pruning over the widened cell box (8
dominators nearest to the centre, the library's slack and margin) for the stored lists, and per octant of a cell the same pruning of
the stored list over the widened octant box (entries within r of the octant box, 8 dominators nearest to the octant's centre).  The
lists counted are those of the queries that pass the sub-cell mask, over the first poses of bench.py's batch.  Rows: today's lists;
octant lists in every cell; what the library builds (a block of eight lines of 8 entries for a cell that keeps more than 8 entries
and whose eight octants each keep at most 8, today's list elsewhere).  The cell counts can be held against stocs_get_grid_octants.

usage: python tools/octant_census.py [--poses 16] [--workloads Cm,small]   (prints a markdown table)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from model_matching_amd import synth  # noqa: E402

K = 8


def incidences(spos, eps):
    """the dilated lists: (o, h, r, n, ukey, first, pts) -- pts sorted by cell key, then scene index; and the sub-cell masks"""
    h = eps
    ext = float((spos.max(0).astype(np.float64) - spos.min(0).astype(np.float64)).max())
    r0 = eps * 1.001
    span = ext + 2.0 * (r0 + 2 * h) + h
    r = max(r0, eps + span / 2097152.0)
    pad = r + 2 * h
    o = (spos.min(0).astype(np.float64) - pad).astype(np.float32).astype(np.float64)
    n = np.floor((spos.max(0).astype(np.float64) + pad - (spos.min(0).astype(np.float64) - pad)) / h).astype(np.int64) + 1
    p = spos.astype(np.float64)
    lo = np.maximum(np.floor((p - r - o) / h).astype(np.int64), 0)
    pts, cells3 = [], []
    for dz in range(4):
        for dy in range(4):
            for dx in range(4):
                c = lo + np.array([dx, dy, dz])
                b0 = o + c * h
                d = np.maximum(np.maximum(b0 - p, p - (b0 + h)), 0.0)
                ok = ((d * d).sum(1) <= r * r) & (c < n).all(1) & (c <= np.floor((p + r - o) / h).astype(np.int64)).all(1)
                pts.append(np.nonzero(ok)[0]); cells3.append(c[ok])
    pts = np.concatenate(pts); cells3 = np.concatenate(cells3)
    key = (cells3[:, 2] * n[1] + cells3[:, 1]) * n[0] + cells3[:, 0]
    order = np.lexsort((pts, key))
    pts, key, cells3 = pts[order], key[order], cells3[order]
    ukey, first = np.unique(key, return_index=True)
    cell_of = np.searchsorted(ukey, key)
    mask = np.zeros(len(ukey), np.uint64)
    hs = h / 4.0
    for s in range(64):
        sc = 4 * cells3 + np.array([s & 3, (s >> 2) & 3, s >> 4])
        b0 = o + sc * hs
        d = np.maximum(np.maximum(b0 - p[pts], p[pts] - (b0 + hs)), 0.0)
        got = np.zeros(len(ukey), bool)
        got[cell_of[(d * d).sum(1) <= r * r]] = True
        mask |= got.astype(np.uint64) << np.uint64(s)
    return dict(o=o, h=h, r=r, n=n, ukey=ukey, first=first, pts=pts, cells3=cells3[first], mask=mask)


def prune(u, hw, margin):
    """u: (m, 3) positions relative to the box centre, in list order -> the kept rows (a boolean mask)"""
    n2 = (u * u).sum(1)
    order = np.lexsort((np.arange(len(u)), n2.astype(np.float32)))[:K]      # nearest to the centre: float distance, then position
    du, dn2 = u[order], n2[order]
    l1 = np.abs(u[:, None, :] - du[None, :, :]).sum(2)
    fmin = (n2[:, None] - dn2[None, :]) - 2.0 * hw * l1
    return ~(fmin > margin).any(1)


def build(spos, eps):
    g = incidences(spos, eps)
    h, r, o = g["h"], g["r"], g["o"]
    ext = float((g["n"] * h).max())
    hh = 0.5 * h + 2.0e-6 * (ext + 1.0) * 0.5 + 1.0e-7
    margin = 4.0e-6 * (r + 2.0 * h) ** 2
    hw = 0.25 * h + (hh - 0.5 * h)
    p = spos.astype(np.float64)
    nc = len(g["ukey"])
    bounds = np.append(g["first"], len(g["pts"]))
    kept = np.zeros(nc, np.int64)
    oct_kept = np.zeros((nc, 8), np.int64)
    for c in range(nc):
        idx = g["pts"][bounds[c]:bounds[c + 1]]
        ctr = o + (g["cells3"][c] + 0.5) * h
        q = p[idx]
        st = q[prune(q - ctr, hh, margin)]                                 # the stored list
        kept[c] = len(st)
        for oc in range(8):
            octr = o + (g["cells3"][c] + 0.25 + 0.5 * np.array([oc & 1, (oc >> 1) & 1, oc >> 2])) * h
            d = np.maximum(np.abs(st - octr) - 0.25 * h, 0.0)
            inr = st[(d * d).sum(1) <= r * r]
            oct_kept[c, oc] = int(prune(inr - octr, hw, margin).sum()) if len(inr) else 0
    g["kept"], g["oct_kept"] = kept, oct_kept
    return g


def lines_row(cnt):
    ln = (cnt + 7) // 8
    return "%.2f | %.1f %% | %.1f %% | %.1f %% | %.3f" % (cnt.mean(), 100.0 * (ln == 1).mean(), 100.0 * (ln == 2).mean(), 100.0 * (ln >= 3).mean(), ln.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--workloads", default="Cm,small")
    args = ap.parse_args()
    for name in args.workloads.split(","):
        m, s, k = synth.workload(name)
        eps = float(getattr(s, "eps", 0.005))
        cs = s.pos.mean(0, dtype=np.float32); cm = m.pos.mean(0, dtype=np.float32)
        # (the library's centroids are sequential float sums; the mean here differs from them in the last bits, the census does not care)
        spos = s.pos - cs; mpos = (m.pos - cm).astype(np.float64)
        g = build(spos, eps)
        long_ = g["kept"] > 8
        fits = long_ & (g["oct_kept"] <= 8).all(1)
        T = synth.make_candidates(synth.centred_gt(s.T_gt, cs.astype(np.float64), cm.astype(np.float64)), k, seed=synth.SEED_CAND)[:args.poses]
        today, every, built, visits_long = [], [], [], 0
        for T16 in T:
            A = T16.reshape(4, 4).T.astype(np.float64)
            qp = mpos @ A[:3, :3].T + A[:3, 3]
            c4 = np.floor((qp - g["o"]) * (4.0 / g["h"])).astype(np.int64)
            c = c4 >> 2
            inside = ((c >= 0) & (c < g["n"])).all(1)
            key = (c[:, 2] * g["n"][1] + c[:, 1]) * g["n"][0] + c[:, 0]
            row = np.minimum(np.searchsorted(g["ukey"], np.where(inside, key, -1)), len(g["ukey"]) - 1)
            found = inside & (g["ukey"][row] == key)
            sb = ((c4[:, 2] & 3) << 4) | ((c4[:, 1] & 3) << 2) | (c4[:, 0] & 3)
            surv = found & (((g["mask"][row] >> sb.astype(np.uint64)) & np.uint64(1)) != 0)
            row, c4 = row[surv], c4[surv]
            oc = ((c4[:, 0] >> 1) & 1) | (((c4[:, 1] >> 1) & 1) << 1) | (((c4[:, 2] >> 1) & 1) << 2)
            today.append(g["kept"][row]); every.append(g["oct_kept"][row, oc])
            built.append(np.where(fits[row], np.where(g["oct_kept"][row, oc] > 0, 8, 0), g["kept"][row]))
            visits_long += int(long_[row].sum())
        today, every, built = np.concatenate(today), np.concatenate(every), np.concatenate(built)
        print("%s: %d non-empty cells, stored entries %.2f per cell (%d padded to lines); %d cells keep more than 8 (%.1f %%), they receive %.1f %% of the %d"
              " list visits of %d poses; in %d of them (%.1f %%) every octant keeps at most 8 (%d octant entries; blocks of 1 KB: %.2f MB beside %.2f MB of lists)\n" % (
                  name, len(g["ukey"]), g["kept"].mean(), int(((g["kept"] + 7) // 8 * 8).sum()), int(long_.sum()), 100.0 * long_.mean(), 100.0 * visits_long / len(today),
                  len(today), len(T), int(fits.sum()), 100.0 * fits.sum() / max(long_.sum(), 1), int(g["oct_kept"][fits].sum()), long_.sum() * 1024 / 1e6,
                  ((g["kept"] + 7) // 8 * 8).sum() * 16 / 1e6))
        print("| %s | mean entries | 1 line | 2 lines | >= 3 lines | mean lines |\n|---|---|---|---|---|---|" % name)
        print("| cell-pruned (today) | %s |" % lines_row(today))
        print("| pruned per octant, every cell | %s |" % lines_row(every[every > 0]))
        print("| octant lines of 8 where all eight octants fit, else today's list | %s |\n" % lines_row(built[built > 0]))


if __name__ == "__main__":
    main()
