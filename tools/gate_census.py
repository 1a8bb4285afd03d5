#!/usr/bin/env python3
"""CPU census of the normal-cone gate of the queue kernel (model_matching_amd/csrc/normal_cone.h): how many of the queries that
survive the sub-cell mask can be counted at all.

A restatement, no GPU: scipy kd-tree for the nearest scene point within epsilon, the grid of grid.hip at cell edge epsilon (float
origin, every scene point within 1.001 epsilon of the cell box in the cell's list -- the DILATED list, a superset of the pruned
list the library stores, so the library's cones are a little tighter), 4x4x4 sub-cell masks, and per cell the cone of its list's
normals packed and decoded as normal_cone.h does (octahedral axis, half-angle class measured against the decoded axis, rounded
outwards) and tested with the kernel's bound and margins in float64.  Per pose: hits (a neighbour within epsilon), counted (it
also passes the 30-degree normal test), queries that survive the mask, those that also survive the cone, and counted points the
cone would have lost (must be 0).

--normal-bits B restates the gate on the PACKED model normal (three signed B-bit components, k = round((2^(B-1) - 1) n), normal_cone.h:
the library packs 10 bits): the gate sees k / (2^(B-1) - 1) and its threshold drops by s (Q (1 + 1e-4) + 1e-6), Q the quantisation bound
(10 bits: the library's STOCS_MODEL_NORMAL_Q = 1.7e-3; any other width: the plain sqrt(3) / (2 (2^(B-1) - 1))), s the norm bound of the pose's linear part; the normal test and the
"counted" column keep the exact normal.  0 (the default): the gate on the exact normal.

usage: python tools/gate_census.py [--axis-bits 6] [--sin-steps 16] [--poses 192] [--normal-bits 10]   (prints a markdown table)
"""
import argparse
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from model_matching_amd import synth  # noqa: E402

DOT_LO = np.float32(np.cos(np.deg2rad(30.0)))


def decode_axis(u, v, amax):
    x = u.astype(np.float64) * (2.0 / amax) - 1.0
    y = v.astype(np.float64) * (2.0 / amax) - 1.0
    z = 1.0 - np.abs(x) - np.abs(y)
    t = np.maximum(-z, 0.0)
    x = x + np.where(x >= 0, -t, t)
    y = y + np.where(y >= 0, -t, t)
    return np.stack([x, y, z], 1)


def build_grid(spos, snrm, eps, axis_bits, sin_steps):
    """cells (dict key -> row), per cell: 64-bit mask, cone axis (unnormalised), sin class (0: no gate)"""
    h, r = eps, eps * 1.001
    pad = r + 2 * h
    o = (spos.min(0).astype(np.float64) - pad).astype(np.float32).astype(np.float64)
    n = np.floor((spos.max(0) + pad - o) / h).astype(np.int64) + 1
    p = spos.astype(np.float64)
    lo = np.maximum(np.floor((p - r - o) / h).astype(np.int64), 0)
    pts, keys, cells3 = [], [], []
    for dz in range(4):
        for dy in range(4):
            for dx in range(4):
                c = lo + np.array([dx, dy, dz])
                b0 = o + c * h
                d = np.maximum(np.maximum(b0 - p, p - (b0 + h)), 0.0)
                ok = ((d * d).sum(1) <= r * r) & (c < n).all(1)
                pts.append(np.nonzero(ok)[0]); cells3.append(c[ok])
    pts = np.concatenate(pts); cells3 = np.concatenate(cells3)
    key = (cells3[:, 2] * n[1] + cells3[:, 1]) * n[0] + cells3[:, 0]
    order = np.lexsort((pts, key))
    pts, key, cells3 = pts[order], key[order], cells3[order]
    ukey, first = np.unique(key, return_index=True)
    cell_of = np.searchsorted(ukey, key)
    # sub-cell masks
    mask = np.zeros(len(ukey), np.uint64)
    hs = h / 4.0
    for s in range(64):
        sc = 4 * cells3 + np.array([s & 3, (s >> 2) & 3, s >> 4])
        b0 = o + sc * hs
        d = np.maximum(np.maximum(b0 - p[pts], p[pts] - (b0 + hs)), 0.0)
        near = (d * d).sum(1) <= r * r
        got = np.zeros(len(ukey), bool)
        got[cell_of[near]] = True
        mask |= got.astype(np.uint64) << np.uint64(s)
    # cones
    nf = snrm.astype(np.float64)[pts]
    ln = np.linalg.norm(nf, axis=1)
    bad = ~(np.abs(ln - 1.0) <= 1e-4)
    unit = nf / np.where(ln > 0, ln, 1.0)[:, None]
    ssum = np.add.reduceat(np.where(bad[:, None], 0.0, unit), first, axis=0)
    any_bad = np.add.reduceat(bad.astype(np.int64), first) > 0
    l1 = np.abs(ssum).sum(1)
    amax = float((1 << axis_bits) - 1)
    q = ssum / np.where(l1 > 0, l1, 1.0)[:, None]
    px, py = q[:, 0].copy(), q[:, 1].copy()
    neg = q[:, 2] < 0
    fx = (1.0 - np.abs(py)) * np.where(px >= 0, 1.0, -1.0); fy = (1.0 - np.abs(px)) * np.where(py >= 0, 1.0, -1.0)
    px = np.where(neg, fx, px); py = np.where(neg, fy, py)
    u = np.clip(np.floor((px * 0.5 + 0.5) * amax + 0.5), 0, amax); v = np.clip(np.floor((py * 0.5 + 0.5) * amax + 0.5), 0, amax)
    axis = decode_axis(u, v, amax)
    ax_unit = axis / np.linalg.norm(axis, axis=1)[:, None]
    cosang = (unit * ax_unit[cell_of]).sum(1)
    cmin = np.minimum.reduceat(np.where(bad, 1.0, cosang), first)
    sd = np.sqrt(np.maximum((1.0 - cmin) * (1.0 + cmin), 0.0))
    cls = np.floor(sd * sin_steps + 1e-4).astype(np.int64) + 1
    cls[(cmin <= 0) | (cls > sin_steps - 1) | any_bad | ~(l1 > 1e-9)] = 0
    half_angle = np.degrees(np.arcsin(np.clip(sd, 0, 1)))
    return dict(o=o, h=h, n=n, ukey=ukey, mask=mask, axis=axis, cls=cls, half_angle=np.where(cmin > 0, half_angle, 180.0), sin_steps=sin_steps)


def rules_out(axis, cls, sin_steps, v, dot_lo=float(DOT_LO)):
    S = (axis * axis).sum(1); W = (v * axis).sum(1); vv = (v * v).sum(1)
    va = W / np.sqrt(S)
    vp = np.sqrt(np.maximum(vv - va * va, 0.0))
    sd = cls / float(sin_steps); cd = np.sqrt(1.0 - sd * sd)
    bound = va * cd + vp * sd
    l1 = np.abs(v).sum(1)
    return (cls != 0) & (vp * cd > va * sd) & (bound * 1.0001 + 2e-3 * l1 < dot_lo)


def quantise(nrm, bits):
    """-> the normals as the gate sees them, the bound Q of the header for this width"""
    scale = float((1 << (bits - 1)) - 1)
    k = np.clip(np.rint(nrm.astype(np.float64) * scale), -scale, scale)
    # 10 bits: the library's constant STOCS_MODEL_NORMAL_Q; any other width: the format's plain bound, half a step per component
    return k / scale, 1.7e-3 if bits == 10 else np.sqrt(3.0) / (2.0 * scale) * (1.0 + 1e-12)


def norm_bound(A3):
    """linear_norm_bound of stocs_math.h: the square root of the largest absolute row sum of A^T A"""
    return float(np.sqrt(np.abs(A3.T @ A3).sum(1).max()) * 1.00001)


def census(scene_pos, scene_nrm, model_pos, model_nrm, T, eps, axis_bits, sin_steps, normal_bits=0):
    cs = scene_pos.mean(0, dtype=np.float32); cm = model_pos.mean(0, dtype=np.float32)
    spos = scene_pos - cs; mpos = model_pos - cm
    snrm = scene_nrm / np.linalg.norm(scene_nrm, axis=1, keepdims=True)
    g = build_grid(spos, snrm, eps, axis_bits, sin_steps)
    tree = cKDTree(spos.astype(np.float64))
    tot = np.zeros(5)
    gate_nrm, q_bound = quantise(model_nrm, normal_bits) if normal_bits else (model_nrm.astype(np.float64), 0.0)
    if normal_bits:
        assert np.linalg.norm(gate_nrm - model_nrm.astype(np.float64), axis=1).max() <= q_bound
    for T16 in T:
        A = T16.reshape(4, 4).T.astype(np.float64)
        qp = mpos.astype(np.float64) @ A[:3, :3].T + A[:3, 3]
        v = model_nrm.astype(np.float64) @ A[:3, :3].T
        d, j = tree.query(qp, distance_upper_bound=eps)
        hit = np.isfinite(d)
        dot = np.zeros(len(qp)); dot[hit] = (snrm[j[hit]].astype(np.float64) * v[hit]).sum(1)
        counted = hit & (dot >= float(DOT_LO)) & (dot <= 1.0)
        c4 = np.floor((qp - g["o"]) * (4.0 / g["h"])).astype(np.int64)
        c = c4 >> 2
        inside = ((c >= 0) & (c < g["n"])).all(1)
        key = (c[:, 2] * g["n"][1] + c[:, 1]) * g["n"][0] + c[:, 0]
        row = np.searchsorted(g["ukey"], np.where(inside, key, -1))
        row = np.minimum(row, len(g["ukey"]) - 1)
        found = inside & (g["ukey"][row] == key)
        sb = ((c4[:, 2] & 3) << 4) | ((c4[:, 1] & 3) << 2) | (c4[:, 0] & 3)
        surv = found & (((g["mask"][row] >> sb.astype(np.uint64)) & np.uint64(1)) != 0)
        thr = float(DOT_LO) - (norm_bound(A[:3, :3]) * (q_bound * 1.0001 + 1e-6) if normal_bits else 0.0)
        ruled = surv & rules_out(g["axis"][row], g["cls"][row], g["sin_steps"], gate_nrm @ A[:3, :3].T, thr)
        tot += [hit.sum(), counted.sum(), surv.sum(), (surv & ~ruled).sum(), (counted & ruled).sum()]
        assert not (hit & ~surv).any(), "a query with a neighbour within epsilon did not survive the mask"
    return tot / len(T), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--axis-bits", type=int, default=6)
    ap.add_argument("--sin-steps", type=int, default=16)
    ap.add_argument("--poses", type=int, default=192)
    ap.add_argument("--workloads", default="Cm,small,Cm_asym")
    ap.add_argument("--normal-bits", type=int, default=0, help="bits per component of the packed model normal the gate reads (0: the exact normal)")
    args = ap.parse_args()
    print("axis %d + %d bits octahedral, sin(half-angle) in %d steps%s; averages per pose\n" % (
        args.axis_bits, args.axis_bits, args.sin_steps, ", the gate on model normals of %d bits per component" % args.normal_bits if args.normal_bits else ""))
    print("| workload | poses | hits | counted | survive the mask | survive mask and cone | counted points lost | median half-angle |")
    print("|---|---|---|---|---|---|---|---|")
    for name in args.workloads.split(","):
        m, s, k = synth.workload(name)
        cs = s.pos.mean(0, dtype=np.float32).astype(np.float64); cm = m.pos.mean(0, dtype=np.float32).astype(np.float64)
        npose = args.poses if name != "Cm_asym" else args.poses // 2
        T = synth.make_candidates(synth.centred_gt(s.T_gt, cs, cm), k, seed=synth.SEED_CAND)[:npose]   # the head of bench.py's own batch
        eps = float(getattr(s, "eps", 0.005))
        t, g = census(s.pos, s.nrm, m.pos, m.nrm, T, eps, args.axis_bits, args.sin_steps, args.normal_bits)
        print("| %s | %d | %.0f | %.0f | %.0f | %.0f (%+.0f %%) | %g | %.1f deg |" % (name, npose, t[0], t[1], t[2], t[3], 100.0 * (t[3] / t[2] - 1.0), t[4] * npose,
                                                                                 float(np.median(g["half_angle"]))))


if __name__ == "__main__":
    main()
