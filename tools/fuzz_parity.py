#!/usr/bin/env python3
"""Randomised parity sweep: N small random workloads (model size, scene size, clutter, seeds all drawn), the whole
hot path on the GPU against the CPU oracle: bases + invariants, per-base quad counts, candidate transforms
(bit-exact) and scores (1e-5; a score beyond it counts as an exact-distance tie, divergence Q11, when the per-point matches show
two scene points equally far from the model point -- reported separately).  Prints one line per mismatch and a summary.
With --instance the workloads also get a random edge map (passable background, random edge segments and speckle,
some in-between values, an isolated pocket around some points) and the sampling runs in instance mode (persistent
device kernel with the union-find flood fill) against the oracle's literal BFS, attempt by attempt, plus the segment of
the last attempt and the decayed class prior.
With --batch every workload also runs four trials as ONE batch (stocs_run_trials): trial 0 against the oracle's run, trials 1-3
against the same seeds run alone through the single-trial calls (bitwise: counts, candidates, scores, winner).
With --exact-ties every context runs with stocs_set_option("exact_ties", 1): no tie escape is applied, and the summary adds the
queries the reference-order kd-tree answered (ties_flagged) and those whose answer differs from the default rule (ties_changed).
usage: python tools/fuzz_parity.py [N] [first_seed] [--instance] [--batch] [--exact-ties]"""
import json
import os
import sys

import numpy as np

n_ties = 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import os as _os; _os.environ.setdefault("STOCS_PIN_BLAS", "1")   # harness side: one BLAS thread under the cgroup CPU quota; the library import itself has no side effects
from model_matching_amd import synth  # noqa: E402
from model_matching_amd.estimator import StocsEstimator  # noqa: E402
from oracle import pyoracle  # noqa: E402


def random_edge_map(rng, pix, H=480, W=640):
    e = np.full((H, W), 255, np.uint8)
    for _ in range(int(rng.integers(5, 60))):          # edge segments (value 0) of thickness 1-3
        r0, c0 = rng.integers(0, H), rng.integers(0, W)
        ang = rng.uniform(0, np.pi); L = int(rng.integers(20, 400)); th = int(rng.integers(1, 4))
        t = np.arange(L)
        rr = np.clip((r0 + t * np.sin(ang)).astype(int), 0, H - 1); cc = np.clip((c0 + t * np.cos(ang)).astype(int), 0, W - 1)
        for d in range(th):
            e[np.clip(rr + d, 0, H - 1), cc] = 0
    k = int(rng.integers(0, 4000))                       # speckle: edge pixels and in-between values (neither pruned nor passable)
    e[rng.integers(0, H, k), rng.integers(0, W, k)] = rng.choice(np.array([0, 0, 128, 254], np.uint8), k)
    for _ in range(int(rng.integers(0, 4))):             # a closed box around a scene point: a pocket the fill cannot leave
        r, c = pix[int(rng.integers(0, len(pix)))]
        h = int(rng.integers(3, 25))
        r0, r1, c0, c1 = max(r - h, 0), min(r + h, H - 1), max(c - h, 0), min(c + h, W - 1)
        e[r0, c0:c1 + 1] = 0; e[r1, c0:c1 + 1] = 0; e[r0:r1 + 1, c0] = 0; e[r0:r1 + 1, c1] = 0
    return e


def instance_leg(est, orc, rng, s, seed, nb):
    import ctypes as C
    edge = random_edge_map(rng, s.pixel)
    est.set_edge_map(edge); orc.set_edge_map(edge)
    est.L.stocs_clear_bases(est.h)
    valid, ids, inv = est.sample_bases(seed, nb, mode=1, dispersion=0.9)
    ok = True
    for a in range(nb):
        o, oi, ov = orc.sample_instance_base(seed, a, 0.9, a + 1)
        ok &= o == bool(valid[a])
        if o and valid[a]:
            ok &= bool(np.array_equal(oi, ids[a]) and np.array_equal(ov, inv[a]))
    # the decayed prior after the attempts (Q8): what the LCP will add
    n = len(s.pos)
    pr = np.zeros(n, np.float32)
    est.L.stocs_get_scene(est.h, None, None, pr.ctypes.data_as(C.POINTER(C.c_float)), None)
    po = np.zeros(n, np.float32); pos3 = np.zeros((n, 3), np.float32); cls = np.zeros(n, np.float32)
    pyoracle.lib().orc_get_scene(orc.h, pos3.ctypes.data_as(C.POINTER(C.c_float)), po.ctypes.data_as(C.POINTER(C.c_float)), cls.ctypes.data_as(C.POINTER(C.c_float)))
    ok &= bool(np.array_equal(pr, cls))
    return ok, int(valid.sum())


def is_distance_tie(est, orc, m, T16):
    """A score beyond the tolerance is the documented divergence Q11 when every model point whose match differs has a match on
    both sides and the two scene points are equally far from it (equal in float32: 1e-8 m apart at most in float64)."""
    hg, cg = est.lcp_detail(T16); ho, co = orc.lcp_detail(T16)
    bad = np.nonzero(hg != ho)[0]
    if len(bad) == 0 or not np.array_equal(np.delete(cg, bad), np.delete(co, bad)):
        return False
    pos = orc.scene_centred().astype(np.float64)
    mc = m.pos.astype(np.float32) - est.get_model_centroid().astype(np.float32)
    T = np.asarray(T16, np.float64).reshape(4, 4).T
    for i in bad:
        if hg[i] < 0 or ho[i] < 0:
            return False
        p = T[:3, :3] @ mc[i].astype(np.float64) + T[:3, 3]
        if abs(np.linalg.norm(p - pos[hg[i]]) - np.linalg.norm(p - pos[ho[i]])) > 1e-8:
            return False
    return True


def main():
    global n_ties
    instance = "--instance" in sys.argv
    batch = "--batch" in sys.argv
    exact = "--exact-ties" in sys.argv
    argv = [a for a in sys.argv if a not in ("--instance", "--batch", "--exact-ties")]
    n = int(argv[1]) if len(argv) > 1 else 20
    first = int(argv[2]) if len(argv) > 2 else 1000
    pyoracle.build()
    bad = 0
    n_inst_bases = 0
    n_batch_trials = 0
    stats = []
    ties_flagged = ties_changed = 0
    for k in range(n):
        rng = np.random.default_rng(first + k)
        nm = int(rng.integers(120, 420))
        ns = int(rng.integers(500, 2200))
        m = synth.make_model(nm, seed=first + 7 * k)
        s = synth.make_scene(m, ns, seed=first + 11 * k, T_gt=synth.gt_pose(seed=first + 13 * k))
        args = (s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm)
        est = StocsEstimator(*args, build_index=True)
        orc = pyoracle.Oracle(*args, build_index=True)
        if exact:
            est.set_option("exact_ties", 1)
        seed = int(rng.integers(1, 1 << 30))
        nb = int(rng.integers(20, 80))
        r = orc.run(seed, nb, 200)
        valid, ids, inv = est.sample_bases(seed, nb)
        ok = int(valid.sum()) == r.n_bases
        tot = est.find_congruent_all()
        ok &= tot == r.n_quads_total
        nc = est.make_transforms(200, seed)
        ok &= nc == r.n_candidates
        To, Po, bo = orc.candidates()
        Tg, Pg, lg, bg = est.get_pose_candidates()
        ok &= Tg.shape == To.shape and np.array_equal(To, Tg) and np.array_equal(Po, Pg) and np.array_equal(bo, bg)
        lcp, idx, pose = est.compute_best_transform()
        if exact:
            f, ch = est.last_tie_counts()
            ties_flagged += f; ties_changed += ch
        dl = abs(lcp - r.best_lcp)
        ok &= dl <= 1e-5
        if len(To):
            lo = orc.lcp_batch(To, nthreads=8)
            dd = np.abs(est.get_pose_candidates()[2] - lo)
            over = np.nonzero(dd > 1e-5)[0]
            if len(over) and not exact and all(is_distance_tie(est, orc, m, To[c]) for c in over):
                n_ties += len(over)            # (Q11: two scene points at the same f32 distance, the kd-tree's visiting order picks the other one)
                dd[over] = 0.0
            dmax = float(dd.max())
            ok &= dmax <= 1e-5
        else:
            dmax = 0.0
        if batch:
            seeds = [seed + j for j in range(4)]
            res = est.run_trials(seeds, nb, mode=0, max_per_base=200, keep_details=True)
            bok = (res[0]["n_bases"], res[0]["n_quads"], res[0]["n_candidates"]) == (r.n_bases, r.n_quads_total, r.n_candidates) and abs(res[0]["best_lcp"] - r.best_lcp) <= 1e-5
            bok &= bool(np.array_equal(est.trial_candidates(0)[0], To))
            kept = [est.trial_candidates(j) for j in range(4)]
            for j in range(1, 4):
                est.reset_trial()
                v1, _, _ = est.sample_bases(seeds[j], nb)
                q1 = est.find_congruent_all(); c1 = est.make_transforms(200, seeds[j]); l1, i1, p1 = est.compute_best_transform()
                T1, P1, s1, b1 = est.get_pose_candidates()
                bok &= (res[j]["n_bases"], res[j]["n_quads"], res[j]["n_candidates"], res[j]["best_index"]) == (int(v1.sum()), q1, c1, i1) and res[j]["best_lcp"] == l1
                bok &= bool(np.array_equal(kept[j][0], T1) and np.array_equal(kept[j][2].view(np.uint32), s1.view(np.uint32)) and np.array_equal(kept[j][3], b1)
                            and np.array_equal(res[j]["best_pose"], p1))
            if not bok:
                print("BATCH MISMATCH", dict(k=k, nm=nm, ns=ns, seed=seed, nb=nb), flush=True)
            ok &= bok
            n_batch_trials += 4
        if instance:
            iok, nv = instance_leg(est, orc, rng, s, seed + 1, nb)
            if not iok:
                print("INSTANCE MISMATCH", dict(k=k, nm=nm, ns=ns, seed=seed + 1, nb=nb), flush=True)
            ok &= iok
            n_inst_bases += nv
        stats.append((nm, ns, nb, r.n_bases, int(tot), int(nc), dmax))
        if not ok:
            bad += 1
            print("MISMATCH", dict(k=k, nm=nm, ns=ns, seed=seed, nb=nb, bases=(int(valid.sum()), r.n_bases), quads=(int(tot), r.n_quads_total),
                                   cands=(int(nc), r.n_candidates), dl=dl, dmax=dmax), flush=True)
        est.close()
        if (k + 1) % 25 == 0:
            print("... %d workloads, %d mismatches" % (k + 1, bad), file=sys.stderr, flush=True)
    print(json.dumps({"workloads": n, "batched_trials_checked": n_batch_trials, "instance_mode": instance, "instance_bases": n_inst_bases, "mismatches": bad, "exact_distance_ties_q11": n_ties, "exact_ties": exact, "ties_flagged": ties_flagged, "ties_changed": ties_changed, "total_quads": int(sum(x[4] for x in stats)), "total_candidates": int(sum(x[5] for x in stats)),
                      "max_abs_lcp_diff": max(x[6] for x in stats)}))


if __name__ == "__main__":
    main()
