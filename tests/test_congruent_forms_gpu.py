"""Every form of the congruent-set phase against the CPU oracle (stocs_internal_find_congruent / CountPass, csrc/congruent.hip).

The phase picks its form per call: pair lists reduced to the entries with a partner cell or kept whole, 32- or 64-bit list keys, one
stream or two, the library's own sort or rocPRIM's, sizes from a capacity or exact -- and per batch size: cone records computed late from
512 bases on, no run table (full lists, 64-bit keys) beyond 8 192 bases on `tiny` (32^3 position cells x nB > 2^28).  Here the per-call
switches run as a product on ONE context in a shuffled order, each cell on other bases than the one before it (state a form forgets to
write shows up as a mismatch); the batch sizes run at their edges; the switches read once per process run in child processes.  Every
result -- per-base quads, walk order, candidates -- is compared with the oracle or, for the candidates, bit for bit with the default form
on the same bases."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "fresh_process_child.py")
SWITCHES = ("STOCS_CONGRUENT_KEEP_ALL", "STOCS_CONGRUENT_WIDE_KEYS", "STOCS_CONGRUENT_ID_BITS", "STOCS_CONGRUENT_TWO_STREAMS",
            "STOCS_CONGRUENT_ONE_STREAM", "STOCS_CONGRUENT_EXACT_SIZES", "STOCS_CONGRUENT_CAPACITY", "STOCS_CONGRUENT_NO_LDS_BITS",
            "STOCS_CONGRUENT_P_FULLSORT", "STOCS_CONGRUENT_DISTANCE_GATE", "STOCS_TRANSFORMS_HOST_PICKS", "STOCS_DEBUG_STREAMS")
WALK_ALL = 4096          # walk order: every rank of a base up to this many quads, a seeded sample (first and last rank included) beyond


class OracleCache:
    """find_congruent / find_congruent_seq of the oracle, once per distinct (base, invariants)."""

    def __init__(self, orc):
        self.orc, self.memo = orc, {}

    def get(self, ids, inv):
        key = (tuple(int(x) for x in ids), np.asarray(inv, np.float32).tobytes())
        if key not in self.memo:
            i1, i2 = float(inv[0]), float(inv[1])
            self.memo[key] = (self.orc.find_congruent(ids, i1, i2), self.orc.find_congruent_seq(ids, i1, i2))
        return self.memo[key]


@pytest.fixture(scope="module")
def forms(oracle_lib):
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, _ = synth.workload("tiny")
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    orc = oracle_lib.Oracle(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=True)
    cache = OracleCache(orc)
    # the pool: valid bases of the oracle's own sampling ...
    ids, inv = [], []
    for a in range(140):
        ok, oi, ov = orc.sample_class_base(31337, a)
        if ok:
            ids.append(oi); inv.append(ov)
    n_valid = len(ids)
    # ... and bases whose first or second pair has no index entry (stocs.cpp:788: both lists empty, zero quads)
    pos, nrm = orc.scene_centred(), oracle_lib.normalize_rows(s.nrm)
    rng = np.random.default_rng(2718)
    found = {0: 0, 1: 0}
    while min(found.values()) < 3:
        b = rng.choice(len(pos), 4, replace=False).astype(np.int32)
        empty = [len(orc.index_lookup(oracle_lib.ppf_compute(pos[b[2 * j]], nrm[b[2 * j]], pos[b[2 * j + 1]], nrm[b[2 * j + 1]]))) == 0 for j in (0, 1)]
        if empty[0] != empty[1] and found[int(empty[1])] < 3:
            found[int(empty[1])] += 1
            ids.append(b); inv.append(rng.uniform(0.2, 0.8, 2).astype(np.float32))
    ids, inv = np.array(ids, np.int32), np.array(inv, np.float32)
    counts = np.array([len(cache.get(ids[k], inv[k])[0]) for k in range(len(ids))])
    assert n_valid >= 110 and (counts[:n_valid] > 0).sum() >= 30, (n_valid, (counts > 0).sum())   # (131 valid, 38 with quads)
    assert (counts[n_valid:] == 0).all()                         # the empty-list bases
    yield est, orc, cache, ids, inv, counts, n_valid
    est.close()


def _set_switches(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _walk_ranks(n, rng):
    if n <= WALK_ALL:
        r = np.arange(n, dtype=np.int64)
        return r[::-1].copy() if rng.random() < 0.5 else r
    return np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 1024)])).astype(np.int64)


def _check_quads(est, cache, ids, inv, total, rng, ctx=""):
    """find_congruent_all's total, every base's quads bit for bit, its walk order (stocs_get_quads_at) against the oracle's sequence."""
    refs = [cache.get(ids[k], inv[k]) for k in range(len(ids))]
    assert total == sum(len(q) for q, _ in refs), ctx
    for k, (qo, so) in enumerate(refs):
        qg = est.get_quads(k)
        assert qg.shape == qo.shape and np.array_equal(qg, qo), (ctx, k, qo.shape, qg.shape)
        assert len(so) == len(qo) == est.num_quads(k), (ctx, k)
        if len(so):
            r = _walk_ranks(len(so), rng)
            assert np.array_equal(est.get_quads_at(k, r), so[r]), (ctx, k)


def _labels(est):
    return [lab for lab, _ in est.last_call_timing(0)]


def _pick(rng, counts, n_valid, n, n_empty):
    """n pool bases with repeats: n_empty of them with an empty list, the rest valid; the last one has quads (the edge of every
    per-base launch)."""
    nz = np.nonzero(counts[:n_valid] > 0)[0]
    sel = rng.permutation(np.concatenate([rng.choice(n_valid, n - n_empty - 1), rng.choice(np.arange(n_valid, len(counts)), n_empty)]))
    return np.concatenate([sel, rng.choice(nz, 1)]).astype(np.int64)


# ---- the per-call switch matrix ----
MAIN = {"lists": ({}, {"STOCS_CONGRUENT_KEEP_ALL": "1"}),
        "keys": ({}, {"STOCS_CONGRUENT_WIDE_KEYS": "1"}, {"STOCS_CONGRUENT_ID_BITS": "16"}),
        "streams": ({}, {"STOCS_CONGRUENT_TWO_STREAMS": "1"}, {"STOCS_CONGRUENT_ONE_STREAM": "1"})}
PAIRED = {"sizing": ({}, {"STOCS_CONGRUENT_EXACT_SIZES": "1"}, {"STOCS_CONGRUENT_CAPACITY": "0.05"}),
          "no_lds_bits": ({}, {"STOCS_CONGRUENT_NO_LDS_BITS": "1"}),
          "p_fullsort": ({}, {"STOCS_CONGRUENT_P_FULLSORT": "1"}),
          "distance_gate": ({}, {"STOCS_CONGRUENT_DISTANCE_GATE": "1"})}


def _matrix():
    """The full product of MAIN; the PAIRED switches chosen greedily per cell so that every value of every switch meets every value of
    every other switch at least once (asserted)."""
    names = list(MAIN) + list(PAIRED)
    sizes = [len(MAIN[n]) for n in MAIN] + [len(PAIRED[n]) for n in PAIRED]
    need = {(i, a, j, b) for i, j in itertools.combinations(range(len(names)), 2) for a in range(sizes[i]) for b in range(sizes[j])}
    cells = []
    for main in itertools.product(*[range(len(MAIN[n])) for n in MAIN]):
        best = max(itertools.product(*[range(len(PAIRED[n])) for n in PAIRED]),
                   key=lambda ext: sum((i, c[i], j, c[j]) in need for c in [main + ext] for i, j in itertools.combinations(range(len(names)), 2)))
        c = main + best
        need -= {(i, c[i], j, c[j]) for i, j in itertools.combinations(range(len(names)), 2)}
        cells.append(dict(zip(names, c)))
    assert not need, sorted(need)[:5]
    return cells


def test_every_combination_of_lists_keys_and_streams_equals_the_oracle(forms, monkeypatch):
    """18 cells of lists x keys x streams (sizing, occupancy bits in device memory, P sorted on all bits and the distance gate
    paired over them) in a seeded, shuffled order on one context, each on its own subset of the pool (repeats and empty-list bases
    among them).  The host steps of the call name the form that ran; quads and walk order equal the oracle's; the candidates of
    make_transforms equal the default form's on the same bases, bit for bit."""
    est, orc, cache, ids, inv, counts, n_valid = forms
    rng = np.random.default_rng(20261015)
    cells = _matrix()
    rng.shuffle(cells)
    est.set_option("device_clock", 1)             # (the "device: ..." steps name the stream form)
    _set_switches(monkeypatch, {})
    sel = _pick(rng, counts, n_valid, 24, 2)
    est.set_bases(ids[sel], inv[sel])
    _check_quads(est, cache, ids[sel], inv[sel], est.find_congruent_all(), rng, "first call")   # (capacities known from here on)
    redone = 0
    try:
        for cell in cells:
            env = {}
            for n in MAIN:
                env.update(MAIN[n][cell[n]])
            for n in PAIRED:
                env.update(PAIRED[n][cell[n]])
            sel = _pick(rng, counts, n_valid, int(rng.integers(6, 48)), int(rng.integers(1, 4)))
            bi, bv = ids[sel], inv[sel]
            _set_switches(monkeypatch, env)
            est.set_bases(bi, bv)
            total = est.find_congruent_all()
            labels = _labels(est)
            reduce, wide = cell["lists"] == 0, cell["keys"] == 1
            one_stream = reduce and not wide and cell["streams"] != 1
            optimistic = reduce and cell["sizing"] != 1
            assert ("wait for the device (plan)" in labels) == (not optimistic), (env, labels)
            assert ("enqueue compact/sort/records/join/scan" in labels) == reduce, (env, labels)
            assert ("enqueue gather/sort/records/join/scan" in labels) == (not reduce), (env, labels)
            assert ("arena reserve (64-bit keys)" in labels) == wide and ("arena reserve" in labels) == (not wide), (env, labels)
            assert any("P and Q as one list" in lab for lab in labels) == one_stream, (env, labels)
            assert any("aux stream" in lab for lab in labels) == (not one_stream), (env, labels)
            redone += "plan beyond the capacities: redone with exact sizes" in labels
            _check_quads(est, cache, bi, bv, total, rng, env)
            seed = int(rng.integers(1, 1 << 30))
            c1 = est.make_transforms(40, seed)
            T1, P1, _, b1 = est.get_pose_candidates()
            _set_switches(monkeypatch, {})
            assert est.find_congruent_all() == total, env
            assert est.make_transforms(40, seed) == c1 and c1 > 0, env
            T0, P0, _, b0 = est.get_pose_candidates()
            assert np.array_equal(T1.view(np.uint32), T0.view(np.uint32)) and np.array_equal(P1.view(np.uint32), P0.view(np.uint32)) and np.array_equal(b1, b0), env
    finally:
        est.set_option("device_clock", 0)
    assert redone >= 1                            # (a capacity of 0.05 x the last call's lists: the redo with exact sizes ran)


# ---- batch sizes at their edges ----
@pytest.mark.parametrize("nB", [1, 511, 512, 8192, 8193])
def test_base_counts_at_the_edges_of_the_forms_equal_the_oracle(forms, monkeypatch, nB):
    """1 and 511 bases: cone records with the jobs; from 512: computed while the device gathers and patched into the jobs
    (patch_cone_kernel); 8 192 bases: the last with the run table (32^3 cells per base); 8 193: no run table -- full lists, 64-bit keys,
    rocPRIM, two streams.  Pool bases repeated, empty-list ones among them; every base against the oracle."""
    est, orc, cache, ids, inv, counts, n_valid = forms
    _set_switches(monkeypatch, {})
    rng = np.random.default_rng(nB)
    sel = _pick(rng, counts, n_valid, nB, 0 if nB == 1 else max(1, nB // 50))
    est.set_bases(ids[sel], inv[sel])
    total = est.find_congruent_all()
    labels = _labels(est)
    assert any(lab.startswith("host: cone records of the bases") for lab in labels) == (nB >= 512), labels
    assert ("arena reserve (no run table, 64-bit keys)" in labels) == (nB > 8192), labels
    assert ("enqueue compact/sort/records/join/scan" in labels) == (nB <= 8192), labels
    _check_quads(est, cache, ids[sel], inv[sel], total, rng, nB)


@pytest.mark.parametrize("nB", [7, 600])
def test_a_call_whose_bases_all_have_empty_lists_then_one_with_quads(forms, monkeypatch, nB):
    est, orc, cache, ids, inv, counts, n_valid = forms
    _set_switches(monkeypatch, {})
    rng = np.random.default_rng(nB + 1)
    sel = rng.choice(np.arange(n_valid, len(counts)), nB)
    est.set_bases(ids[sel], inv[sel])
    assert est.find_congruent_all() == 0
    assert all(est.num_quads(k) == 0 for k in range(nB)) and est.get_quads(nB - 1).shape == (0, 4)
    assert est.make_transforms(40, 5) == 0
    sel = _pick(rng, counts, n_valid, nB, 1)
    est.set_bases(ids[sel], inv[sel])
    _check_quads(est, cache, ids[sel], inv[sel], est.find_congruent_all(), rng, nB)


# ---- a trial batch ----
def test_trial_batch_with_full_lists_equals_the_default(forms, monkeypatch):
    """run_trials (three seeds) with the lists kept whole: bit for bit the default batch."""
    est, *_ = forms
    _set_switches(monkeypatch, {})
    seeds = [404, 405, 406]
    res0 = est.run_trials(seeds, 24, max_per_base=40, keep_details=True)
    d0 = [(est.trial_quad_counts(t), est.trial_candidates(t)) for t in range(3)]
    _set_switches(monkeypatch, {"STOCS_CONGRUENT_KEEP_ALL": "1"})
    res1 = est.run_trials(seeds, 24, max_per_base=40, keep_details=True)
    for t in range(3):
        r0, r1 = res0[t], res1[t]
        assert (r1["n_bases"], r1["n_quads"], r1["n_candidates"], r1["best_index"]) == (r0["n_bases"], r0["n_quads"], r0["n_candidates"], r0["best_index"]), t
        assert np.float32(r1["best_lcp"]).view(np.uint32) == np.float32(r0["best_lcp"]).view(np.uint32)
        assert np.array_equal(np.asarray(r1["best_pose"]).view(np.uint32), np.asarray(r0["best_pose"]).view(np.uint32))
        qc, (T, P, l, b) = est.trial_quad_counts(t), est.trial_candidates(t)
        assert np.array_equal(qc, d0[t][0]) and qc.sum() > 0
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip((T, P, l, b), d0[t][1]))


# ---- switches read once per process: child processes ----
def test_switches_read_once_per_process_equal_the_oracle(forms, tmp_path):
    """rocPRIM sorting the 32-bit pair lists (STOCS_SORT=rocprim: default, full lists) and the gather / survivor count with
    1, 3 and 7 workgroups (STOCS_GATHER_WGS: every workgroup walks many tiles across base boundaries), 600 bases each (cone records
    deferred): one child process per setting, one after the other, stopping at the first that fails."""
    est, orc, cache, ids, inv, counts, n_valid = forms
    rng = np.random.default_rng(600)
    sel = _pick(rng, counts, n_valid, 600, 8)
    bi, bv = ids[sel], inv[sel]
    path = str(tmp_path / "bases.npz")
    np.savez(path, ids=bi, inv=bv)
    refs = [cache.get(bi[k], bv[k]) for k in range(len(bi))]
    cells = [{"STOCS_SORT": "rocprim"}, {"STOCS_SORT": "rocprim", "STOCS_CONGRUENT_KEEP_ALL": "1"},
             {"STOCS_GATHER_WGS": "1"}, {"STOCS_GATHER_WGS": "3"}, {"STOCS_GATHER_WGS": "7"},
             {"STOCS_GATHER_WGS": "3", "STOCS_CONGRUENT_TWO_STREAMS": "1"}]   # (one list per launch, first side 0 and 1, many tiles per workgroup)
    for cell in cells:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES and k not in ("STOCS_SORT", "STOCS_GATHER_WGS")}
        env.update(cell)
        p = subprocess.run([sys.executable, CHILD, "congruent", path], env=env, capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, (cell, p.returncode, p.stderr[-3000:])
        out = json.loads(p.stdout.strip().splitlines()[-1])
        assert out["total"] == sum(len(q) for q, _ in refs), cell
        assert any(lab.startswith("host: cone records of the bases") for lab in out["labels"]), (cell, out["labels"])
        for k, (qo, so) in enumerate(refs):
            assert np.array_equal(np.array(out["quads"][k], np.int32).reshape(-1, 4), qo), (cell, k)
            assert np.array_equal(np.array(out["walk"][k], np.int32).reshape(-1, 4), so[: len(out["walk"][k]) // 4]), (cell, k)
            assert len(out["walk"][k]) // 4 == min(len(so), 300), (cell, k)
