"""The layer around the LCP scan kernels: which candidate a workgroup scores (lcp_candidate: processing order, XCD placement, ragged
last workgroups), who wins the arg-max (best_single_kernel, best_kernel, the key epilogue of lcp_store under an order) and the batched
detail rows behind stocs_lcp_hit_count.

Every scoring launch here goes through the device API and writes into a buffer filled with the sentinel -1.0 (scores are >= 0 by
construction): stocs_score_transforms writes into the context's scratch block, which still holds the previous call's scores, so a
candidate that a launch skipped would read back as its old, correct value there.  Everything is bitwise except the one oracle sample,
which uses the tolerances of test_lcp_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LCP_TOL = 1e-5        # test_lcp_gpu.py: against the oracle's running float sum
EXACT_TOL = 1e-7      # test_lcp_gpu.py: against the oracle's exact sum (the final rounding to float)
SENTINEL = np.float32(-1.0)
ORDERS = (0, 1, 2, 3, 5, 128, 4096)
FORM_DEFAULTS = (("lcp_variant", 99), ("lcp_split", 1), ("exact_ties", 0), ("lcp_order", 1))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _key_rule(s, id_offset):
    """compute_best_transform's arg-max as stocs_best_device states it: the largest of the scores > 0 (NaN, -0.0, 0 and negatives never
    win), among equals the lowest index; key = bits(s) << 32 | (0xFFFFFFFF - (id_offset + i)); nothing eligible -> key 0, (0.0, -1)"""
    s = np.asarray(s, np.float32)
    with np.errstate(invalid="ignore"):
        elig = s > 0
    if not elig.any():
        return 0, (0.0, -1)
    top = s[elig].max()
    i = int(np.flatnonzero(elig & (s == top))[0])
    gid = id_offset + i
    assert gid <= 0xFFFFFFFF
    return (int(_bits(s[i:i + 1])[0]) << 32) | (0xFFFFFFFF - gid), (float(s[i]), gid)


class _Dev:
    """a context with device buffers for up to cap candidates: transforms, scores, one key word"""

    def __init__(self, name, cap, oracle_lib=None):
        from model_matching_amd import synth
        from model_matching_amd.estimator import StocsEstimator
        m, s, _ = synth.workload(name)
        self.est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
        self.orc = oracle_lib.Oracle(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False) if oracle_lib else None
        cs, cm = self.est.get_scene_centroid().astype(np.float64), self.est.get_model_centroid().astype(np.float64)
        self.Tgt = synth.centred_gt(s.T_gt, cs, cm)
        self.cap = cap
        self.dT, self.dL, self.dK = self.est.dev_alloc(cap * 64), self.est.dev_alloc(cap * 4), self.est.dev_alloc(8)
        self.sentinel = np.full(cap, SENTINEL, np.float32)
        self.batches = {}

    def close(self):
        for p in (self.dT, self.dL, self.dK):
            self.est.dev_free(p)
        self.est.close()

    def forms(self, **opts):
        for k, v in FORM_DEFAULTS:
            self.est.set_option(k, opts.get(k, v))

    def upload(self, T):
        assert len(T) <= self.cap
        self.est.dev_upload(self.dT, T)

    def score(self, n, what=""):
        """the n uploaded candidates into the sentinel-filled score buffer: every element must have been written"""
        self.est.dev_upload(self.dL, self.sentinel[:n])
        self.est.score_device(self.dT, n, self.dL)
        return self._scores(n, what)

    def score_with_key(self, n, id_offset, what=""):
        """scores and the key of the kernel's epilogue; the key word holds all ones before the launch (the launch has to zero it)"""
        self.est.dev_upload(self.dL, self.sentinel[:n])
        self.est.dev_upload(self.dK, np.array([0xFFFFFFFFFFFFFFFF], np.uint64))
        self.est.score_best_device_async(self.dT, n, self.dL, id_offset, self.dK.value)
        key = np.zeros(1, np.uint64)
        self.est.dev_download(self.dK, key)
        return self._scores(n, what), int(key[0])

    def _scores(self, n, what):
        got = np.zeros(n, np.float32)
        self.est.dev_download(self.dL, got)
        skipped = np.flatnonzero(got == SENTINEL)
        assert len(skipped) == 0, (what, "candidates never scored", skipped[:8], len(skipped))
        assert np.isfinite(got).all() and got.min() >= 0.0, what
        return got

    def planted(self, n):
        """n candidates with the rows that an ordered launch could lose or mis-rank: a NaN translation, +inf and -inf translation
        entries, a duplicate of an early row placed late, a duplicate of the best row in the last slot.  -> (T, dict of row ids)"""
        if n not in self.batches:
            from model_matching_amd import synth
            T = synth.make_candidates(self.Tgt, n)
            rows = dict(nan=11, pinf=n // 3, ninf=n // 2 + 1, early=17, late=n - 501, last=n - 1)
            T[rows["nan"], 12:15] = np.nan
            T[rows["pinf"], 12] = np.inf
            T[rows["ninf"], 13] = -np.inf
            T[rows["late"]] = T[rows["early"]]
            self.forms()
            self.upload(T)
            rows["best"] = int(np.argmax(self.score(n, "planting")[:n - 1]))
            assert rows["best"] not in (rows["nan"], rows["pinf"], rows["ninf"], rows["late"])
            T[rows["last"]] = T[rows["best"]]
            self.batches[n] = (T, rows)
        return self.batches[n]


def _check_planted(got, rows, what, default_rule=True):
    assert got[rows["nan"]] == 0.0 and got[rows["pinf"]] == 0.0 and got[rows["ninf"]] == 0.0, what
    assert _bits(got)[rows["early"]] == _bits(got)[rows["late"]] and _bits(got)[rows["best"]] == _bits(got)[rows["last"]], what
    assert got[rows["best"]] > 0.05, what
    if default_rule:     # (the planting scored with the default tie rule; exact_ties may rank two near-equal candidates the other way)
        assert int(np.flatnonzero(got == got.max())[0]) == rows["best"], what


# ---- A. ordered and placed launches at ragged sizes ----
# (context, options): the grid of the scoring launch is n workgroups for the split and the one-wavefront forms, (n + 3) / 4 for the
# plain and the exact kernels, whose last workgroup is ragged at every size below
CM_CONTEXTS = (("split", {}), ("one_wave", {"lcp_split": 0}), ("plain", {"lcp_variant": 0}), ("exact", {"exact_ties": 1}))
CM_SIZES = (29999, 30001, 30002, 30007)      # x 5 000 model points: 29 999 is just below the ordering threshold of launch_lcp (1.5e8)


@pytest.fixture(scope="module")
def cm(oracle_lib):
    d = _Dev("Cm", 30007, oracle_lib)
    assert (d.est.nS, d.est.nM) == (20000, 5000)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dense():
    d = _Dev("dense", 50007)
    assert d.est.nM == 3000
    yield d
    d.close()


def _cross_orders(d, n, contexts, orders):
    """every (context, lcp_order) cell bitwise equal to lcp_order 0 of its context, every cell written in full -> {context: scores}"""
    T, rows = d.planted(n)
    d.upload(T)
    assert orders[0] == 0
    base = {}
    for name, opts in contexts:
        for order in orders:
            d.forms(**dict(opts, lcp_order=order))
            got = d.score(n, (n, name, order))
            if order == 0:
                base[name] = got
                _check_planted(got, rows, (n, name), default_rule=not opts.get("exact_ties"))
            else:
                assert np.array_equal(_bits(got), _bits(base[name])), (n, name, order, np.flatnonzero(_bits(got) != _bits(base[name]))[:8])
            # the two-kernel arg-max on what the launch left: the first maximum, not its duplicate in the last slot
            key, (s, gid) = _key_rule(got, 0)
            assert d.est.best_device(d.dL, n) == (s, gid, key) and gid < n - 1, (n, name, order)
    d.forms()
    return base


@pytest.mark.parametrize("n", CM_SIZES)
def test_ordered_launches_at_ragged_sizes(cm, n):
    """n mod 8 in {7, 1, 2, 7} and n mod 4 in {3, 1, 2, 3}: the remainders of lcp_candidate's XCD runs and the ragged last workgroup of
    the four-candidate kernels, under every lcp_order from plain batch order to runs of 4 096 (longer than the grid: no full run)"""
    base = _cross_orders(cm, n, CM_CONTEXTS, ORDERS)
    for name in ("one_wave", "plain"):
        assert np.array_equal(_bits(base[name]), _bits(base["split"])), (n, name)
    # exact_ties may differ from the default rule where test_exact_ties_gpu.py lets it (exact distance ties); it is compared with its own
    # lcp_order 0 above


def test_ordered_sample_equals_oracle(cm):
    n = 30007
    T, rows = cm.planted(n)
    cm.upload(T)
    cm.forms(lcp_order=3)
    got = cm.score(n, "lcp_order 3")
    cm.forms()
    fixed = sorted(set(list(range(8)) + list(range(n - 8, n)) + list(rows.values())))
    rest = np.setdiff1d(np.arange(n), fixed)
    idx = np.concatenate([fixed, np.random.default_rng(20).choice(rest, 256 - len(fixed), replace=False)]).astype(np.int64)
    assert len(idx) == 256 and len(set(idx.tolist())) == 256
    nthreads = max(1, min(16, len(os.sched_getaffinity(0))))
    ref, exact = cm.orc.lcp_batch_exact(T[idx], nthreads=nthreads)
    assert np.abs(got[idx] - ref).max() <= LCP_TOL
    assert np.abs(got[idx].astype(np.float64) - exact).max() <= EXACT_TOL
    assert got[idx].max() > 0.2


def test_batch_invariance_under_ordering(cm):
    n = 30007
    T, rows = cm.planted(n)
    cm.upload(T)
    cm.forms(lcp_order=2)
    got = cm.score(n, "whole")
    perm = np.random.default_rng(21).permutation(n)
    cm.upload(T[perm])
    assert np.array_equal(_bits(cm.score(n, "permuted")), _bits(got[perm]))
    cm.upload(T[:n - 3])
    assert np.array_equal(_bits(cm.score(n - 3, "shortened")), _bits(got[:n - 3]))
    cm.forms()


@pytest.mark.parametrize("name,opts", CM_CONTEXTS, ids=[c[0] for c in CM_CONTEXTS])
def test_key_epilogue_under_ordering(cm, name, opts):
    """the ordered path zeroes the key word in order_keys_kernel and lcp_store joins it through the order array: the key of the two-kernel
    arg-max and of the numpy rule, the scores the launch without a key writes"""
    n = 30007
    T, rows = cm.planted(n)
    cm.upload(T)
    cm.forms(**dict(opts, lcp_order=0))
    plain = cm.score(n, (name, "no key"))
    for order in (0, 2, 128):
        cm.forms(**dict(opts, lcp_order=order))
        for off in (0, 7 * n):
            got, key = cm.score_with_key(n, off, (name, order, off))
            assert np.array_equal(_bits(got), _bits(plain)), (name, order, off)
            want, (s, gid) = _key_rule(plain, off)
            assert key == want and gid < off + n - 1, (name, order, off, hex(key), hex(want))
            assert gid == off + rows["best"] or opts.get("exact_ties"), (name, order, off)
            assert cm.est.best_device(cm.dL, n, off) == (s, gid, want), (name, order, off)
    cm.forms()


DENSE_CONTEXTS = (("queue39", {"lcp_variant": 39}), ("step31", {"lcp_variant": 31}), ("step31_one_wave", {"lcp_variant": 31, "lcp_split": 0}))


@pytest.mark.parametrize("n", [50001, 50007])
def test_ordered_launches_dense_forms(dense, n):
    """the centre-sorted forms (queue kernel 39, always split) and the per-step kernel (31, split and one wavefront per candidate);
    x 3 000 model points: ordered from 50 000 candidates on"""
    base = _cross_orders(dense, n, DENSE_CONTEXTS, (0, 2, 5))
    for name in ("step31", "step31_one_wave"):
        assert np.array_equal(_bits(base[name]), _bits(base["queue39"])), (n, name)
    T, rows = dense.planted(n)
    for name, opts in DENSE_CONTEXTS[:2]:
        for order in (0, 2, 5):
            dense.forms(**dict(opts, lcp_order=order))
            got, key = dense.score_with_key(n, 7 * n, (name, order))
            assert np.array_equal(_bits(got), _bits(base[name])), (name, order)
            assert key == _key_rule(base[name], 7 * n)[0], (name, order)
    dense.forms()


# ---- B. the arg-max kernels on synthetic score arrays ----
SINGLE_MAX = 1 << 18          # enqueue_best: one workgroup of 1 024 threads up to here, else best_kernel
ARGMAX_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, SINGLE_MAX - 1, SINGLE_MAX, SINGLE_MAX + 1, 2 * SINGLE_MAX + 3, (1 << 20) + 7)


def _stride(n):
    """elements one pass of the kernel that enqueue_best takes for n covers"""
    return 1024 if n <= SINGLE_MAX else min((n + 255) // 256, 1024) * 256


def _pairs(n):
    """positions (i < j) of a maximum planted twice"""
    st = _stride(n)
    mid = (n // 2) & ~63
    cand = [("adjacent lanes", 5, 6), ("adjacent lanes, middle", mid + 5, mid + 6), ("lanes 63 and 64", 63, 64),
            ("lanes 63 and 64, middle", mid + 63, mid + 64), ("end of one stride, start of the next", st - 1, st),
            ("same thread, two passes", 7, 7 + st), ("same thread, last pass", 1, 1 + ((n - 2) // st) * st), ("first and last", 0, n - 1)]
    if n > SINGLE_MAX:
        cand += [("two workgroups", 100, 256 * 7 + 100), ("two workgroups, far", 256 * 3 + 9, n - 256 * 5)]
    return [(w, i, j) for w, i, j in cand if 0 <= i < j < n]


def _patterns(n, seed):
    rng = np.random.default_rng(seed)
    u = (rng.random(n, dtype=np.float32) * np.float32(0.5) + np.float32(0.25)).astype(np.float32)     # in [0.25, 0.75): 0.875 is above all
    top = np.float32(0.875)
    out = []
    for what, i, j in _pairs(n):
        s = u.copy(); s[i] = s[j] = top
        out.append(("twice: " + what, s, i))
        s = u.copy(); s[j] = top
        out.append(("once at the later of: " + what, s, j))
    s = u.copy(); s[0] = top
    out.append(("maximum first", s, 0))
    s = u.copy(); s[n - 1] = top
    out.append(("maximum last", s, n - 1))
    out.append(("all zero", np.zeros(n, np.float32), -1))
    s = -u; s[::3] = np.nan; s[1::7] = np.float32(-0.0)
    out.append(("negative, NaN and -0.0", s.copy(), -1))
    k = (2 * n) // 3
    s[k] = np.float32(1e-45)            # the smallest denormal: bits 1
    out.append(("one denormal among them", s.copy(), k))
    s = u.copy(); s[n - 1] = np.nan; s[k] = np.inf
    out.append(("one +inf", s, k))
    return out


@pytest.fixture(scope="module")
def argmax_ctx():
    d = _Dev("tiny", 16)
    d.dS = d.est.dev_alloc(4 * ARGMAX_SIZES[-1])
    yield d
    d.est.dev_free(d.dS)
    d.close()


def _both_entry_points(d, n, off, want, what):
    key, (s, gid) = want
    assert d.est.best_device(d.dS, n, off) == (s, gid, key), (what, hex(d.est.best_device(d.dS, n, off)[2]), hex(key))
    d.est.dev_upload(d.dK, np.array([0xFFFFFFFFFFFFFFFF], np.uint64))
    d.est.best_device_async(d.dS, n, off, d.dK.value)
    got = np.zeros(1, np.uint64)
    d.est.dev_download(d.dK, got)
    assert int(got[0]) == key, (what, "async", hex(int(got[0])), hex(key))


@pytest.mark.parametrize("n", ARGMAX_SIZES)
def test_argmax_kernels_equal_the_rule(argmax_ctx, n):
    from model_matching_amd import dist as sd
    d = argmax_ctx
    L = d.est.L
    assert int(np.float32(1e-45).view(np.uint32)) == 1
    offsets = (0, 1000, 1 << 31, (1 << 32) - n)          # the last: the final element's id is 0xFFFFFFFF, the low key word 0
    for what, s, winner in _patterns(n, 1000 + n % 977):
        d.est.dev_upload(d.dS, s)
        for off in offsets:
            want = _key_rule(s, off)
            key, (sc, gid) = want
            assert gid == (off + winner if winner >= 0 else -1), (n, what, off)
            _both_entry_points(d, n, off, want, (n, what, off))
            # the host forms of the key
            if key:
                assert int(L.stocs_pack_best(C.c_float(sc), C.c_uint32(gid))) == key == sd.pack_best(sc, gid), (n, what, off)
                fs, fi = C.c_float(0), C.c_uint32(0)
                L.stocs_unpack_best(C.c_uint64(key), C.byref(fs), C.byref(fi))
                assert (fs.value, int(fi.value)) == (sc, gid) == sd.unpack_best(key), (n, what, off)
            else:
                assert int(L.stocs_pack_best(C.c_float(0.0), C.c_uint32(off))) == 0 == sd.pack_best(0.0, off)
    if n == ARGMAX_SIZES[-1]:
        s = np.zeros(n, np.float32); s[n - 1] = np.float32(0.5)
        d.est.dev_upload(d.dS, s)
        assert d.est.best_device(d.dS, n, (1 << 32) - n)[2] == (int(_bits(s[n - 1:])[0]) << 32)      # low word 0, key not 0


def test_argmax_key_word_is_not_left_over(argmax_ctx):
    """the context's key word is shared by every stocs_best_device call: after a many-workgroup call (zero fill + atomic max) a smaller
    all-zero array gives key 0, whichever kernel takes it"""
    d = argmax_ctx
    big = SINGLE_MAX + 1
    s = np.zeros(big, np.float32); s[big - 1] = np.float32(0.75)
    for small in (65, SINGLE_MAX, SINGLE_MAX + 1):
        d.est.dev_upload(d.dS, s)
        assert d.est.best_device(d.dS, big, 5)[:2] == (0.75, 5 + big - 1)
        d.est.dev_upload(d.dS, np.zeros(small, np.float32))
        assert d.est.best_device(d.dS, small) == (0.0, -1, 0), small
        d.est.dev_upload(d.dS, s)
    # and the other way round: the key of a one-workgroup call does not join the atomic max of the next
    d.est.dev_upload(d.dS, np.full(64, 0.9, np.float32))
    assert d.est.best_device(d.dS, 64)[:2] == (float(np.float32(0.9)), 0)
    d.est.dev_upload(d.dS, s)
    assert d.est.best_device(d.dS, big)[:2] == (0.75, big - 1)


# ---- C. batched detail rows through the hit count ----
HIT_SIZES = (1, 2, 3, 5, 7, 37)


def _hit_candidates(d, n):
    from model_matching_amd import synth
    T = synth.make_candidates(d.Tgt, n)
    far = np.eye(4); far[:3, 3] = [50.0, -40.0, 30.0]
    T[1] = far.T.reshape(16).astype(np.float32)          # far outside the scene grid: no hit
    T[2, 12] = np.nan
    T[0] = d.Tgt.T.reshape(16).astype(np.float32)        # the ground truth: many hits
    return T


@pytest.mark.parametrize("name", ["tiny", "small", "dense"])
def test_hit_count_equals_the_detail_rows(name):
    """stocs_lcp_hit_count launches the detail forms on batches (four candidates per 256-thread workgroup, ragged n); stocs_lcp_detail
    launches them one candidate at a time.  The two totals must be the sums over the single rows, form by form."""
    d = _Dev(name, HIT_SIZES[-1])
    T = _hit_candidates(d, HIT_SIZES[-1])
    d.upload(T)
    try:
        for cull in (0, 2):
            for variant in (99, 0):          # (a dense grid has no plain detail kernel: variant 0 runs the per-step one there)
                d.est.set_option("lcp_cull", cull); d.est.set_option("lcp_variant", variant)
                rows = [d.est.lcp_detail(T[i]) for i in range(len(T))]
                hits = np.array([int((h >= 0).sum()) for h, c in rows]); counted = np.array([int(c.sum()) for h, c in rows])
                assert hits[0] > 0 and counted[0] > 0 and hits[1] == 0 and hits[2] == 0, (name, cull, variant)
                assert (counted <= hits).all()
                for n in HIT_SIZES:
                    assert d.est.lcp_hit_count(d.dT, n) == (int(hits[:n].sum()), int(counted[:n].sum())), (name, cull, variant, n)
    finally:
        d.close()


def test_hit_count_in_more_than_one_chunk():
    """stocs_lcp_hit_count cuts a batch into chunks of 256 MiB of rows (5 bytes per model point and candidate): a batch of one chunk
    and five candidates equals its two halves, which take one chunk each"""
    from model_matching_amd import synth
    chunk = (256 << 20) // (5 * 1000)
    n = chunk + 5
    d = _Dev("small", n)
    assert d.est.nM == 1000
    try:
        T = synth.make_candidates(d.Tgt, n)
        T[chunk - 1, 12] = np.nan
        T[chunk] = d.Tgt.T.reshape(16).astype(np.float32)     # the first candidate of the second chunk: the ground truth
        d.upload(T)
        whole = d.est.lcp_hit_count(d.dT, n)
        h = n // 2
        assert h < chunk and n - h < chunk
        first = d.est.lcp_hit_count(d.dT, h)
        second = d.est.lcp_hit_count(C.c_void_p(d.dT.value + h * 64), n - h)
        assert whole == (first[0] + second[0], first[1] + second[1])
        assert whole[0] > 0 and 0 < whole[1] <= whole[0]
        # the second chunk alone: its five candidates one by one
        rows = [d.est.lcp_detail(T[i]) for i in range(chunk, n)]
        tail = d.est.lcp_hit_count(C.c_void_p(d.dT.value + chunk * 64), 5)
        assert tail == (sum(int((hh >= 0).sum()) for hh, c in rows), sum(int(c.sum()) for hh, c in rows))
        head = d.est.lcp_hit_count(d.dT, chunk)
        assert whole == (head[0] + tail[0], head[1] + tail[1])
    finally:
        d.close()
