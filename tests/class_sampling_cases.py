"""Case table and scene builders of the class-mode sampling edge tests (tests/test_class_sampling_cases_cpu.py checks them with the
oracle alone, tests/test_class_sampling_edges_gpu.py runs them on the device).  No GPU, no library call: numpy and model_matching_amd.synth.

The sizes sit on both sides of every number at which sample.hip takes another kernel form or another trip count of a chunked loop:
63/64/65 (lean_usable, the 64-lane search), 2047..2049 (one draw pass), 4095..4097 (one compaction trip), 8000/8001 (256 -> 512 threads),
8192/8193 (one prior load), 24000/24001 (512 -> 1024 threads), 26000/26001 (working set in LDS -> device memory).  The form rule restated
in expected_form() is the one documented at stocs_last_sampling_form in include/stocs_hip.h."""
import functools

import numpy as np

from model_matching_amd import synth

SIZES = (63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 8000, 8001, 8192, 8193, 24000, 24001, 26000, 26001)
SEED = 4242               # sizes
SEED_PRIOR = 7            # degenerate priors
PRIOR_SIZES = (1500, 8001)
POINT1_SIZES = (64, 65, 4096, 4097, 26000)
PRIORS = ("all_zero", "only_first", "only_last", "all_below_resolution", "clutter_below_resolution", "clutter_zero", "all_one",
          "every_second_zero", "object_at_end")
ZERO_TOTAL = ("all_zero", "all_below_resolution")                      # the draw's total is zero: point 1 is -1
NO_VALID = ("all_zero", "only_first", "only_last", "all_below_resolution")   # no attempt can find four points
BELOW_RESOLUTION = np.float32(1e-11)                                   # < 2^-32: non-zero as a float, zero for the draw
LEAN_MIN_S, LEAN_QUARTER_S, LEAN_HALF_S, LDS_MAX_S = 64, 8000, 24000, 26000
FIRST, LAST = 40, 8       # attempts of a call compared with the oracle: its first 40 and its last 8


@functools.lru_cache(maxsize=None)
def model():
    return synth.make_model(400, seed=synth.SEED_MODEL + 7)            # the model of synth.workload("tiny")


@functools.lru_cache(maxsize=None)
def scene(n):
    return synth.make_scene(model(), n, seed=synth.SEED_SCENE + 7)     # n = 1500 is the scene of synth.workload("tiny")


def n_attempts_many(n):
    """attempts of a call that prefers the lean kernel (> 256).  The 63..65-point scenes hold a 16-point object of which a few
    attempts in a hundred find a base: they run 400 attempts, and all of them are compared (the oracle needs microseconds there)."""
    return 400 if n <= 65 else 257


def n_attempts_few(n):
    """attempts of a call that does not (<= 256 on a fresh context)"""
    return 256 if n <= 65 else 40


def compared_attempts(n_attempts, n):
    if n <= 65:
        return list(range(n_attempts))
    return sorted(set(range(min(FIRST, n_attempts))) | set(range(max(0, n_attempts - LAST), n_attempts)))


def with_prior(sc, kind):
    """-> (pos, nrm, prob, pixel) of scene sc under the prior `kind`.  Only object_at_end moves points: the object's n_object points go
    behind the clutter, in their order."""
    S, k = len(sc.pos), sc.n_object
    pos, nrm, pix, own = sc.pos, sc.nrm, sc.pixel, sc.prob.astype(np.float32)
    p = np.zeros(S, np.float32)
    if kind == "own":
        p = own.copy()
    elif kind == "all_zero":
        pass
    elif kind == "only_first":
        p[0] = own[0]
    elif kind == "only_last":
        p[S - 1] = own[S - 1]
    elif kind == "all_below_resolution":
        p[:] = BELOW_RESOLUTION
    elif kind == "clutter_below_resolution":
        p[:k] = own[:k]; p[k:] = BELOW_RESOLUTION
    elif kind == "clutter_zero":
        p[:k] = own[:k]
    elif kind == "all_one":
        p[:] = 1.0
    elif kind == "every_second_zero":
        p = own.copy(); p[1::2] = 0.0
    elif kind in ("object_at_end", "object_at_end_own"):
        order = np.concatenate([np.arange(k, S), np.arange(k)])
        pos, nrm, pix = pos[order], nrm[order], pix[order]
        if kind == "object_at_end":
            p[S - k:] = own[:k]
        else:
            p = own[order]                                             # (the same positions under the scene's own weights: the prior-cache test)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(pos), np.ascontiguousarray(nrm), np.ascontiguousarray(p), np.ascontiguousarray(pix)


# ---- the form rule of include/stocs_hip.h (stocs_last_sampling_form), restated ----
def a16(x):
    return (x + 15) // 16 * 16


def expected_form(S, env=(), n_attempts=257, prefix_sums_current=False, batch=False, cap_env=None):
    """-> dict(kernel, threads, lds_bytes, cap, launches) for a scene of S points; env: the STOCS_* switches set."""
    env = set(env)
    if "STOCS_CLASS_MULTI_KERNEL" in env and not batch:
        return dict(kernel="nine_launch", threads=0, lds_bytes=0, cap=0, launches=0)
    lds_ok = S <= LDS_MAX_S and "STOCS_INSTANCE_NO_LDS" not in env
    wants = batch or n_attempts > 256 or prefix_sums_current or "STOCS_CLASS_LEAN_KERNEL" in env
    if lds_ok and wants and S >= LEAN_MIN_S and "STOCS_CLASS_FULL_KERNEL" not in env:
        threads = 256 if S <= LEAN_QUARTER_S else (512 if S <= LEAN_HALF_S else 1024)
        if "STOCS_CLASS_LEAN_512" in env:
            threads = max(threads, 512)
        if "STOCS_CLASS_LEAN_1024" in env:
            threads = 1024
        top = {256: 16384, 512: 36864, 1024: 76800}[threads]
        lds = max(a16(2 * S), min(top, a16(6 * S + 16)))
        cap = min(S + 1, (lds - 8) // 6) // 2 * 2
        if cap_env is not None:
            cap = max(2, min(cap, cap_env // 2 * 2))
        return dict(kernel="lean", threads=threads, lds_bytes=lds, cap=cap, launches=1)
    if lds_ok:
        return dict(kernel="full_lds", threads=1024, lds_bytes=a16(4 * S) + 2 * S + 16, cap=0, launches=1)
    per = max(1, min(n_attempts, (1 << 30) // (8 * S))) if batch else n_attempts
    return dict(kernel="full_device_memory", threads=1024, lds_bytes=0, cap=0, launches=-(-n_attempts // per))


def form_cases():
    """-> [(id, S, env tuple, attempts, fresh context)]: every size with every form it can reach."""
    out = []
    for S in SIZES:
        out.append(("%d-few" % S, S, (), n_attempts_few(S), True))
        out.append(("%d-many" % S, S, (), n_attempts_many(S), False))
        if LEAN_MIN_S <= S <= LEAN_QUARTER_S:
            out.append(("%d-lean512" % S, S, ("STOCS_CLASS_LEAN_512",), n_attempts_many(S), False))
        if LEAN_MIN_S <= S <= LEAN_HALF_S:
            out.append(("%d-lean1024" % S, S, ("STOCS_CLASS_LEAN_1024",), n_attempts_many(S), False))
        out.append(("%d-full" % S, S, ("STOCS_CLASS_FULL_KERNEL",), n_attempts_many(S), False))
        out.append(("%d-no_lds" % S, S, ("STOCS_INSTANCE_NO_LDS",), n_attempts_many(S), False))
        out.append(("%d-nine" % S, S, ("STOCS_CLASS_MULTI_KERNEL",), n_attempts_many(S), False))
    return out


# ---- point 1: the draw's fixed-point arithmetic as oracle/stocs_oracle.h states it (W_i = (uint64)(w_i * 2^32)) ----
def fixed_weights(prior):
    """-> list of Python ints W_i (0 for w <= 0)"""
    w = np.asarray(prior, np.float32).astype(np.float64)
    return [int(v * 4294967296.0) if v > 0 else 0 for v in w.tolist()]


def mulhi64(a, b):
    return (a * b) >> 64


def boundary_indices(S):
    """64 scene indices spread over the scene: first, last, around every multiple of 4096, and around multiples of 64"""
    idx = {0, S - 1}
    for m in range(4096, S + 1, 4096):
        idx.update(i for i in (m - 1, m, m + 1) if 0 <= i < S)
    mult64 = list(range(64, S, 64))
    step = max(1, len(mult64) // 24)
    for m in mult64[::step]:
        if len(idx) >= 63:
            break
        idx.update(i for i in (m - 1, m) if 0 <= i < S)
    extra = np.linspace(0, S - 1, 64).astype(int).tolist()
    for i in extra:
        if len(idx) >= 64:
            break
        idx.add(i)
    return sorted(idx)[:64]


def boundary_words(prior):
    """For the inclusive prefix sum c of each boundary index: the smallest 64-bit word r with mulhi64(r, total) == c - 1 and the
    smallest with == c (r = ceil(t * 2^64 / total)), each verified; targets outside [0, total) have no word and are left out."""
    W = fixed_weights(prior)
    total = sum(W)
    if total == 0:
        return []
    pre, c = [], 0
    for v in W:
        c += v
        pre.append(c)
    words = []
    for i in boundary_indices(len(W)):
        for t in (pre[i] - 1, pre[i]):
            if not 0 <= t < total:
                continue
            r = -(-(t << 64) // total)
            if r >= 1 << 64:
                continue
            assert mulhi64(r, total) == t and (r == 0 or mulhi64(r - 1, total) == t - 1), (i, t)
            words.append(r)
    return words


def point1_words(prior, rng_seed=11):
    rng = np.random.default_rng(rng_seed)
    rand = [int(x) for x in rng.integers(0, 1 << 64, 200, dtype=np.uint64)]
    return [0, 1, 1 << 63, (1 << 64) - 2, (1 << 64) - 1] + rand + boundary_words(prior)


# ---- the overflow edge: survivors of pass 1 per attempt, from the oracle alone ----
def survivor_counts(oracle_lib, orc, prior, seed, n_attempts):
    """-> (first point, survivors of pass 1) per attempt: point 1 is orc_draw(prior, rng(seed, attempt, 0)), the survivors are the
    non-zero weights Oracle.class_pass(1, ...) leaves of the prior.  first point -1 (count 0) when the draw fails."""
    import ctypes as C
    L = oracle_lib.lib()
    w = np.ascontiguousarray(prior, np.float32)
    pw = w.ctypes.data_as(C.POINTER(C.c_float))
    first, count = [], []
    for a in range(n_attempts):
        b1 = L.orc_draw(pw, len(w), L.orc_rng(seed, a, 0))
        first.append(b1)
        count.append(int(np.count_nonzero(orc.class_pass(1, np.array([b1, 0, 0], np.int32), w))) if b1 >= 0 else 0)
    return np.array(first), np.array(count)


def pick_overflow_attempt(counts, cap):
    """the first attempt whose survivor count k is even, >= 4 and fits the default list: the caps k, k - 2 and 2 are then all honoured"""
    for a, k in enumerate(counts.tolist()):
        if k % 2 == 0 and 4 <= k <= cap:
            return a, k
    raise AssertionError("no attempt with an even survivor count")
