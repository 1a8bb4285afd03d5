"""Reference for stocs_select_instances / stocs_select_instances_rows (include/stocs_hip.h): the contract's steps on given detail rows,
in python sets and one float32 multiply.  Depends on numpy alone.  Not a test module."""
import numpy as np

DTYPE = np.dtype([("rank", np.int32), ("own", np.int32), ("exclusive", np.int32), ("lcp", np.float32)])


def pack_best(lcp, index):
    """stocs_pack_best: (score bits << 32) | ~index for a positive score, else 0"""
    l = np.float32(lcp)
    if not l > 0:
        return 0
    return (int(np.array(l).view(np.uint32)) << 32) | (0xFFFFFFFF - int(index))


def explained_sets(hit, counted, valid=None):
    """step 1 (and 2): E_h as python sets; an invalid hypothesis explains nothing"""
    hit = np.asarray(hit).reshape(len(hit), -1)
    counted = np.asarray(counted).reshape(len(counted), -1)
    return [set(np.unique(hit[h][counted[h] != 0]).tolist()) if (valid is None or valid[h]) else set() for h in range(len(hit))]


def order_of(lcp):
    """step 3: descending key, lower index first among equal keys (equal keys exist only at 0)"""
    return sorted(range(len(lcp)), key=lambda h: (-pack_best(lcp[h], h), h))


def passes(excl, own, min_points, min_fraction):
    return excl >= min_points and bool(np.float32(excl) >= np.float32(min_fraction) * np.float32(own))


def select(hit, counted, lcp, max_instances=16, min_points=20, min_exclusive_fraction=0.5, valid=None, early=None):
    """-> (records (n,) DTYPE, selected (k,) int32 in rank order).
    valid (n,) bools: step 2's flags (None: all valid).  early: a numpy Generator -- before every step of the walk some pending
    hypotheses further down the order are tested against the cover of the moment and dropped for good when they fail (what a parallel
    walk does); the results may not depend on it."""
    n = len(lcp)
    lcp = np.array(lcp, np.float32).reshape(n)
    if valid is not None:
        lcp = np.where(np.asarray(valid, bool), lcp, np.float32(0)).astype(np.float32)
    E = explained_sets(hit, counted, valid) if n else []
    order = order_of(lcp)
    rec = np.zeros(n, DTYPE)
    rec["rank"] = -1
    rec["lcp"] = lcp
    covered, selected, dropped = set(), [], set()
    for pos, h in enumerate(order):
        if len(selected) >= max_instances:
            break
        if early is not None and pos + 1 < n:
            for g in early.choice(order[pos + 1:], size=min(3, n - pos - 1), replace=False):
                if not passes(len(E[g] - covered), len(E[g]), min_points, min_exclusive_fraction):
                    dropped.add(int(g))
        if h in dropped:
            continue
        excl = len(E[h] - covered)
        if passes(excl, len(E[h]), min_points, min_exclusive_fraction):
            rec["rank"][h] = len(selected)
            rec["exclusive"][h] = excl
            selected.append(h)
            covered |= E[h]
    for h in range(n):
        rec["own"][h] = len(E[h])
        if rec["rank"][h] < 0:
            rec["exclusive"][h] = len(E[h] - covered)
    return rec, np.array(selected, np.int32)


def records_equal(a, b):
    """integer fields equal, the score bit for bit"""
    a = np.asarray(a); b = np.asarray(b)
    return (a.shape == b.shape and all(np.array_equal(a[f], b[f]) for f in ("rank", "own", "exclusive"))
            and np.array_equal(np.ascontiguousarray(a["lcp"]).view(np.uint32), np.ascontiguousarray(b["lcp"]).view(np.uint32)))
