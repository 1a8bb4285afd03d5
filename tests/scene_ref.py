"""float32 / integer numpy restatement of the scene-selection contract written at stocs_scene_footprints and stocs_scene_select in
include/stocs_hip.h.  The footprints are built on render_ref (one pose rendered alone into a cleared key buffer, then classified) and so
on depth_check_ref.point_flags; the walk is a plain sequential loop over python sets.  Written from the contract, not from the kernels;
the GPU tests compare the library's rows and records with it for equality.  Depends on numpy alone.  Not a test module."""
import numpy as np

import render_ref as rref

F = np.float32
RECORD = ("footprint", "no_depth", "agree", "in_front", "behind", "on_mask", "claimed")
RECORD_DTYPE = np.dtype([(k, np.int32) for k in RECORD])
RESULT = ("rank", "own", "exclusive", "reason")
RESULT_DTYPE = np.dtype([(k, np.int32) for k in RESULT])
DEFAULTS = dict(max_selected=64, min_pixels=50, min_exclusive_fraction=0.5, max_violation_fraction=0.2)
CLAIMS = {"agree": 0, "on_mask": 1}


def row_words(npix):
    """Wr: ceil(npix / 32) rounded up to a multiple of 4"""
    return ((npix + 31) // 32 + 3) // 4 * 4


def pack_rows(masks):
    """(n, npix) booleans -> (n, Wr) uint32: pixel i is bit i & 31 of word i >> 5, padding bits zero"""
    masks = np.asarray(masks, bool).reshape(len(masks), -1)
    n, npix = masks.shape
    bits = np.zeros((n, row_words(npix) * 32), np.uint8)
    bits[:, :npix] = masks
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(n, -1)


def unpack_rows(rows, npix):
    """(n, Wr) uint32 -> (n, npix) booleans; the padding bits must be zero"""
    rows = np.ascontiguousarray(rows, "<u4")
    bits = np.unpackbits(rows.view(np.uint8).reshape(len(rows), -1), axis=1, bitorder="little").astype(bool)
    assert not bits[:, npix:].any(), "padding bits set"
    return bits[:, :npix]


def footprints(poses16, model_pos, model_nrm, depth_u16, prob_u16, K, depth_scale, claim="agree", **render_params):
    """stocs_scene_footprints -> (records (n,) RECORD_DTYPE, masks (n, npix) booleans of the claimed pixels, z (n, npix) uint32: the
    bits of Z_h, all ones where pose h touches nothing)"""
    H, W = depth_u16.shape
    P = np.asarray(poses16, F).reshape(-1, 16)
    rec = np.zeros(len(P), RECORD_DTYPE)
    masks = np.zeros((len(P), H * W), bool)
    z = np.full((len(P), H * W), 0xFFFFFFFF, np.uint32)
    for h in range(len(P)):
        zkey = rref.render(rref.empty_keys(W, H), P[h], model_pos, model_nrm, K, W, H, 0, True, **render_params)   # this pose alone
        st = rref.classify(zkey, depth_u16, prob_u16, depth_scale, **render_params)
        touched = zkey != rref.EMPTY
        z[h][touched] = (zkey[touched] >> np.uint64(32)).astype(np.uint32)
        masks[h] = (st & 15) == 2 if CLAIMS[claim] == 0 else (st & 16) != 0
        rec[h] = (int(touched.sum()), int(((st & 15) == 1).sum()), int(((st & 15) == 2).sum()), int(((st & 15) == 3).sum()), int(((st & 15) == 4).sum()),
                  int(((st & 16) != 0).sum()), int(masks[h].sum()))
    return rec, masks, z


def default_score(rec):
    """float32(agree) / float32(footprint), 0 where the footprint is empty"""
    s = np.zeros(len(rec), F)
    some = rec["footprint"] > 0
    s[some] = rec["agree"][some].astype(F) / rec["footprint"][some].astype(F)
    return s


def pack_best(score, index):
    """stocs_pack_best: (score bits << 32) | ~index for a positive score, else 0"""
    s = F(score)
    if not s > 0:
        return 0
    return (int(np.array(s).view(np.uint32)) << 32) | (0xFFFFFFFF - int(index))


def order_of(score):
    return sorted(range(len(score)), key=lambda h: (-pack_best(score[h], h), h))


def _prm(params):
    prm = dict(DEFAULTS); prm.update(params)
    return prm


def eligible(score, own, rec, prm):
    s = F(score)
    return bool(s > 0) and own >= prm["min_pixels"] and bool(F(rec["in_front"]) <= F(prm["max_violation_fraction"]) * F(rec["footprint"]))


def passes(excl, own, prm):
    return excl >= prm["min_pixels"] and bool(F(excl) >= F(prm["min_exclusive_fraction"]) * F(own))


def _finish(A, score, group, rec, cap, prm, order, rank, excl_at, covered, cnt):
    """the records from the FINAL state"""
    n = len(A)
    out = np.zeros(n, RESULT_DTYPE)
    for h in range(n):
        own = len(A[h])
        if rank[h] >= 0:
            out[h] = (rank[h], own, excl_at[h], 0)
            continue
        ex = len(A[h] - covered)
        if not eligible(score[h], own, rec[h], prm):
            reason = 1
        elif not passes(ex, own, prm):
            reason = 2
        elif cap is not None and cnt[group[h]] >= cap[group[h]]:
            reason = 3
        else:
            reason = 4
        out[h] = (-1, own, ex, reason)
    return out


def select(masks, score, group, rec, n_groups, group_cap=None, per_round=None, **params):
    """stocs_scene_select on (n, npix) boolean masks -> (records (n,) RESULT_DTYPE, selected (k,) int32 in rank order).
    per_round None: the contract's sequential walk.  per_round = k: the walk as a kernel that tests k pending slots per round against
    the state at the start of the round, selects the first that passes, drops those before it and tests those behind it again -- the
    results may not depend on it."""
    prm = _prm(params)
    masks = np.asarray(masks, bool).reshape(len(score), -1) if len(score) else np.zeros((0, 0), bool)
    n = len(score)
    A = [set(np.flatnonzero(masks[h]).tolist()) for h in range(n)]
    score = np.asarray(score, F).reshape(n)
    group = np.asarray(group, np.int64).reshape(n)
    cap = None if group_cap is None else [int(c) for c in group_cap]
    order = order_of(score)
    rank, excl_at = [-1] * n, [0] * n
    covered, cnt, selected = set(), [0] * n_groups, []

    def test(h):
        own = len(A[h])
        ex = len(A[h] - covered)
        ok = eligible(score[h], own, rec[h], prm) and (cap is None or cnt[group[h]] < cap[group[h]]) and passes(ex, own, prm)
        return ok, ex

    def take(h, ex):
        rank[h] = len(selected); excl_at[h] = ex
        selected.append(h)
        covered.update(A[h]); cnt[group[h]] += 1

    if per_round is None:
        for h in order:
            if len(selected) >= prm["max_selected"]:
                break
            ok, ex = test(h)
            if ok:
                take(h, ex)
    else:
        p = 0
        while p < n and len(selected) < prm["max_selected"]:
            res = [test(h) for h in order[p:p + per_round]]          # all against the state at the start of the round
            first = next((k for k, (ok, _) in enumerate(res) if ok), None)
            if first is None:
                p += per_round
            else:
                take(order[p + first], res[first][1])
                p += first + 1
    return _finish(A, score, group, rec, cap, prm, order, rank, excl_at, covered, cnt), np.array(selected, np.int32)


def records_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype.names == b.dtype.names and all(np.array_equal(a[f], b[f]) for f in a.dtype.names)
