"""The 16-point sub-patches of the model order (ctx.hip, host code): the unit of the scoring kernels' patch test at
lcp_cull_unit = 16.  The walk order is one permutation for both units, every 64-slot patch is the union of its four
16-slot runs, and every sub-patch sphere contains its points in the float-centred frame the library scores in."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def capi():
    import os
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def _centred(pos):
    c = np.zeros(3, np.float32)
    for p in pos:                                   # centroid_shift: sequential float sums (stocs.cpp:943-964)
        c = (c + p).astype(np.float32)
    return (pos - (c / np.float32(len(pos))).astype(np.float32)).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("n", [1, 15, 63, 64, 130, 1000, 5000])
def test_subpatch_spheres_contain_their_points(capi, n):
    from model_matching_amd import synth
    L = capi.load()
    m = synth.make_model(max(n, 400), seed=7 + n)
    pos = np.ascontiguousarray(m.pos[:n], np.float32)
    npat, nsub = (n + 63) // 64, (n + 15) // 16
    perm64 = np.zeros(n, np.int32); pat = np.zeros((npat, 4), np.float32)
    assert L.stocs_model_patch_order(pos.ctypes.data_as(capi._fp), n, perm64.ctypes.data_as(capi._ip), pat.ctypes.data_as(capi._fp)) == 0
    perm = np.zeros(n, np.int32); sub = np.zeros((nsub, 4), np.float32)
    assert L.stocs_model_subpatches(pos.ctypes.data_as(capi._fp), n, perm.ctypes.data_as(capi._ip), sub.ctypes.data_as(capi._fp)) == 0
    assert sorted(perm.tolist()) == list(range(n))
    assert np.array_equal(perm, perm64)             # one walk order for both units
    cen = _centred(pos)
    for q in range(nsub):
        pts = cen[perm[16 * q: 16 * q + 16]]
        assert np.isfinite(sub[q]).all() and sub[q, 3] >= 0.0
        assert np.linalg.norm(pts - sub[q, :3].astype(np.float64), axis=1).max() <= float(sub[q, 3]) + 1e-7, q
    for j in range(npat):                           # a patch's four runs are its own points: its sphere holds all of them
        pts = cen[perm[64 * j: 64 * j + 64]]
        assert np.linalg.norm(pts - pat[j, :3].astype(np.float64), axis=1).max() <= float(pat[j, 3]) + 1e-7, j
    if n >= 1000:                                   # the runs are compact: well below the radius of their patches
        assert np.median(sub[:, 3]) < 0.7 * np.median(pat[:, 3])


def test_invalid_arguments(capi):
    L = capi.load()
    pos = np.zeros(30, np.float32); perm = np.zeros(10, np.int32); sub = np.zeros(4, np.float32)
    assert L.stocs_model_subpatches(None, 10, perm.ctypes.data_as(capi._ip), sub.ctypes.data_as(capi._fp)) == -1
    assert L.stocs_model_subpatches(pos.ctypes.data_as(capi._fp), 0, perm.ctypes.data_as(capi._ip), sub.ctypes.data_as(capi._fp)) == -1
    assert L.stocs_model_subpatches(pos.ctypes.data_as(capi._fp), 10, None, sub.ctypes.data_as(capi._fp)) == -1
    assert L.stocs_model_subpatches(pos.ctypes.data_as(capi._fp), 10, perm.ctypes.data_as(capi._ip), sub.ctypes.data_as(capi._fp)) == 0
    assert sorted(perm.tolist()) == list(range(10)) and sub[3] >= 0.0    # ten coincident points: a sphere of radius ~0
