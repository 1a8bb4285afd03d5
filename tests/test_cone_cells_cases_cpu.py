"""The query sets of test_cone_cells_gpu.py (cone_cells_cases.py) checked against themselves on the CPU: the adversarial set does sit on the
cell boundaries, the cone fields computed in Python are the library's, the numpy float32 restatements of quat_from_z and cone_cell_exact
give the host's exact bitsets, and the host's evaluation of the filter never disagrees on either set.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cone_cells_cases as cc  # noqa: E402


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


@pytest.fixture(scope="module")
def sets():
    nr, cr, special = cc.random_queries()
    na, ca, target = cc.adversarial_queries()
    return {"random": (nr, cr), "adversarial": (na, ca)}, special, target


def test_adversarial_queries_sit_on_the_cell_boundaries(sets):
    (na, ca), target = sets[0]["adversarial"], sets[2]
    share, reached, dist = cc.adversarial_condition(na, ca)
    assert len(na) == cc.N_QUERIES and share >= 0.5, share
    assert {(ax, k) for ax in range(3) for k in range(1, 7)} <= reached
    assert {(int(a), int(k)) for a, k, _ in target} == {(ax, k) for ax in range(3) for k in range(1, 7)}
    # the offsets land where they were aimed: the built sample's coordinate is |offset| from its integer, to float32 resolution of the normal
    want = np.abs(np.array(cc.OFFSETS))[target[:, 2]]
    assert np.all(dist.min(1) <= want + 2e-6), np.abs(dist.min(1) - want).max()
    assert (dist.min(1) < 2e-6).sum() >= 200                       # the crossings themselves


@pytest.mark.parametrize("name", ["random", "adversarial"])
def test_restatements_equal_the_host_library(capi, sets, name):
    L = capi.load()
    nrm, ca = sets[0][name]
    nb, sa = cc.cone_fields(ca)
    d, valid = cc.samples(ca, nb, sa)
    q, branch = cc.quat_float32(nrm)
    ids = np.where(valid, cc.cell_ids(cc.t_exact_float32(q, d)), -1)
    bits = np.zeros((len(nrm), 11), np.uint32)
    i, a = np.nonzero(ids >= 0)
    np.bitwise_or.at(bits, (i, ids[i, a] >> 5), np.uint32(1) << (ids[i, a] & 31).astype(np.uint32))
    ex, ke = (C.c_uint32 * 11)(), (C.c_uint32 * 11)()
    ns, nu = C.c_int(), C.c_int()
    und = 0
    for k in range(len(nrm)):
        v = np.ascontiguousarray(nrm[k], np.float32)
        assert L.stocs_cone_cells_host(v.ctypes.data_as(capi._fp), C.c_float(ca[k]), ex, ke, C.byref(ns), C.byref(nu)) == 0
        assert ns.value == nb[k], (k, ca[k])
        assert list(ex) == list(ke) == bits[k].tolist(), (k, nrm[k], ca[k])
        und += nu.value
    if name == "random":
        assert und < 1e-3 * nb.sum() and 200 < branch.sum() < 1000
        sp = sets[1]
        assert all(branch[sp["c_below_" + c]] and not branch[sp["c_at_" + c]] and not branch[sp["c_above_" + c]] and branch[sp["minus_z_" + c]] for c in ("0.3", "-0.6"))
    else:
        assert und > 5e-3 * nb.sum() and not branch.any()
