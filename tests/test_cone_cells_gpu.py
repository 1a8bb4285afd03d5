"""The cone colouring of the congruent join as the DEVICE evaluates it (stocs_cone_cells_device: one lane per query through the shared
functions of csrc/cone_cells.h, in join_one's order) against the host's exact arithmetic, bit for bit, and against a float64 evaluation
of the same cell coordinates: the filter may only ever decide a sample whose cell the reference's arithmetic gives too, and the
inequality that guarantees it -- (filter's error) + (exact arithmetic's error) < STOCS_CONE_MARGIN -- is measured and asserted.

On the device the filter's reciprocal square root is the hardware approximation (__frsqrt_rn) and its FMAs are __fmaf_rn; the host test
(test_abi_cpu.py) sees 1 / sqrtf and libm's fmaf instead.  Inputs and references: cone_cells_cases.py.  Measured figures:
profiles/cone_filter_device.md."""
import ctypes as C

import numpy as np
import pytest

import cone_cells_cases as cc

pytestmark = pytest.mark.gpu

U32P = C.POINTER(C.c_uint32)


def _host(L, capi, nrm, ca):
    ex, ke = (C.c_uint32 * 11)(), (C.c_uint32 * 11)()
    ns, nu = C.c_int(), C.c_int()
    E, K = np.zeros((len(nrm), 11), np.uint32), np.zeros((len(nrm), 11), np.uint32)
    NS, NU = np.zeros(len(nrm), np.int32), np.zeros(len(nrm), np.int32)
    for i in range(len(nrm)):
        v = np.ascontiguousarray(nrm[i], np.float32)
        assert L.stocs_cone_cells_host(v.ctypes.data_as(capi._fp), C.c_float(ca[i]), ex, ke, C.byref(ns), C.byref(nu)) == 0
        E[i], K[i], NS[i], NU[i] = list(ex), list(ke), ns.value, nu.value
    return E, K, NS, NU


def _device(L, capi, nrm, ca):
    n = len(nrm)
    nrm, ca = np.ascontiguousarray(nrm, np.float32), np.ascontiguousarray(ca, np.float32)
    o = dict(exact=np.full((n, 11), 0xDEADBEEF, np.uint32), kernel=np.full((n, 11), 0xDEADBEEF, np.uint32), ns=np.full(n, -7, np.int32),
             nu=np.full(n, -7, np.int32), q=np.full((n, 4), 77, np.float32), fid=np.full((n, cc.MAX_CONE), -7, np.int32),
             eid=np.full((n, cc.MAX_CONE), -7, np.int32), t=np.full((n, cc.MAX_CONE, 3), 77, np.float32))
    rc = L.stocs_cone_cells_device(-1, nrm.ctypes.data_as(capi._fp), ca.ctypes.data_as(capi._fp), n, o["exact"].ctypes.data_as(U32P),
                                   o["kernel"].ctypes.data_as(U32P), o["ns"].ctypes.data_as(capi._ip), o["nu"].ctypes.data_as(capi._ip),
                                   o["q"].ctypes.data_as(capi._fp), o["fid"].ctypes.data_as(capi._ip), o["eid"].ctypes.data_as(capi._ip),
                                   o["t"].ctypes.data_as(capi._fp))
    assert rc == 0, L.stocs_last_error()
    return o


def _evaluate(L, capi, nrm, ca):
    host = _host(L, capi, nrm, ca)
    dev = _device(L, capi, nrm, ca)
    nb, sa = cc.cone_fields(ca)
    d, valid = cc.samples(ca, nb, sa)
    t64 = cc.t_float64(dev["q"], d)
    tx = cc.t_exact_float32(dev["q"], d)
    fin = valid & np.isfinite(t64).all(-1)                   # samples of finite queries
    with np.errstate(invalid="ignore"):
        e_f = float(np.abs(dev["t"].astype(np.float64) - t64)[fin].max())
        e_x = float(np.abs(tx.astype(np.float64) - t64)[fin].max())
    q32, branch = cc.quat_float32(nrm)
    return dict(nrm=nrm, ca=ca, host=host, dev=dev, nb=nb, d=d, valid=valid, t64=t64, tx=tx, fin=fin, e_f=e_f, e_x=e_x, q32=q32, branch=branch,
                undecided=float(dev["nu"].sum()) / float(nb.sum()))


@pytest.fixture(scope="module")
def sets():
    import __graft_entry__  # noqa: F401  (puts the repository root on the path)
    from model_matching_amd import capi
    L = capi.load()
    nr, cr, special = cc.random_queries()
    na, ca, target = cc.adversarial_queries()
    out = {"random": _evaluate(L, capi, nr, cr), "adversarial": _evaluate(L, capi, na, ca)}
    out["random"]["special"] = special
    out["adversarial"]["target"] = target
    for name, s in out.items():
        print("cone filter on the device, %s set: e_f = %.3e  e_x = %.3e  e_f + e_x = %.3e (margin %.1e)  undecided %.3e of %d samples"
              % (name, s["e_f"], s["e_x"], s["e_f"] + s["e_x"], cc.MARGIN, s["undecided"], int(s["nb"].sum())))
    return out


def test_the_adversarial_set_sits_on_the_cell_boundaries(sets):
    """From the float32 inputs, in float64: at least half of the adversarial queries have a sample coordinate within 2e-5 of an integer,
    on every axis and at every boundary k in 1..6."""
    s = sets["adversarial"]
    share, reached, _ = cc.adversarial_condition(s["nrm"], s["ca"])
    assert share >= 0.5, share
    assert {(ax, k) for ax in range(3) for k in range(1, 7)} <= reached, reached
    assert len(s["nrm"]) == len(sets["random"]["nrm"]) == 4096


@pytest.mark.parametrize("name", ["random", "adversarial"])
def test_device_exact_cells_equal_the_host_bit_for_bit(sets, name):
    """1. the exact path is the same IEEE operations on both sides: the device's exact bitset == stocs_cone_cells_host's, every query;
    the number of samples too; and per sample the device's exact cell == the numpy float32 restatement of cone_cell_exact."""
    s = sets[name]
    E, K, NS, NU = s["host"]
    dev = s["dev"]
    assert np.array_equal(dev["ns"], NS) and np.array_equal(dev["ns"], s["nb"])
    bad = np.nonzero((dev["exact"] != E).any(1))[0]
    assert not len(bad), (bad[:8], s["nrm"][bad[:8]], s["ca"][bad[:8]])
    ids = cc.cell_ids(s["tx"])
    assert np.array_equal(np.where(s["valid"], ids, -1), dev["eid"])
    assert (dev["fid"][~s["valid"]] == -1).all() and (dev["t"][~s["valid"]] == 0).all()


@pytest.mark.parametrize("name", ["random", "adversarial"])
def test_the_filter_never_decides_differently(sets, name):
    """2. what the join builds == the exact bitset, every query; per sample the filtered cell is -1 or the exact cell; the undecided count is
    the number of -1s; the host's evaluation of the filter builds the same set (it may be undecided on other samples)."""
    s = sets[name]
    dev, v = s["dev"], s["valid"]
    bad = np.nonzero((dev["kernel"] != dev["exact"]).any(1))[0]
    assert not len(bad), (bad[:8], s["nrm"][bad[:8]], s["ca"][bad[:8]])
    fid, eid = dev["fid"], dev["eid"]
    wrong = v & (fid != -1) & (fid != eid)
    assert not wrong.any(), (np.argwhere(wrong)[:8], fid[wrong][:8], eid[wrong][:8])
    assert np.array_equal((v & (fid == -1)).sum(1), dev["nu"])
    assert np.array_equal(s["host"][1], dev["kernel"])
    # the bitsets are the union of the per-sample cells
    for which, ids in (("exact", eid), ("kernel", np.where(fid >= 0, fid, eid))):
        bits = np.zeros_like(dev[which])
        i, a = np.nonzero(v & (ids >= 0))
        np.bitwise_or.at(bits, (i, ids[i, a] >> 5), np.uint32(1) << (ids[i, a] & 31).astype(np.uint32))
        assert np.array_equal(bits, dev[which]), which


def test_branch_points_of_the_quaternion_and_the_cone_table(sets):
    """The queries added by hand.  NaN normals colour nothing and every sample is undecided.  A ZERO normal is not such a case: normalized3
    leaves it alone (as Eigen's normalized() does), so c = 0, the axis is zero and q = (0, 0, 0, sqrt(2) / 2) -- a rotation by nothing;
    it colours exactly the cells of the query (0, 0, 1), whose q = (0, 0, 0, 1) (asserted so, bit for bit).  The exactly anti-parallel
    normal and the normals one float either side of c = -1 + 1e-5 take their branch (q compared with the branch's own formula);
    cos alpha = 1 and > 1 give no samples, the float below 1 two, -1 fifty-six."""
    s = sets["random"]
    dev, sp, nb = s["dev"], s["special"], s["nb"]
    for name in ("nan_x", "nan_all"):
        i = sp[name]
        assert nb[i] == 8 and dev["nu"][i] == 8 and not dev["exact"][i].any() and not dev["kernel"][i].any()
        assert (dev["fid"][i, :8] == -1).all() and (dev["eid"][i, :8] == -1).all()
    r2 = np.float32(np.sqrt(np.float32(2.0))) * np.float32(0.5)
    for c in ("0.3", "-0.6"):
        z, p, m = sp["zero_" + c], sp["plus_z_" + c], sp["minus_z_" + c]
        assert nb[z] == nb[p] > 30 and dev["exact"][z].any()
        assert np.array_equal(dev["q"][z], np.array([0, 0, 0, r2], np.float32)) and np.array_equal(dev["q"][p], np.array([0, 0, 0, 1], np.float32))
        assert np.array_equal(dev["exact"][z], dev["exact"][p]) and np.array_equal(dev["eid"][z], dev["eid"][p])
        assert np.array_equal(dev["q"][m], np.array([1, 0, 0, 0], np.float32))          # the x2 == 0 axis choice: a half turn about x
        assert dev["exact"][m].any() and not np.array_equal(dev["exact"][m], dev["exact"][p])
        # either side of the branch point: below it the half-angle form, at and above it the general form (told apart bit for bit below)
        for name, branch in (("c_below_", True), ("c_at_", False), ("c_above_", False)):
            i = sp[name + c]
            assert bool(s["branch"][i]) == branch and dev["exact"][i].any(), name
    # the quaternion of EVERY query, both sets: the float32 operations of quat_from_z restated in numpy, bit for bit (the divides and
    # square roots the device compiler emits are the correctly rounded ones); both branches occur
    for sname in ("random", "adversarial"):
        t = sets[sname]
        assert np.array_equal(t["dev"]["q"], t["q32"], equal_nan=True), np.nonzero((t["dev"]["q"] != t["q32"]).any(1))[0][:8]
    assert 200 < s["branch"].sum() < 1000 and not sets["adversarial"]["branch"].any()
    for name, want_nb in (("cos_1", 0), ("cos_above_1", 0), ("cos_below_1", 2), ("cos_minus_1", 56)):
        for suffix in ("", "_minus_z"):
            i = sp[name + suffix]
            assert nb[i] == want_nb == dev["ns"][i], (name, nb[i])
            assert bool(dev["exact"][i].any()) == (want_nb > 0)


def test_error_budget_of_the_filter(sets):
    """3. t = (normalize(M(q) d) / 2 + 0.5) / nepsilon in float64 from the device's own float32 q and the float32 sample; e_f = max |t_filter - t64|
    (the device's filter coordinates), e_x = the same for the float32 operations of cone_cell_exact.  A sample the filter decides is more than
    the margin away from every integer in ITS evaluation, so the exact evaluation truncates to the same cell whenever e_f + e_x < margin:
    the inequality the filter rests on, with the project's own number."""
    for name in ("random", "adversarial"):
        s = sets[name]
        assert s["fin"].sum() > 100_000, name
        assert s["e_f"] + s["e_x"] < cc.MARGIN, (name, s["e_f"], s["e_x"])


def test_undecided_fractions(sets):
    """4. random queries: below 1e-3 of the samples (the host test's bound).  Adversarial queries: every sample that float64 places inside the
    margin by more than e_f (+ 1e-7: the float32 constant 1 - margin and the subtraction t - floor(t) at t < 7 are exact to that) is undecided
    on the device, so the undecided fraction is at least their share."""
    assert sets["random"]["undecided"] < 1e-3, sets["random"]["undecided"]
    s = sets["adversarial"]
    t64 = s["t64"]
    dist = np.where(s["fin"][..., None], np.abs(t64 - np.rint(t64)), np.inf).min(-1)
    must = dist < cc.MARGIN - s["e_f"] - 1e-7
    assert must.sum() > 1000                                          # (the set does sit on the boundaries)
    assert (s["dev"]["fid"][must] == -1).all(), np.argwhere(must & (s["dev"]["fid"] != -1))[:8]
    assert s["undecided"] >= must.sum() / float(s["nb"].sum())
    print("adversarial set: %.3e of the samples inside the margin in float64, %.3e inside it by more than e_f, %.3e undecided"
          % ((dist < cc.MARGIN).sum() / float(s["nb"].sum()), must.sum() / float(s["nb"].sum()), s["undecided"]))
