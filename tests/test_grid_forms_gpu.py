"""Every form of the scene grid build (grid.hip) under every scan kernel form (lcp.hip), on the adversarial cases of grid_cases.py,
against the numpy restatement of grid_ref.py: the grid info names the form that was asked for, the geometry and the incidence counts
equal the restatement, every model point of every transform finds the reference's scene point (no allowance), counted flags agree,
and scores are bitwise the restated integer score -- hence bitwise equal across all contexts and kernel forms.

Contexts per case: pruned / index-ordered / centre-sorted lists at cell edges eps, eps/2, eps/4; eps/3 pruned and index-ordered; on
the pruned grids at eps and eps/2 also STOCS_GRID_PRUNE_K 4 and 16, no cones, no flat table.  The build's switches are read per build,
so setting the environment around the estimator's construction selects the form."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_cases as cases  # noqa: E402
import grid_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCHES = ("STOCS_GRID_DIV", "STOCS_GRID_PRUNE", "STOCS_GRID_DENSE", "STOCS_GRID_PRUNE_K", "STOCS_GRID_CONES", "STOCS_LCP_FLAT", "STOCS_SORT")
LAYOUTS = {"pruned": {"STOCS_GRID_PRUNE": "1"}, "index": {"STOCS_GRID_PRUNE": "0", "STOCS_GRID_DENSE": "0"},
           "centre": {"STOCS_GRID_PRUNE": "0", "STOCS_GRID_DENSE": "1"}}
VARIANTS = (99, 0, 24, 39, 31)          # (a variant the grid cannot run maps to the queue form of that grid)


def contexts(case, extra=()):
    out = []
    for d in case["divs"]:
        for layout in (("pruned", "index") if d == 3 else ("pruned", "index", "centre")):
            out.append((d, layout, {}))
        if d in (1, 2):
            out += [(d, "pruned", {"STOCS_GRID_PRUNE_K": "4"}), (d, "pruned", {"STOCS_GRID_PRUNE_K": "16"}), (d, "pruned", {"STOCS_GRID_CONES": "0"}),
                    (d, "pruned", {"STOCS_LCP_FLAT": "0"})]
    return out + list(extra)


def make(monkeypatch, case, d, layout, more):
    from model_matching_amd import capi
    from model_matching_amd.estimator import StocsEstimator
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    env = dict(LAYOUTS[layout], STOCS_GRID_DIV=str(d), **more)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prm = capi.default_params()
    prm.distance_threshold = float(case["eps"])
    est = StocsEstimator(case["spos"], case["snrm"], case["sprob"], case["spix"], case["mpos"], case["mnrm"], params=prm, build_index=False)
    for k in env:
        monkeypatch.delenv(k)
    return est


_INC = {}


def restated(case, d):
    key = (case["name"], d)
    if key not in _INC:
        sc = case["_centred"][0]
        g = ref.geometry(sc, case["eps"], d)
        _INC[key] = (g, ref.incidences(sc, g))
    return _INC[key]


def check_info(case, est, d, layout, more):
    """The form that was asked for, the geometry bit for bit, the counts of the restated incidence predicate."""
    from model_matching_amd import capi
    gi = est.grid_info()
    g, inc = restated(case, d)
    tag = (case["name"], d, layout, more)
    assert gi["div"] == d and gi["pruned"] == (layout == "pruned") and gi["centre_sorted"] == (layout == "centre"), (tag, gi)
    assert gi["has_nearest"] == (d > 1 and layout != "index"), (tag, gi)
    assert gi["has_cones"] == (more.get("STOCS_GRID_CONES") != "0"), (tag, gi)
    n_flat = g["cells"][0] * g["cells"][1] * g["cells"][2]
    assert gi["has_flat"] == (d == 1 and layout != "centre" and more.get("STOCS_LCP_FLAT") != "0" and n_flat * 16 <= (512 << 20)), (tag, gi)
    assert np.array_equal(gi["origin"].view(np.uint32), g["origin"].view(np.uint32)) and gi["h"] == g["h"] and gi["inv_h"] == g["inv_h"], (tag, gi, g)
    assert gi["cells"] == g["cells"] and gi["bricks"] == g["bricks"], (tag, gi, g)
    assert gi["n_incidences"] == inc["n_incidences"] and gi["n_cells"] == inc["n_cells"] and gi["n_bricks"] == inc["n_bricks"], (tag, gi, {k: inc[k] for k in ("n_incidences", "n_cells", "n_bricks")})
    # the sort: the library's own from 65 536 incidences on when the key fits 32 bits, rocPRIM's otherwise and on request
    n_top = g["bricks"][0] * g["bricks"][1] * g["bricks"][2]
    cell_bits = 1
    while (1 << cell_bits) < n_top * 512:
        cell_bits += 1
    own = cell_bits + (16 if layout == "centre" else 0) <= 32 and inc["n_incidences"] >= 65536 and more.get("STOCS_SORT") != "rocprim"
    assert gi["sort"] == (capi.GRID_SORT_OWN if own else capi.GRID_SORT_ROCPRIM), (tag, gi)
    if layout == "pruned":
        assert gi["prune_k"] == int(more.get("STOCS_GRID_PRUNE_K", 8)), (tag, gi)
        assert gi["prune_group"] == (16 if inc["n_incidences"] <= 12 * inc["n_cells"] else 64), (tag, gi)
        assert 1 <= gi["longest_list"] <= inc["longest"] and gi["n_entries"] <= inc["n_entries_unpruned"] and gi["n_entries"] % 8 == 0, (tag, gi)
    else:
        assert gi["prune_k"] == 0 and gi["prune_group"] == 0, (tag, gi)
        assert gi["longest_list"] == inc["longest"] and gi["n_entries"] == inc["n_entries_unpruned"], (tag, gi, inc["longest"], inc["n_entries_unpruned"])
    return gi


def check_kernels(case, est, tag, variants=VARIANTS, culls=(0, 2)):
    """Hit indices and counted flags of every model point of every transform, and the scores at batch sizes 1, 3 and all."""
    R = ref.reference(case)
    T = case["T"]
    want = np.array([r["score"] for r in R], np.float32)
    bad = []
    for v in variants:
        est.set_option("lcp_variant", v)
        for cull in culls:
            est.set_option("lcp_cull", cull)
            for ti in range(len(T)):
                hit, cnt = est.lcp_detail(T[ti])
                wrong = np.nonzero(hit != R[ti]["hit"])[0]
                if len(wrong):
                    i = int(wrong[0])
                    bad.append(("hit", v, cull, ti, len(wrong), i, int(hit[i]), int(R[ti]["hit"][i]), R[ti]["q"][i].tolist()))
                elif not np.array_equal(cnt.astype(bool), R[ti]["counted"]):
                    bad.append(("counted", v, cull, ti, int((cnt.astype(bool) != R[ti]["counted"]).sum())))
            for split in (0, 1):
                est.set_option("lcp_split", split)
                for n in sorted({1, min(3, len(T)), len(T)}):
                    got = est.score_transforms(T[:n])
                    if not np.array_equal(got.view(np.uint32), want[:n].view(np.uint32)):
                        bad.append(("score", v, cull, split, n, got.tolist(), want[:n].tolist()))
    est.set_option("lcp_variant", 99); est.set_option("lcp_cull", 1); est.set_option("lcp_split", 1)
    assert not bad, (tag, len(bad), bad[:4])


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_grid_form_answers_like_the_reference(name, monkeypatch):
    case = cases.build(name)
    ref.reference(case)
    extra = [(1, "pruned", {"STOCS_SORT": "rocprim"}), (1, "index", {"STOCS_SORT": "rocprim"})] if name.startswith("sort_") else []
    failures = []
    for d, layout, more in contexts(case, extra):
        est = make(monkeypatch, case, d, layout, more)
        try:
            assert not est.get_scene_centroid().any() or name == "one_point"
            assert not est.get_model_centroid().any()
            check_info(case, est, d, layout, more)
            check_kernels(case, est, (name, d, layout, more))
        except AssertionError as e:            # (every context is run: the report names all the forms that fail, not the first)
            failures.append(str(e)[:1500])
        finally:
            est.close()
    assert not failures, "%d of %d contexts failed:\n%s" % (len(failures), len(contexts(case, extra)), "\n".join(failures[:6]))


def test_sort_threshold_scenes_take_either_sort(monkeypatch):
    """Just below 65 536 incidences rocPRIM's sort runs, from there on the library's own, and STOCS_SORT=rocprim overrides it."""
    from model_matching_amd import capi
    kinds = {}
    for name in ("sort_below", "sort_above"):
        case = cases.build(name)
        ref.reference(case)
        for more in ({}, {"STOCS_SORT": "rocprim"}):
            est = make(monkeypatch, case, 1, "pruned", more)
            gi = est.grid_info()
            est.close()
            assert gi["n_incidences"] == case["n_incidences_div1"]
            kinds[(name, bool(more))] = gi["sort"]
    assert kinds == {("sort_below", False): capi.GRID_SORT_ROCPRIM, ("sort_below", True): capi.GRID_SORT_ROCPRIM,
                     ("sort_above", False): capi.GRID_SORT_OWN, ("sort_above", True): capi.GRID_SORT_ROCPRIM}


def test_prune_group_follows_the_average_list(monkeypatch):
    groups = {}
    for name in ("lists", "lists_sparse"):
        case = cases.build(name)
        ref.reference(case)
        est = make(monkeypatch, case, 1, "pruned", {})
        groups[name] = est.grid_info()["prune_group"]
        est.close()
    assert groups == {"lists": 64, "lists_sparse": 16}


@pytest.mark.parametrize("layout", ["pruned", "index", "centre"])
def test_65535_coincident_points_build_and_answer(layout, monkeypatch):
    """The longest list the 16-bit count of a cell word can hold: every cell within r of the point lists all 65 535 copies."""
    case = cases.coincident(65535)
    ref.reference(case)
    est = make(monkeypatch, case, 1, layout, {})
    gi = est.grid_info()
    g, inc = restated(case, 1)
    assert gi["n_incidences"] == inc["n_incidences"] and gi["n_cells"] == inc["n_cells"] and inc["longest"] == 65535
    assert gi["longest_list"] == (65535 if layout != "pruned" else gi["longest_list"]) and 1 <= gi["longest_list"] <= 65535
    check_kernels(case, est, ("coincident", layout), variants=(99, 0), culls=(0,))
    est.close()


def test_65536_coincident_points_are_refused_and_leave_no_scene(monkeypatch):
    from model_matching_amd import capi
    small, big = cases.coincident(64), cases.coincident(65536)
    for layout in ("pruned", "index"):
        est = make(monkeypatch, small, 1, layout, {})
        for k, v in dict(LAYOUTS[layout], STOCS_GRID_DIV="1").items():
            monkeypatch.setenv(k, v)
        with pytest.raises(capi.StocsError) as ei:
            est.set_scene(big["spos"], big["snrm"], big["sprob"], big["spix"])
        assert ei.value.code == capi.ERR_INVALID and "more than 65535 scene points within epsilon of one grid cell" in str(ei.value)
        gi = capi.GridInfo()
        gi.div = 9
        assert est.L.stocs_get_grid_info(est.h, C.byref(gi)) == capi.ERR_STATE and b"no scene" in est.L.stocs_last_error()
        assert bytes(gi) == bytes(C.sizeof(gi))
        est.set_scene(small["spos"], small["snrm"], small["sprob"], small["spix"])      # and the context recovers
        assert est.grid_info()["longest_list"] >= 1
        est.close()
