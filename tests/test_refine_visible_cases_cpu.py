"""The numpy restatement of the visible-surface refinement (tests/refine_visible_ref.py) against itself and against mesh_ref, without
a GPU: the keys' depths are mesh_ref's image, a duplicated triangle resolves to the lower index in either order, every state class is hit
by the case named for it, the row linearises the motion it says it does, and the convergence cases the GPU tests rely on converge."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_cases as mc  # noqa: E402
import mesh_ref  # noqa: E402
import refine_visible_cases as rc  # noqa: E402
import refine_visible_ref as ref  # noqa: E402
import vsd_cases as vc  # noqa: E402

F = np.float32
CONVERGE = rc.convergence_cases()
STATES = rc.state_cases()


@pytest.mark.parametrize("case", CONVERGE + [STATES["counted"]], ids=repr)
def test_keys_hold_the_depth_image_and_a_live_triangle(case):
    k = ref.keys(case.start16, case.verts, case.tris, case.K, case.W, case.H)
    z = mesh_ref.render_bits(case.start16, case.verts, case.tris, case.K, case.W, case.H)
    assert np.array_equal((k >> np.uint64(32)).astype(np.uint32), z)
    t = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)[z != mesh_ref.EMPTY]
    assert len(t) and t.min() >= 0 and t.max() < len(case.tris)
    assert np.all((k == ref.EMPTY_KEY) == (z == mesh_ref.EMPTY))


def test_a_duplicated_triangle_gives_the_lower_index_in_either_order():
    case = STATES["counted"]
    k0 = ref.keys(case.start16, case.verts, case.tris, case.K, case.W, case.H)
    t0 = (k0 & np.uint64(0xFFFFFFFF)).astype(np.int64)
    which = int(np.bincount(t0[k0 != ref.EMPTY_KEY]).argmax())          # the triangle that wins the most pixels
    nt = len(case.tris)
    for front in (True, False):
        v, t = rc.duplicated(case.verts, case.tris, which, front)
        k = ref.keys(case.start16, v, t, case.K, case.W, case.H)
        assert np.array_equal(k >> np.uint64(32), k0 >> np.uint64(32))
        tk = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
        won = (t0 == which) & (k0 != ref.EMPTY_KEY)
        assert won.sum() > 0
        if front:      # the copy is triangle 0, the original which + 1: the copy wins; everybody else moves up by one
            assert np.all(tk[won] == 0) and np.array_equal(tk[~won & (k0 != ref.EMPTY_KEY)], t0[~won & (k0 != ref.EMPTY_KEY)] + 1)
        else:          # the copy is triangle nt: the original keeps every pixel
            assert np.array_equal(tk, t0) and not np.any(tk[k != ref.EMPTY_KEY] == nt)


@pytest.mark.parametrize("name", ["counted", "no_depth", "off_class", "too_far", "grazing"])
def test_each_state_class_is_hit_by_its_case(name):
    case = STATES[name]
    ev = ref.evaluate(case.start16, *case.args(), **case.prm)
    rec = ref.record_of(ev)
    assert rec[name] > 20, rec
    assert rec["present"] == rec["no_depth"] + rec["off_class"] + rec["too_far"] + rec["grazing"] + rec["counted"] == int((ev["keys"] != ref.EMPTY_KEY).sum())
    assert ev["sums"][27] == rec["counted"] == len(ev["b"])
    if name != "counted":       # the class takes pixels away from the counted ones of the plain case
        assert rec["counted"] < ref.record_of(ref.evaluate(STATES["counted"].start16, *STATES["counted"].args()))["counted"]


def test_a_degenerate_facet_is_grazing_with_the_gate_off():
    case = rc.degenerate_case()
    ev = ref.evaluate(case.start16, *case.args(), **case.prm)
    rec = ref.record_of(ev)
    tk = (ev["keys"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    won = (tk == 1) & (ev["keys"] != ref.EMPTY_KEY)
    assert won[0] and won.sum() == 1                       # the tiny facet wins the on-axis pixel, and that one alone
    assert ev["state"][0] == ref.GRAZING and rec["grazing"] == 1 and rec["counted"] > 100 and rec["too_far"] == 0


@pytest.mark.parametrize("kind", ["translation", "rotation"])
def test_one_step_recovers_a_small_pure_motion_to_first_order(kind):
    """the row's claim: r ~ n.(p - q) + omega.(q x n) + t.n for a motion applied on the left.  A start that is G moved by a small pure
    translation (rotation) comes back after ONE step up to second order in the motion and the frame's quantisation: the vertex error
    falls to below a quarter (measured: below a tenth), where a wrong sign or a motion applied on the right would raise it."""
    case = CONVERGE[0]
    G = np.asarray(case.G16, F).reshape(4, 4).T.astype(np.float64)
    start = vc.pose16(rc.perturbed(G, (0.3, -1.0, 0.5), 0.0 if kind == "translation" else 0.7, (0.0012, -0.0008, 0.0015) if kind == "translation" else (0, 0, 0)))
    e0 = ref.vertex_error(start, case.G16, case.verts)
    P1, ev, frozen = ref.step(start, *case.args(), max_distance=0.02)
    e1 = ref.vertex_error(P1, case.G16, case.verts)
    print("LINEARISATION %s e0 %.3g e1 %.3g" % (kind, e0, e1))
    assert not frozen and e0 > 5 * rc.SCALE and e1 <= 0.25 * e0


@pytest.mark.parametrize("case", CONVERGE, ids=repr)
def test_convergence_cases_converge_in_the_restatement(case):
    e0 = ref.vertex_error(case.start16, case.G16, case.verts)
    P, rec, trail = ref.refine(case.start16, *case.args(), **case.prm)
    e_ref = ref.vertex_error(P, case.G16, case.verts)
    print("CONVERGENCE %s e0 %.4g e_ref %.4g iterations %d counted %d" % (case.name, e0, e_ref, rec["iterations"], rec["counted"]))
    assert rec["iterations"] == case.prm["max_iterations"] and rec["frozen"] == 0
    assert e_ref <= 0.1 * e0


def test_invalid_poses_and_zero_iterations():
    case = STATES["counted"]
    for bad in (np.zeros(16, F), np.where(np.arange(16) == 13, np.nan, case.start16).astype(F)):
        P, rec, trail = ref.refine(bad, *case.args())
        assert np.array_equal(P.view(np.uint32), bad.view(np.uint32)) and all(rec[k] == 0 for k in ref.RECORD_FIELDS)
    P, rec, _ = ref.refine(case.start16, *case.args(), max_iterations=0)
    assert np.array_equal(P, case.start16) and rec["iterations"] == 0 and rec["counted"] > 100
