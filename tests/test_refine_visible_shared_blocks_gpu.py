"""The visible-surface refinement's shared device blocks: the damped and the contour form carve one grow-only block, both detail entry
points another, each with its own layout.  A call that follows another form's, with fewer or more poses, with or without a trace, in one
chunk or several, must give the bits of the same call on a fresh context: a stale tail or a wrong offset of the shared layout would show.
Every comparison is for equality; the frame is refine_visible_contour_cases.small_solid_case()'s, 128 x 96 pixels."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import refine_visible_contour_cases as cc  # noqa: E402
import refine_visible_damped_ref as dref  # noqa: E402
from test_refine_visible_contour_gpu import CCtx  # noqa: E402
from test_refine_visible_gpu import _seven  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(result):
    """(poses, records, trace or None) of a batch call, or the arrays of a detail call, as bytes"""
    return tuple(None if a is None else np.ascontiguousarray(a).tobytes() for a in result)


def _batch(cx, form, poses, trace):
    return _bits(getattr(cx, form)(poses, trace=trace))


def test_damped_and_contour_calls_in_turn_on_one_block_are_fresh_calls():
    case = cc.small_solid_case()
    poses = _seven(case)
    calls = [("damped", 4, True), ("contour", 2, False), ("damped", 4, True), ("contour", 4, True), ("damped", 1, True)]
    fresh = {}
    for call in set(calls):
        cx = CCtx(case)
        fresh[call] = _batch(cx, call[0], poses[: call[1]], call[2])
        cx.close()
    assert fresh[calls[1]][2] is None and len(fresh[calls[3]][2]) == 4 * (case.prm["max_iterations"] + 1) * 88
    cx = CCtx(case)
    for i, call in enumerate(calls):
        assert _batch(cx, call[0], poses[: call[1]], call[2]) == fresh[call], (i, call)
    cx.close()


def test_both_detail_paths_in_turn_on_one_block_and_a_second_round_allocates_nothing():
    case = cc.small_solid_case()
    poses = _seven(case)[:4]
    plain_prm = dict((k, v) for k, v in case.prm.items() if k in dref.BASE_KEYS or k == "max_iterations")
    cx = CCtx(case)
    want_plain = _bits(cx.detail(poses[0]))             # keys, state, sums
    cx.close()
    cx = CCtx(case)
    want_contour = _bits(cx.cdetail(poses[0]))          # state, nearest indices, sums
    cx.close()
    assert len(want_plain[0]) == 8 * case.W * case.H and len(want_contour[1]) == 4 * case.W * case.H
    cx = CCtx(case)
    assert _bits(cx.detail(poses[0])) == want_plain
    assert _bits(cx.cdetail(poses[0])) == want_contour
    assert _bits(cx.detail(poses[0])) == want_plain

    def one_round():
        return [_bits(cx.refine(poses, **plain_prm)), _batch(cx, "damped", poses, True), _batch(cx, "contour", poses, True), _bits(cx.detail(poses[1])),
                _bits(cx.cdetail(poses[1]))]

    first = one_round()
    before = cx.L.stocs_device_alloc_count()
    assert one_round() == first
    assert cx.L.stocs_device_alloc_count() == before
    cx.close()


def test_chunks_of_three_across_the_shared_layout_change_no_bit(monkeypatch):
    case = cc.small_solid_case()
    poses = _seven(case)
    assert len(poses) == 7
    monkeypatch.delenv("STOCS_REFINE_VISIBLE_CHUNK", raising=False)
    cx = CCtx(case)
    want_contour, want_damped = _batch(cx, "contour", poses, True), _batch(cx, "damped", poses, True)
    cx.close()
    assert len(set(want_contour[0][64 * i: 64 * i + 64] for i in range(7))) == 7      # seven different results: an offset h0 taken wrongly shows
    monkeypatch.setenv("STOCS_REFINE_VISIBLE_CHUNK", "3")                             # chunks at h0 = 0, 3, 6
    cx = CCtx(case)
    assert _batch(cx, "contour", poses, True) == want_contour
    assert _batch(cx, "damped", poses, True) == want_damped
    cx.close()
