"""The calling thread's cached memory behind the entry points without a context (csrc/thread_cache.h): ingest.hip and segment.hip each keep
an instance of their own.  What the shared struct could break and no other test looks at: calls of both files interleaved on one thread
return what each returns alone, neither instance evicts the other's memory, stocs_trim gives both back and the next round allocates
again with equal results, a second thread's calls and its stocs_trim leave the first thread's cache and its last moments alone, and under
STOCS_SEGMENT_CLOCK=1 a plain call after a convex one leaves no bend time behind.  Frames: segment_cases' 129 x 33 (one tile row and a
ragged edge) and 64 x 16 (exactly one tile), and the smallest frame test_ingest_edges_gpu.py ingests (11 x 13)."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import segment_cases as sc  # noqa: E402
import test_ingest_edges_gpu as ie  # noqa: E402

pytestmark = pytest.mark.gpu
BIG, SMALL = (129, 33), (64, 16)


@pytest.fixture(scope="module")
def lib():
    from model_matching_amd import capi
    return capi, capi.load()


@pytest.fixture(autouse=True)
def default_forms(monkeypatch):
    for name in ("STOCS_SEGMENT_FORM", "STOCS_SEGMENT_BEND_FORM", "STOCS_SEGMENT_CLOCK"):
        monkeypatch.delenv(name, raising=False)


def _table(size, seed):
    """a table frame with two boxes that fit `size`: the plane search runs, so the refit's moments are not zero"""
    W, H = size
    boxes = ((W // 8, H // 4, W // 4, H // 2, 0.08), (5 * W // 8, H // 4, W // 4, H // 2, 0.12))
    d, K, _, _ = sc.table_frame(W=W, H=H, seed=seed, boxes=boxes, noise_mm=1.0)
    return d, K


def _ingest_case():
    small = [c for c in ie.SCENE_CASES if "crop" in c and "up" not in c and "edit" not in c]
    return ie._case_inputs(min(small, key=lambda c: c["crop"][2] * c["crop"][3]))


def _calls():
    """name -> a function that makes the call and returns its whole result as a tuple of bytes"""
    from model_matching_amd import estimator as E
    depth, prob, K, scale, voxel, thr = _ingest_case()
    assert depth.shape == (11, 13)
    big, Kb = _table(BIG, 1)
    small, Ks = _table(SMALL, 2)

    def seg(d, K, **kw):
        res, rec, img = E.segment_frame(d, K, sc.SCALE, min_pixels=20, seed=3, **kw)
        return tuple((k, np.asarray(v).tobytes()) for k, v in sorted(res.items())) + (rec.tobytes(),) + tuple((k, v.tobytes()) for k, v in sorted(img.items()))

    return {
        "ingest": lambda: tuple(a.tobytes() for a in E.ingest_scene(depth, prob, K, scale, voxel, thr)),
        "segment big": lambda: seg(big, Kb),
        "convex big": lambda: seg(big, Kb, convex=True, images=("class_prob", "labels", "edge", "cut", "smoothed")),
        "segment small": lambda: seg(small, Ks),
    }


ROUND = ("ingest", "segment big", "ingest", "convex big", "segment big", "segment small")


def _moments(L):
    m = np.zeros(10, np.int64)
    assert L.stocs_segment_last_moments(m.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    return m


def test_interleaved_calls_equal_the_calls_alone(lib):
    calls = _calls()
    alone = {name: fn() for name, fn in calls.items()}
    assert len(set(alone.values())) == len(alone)                # four different results: a mixed-up buffer would show
    for name in ROUND + ROUND[::-1]:
        assert calls[name]() == alone[name], name


def test_the_two_instances_do_not_evict_each_other(lib):
    capi, L = lib
    calls = _calls()
    for name in ("ingest", "convex big", "segment big"):        # the largest of each call
        calls[name]()
    before = L.stocs_device_alloc_count()
    for name in ROUND:
        calls[name]()
    assert L.stocs_device_alloc_count() == before


def test_trim_gives_both_back(lib):
    capi, L = lib
    calls = _calls()
    first = [calls[name]() for name in ROUND]
    before = L.stocs_device_alloc_count()
    assert L.stocs_trim() == 0 and L.stocs_trim() == 0          # the second finds nothing to give back
    assert L.stocs_device_alloc_count() == before
    assert calls["ingest"]() == first[0]
    after_ingest = L.stocs_device_alloc_count()
    assert after_ingest > before                                # the ingest's arena and pinned block were gone ...
    assert calls["segment big"]() == first[1]
    assert L.stocs_device_alloc_count() > after_ingest          # ... and so were the segmentation's own
    assert [calls[name]() for name in ROUND] == first


def test_a_second_thread_has_a_cache_of_its_own(lib):
    capi, L = lib
    calls = _calls()
    ingested = calls["ingest"]()
    alone = calls["segment big"]()
    mine = _moments(L)
    assert mine[0] > 0
    before = L.stocs_device_alloc_count()
    seen = {}

    def other():
        seen["small"] = calls["segment small"]()
        seen["moments"] = _moments(L)
        seen["ingest"] = calls["ingest"]()
        seen["trim"] = L.stocs_trim()

    t = threading.Thread(target=other)
    t.start()
    t.join()
    after = L.stocs_device_alloc_count()
    assert seen["trim"] == 0 and after > before                 # the other thread allocated arenas and pinned blocks of its own, and gave them back
    assert np.array_equal(_moments(L), mine) and not np.array_equal(seen["moments"], mine)   # this thread's last call's, not the other thread's
    assert calls["segment big"]() == alone and calls["ingest"]() == ingested
    assert L.stocs_device_alloc_count() == after                # the other thread's stocs_trim took nothing of this thread's cache
    assert seen["small"] == calls["segment small"]() and seen["ingest"] == ingested


def test_a_plain_call_after_a_convex_call_leaves_no_bend_time(lib, monkeypatch):
    capi, L = lib
    calls = _calls()
    monkeypatch.setenv("STOCS_SEGMENT_CLOCK", "1")
    s, l, b = C.c_float(-1), C.c_float(-1), C.c_float(-1)
    calls["convex big"]()
    assert L.stocs_segment_last_bend_ms(C.byref(b)) == 0 and b.value > 0
    assert L.stocs_segment_last_device_ms(C.byref(s), C.byref(l)) == 0 and s.value > 0 and l.value > 0
    calls["segment big"]()
    assert L.stocs_segment_last_bend_ms(C.byref(b)) == capi.ERR_STATE
    assert L.stocs_segment_last_device_ms(C.byref(s), C.byref(l)) == 0
    assert L.stocs_trim() == 0                                  # the events go with the cache; the next clocked call makes them anew
    calls["convex big"]()
    assert L.stocs_segment_last_bend_ms(C.byref(b)) == 0 and b.value > 0
    monkeypatch.delenv("STOCS_SEGMENT_CLOCK")
    calls["convex big"]()
    assert L.stocs_segment_last_bend_ms(C.byref(b)) == capi.ERR_STATE and L.stocs_segment_last_device_ms(C.byref(s), C.byref(l)) == capi.ERR_STATE
