"""The library's own stable radix sort of (u32 key, u32 value) pairs (csrc/sort32.hip) -- the sort behind the pair lists of the
congruent-set phase, where the reference keeps a pointer grid of per-cell vectors filled one pair at a time (IndexedNormalSet::addElement,
reference include/super4pcs/accelerators/normalset.hpp:114-131; src/stocs.cpp:806-866): a run of equal keys is a cell's vector in insertion
order, so the sort must be STABLE.  Checked against numpy's stable argsort and against rocPRIM, bit for bit, on the key shapes of the path."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _sort(keys, vals, end_bit, which, reps=1, seg_off=None):
    from model_matching_amd import capi
    L = capi.load()
    k = np.ascontiguousarray(keys, np.uint32); v = np.ascontiguousarray(vals, np.uint32)
    ko = np.zeros_like(k); vo = np.zeros_like(v)
    ms = C.c_float(0)
    u32p = C.POINTER(C.c_uint32)
    so = None if seg_off is None else np.ascontiguousarray(seg_off, np.uint32)
    capi.check(L.stocs_debug_sort_pairs(-1, k.ctypes.data_as(u32p), v.ctypes.data_as(u32p), len(k), end_bit, which, reps,
                                        ko.ctypes.data_as(u32p), vo.ctypes.data_as(u32p), C.byref(ms),
                                        None if so is None else so.ctypes.data_as(u32p), 0 if so is None else len(so) - 1))
    return ko, vo, ms.value


@pytest.mark.parametrize("n,end_bit", [(0, 8), (1, 1), (63, 5), (4096, 8), (4097, 15), (100003, 22), (1 << 20, 28), (3000017, 22), (2500000, 15), (777777, 32), (50000, 9), (50000, 17)])
def test_own_sort_is_stable_and_equals_numpy_and_rocprim(n, end_bit):
    rng = np.random.default_rng(n + end_bit)
    mask = np.uint64((1 << end_bit) - 1)
    keys = (rng.integers(0, 1 << 32, n, dtype=np.uint64) & mask).astype(np.uint32)
    if n > 1000:                                   # the key shapes of the path: long runs of one (base, cell), a few heavy cells, bits above end_bit set
        keys[: n // 3] = np.sort(keys[: n // 3])
        keys[n // 2: n // 2 + n // 8] = keys[0]
        keys |= (rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)) if end_bit < 32 else np.uint32(0)
    vals = np.arange(n, dtype=np.uint32)[::-1].copy()
    ko, vo, _ = _sort(keys, vals, end_bit, 1)
    order = np.argsort(keys & np.uint32(mask), kind="stable")
    assert np.array_equal(ko, keys[order]) and np.array_equal(vo, vals[order])
    kr, vr, _ = _sort(keys, vals, end_bit, 0)
    assert np.array_equal(ko, kr) and np.array_equal(vo, vr)


def test_all_keys_equal_and_all_distinct():
    n = 300000
    vals = np.arange(n, dtype=np.uint32)
    ko, vo, _ = _sort(np.full(n, 12345, np.uint32), vals, 22, 1)
    assert np.array_equal(vo, vals) and (ko == 12345).all()             # one run: the order of the input
    keys = np.random.default_rng(5).permutation(n).astype(np.uint32)
    ko, vo, _ = _sort(keys, vals, 19, 1)
    assert np.array_equal(ko, np.arange(n, dtype=np.uint32)) and np.array_equal(keys[vo], ko)


@pytest.mark.parametrize("n,n_seg,cell_bits", [(200000, 7, 15), (3000000, 100, 15), (1500000, 4000, 16), (50000, 300, 9), (4096 * 3, 3, 8)])
def test_segmented_by_base_equals_a_full_sort_of_base_and_cell(n, n_seg, cell_bits):
    """The form the congruent-set phase uses: the list is base-major, every base's stretch is sorted by its cell bits alone (two passes) --
    the result must be the stable sort by the whole (base, cell) key.  Segment lengths as uneven as the bases of a trial (a dozen bases carry
    most of the entries, many are short, some are empty); bits above the cell bits hold the base and must be ignored by the passes."""
    rng = np.random.default_rng(n_seg * 31 + cell_bits)
    w = rng.pareto(0.8, n_seg) + 0.01
    w[rng.integers(0, n_seg, max(1, n_seg // 10))] = 0.0                      # empty bases
    lens = np.floor(w / w.sum() * n).astype(np.int64)
    lens[int(np.argmax(lens))] += n - int(lens.sum())
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    base = np.repeat(np.arange(n_seg, dtype=np.uint32), lens)
    cell = rng.integers(0, 1 << cell_bits, n, dtype=np.uint32)
    cell[: n // 4] = np.sort(cell[: n // 4]) >> np.uint32(3) << np.uint32(3)   # long runs of one cell
    keys = (base << np.uint32(cell_bits)) | cell
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ko, vo, _ = _sort(keys, vals, cell_bits, 1, seg_off=off)
    order = np.argsort(keys, kind="stable")                                   # (base-major input: sorting the whole key = sorting every segment by cell)
    assert np.array_equal(ko, keys[order]) and np.array_equal(vo, vals[order])


# ---- the forms the sort takes at large sizes and at segment lengths on its boundaries ----
# Segments of at most SMALL_CAP = 2 048 pairs are sorted whole in LDS; longer ones are cut into tiles of 64 x wavefronts x pairs per
# thread (4x8: 2 048, 4x16 and 8x8: 4 096, 8x16 and 16x8: 8 192, 16x16: 16 384); by the list's length the sort takes 4x16 below 1 M
# pairs, 8x16 from 1 M, 16x16 from 32 M, and one histogram workgroup per tile (hist_sub 1) from 16 M on, four below.
SMALL_CAP = 2048
TILES = (2048, 4096, 8192, 16384)
BOUNDARY_LENS = [0, 1, 0, SMALL_CAP - 1, SMALL_CAP, SMALL_CAP + 1] + [x for t in TILES for x in (t - 1, t, t + 1, 2 * t + 1)] + [0]
SHAPES = ("4x8", "4x16", "8x8", "8x16", "16x8", "16x16")


def _unsegmented_case(n, end_bit, seed):
    rng = np.random.default_rng(seed)
    mask = np.uint64((1 << end_bit) - 1)
    keys = (rng.integers(0, 1 << 32, n, dtype=np.uint64) & mask).astype(np.uint32)
    keys[: n // 3] = np.sort(keys[: n // 3])                      # long sorted stretches, one heavy key, bits above end_bit set
    keys[n // 2: n // 2 + n // 8] = keys[0]
    if end_bit < 32:
        keys |= rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    order = np.argsort(keys & np.uint32(mask), kind="stable")
    return keys, vals, keys[order], vals[order]


def _segmented_case(lens, cell_bits, seed):
    """Base-major keys (segment << cell_bits | cell): sorting every segment by its cell bits = the stable sort of the whole key."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    assert len(lens) <= 1 << (32 - cell_bits)
    n = int(lens.sum())
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    cell = rng.integers(0, 1 << cell_bits, n, dtype=np.uint32)
    cell[: n // 4] = np.sort(cell[: n // 4]) >> np.uint32(3) << np.uint32(3)   # long runs of one cell
    keys = (np.repeat(np.arange(len(lens), dtype=np.uint32), lens) << np.uint32(cell_bits)) | cell
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    order = np.argsort(keys, kind="stable")
    return keys, vals, off, keys[order], vals[order]


@pytest.mark.parametrize("n,end_bit", [((16 << 20) + 3, 22), ((32 << 20) + 5, 32)])
def test_own_sort_at_the_sizes_of_its_large_forms_equals_numpy(n, end_bit):
    """16 M + 3 pairs: 8x16 tiles, one histogram workgroup per tile; 32 M + 5: 16x16 tiles (four passes over 32 bits)."""
    keys, vals, rk, rv = _unsegmented_case(n, end_bit, n)
    ko, vo, _ = _sort(keys, vals, end_bit, 1)
    assert np.array_equal(ko, rk) and np.array_equal(vo, rv)


def test_segmented_sort_of_16M_pairs_over_20000_segments_equals_numpy():
    """A trial batch's list: 20 000 segments, uneven (a few thousand pairs typical, some on the tile boundaries, some empty), 16 M+ pairs."""
    rng = np.random.default_rng(16)
    w = np.minimum(rng.pareto(1.2, 20000) + 0.002, 500.0)
    lens = np.floor(w / w.sum() * (16 << 20)).astype(np.int64)
    lens[rng.integers(0, 20000, 1500)] = 0
    lens[rng.integers(0, 20000, 1500)] = rng.integers(0, 2 * SMALL_CAP, 1500)
    b = np.array(BOUNDARY_LENS * 8, np.int64)
    lens[rng.choice(20000, len(b), replace=False)] = b
    lens[0] += max(0, (16 << 20) + 1 - int(lens.sum()))
    keys, vals, off, rk, rv = _segmented_case(lens, 17, 17)
    assert len(keys) > (16 << 20)
    ko, vo, _ = _sort(keys, vals, 17, 1, seg_off=off)
    assert np.array_equal(ko, rk) and np.array_equal(vo, rv)


@pytest.mark.parametrize("filler", [0, 1500000])
def test_segment_lengths_on_every_boundary_equal_numpy(filler):
    """Segments of 0, 1, SMALL_CAP - 1 .. SMALL_CAP + 1 and tile - 1, tile, tile + 1, 2 tile + 1 pairs for every tile size, alone (4x16
    tiles) and behind a long segment that takes the list beyond 1 M pairs (8x16)."""
    lens = BOUNDARY_LENS + ([filler] if filler else [])
    for cell_bits in (9, 16):
        keys, vals, off, rk, rv = _segmented_case(lens, cell_bits, cell_bits + filler)
        ko, vo, _ = _sort(keys, vals, cell_bits, 1, seg_off=off)
        assert np.array_equal(ko, rk) and np.array_equal(vo, rv), cell_bits


def test_every_forced_tile_shape_and_histogram_split_equals_numpy(tmp_path):
    """STOCS_SORT_SHAPE (six shapes) x STOCS_SORT_HIST_SUB {1, 4} -- read once per process: one child process per setting, one after the
    other, stopping at the first that fails; each sorts the boundary list and a 3 M-pair unsegmented list."""
    import os
    import subprocess
    import sys
    keys, vals, off, rk, rv = _segmented_case(BOUNDARY_LENS, 16, 99)
    fk, fv, frk, frv = _unsegmented_case(3000007, 22, 98)
    path_in = str(tmp_path / "in.npz")
    np.savez(path_in, seg_keys=keys, seg_vals=vals, seg_off=off, seg_end_bit=16, flat_keys=fk, flat_vals=fv, flat_end_bit=22)
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fresh_process_child.py")
    for shape in SHAPES:
        for hist_sub in ("1", "4"):
            env = dict(os.environ)
            env.update(STOCS_SORT_SHAPE=shape, STOCS_SORT_HIST_SUB=hist_sub)
            path_out = str(tmp_path / ("out_%s_%s.npz" % (shape, hist_sub)))
            p = subprocess.run([sys.executable, child, "sort", path_in, path_out], env=env, capture_output=True, text=True, timeout=180)
            assert p.returncode == 0, (shape, hist_sub, p.returncode, p.stderr[-3000:])
            z = np.load(path_out)
            assert np.array_equal(z["seg_keys"], rk) and np.array_equal(z["seg_vals"], rv), (shape, hist_sub)
            assert np.array_equal(z["flat_keys"], frk) and np.array_equal(z["flat_vals"], frv), (shape, hist_sub)
