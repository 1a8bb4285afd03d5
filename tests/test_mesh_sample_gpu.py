"""Mesh sampling on the GPU against its numpy restatement (tests/mesh_sample_ref.py): counts, area, positions, normals and triangle
indices bit for bit on single triangles, runs of empty triangles, counts and totals either side of a wavefront and a workgroup, the box
at a fine spacing and a level-5 mesh at a coarse one, under every forced form of the sample kernel; then the entry points' answers, and
stocs_preprocess_model_mesh against the restatement's samples through the oracle's voxel grid."""
import ctypes as C
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_sample_cases as mc  # noqa: E402
import mesh_sample_ref as ref  # noqa: E402
from model_matching_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, CAPACITY = -1, -4
FORMS = (None, "1", "2")              # STOCS_MESH_SAMPLE_FORM: the default, every lane searches the whole array (the default named), the workgroup's window
CASES = mc.gpu_cases()


@functools.lru_cache(maxsize=None)
def _ref(name):
    v, t, h, seed = CASES[name]
    return ref.counts(v, t, h, seed), ref.sample(v, t, h, seed)[:3]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, what):
    for g, w, field in zip(got, want, ("positions", "normals", "triangle indices")):
        assert g.shape == w.shape, "%s: %d %s for %d" % (what, len(g), field, len(w))
        bad = np.flatnonzero((_bits(g) != _bits(w)).reshape(len(g), int(np.prod(g.shape[1:]))).any(axis=1))
        assert len(bad) == 0, "%s: %d of %d %s differ, first sample %d: %r for %r" % (what, len(bad), len(g), field, bad[0], g[bad[0]], w[bad[0]])


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_equal_the_restatement_under_every_form(name, monkeypatch):
    from model_matching_amd.estimator import mesh_sample, mesh_sample_counts
    v, t, h, seed = CASES[name]
    (n, area, total, skipped), want = _ref(name)
    got_n, got_area, got_total, got_skipped = mesh_sample_counts(v, t, h, seed)
    assert np.array_equal(got_n, n) and got_total == total and got_skipped == skipped, name
    assert np.float64(got_area).view(np.uint64) == np.float64(area).view(np.uint64), "%s: area %r for %r" % (name, got_area, area)
    for form in FORMS:
        if form is None:
            monkeypatch.delenv("STOCS_MESH_SAMPLE_FORM", raising=False)
        else:
            monkeypatch.setenv("STOCS_MESH_SAMPLE_FORM", form)
        _same(mesh_sample(v, t, h, seed), want, "%s, form %s" % (name, form))


def test_the_cases_hold_what_they_are_for():
    assert _ref("legs_4h")[0][2] == 8 and _ref("below_one_none")[0][2] == 0 and _ref("below_one_one")[0][2] == 1 and _ref("total_0")[0][2] == 0
    for n in (255, 256, 257):
        assert _ref("total_%d" % n)[0][2] == n and len(CASES["nt_%d" % n][1]) == n and _ref("count_%d" % n)[0][0].tolist() == [3, n, 2]
    n = _ref("box_fine")[0][0]
    assert n.min() > 2000                                                       # thousands of samples share a triangle
    n = _ref("level5_coarse")[0][0]
    assert (n == 0).mean() > 0.8 and n.sum() > 1000                             # most triangles have none
    n = _ref("empty_long_runs")[0][0]
    assert n[0] == 0 and n[-1] == 0 and (n == 0).sum() == len(n) - 2            # empty at the start, in the middle and at the end, longer than a window


def test_a_nan_corner_is_a_skipped_triangle_for_the_counts_and_refused_by_the_sampler():
    from model_matching_amd import capi
    from model_matching_amd.estimator import mesh_sample, mesh_sample_counts
    v, t = mc.degenerate("nan")
    n, area, total, skipped = ref.counts(v, t, mc.H, 3)
    got = mesh_sample_counts(v, t, mc.H, 3)
    assert got[0].tolist() == n.tolist() == [3, 0, 2] and got[1] == area and got[2:] == (total, skipped) == (5, 1)
    with pytest.raises(capi.StocsError, match="finite"):
        mesh_sample(v, t, mc.H, 3)


def test_orientation_modes_and_reversed_winding():
    from model_matching_amd.estimator import mesh_sample
    v, t, wall = mc.bowl()
    for orient in (0, 1):
        _same(mesh_sample(v, t, 0.003, mc.SEED, orient=orient), ref.sample(v, t, 0.003, mc.SEED, orient)[:3], "bowl, orient %d" % orient)
    pos, nrm, tri = mesh_sample(v, t, 0.003, mc.SEED)
    assert not ((nrm * mc.bowl_true_normal(pos.astype(np.float64), wall[tri])).sum(axis=1) < 0).any()
    pos_r, nrm_r, tri_r = mesh_sample(v, t[:, [0, 2, 1]].copy(), 0.003, mc.SEED)
    assert np.array_equal(tri_r, tri) and np.array_equal(nrm_r, -nrm)           # the exact negative (u and v change places: other positions)


def test_same_seed_same_bits_and_another_seed_differs():
    from model_matching_amd.estimator import mesh_sample
    v, t = synth.make_model_mesh(3)
    a, b, c = mesh_sample(v, t, 0.002, 5), mesh_sample(v, t, 0.002, 5), mesh_sample(v, t, 0.002, 6)
    _same(a, b, "the same seed twice")
    assert len(c[0]) != len(a[0]) or not np.array_equal(c[0], a[0])
    _same(mesh_sample(v, t, 0.002, 2 ** 64 - 1), ref.sample(v, t, 0.002, 2 ** 64 - 1)[:3], "seed 2^64 - 1")


def _raw_sample(v, t, h, seed, cap, orient=0, fill=-12345.0):
    from model_matching_amd import capi
    L = capi.load()
    pos = np.full((max(cap, 1) + 4, 3), fill, F); nrm = np.full((max(cap, 1) + 4, 3), fill, F); tri = np.full(max(cap, 1) + 4, -77, np.int32)
    n = C.c_int(-1)
    rc = L.stocs_mesh_sample(v.ctypes.data_as(capi._fp), len(v), t.ctypes.data_as(capi._ip), len(t), h, seed, orient, -1, pos.ctypes.data_as(capi._fp),
                             nrm.ctypes.data_as(capi._fp), tri.ctypes.data_as(capi._ip), cap, C.byref(n))
    return rc, n.value, pos, nrm, tri


def test_capacity_and_a_total_of_zero():
    v, t, h, seed = CASES["count_257"]
    total = 262
    rc, n, pos, nrm, tri = _raw_sample(v, t, h, seed, total)
    assert rc == 0 and n == total
    _same((pos[:total], nrm[:total], tri[:total]), _ref("count_257")[1], "cap == total")
    assert np.all(pos[total:] == -12345.0) and np.all(nrm[total:] == -12345.0) and np.all(tri[total:] == -77)      # nothing behind the samples
    rc, n, pos, nrm, tri = _raw_sample(v, t, h, seed, total - 1)
    assert rc == CAPACITY and n == total
    assert np.all(pos == -12345.0) and np.all(nrm == -12345.0) and np.all(tri == -77)                               # the outputs are untouched
    v, t, h, seed = CASES["total_0"]
    rc, n, pos, nrm, tri = _raw_sample(v, t, h, seed, 0)
    assert rc == 0 and n == 0 and np.all(pos == -12345.0)


def test_overflow_is_refused_before_the_capacity_is_looked_at():
    from model_matching_amd import capi
    from model_matching_amd.estimator import mesh_sample_counts, preprocess_model_mesh
    v, t = mc.box()
    with pytest.raises(ValueError):
        ref.counts(v, t, 1e-7, 0)
    rc, n, pos, nrm, tri = _raw_sample(v, t, 1e-7, 0, 0)
    assert rc == INVALID and b"spacing" in capi.load().stocs_last_error() and n == 0 and np.all(pos == -12345.0)
    with pytest.raises(capi.StocsError, match="spacing"):
        mesh_sample_counts(v, t, 1e-7, 0)
    with pytest.raises(capi.StocsError, match="spacing"):
        preprocess_model_mesh(v, t, 0.005, spacing=1e-7)
    rc, n, pos, nrm, tri = _raw_sample(v, t, 2e-6, 0, 0)            # 6.2e9 samples, no triangle above 2^32 - 1: the total is what is refused
    assert rc == INVALID and b"spacing" in capi.load().stocs_last_error()


def test_second_call_of_the_same_size_allocates_nothing():
    from model_matching_amd import capi
    from model_matching_amd.estimator import mesh_sample, mesh_sample_counts, preprocess_model_mesh
    L = capi.load()
    v, t = synth.make_model_mesh(4)
    for call in (lambda: mesh_sample(v, t, 0.001, 1), lambda: mesh_sample_counts(v, t, 0.001, 1), lambda: preprocess_model_mesh(v, t, 0.005, seed=1)):
        first = call()
        before = L.stocs_device_alloc_count()
        second = call()
        assert L.stocs_device_alloc_count() == before
        for a, b in zip(first, second):
            assert np.array_equal(np.asarray(a), np.asarray(b))


# stocs_preprocess_model on a seeded cloud (1 664 points), as the library computed it on an MI355X before its tail moved into the helper the
# mesh path shares: SHA-256 of the positions' then the normals' bytes
PREPROCESS_MODEL_DIGEST = "8f85cf1d21f88b9eb127b0892865e2ef47394fa4a92d1767925b38ac938b228a"


def preprocess_model_digest():
    from model_matching_amd.estimator import preprocess_model
    raw = synth.make_model(3000).pos * F(1000.0)
    pos, nrm = preprocess_model(raw, 6.0, 5.0, 0.001)
    return hashlib.sha256(pos.tobytes() + nrm.tobytes()).hexdigest(), len(pos)


def test_preprocess_model_gives_the_bits_it_gave_before():
    digest, n = preprocess_model_digest()
    assert n > 300 and digest == PREPROCESS_MODEL_DIGEST


MODEL_CASES = [("box", mc.box, v, 0.0, 0) for v in mc.VOXELS] + [("Cm level 4", lambda: synth.make_model_mesh(4), 0.005, 0.0, 0),
                                                                   ("Cm level 4, spacing 2 mm, scale 1000, origin rule", lambda: synth.make_model_mesh(4), 0.01, 0.002, 1)]


@pytest.mark.parametrize("mi", range(len(MODEL_CASES)))
def test_preprocess_model_mesh_equals_the_restatement(mi):
    from oracle.ingest_oracle import voxel_grid
    from model_matching_amd.estimator import preprocess_model_mesh
    name, make, voxel, spacing, orient = MODEL_CASES[mi]
    scale = 1000.0 if orient else 1.0
    v, t = make()
    pos, nrm = preprocess_model_mesh(v, t, voxel, spacing=spacing, seed=mc.SEED, orient=orient, model_scale=scale)
    rpos, rnrm = ref.preprocess_model_mesh(v, t, voxel, spacing, mc.SEED, orient, scale, voxel_grid)
    what = "%s, voxel %g" % (name, voxel)
    assert len(pos) == len(rpos) and len(pos) > 50, what
    dp, dn = np.abs(pos - rpos).max(), np.abs(nrm - rnrm).max()
    print("%s: %d points, positions within %.3g (bound %.3g), normals within %.3g (bound %.3g)" % (what, len(pos), dp, 1e-6 * max(1.0, np.abs(pos).max()), dn, 2.0 ** -22))
    assert dp <= 1e-6 * max(1.0, np.abs(pos).max()), what
    assert dn <= 2.0 ** -22, what
