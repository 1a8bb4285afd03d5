"""The mesh sampling contract on its own (tests/mesh_sample_ref.py, no library): the counts and their total, where the samples lie, the
box and the bowl, what the vertex path makes of the box, and the independence of a triangle's samples from the rest of the mesh."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_sample_cases as mc  # noqa: E402
import mesh_sample_ref as ref  # noqa: E402
from model_matching_amd import synth  # noqa: E402

F = np.float32


def test_hash_is_the_librarys_rng64():
    """the sample hash is stocs_math.h rng64(seed, t, j): one known answer computed by hand from the constants, in Python integers"""
    M = 2 ** 64 - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    for seed, t, j in ((0, 0, 0), (mc.SEED, 5, 7), (2 ** 64 - 1, 2 ** 22 - 1, 2 ** 32 - 2)):
        key = mix(mix((seed + 0x9E3779B97F4A7C15) & M) ^ ((t * 0xD1B54A32D192ED03 + 0x8CB92BA72F3D8DD7) & M))
        assert int(ref.tri_key(seed, t)[0]) == key
        assert ref.dither(seed, t)[0] == (key >> 40) / 2.0 ** 24


def test_counts_are_floor_or_floor_plus_one_and_the_total_follows_the_area():
    v, t = synth.make_model_mesh(4)
    assert len(t) == 6400
    for h in (0.002, 0.0005, 0.0101):
        n, area_total, total, skipped = ref.counts(v, t, h, mc.SEED)
        x = ref.triangle_terms(v, t, h)[3]
        assert skipped == 0 and np.all((n == np.floor(x)) | (n == np.floor(x) + 1)) and total == n.sum()
        expect = area_total / (np.float64(F(h)) ** 2)
        print("h %g: total %d, area/h^2 %.1f, difference %.1f, bound %.1f" % (h, total, expect, total - expect, 2 * np.sqrt(len(t))))
        assert abs(total - expect) <= 2 * np.sqrt(len(t))
    # many tiny triangles and a few large ones get the same density
    v5, t5 = synth.make_model_mesh(5)
    n5 = ref.counts(v5, t5, 0.002, mc.SEED)[2]
    a4, a5 = ref.counts(v, t, 0.002, mc.SEED)[1], ref.counts(v5, t5, 0.002, mc.SEED)[1]
    assert abs(n5 / a5 - ref.counts(v, t, 0.002, mc.SEED)[2] / a4) * 0.002 ** 2 < 0.02


def test_built_counts_are_what_the_cases_say():
    for ns in ([8], [0, 0, 0, 5, 0, 0, 0, 0, 7, 3, 0, 0], [3, 257, 2], [100, 0, 156]):
        v, t = mc.counted(ns)
        for seed in (0, 1, mc.SEED):
            assert ref.counts(v, t, mc.H, seed)[0].tolist() == ns
    v, t = mc.mesh_of([mc.right_triangle((4 * mc.H, 4 * mc.H), (0, 0, 0))])
    assert all(ref.counts(v, t, mc.H, s)[2] == 8 for s in range(16))
    v, t, none, one = mc.below_one()
    assert ref.counts(v, t, mc.H, none)[2] == 0 and ref.counts(v, t, mc.H, one)[2] == 1
    for kind in ("collinear", "repeated", "nan"):
        v, t = mc.degenerate(kind)
        n, area, total, skipped = ref.counts(v, t, mc.H, 3)
        assert n.tolist() == [3, 0, 2] and skipped == 1 and area == 5 * mc.H ** 2
    with pytest.raises(ValueError):
        ref.counts(*mc.box(), 1e-7, 0)      # 0.003 m^2 / 1e-14: above 2^32 - 1 on a triangle


def test_samples_lie_in_their_triangles():
    for v, t in (synth.make_model_mesh(3), mc.box(), mc.random_small(257, 1)):
        s = ref.sample(v, t, 0.001, mc.SEED)
        pos, nrm, tri = s[:3]
        u, w = ref.barycentrics(s)
        assert np.all(u >= 0) and np.all(w >= 0) and np.all(u + w < 1) and len(pos) == ref.counts(v, t, 0.001, mc.SEED)[2]
        assert np.all(np.diff(tri) >= 0)                                                  # (t, j) order
        A = v[t[tri, 0]].astype(np.float64)
        scale = np.abs(v).max()
        assert np.abs(((pos - A) * nrm.astype(np.float64)).sum(axis=1)).max() <= 8 * np.finfo(F).eps * scale          # in the plane, to float rounding
        assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() <= 2 * np.finfo(F).eps


@pytest.mark.parametrize("voxel", mc.VOXELS)
def test_box_has_axis_normals_on_all_six_faces(voxel):
    v, t = mc.box()
    pos, nrm, tri = ref.sample(v, t, voxel / 4, mc.SEED)[:3]
    faces = set()
    half = np.asarray(mc.BOX_SIZE) / 2
    for p, n in zip(pos, nrm):
        ax = int(np.flatnonzero(n != 0)[0])
        assert np.count_nonzero(n) == 1 and abs(n[ax]) == 1.0 and abs(p[ax] - n[ax] * half[ax]) < 1e-7       # outward, on its face
        faces.add((ax, float(n[ax])))
    assert len(faces) == 6


def test_vertex_path_makes_nothing_of_the_box():
    from oracle import ingest_oracle
    v, _ = mc.box()
    pos, nrm = ingest_oracle.preprocess_model(v, 0.005, 0.01, 1.0)
    assert len(pos) == 0 and len(nrm) == 0


def test_bowl_winding_orients_every_sample_and_the_origin_rule_does_not():
    v, t, wall = mc.bowl()
    pos0, nrm0, tri0 = ref.sample(v, t, 0.003, mc.SEED, orient=0)[:3]
    pos1, nrm1, tri1 = ref.sample(v, t, 0.003, mc.SEED, orient=1)[:3]
    assert np.array_equal(pos0, pos1) and np.array_equal(tri0, tri1)
    true = mc.bowl_true_normal(pos0.astype(np.float64), wall[tri0])
    wrong0 = (nrm0 * true).sum(axis=1) < 0
    wrong1 = (nrm1 * true).sum(axis=1) < 0
    assert not wrong0.any()
    for w in (0, 1):
        share = wrong1[wall[tri0] == w].mean()
        print("wall %d: the origin rule turns %.0f %% of %d samples against the surface" % (w, 100 * share, (wall[tri0] == w).sum()))
        assert share > 0


def test_a_triangles_samples_do_not_move_when_others_change():
    v, t = synth.make_model_mesh(2)
    pos, nrm, tri = ref.sample(v, t, 0.002, mc.SEED)[:3]
    v2 = v.copy()
    keep = 17
    others = np.setdiff1d(np.arange(len(v)), t[keep])
    v2[others] *= F(1.5)                                                     # every other vertex moves
    t2 = np.concatenate([t, t[:40][:, [0, 2, 1]]])                           # and triangles are appended
    pos2, nrm2, tri2 = ref.sample(v2, t2, 0.002, mc.SEED)[:3]
    a, b = tri == keep, tri2 == keep
    assert a.sum() > 0 and np.array_equal(pos[a].view(np.uint32), pos2[b].view(np.uint32)) and np.array_equal(nrm[a].view(np.uint32), nrm2[b].view(np.uint32))
    assert not np.array_equal(ref.sample(v, t, 0.002, mc.SEED + 1)[0][:8], pos[:8])
