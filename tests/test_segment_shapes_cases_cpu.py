"""The numpy restatement of the segment shapes (tests/segment_shapes_ref.py) against itself and against independent arithmetic, and the
cases (tests/segment_shapes_cases.py) against what they are named for.  No GPU, no library."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import segment_cases as sc  # noqa: E402
import segment_shapes_cases as shc  # noqa: E402
import segment_shapes_ref as shr  # noqa: E402

F = np.float32


def ref(c):
    return shr.segment_shapes(c["depth"], c["labels"], c["K"], c["scale"], c["n_labels"], c["max_depth"])


@pytest.mark.parametrize("case_id", shc.FRAME_IDS)
def test_counts_and_moments_against_python_integers(case_id):
    c = shc.frame(case_id)
    P, lab, used, counts = shr.used_pixels(c["depth"], c["labels"], c["K"], c["scale"], c["n_labels"], c["max_depth"])
    assert counts["n_labelled"] == counts["n_used"] + counts["n_invalid"] + counts["n_far"]
    assert counts["n_out_of_range"] == int(((c["labels"] < 0) | (c["labels"] > c["n_labels"])).sum())
    M = shr.moments(P, lab, used, c["n_labels"])
    want = [[0] * 10 for _ in range(c["n_labels"])]
    for (i, j) in zip(*np.nonzero(used)):
        x, y, z = (int(round(float(v) * 65536.0)) for v in P[i, j])     # round(): nearest even, as rint; the product is exact in double
        for k, t in enumerate((1, x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
            want[lab[i, j] - 1][k] += t
    assert M.tolist() == want
    assert M[:, 0].sum() == counts["n_used"]


def test_the_cases_hold_what_they_are_named_for():
    assert set(shc.N_LABELS) <= {shc.frame(i)["n_labels"] for i in shc.FRAME_IDS}
    for W, H in shc.SIZES:
        c = shc.mixed(W, H)
        s, M, counts = ref(c)
        assert counts["n_out_of_range"] == 24 and counts["n_invalid"] > 18 and s[1]["flags"] == shr.EMPTY and s[2]["flags"] == shr.EMPTY and s[0]["n_used"] > 0
        assert (c["depth"][c["labels"] == 2] == 0).all() and s[1]["n_used"] == 0 and not s[1]["extent"].any() and not s[1]["axis"].any()
        o = shc.overflow(W, H)
        tile = o["labels"][:sc.TILE[1], :sc.TILE[0]]
        assert len(np.unique(tile)) > shc.TABLE_SLOTS
    c = shc.far()
    _, _, counts = ref(c)
    assert counts["n_far"] == int((c["depth"] >= 32000).sum()) and counts["n_far"] > 20 and counts["n_invalid"] == 0
    c = shc.no_labels()
    s, M, counts = ref(c)
    assert len(s) == 0 and counts["n_labelled"] == 0 and counts["n_out_of_range"] == 52
    b = shc.big()
    z = F(65535) * F(b["scale"])
    q = int(np.rint(np.float64(z) * 65536.0))
    assert z < 16 and 2 ** 61 < b["depth"].size * q * q < 2 ** 62 and b["depth"].size == 1 << 22


def test_key_map_is_monotone():
    t = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, np.inf], F)
    k = shr.key_of(t)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert shr.unkey(k).tobytes() == t.tobytes()


@pytest.mark.parametrize("case_id", shc.SEPARATED)
def test_axes_against_eigh_on_the_separated_cases(case_id):
    c = shc.frame(case_id)
    s, M, _ = ref(c)
    for l in range(c["n_labels"]):
        assert M[l, 0] >= 3
        w, ax = shr.eigh64(M[l])
        gaps = min(w[0] - w[1], w[1] - w[2])
        assert gaps >= shc.MIN_GAP * w[0], (case_id, l, w)
        _, _, _, flags, (ev, a64) = shr.axes_from_moments(M[l])
        assert flags == 0
        for k in range(3):
            assert shr.angle(a64[k], ax[k]) <= 1e-9, (case_id, l, k)           # the sweeps have converged: far below the float cast
            assert abs(ev[k] - w[k]) <= 1e-9 * w[0]
            assert shr.angle(s[l]["axis"][k], ax[k]) <= 1.2e-7                 # the cast moves a unit vector by about 1.1e-7 rad at most
            big = np.argmax(np.abs(a64[k]))
            assert a64[k][big] > 0
        assert abs(np.linalg.det(np.array(a64))) == pytest.approx(1.0, abs=1e-12)
        assert list(s[l]["eigenvalue"]) == sorted(s[l]["eigenvalue"], reverse=True)


def test_equal_eigenvalues_keep_the_lower_column_first_and_the_sign_rule():
    # an isotropic cloud: eight corners of a cube, the covariance is a multiple of the identity, no rotation happens
    pts = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (1.0, 2.0)], F)
    s, M = shr.points_shape(pts)
    assert s["n_used"] == 8 and s["axis"].tolist() == np.eye(3).tolist() and s["eigenvalue"][0] == s["eigenvalue"][1] == s["eigenvalue"][2] == F(0.25)
    assert s["extent"].tolist() == [1.0, 1.0, 1.0] and s["centroid"].tolist() == [0.0, 0.0, 1.5]
    assert shr.signed([-0.6, 0.6, 0.0]) == [0.6, -0.6, 0.0] and shr.signed([0.6, -0.6, 0.0]) == [0.6, -0.6, 0.0] and shr.signed([0.0, 0.0, -1.0]) == [0.0, 0.0, 1.0]


def test_the_non_finite_branch_of_the_restatement(monkeypatch):
    # integer moments cannot make a non-finite covariance (the library's branch says why), so one is forced: identity axes, zero eigenvalues,
    # a non-finite centroid component zeroed, the flag
    M = np.array([4, 0, 0, 4 * 65536, 0, 0, 0, 0, 0, 4 * 65536 * 65536], np.int64)
    assert shr.axes_from_moments(M)[3] == 0
    monkeypatch.setattr(shr, "covariance", lambda m: ([0.5, float("inf"), 1.0], [float("nan"), 0.0, 0.0, 1.0, 0.0, 2.0]))
    c, ev, ax, flags, _ = shr.axes_from_moments(M)
    assert flags == shr.NONFINITE and c.tolist() == [0.5, 0.0, 1.0] and ev.tolist() == [0.0, 0.0, 0.0] and ax.tolist() == np.eye(3).tolist()
    s = np.zeros(1, shr.SHAPE_DTYPE); s["n_used"] = 10; s["flags"] = flags; s["extent"] = 0.1
    assert shr.gate(s, [shc.box_size(0.1, 0.1, 0.1)]).tolist() == [[shr.NO_SHAPE]]


def test_extents_against_a_float64_projection():
    c = shc.whole(129, 33)
    P, lab, used, _ = shr.used_pixels(c["depth"], c["labels"], c["K"], c["scale"], c["n_labels"], c["max_depth"])
    s, _ = shr.shapes_from(P, lab, used, 1)
    t = (P[used].astype(np.float64) - s[0]["centroid"].astype(np.float64)) @ s[0]["axis"].astype(np.float64).T
    assert np.abs(t.min(axis=0) - s[0]["lo"]).max() < 1e-6 and np.abs(t.max(axis=0) - s[0]["hi"]).max() < 1e-6
    assert (s[0]["extent"] == s[0]["hi"] - s[0]["lo"]).all() and s[0]["extent"][0] > s[0]["extent"][1] > s[0]["extent"][2] > 0


def test_gate_on_the_ray_cast_scenes_and_the_stack():
    expect = {"sphere_and_big_box": [[0, shr.TOO_LARGE], [shr.TOO_SMALL, 0]], "like_boxes": [[0, 0], [0, 0]], "two_spheres": [[0, shr.TOO_SMALL], [shr.TOO_LARGE, 0]]}
    for name, want in expect.items():
        c, objects = shc.gate_scene(name)
        s, _, counts = ref(c)
        assert c["n_labels"] == 2 and (s["n_used"] > 50).all(), (name, s["n_used"])
        r = shr.gate(s, objects, **shr.GATE_DEFAULTS)
        assert r.tolist() == want, (name, r, s["extent"], objects)
        st = shr.stack(c["labels"], c["n_labels"], r)
        for k in range(2):
            allowed = [l + 1 for l in range(2) if r[k, l] == 0]
            assert ((st[k] == 10000) == np.isin(c["labels"], allowed)).all() and set(np.unique(st[k])) <= {0, 10000}
    # the bits are independent: an empty shape is NO_SHAPE and, beside an object with a middle extent, TOO_SMALL
    empty = np.zeros(1, shr.SHAPE_DTYPE); empty["flags"] = shr.EMPTY
    assert shr.gate(empty, [shc.box_size(0.1, 0.1, 0.1)]).tolist() == [[shr.NO_SHAPE | shr.TOO_SMALL]]
    d, e = shr.object_size([3.0, 4.0, 12.0])
    assert d == F(13.0) and shr.object_size([3.0, 4.0, 12.0], 12.5)[0] == F(12.5)
