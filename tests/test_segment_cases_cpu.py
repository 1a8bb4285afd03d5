"""The restatement of stocs_segment_frame (tests/segment_ref.py) on its own, no GPU: components against a plain breadth-first search, a case
per pixel class, tolerance and jump at equality and one float either side, the edge rule against a flood fill, the refit against a float64 SVD
fit of the unquantised inliers."""
from collections import deque

import numpy as np
import pytest

import segment_cases as sc
import segment_ref as sr

F = np.float32


def bfs_roots(fg, z, ja, jr):
    H, W = fg.shape
    root = np.full((H, W), -1, np.int64)
    ja, jr = F(ja), F(jr)
    for i0 in range(H):
        for j0 in range(W):
            if not fg[i0, j0] or root[i0, j0] >= 0:
                continue
            r = i0 * W + j0                                  # raster order: the first pixel met is the component's lowest index
            root[i0, j0] = r
            todo = deque([(i0, j0)])
            while todo:
                i, j = todo.popleft()
                for a, b in ((i, j - 1), (i, j + 1), (i - 1, j), (i + 1, j)):
                    if 0 <= a < H and 0 <= b < W and fg[a, b] and root[a, b] < 0 and abs(F(z[i, j] - z[a, b])) <= F(ja + F(jr * min(z[i, j], z[a, b]))):
                        root[a, b] = r
                        todo.append((a, b))
    return root


@pytest.mark.parametrize("name", ["blobs0", "blobs1", "serpentine", "checkerboard", "diagonal", "relative"])
def test_components_against_a_breadth_first_search(name):
    W, H = 65, 33
    jr = 0.0
    d = {"blobs0": lambda: sc.blobs(W, H, 0), "blobs1": lambda: sc.blobs(W, H, 1), "serpentine": lambda: sc.serpentine(W, H),
         "checkerboard": lambda: sc.checkerboard(W, H), "diagonal": lambda: sc.diagonal_pair(W, H), "relative": lambda: sc.blobs(W, H, 2)}[name]()
    if name == "relative":
        jr = 0.019
    z = d.astype(F) * F(sc.SCALE)
    fg = d != 0
    got = sr.components(fg, z, 0.005, jr)
    want = bfs_roots(fg, z, 0.005, jr)
    assert np.array_equal(got, want)
    n = np.unique(want[want >= 0]).size
    if name == "serpentine":
        assert n == 1
    if name == "checkerboard":
        assert n == W * H
    if name == "diagonal":
        assert n == 2
    if name.startswith("blobs"):
        assert n > 10


def test_a_case_per_pixel_class():
    boxes = ((20, 45, 20, 16, 0.08), (60, 50, 20, 16, -0.05), (90, 60, 16, 12, 0.62))     # standing on it, a pit below it, above max_height
    depth, K, (n, d), m = sc.table_frame(boxes=boxes, holes=0.03, seed=3)
    p = sr.params()
    P, valid = sr.points(depth, K, sc.SCALE, p["max_depth"])
    assert np.array_equal(valid, ~m["hole"])                                               # a hole is not valid; the wall (1.7 m) is
    cl = sr.classify(P, valid, np.array([n[0], n[1], n[2], d], F), p)
    assert cl["on"][m["table"]].all() and not cl["fg"][m["table"]].any()                   # depth is rounded to 1 mm, tol is 10
    assert cl["fg"][m["box"][0]].all() and cl["above"][m["box"][0]].all()
    assert cl["below"][m["box"][1]].all() and not cl["fg"][m["box"][1]].any()
    assert cl["above"][m["box"][2]].all() and not cl["fg"][m["box"][2]].any()
    assert not (cl["on"] | cl["above"] | cl["below"])[m["hole"]].any()
    assert np.array_equal(cl["on"] | cl["above"] | cl["below"], valid) and not (cl["on"] & cl["above"]).any() and not (cl["on"] & cl["below"]).any()
    far = sr.points(depth, K, sc.SCALE, 1.5)[1]
    assert not far[m["wall"]].any() and far[m["box"][0]].all()                             # beyond max_depth: not valid
    none = sr.classify(P, valid, None, p)
    assert np.array_equal(none["fg"], valid) and not none["on"].any()


def test_tolerance_at_equality_and_one_float_either_side():
    P = np.zeros((1, 1, 3), F); P[0, 0] = (0.1, -0.2, 1.0)
    valid = np.ones((1, 1), bool)
    plane = np.array([0, 0, -1, 1.03], F)
    h = F(F(0) * P[0, 0, 0] + F(F(0) * P[0, 0, 1] + F(-1) * P[0, 0, 2])) + F(1.03)
    assert h > 0
    for tol, want in ((h, "on"), (np.nextafter(h, F(0)), "above"), (np.nextafter(h, F(1)), "on")):
        cl = sr.classify(P, valid, plane, sr.params(plane_tolerance=tol))
        assert cl[want][0, 0] and cl["fg"][0, 0] == (want == "above"), (tol, want)
    for mh, fg in ((h, True), (np.nextafter(h, F(0)), False)):                             # h <= max_height
        assert sr.classify(P, valid, plane, sr.params(plane_tolerance=0.001, max_height=mh))["fg"][0, 0] == fg
    low = np.array([0, 0, -1, 0.97], F)
    hl = F(F(-1) * P[0, 0, 2]) + F(0.97)
    for tol, want in ((-hl, "on"), (np.nextafter(-hl, F(0)), "below")):
        assert sr.classify(P, valid, low, sr.params(plane_tolerance=tol))[want][0, 0]


def test_jump_at_equality_and_one_float_either_side():
    d, step = sc.jump_pair(8, 2)
    z = d.astype(F) * F(sc.SCALE)
    fg = d != 0
    for ja, n in ((step, 1), (np.nextafter(step, F(0)), 2), (np.nextafter(step, F(1)), 1)):
        assert np.unique(sr.components(fg, z, ja, 0.0)).size == n, ja
    rel = F(0.004)
    thr = F(rel * z.min())                                                                  # jump_abs 0: the relative term alone
    ja = F(step - thr)
    assert F(ja + thr) == step                                                              # exactly representable here
    assert np.unique(sr.components(fg, z, ja, rel)).size == 1
    assert np.unique(sr.components(fg, z, np.nextafter(ja, F(0)), rel)).size == (1 if F(np.nextafter(ja, F(0)) + thr) >= step else 2)


def flood8(open_px, start):
    H, W = open_px.shape
    seen = np.zeros((H, W), bool)
    seen[start] = True
    todo = deque([start])
    while todo:
        i, j = todo.popleft()
        for a in (i - 1, i, i + 1):
            for b in (j - 1, j, j + 1):
                if 0 <= a < H and 0 <= b < W and open_px[a, b] and not seen[a, b]:
                    seen[a, b] = True
                    todo.append((a, b))
    return seen


@pytest.mark.parametrize("seed", [0, 1])
def test_a_flood_fill_over_non_edge_pixels_stays_in_its_segment(seed):
    d = sc.blobs(96, 64, seed)
    out = sr.segment_frame(d, sc.camera(96, 64), sc.SCALE, **dict(sc.LABEL, min_pixels=12))
    labels, edge = out["labels"], out["edge"]
    assert out["n_segments"] >= 3
    assert set(np.unique(edge)) <= {0, 255} and not edge[labels == 0].any()
    started = 0
    for k in range(1, out["n_segments"] + 1):
        inner = (labels == k) & (edge == 255)
        todo = inner.copy()
        reached = np.zeros_like(inner)
        while todo.any():                                   # a segment's interior may fall into several 8-connected pieces: start in each
            i, j = np.argwhere(todo)[0]
            seen = flood8(edge == 255, (i, j))
            assert (labels[seen] == k).all(), k             # the fill never leaves the segment
            reached |= seen; todo &= ~seen; started += 1
        assert np.array_equal(reached, inner)
    assert started >= out["n_segments"] // 2


def test_the_refit_against_a_float64_fit_of_the_unquantised_inliers():
    worst = 0.0
    for seed, noise in ((0, 0.0), (1, 1.0), (2, 2.0)):
        depth, K, (n, d), m = sc.table_frame(seed=seed, noise_mm=noise)
        out = sr.segment_frame(depth, K, sc.SCALE, seed=seed + 1)
        assert out["plane_found"] == 1 and out["n_refit"] == out["moments"][0] >= 3
        pts = out["P"][out["inl"]].astype(np.float64)
        n64, d64 = sr.fit64(pts)
        nq, dq = sr.plane_from_moments(out["moments"])
        theta, bound_d, _ = sc.plane_bound(pts)
        assert theta < 0.01
        assert np.linalg.norm(nq - n64) <= theta + 1e-12 and abs(dq - d64) <= bound_d + 1e-12
        worst = max(worst, np.linalg.norm(nq - n64) / theta, abs(dq - d64) / bound_d)
        assert np.degrees(np.arccos(min(1.0, abs(float(n64 @ n))))) < 1.0 and abs(d64 - d) < 0.01    # and it is the table
        assert out["n_segments"] == 2 and out["labels"][m["box"][0]].all() and out["labels"][m["box"][1]].all()
    assert worst < 1.0


def test_winner_and_share():
    depth, K, _, _ = sc.table_frame(seed=5)
    a = sr.segment_frame(depth, K, sc.SCALE)
    assert a["plane_found"] == 1 and a["winner_count"] == max(a["counts"]) and a["counts"].index(a["winner_count"]) == a["winner"]
    b = sr.segment_frame(depth, K, sc.SCALE, plane_min_share=1.0)
    assert b["plane_found"] == 0 and b["winner"] == a["winner"] and b["n_refit"] == 0 and np.array_equal(b["fg"], b["valid"])
    c = sr.segment_frame(depth, K, sc.SCALE, plane_hypotheses=0)
    assert c["plane_found"] == 0 and c["winner"] == -1 and c["n_on_plane"] == 0
