"""The restatement of the concavity cut (tests/segment_convex_ref.py) alone, on the cases of tests/segment_convex_cases.py: every case holds
what it is named for, the thresholds are met from either side, and the scenes of the GPU tests meet their conditions here before a GPU
sees them.  No GPU."""
import numpy as np
import pytest

import segment_cases as sc
import segment_convex_cases as cc
import segment_convex_ref as cr
import segment_ref as sr

F = np.float32


def run(depth, W, H, convex, **kw):
    return cr.segment_frame_convex(depth, sc.camera(W, H), cc.SCALE, convex=convex, **dict(cc.LABEL, **kw))


@pytest.mark.parametrize("W,H", cc.SIZES)
def test_a_valley_is_cut_in_two_along_its_crease_also_on_a_tile_border(W, H):
    frames = cc.label_frames(W, H)
    seen = 0
    for name, (depth, cv) in frames.items():
        if not name.startswith("valley-col") and not name.startswith("valley-row"):
            continue
        out = run(depth, W, H, cv)
        r = cv["bend_radius"]
        axis = "h" if "col" in name else "v"
        assert out["plain"]["n_components"] == 1, name
        assert out["n_cut_" + axis] > 0 and out["n_cut_" + ("v" if axis == "h" else "h")] == 0, (name, {k: out[k] for k in cr.COUNTS})
        assert out["n_components"] == 2 and out["n_segments"] == 2, (name, out["n_components"])
        # the two pixels either side of the crease are cut along its whole length, and nothing farther than r from it
        if axis == "h":
            col = 64 if W > 64 + r else W // 2
            assert out["cut_h"][:, col - 1:col + 1].all() and not out["cut_h"][:, :max(col - 1 - r, 0)].any() and not out["cut_h"][:, col + 1 + r:].any(), name
            if W > 64 + r:
                assert col % sc.TILE[0] == 0
        else:
            row = 16 if H > 16 + r else H // 2
            assert out["cut_v"][row - 1:row + 1].all() and not out["cut_v"][:max(row - 1 - r, 0)].any() and not out["cut_v"][row + 1 + r:].any(), name
            if H > 16 + r:
                assert row % sc.TILE[1] == 0
        seen += 1
    assert seen >= 2


@pytest.mark.parametrize("W,H", cc.SIZES)
def test_a_crease_within_the_radius_of_the_border_and_a_ridge_are_not_cut(W, H):
    frames = cc.label_frames(W, H)
    for name, (depth, cv) in frames.items():
        if name.startswith("valley-border"):
            out = run(depth, W, H, cv)
            r = cv["bend_radius"]
            # the crease lies on column r - 1: no triple is centred on it or left of it, so it is not cut, whatever happens farther in
            assert not out["tested_h"][:, :r].any() and not out["tested_h"][:, W - r:].any() and out["n_tested_h"] == H * (W - 2 * r), name
            assert not out["cut_h"][:, :r].any() and out["n_cut_v"] == 0, name
            inner = run(cc.valley(W, H, col=W // 2, top=900, on_pixel=True), W, H, cv)               # the same valley away from the border is cut on its crease
            assert inner["cut_h"][:, W // 2].all(), name
        if name.startswith("ridge"):
            out = run(depth, W, H, cv)
            assert out["n_tested_h"] > 0 and out["n_cut"] == 0 and out["n_components"] == 1, name
            r = cv["bend_radius"]
            col = 64 if W > 64 + r else W // 2
            t = cr.triple(out["Ps"][:, col - r], out["Ps"][:, col], out["Ps"][:, col + r], r, cc.LABEL["jump_abs"], cc.LABEL["jump_rel"], cr.CONVEX_DEFAULTS["bend_cos"])
            assert t["tested"].all() and t["bend"].all() and not t["toward"].any(), name     # it bends as much as the valley, away from the viewer


def test_a_hole_and_a_jump_inside_the_window_do_not_count():
    W, H = 65, 17
    depth, look = cc.hole_and_jump(W, H)
    out = run(depth, W, H, dict(bend_radius=1, smooth_radius=4))
    raw = depth.astype(np.int64)
    for (i, j) in look:
        ys, xs = slice(max(i - 4, 0), min(i + 5, H)), slice(max(j - 4, 0), min(j + 5, W))
        win = raw[ys, xs]
        same = (win != 0) & (np.abs(win - raw[i, j]) <= 5)                                  # LABEL: 5 mm, no relative part; levels are 300 mm apart
        assert out["S"][i, j] == win[same].sum() and out["N"][i, j] == same.sum() and same.sum() < win.size, (i, j)
        assert out["smoothed"][i, j] == (F(out["S"][i, j]) / F(out["N"][i, j])) * F(cc.SCALE)
    assert np.isnan(out["smoothed"][4, 6]) and out["cut"][4, 6] == 0
    assert np.isnan(out["smoothed"]).sum() == 1


@pytest.mark.parametrize("r", [1, 8])
def test_a_far_pixel_one_raw_unit_beyond_the_scaled_jump_is_not_tested(r):
    W, H = 65, 17
    at, above, (i, j) = cc.far_pixel_pair(W, H, r)
    cv = dict(bend_radius=r, smooth_radius=0)
    a, b = run(at, W, H, cv), run(above, W, H, cv)
    assert a["tested_h"][i, j] and not b["tested_h"][i, j]
    assert a["tested_h"][i, j + 2 * r] and not b["tested_h"][i, j + 2 * r]                  # the pixel is the left end of that triple
    assert int(above[i, j + r]) - int(at[i, j + r]) == 1


def test_bend_cos_at_a_pixels_own_threshold_and_one_float_either_side():
    W, H = 65, 17
    depth = cc.valley(W, H, col=32, slope=2)
    r, (i, j) = 4, (8, 31)
    base = run(depth, W, H, dict(bend_radius=r, smooth_radius=2))
    t = cr.triple(base["Ps"][i, j - r], base["Ps"][i, j], base["Ps"][i, j + r], r, cc.LABEL["jump_abs"], cc.LABEL["jump_rel"], 0.5)
    assert t["tested"] and t["toward"] and t["ab"] > 0
    ratio = np.float64(t["ab"] * t["ab"]) / np.float64(t["aa"] * t["bb"])
    c0 = F(np.sqrt(ratio))                                                                  # bend_cos whose square is nearest the pixel's own ratio
    seen = set()
    for c in (np.nextafter(c0, F(0)), c0, np.nextafter(c0, F(2))):
        out = run(depth, W, H, dict(bend_radius=r, smooth_radius=2, bend_cos=float(c)))
        want = bool(t["ab"] * t["ab"] < (F(c) * F(c)) * (t["aa"] * t["bb"]))              # the contract's own comparison, in float32
        assert bool(out["cut_h"][i, j]) == want, float(c)
        seen.add(want)
    assert seen == {False, True}                                                            # the three values straddle the threshold
    assert not run(depth, W, H, dict(bend_radius=r, smooth_radius=2, bend_cos=0.0))["n_cut"]
    assert run(depth, W, H, dict(bend_radius=r, smooth_radius=2, bend_cos=1.0))["cut_h"][i, j]


def test_the_window_sum_is_exact_at_the_largest_window_and_raw_depth():
    W, H = 20, 12
    depth = sc.blank(W, H, 65535)
    p = sr.params(**dict(cc.LABEL, max_depth=70.0))
    S, N = cr.window_sums(depth, depth != 0, cc.SCALE, p["jump_abs"], p["jump_rel"], 4)
    assert S.max() == 81 * 65535 < 2 ** 24 and N.max() == 81 and S[0, 0] == 25 * 65535
    assert (F(S.max()) == np.float64(S.max())) and int(F(S.max())) == 81 * 65535           # exact as a float
    out = cr.segment_frame_convex(depth, sc.camera(W, H), cc.SCALE, convex=dict(smooth_radius=4, bend_radius=1), **dict(cc.LABEL, max_depth=70.0))
    assert (out["smoothed"] == F(65535) * F(cc.SCALE)).all()


def test_no_smoothing_gives_step_ones_depth_and_no_radius_gives_the_plain_result():
    W, H = 65, 33
    depth = sc.blobs(W, H, 5)
    out = run(depth, W, H, dict(bend_radius=4, smooth_radius=0))
    fg = out["plain"]["fg"]
    assert np.array_equal(out["smoothed"][fg], out["P"][..., 2][fg]) and np.isnan(out["smoothed"][~fg]).all()
    assert np.array_equal(out["Ps"][fg], out["P"][fg])
    zero = run(depth, W, H, dict(bend_radius=0, smooth_radius=2))
    assert all(zero[k] == 0 for k in cr.COUNTS) and not zero["cut"].any()
    for k in ("labels", "class_prob", "edge"):
        assert np.array_equal(zero[k], zero["plain"][k])
    assert zero["records"] == zero["plain"]["records"] and zero["n_components"] == zero["plain"]["n_components"]


def test_the_neighbours_of_a_cut_pixel_are_edges():
    W, H = 129, 33
    out = run(cc.valley(W, H, col=64), W, H, dict(bend_radius=4, smooth_radius=2))
    cut = out["cut"] != 0
    assert (out["labels"][cut] == 0).all() and (out["class_prob"][cut] == 0).all()
    near = np.zeros_like(cut)
    near[:, 1:] |= cut[:, :-1]; near[:, :-1] |= cut[:, 1:]
    assert (out["edge"][near & ~cut & (out["labels"] != 0)] == 0).all() and (near & ~cut & (out["labels"] != 0)).any()


@pytest.mark.parametrize("noise", cc.NOISES)
@pytest.mark.parametrize("name", ["two_spheres", "box_behind_box"])
def test_touching_objects_are_one_segment_plain_and_two_pure_ones_with_the_defaults(name, noise):
    depth, K, obj = cc.scene(name, noise)
    out = cr.segment_frame_convex(depth, K, cc.SCALE, **cc.SCENE_PARAMS)
    assert out["plane_found"] == 1 and out["plain"]["n_segments"] == 1 and out["n_segments"] == 2, (out["plain"]["n_segments"], out["n_segments"])
    pure = cc.purity(out["labels"], obj)
    assert sorted(o for _, _, o, _ in pure) == [1, 2] and all(share == 1.0 for _, _, _, share in pure), pure
    assert cc.purity(out["plain"]["labels"], obj)[0][3] < 0.7                              # the plain segment is a mixture


@pytest.mark.parametrize("noise", cc.NOISES)
@pytest.mark.parametrize("name", ["lone_sphere", "lone_box"])
def test_a_lone_convex_object_stays_one_segment_and_loses_at_most_two_percent(name, noise):
    depth, K, obj = cc.scene(name, noise)
    out = cr.segment_frame_convex(depth, K, cc.SCALE, **cc.SCENE_PARAMS)
    assert out["plane_found"] == 1 and out["plain"]["n_segments"] == 1 and out["n_segments"] == 1
    fg = out["plain"]["fg"] & (obj == 1)
    lost = int(((out["cut"] != 0) & fg).sum())
    print("[segment convex] %s noise %g mm: %d of %d foreground pixels cut" % (name, noise, lost, int(fg.sum())))
    assert lost <= 0.02 * fg.sum()
