"""Seeded cases for stocs_segment_shapes / stocs_segment_assign, built on the generators of segment_cases.py and segment_convex_cases.py:
label frames around the 64 x 16 tile where the moment and extent kernels can go wrong, and ray-cast boxes and spheres for the gate.
A case is a dict(depth, labels, n_labels, K, scale, max_depth)."""
import numpy as np

import segment_cases as sc
import segment_convex_cases as scc

F = np.float32
SIZES = sc.SIZES
TABLE_SLOTS = 32          # stocs_segment_shapes_table; test_segment_shapes_abi_cpu.py checks the library says the same
N_LABELS = (0, 1, 2, 17, 300)


def case(depth, labels, n_labels, K, scale=sc.SCALE, max_depth=2.0):
    return dict(depth=np.ascontiguousarray(depth, np.uint16), labels=np.ascontiguousarray(labels, np.int32), n_labels=int(n_labels), K=K, scale=scale, max_depth=max_depth)


def table(W, H, seed=0):
    """an oblique plane with two slabs, 2 % holes (raw 0) and a wall at 1.7 m"""
    depth, K, _, _ = sc.table_frame(W, H, seed=seed, boxes=((W // 4, H // 4, W // 3, H // 3, 0.08),))
    return depth, K


def whole(W, H):
    """one label over the whole frame (holes included: labelled, not used)"""
    depth, K = table(W, H)
    return case(depth, np.ones((H, W)), 1, K)


def checker(W, H):
    """a per-pixel checkerboard of two labels: the wavefront's leading run is every second lane, the others add on their own"""
    depth, K = table(W, H, seed=1)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    return case(depth, 1 + (ii + jj) % 2, 2, K)


def blobs17(W, H, seed=2):
    """sc.blobs as the depth, 17 labels on 4 x 4 cells (0 among them), labels on zero-depth pixels too"""
    rng = np.random.default_rng(seed)
    depth = sc.blobs(W, H, seed)
    lab = np.kron(rng.integers(0, 18, ((H + 3) // 4, (W + 3) // 4)), np.ones((4, 4), np.int64))[:H, :W]
    return case(depth, lab, 17, sc.camera(W, H), max_depth=4.0)


def overflow(W, H):
    """300 labels, consecutive pixels consecutive labels: every tile holds far more labels than the LDS table has slots"""
    depth, K = table(W, H, seed=3)
    lab = 1 + np.arange(W * H).reshape(H, W) % 300
    assert len(np.unique(lab[:sc.TILE[1], :sc.TILE[0]])) > TABLE_SLOTS
    return case(depth, lab, 300, K)


def mixed(W, H):
    """three labels: label 1 with raw == 0 and z > max_depth pixels inside it, label 2 all invalid (raw 0), label 3 never present; labels
    n_labels + 1 and -1 in two corners"""
    depth = np.full((H, W), 1000, np.uint16)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    depth = (depth + 3 * jj + 5 * ii).astype(np.uint16)
    lab = np.zeros((H, W), np.int32)
    lab[:, : W // 2] = 1
    depth[2:5, 3:9] = 0
    depth[6:9, 3:9] = 2600                     # 2.6 m > max_depth 2.0
    lab[:, W // 2: W // 2 + 5] = 2
    depth[:, W // 2: W // 2 + 5] = 0
    lab[0:3, W - 4:] = 4
    lab[H - 3:, W - 4:] = -1
    return case(depth, lab, 3, sc.camera(W, H))


def far(W=65, H=17):
    """depth_scale 0.5 mm: raw 40000 is 20 m, at or beyond the 16 m the integer moments allow: labelled, valid, skipped as far"""
    depth = np.full((H, W), 2000, np.uint16)
    depth[::3, ::4] = 40000
    depth[1, 1] = 32000                        # exactly 16 m: far
    depth[1, 2] = 31999                        # just inside
    lab = np.ones((H, W), np.int32)
    lab[:, W // 2:] = 2
    return case(depth, lab, 2, sc.camera(W, H), scale=0.0005, max_depth=100.0)


def no_labels(W=65, H=17):
    """n_labels == 0: every non-zero label is out of range"""
    depth, K = table(W, H)
    lab = np.zeros((H, W), np.int32)
    lab[3:6, 3:20] = 1
    lab[8, 8] = -5
    return case(depth, lab, 0, K)


def big():
    """2048 x 2048 pixels of raw 65535 at just under 16 m, one label: Szz approaches 2^62"""
    W = H = 2048
    scale = float(F(15.9999) / F(65535))
    assert F(65535) * F(scale) < F(16)
    return case(np.full((H, W), 65535, np.uint16), np.ones((H, W), np.int32), 1, sc.camera(W, H), scale=scale, max_depth=16.0)


FRAMES = {"whole": whole, "checker": checker, "blobs17": blobs17, "overflow": overflow, "mixed": mixed}
FRAME_IDS = ["%s-%dx%d" % (name, W, H) for name in FRAMES for (W, H) in SIZES] + ["far", "no_labels"]
# the cases whose covariance has eigenvalue gaps of at least 5 % of the largest eigenvalue in every label that holds three used pixels or
# more: the axes are asserted on these (test_segment_shapes_cases_cpu.py checks the gaps)
SEPARATED = ["whole-%dx%d" % s for s in SIZES] + ["checker-%dx%d" % s for s in SIZES]
MIN_GAP = 0.05


def frame(case_id):
    if case_id == "far":
        return far()
    if case_id == "no_labels":
        return no_labels()
    name, size = case_id.split("-")
    W, H = (int(v) for v in size.split("x"))
    return FRAMES[name](W, H)


# ---- the gate: ray-cast scenes (segment_convex_cases.raycast), the object image as the labels, the objects' sizes from their dimensions
def sphere_size(r):
    return (F(2 * r), np.array([2 * r, 2 * r, 2 * r], F))


def box_size(a, b, h):
    return (F(np.sqrt(a * a + b * b + h * h)), np.array(sorted((a, b, h), reverse=True), F))


GATE_SCENES = {
    # a 6 cm sphere beside a 30 x 24 x 20 cm box: each is too small / too large for the other
    "sphere_and_big_box": dict(spheres=((-0.22, 0.0, 0.03),), boxes=((0.0, 0.30, -0.12, 0.12, 0.20),), objects=[sphere_size(0.03), box_size(0.30, 0.24, 0.20)]),
    # two boxes of like size: the gate keeps both segments for both objects
    "like_boxes": dict(boxes=((-0.16, -0.04, -0.05, 0.05, 0.09), (0.04, 0.17, -0.05, 0.05, 0.08)), objects=[box_size(0.12, 0.10, 0.09), box_size(0.13, 0.10, 0.08)]),
    "two_spheres": dict(spheres=((-0.10, 0.0, 0.06), (0.10, 0.0, 0.025)), objects=[sphere_size(0.06), sphere_size(0.025)]),
}
GATE_SIZE = (160, 120)


def gate_scene(name):
    """(case, objects): labels k = the k-th ray-cast body (spheres first, then boxes), 0 the table and the wall"""
    s = dict(GATE_SCENES[name])
    objects = s.pop("objects")
    depth, K, obj = scc.raycast(GATE_SIZE[0], GATE_SIZE[1], **s)
    lab = np.where(obj > 0, obj, 0)
    return case(depth, lab, int(lab.max()), K, max_depth=2.0), objects
