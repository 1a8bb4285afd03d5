"""Hand-built and seeded inputs of the scene-selection tests (tests/test_scene_cases_cpu.py, tests/test_scene_gpu.py): pools for the walk of
stocs_scene_select, each named for the branch it must reach, and the small models, poses and frames of the footprint tests.  Depends on
numpy and scene_ref alone.  Not a test module."""
import numpy as np

import scene_ref as ref

F = np.float32


# ---- pools for the walk ----
def records_for(masks, in_front=None, footprint=None):
    """footprint records that make every slot pass the violation test unless told otherwise: footprint = agree = claimed = own"""
    masks = np.asarray(masks, bool)
    rec = np.zeros(len(masks), ref.RECORD_DTYPE)
    own = masks.sum(axis=1) if len(masks) else np.zeros(0, int)
    rec["footprint"] = own if footprint is None else footprint
    rec["agree"] = own; rec["claimed"] = own
    rec["in_front"] = 0 if in_front is None else in_front
    return rec


def pool(name, npix, claims, score=None, group=None, n_groups=None, cap=None, rec=None, **params):
    """claims: one iterable of pixel indices per slot; the scores default to descending in slot order, so that the order is the slot order"""
    n = len(claims)
    masks = np.zeros((n, npix), bool)
    for h, px in enumerate(claims):
        masks[h, list(px)] = True
    score = np.asarray([1.0 - h / 65536.0 for h in range(n)] if score is None else score, F)
    group = np.zeros(n, np.int32) if group is None else np.asarray(group, np.int32)
    n_groups = (int(group.max()) + 1 if n else 1) if n_groups is None else n_groups
    return dict(name=name, masks=masks, score=score, group=group, n_groups=n_groups, cap=None if cap is None else np.asarray(cap, np.int32),
                rec=records_for(masks) if rec is None else rec, params=params)


def run_ref(c, per_round=None):
    return ref.select(c["masks"], c["score"], c["group"], c["rec"], c["n_groups"], c["cap"], per_round=per_round, **c["params"])


def R(a, b):
    return range(a, b)


def hand_pools():
    """name -> pool; what each must reach is asserted from these inputs in tests/test_scene_cases_cpu.py (EXPECT below)"""
    P = []
    for npix in (1, 31, 32, 33, 129):                        # the last pixel of the frame decides: slot 1 claims only it, slot 2 repeats slot 0
        P.append(pool("npix_%d" % npix, npix, [R(0, max(npix - 1, 1)), [npix - 1], R(0, max(npix - 1, 1))], min_pixels=1))
    top = 1 << 19
    P.append(pool("npix_2^19", top, [list(R(0, 100)) + [top - 1], list(R(40, 100)) + [top - 1], R(top - 200, top - 1)], min_pixels=1))
    for n in (1, 15, 16, 17, 33):                            # pairs: every odd slot repeats the even slot in front of it
        P.append(pool("n_%d" % n, 80, [[2 * (h // 2), 2 * (h // 2) + 1] for h in range(n)], min_pixels=1))
    small = [[200 + h] for h in range(15)]                   # own 1 < min_pixels 2: not eligible
    P.append(pool("mid_round", 256, small[:5] + [R(0, 8), R(0, 8), R(8, 16)] + [R(4, 12)] * 10, min_pixels=2))
    P.append(pool("round_boundary", 256, small + [R(0, 8), R(8, 16), R(8, 16), R(16, 24)], min_pixels=2))
    P.append(pool("max_selected_mid_round", 256, [R(8 * h, 8 * h + 8) for h in range(20)], min_pixels=2, max_selected=3))
    P.append(pool("one_group_cap_1", 256, [R(8 * h, 8 * h + 8) for h in range(20)], cap=[1], min_pixels=2))
    P.append(pool("groups_1024", 64, [R(0, 8), R(8, 16), R(16, 24), R(24, 32)], group=[0, 1023, 1023, 512], n_groups=1024, cap=[1] * 1024, min_pixels=2))
    P.append(pool("equal_scores", 64, [R(0, 8), R(0, 8), R(8, 16), R(8, 16)], score=[0.5, 0.5, 0.75, 0.75], min_pixels=2))
    P.append(pool("bad_scores", 64, [R(8 * h, 8 * h + 8) for h in range(7)], score=[0.0, -1.0, float("nan"), -0.0, float("inf"), 1e-30, float("-inf")], min_pixels=2))
    P.append(pool("excl_at_min_pixels", 64, [R(0, 10), R(5, 15), list(R(0, 6)) + list(R(20, 24))], min_pixels=5, min_exclusive_fraction=0.1))
    P.append(pool("fraction_half_of_8", 64, [R(0, 4), R(0, 8), [0, 1, 2, 3, 4, 8, 9, 10]], min_pixels=1, min_exclusive_fraction=0.5))
    m = [R(0, 4), R(8, 12)]
    mk = np.zeros((2, 64), bool); mk[0, 0:4] = True; mk[1, 8:12] = True
    P.append(pool("violation_quarter", 64, m, rec=records_for(mk, in_front=[1, 2], footprint=[4, 7]), min_pixels=1, max_violation_fraction=0.25))
    P.append(pool("every_reason", 64, [R(0, 8), R(8, 16), R(0, 8), R(16, 24), R(24, 32), R(32, 40)], score=[0.9, 0.0, 0.8, 0.7, 0.6, 0.5], group=[0, 0, 0, 0, 1, 2],
                  cap=[1, 5, 5], min_pixels=2, max_selected=2))
    return {c["name"]: c for c in P}


# name -> (ranks by slot, reasons by slot): what the inputs above were built to give
EXPECT = {
    "npix_1": ([0, -1, -1], [0, 2, 2]),
    "npix_33": ([0, 1, -1], [0, 0, 2]),
    "npix_2^19": ([0, -1, 1], [0, 2, 0]),
    "n_17": ([h // 2 if h % 2 == 0 else -1 for h in range(17)], [0 if h % 2 == 0 else 2 for h in range(17)]),
    "mid_round": ([-1] * 5 + [0, -1, 1] + [-1] * 10, [1] * 5 + [0, 2, 0] + [2] * 10),
    "round_boundary": ([-1] * 15 + [0, 1, -1, 2], [1] * 15 + [0, 0, 2, 0]),
    "max_selected_mid_round": ([0, 1, 2] + [-1] * 17, [0, 0, 0] + [4] * 17),
    "one_group_cap_1": ([0] + [-1] * 19, [0] + [3] * 19),
    "groups_1024": ([0, 1, -1, 2], [0, 0, 3, 0]),
    "equal_scores": ([1, -1, 0, -1], [0, 2, 0, 2]),
    "bad_scores": ([-1, -1, -1, -1, 0, 1, -1], [1, 1, 1, 1, 0, 0, 1]),
    "excl_at_min_pixels": ([0, 1, -1], [0, 0, 2]),
    "fraction_half_of_8": ([0, 1, -1], [0, 0, 2]),
    "violation_quarter": ([0, -1], [0, 1]),
    "every_reason": ([0, -1, -1, -1, 1, -1], [0, 1, 2, 3, 0, 4]),
}


def random_pool(seed):
    """at most 40 slots and 300 pixels; ties, non-positive and NaN scores, caps, violations and every parameter drawn"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 41)); npix = int(rng.integers(1, 301)); n_groups = int(rng.integers(1, 6))
    centres = rng.integers(0, npix, n)
    widths = rng.integers(1, max(2, npix // 3 + 1), n)
    masks = np.zeros((n, npix), bool)
    for h in range(n):
        if rng.random() < 0.3 and h:                         # near copies of an earlier slot
            masks[h] = masks[rng.integers(0, h)] ^ (rng.random(npix) < 0.05)
        else:
            masks[h, max(0, centres[h] - widths[h]):centres[h] + widths[h]] = True
            masks[h] &= rng.random(npix) < 0.9
    score = rng.choice(np.array([0.25, 0.5, 0.5, 0.75, 0.9, 0.0, -1.0, np.nan], F), n).astype(F)
    score = np.where(rng.random(n) < 0.5, score, rng.random(n).astype(F)).astype(F)
    foot = masks.sum(axis=1) + rng.integers(0, 10, n)
    rec = records_for(masks, in_front=rng.integers(0, 6, n), footprint=foot)
    cap = None if rng.random() < 0.4 else rng.integers(1, 4, n_groups).astype(np.int32)
    return dict(name="random_%d" % seed, masks=masks, score=score, group=rng.integers(0, n_groups, n).astype(np.int32), n_groups=n_groups, cap=cap, rec=rec,
                params=dict(max_selected=int(rng.integers(1, n + 2)), min_pixels=int(rng.integers(1, 7)),
                            min_exclusive_fraction=float(rng.choice([0.1, 0.25, 0.5, 0.75, 1.0])), max_violation_fraction=float(rng.choice([0.0, 0.1, 0.25, 0.5, 1.0]))))


def walk_pair(seed):
    """the same sets for the two entry points of the shared cover walk: a rows case of instances_cases.random_rows (40 hypotheses, more than
    two rounds of sixteen; 300 scene points, a row of 10 words padded to 12) with its scores made strictly positive, ties kept, and the pool
    that is the same selection to stocs_scene_select: every hypothesis's counted hits as a pixel mask of 300 bits, one group without a cap,
    no violation, min_pixels = min_points, the same fraction and maximum -> (rows case, pool)"""
    import instances_cases
    import instances_ref
    rows = instances_cases.random_rows(seed, n=40, nS=300)
    rows["lcp"] = (rows["lcp"] + F(1.0 / 64)).astype(F)
    assert (rows["lcp"] > 0).all() and len(np.unique(rows["lcp"])) < len(rows["lcp"])
    claims = instances_ref.explained_sets(rows["hit"], rows["counted"])
    prm = rows["prm"]
    return rows, pool("walk_pair_%d" % seed, 300, claims, score=rows["lcp"], max_selected=prm["max_instances"], min_pixels=prm["min_points"],
                      min_exclusive_fraction=prm["min_exclusive_fraction"], max_violation_fraction=1.0)


# ---- models, poses and frames of the footprint tests (hand-built frames: power-of-two intrinsics and depth scale) ----
EPS = float(2.0 ** -7)          # tolerance of the hand-built cases: a representable float
SCALE = float(2.0 ** -10)       # depth unit of the hand-built frames: raw 1024 is exactly 1 m
K64 = (32.0, 32.0, 32.0, 24.0)  # 64 x 48 camera
K_ROUGH = (60.0, 31.5, 60.0, 23.5)
PRM_ROUGH = dict(point_radius=0.01, max_splat_px=3, tolerance=0.05, class_threshold=0.15)


def pose(R=None, t=(0, 0, 0)):
    P = np.eye(4)
    if R is not None:
        P[:3, :3] = R
    P[:3, 3] = t
    return P.T.reshape(16).astype(F)


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def flat_frame(W, H, raw=1024):
    """a wall at raw depth units with a hole (no depth) at pixel (row 24, col 33), and a class image that is exactly at the 0.1 threshold at
    the centre pixel (raw 1000), just below it one column to the left (999), 1.0 elsewhere"""
    depth = np.full((H, W), raw, np.uint16)
    prob = np.full((H, W), 10000, np.uint16)
    depth[24, 33] = 0
    prob[24, 32] = 1000
    prob[24, 31] = 999
    return depth, prob


def seeded_model(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    pos = (u * np.array([0.06, 0.04, 0.03])).astype(F)
    nrm = (u / np.array([0.06, 0.04, 0.03])).astype(F)        # not unit: the context normalises
    return pos, nrm


def seeded_poses(n, seed, z=(0.3, 0.9), xy=0.25):
    rng = np.random.default_rng(seed)
    return np.stack([pose(rot(rng.normal(size=3), rng.uniform(0, 180)), (rng.uniform(-xy, xy), rng.uniform(-xy, xy), rng.uniform(*z))) for _ in range(n)])


def rough_frame(W, H, seed, raw=(3000, 9000)):
    rng = np.random.default_rng(seed)
    depth = rng.integers(raw[0], raw[1], (H, W)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.15] = 0
    prob = rng.integers(0, 3000, (H, W)).astype(np.uint16)
    return depth, prob


def chunk_case():
    """the n = 7 pool of the chunking test and its child process: a 257-point model, seven poses (one NaN, one all zero) on a 37 x 29 frame"""
    depth, prob = rough_frame(37, 29, 51)
    pos, nrm = seeded_model(257, 52)
    poses = seeded_poses(7, 53, xy=0.1)
    poses[2] = np.nan; poses[5] = 0
    return dict(pos=pos, nrm=nrm, depth=depth, prob=prob, K=(40.0, 18.0, 40.0, 14.0), scale=1e-4, poses=poses, prm=dict(PRM_ROUGH, max_splat_px=8))


def scene_of_two():
    """the end-to-end scene: a box face and a disc, side by side at different depths in a 64 x 48 frame whose depth is the restatement's own
    z of their true poses; the pool holds the true poses, a near duplicate of each, and the box laid over the disc's pixels (an impostor,
    standing in front of the disc's surface).  -> dict(models, true poses, pool per object, depth, prob per object)"""
    g = np.arange(-10, 11) / 10.0
    xx, yy = np.meshgrid(g, g)
    box = np.stack([0.2 * xx.ravel(), 0.2 * yy.ravel(), np.zeros(xx.size)], 1).astype(F)            # a 0.4 m square, 21 x 21 points
    keep = xx.ravel() ** 2 + yy.ravel() ** 2 <= 1.0
    disc = np.stack([0.18 * xx.ravel()[keep], 0.18 * yy.ravel()[keep], np.zeros(int(keep.sum()))], 1).astype(F)
    nb, nd = np.tile([0, 0, -1.0], (len(box), 1)).astype(F), np.tile([0, 0, -1.0], (len(disc), 1)).astype(F)
    true_box, true_disc = pose(t=(-0.45, 0.0, 1.0)), pose(t=(0.5, 0.0, 1.5))
    W, H, K = 64, 48, K64
    prm = dict(point_radius=float(2.0 ** -5), max_splat_px=2, tolerance=EPS, class_threshold=0.1)
    blank = np.zeros((H, W), np.uint16)
    _, _, zb = ref.footprints(true_box, box, nb, blank, None, K, SCALE, **prm)
    _, _, zd = ref.footprints(true_disc, disc, nd, blank, None, K, SCALE, **prm)
    z = np.minimum(zb[0], zd[0])
    zz = np.where(z == 0xFFFFFFFF, np.uint32(0), z).astype(np.uint32)
    depth = np.round(zz.view(F) / F(SCALE)).astype(np.uint16).reshape(H, W)                               # 1 m and 1.5 m are whole depth units; 0: no depth
    prob_box = np.where((zb[0] != 0xFFFFFFFF).reshape(H, W), 9000, 100).astype(np.uint16)
    prob_disc = np.where((zd[0] != 0xFFFFFFFF).reshape(H, W), 9000, 100).astype(np.uint16)
    near = lambda P, dx: (P + np.array([0] * 12 + [dx, 0, 0, 0], F)).astype(F)
    # the box: true, near duplicate, laid over the disc's pixels 0.5 m in front of its surface (free-space violation), and laid on the disc's surface
    pools = [np.stack([true_box, near(true_box, 1 / 64), pose(t=(0.3, 0.0, 1.0)), pose(t=(0.5, 0.0, 1.5))]),
             np.stack([near(true_disc, 1 / 64), true_disc])]                               # (the duplicate first: the order is by score, not by slot)
    return dict(models=[(box, nb), (disc, nd)], pools=pools, depth=depth, probs=[prob_box, prob_disc], K=K, scale=SCALE, prm=prm)
