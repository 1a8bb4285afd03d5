"""Seeded cases for stocs_segment_frame: a small synthetic frame builder (a support plane seen obliquely, slabs standing on it, depth holes, a
far wall) and the label frames built where the label kernel can go wrong.  Depths are uint16 millimetres (depth_scale 0.001)."""
import numpy as np

F = np.float32
SCALE = 0.001
TILE = (64, 16)          # stocs_segment_tile; test_segment_abi_cpu.py checks the library says the same


def camera(W, H):
    f = 1.1 * W
    return (f, (W - 1) / 2.0, f, (H - 1) / 2.0)


def table_frame(W=128, H=96, seed=0, tilt_deg=55.0, dist=0.9, boxes=((30, 40, 28, 24, 0.08), (80, 50, 30, 20, 0.12)), holes=0.02, wall_z=1.7, noise_mm=0.0):
    """A plane n.X + d = 0 seen obliquely (tilt_deg between the optical axis and the plane's normal), boxes = (col, row, w, h, height) image
    rectangles lifted `height` metres off the plane along their rays, a wall at wall_z where the plane lies farther, a share `holes` of
    zero-depth pixels.  Returns depth (uint16), K, the plane (n, d) in float64, and the masks dict(table, box (list), wall, hole)."""
    rng = np.random.default_rng(seed)
    K = camera(W, H)
    t = np.deg2rad(tilt_deg)
    n = np.array([0.0, -np.sin(t), -np.cos(t)])          # faces the camera: n . X + d = 0 with d > 0 for points in front
    d = dist * np.cos(t)
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    r = np.stack([(jj - K[1]) / K[0], (ii - K[3]) / K[2], np.ones((H, W))], axis=-1)
    nr = r @ n
    with np.errstate(all="ignore"):
        zt = np.where(nr < 0, -d / nr, np.inf)
    wall = zt > wall_z
    z = np.where(wall, wall_z, zt)
    box_masks = []
    for (c, rr, w, h, height) in boxes:
        m = np.zeros((H, W), bool); m[rr:rr + h, c:c + w] = True
        m &= ~wall
        z = np.where(m, zt * (1.0 - height / d), z)      # a point scaled by f along its ray stands d (1 - f) off the plane
        box_masks.append(m)
    z = z + rng.normal(0.0, 1.0, z.shape) * noise_mm * 1e-3
    hole = rng.random((H, W)) < holes
    depth = np.where(hole, 0, np.clip(np.rint(z / SCALE), 1, 65535)).astype(np.uint16)
    inbox = np.zeros((H, W), bool)
    for m in box_masks:
        inbox |= m
    return depth, K, (n, d), dict(table=~wall & ~inbox & ~hole, box=[m & ~hole for m in box_masks], wall=wall & ~hole, hole=hole)


# ---- label frames: no plane search (plane_hypotheses = 0), every non-zero pixel is foreground; near = 1000 mm
LABEL = dict(plane_hypotheses=0, jump_abs=0.005, jump_rel=0.0, max_depth=4.0)


def blank(W, H, raw=0):
    return np.full((H, W), raw, np.uint16)


def serpentine(W, H):
    """a one-pixel path through the whole frame: every second row is full, joined to the next at alternating ends"""
    d = blank(W, H)
    d[0::2, :] = 1000
    for k, i in enumerate(range(1, H, 2)):
        d[i, W - 1 if k % 2 == 0 else 0] = 1000
    return d


def checkerboard(W, H):
    """all valid, neighbours 300 mm apart: no joins, every pixel its own component"""
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    return np.where((ii + jj) % 2 == 0, 1000, 1300).astype(np.uint16)


def diagonal_pair(W, H):
    """two squares that touch at one corner only"""
    d = blank(W, H)
    a = min(W, H) // 2
    d[0:a, 0:a] = 1000
    d[a:2 * a, a:2 * a] = 1000
    return d


def blobs(W, H, seed):
    """random foreground with random depth steps: many components of every size, crossing every tile border"""
    rng = np.random.default_rng(seed)
    coarse = rng.random(((H + 3) // 4, (W + 3) // 4))
    fg = np.kron(coarse, np.ones((4, 4)))[:H, :W] < 0.6
    fg &= rng.random((H, W)) < 0.93
    level = np.kron(rng.integers(0, 3, ((H + 7) // 8, (W + 7) // 8)), np.ones((8, 8), np.int64))[:H, :W]
    return np.where(fg, 1000 + 20 * level + rng.integers(0, 3, (H, W)), 0).astype(np.uint16)


def two_sizes(W, H, n):
    """a component of exactly n pixels and one of n - 1, apart"""
    d = blank(W, H)
    assert n <= W * (H // 2) and n - 1 <= W * (H - H // 2 - 1)
    a = np.zeros(W * (H // 2), np.uint16); a[:n] = 1000
    d[:H // 2] = _snake(a, W)
    b = np.zeros(W * (H - H // 2 - 1), np.uint16); b[:n - 1] = 1000
    d[H // 2 + 1:] = _snake(b, W)
    return d


def _snake(flat, W):
    """lay a run of pixels out row by row, reversing every second row, so that the run stays 4-connected"""
    rows = flat.reshape(-1, W).copy()
    rows[1::2] = rows[1::2, ::-1]
    return rows


def jump_pair(W, H):
    """left half at 1000 mm, right half at 1010 mm: the step between them is the float |1.000 - 1.010|"""
    d = blank(W, H, 1000)
    d[:, W // 2:] = 1010
    step = abs(F(1000) * F(SCALE) - F(1010) * F(SCALE))
    return d, F(step)


def two_planes(W, H):
    """two fronto-parallel halves, 200 mm apart, the same number of lattice pixels on each: hypotheses on either tie"""
    d = blank(W, H, 1000)
    d[:, W // 2:] = 1200
    return d


def plane_bound(points64):
    """How far the plane fitted to coordinates rounded to 2^-16 m can lie from the plane of the points themselves.  Every coordinate moves by at
    most 2^-17, a point by eps = sqrt(3) 2^-17.  With X the centred points and S = X'X / N (eigenvalues l1 >= l2 >= l3), the rounded points
    give S + E with |E| <= 2 sqrt(l1) eps + eps^2 (Cauchy-Schwarz on X'D / N, D the displacements, centred).  Davis-Kahan (in the form of Yu,
    Wang and Samworth 2015) bounds the angle of the smallest eigenvector: sin(theta) <= 2 |E| / (l2 - l3).  The centroid moves by at most eps,
    so d = -n.c moves by at most theta |c| + eps.  Returns (theta, the bound on d, eps)."""
    eps = np.sqrt(3.0) * 2.0 ** -17
    c = points64.mean(axis=0)
    w = np.linalg.eigvalsh(np.cov((points64 - c).T, bias=True))          # ascending
    E = 2.0 * np.sqrt(w[2]) * eps + eps * eps
    theta = float(np.arcsin(min(1.0, 2.0 * E / (w[1] - w[0]))))
    return theta, theta * float(np.linalg.norm(c)) + eps, eps


SIZES = [(63, 15), (64, 16), (65, 17), (128, 16), (129, 33)]
