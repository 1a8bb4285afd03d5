"""Seeded meshes for the mesh sampling tests (tests/test_mesh_sample_*): single triangles with a known count, runs of empty triangles,
counts and totals at the kernel's sizes (a wavefront's 64, a workgroup's 256), the box, the bowl and the Cm solid.  Everything is built
so that the intended counts are exact: with h = 2^-8 a right triangle of legs 2 n h and h has x = n, and one of legs h 2^-30 and h has
x = 2^-31, below every non-zero dither."""
import numpy as np

from model_matching_amd import synth
import mesh_sample_ref as ref

F = np.float32
H = 2.0 ** -8
SEED = 20240607
VOXELS = (0.005, 0.0075, 0.01)
BOX_SIZE = (0.10, 0.06, 0.04)


def right_triangle(legs, at):
    a, b = legs
    o = np.asarray(at, np.float64)
    return np.array([o, o + (a, 0, 0), o + (0, b, 0)], np.float64)


def mesh_of(tri_verts):
    """every triangle on three vertices of its own"""
    v = np.concatenate(tri_verts).astype(F)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def counted(ns, h=H):
    """a mesh whose triangle i has exactly ns[i] samples at spacing h whatever the seed (0: a live triangle too small for one)"""
    out = []
    for i, n in enumerate(ns):
        legs = (2 * n * h, h) if n else (h * 2.0 ** -30, h)
        out.append(right_triangle(legs, (0.0, 2 * h * i, 0.25 * (i % 3))))
    return mesh_of(out)


def below_one():
    """one triangle with x = 1 - 2^-6, and two seeds: the first gives it no sample, the second one"""
    v, t = mesh_of([right_triangle((2 * (1 - 2.0 ** -6) * H, H), (0, 0, 0))])
    d = np.array([ref.dither(s, 0)[0] for s in range(4096)])
    none, one = int(np.flatnonzero(d >= 1 - 2.0 ** -6)[0]), int(np.flatnonzero(d < 1 - 2.0 ** -6)[0])
    return v, t, none, one


def degenerate(kind):
    """live (3 samples), a triangle without area, live (2 samples)"""
    live0, live1 = right_triangle((6 * H, H), (0, 0, 0)), right_triangle((4 * H, H), (0, 4 * H, 0.5))
    o = np.array([0.125, 0.25, 0.5])
    if kind == "collinear":
        mid = np.array([o, o + (H, 2 * H, 0), o + (2 * H, 4 * H, 0)])
    elif kind == "repeated":
        mid = np.array([o, o, o + (H, 0, H)])
    else:   # "nan"
        mid = np.array([o, o + (np.nan, 0, 0), o + (0, H, 0)])
    return mesh_of([live0, mid, live1])


def random_small(nt, seed):
    """a strip of nt triangles with x around 1 at spacing H, on shared vertices (a random walk with steps of about H)"""
    rng = np.random.default_rng(seed)
    v = (0.25 + np.cumsum(rng.standard_normal((nt + 2, 3)) * (0.7 * H), axis=0)).astype(F)
    t = np.stack([np.arange(nt), np.arange(nt) + 1, np.arange(nt) + 2], axis=1).astype(np.int32)
    return v, t


def box():
    return synth.box_mesh(BOX_SIZE)


BOWL_CENTRE = np.array([0.0, 0.0, 0.1])


def bowl(r_out=0.060, r_in=0.055, n_lat=16, n_lon=32):
    """a two-walled open hemisphere (the lower half of a sphere about BOWL_CENTRE, 100 mm above the origin; a flat rim joins the walls)
    -> (vertices, triangles wound along the surface's true normal, wall (nt,): 0 outer, 1 inner, 2 rim)"""
    def wall(r):
        th = (np.arange(1, n_lat + 1) * (np.pi / 2) / n_lat)[:, None]
        ph = (np.arange(n_lon) * 2 * np.pi / n_lon)[None, :]
        ring = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th) * np.ones_like(ph)], axis=2).reshape(-1, 3)
        return np.concatenate([[[0.0, 0.0, -1.0]], ring]) * r + BOWL_CENTRE
    idx = lambda i, k: 1 + (i - 1) * n_lon + k % n_lon
    tw = [(0, idx(1, k), idx(1, k + 1)) for k in range(n_lon)]
    for i in range(1, n_lat):
        for k in range(n_lon):
            tw += [(idx(i, k), idx(i + 1, k), idx(i + 1, k + 1)), (idx(i, k), idx(i + 1, k + 1), idx(i, k + 1))]
    tw = np.asarray(tw, np.int64)
    nw = 1 + n_lat * n_lon
    rim = []
    for k in range(n_lon):
        o0, o1, i0, i1 = idx(n_lat, k), idx(n_lat, k + 1), nw + idx(n_lat, k), nw + idx(n_lat, k + 1)
        rim += [(o0, o1, i1), (o0, i1, i0)]
    verts = np.concatenate([wall(r_out), wall(r_in)]).astype(F)
    tris = np.concatenate([tw, tw + nw, np.asarray(rim, np.int64)])
    wall_id = np.concatenate([np.zeros(len(tw), int), np.ones(len(tw), int), np.full(len(rim), 2)])
    # wind every triangle along the true normal of its wall
    v = verts.astype(np.float64)
    A, B, C = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    n = np.cross(B - A, C - A)
    want = bowl_true_normal((A + B + C) / 3, wall_id)
    flip = (n * want).sum(axis=1) < 0
    tris[flip] = tris[flip][:, [0, 2, 1]]
    return verts, tris.astype(np.int32), wall_id


def bowl_true_normal(p, wall_id):
    r = p - BOWL_CENTRE
    r = r / np.linalg.norm(r, axis=1, keepdims=True)
    return np.where((wall_id == 0)[:, None], r, np.where((wall_id == 1)[:, None], -r, np.array([0.0, 0.0, 1.0])))


def ellipsoid(level):
    """icosphere(level) scaled to the Cm solid's ellipsoid, with the analytic normal as a function"""
    v, t = synth.icosphere(level)
    return (v * ELL_ABC).astype(F), t


ELL_ABC = np.array([0.08, 0.08, 0.03])


def ellipsoid_normal(p):
    n = np.asarray(p, np.float64) / ELL_ABC ** 2
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def gpu_cases():
    """name -> (verts, tris, spacing, seed): the meshes the GPU test compares bit for bit with the restatement"""
    out = {"integer_x": counted([8]) + (H, 1)}
    v, t = mesh_of([right_triangle((4 * H, 4 * H), (0, 0, 0))])
    out["legs_4h"] = (v, t, H, 2)
    v, t, none, one = below_one()
    out["below_one_none"] = (v, t, H, none)
    out["below_one_one"] = (v, t, H, one)
    for kind in ("collinear", "repeated"):
        out["degenerate_" + kind] = degenerate(kind) + (H, 3)
    out["empty_runs"] = counted([0, 0, 0, 5, 0, 0, 0, 0, 7, 3, 0, 0]) + (H, 4)
    out["empty_long_runs"] = counted([0] * 300 + [2] + [0] * 3000 + [300] + [0] * 270) + (H, 5)
    for n in (63, 64, 65, 255, 256, 257):
        out["count_%d" % n] = counted([3, n, 2]) + (H, 6)
        out["only_%d" % n] = counted([n]) + (H, 6)
    for n in (255, 256, 257):
        out["total_%d" % n] = counted([100, 0, n - 100]) + (H, 7)
        out["nt_%d" % n] = random_small(n, n) + (H, 8)
    out["total_0"] = counted([0, 0, 0]) + (H, 9)
    out["box_fine"] = box() + (0.0005, 10)
    out["level5_coarse"] = synth.make_model_mesh(5) + (0.005, 11)
    return out


# ---- the closed loop: mesh -> rendered frame -> scene, mesh -> model, trials, errors against the ground truth (needs a GPU)
LOOP_TRIALS = 16
LOOP_VOXEL = 0.005


def closed_loop(verts, tris, model=None, symmetries=None, seed0=100):
    """The mesh at synth.gt_pose() rendered by tests/mesh_ref.py into a depth frame in front of a wall at 1.5 m, the scene ingested from
    the frame, the model from preprocess_model_mesh (or `model` = (pos, nrm), to compare), LOOP_TRIALS seeded trials.  symmetries: a
    (K, 16) set for pose_errors_sym, None for pose_errors.  -> dict: the trials' ADD (symmetric ADD with a set) over the diameter, the
    index of the trial with the smallest one (`best`) and of the one with the highest score (`winner`), the VSD records of both poses
    on the mesh (BOP's taus), the model's size."""
    import mesh_ref
    import vsd_cases as vc
    from model_matching_amd.estimator import StocsEstimator, ingest_scene, preprocess_model_mesh
    W, Hh = 640, 480
    G = vc.pose16(synth.gt_pose())
    z = mesh_ref.render_depth(G, verts, tris, vc.YCB_K, W, Hh)[0]
    frame = vc.raw_from_depth(np.where(z > 0, z, 1.5))
    prob = np.where(z > 0, 10000, 0).astype(np.uint16)
    spos, snrm, sprob, spix = ingest_scene(frame, prob, vc.YCB_K, vc.DEPTH_SCALE, voxel_size=LOOP_VOXEL)
    mpos, mnrm = preprocess_model_mesh(verts, tris, LOOP_VOXEL, seed=SEED) if model is None else model
    est = StocsEstimator(spos, snrm, sprob, spix, mpos, mnrm, build_index=True)
    try:
        res = est.run_trials(np.arange(seed0, seed0 + LOOP_TRIALS, dtype=np.uint64), 100)
        P = np.stack([r["best_pose"] for r in res]).astype(F)
        lcp = np.array([r["best_lcp"] for r in res])
        dia = float(est.model_diameter())
        if symmetries is None:
            err = est.pose_errors(P, G)
        else:
            err = est.pose_errors_sym(P, G, symmetries)
        add = np.where(err["valid"] != 0, err["add"], np.inf) / dia
        best, winner = int(np.argmin(add)), int(np.argmax(lcp))
        est.set_frame(frame, None, vc.YCB_K, vc.DEPTH_SCALE)
        est.set_mesh(verts, tris)
        vsd, vsd_winner = est.pose_errors_vsd_mesh(P[[best, winner]], G)
    finally:
        est.close()
    return {"scene_points": len(spos), "model_points": len(mpos), "diameter": dia, "add_over_diameter": add, "lcp": lcp, "best": best, "winner": winner, "vsd": vsd,
            "vsd_winner": vsd_winner}
