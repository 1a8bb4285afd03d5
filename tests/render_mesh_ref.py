"""float32 numpy restatement of the contract written at stocs_render_poses_mesh in include/stocs_hip.h: the joint renderer and the scene
footprints on a triangle mesh.  Everything is defined through Z_h, the z-buffer of float bits mesh_ref.render_bits gives for pose h alone;
the key minimum, the classification (render_ref.classify), the labels (render_ref.labels) and the rows (scene_ref) are composed on top of
it and none of those files is changed.  Written from the contract, not from the kernels; the GPU tests compare the library's key buffers,
records, labels, states and rows with it for equality.  z_bits keeps what it rendered (read-only), so that the tests of one process
share one reference.  No GPU, numpy only.  Not a test module."""
import numpy as np

import mesh_ref
import render_ref as rref
import scene_ref as sref

F = np.float32
EMPTY = rref.EMPTY
EMPTY32 = np.uint32(0xFFFFFFFF)
DTYPE = rref.DTYPE
COUNTS = rref.COUNTS
records_equal = rref.records_equal
empty_keys = rref.empty_keys
labels = rref.labels
_cache = {}


def z_bits(pose16, verts, tris, K, W, H):
    """Z_h: (H * W) uint32 float bits of the mesh under this pose alone, empty = all ones (read-only, cached)"""
    P = np.ascontiguousarray(pose16, F).reshape(16)
    v = np.ascontiguousarray(verts, F)
    t = np.ascontiguousarray(tris, np.int32)
    key = (P.tobytes(), v.tobytes(), t.tobytes(), tuple(float(F(k)) for k in K), W, H)
    if key not in _cache:
        z = mesh_ref.render_bits(P, v, t, K, W, H)
        z.setflags(write=False)
        _cache[key] = z
    return _cache[key]


def render(zkey, poses16, verts, tris, K, W, H, id_base=0, clear=False):
    """stocs_render_poses_mesh on a flat uint64 key buffer of W*H (in place; returned)"""
    P = np.asarray(poses16, F).reshape(-1, 16)
    if clear and len(P):
        zkey[:] = EMPTY
    for h in range(len(P)):
        z = z_bits(P[h], verts, tris, K, W, H)
        on = z != EMPTY32
        key = (z[on].astype(np.uint64) << np.uint64(32)) | np.uint64(id_base + h)
        zkey[on] = np.minimum(zkey[on], key)
    return zkey


def resolve(zkey, poses16, verts, tris, depth_u16, prob_u16, K, depth_scale, id_base=0, **params):
    """stocs_render_resolve_mesh -> records of DTYPE"""
    H, W = depth_u16.shape
    P = np.asarray(poses16, F).reshape(-1, 16)
    state = rref.classify(zkey, depth_u16, prob_u16, depth_scale, **params)
    low = (zkey & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out = np.zeros(len(P), DTYPE)
    for h in range(len(P)):
        C = np.flatnonzero(z_bits(P[h], verts, tris, K, W, H) != EMPTY32)
        vis = (low[C] == id_base + h) & (zkey[C] != EMPTY)
        st = state[C][vis]
        out[h] = (len(C), int(vis.sum()), int((~vis).sum()), int(((st & 15) == 1).sum()), int(((st & 15) == 2).sum()), int(((st & 15) == 3).sum()),
                  int(((st & 15) == 4).sum()), int(((st & 16) != 0).sum()))
    return out


def explain(poses16, verts, tris, depth_u16, prob_u16, K, depth_scale, **params):
    """stocs_explain_poses_mesh -> (records, labels, state, key buffer)"""
    H, W = depth_u16.shape
    zkey = render(empty_keys(W, H), poses16, verts, tris, K, W, H, 0, True)
    rec = resolve(zkey, poses16, verts, tris, depth_u16, prob_u16, K, depth_scale, 0, **params)
    lab, st = labels(zkey, depth_u16, prob_u16, depth_scale, **params)
    return rec, lab, st, zkey


def footprints(poses16, verts, tris, depth_u16, prob_u16, K, depth_scale, claim="agree", **params):
    """stocs_scene_footprints_mesh -> (records (n,) scene_ref.RECORD_DTYPE, masks (n, npix) booleans of the claimed pixels)"""
    H, W = depth_u16.shape
    P = np.asarray(poses16, F).reshape(-1, 16)
    rec = np.zeros(len(P), sref.RECORD_DTYPE)
    masks = np.zeros((len(P), H * W), bool)
    for h in range(len(P)):
        zkey = render(empty_keys(W, H), P[h], verts, tris, K, W, H, 0, True)                # this pose alone
        st = rref.classify(zkey, depth_u16, prob_u16, depth_scale, **params)
        masks[h] = (st & 15) == 2 if sref.CLAIMS[claim] == 0 else (st & 16) != 0
        rec[h] = (int((zkey != EMPTY).sum()), int(((st & 15) == 1).sum()), int(((st & 15) == 2).sum()), int(((st & 15) == 3).sum()), int(((st & 15) == 4).sum()),
                  int(((st & 16) != 0).sum()), int(masks[h].sum()))
    return rec, masks
