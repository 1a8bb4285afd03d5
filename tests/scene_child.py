"""Child process of tests/test_scene_gpu.py: STOCS_SCENE_CHUNK is read from the environment, so the parent sets it for this process
alone.  Runs stocs_scene_footprints on the n = 7 pool of tests/scene_cases.py (chunk_case) and saves the rows and the records.  Not a
test module.

    scene_child.py <out.npz> <claim>    -> rows (7, Wr) uint32, rec (7, 7) int32
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("STOCS_PIN_BLAS", "1")

import numpy as np  # noqa: E402

import scene_cases as cases  # noqa: E402


def run(est, c, claim, poses=None, slot_base=0, n_slots=None):
    """-> (the whole pool as (n_slots, Wr) uint32, pre-filled with ones; records)"""
    from model_matching_amd.estimator import scene_row_words
    poses = c["poses"] if poses is None else poses
    n_slots = len(poses) if n_slots is None else n_slots
    Wr = scene_row_words(c["depth"].shape)
    pool = np.full((n_slots, Wr), 0xFFFFFFFF, np.uint32)
    d = est.dev_alloc(pool.nbytes)
    try:
        est.dev_upload(d, pool)
        rec = est.scene_footprints(poses, d, slot_base, n_slots, claim, **c["prm"])
        est.dev_download(d, pool)
    finally:
        est.dev_free(d)
    return pool, rec


def make_est(c):
    from model_matching_amd.estimator import StocsEstimator
    rng = np.random.default_rng(1)
    sp = rng.normal(0, 0.05, (32, 3)).astype(np.float32)
    sn = sp / np.linalg.norm(sp, axis=1, keepdims=True)
    est = StocsEstimator(sp, sn, np.ones(32, np.float32), None, c["pos"], c["nrm"], build_index=False)
    est.set_frame(c["depth"], c["prob"], c["K"], c["scale"])
    return est


def main(path_out, claim):
    c = cases.chunk_case()
    est = make_est(c)
    try:
        rows, rec = run(est, c, claim)
    finally:
        est.close()
    np.savez(path_out, rows=rows, rec=rec.view(np.int32).reshape(-1, 7))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
