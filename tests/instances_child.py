"""Child process of tests/test_instances_gpu.py: STOCS_INSTANCES_CHUNK is read from the environment, so the parent sets it for this
process alone.  Runs stocs_select_instances on the planted frame of tests/instances_cases.py and saves the result.  Not a test module.

    instances_child.py <out.npz>    -> T (n, 16), rec (n, 4) as raw 32-bit words, sel
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("STOCS_PIN_BLAS", "1")

import numpy as np  # noqa: E402

import instances_cases as cases  # noqa: E402


def main(path_out):
    from model_matching_amd.estimator import StocsEstimator
    fr = cases.planted_frame()
    m = fr["model"]
    est = StocsEstimator(fr["scene_pos"], fr["scene_nrm"], fr["scene_prob"], fr["scene_pixel"], m.pos, m.nrm, build_index=False)
    try:
        T = cases.planted_hypotheses(fr, est.get_scene_centroid(), est.get_model_centroid())
        rec, sel = est.select_instances(T)
    finally:
        est.close()
    np.savez(path_out, T=T, rec=rec.view(np.uint32).reshape(-1, 4), sel=sel)


if __name__ == "__main__":
    main(sys.argv[1])
