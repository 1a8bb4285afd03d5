#!/usr/bin/env python3
"""Surface quality of the triangle rasteriser's contract on synth:Cm, by the float32 numpy restatement alone (tests/mesh_ref.py; no GPU):
synth.make_model_mesh(level) at synth.gt_pose() through the 640 x 480 YCB camera against the float64 ray-cast of the solid
(tests/vsd_cases.py::cm_analytic_depth).  Prints the rows of profiles/mesh.md.

    python tools/mesh_quality.py [levels ...]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_ref as ref  # noqa: E402
import vsd_cases as vc  # noqa: E402
from model_matching_amd import synth  # noqa: E402


def erode4(mask):
    m = mask.copy()
    m[1:, :] &= mask[:-1, :]; m[:-1, :] &= mask[1:, :]; m[:, 1:] &= mask[:, :-1]; m[:, :-1] &= mask[:, 1:]
    m[0, :] = m[-1, :] = False; m[:, 0] = m[:, -1] = False
    return m


def main():
    levels = [int(x) for x in sys.argv[1:]] or [3, 4, 5]
    W, H = 640, 480
    T = synth.gt_pose()
    za = vc.cm_analytic_depth(T, vc.cm_ellipsoid_centre(synth.make_model(5000).pos), vc.YCB_K, W, H)
    sil = za > 0
    print("analytic silhouette: %d pixels" % sil.sum())
    print("| level | triangles | empty inside the eroded silhouette | empty inside the silhouette | hit outside it | depth error median / p99 / max (mm) |")
    print("|---|---|---|---|---|---|")
    for lv in levels:
        v, t = synth.make_model_mesh(lv)
        z = ref.bits_to_depth(ref.render_bits(vc.pose16(T), v, t, vc.YCB_K, W, H), W, H)
        both = sil & (z > 0)
        e = np.abs(z[both].astype(np.float64) - za[both]) * 1e3
        print("| %d | %d | %d | %d | %d | %.3f / %.3f / %.3f |" % (lv, len(t), (erode4(sil) & (z == 0)).sum(), (sil & (z == 0)).sum(), ((z > 0) & ~sil).sum(),
                                                               np.median(e), np.percentile(e, 99), e.max()))


if __name__ == "__main__":
    main()
