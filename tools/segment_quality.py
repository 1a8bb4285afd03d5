#!/usr/bin/env python3
"""What the depth-only segmentation finds on the three example frames of tests/golden (needs the GPU) -> profiles/segment_quality.json.  Per
frame, at the library's defaults: the plane found and the pixel classes; the overlap of the kept segments with the object pixels of the shipped
class image (class probability above 0.10): the share of the object's pixels inside a kept segment (coverage), the share of the kept pixels
that are object pixels (purity), and the same two figures for the one segment that holds most object pixels.  Recorded, not asserted: the
example class images come from a network and mark one object each, the segmentation marks everything that stands on the plane.

    python tools/segment_quality.py [--out profiles/segment_quality.json]"""
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from model_matching_amd import estimator as E  # noqa: E402


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "segment_quality.json")
    rows = []
    for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "example_*_raw.npz"))):
        raw = np.load(f)
        depth, K, scale = raw["depth"].astype(np.uint16), [float(x) for x in raw["K"]], float(raw["depth_scale"])
        obj = raw["prob"].astype(np.float32) * np.float32(1.0 / 10000) > np.float32(0.10)
        res, records, img = E.segment_frame(depth, K, scale)
        lab = img["labels"]
        kept = lab > 0
        row = {"frame": os.path.basename(f)[len("example_"):-len("_raw.npz")], "pixels": int(depth.size), "object_pixels": int(obj.sum()),
               "result": {k: (v.tolist() if k == "plane" else int(v)) for k, v in res.items()}, "kept_pixels": int(kept.sum()),
               "coverage": float((kept & obj).sum() / max(int(obj.sum()), 1)), "purity": float((kept & obj).sum() / max(int(kept.sum()), 1))}
        ids, cnt = np.unique(lab[kept & obj], return_counts=True)
        if ids.size:
            k = int(ids[np.argmax(cnt)])
            row["best_segment"] = {"label": k, "pixels": int((lab == k).sum()), "coverage": float(cnt.max() / max(int(obj.sum()), 1)),
                                   "purity": float(cnt.max() / int((lab == k).sum())), "zmin": float(records["zmin"][k - 1]), "zmax": float(records["zmax"][k - 1])}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"what": "stocs_segment_frame at the library's defaults on the example frames of tests/golden, on an MI355X: the plane, the pixel classes, and the overlap of the "
                   "kept segments with the shipped class image's object pixels (class probability above 0.10); recorded, not asserted",
           "defaults_retuned_from_these": "none", "rows": rows, "unmeasured": "real frames beyond these three"}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
