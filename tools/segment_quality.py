#!/usr/bin/env python3
"""What the depth-only segmentation finds on the three example frames of tests/golden (needs the GPU) -> profiles/segment_quality.json.  Per
frame, at the library's defaults: the plane found and the pixel classes; the overlap of the kept segments with the object pixels of the shipped
class image (class probability above 0.10): the share of the object's pixels inside a kept segment (coverage), the share of the kept pixels
that are object pixels (purity), and the same two figures for the one segment that holds most object pixels.  Recorded, not asserted: the
example class images come from a network and mark one object each, the segmentation marks everything that stands on the plane.

    python tools/segment_quality.py [--out profiles/segment_quality.json]

With --convex: the same figures with and without the concavity cut at its defaults (stocs_segment_frame_convex), and the share of the
foreground the cut takes -> profiles/segment_convex_quality.json.  Recorded, not asserted; no default is retuned from three frames.

    python tools/segment_quality.py --convex [--out profiles/segment_convex_quality.json]"""
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from model_matching_amd import estimator as E  # noqa: E402


def overlap(lab, records, obj):
    """coverage and purity of the kept segments against the object pixels, and of the one segment that holds most of them"""
    kept = lab > 0
    row = {"kept_pixels": int(kept.sum()), "coverage": float((kept & obj).sum() / max(int(obj.sum()), 1)), "purity": float((kept & obj).sum() / max(int(kept.sum()), 1))}
    ids, cnt = np.unique(lab[kept & obj], return_counts=True)
    if ids.size:
        k = int(ids[np.argmax(cnt)])
        row["best_segment"] = {"label": k, "pixels": int((lab == k).sum()), "coverage": float(cnt.max() / max(int(obj.sum()), 1)),
                               "purity": float(cnt.max() / int((lab == k).sum())), "zmin": float(records["zmin"][k - 1]), "zmax": float(records["zmax"][k - 1])}
    return row


def main_convex():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "segment_convex_quality.json")
    rows = []
    for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "example_*_raw.npz"))):
        raw = np.load(f)
        depth, K, scale = raw["depth"].astype(np.uint16), [float(x) for x in raw["K"]], float(raw["depth_scale"])
        obj = raw["prob"].astype(np.float32) * np.float32(1.0 / 10000) > np.float32(0.10)
        res0, rec0, img0 = E.segment_frame(depth, K, scale)
        res1, rec1, img1 = E.segment_frame(depth, K, scale, convex=True, images=("labels", "cut"))
        fg = int(np.isfinite(E.segment_frame(depth, K, scale, convex=True, images=("smoothed",))[2]["smoothed"]).sum())
        row = {"frame": os.path.basename(f)[len("example_"):-len("_raw.npz")], "pixels": int(depth.size), "object_pixels": int(obj.sum()), "foreground_pixels": fg,
               "plain": dict(overlap(img0["labels"], rec0, obj), n_components=int(res0["n_components"]), n_segments=int(res0["n_segments"])),
               "convex": dict(overlap(img1["labels"], rec1, obj), n_components=int(res1["n_components"]), n_segments=int(res1["n_segments"]),
                              **{k: int(res1[k]) for k in ("n_tested_h", "n_tested_v", "n_cut_h", "n_cut_v", "n_cut")}),
               "foreground_share_cut": float(res1["n_cut"] / max(fg, 1)), "object_pixels_cut": int(((img1["cut"] != 0) & obj).sum())}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"what": "stocs_segment_frame and stocs_segment_frame_convex (radius 4, smoothing 2, 25 degrees) at the library's defaults on the example frames of tests/golden, on "
                   "an MI355X: the overlap of the kept segments with the shipped class image's object pixels (class probability above 0.10) with and without the cut, and "
                   "the share of the foreground the cut takes; recorded, not asserted",
           "defaults_retuned_from_these": "none", "rows": rows, "unmeasured": "real frames beyond these three"}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    if "--convex" in sys.argv:
        return main_convex()
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
