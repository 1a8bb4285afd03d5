#!/usr/bin/env python3
"""Times of stocs_segment_frame on the GPU -> profiles/segment_time.json: per frame and label form (1: union-find in device memory, 2: tiles
in LDS) the host time of the whole call and, under STOCS_SEGMENT_CLOCK=1, the HIP-event times of the scoring group and of the label group,
each the median of REPS calls after WARM warm-up calls; beside them the numpy restatement's host time on the same frame, for scale.  Frames:
640 x 480 (a table scene, the three example frames of tests/golden, blobs, a checkerboard, one component) and the sizes the tests use.  The
default form (SEG_DEFAULT_FORM in csrc/segment.hip) is chosen on the 640 x 480 rows.

    python tools/segment_time.py [--out profiles/segment_time.json]

With --convex: the concavity cut (stocs_segment_frame_convex) on the same frames -> profiles/segment_convex_time.json.  Per frame, at the cut's
defaults and the default label form: the HIP-event time of the bend step under both bend forms (1: a lane per pixel, device memory; 2: tiles in
LDS) beside the label group's, the host time of the whole call with and without the cut, and, with --parent-lib PATH (a libstocs_hip.so built
from the parent commit), the plain and the convex call through that library in alternation with the same through this one, their HIP-event
group times beside them: A/B evidence that nothing existing moved.

    python tools/segment_time.py --convex [--parent-lib PATH] [--out profiles/segment_convex_time.json]

With --shapes: the shapes step (stocs_segment_shapes, and stocs_segment_assign with two objects) on the labels of the 640 x 480 frames, its
HIP-event time beside the label group's of the same frame -> profiles/segment_shapes_time.json; --parent-lib as above.

    python tools/segment_time.py --shapes [--parent-lib PATH] [--out profiles/segment_shapes_time.json]"""
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import segment_cases as sc  # noqa: E402
import segment_ref as sr  # noqa: E402
from model_matching_amd import estimator as E  # noqa: E402

WARM, REPS = 3, 20


def frames():
    out = []
    d, K, _, _ = sc.table_frame(W=640, H=480, seed=0, noise_mm=1.0, boxes=((150, 200, 140, 120, 0.08), (400, 250, 150, 100, 0.12)))
    out.append(("table 640x480", d, K, sc.SCALE, {}))
    for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "example_*_raw.npz"))):
        raw = np.load(f)
        out.append((os.path.basename(f)[len("example_"):-len("_raw.npz")] + " 640x480", raw["depth"].astype(np.uint16), [float(x) for x in raw["K"]], float(raw["depth_scale"]), {}))
    out.append(("blobs 640x480, no plane search", sc.blobs(640, 480, 0), sc.camera(640, 480), sc.SCALE, dict(sc.LABEL, min_pixels=20)))
    out.append(("checkerboard 640x480, no plane search", sc.checkerboard(640, 480), sc.camera(640, 480), sc.SCALE, dict(sc.LABEL, min_pixels=200)))
    out.append(("one component 640x480, no plane search", sc.blank(640, 480, 1000), sc.camera(640, 480), sc.SCALE, dict(sc.LABEL)))
    out.append(("serpentine 640x480, no plane search", sc.serpentine(640, 480), sc.camera(640, 480), sc.SCALE, dict(sc.LABEL)))
    d, K, _, _ = sc.table_frame(seed=1, noise_mm=1.5)
    out.append(("table 128x96", d, K, sc.SCALE, {}))
    out.append(("blobs 129x33, no plane search", sc.blobs(129, 33, 162), sc.camera(129, 33), sc.SCALE, dict(sc.LABEL, min_pixels=3)))
    return out


def timed(fn, clock):
    """medians over REPS calls after WARM: host ms of fn() and of each value clock() returns"""
    host, dev = [], []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        res = fn()
        dt = (time.perf_counter() - t0) * 1e3
        c = clock()
        if i >= WARM:
            host.append(dt); dev.append(c)
    return res, float(np.median(host)), float(np.min(host)), [float(x) for x in np.median(np.array(dev, np.float64).reshape(len(host), -1), axis=0)]


def plain_through(lib_path, frames_):
    """host ms (median, min) of the plain stocs_segment_frame per frame through another build of the library, then the same of
    stocs_segment_frame_convex at the default forms, then the medians of their HIP-event times ([score, label] and [bend, score, label]); in a
    child process so that the two libraries never share a process; prints one JSON list"""
    import subprocess
    code = ("import json, sys, time, numpy as np\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from model_matching_amd import capi\n"
            "capi.LIB_PATH = %r\n"
            "import ctypes\n"
            "capi.SIGNATURES = {k: v for k, v in capi.SIGNATURES.items() if hasattr(ctypes.CDLL(capi.LIB_PATH), k)}   # an older build lacks the newer entry points\n"
            "import tools.segment_time as st\n"
            "rows = []\n"
            "for name, d, K, scale, kw in st.frames():\n"
            "    _, med, mn, dev = st.timed(lambda: st.E.segment_frame(d, K, scale, **kw), st.E.segment_last_device_ms)\n"
            "    _, cmed, cmn, cdev = st.timed(lambda: st.E.segment_frame(d, K, scale, convex=True, **kw), lambda: (st.E.segment_last_bend_ms(),) + tuple(st.E.segment_last_device_ms()))\n"
            "    rows.append([name, med, mn, cmed, cmn, dev, cdev])\n"
            "print('ROWS ' + json.dumps(rows))\n") % (ROOT, os.path.join(ROOT, "tests"), lib_path)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return {row[0]: tuple(row[1:]) for row in json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")][0][5:])}


def main_convex():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "segment_convex_time.json")
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    os.environ["STOCS_SEGMENT_CLOCK"] = "1"
    os.environ.pop("STOCS_SEGMENT_FORM", None)
    fr = frames()
    this_lib = os.path.join(ROOT, "model_matching_amd", "libstocs_hip.so")
    order = ("this", "parent", "this", "parent", "parent", "this")
    aa = [plain_through(parent if w == "parent" else this_lib, fr) for w in order] if parent else None
    rows = []
    for name, d, K, scale, kw in fr:
        res0, plain_med, plain_min, (score0, label0) = timed(lambda: E.segment_frame(d, K, scale, **kw)[0], E.segment_last_device_ms)
        row = {"frame": name, "plain": {"call_host_ms_median": plain_med, "call_host_ms_min": plain_min, "label_device_ms_median": label0, "n_segments": res0["n_segments"]}}
        for form in ("1", "2"):
            os.environ["STOCS_SEGMENT_BEND_FORM"] = form
            res, med, mn, (bend, label) = timed(lambda: E.segment_frame(d, K, scale, convex=True, **kw)[0], lambda: (E.segment_last_bend_ms(), E.segment_last_device_ms()[1]))
            row["bend_form_%s" % form] = {"call_host_ms_median": med, "call_host_ms_min": mn, "bend_device_ms_median": bend, "label_device_ms_median": label,
                                           "n_segments": res["n_segments"], "n_cut": res["n_cut"], "n_tested": res["n_tested_h"] + res["n_tested_v"]}
        del os.environ["STOCS_SEGMENT_BEND_FORM"]
        assert row["bend_form_1"]["n_cut"] == row["bend_form_2"]["n_cut"] and row["bend_form_1"]["n_segments"] == row["bend_form_2"]["n_segments"], name
        row["faster_bend_form"] = 1 if row["bend_form_1"]["bend_device_ms_median"] < row["bend_form_2"]["bend_device_ms_median"] else 2
        if aa:
            row["plain_call_host_ms_median_aa"] = [[w, a[name][0]] for w, a in zip(order, aa)]
            row["convex_call_host_ms_median_aa"] = [[w, a[name][2]] for w, a in zip(order, aa)]
            row["device_ms_median_aa"] = [[w, a[name][4], a[name][5]] for w, a in zip(order, aa)]     # plain [score, label], convex [bend, score, label]
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"what": "stocs_segment_frame_convex on an MI355X at the cut's defaults (radius 4, smoothing 2, 25 degrees) and the default label form: HIP-event time of the bend "
                   "step per bend form beside the label group's, host time of the whole call (through the Python wrapper) with and without the cut; medians of %d calls "
                   "after %d.  plain_call_host_ms_median_aa, convex_call_host_ms_median_aa: the plain and the convex call through a library built from the parent "
                   "commit and through this one, each run in a process of its own, in the order listed" % (REPS, WARM),
           "default_bend_form": 1, "rows": rows, "unmeasured": "frame sizes other than those listed; real frames beyond the three examples; radii and smoothing off the defaults"}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main_shapes():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "segment_shapes_time.json")
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    os.environ["STOCS_SEGMENT_CLOCK"] = "1"
    os.environ.pop("STOCS_SEGMENT_FORM", None)
    fr = [f for f in frames() if "640x480" in f[0]]
    this_lib = os.path.join(ROOT, "model_matching_amd", "libstocs_hip.so")
    order = ("this", "parent", "this", "parent", "parent", "this")
    aa = [plain_through(parent if w == "parent" else this_lib, fr) for w in order] if parent else None
    objects = np.zeros(2, E.capi.OBJECT_DTYPE)
    objects["diameter"] = (0.12, 0.25); objects["extent"] = ((0.10, 0.06, 0.04), (0.16, 0.16, 0.06))
    rows = []
    for name, d, K, scale, kw in fr:
        (res, _, img), seg_med, _, (score, label) = timed(lambda: E.segment_frame(d, K, scale, **kw), E.segment_last_device_ms)
        lab, n = img["labels"], res["n_segments"]
        (_, counts), sh_med, sh_min, (sh_dev,) = timed(lambda: E.segment_shapes(d, lab, K, scale, n_labels=n, max_depth=kw.get("max_depth", 2.0)), lambda: (E.segment_shapes_last_device_ms(),))
        out4, as_med, as_min, (as_dev,) = timed(lambda: E.segment_assign(d, lab, K, scale, objects, n_labels=n, max_depth=kw.get("max_depth", 2.0)), lambda: (E.segment_shapes_last_device_ms(),))
        row = {"frame": name, "n_segments": n, "n_used": counts["n_used"], "segment_frame": {"call_host_ms_median": seg_med, "score_device_ms_median": score, "label_device_ms_median": label},
               "segment_shapes": {"call_host_ms_median": sh_med, "call_host_ms_min": sh_min, "device_ms_median": sh_dev},
               "segment_assign_2_objects": {"call_host_ms_median": as_med, "call_host_ms_min": as_min, "device_ms_median": as_dev, "compatible": (out4[1] == 0).sum(axis=1).tolist()}}
        if aa:
            row["plain_call_host_ms_median_aa"] = [[w, a[name][0]] for w, a in zip(order, aa)]
            row["plain_device_ms_median_aa"] = [[w, a[name][4]] for w, a in zip(order, aa)]      # [score, label]
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"what": "stocs_segment_shapes and stocs_segment_assign (two objects) on an MI355X on the labels of stocs_segment_frame, 640 x 480 frames: HIP-event time of every "
                   "kernel of the call (moments, shape, extents, finish; gate and stack with objects) beside the label group's of the same frame, host time of the whole call "
                   "through the Python wrapper; medians of %d calls after %d.  plain_call_host_ms_median_aa: the plain stocs_segment_frame through a library built from the "
                   "parent commit and through this one, each in a process of its own, in the order listed" % (REPS, WARM),
           "rows": rows, "unmeasured": "frame sizes other than 640 x 480; real frames beyond the three examples; more than two objects; labels not made by stocs_segment_frame"}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    if "--shapes" in sys.argv:
        return main_shapes()
    if "--convex" in sys.argv:
        return main_convex()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "segment_time.json")
    os.environ["STOCS_SEGMENT_CLOCK"] = "1"
    rows = []
    for name, d, K, scale, kw in frames():
        t0 = time.perf_counter()
        ref = sr.segment_frame(d, K, scale, **kw)
        row = {"frame": name, "restatement_host_ms": (time.perf_counter() - t0) * 1e3, "n_valid": ref["n_valid"], "plane_found": ref["plane_found"],
               "n_components": ref["n_components"], "n_segments": ref["n_segments"]}
        for form in ("1", "2"):
            os.environ["STOCS_SEGMENT_FORM"] = form
            call, score, label = [], [], []
            for i in range(WARM + REPS):
                t0 = time.perf_counter()
                res, _, _ = E.segment_frame(d, K, scale, **kw)
                dt = (time.perf_counter() - t0) * 1e3
                s, l = E.segment_last_device_ms()
                if i >= WARM:
                    call.append(dt); score.append(s); label.append(l)
            assert res["n_components"] == ref["n_components"] and res["n_segments"] == ref["n_segments"], (name, form)
            row["form_%s" % form] = {"call_host_ms_median": float(np.median(call)), "call_host_ms_min": float(np.min(call)), "score_device_ms_median": float(np.median(score)),
                                     "label_device_ms_median": float(np.median(label)), "label_device_ms_min": float(np.min(label)), "label_device_ms_max": float(np.max(label))}
        row["faster_label_form"] = 1 if row["form_1"]["label_device_ms_median"] < row["form_2"]["label_device_ms_median"] else 2
        rows.append(row)
        print(json.dumps(row), flush=True)
    del os.environ["STOCS_SEGMENT_FORM"]
    out = {"what": "stocs_segment_frame on an MI355X: host time of the whole call (through the Python wrapper, which allocates the output arrays), HIP-event time of the "
                   "scoring group (hypotheses, scoring, winner) and of the label group (union or tiles + borders, flatten), per label form; medians of %d calls after %d; "
                   "the numpy restatement's host time beside them for scale" % (REPS, WARM),
           "default_form": 2, "rows": rows,
           "unmeasured": "frame sizes other than those listed; real frames beyond the three examples"}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
