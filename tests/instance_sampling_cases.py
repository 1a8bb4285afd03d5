"""Case table, scene and edge-map builders of the instance-mode sampling edge tests (tests/test_instance_sampling_cases_cpu.py checks them
with the oracle alone, tests/test_instance_sampling_edges_gpu.py runs them on the device).  No GPU, no library call: numpy and
model_matching_amd.synth.

The sizes sit on both sides of every number at which instance_attempts_kernel (sample.hip) takes another trip count or another form:
63/64/65 (one wavefront), 1023/1025 (one workgroup), 4095..4097 (one trip of the 4 x 1024-point stages), 8193 (a third trip),
16000/16001 (working set in LDS -> device memory).  The maps put the disc's run count on both sides of 16384 (union-find parents in LDS ->
device memory), the scene on the image border, and the pixel distances on ties.  The form rule restated in expected_form() is the one
documented at stocs_last_sampling_form in include/stocs_hip.h."""
import functools

import numpy as np

import class_sampling_cases as cs

SIZES = (63, 64, 65, 1023, 1025, 4095, 4096, 4097, 8193, 16000, 16001)
SEED = 5
INST_LDS_POINTS, INST_MAX_NODES = 16000, 16384
LDS_PARENTS = 65552                    # a16(4 * (INST_MAX_NODES + 1))
NO_LDS, TIMING = "STOCS_INSTANCE_NO_LDS", "STOCS_DEBUG_TIMING"
FULL, SMALL = (480, 640), (64, 640)    # (H, W)
MAPS = ("box_and_lines", "dense_speckle", "no_edges", "lattice8", "top_left", "bottom_right", "rows64_16384", "rows64_16385")
EDGE_MAPS = ("lattice8", "top_left", "bottom_right", "rows64_16384", "rows64_16385")
EDGE_SIZES = (4097, 16000, 16001)
BATCH_SIZES = (4097, 16001)            # trial batches: working set in LDS and in device memory
BATCH_SEEDS = (9100, 9113, 9126)
BATCH_ATTEMPTS = 24
MANY_S, MANY_ATTEMPTS = 1025, 12       # the batch that takes two launches
N_POSES = 8

model, scene = cs.model, cs.scene


def image_size(kind):
    return SMALL if kind.startswith("rows64") else FULL


def count_runs(edge):
    """passable runs (maximal stretches of 255 inside a row) of the whole map"""
    p = (np.asarray(edge) == 255).astype(np.int8)
    return int(p[:, 0].sum() + (np.diff(p, axis=1) == 1).sum())


def _rows64_map(extra):
    """64 x 640, 255 passable / 128 neither.  Rows 0..62: the 5-pixel pattern 255 255 128 255 128 (two runs), shifted by row % 4 so that the
    runs of consecutive rows touch diagonally and the whole pattern is one component: 128 periods x 2 = 256 runs a row.  Row 63: single
    pixels at the even columns 0..508 (255 runs) and one run over columns 511..630, 256 as well: 64 x 256 = 16384 runs in all.  extra:
    (63, 635) passable too, a run of its own (columns 631..639 are otherwise 128)."""
    H, W = SMALL
    pat = np.array([255, 255, 128, 255, 128], np.uint8)
    edge = np.empty((H, W), np.uint8)
    for r in range(H - 1):
        edge[r] = pat[(np.arange(W) - r % 4) % 5]
    edge[H - 1] = 128
    edge[H - 1, 0:510:2] = 255
    edge[H - 1, 511:631] = 255
    if extra:
        edge[H - 1, 635] = 255
    return edge


@functools.lru_cache(maxsize=None)
def case_input(S, kind):
    """-> (edge map (H, W) uint8, pixel (S, 2) int32) of scene(S) under the map `kind`; positions, normals and prior are the scene's own"""
    sc = scene(S)
    H, W = image_size(kind)
    pix = sc.pixel.astype(np.int32).copy()
    if kind == "box_and_lines":                                    # the map of test_instance_mode_equals_oracle
        edge = np.full((H, W), 255, np.uint8)
        rows, cols = pix[:sc.n_object, 0], pix[:sc.n_object, 1]
        r0, r1, c0, c1 = max(rows.min() - 3, 0), min(rows.max() + 3, H - 1), max(cols.min() - 3, 0), min(cols.max() + 3, W - 1)
        edge[r0, c0:c1 + 1] = 0; edge[r1, c0:c1 + 1] = 0; edge[r0:r1 + 1, c0] = 0; edge[r0:r1 + 1, c1] = 0
        edge[::37, :] = 0
    elif kind == "dense_speckle":                                  # about 77 000 runs: any 110 rows hold more than INST_MAX_NODES
        edge = np.where(np.random.default_rng(20261018).random((H, W)) < 0.5, 255, 128).astype(np.uint8)
    elif kind == "no_edges":
        edge = np.full((H, W), 255, np.uint8)
    elif kind == "lattice8":                                       # equal pixel distances, perfect-square maxd2, many points per pixel
        edge = np.full((H, W), 255, np.uint8)
        pix = pix // 8 * 8
    elif kind in ("top_left", "bottom_right"):
        # every 37th row and 53rd column an edge, counted so that neither border row nor border column is one (36, 73, ...; 52, 105, ...):
        # a point on the border must be able to be a seed for the 3x3 neighbourhood to leave the image
        edge = np.full((H, W), 255, np.uint8)
        edge[36::37, :] = 0; edge[:, 52::53] = 0
        assert (H - 1 - 36) % 37 and (W - 1 - 52) % 53 and edge[0, 0] == edge[H - 1, W - 1] == 255
        pix = pix - pix.min(axis=0) if kind == "top_left" else pix + (np.array([H - 1, W - 1]) - pix.max(axis=0))
    elif kind in ("rows64_16384", "rows64_16385"):
        edge = _rows64_map(kind.endswith("5"))
        pix[:, 0] = pix[:, 0] * 64 // 480
    else:
        raise KeyError(kind)
    pix = np.ascontiguousarray(pix, np.int32)
    assert pix[:, 0].min() >= 0 and pix[:, 0].max() < H and pix[:, 1].min() >= 0 and pix[:, 1].max() < W
    edge.setflags(write=False); pix.setflags(write=False)
    return edge, pix


# ---- the case table: (id, S, map, (H, W), dispersion, calls [(first_attempt, n_attempts)], env) ----
def _n(S):
    return 254 if S <= 65 else 60     # the 63..65-point scenes hold a 16-point object of which few attempts find a base


def _case(S, kind, disp=0.9, calls=None, env=(), tag=""):
    calls = tuple(calls or [(0, _n(S))])
    name = "%d-%s%s%s%s" % (S, kind, "-no_lds" if NO_LDS in env else "", "-timing" if TIMING in env else "", tag)
    return (name, S, kind, image_size(kind), float(disp), calls, tuple(env))


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for S in SIZES:
        out.append(_case(S, "box_and_lines"))
        out.append(_case(S, "dense_speckle"))
        if S <= INST_LDS_POINTS:
            out.append(_case(S, "dense_speckle", env=(NO_LDS,)))
    for kind in EDGE_MAPS:
        for S in EDGE_SIZES:
            out.append(_case(S, kind))
        out.append(_case(4097, kind, env=(NO_LDS,)))
    for S in (4097, 16001):
        for disp in (0.0, 1.0):
            out.append(_case(S, "box_and_lines", disp=disp, tag="-disp%g" % disp))
    for env in ((), (NO_LDS,)):
        out.append(_case(4097, "box_and_lines", calls=[(0, 254)], env=env, tag="-single254"))
        out.append(_case(4097, "box_and_lines", calls=[(0, 100), (100, 154)], env=env, tag="-split254"))
    out.append(_case(4097, "dense_speckle", env=(TIMING,)))       # the stage clocks on, a disc of more than INST_MAX_NODES runs
    assert len({c[0] for c in out}) == len(out)
    return tuple(out)


def case_by_id(name):
    return next(c for c in cases() if c[0] == name)


def n_attempts(case):
    first, n = case[5][-1]
    assert case[5][0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(case[5], case[5][1:]))   # the calls follow one another from attempt 0
    return first + n


def reference_key(case):
    """cases with the same key have the same oracle results: the oracle knows neither the working-set form nor how the attempts are cut into calls"""
    return (case[1], case[2], case[4], n_attempts(case))


# ---- the form rule of include/stocs_hip.h (stocs_last_sampling_form, instance mode), restated ----
def expected_form(S, env=(), n_trials=None, n_cu=None):
    """-> dict(kernel, threads, lds_bytes, cap, launches, redone); n_trials: a trial batch on a device of n_cu compute units"""
    wlds = S <= INST_LDS_POINTS and NO_LDS not in set(env)
    launches = 1 if n_trials is None else -(-n_trials // max(1, n_cu // 2))
    return dict(kernel="instance_lds" if wlds else "instance_device_memory", threads=1024,
                lds_bytes=LDS_PARENTS + (cs.a16(4 * S) + 2 * S + 16 if wlds else 0), cap=0, launches=launches, redone=0)


def working_set_form(case):
    return expected_form(case[1], case[6])["kernel"]


# ---- the per-attempt records of stocs_last_instance_attempts: (survivors, point 1, reached its mask, nodes or -1) ----
PATHS = ("fill_parents_lds", "fill_parents_device_memory", "reused_mask", "failed_first_draw")


def path_of(rec):
    surv, p1, reached, nodes = (int(v) for v in rec)
    if not reached:
        assert p1 == -1 and nodes == 0 and surv == 0, rec
        return "failed_first_draw"
    assert p1 >= 0, rec
    if nodes == -1:
        return "reused_mask"
    assert nodes >= 0, rec
    return "fill_parents_lds" if nodes <= INST_MAX_NODES else "fill_parents_device_memory"


def path_counts(recs):
    out = dict.fromkeys(PATHS, 0)
    for r in recs:
        out[path_of(r)] += 1
    return out


# ---- the oracle's side of a case ----
def pruned_weights(edge, pix, prob):
    """the weights point 1 of an attempt is drawn from: the current prior with the points on edge pixels (png value 0) at zero"""
    w = np.asarray(prob, np.float32).copy()
    w[edge[pix[:, 0], pix[:, 1]] == 0] = 0.0
    return w


def make_oracle(oracle_lib, S, kind):
    """a fresh oracle on scene(S) under the map `kind`, with the map's image size"""
    sc, m = scene(S), model()
    H, W = image_size(kind)
    edge, pix = case_input(S, kind)
    orc = oracle_lib.Oracle(sc.pos, sc.nrm, sc.prob, pix, m.pos, m.nrm, params=oracle_lib.default_params(image_height=H, image_width=W))
    orc.set_edge_map(edge)
    return orc


def oracle_trial(oracle_lib, orc, S, kind, seed, n, disp, with_lcp=True):
    """Attempts 0 .. n - 1 of one trial on an oracle that is fresh, or restarted (Oracle.restart_trial) -> dict(valid, ids, inv per attempt;
    seg_sizes: `segment` after every attempt; failed_first: attempts whose first draw finds every weight zero; segment, prob after the last
    attempt; prob0: the prior; poses, lcp: N_POSES candidate poses and their oracle scores under the decayed prior)."""
    import ctypes as C
    from model_matching_amd import synth
    sc = scene(S)
    edge, pix = case_input(S, kind)
    L = oracle_lib.lib()
    valid, ids, inv, seg_sizes, failed_first = np.zeros(n, bool), np.zeros((n, 4), np.int32), np.zeros((n, 2), np.float32), [], []
    for a in range(n):
        valid[a], ids[a], inv[a] = orc.sample_instance_base(seed, a, disp, a + 1)
        # the prior changes only by the decay at the start of an attempt: what the oracle holds now is what this attempt's first draw saw
        w = pruned_weights(edge, pix, orc.scene_class_prob())
        if L.orc_draw(w.ctypes.data_as(C.POINTER(C.c_float)), S, L.orc_rng(seed, a, 0)) < 0:
            failed_first.append(a)
        seg_sizes.append(len(orc.get_segment()))
    out = dict(valid=valid, ids=ids, inv=inv, seg_sizes=np.array(seg_sizes), failed_first=failed_first, segment=orc.get_segment().copy(),
               prob=orc.scene_class_prob().copy(), prob0=sc.prob.astype(np.float32))
    if with_lcp:
        c_s, c_m = orc.centroids()
        out["poses"] = synth.make_candidates(synth.centred_gt(sc.T_gt, c_s.astype(np.float64), c_m.astype(np.float64)), N_POSES)
        out["lcp"] = orc.lcp_batch(out["poses"])
    return out


def run_oracle(oracle_lib, case, with_lcp=True):
    """one fresh oracle through the attempts of the case"""
    name, S, kind, size, disp, calls, env = case
    return oracle_trial(oracle_lib, make_oracle(oracle_lib, S, kind), S, kind, SEED, n_attempts(case), disp, with_lcp)
