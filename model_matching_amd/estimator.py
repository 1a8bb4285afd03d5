"""Python mirror of the reference's ``stocs::stocs_estimator`` (reference include/stocs.hpp:16-180)
over the C ABI of libstocs_hip.so.  Same method names and argument meaning as the reference class
(flat clouds instead of PLY/PNG paths); every method forwards to the HIP library -- nothing is
computed in Python."""
from __future__ import annotations

import atexit
import ctypes as C
import math
import weakref

import numpy as np

from . import capi

# contexts still open when the interpreter exits are destroyed before module teardown, i.e. while the HIP runtime
# (possibly shared with PyTorch) is still up; a __del__ that runs after the runtime's own shutdown would free twice
_LIVE = weakref.WeakSet()


@atexit.register
def _close_all():
    for est in list(_LIVE):
        try:
            est.close()
        except Exception:
            pass


# stocs_trial_result as a numpy record (same layout as capi.TrialResult: 4 + 4 + 8 + 4 + 4 + 64 bytes)
_TRIAL_DTYPE = np.dtype([("n_bases", np.int32), ("n_candidates", np.int32), ("n_quads", np.int64), ("best_lcp", np.float32), ("best_index", np.int32),
                         ("best_pose16", np.float32, (16,))])
assert _TRIAL_DTYPE.itemsize == C.sizeof(capi.TrialResult)
_HYP_DTYPE = np.dtype([("candidate_index", np.int32), ("base_index", np.int32), ("lcp", np.float32), ("pose16", np.float32, 16),
                       ("refined_lcp", np.float32), ("refined_pose16", np.float32, 16), ("n_correspondences", np.int32), ("iterations", np.int32)])
assert _HYP_DTYPE.itemsize == C.sizeof(capi.TrialHypothesis)
_TRACK_DTYPE = np.dtype([("prior_lcp", np.float32), ("lcp", np.float32), ("pose16", np.float32, 16), ("refined_lcp", np.float32), ("refined_pose16", np.float32, 16),
                         ("n_correspondences", np.int32), ("iterations", np.int32)])
assert _TRACK_DTYPE.itemsize == C.sizeof(capi.TrackResult)
_DEPTH_DTYPE = np.dtype([("facing", np.int32), ("in_image", np.int32), ("self_occluded", np.int32), ("no_depth", np.int32), ("agree", np.int32),
                         ("in_front", np.int32), ("behind", np.int32), ("on_mask", np.int32), ("score", np.float32), ("violation", np.float32)])
assert _DEPTH_DTYPE.itemsize == C.sizeof(capi.DepthResult)
_POSE_ERROR_DTYPE = np.dtype([("add_fix", np.uint64), ("adds_fix", np.uint64), ("add", np.float32), ("add_max", np.float32), ("adds", np.float32),
                              ("adds_max", np.float32), ("valid", np.int32), ("reserved", np.int32)])
assert _POSE_ERROR_DTYPE.itemsize == C.sizeof(capi.PoseError)
_POSE_ERROR_SYM_DTYPE = np.dtype([("add_fix", np.uint64), ("add", np.float32), ("mssd", np.float32), ("mspd", np.float32), ("reserved_f", np.float32),
                                  ("k_add", np.int32), ("k_mssd", np.int32), ("k_mspd", np.int32), ("valid", np.int32)])
assert _POSE_ERROR_SYM_DTYPE.itemsize == C.sizeof(capi.PoseErrorSym)
_VSD_DTYPE = np.dtype([("px_est", np.int32), ("px_gt", np.int32), ("vis_est", np.int32), ("vis_gt", np.int32), ("inter", np.int32), ("uni", np.int32),
                       ("far", np.int32, (16,)), ("e", np.float32, (16,)), ("valid", np.int32), ("reserved", np.int32)])
assert _VSD_DTYPE.itemsize == C.sizeof(capi.VsdRecord)
_SYMMETRY_ERROR_DTYPE = np.dtype([("sum_fix", np.uint64), ("mean", np.float32), ("max", np.float32), ("n_far", np.int32), ("n_normal_bad", np.int32),
                                  ("valid", np.int32), ("reserved", np.int32)])
assert _SYMMETRY_ERROR_DTYPE.itemsize == C.sizeof(capi.SymmetryError)
_SYMMETRY_AXIS_DTYPE = np.dtype([("axis", np.float32, (3,)), ("order", np.int32), ("max", np.float32), ("mean", np.float32), ("n_normal_bad", np.int32),
                                 ("reserved", np.int32)])
assert _SYMMETRY_AXIS_DTYPE.itemsize == C.sizeof(capi.SymmetryAxis)
_RENDER_DTYPE = np.dtype([(f[0], np.int32) for f in capi.RenderResult._fields_])
assert _RENDER_DTYPE.itemsize == C.sizeof(capi.RenderResult)
_INSTANCE_DTYPE = np.dtype([("rank", np.int32), ("own", np.int32), ("exclusive", np.int32), ("lcp", np.float32)])
assert _INSTANCE_DTYPE.itemsize == C.sizeof(capi.InstanceResult)
_REFINE_VISIBLE_DTYPE = np.dtype([(f[0], np.float32 if f[0] == "rms" else np.int32) for f in capi.RefineVisibleResult._fields_])
assert _REFINE_VISIBLE_DTYPE.itemsize == C.sizeof(capi.RefineVisibleResult)
_REFINE_VISIBLE_DAMPED_DTYPE = np.dtype(_REFINE_VISIBLE_DTYPE.descr + [("evaluations", np.int32), ("rejected", np.int32), ("cost", np.float32), ("lambda", np.float32)])
assert _REFINE_VISIBLE_DAMPED_DTYPE.itemsize == C.sizeof(capi.RefineVisibleDampedResult)
_REFINE_VISIBLE_CONTOUR_DTYPE = np.dtype(_REFINE_VISIBLE_DAMPED_DTYPE.descr + [(k, np.int32) for k in ("object_px", "uncovered", "unreached", "beyond", "pulled")] +
                                         [("pull_rms", np.float32)])
assert _REFINE_VISIBLE_CONTOUR_DTYPE.itemsize == C.sizeof(capi.RefineVisibleContourResult)
_REFINE_VISIBLE_TRACE_DTYPE = np.dtype([("pose", np.float32, 16), ("cost", np.float64), ("lambda", np.float64), ("accepted", np.int32), ("state", np.int32)])
assert _REFINE_VISIBLE_TRACE_DTYPE.itemsize == C.sizeof(capi.RefineVisibleTrace)
# the forms of the visible-surface refinement by the suffix of their entry points: parameter struct, record struct, record dtype
_REFINE_VISIBLE_FORMS = {"": (capi.RefineVisibleParams, capi.RefineVisibleResult, _REFINE_VISIBLE_DTYPE),
                         "_damped": (capi.RefineVisibleDampedParams, capi.RefineVisibleDampedResult, _REFINE_VISIBLE_DAMPED_DTYPE),
                         "_contour": (capi.RefineVisibleContourParams, capi.RefineVisibleContourResult, _REFINE_VISIBLE_CONTOUR_DTYPE)}
_SCENE_RECORD_DTYPE = np.dtype([(f[0], np.int32) for f in capi.SceneRecord._fields_])
assert _SCENE_RECORD_DTYPE.itemsize == C.sizeof(capi.SceneRecord)
_SCENE_RESULT_DTYPE = np.dtype([(f[0], np.int32) for f in capi.SceneResult._fields_])
assert _SCENE_RESULT_DTYPE.itemsize == C.sizeof(capi.SceneResult)
SCENE_CLAIMS = {"agree": 0, "on_mask": 1}

# defaults of track_poses (tools/track_time.py's sweep, profiles/track_time.json)
TRACK_DEFAULTS = dict(rounds=6, samples=2048, max_translation=0.02, max_rotation_deg=10.0, shrink=0.7, seed=0, refine_iterations=0,
                      max_correspondence_distance=0.035)


class StocsEstimator:
    def __init__(self, scene_pos, scene_nrm, scene_prob, scene_pixel, model_pos, model_nrm,
                 params: capi.Params | None = None, build_index: bool = True, device: int = -1):
        self.L = capi.load()
        self.prm = params or capi.default_params()
        self._sp, psp = capi.f32(scene_pos)
        self._sn, psn = capi.f32(scene_nrm)
        self._spr, pspr = capi.f32(scene_prob)
        ppx = None
        if scene_pixel is not None:
            self._spx, ppx = capi.i32(scene_pixel)
        self._mp, pmp = capi.f32(model_pos)
        self._mn, pmn = capi.f32(model_nrm)
        self.nS, self.nM = len(self._sp), len(self._mp)
        self.h = C.c_void_p()
        capi.check(self.L.stocs_ctx_create(C.byref(self.prm), psp, psn, pspr, ppx, self.nS, pmp, pmn, self.nM,
                                           1 if build_index else 0, device, C.byref(self.h)))
        _LIVE.add(self)

    def set_scene(self, scene_pos, scene_nrm, scene_prob, scene_pixel=None):
        """The next camera frame against the same model (stocs_ctx_set_scene): keeps the model and its PPF index."""
        self._sp, psp = capi.f32(scene_pos)
        self._sn, psn = capi.f32(scene_nrm)
        self._spr, pspr = capi.f32(scene_prob)
        ppx = None
        if scene_pixel is not None:
            self._spx, ppx = capi.i32(scene_pixel)
        capi.check(self.L.stocs_ctx_set_scene(self.h, psp, psn, pspr, ppx, len(self._sp)))
        self.nS = len(self._sp)

    def close(self):
        _LIVE.discard(self)
        if getattr(self, "h", None) and self.h.value:
            self.L.stocs_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- getters (stocs.hpp:115-134) ----
    def get_scene_centroid(self):
        s = np.zeros(3, np.float32)
        capi.check(self.L.stocs_get_centroids(self.h, s.ctypes.data_as(capi._fp), None))
        return s

    def get_model_centroid(self):
        m = np.zeros(3, np.float32)
        capi.check(self.L.stocs_get_centroids(self.h, None, m.ctypes.data_as(capi._fp)))
        return m

    def set_edge_map(self, edge):
        e = np.ascontiguousarray(edge, np.uint8)
        capi.check(self.L.stocs_set_edge_map(self.h, e.ctypes.data_as(capi._u8p)))

    def reset_trial(self):
        capi.check(self.L.stocs_reset_trial(self.h))

    # ---- PPF index ----
    def index_exists(self, key):
        k, pk = capi.i32(key)
        r = C.c_int(0)
        capi.check(self.L.stocs_index_exists(self.h, pk, C.byref(r)))
        return bool(r.value)

    def index_lookup(self, key):
        k, pk = capi.i32(key)
        n = C.c_int64(0)
        capi.check(self.L.stocs_index_lookup(self.h, pk, None, 0, C.byref(n)))
        out = np.zeros((n.value, 2), np.int32)
        if n.value:
            capi.check(self.L.stocs_index_lookup(self.h, pk, out.ctypes.data_as(capi._ip), n.value, C.byref(n)))
        return out

    def index_save(self, path):
        capi.check(self.L.stocs_index_save(self.h, str(path).encode()))

    def index_load(self, path):
        capi.check(self.L.stocs_index_load(self.h, str(path).encode()))

    def index_stats(self):
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        capi.check(self.L.stocs_index_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # ---- base sampling (stocs.hpp:80-91) ----
    def sample_bases(self, seed, n_attempts, first_attempt=0, mode=0, dispersion=0.9):
        ids = np.zeros((n_attempts, 4), np.int32)
        inv = np.zeros((n_attempts, 2), np.float32)
        valid = np.zeros(n_attempts, np.int32)
        capi.check(self.L.stocs_sample_bases(self.h, mode, seed, first_attempt, n_attempts, dispersion,
                                             ids.ctypes.data_as(capi._ip), inv.ctypes.data_as(capi._fp),
                                             valid.ctypes.data_as(capi._ip)))
        return valid.astype(bool), ids, inv

    def sample_class_base(self, seed, attempt):
        v, ids, inv = self.sample_bases(seed, 1, attempt, 0)
        return bool(v[0]), ids[0], inv[0]

    def set_bases(self, ids, inv):
        ids, pi = capi.i32(np.asarray(ids).reshape(-1, 4))
        inv, pv = capi.f32(np.asarray(inv).reshape(-1, 2))
        capi.check(self.L.stocs_set_bases(self.h, len(ids), pi, pv))

    def class_pass(self, k, b3, w_in):
        b, pb = capi.i32(b3)
        w, pw = capi.f32(w_in)
        out = np.zeros_like(w)
        capi.check(self.L.stocs_class_pass(self.h, k, pb, pw, out.ctypes.data_as(capi._fp)))
        return out

    def try_sampled_base(self, ids):
        ids, pi = capi.i32(np.array(ids).copy())
        inv = np.zeros(2, np.float32)
        ok = C.c_int(0)
        capi.check(self.L.stocs_try_sampled_base(self.h, pi, inv.ctypes.data_as(capi._fp), C.byref(ok)))
        return bool(ok.value), ids, inv

    def draw(self, w, r64):
        w, pw = capi.f32(w)
        idx = C.c_int(0)
        capi.check(self.L.stocs_draw(self.h, pw, len(w), r64, C.byref(idx)))
        return idx.value

    def last_sampling_form(self):
        """-> dict(kernel, threads, lds_bytes, cap, launches, redone) of the last sample_bases / run_trials call, class or instance mode
        (stocs_last_sampling_form); kernel is one of capi.FORM_NAMES' names."""
        k, t, cap, nl, nr = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        lds = C.c_int64(0)
        capi.check(self.L.stocs_last_sampling_form(self.h, C.byref(k), C.byref(t), C.byref(lds), C.byref(cap), C.byref(nl), C.byref(nr)))
        return dict(kernel=capi.FORM_NAMES[k.value], threads=t.value, lds_bytes=lds.value, cap=cap.value, launches=nl.value, redone=nr.value)

    def last_instance_attempts(self):
        """-> (n, 4) int32, one row per attempt of the last sample_bases(mode=1) call: survivors inside the mask, point 1, whether the
        attempt reached its mask, and the mask's path -- runs in the disc's rows for a new flood fill, -1 for a reused mask, 0 for a
        failed first draw (stocs_last_instance_attempts)."""
        n = C.c_int(0)
        capi.check(self.L.stocs_last_instance_attempts(self.h, None, 0, C.byref(n)))
        rec = np.zeros((n.value, 4), np.int32)
        if n.value:
            capi.check(self.L.stocs_last_instance_attempts(self.h, rec.ctypes.data_as(capi._ip), n.value, C.byref(n)))
        return rec

    def debug_draw_point1(self, r64):
        """-> the point the lean class kernel draws first for every 64-bit word of r64 against the current prior, -1 for a zero
        total (stocs_debug_draw_point1)."""
        r = np.ascontiguousarray(r64, np.uint64)
        idx = np.zeros(len(r), np.int32)
        capi.check(self.L.stocs_debug_draw_point1(self.h, r.ctypes.data_as(C.POINTER(C.c_uint64)), len(r), idx.ctypes.data_as(capi._ip)))
        return idx

    # ---- congruent sets (stocs.hpp:93-96) ----
    def find_congruent_all(self):
        n = C.c_int64(0)
        capi.check(self.L.stocs_find_congruent_all(self.h, C.byref(n)))
        return n.value

    def get_quads(self, slot):
        n = C.c_int64(0)
        capi.check(self.L.stocs_get_quads(self.h, slot, None, 0, C.byref(n)))
        out = np.zeros((n.value, 4), np.int32)
        if n.value:
            capi.check(self.L.stocs_get_quads(self.h, slot, out.ctypes.data_as(capi._ip), n.value, C.byref(n)))
        return out

    def num_quads(self, slot):
        n = C.c_int64(0)
        capi.check(self.L.stocs_get_quads(self.h, slot, None, 0, C.byref(n)))
        return n.value

    def get_quads_at(self, slot, ranks):
        """Quads of base `slot` at ranks of its walk order (stocs_get_quads_at)."""
        r = np.ascontiguousarray(ranks, np.int64)
        out = np.zeros((len(r), 4), np.int32)
        capi.check(self.L.stocs_get_quads_at(self.h, slot, r.ctypes.data_as(capi._i64p), len(r), out.ctypes.data_as(capi._ip)))
        return out

    def find_congruent_sets_on_model(self, base_indices, invariant1, invariant2):
        self.set_bases(np.asarray(base_indices).reshape(1, 4), np.array([[invariant1, invariant2]], np.float32))
        self.find_congruent_all()
        return self.get_quads(0)

    # ---- transforms (stocs.hpp:98-101) ----
    def get_rigid_transform_from_congruent_pair(self, base_indices, quad):
        ids, pi = capi.i32(base_indices)
        q, pq = capi.i32(quad)
        T = np.zeros(16, np.float32); P = np.zeros(16, np.float32)
        ok = C.c_int(0)
        capi.check(self.L.stocs_rigid_transform(self.h, pi, pq, T.ctypes.data_as(capi._fp), P.ctypes.data_as(capi._fp), C.byref(ok)))
        return bool(ok.value), T, P

    def make_transforms(self, max_per_base=200, seed=0):
        n = C.c_int(0)
        capi.check(self.L.stocs_make_transforms(self.h, max_per_base, seed, C.byref(n)))
        return n.value

    def get_pose_candidates(self):
        n = C.c_int(0)
        capi.check(self.L.stocs_get_candidates(self.h, None, None, None, None, 0, C.byref(n)))
        T = np.zeros((n.value, 16), np.float32); P = np.zeros((n.value, 16), np.float32)
        l = np.zeros(n.value, np.float32); b = np.zeros(n.value, np.int32)
        if n.value:
            capi.check(self.L.stocs_get_candidates(self.h, T.ctypes.data_as(capi._fp), P.ctypes.data_as(capi._fp),
                                                   l.ctypes.data_as(capi._fp), b.ctypes.data_as(capi._ip), n.value, C.byref(n)))
        return T, P, l, b

    # ---- verification (stocs.hpp:103-107) ----
    def compute_alignment_score_for_rigid_transform(self, T16):
        return float(self.score_transforms(np.asarray(T16, np.float32).reshape(1, 16))[0])

    def score_transforms(self, T16):
        T, pT = capi.f32(T16)
        n = T.size // 16
        out = np.zeros(n, np.float32)
        capi.check(self.L.stocs_score_transforms(self.h, pT, n, out.ctypes.data_as(capi._fp)))
        return out

    def refine_poses(self, T16, max_iterations=5, max_correspondence_distance=0.035, src_idx=None):
        """Point-to-plane refinement of n centred-frame hypotheses on this context (stocs_refine_poses; the reference's
        clustering::point_to_plane_icp per hypothesis) -> (T16_refined (n, 16), pose16_camera (n, 16), lcp (n,), n_corr (n,),
        iterations (n,))."""
        T, pT = capi.f32(T16)
        n = T.size // 16
        idx, pidx = (None, None) if src_idx is None else capi.i32(src_idx)
        To = np.zeros((n, 16), np.float32); Po = np.zeros((n, 16), np.float32); lcp = np.zeros(n, np.float32)
        nc = np.zeros(n, np.int32); it = np.zeros(n, np.int32)
        capi.check(self.L.stocs_refine_poses(self.h, pT, n, pidx, 0 if idx is None else len(idx), max_iterations, max_correspondence_distance,
                                             To.ctypes.data_as(capi._fp), Po.ctypes.data_as(capi._fp), lcp.ctypes.data_as(capi._fp),
                                             nc.ctypes.data_as(capi._ip), it.ctypes.data_as(capi._ip)))
        return To, Po, lcp, nc, it

    def refine_detail(self, T16, max_correspondence_distance=0.035, src_idx=None, sums=True):
        """The refinement's first evaluation of one centred-frame hypothesis (stocs_refine_detail) -> (match (n_src,) model index or
        -1, counted (n_src,) uint8, sums28 (28,) float64: A^T A upper triangle | A^T b | count, or None)."""
        T, pT = capi.f32(T16)
        assert T.size == 16
        idx, pidx = (None, None) if src_idx is None else capi.i32(src_idx)
        n = self.nS if idx is None else len(idx)
        match = np.zeros(max(n, 1), np.int32); counted = np.zeros(max(n, 1), np.uint8)
        s28 = np.zeros(28, np.float64) if sums else None
        capi.check(self.L.stocs_refine_detail(self.h, pT, pidx, 0 if idx is None else n, max_correspondence_distance, match.ctypes.data_as(capi._ip),
                                              counted.ctypes.data_as(capi._u8p), s28.ctypes.data_as(C.POINTER(C.c_double)) if sums else None))
        return match[:n], counted[:n], s28

    @staticmethod
    def robust_params(max_iterations=5, max_correspondence_distance=0.035, keep_ratio=0.7, max_normal_deg=30.0):
        """stocs_refine_robust_params from the Python arguments.  max_normal_deg -> min_normal_cos ONCE: the cosine of the angle in
        double (math.cos(deg * pi / 180)), rounded to float when it enters the struct -- the conversion include/stocs.hpp's
        refine_pose_candidates_robust makes; None turns the gate off (min_normal_cos = -2).  A caller who needs an exact cosine (-1, 0,
        1 at the gate's edges) passes a capi.RefineRobustParams of their own."""
        mc = -2.0 if max_normal_deg is None else math.cos(float(max_normal_deg) * math.pi / 180.0)
        return capi.RefineRobustParams(int(max_iterations), float(max_correspondence_distance), float(keep_ratio), mc)

    @staticmethod
    def robust_setting(keep_ratio, max_normal_deg):
        """(keep_ratio, min_normal_cos) as the two floats of stocs_run_trials_post_robust / stocs_track_poses_robust: the conversion of
        robust_params (degrees -> cosine once, in double, rounded to float at the call; None: gate off)."""
        prm = StocsEstimator.robust_params(0, 1.0, keep_ratio, max_normal_deg)
        return prm.keep_ratio, prm.min_normal_cos

    def refine_poses_robust(self, T16, max_iterations=5, max_correspondence_distance=0.035, keep_ratio=0.7, max_normal_deg=30.0, src_idx=None, params=None):
        """Trimmed, normal-gated point-to-plane refinement of n centred-frame hypotheses (stocs_refine_poses_robust): per iteration
        the nearest keep_ratio of the candidate pairs enter the system, and a pair whose normals differ by more than max_normal_deg
        (None: no gate; converted as robust_params documents) is no candidate.  params: a capi.RefineRobustParams that replaces the
        four scalars.  -> (T16_refined (n, 16), pose16_camera (n, 16), lcp (n,), n_corr (n,) kept pairs, n_cand (n,), iterations (n,))."""
        T, pT = capi.f32(T16)
        n = T.size // 16
        idx, pidx = (None, None) if src_idx is None else capi.i32(src_idx)
        prm = params if params is not None else self.robust_params(max_iterations, max_correspondence_distance, keep_ratio, max_normal_deg)
        To = np.zeros((n, 16), np.float32); Po = np.zeros((n, 16), np.float32); lcp = np.zeros(n, np.float32)
        nc = np.zeros(n, np.int32); ncand = np.zeros(n, np.int32); it = np.zeros(n, np.int32)
        capi.check(self.L.stocs_refine_poses_robust(self.h, pT, n, pidx, 0 if idx is None else len(idx), C.byref(prm), To.ctypes.data_as(capi._fp),
                                                    Po.ctypes.data_as(capi._fp), lcp.ctypes.data_as(capi._fp), nc.ctypes.data_as(capi._ip),
                                                    ncand.ctypes.data_as(capi._ip), it.ctypes.data_as(capi._ip)))
        return To, Po, lcp, nc, ncand, it

    def refine_robust_detail(self, T16, max_correspondence_distance=0.035, keep_ratio=0.7, max_normal_deg=30.0, src_idx=None, params=None):
        """The robust refinement's first evaluation of one centred-frame hypothesis (stocs_refine_robust_detail; arguments as
        refine_poses_robust) -> dict: match (n_src,) model index or -1, candidate, kept (n_src,) uint8, rank (n_src,) uint32 (the bits
        of the float squared distance, 0xFFFFFFFF for a non-candidate), k, n_cand, sums28 (28,) float64 over the kept pairs."""
        T, pT = capi.f32(T16)
        assert T.size == 16
        idx, pidx = (None, None) if src_idx is None else capi.i32(src_idx)
        n = self.nS if idx is None else len(idx)
        prm = params if params is not None else self.robust_params(1, max_correspondence_distance, keep_ratio, max_normal_deg)
        m = max(n, 1)
        match = np.zeros(m, np.int32); cand = np.zeros(m, np.uint8); kept = np.zeros(m, np.uint8); rank = np.zeros(m, np.uint32)
        k = C.c_int32(0); ncand = C.c_int32(0); s28 = np.zeros(28, np.float64)
        capi.check(self.L.stocs_refine_robust_detail(self.h, pT, pidx, 0 if idx is None else n, C.byref(prm), match.ctypes.data_as(capi._ip),
                                                     cand.ctypes.data_as(capi._u8p), kept.ctypes.data_as(capi._u8p), rank.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                     C.byref(k), C.byref(ncand), s28.ctypes.data_as(C.POINTER(C.c_double))))
        return dict(match=match[:n], candidate=cand[:n], kept=kept[:n], rank=rank[:n], k=int(k.value), n_cand=int(ncand.value), sums28=s28)

    def refine_robust_workspace(self):
        """(address, bytes) of the robust refinement's device workspace (stocs_refine_robust_workspace)."""
        p = C.c_void_p(); b = C.c_uint64(0)
        capi.check(self.L.stocs_refine_robust_workspace(self.h, C.byref(p), C.byref(b)))
        return int(p.value or 0), int(b.value)

    def cluster_trials_device(self, poses16, lcp, cand_off, best_score, acceptable_fraction, maximum_pose_count, min_distance, min_angle, sym):
        """The device clustering of trial batches on given candidates (stocs_cluster_trials_device) -> (out_off (n_trials + 1,), out_cnt
        (n_trials,), out_idx (out_off[-1],) with -1 in the unused slots, round0_survivors (n_trials,))."""
        P, pP = capi.f32(poses16); l, pl = capi.f32(lcp); off, poff = capi.i32(cand_off); b, pb = capi.f32(best_score); s, ps = capi.f32(sym)
        nT = len(off) - 1
        assert nT >= 0 and len(b) == nT and s.size == 3
        n = np.diff(off.astype(np.int64))
        cap = int(np.minimum(max(int(maximum_pose_count), 0) + 1, np.maximum(n, 0)).sum()) if nT else 0
        out_off = np.zeros(nT + 1, np.int32); out_cnt = np.zeros(max(nT, 1), np.int32); out_idx = np.zeros(max(cap, 1), np.int32)
        surv = np.zeros(max(nT, 1), np.int32)
        capi.check(self.L.stocs_cluster_trials_device(self.h, pP, pl, poff, pb, nT, acceptable_fraction, maximum_pose_count, min_distance, min_angle, ps,
                                                      out_off.ctypes.data_as(capi._ip), out_cnt.ctypes.data_as(capi._ip), out_idx.ctypes.data_as(capi._ip),
                                                      cap, surv.ctypes.data_as(capi._ip)))
        return out_off, out_cnt[:nT], out_idx[:cap], surv[:nT]

    def track_poses(self, priors_pose16_camera, rounds=TRACK_DEFAULTS["rounds"], samples=TRACK_DEFAULTS["samples"],
                    max_translation=TRACK_DEFAULTS["max_translation"], max_rotation_deg=TRACK_DEFAULTS["max_rotation_deg"], shrink=TRACK_DEFAULTS["shrink"],
                    seed=TRACK_DEFAULTS["seed"], refine_iterations=TRACK_DEFAULTS["refine_iterations"],
                    max_correspondence_distance=TRACK_DEFAULTS["max_correspondence_distance"], keep_details=False, keep_ratio=None, max_normal_deg=None):
        """Local search around n camera-frame priors (column-major 16 floats each) on this context's scene (stocs_track_poses) -> a
        structured array with the fields of stocs_track_result (prior_lcp, lcp, pose16, refined_lcp, refined_pose16, n_correspondences,
        iterations), one record per prior.  keep_details: every round's candidates and scores stay readable through track_round.
        keep_ratio / max_normal_deg: with either given, the final incumbents are refined by the trimmed, normal-gated form
        (stocs_track_poses_robust; keep_ratio defaults to 1, max_normal_deg None leaves the gate off, converted as robust_params
        documents); both None: the plain entry point."""
        P, pP = capi.f32(priors_pose16_camera)
        n = P.size // 16
        prm = capi.TrackParams(rounds, samples, max_translation, max_rotation_deg, shrink, seed, refine_iterations, max_correspondence_distance,
                               1 if keep_details else 0)
        buf = (capi.TrackResult * max(n, 1))()
        if keep_ratio is None and max_normal_deg is None:
            capi.check(self.L.stocs_track_poses(self.h, pP, n, C.byref(prm), buf))
        else:
            keep, mc = self.robust_setting(1.0 if keep_ratio is None else keep_ratio, max_normal_deg)
            capi.check(self.L.stocs_track_poses_robust(self.h, pP, n, C.byref(prm), keep, mc, buf))
        return np.frombuffer(buf, dtype=_TRACK_DTYPE, count=n).copy()

    def set_frame(self, depth_u16, prob_u16, K, depth_scale):
        """The camera frame this context's scene came from (stocs_ctx_set_frame): depth (height, width) uint16, the object's
        class-probability image of the same shape or None, K = (fx, cx, fy, cy), metres per depth unit.  Kept on the device until the
        next set_frame; independent of set_scene."""
        d = np.ascontiguousarray(depth_u16, np.uint16)
        if d.ndim != 2:
            raise ValueError("depth image must be (height, width)")
        pp = None
        if prob_u16 is not None:
            p = np.ascontiguousarray(prob_u16, np.uint16)
            if p.shape != d.shape:
                raise ValueError("class-probability image %s does not match the depth image %s" % (p.shape, d.shape))
            pp = p.ctypes.data_as(C.POINTER(C.c_uint16))
        cam = capi.Camera(float(K[0]), float(K[1]), float(K[2]), float(K[3]), float(depth_scale), d.shape[1], d.shape[0], 0)
        capi.check(self.L.stocs_ctx_set_frame(self.h, C.byref(cam), d.ctypes.data_as(C.POINTER(C.c_uint16)), pp))
        self._frame_hw = d.shape   # the label images of render_labels / explain_poses take their shape from it

    def depth_check_poses(self, poses16, **params):
        """n camera-frame poses (column-major 16 floats each) against the frame of set_frame (stocs_depth_check_poses) -> a structured
        array with the fields of stocs_depth_result, one record per pose.  params: fields of stocs_depth_params (tolerance,
        class_threshold, self_occlusion, cell_px, occlusion_margin) over the library's defaults."""
        P, pP = capi.f32(poses16)
        n = P.size // 16
        prm = capi.DepthParams()
        self.L.stocs_default_depth_params(C.byref(prm))
        for k, v in params.items():
            if k not in dict(capi.DepthParams._fields_):
                raise TypeError("depth_check_poses: unknown parameter %r" % k)
            setattr(prm, k, v)
        buf = (capi.DepthResult * max(n, 1))()
        capi.check(self.L.stocs_depth_check_poses(self.h, pP, n, C.byref(prm), buf))
        return np.frombuffer(buf, dtype=_DEPTH_DTYPE, count=n).copy()

    def _vsd_params(self, who, params, taus=None):
        prm = capi.VsdParams()
        self.L.stocs_default_vsd_params(C.byref(prm))
        for k, v in params.items():
            if k not in ("surfel_radius", "max_splat_px", "delta"):
                raise TypeError("%s: unknown parameter %r" % (who, k))
            setattr(prm, k, v)
        if taus is not None:
            t = [float(x) for x in np.asarray(taus, np.float32).reshape(-1)]
            if len(t) > 16:
                raise ValueError("%s: at most 16 taus" % who)
            prm.n_tau = len(t)
            for i, x in enumerate(t):
                prm.tau[i] = x
        return prm

    def render_depth(self, poses16, **params):
        """The surfel depth image of each of n camera-frame poses against the camera of set_frame (stocs_render_depth) -> (n, height,
        width) float32, the z of the nearest surfel per pixel, 0 where nothing is.  params: surfel_radius, max_splat_px over the
        library's defaults."""
        P, pP = capi.f32(poses16)
        n = P.size // 16
        prm = self._vsd_params("render_depth", params)
        H, W = self._frame_shape("render_depth")
        out = np.zeros((n, H, W), np.float32)
        capi.check(self.L.stocs_render_depth(self.h, pP, n, C.byref(prm), out.ctypes.data_as(capi._fp)))
        return out

    def pose_errors_vsd(self, est, gt, taus=None, **params):
        """n estimated camera-frame poses against ground truth by BOP's visible-surface discrepancy on the frame of set_frame
        (stocs_pose_errors_vsd): gt holds one pose or n; taus the misalignment tolerances in metres (at most 16), None: BOP's 0.05,
        0.10 .. 0.50 times model_diameter() -> a structured array with the fields of stocs_vsd_record, one record per estimate: `e`
        holds the error per tau (entries beyond the taus are 0).  params: surfel_radius, max_splat_px, delta over the library's defaults."""
        P, pP = capi.f32(est)
        G, pG = capi.f32(gt)
        if P.size % 16 or G.size % 16 or G.size == 0:
            raise ValueError("pose_errors_vsd: poses are 16 floats each")
        n, n_gt = P.size // 16, G.size // 16
        if taus is None:
            d = np.float32(self.model_diameter())
            taus = [np.float32(t) * d for t in BOP_VSD_TAUS]
        prm = self._vsd_params("pose_errors_vsd", params, taus)
        buf = (capi.VsdRecord * max(n, 1))()
        capi.check(self.L.stocs_pose_errors_vsd(self.h, pP, n, pG, n_gt, C.byref(prm), buf))
        return np.frombuffer(buf, dtype=_VSD_DTYPE, count=n).copy()

    def set_mesh(self, vertices, triangles):
        """The model as a triangle mesh, in the frame of the model points the estimator was made with (stocs_ctx_set_mesh): vertices
        (nv, 3) float32, triangles (nt, 3) int32.  It stays on the device until the next call; no triangles drops it."""
        V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        T = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        capi.check(self.L.stocs_ctx_set_mesh(self.h, V.ctypes.data_as(capi._fp), len(V), T.ctypes.data_as(capi._ip), len(T)))
        # refine_poses_visible_damped's default pivot: the mean of the vertices
        self._mesh_centre = tuple(float(x) for x in V.astype(np.float64).mean(axis=0).astype(np.float32)) if len(V) and len(T) else (0.0, 0.0, 0.0)

    def mesh_info(self):
        """(vertices, triangles) of the mesh on the context, (0, 0) without one"""
        nv, nt = C.c_int(0), C.c_int(0)
        capi.check(self.L.stocs_ctx_mesh_info(self.h, C.byref(nv), C.byref(nt)))
        return nv.value, nt.value

    def render_depth_mesh(self, poses16):
        """render_depth from the mesh of set_mesh (stocs_render_depth_mesh): exact, watertight, no radius -> (n, height, width) float32"""
        P, pP = capi.f32(poses16)
        n = P.size // 16
        H, W = self._frame_shape("render_depth_mesh")
        out = np.zeros((n, H, W), np.float32)
        capi.check(self.L.stocs_render_depth_mesh(self.h, pP, n, out.ctypes.data_as(capi._fp)))
        return out

    def pose_errors_vsd_mesh(self, est, gt, taus=None, **params):
        """pose_errors_vsd with the mesh of set_mesh rendered in place of the surfels (stocs_pose_errors_vsd_mesh): the same records, for
        pose_recall_vsd as they are.  params: delta over the library's default."""
        P, pP = capi.f32(est)
        G, pG = capi.f32(gt)
        if P.size % 16 or G.size % 16 or G.size == 0:
            raise ValueError("pose_errors_vsd_mesh: poses are 16 floats each")
        n, n_gt = P.size // 16, G.size // 16
        if "surfel_radius" in params or "max_splat_px" in params:
            raise TypeError("pose_errors_vsd_mesh: a mesh has no surfel parameters")
        if taus is None:
            d = np.float32(self.model_diameter())
            taus = [np.float32(t) * d for t in BOP_VSD_TAUS]
        prm = self._vsd_params("pose_errors_vsd_mesh", params, taus)
        buf = (capi.VsdRecord * max(n, 1))()
        capi.check(self.L.stocs_pose_errors_vsd_mesh(self.h, pP, n, pG, n_gt, C.byref(prm), buf))
        return np.frombuffer(buf, dtype=_VSD_DTYPE, count=n).copy()

    def last_mesh_call_timing(self):
        """last_call_timing for the last pose_errors_vsd_mesh (stocs_mesh_last_call_timing)"""
        labels = (C.c_char_p * 18)()
        ms = (C.c_double * 18)()
        n = C.c_int(0)
        capi.check(self.L.stocs_mesh_last_call_timing(self.h, labels, ms, 18, C.byref(n)))
        return [(labels[i].decode(), ms[i]) for i in range(n.value)]

    def pose_errors(self, est, gt):
        """n estimated camera-frame poses (column-major 16 floats each) against ground truth (stocs_pose_errors): gt holds one pose (every
        estimate against it) or n (estimate k against gt k) -> a structured array with the fields of stocs_pose_error, one record per
        estimate: ADD (`add`), ADD-S (`adds`), their maxima, in metres."""
        P, pP = capi.f32(est)
        G, pG = capi.f32(gt)
        if P.size % 16 or G.size % 16 or G.size == 0:
            raise ValueError("pose_errors: poses are 16 floats each")
        n, n_gt = P.size // 16, G.size // 16
        buf = (capi.PoseError * max(n, 1))()
        capi.check(self.L.stocs_pose_errors(self.h, pP, n, pG, n_gt, buf))
        return np.frombuffer(buf, dtype=_POSE_ERROR_DTYPE, count=n).copy()

    def pose_errors_detail(self, est, gt):
        """One pair of camera-frame poses (stocs_pose_errors_detail) -> (e, s, nn), one entry per model point: the distance to the same
        point under gt, the distance to the nearest point under gt, and that point's index (-1: none)."""
        P, pP = capi.f32(est)
        G, pG = capi.f32(gt)
        if P.size != 16 or G.size != 16:
            raise ValueError("pose_errors_detail: one pose of 16 floats each")
        e, s, nn = np.empty(self.nM, np.float32), np.empty(self.nM, np.float32), np.empty(self.nM, np.int32)
        capi.check(self.L.stocs_pose_errors_detail(self.h, pP, pG, e.ctypes.data_as(capi._fp), s.ctypes.data_as(capi._fp), nn.ctypes.data_as(capi._ip)))
        return e, s, nn

    @staticmethod
    def _sym_camera(camera):
        """camera: None, a capi.Camera, or the intrinsics (fx, cx, fy, cy) in set_frame's order"""
        if camera is None or isinstance(camera, capi.Camera):
            return camera
        K = [float(x) for x in camera]
        if len(K) != 4:
            raise ValueError("camera: the four intrinsics fx, cx, fy, cy")
        return capi.Camera(K[0], K[1], K[2], K[3], 1.0, 0, 0, 0)

    def pose_errors_sym(self, est, gt, symmetries, camera=None):
        """n estimated camera-frame poses against ground truth under K model symmetries (stocs_pose_errors_sym): gt holds one pose or n,
        symmetries K column-major 4x4 transforms of the model frame (symmetry_set builds them from a descriptor), camera None (no MSPD),
        the intrinsics (fx, cx, fy, cy) or a capi.Camera -> a structured array with the fields of stocs_pose_error_sym, one record per
        estimate: MSSD (`mssd`) and symmetric ADD (`add`) in metres, MSPD (`mspd`) in pixels, and the symmetry that attains each."""
        P, pP = capi.f32(est)
        G, pG = capi.f32(gt)
        S, pS = capi.f32(symmetries)
        if P.size % 16 or G.size % 16 or G.size == 0 or S.size % 16:
            raise ValueError("pose_errors_sym: poses and symmetries are 16 floats each")
        n, n_gt, K = P.size // 16, G.size // 16, S.size // 16
        cam = self._sym_camera(camera)
        buf = (capi.PoseErrorSym * max(n, 1))()
        capi.check(self.L.stocs_pose_errors_sym(self.h, pP, n, pG, n_gt, pS, K, None if cam is None else C.byref(cam), buf))
        return np.frombuffer(buf, dtype=_POSE_ERROR_SYM_DTYPE, count=n).copy()

    def pose_errors_sym_detail(self, est, gt, symmetries, camera=None):
        """One pair of camera-frame poses under K symmetries (stocs_pose_errors_sym_detail) -> (add_fix, max3, max2), one entry per
        symmetry: the fixed-point sum of the distances, their maximum (metres) and the maximum projected distance (pixels; +inf without
        a camera)."""
        P, pP = capi.f32(est)
        G, pG = capi.f32(gt)
        S, pS = capi.f32(symmetries)
        if P.size != 16 or G.size != 16 or S.size % 16:
            raise ValueError("pose_errors_sym_detail: one pose of 16 floats each, symmetries of 16 floats each")
        K = S.size // 16
        cam = self._sym_camera(camera)
        af, m3, m2 = np.empty(max(K, 1), np.uint64), np.empty(max(K, 1), np.float32), np.empty(max(K, 1), np.float32)
        capi.check(self.L.stocs_pose_errors_sym_detail(self.h, pP, pG, pS, K, None if cam is None else C.byref(cam),
                                                       af.ctypes.data_as(C.POINTER(C.c_uint64)), m3.ctypes.data_as(capi._fp), m2.ctypes.data_as(capi._fp)))
        return af[:K], m3[:K], m2[:K]

    @staticmethod
    def _symmetry_params(reach, cos_normal):
        return capi.SymmetryParams(float(reach), float(cos_normal), (C.c_int32 * 2)(0, 0))

    def symmetry_errors(self, transforms, reach, cos_normal=0.8660254037844387):
        """The model under K transforms of its own frame against itself (stocs_symmetry_errors): transforms K column-major 4x4, reach the
        largest distance at which a transformed point still has a neighbour -> a structured array with the fields of
        stocs_symmetry_error, one record per transform: the clamped mean and the largest nearest-neighbour distance in metres, the count
        of points with no neighbour within reach, and the count of matched points whose normals disagree."""
        S, pS = capi.f32(transforms)
        if S.size % 16:
            raise ValueError("symmetry_errors: transforms are 16 floats each")
        K = S.size // 16
        prm = self._symmetry_params(reach, cos_normal)
        buf = (capi.SymmetryError * max(K, 1))()
        capi.check(self.L.stocs_symmetry_errors(self.h, pS, K, C.byref(prm), buf))
        return np.frombuffer(buf, dtype=_SYMMETRY_ERROR_DTYPE, count=K).copy()

    def symmetry_errors_detail(self, transform, reach, cos_normal=0.8660254037844387):
        """One transform (stocs_symmetry_errors_detail) -> (s, nn, dot), one entry per model point: the distance to the nearest
        untransformed point (+inf beyond reach), that point's index (-1 beyond reach) and the cosine between the two normals."""
        S, pS = capi.f32(transform)
        if S.size != 16:
            raise ValueError("symmetry_errors_detail: one transform of 16 floats")
        prm = self._symmetry_params(reach, cos_normal)
        s, nn, dot = np.empty(self.nM, np.float32), np.empty(self.nM, np.int32), np.empty(self.nM, np.float32)
        capi.check(self.L.stocs_symmetry_errors_detail(self.h, pS, C.byref(prm), s.ctypes.data_as(capi._fp), nn.ctypes.data_as(capi._ip),
                                                       dot.ctypes.data_as(capi._fp)))
        return s, nn, dot

    def find_symmetries(self, center=None, cap_set=capi.POSE_SYM_MAX, **search):
        """The model's symmetry axes and the set they generate (stocs_find_symmetries): center None (the centroid) or the point the axes
        pass through, search any field of stocs_symmetry_search -> (axes, set, sym3, flags): a structured array with the fields of
        stocs_symmetry_axis, best first; (K, 16) float32 transforms for pose_errors_sym, entry 0 the identity; the clustering descriptor
        (zeros when it cannot name what was found: capi.SYMMETRY_DESCRIPTOR_INEXACT in flags); flags."""
        prm = symmetry_search(**search)
        c3 = None if center is None else (C.c_float * 3)(*[float(x) for x in center])
        cap_axes = int(prm.n_refine)
        axes = (capi.SymmetryAxis * max(cap_axes, 1))()
        out = np.empty((max(int(cap_set), 1), 16), np.float32)
        n, K, flags = C.c_int(0), C.c_int(0), C.c_int(0)
        sym3 = (C.c_float * 3)()
        capi.check(self.L.stocs_find_symmetries(self.h, C.byref(prm), c3, axes, cap_axes, C.byref(n), out.ctypes.data_as(capi._fp), int(cap_set), C.byref(K),
                                                sym3, C.byref(flags)))
        return (np.frombuffer(axes, dtype=_SYMMETRY_AXIS_DTYPE, count=min(n.value, cap_axes)).copy(), out[:K.value].copy(),
                np.array(list(sym3), np.float32), flags.value)

    def model_diameter(self):
        """The largest distance between two model points (stocs_model_diameter), computed on the device once per context."""
        d = C.c_float()
        capi.check(self.L.stocs_model_diameter(self.h, C.byref(d)))
        return np.float32(d.value)

    def _render_params(self, who, params):
        prm = capi.RenderParams()
        self.L.stocs_default_render_params(C.byref(prm))
        for k, v in params.items():
            if k not in dict(capi.RenderParams._fields_):
                raise TypeError("%s: unknown parameter %r" % (who, k))
            setattr(prm, k, v)
        return prm

    def _frame_shape(self, who):
        if getattr(self, "_frame_hw", None) is None:
            raise ValueError("%s: no frame (set_frame)" % who)
        return self._frame_hw

    def render_poses(self, poses16, zkey, id_base=0, clear=False, **params):
        """n camera-frame poses (column-major 16 floats each) splatted into the device key buffer zkey (width*height uint64, e.g. from
        dev_alloc; stocs_render_poses): pose h writes id id_base + h wherever it is the nearest surface.  clear: the buffer is emptied
        first.  params: fields of stocs_render_params (point_radius, max_splat_px, tolerance, class_threshold) over the defaults."""
        P, pP = capi.f32(poses16)
        prm = self._render_params("render_poses", params)
        capi.check(self.L.stocs_render_poses(self.h, pP, P.size // 16, int(id_base), C.byref(prm), zkey, 1 if clear else 0))

    def render_resolve(self, poses16, zkey, id_base=0, **params):
        """The same poses and ids against the finished key buffer (stocs_render_resolve) -> a structured array with the fields of
        stocs_render_result (footprint, visible, hidden, no_depth, agree, in_front, behind, on_mask), one record per pose."""
        P, pP = capi.f32(poses16)
        n = P.size // 16
        prm = self._render_params("render_resolve", params)
        buf = (capi.RenderResult * max(n, 1))()
        capi.check(self.L.stocs_render_resolve(self.h, pP, n, int(id_base), C.byref(prm), zkey, buf))
        return np.frombuffer(buf, dtype=_RENDER_DTYPE, count=n).copy()

    def render_labels(self, zkey, **params):
        """-> (labels int32, state uint8), both (height, width), of the key buffer (stocs_render_labels): -1 / the id that owns the pixel;
        0 empty, 1 no_depth, 2 agree, 3 in_front, 4 behind, plus 16 when on_mask."""
        H, W = self._frame_shape("render_labels")
        prm = self._render_params("render_labels", params)
        lab = np.zeros((H, W), np.int32); st = np.zeros((H, W), np.uint8)
        capi.check(self.L.stocs_render_labels(self.h, zkey, C.byref(prm), lab.ctypes.data_as(capi._ip), st.ctypes.data_as(capi._u8p)))
        return lab, st

    def explain_poses(self, poses16, labels=False, **params):
        """n camera-frame poses of this context's model rendered together against the frame of set_frame (stocs_explain_poses) -> records
        (as render_resolve), or (records, labels, state) with labels=True (as render_labels; ids are the poses' indices)."""
        P, pP = capi.f32(poses16)
        n = P.size // 16
        prm = self._render_params("explain_poses", params)
        buf = (capi.RenderResult * max(n, 1))()
        if not labels:
            capi.check(self.L.stocs_explain_poses(self.h, pP, n, C.byref(prm), buf, None, None))
            return np.frombuffer(buf, dtype=_RENDER_DTYPE, count=n).copy()
        H, W = self._frame_shape("explain_poses")
        lab = np.zeros((H, W), np.int32); st = np.zeros((H, W), np.uint8)
        capi.check(self.L.stocs_explain_poses(self.h, pP, n, C.byref(prm), buf, lab.ctypes.data_as(capi._ip), st.ctypes.data_as(capi._u8p)))
        return np.frombuffer(buf, dtype=_RENDER_DTYPE, count=n).copy(), lab, st

    def scene_footprints(self, poses16, rows, slot_base, n_slots, claim="agree", **render_params):
        """n camera-frame poses of this context's model against the frame of set_frame (stocs_scene_footprints): pose h writes the pixels it
        claims -- claim "agree" or "on_mask" -- as the bit row of slot slot_base + h of the device pool rows (n_slots rows of
        scene_row_words(shape) uint32 each, e.g. from dev_alloc) -> a structured array with the fields of stocs_scene_record (footprint,
        no_depth, agree, in_front, behind, on_mask, claimed), one record per pose.  render_params: fields of stocs_render_params."""
        P, pP = capi.f32(poses16)
        n = P.size // 16
        if claim not in SCENE_CLAIMS:
            raise ValueError("scene_footprints: claim %r is neither 'agree' nor 'on_mask'" % (claim,))
        prm = self._render_params("scene_footprints", render_params)
        buf = (capi.SceneRecord * max(n, 1))()
        capi.check(self.L.stocs_scene_footprints(self.h, pP, n, int(slot_base), int(n_slots), C.byref(prm), SCENE_CLAIMS[claim], rows, buf))
        return np.frombuffer(buf, dtype=_SCENE_RECORD_DTYPE, count=n).copy()

    def _render_params_mesh(self, who, params):
        if "point_radius" in params or "max_splat_px" in params:
            raise TypeError("%s: a mesh has no splat parameters" % who)
        return self._render_params(who, params)

    def render_poses_mesh(self, poses16, zkey, id_base=0, clear=False):
        """render_poses from the mesh of set_mesh (stocs_render_poses_mesh): pose h writes id id_base + h wherever its exact surface is
        the nearest.  The key buffer may be shared with render_poses calls of this or other estimators.  No parameters: no radius."""
        P, pP = capi.f32(poses16)
        capi.check(self.L.stocs_render_poses_mesh(self.h, pP, P.size // 16, int(id_base), zkey, 1 if clear else 0))

    def render_resolve_mesh(self, poses16, zkey, id_base=0, **params):
        """render_resolve for poses rendered by render_poses_mesh (stocs_render_resolve_mesh) -> the same records; a pose's footprint is
        the pixel set of its own mesh image.  params: tolerance, class_threshold."""
        P, pP = capi.f32(poses16)
        n = P.size // 16
        prm = self._render_params_mesh("render_resolve_mesh", params)
        buf = (capi.RenderResult * max(n, 1))()
        capi.check(self.L.stocs_render_resolve_mesh(self.h, pP, n, int(id_base), C.byref(prm), zkey, buf))
        return np.frombuffer(buf, dtype=_RENDER_DTYPE, count=n).copy()

    def explain_poses_mesh(self, poses16, labels=False, **params):
        """explain_poses on the mesh of set_mesh (stocs_explain_poses_mesh) -> records, or (records, labels, state) with labels=True.
        params: tolerance, class_threshold."""
        P, pP = capi.f32(poses16)
        n = P.size // 16
        prm = self._render_params_mesh("explain_poses_mesh", params)
        buf = (capi.RenderResult * max(n, 1))()
        if not labels:
            capi.check(self.L.stocs_explain_poses_mesh(self.h, pP, n, C.byref(prm), buf, None, None))
            return np.frombuffer(buf, dtype=_RENDER_DTYPE, count=n).copy()
        H, W = self._frame_shape("explain_poses_mesh")
        lab = np.zeros((H, W), np.int32); st = np.zeros((H, W), np.uint8)
        capi.check(self.L.stocs_explain_poses_mesh(self.h, pP, n, C.byref(prm), buf, lab.ctypes.data_as(capi._ip), st.ctypes.data_as(capi._u8p)))
        return np.frombuffer(buf, dtype=_RENDER_DTYPE, count=n).copy(), lab, st

    def scene_footprints_mesh(self, poses16, rows, slot_base, n_slots, claim="agree", **render_params):
        """scene_footprints from the mesh of set_mesh (stocs_scene_footprints_mesh): the same rows and records, for scene_select as they
        are; a pool may mix slots of both kinds.  render_params: tolerance, class_threshold."""
        P, pP = capi.f32(poses16)
        n = P.size // 16
        if claim not in SCENE_CLAIMS:
            raise ValueError("scene_footprints_mesh: claim %r is neither 'agree' nor 'on_mask'" % (claim,))
        prm = self._render_params_mesh("scene_footprints_mesh", render_params)
        buf = (capi.SceneRecord * max(n, 1))()
        capi.check(self.L.stocs_scene_footprints_mesh(self.h, pP, n, int(slot_base), int(n_slots), C.byref(prm), SCENE_CLAIMS[claim], rows, buf))
        return np.frombuffer(buf, dtype=_SCENE_RECORD_DTYPE, count=n).copy()

    def render_mesh_last_device_ms(self):
        """(key render, resolve kernel) HIP-event ms of the last mesh render call with the option device_clock on; -1: not taken"""
        a, b = C.c_float(-1), C.c_float(-1)
        capi.check(self.L.stocs_render_mesh_last_device_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    @staticmethod
    def _fill_params(who, prm, params):
        """keyword arguments into a ctypes parameter struct.  A struct that extends another holds it in its first member, `base` or
        `damped`: a name is set in the struct that has it, a name that none has is a TypeError -> the innermost struct"""
        levels = [prm]
        while levels[-1]._fields_[0][0] in ("base", "damped"):
            levels.append(getattr(levels[-1], levels[-1]._fields_[0][0]))
        for k, v in params.items():
            s = next((s for s in levels if k in dict(s._fields_) and k not in ("base", "damped")), None)
            if s is None:
                raise TypeError("%s: unknown parameter %r" % (who, k))
            setattr(s, k, v)
        return levels[-1]

    def _take_pivot_model(self, who, params, damped):
        """params without pivot_model, which goes into the damped parameters: 3 floats, by default the mean of the vertices of set_mesh"""
        params = dict(params)
        pm = np.asarray(params.pop("pivot_model", getattr(self, "_mesh_centre", (0.0, 0.0, 0.0))), np.float32).reshape(-1)
        if pm.size != 3:
            raise ValueError("%s: pivot_model is 3 floats" % who)
        damped.pivot_model[:] = [float(x) for x in pm]
        return params

    def _refine_visible_params(self, who, params, form=""):
        """the parameter struct of a form ("", "_damped", "_contour"): params over the library's defaults -> (struct, its plain part)"""
        prm = _REFINE_VISIBLE_FORMS[form][0]()
        getattr(self.L, "stocs_default_refine_visible%s_params" % form)(C.byref(prm))
        if form:
            params = self._take_pivot_model(who, params, prm if form == "_damped" else prm.damped)
        return prm, self._fill_params(who, prm, params)

    def _refine_poses_visible(self, form, poses16, params, trace=None):
        """poses in, (n, 16) out, the form's records and, for a form that has one (trace is not None) and when asked for, the trace"""
        who = "refine_poses_visible" + form
        P, pP = capi.f32(poses16)
        if P.size % 16:
            raise ValueError("%s: poses are 16 floats each" % who)
        n = P.size // 16
        prm, base = self._refine_visible_params(who, params, form)
        out = np.zeros((n, 16), np.float32)
        buf = (_REFINE_VISIBLE_FORMS[form][1] * max(n, 1))()
        rows = max(base.max_iterations, 0) + 1
        tr = (capi.RefineVisibleTrace * max(n * rows, 1))() if trace else None
        capi.check(getattr(self.L, "stocs_" + who)(self.h, pP, n, C.byref(prm), out.ctypes.data_as(capi._fp), buf, *(() if trace is None else (tr,))))
        rec = np.frombuffer(buf, dtype=_REFINE_VISIBLE_FORMS[form][2], count=n).copy()
        if not trace:
            return out, rec
        return out, rec, np.frombuffer(tr, dtype=_REFINE_VISIBLE_TRACE_DTYPE, count=n * rows).copy().reshape(n, rows)

    def refine_poses_visible(self, poses16, **params):
        """n camera-frame poses of the mesh of set_mesh refined against the frame of set_frame on the surface each pose shows
        (stocs_refine_poses_visible): projective point-to-plane, every depth pixel under the rendered silhouette -> (poses (n, 16)
        float32, records): a structured array with the fields of stocs_refine_visible_result, one per pose, describing the last
        evaluation.  params: max_iterations, max_distance, min_view_cos, class_threshold over the library's defaults;
        max_iterations=0 scores the poses and changes nothing."""
        return self._refine_poses_visible("", poses16, params)

    def refine_poses_visible_damped(self, poses16, trace=False, **params):
        """refine_poses_visible with damped, bounded steps about a point of the object that are taken only when they lower the cost
        (stocs_refine_poses_visible_damped) -> (poses (n, 16) float32, records), or (poses, records, trace) with trace=True: records a
        structured array with the fields of stocs_refine_visible_damped_result (the plain record of the RETURNED pose, evaluations,
        rejected, cost, lambda), trace (n, max_iterations + 1) rows of stocs_refine_visible_trace.  params: the plain form's and lambda0,
        lambda_down, lambda_up, max_step_rotation (rad), max_step_translation (m), pivot (0: the camera's origin, 1: pivot_model),
        pivot_model (3 floats in the model frame; default: the mean of the vertices given to set_mesh) over the library's defaults."""
        return self._refine_poses_visible("_damped", poses16, params, bool(trace))

    def refine_poses_visible_contour(self, poses16, trace=False, **params):
        """refine_poses_visible_damped with the contour term: the frame's object pixels (class image) that a pose's render leaves uncovered
        pull it towards them (stocs_refine_poses_visible_contour) -> (poses (n, 16) float32, records), or (poses, records, trace) with
        trace=True: records a structured array with the fields of stocs_refine_visible_contour_result (the damped record of the RETURNED
        pose, object_px, uncovered, unreached, beyond, pulled, pull_rms).  params: the damped form's and contour_weight, pull_radius_px,
        pull_distance over the library's defaults; the frame of set_frame must carry a class image."""
        return self._refine_poses_visible("_contour", poses16, params, bool(trace))

    def refine_visible_contour_detail(self, pose16, **params):
        """The contour pass of one evaluation of one pose (stocs_refine_visible_contour_detail) -> (state (height, width) uint8: 1
        unreached, 2 beyond, 3 pulled, 0 everything else; nearest (height, width) int32: the linear index of the nearest silhouette
        pixel, -1 where there is none; the 29 contour sums float64)"""
        P, pP = capi.f32(pose16)
        if P.size != 16:
            raise ValueError("refine_visible_contour_detail: one pose of 16 floats")
        prm, _ = self._refine_visible_params("refine_visible_contour_detail", params, "_contour")
        H, W = self._frame_shape("refine_visible_contour_detail")
        st = np.zeros((H, W), np.uint8); near = np.zeros((H, W), np.int32); sums = np.zeros(29, np.float64)
        capi.check(self.L.stocs_refine_visible_contour_detail(self.h, pP, C.byref(prm), st.ctypes.data_as(capi._u8p), near.ctypes.data_as(capi._ip),
                                                              sums.ctypes.data_as(C.POINTER(C.c_double))))
        return st, near, sums

    def refine_visible_contour_last_device_ms(self):
        """HIP-event ms of the contour kernel of the last evaluation of the last refine_poses_visible_contour call with the option
        device_clock on; -1: not taken"""
        a = C.c_float(-1)
        capi.check(self.L.stocs_refine_visible_contour_last_device_ms(self.h, C.byref(a)))
        return a.value

    def refine_visible_detail(self, pose16, **params):
        """One evaluation of one pose as refine_poses_visible makes it (stocs_refine_visible_detail) -> (keys (height, width) uint64:
        float bits of the depth << 32 | triangle, all ones where empty; state (height, width) uint8: 0 empty, 1 no_depth, 2 off_class,
        3 too_far, 4 grazing, 5 counted; the 29 sums float64)"""
        P, pP = capi.f32(pose16)
        if P.size != 16:
            raise ValueError("refine_visible_detail: one pose of 16 floats")
        prm, _ = self._refine_visible_params("refine_visible_detail", params)
        H, W = self._frame_shape("refine_visible_detail")
        keys = np.zeros((H, W), np.uint64); st = np.zeros((H, W), np.uint8); sums = np.zeros(29, np.float64)
        capi.check(self.L.stocs_refine_visible_detail(self.h, pP, C.byref(prm), keys.ctypes.data_as(C.POINTER(C.c_uint64)), st.ctypes.data_as(capi._u8p),
                                                      sums.ctypes.data_as(C.POINTER(C.c_double))))
        return keys, st, sums

    def refine_visible_last_device_ms(self):
        """(render, accumulation, solve) HIP-event ms of the last iteration of the last refine_poses_visible call with the option
        device_clock on; -1: not taken"""
        a, b, d = C.c_float(-1), C.c_float(-1), C.c_float(-1)
        capi.check(self.L.stocs_refine_visible_last_device_ms(self.h, C.byref(a), C.byref(b), C.byref(d)))
        return a.value, b.value, d.value

    def scene_select(self, rows, shape, score, group, rec, group_cap=None, **params):
        """The walk over slots 0 .. n-1 of the pool rows of a frame of shape (height, width) (stocs_scene_select): score (n,), group (n,)
        ids, rec (n,) records of scene_footprints, group_cap one cap per group or None -> (records, selected): a structured array with
        the fields of stocs_scene_result (rank or -1, own, exclusive, reason), one per slot, and the selected slots in rank order.
        params: fields of stocs_scene_params (max_selected, min_pixels, min_exclusive_fraction, max_violation_fraction), and n_groups
        (default: the number of caps, else the largest group id + 1).  Uses this context's device and workspace only."""
        sc, psc = capi.f32(score)
        gr, pgr = capi.i32(group)
        rc = np.ascontiguousarray(rec, _SCENE_RECORD_DTYPE)
        n = sc.size
        if gr.size != n or rc.size != n:
            raise ValueError("scene_select: %d scores, %d groups, %d records" % (n, gr.size, rc.size))
        params = dict(params)
        pcap = None
        if group_cap is not None:
            cap, pcap = capi.i32(group_cap)
        n_groups = params.pop("n_groups", None)
        if n_groups is None:
            n_groups = cap.size if group_cap is not None else (int(gr.max()) + 1 if n else 1)
        if group_cap is not None and cap.size != n_groups:
            raise ValueError("scene_select: %d caps for %d groups" % (cap.size, n_groups))
        prm = capi.SceneParams()
        self.L.stocs_default_scene_params(C.byref(prm))
        for k, v in params.items():
            if k not in dict(capi.SceneParams._fields_):
                raise TypeError("scene_select: unknown parameter %r" % k)
            setattr(prm, k, v)
        buf = (capi.SceneResult * max(n, 1))()
        sel = np.zeros(max(n, 1), np.int32); ns = C.c_int(0)
        capi.check(self.L.stocs_scene_select(self.h, rows, n, int(shape[1]), int(shape[0]), psc, pgr, rc.ctypes.data_as(C.POINTER(capi.SceneRecord)), int(n_groups),
                                             pcap, C.byref(prm), buf, sel.ctypes.data_as(capi._ip), C.byref(ns)))
        return np.frombuffer(buf, dtype=_SCENE_RESULT_DTYPE, count=n).copy(), sel[:ns.value].copy()

    def select_instances(self, T16, max_instances=16, min_points=20, min_exclusive_fraction=0.5):
        """Which of n centred-frame hypotheses (column-major 16 floats each) are distinct instances (stocs_select_instances): walked best
        first, one is kept only if enough of the scene points it explains are explained by none kept before it -> (records, selected):
        a structured array with the fields of stocs_instance_result (rank or -1, own, exclusive, lcp), one record per hypothesis, and
        the indices of the selected ones in rank order."""
        T, pT = capi.f32(T16)
        n = T.size // 16
        prm = capi.InstanceParams(max_instances, min_points, min_exclusive_fraction)
        buf = (capi.InstanceResult * max(n, 1))()
        sel = np.zeros(max(min(max(int(max_instances), 0), n), 1), np.int32); ns = C.c_int(0)
        capi.check(self.L.stocs_select_instances(self.h, pT, n, C.byref(prm), buf, sel.ctypes.data_as(capi._ip), C.byref(ns)))
        return np.frombuffer(buf, dtype=_INSTANCE_DTYPE, count=n).copy(), sel[:ns.value].copy()

    def select_instances_rows(self, hit, counted, lcp, nS, max_instances=16, min_points=20, min_exclusive_fraction=0.5):
        """The set arithmetic, order and walk of select_instances on GIVEN detail rows (stocs_select_instances_rows): hit (n, nM) int32,
        counted (n, nM) uint8, lcp (n,) over nS scene points -> (records, selected).  Uses this context's device and workspace only."""
        H, pH = capi.i32(hit)
        K = np.ascontiguousarray(counted, np.uint8)
        l, pl = capi.f32(lcp)
        n = l.size
        if H.shape != K.shape or H.ndim != 2 or H.shape[0] != n:
            raise ValueError("hit %s and counted %s must both be (n, nM) with n = %d scores" % (H.shape, K.shape, n))
        prm = capi.InstanceParams(max_instances, min_points, min_exclusive_fraction)
        buf = (capi.InstanceResult * max(n, 1))()
        sel = np.zeros(max(min(max(int(max_instances), 0), n), 1), np.int32); ns = C.c_int(0)
        capi.check(self.L.stocs_select_instances_rows(self.h, pH, K.ctypes.data_as(capi._u8p), pl, n, H.shape[1], int(nS), C.byref(prm), buf,
                                                      sel.ctypes.data_as(capi._ip), C.byref(ns)))
        return np.frombuffer(buf, dtype=_INSTANCE_DTYPE, count=n).copy(), sel[:ns.value].copy()

    def track_round(self, prior, round):
        """-> (T16_centred (samples, 16), lcp (samples,)) of one round of one prior of the last track_poses(keep_details=True)."""
        n = C.c_int(0)
        capi.check(self.L.stocs_track_get_round(self.h, prior, round, None, None, 0, C.byref(n)))
        T = np.zeros((n.value, 16), np.float32); l = np.zeros(n.value, np.float32)
        capi.check(self.L.stocs_track_get_round(self.h, prior, round, T.ctypes.data_as(capi._fp), l.ctypes.data_as(capi._fp), n.value, C.byref(n)))
        return T, l

    def lcp_detail(self, T16):
        T, pT = capi.f32(T16)
        hit = np.zeros(self.nM, np.int32); counted = np.zeros(self.nM, np.uint8)
        capi.check(self.L.stocs_lcp_detail(self.h, pT, hit.ctypes.data_as(capi._ip), counted.ctypes.data_as(capi._u8p)))
        return hit, counted

    def lcp_hit_count(self, dT, n):
        """(hits, counted) over n device-resident transforms (stocs_lcp_hit_count): point queries that found a scene point within
        epsilon, and those of them that passed the normal test."""
        h = C.c_int64(0); k = C.c_int64(0)
        capi.check(self.L.stocs_lcp_hit_count(self.h, dT, n, C.byref(h), C.byref(k)))
        return h.value, k.value

    def lcp_gate_count(self, dT, n):
        """(queries in non-empty, mask-surviving cells; those the normal-cone gate rules out; ruled-out ones the detail form counts -- 0)
        over n device-resident transforms (stocs_lcp_gate_count)."""
        out = (C.c_int64 * 3)(0, 0, 0)
        capi.check(self.L.stocs_lcp_gate_count(self.h, dT, n, out))
        return int(out[0]), int(out[1]), int(out[2])

    def lcp_patch_normal_count(self, dT, n):
        """(sub-patches the sphere test leaves alive; those the normal-cone test rules out; ruled-out ones that hold a point the detail
        form counts -- 0) over n device-resident transforms (stocs_lcp_patch_normal_count)."""
        out = (C.c_int64 * 3)(0, 0, 0)
        capi.check(self.L.stocs_lcp_patch_normal_count(self.h, dT, n, out))
        return int(out[0]), int(out[1]), int(out[2])

    def patch_normal_info(self):
        """{"reach", "window", "filled", "launches"} of the sub-patch normal-cone test (stocs_patch_normal_info)"""
        out = (C.c_double * 4)()
        capi.check(self.L.stocs_patch_normal_info(self.h, out))
        return {"reach": out[0], "window": int(out[1]), "filled": bool(out[2]), "launches": int(out[3])}

    def compute_best_transform(self):
        s = C.c_float(0); i = C.c_int(-1)
        P = np.zeros(16, np.float32)
        capi.check(self.L.stocs_verify_all(self.h, C.byref(s), C.byref(i), P.ctypes.data_as(capi._fp)))
        self.best_lcp, self.best_index, self.best_pose = s.value, i.value, P
        return s.value, i.value, P

    # ---- trial batches: N independent trials in one set of launches (stocs_run_trials) ----
    def run_trials(self, seeds, n_attempts=100, mode=0, dispersion=0.9, max_per_base=200, keep_details=False, post=None, robust=None):
        """-> list of dicts (n_bases, n_candidates, n_quads, best_lcp, best_index, best_pose 16 floats), one per seed.
        post (a dict of trial_post's fields, or a capi.TrialPost): cluster, and refine, every trial's candidates inside the batch
        (stocs_run_trials_post); the hypotheses are then read with trials_get_hypotheses(t).
        robust (needs post): dict(keep_ratio=0.7, max_normal_deg=30.0 | None) -- the kept hypotheses are refined by the trimmed,
        normal-gated form (stocs_run_trials_post_robust; a missing key takes the default shown, None for the angle leaves the gate
        off); None: the plain entry point."""
        sd = np.ascontiguousarray(seeds, np.uint64)
        res = (capi.TrialResult * max(len(sd), 1))()
        if robust is not None and post is None:
            raise ValueError("run_trials: robust needs post (there is nothing to refine without it)")
        if post is None:
            capi.check(self.L.stocs_run_trials(self.h, mode, len(sd), sd.ctypes.data_as(C.POINTER(C.c_uint64)), n_attempts, dispersion, max_per_base,
                                               1 if keep_details else 0, res))
        else:
            pp = post if isinstance(post, capi.TrialPost) else trial_post(**post)
            if robust is None:
                capi.check(self.L.stocs_run_trials_post(self.h, mode, len(sd), sd.ctypes.data_as(C.POINTER(C.c_uint64)), n_attempts, dispersion, max_per_base,
                                                        1 if keep_details else 0, C.byref(pp), res))
            else:
                unknown = set(robust) - {"keep_ratio", "max_normal_deg"}
                if unknown:
                    raise ValueError("run_trials: robust has no %s" % sorted(unknown))
                keep, mc = self.robust_setting(robust.get("keep_ratio", 0.7), robust.get("max_normal_deg", 30.0))
                capi.check(self.L.stocs_run_trials_post_robust(self.h, mode, len(sd), sd.ctypes.data_as(C.POINTER(C.c_uint64)), n_attempts, dispersion,
                                                               max_per_base, 1 if keep_details else 0, C.byref(pp), keep, mc, res))
        # (one view of the whole result array: a ctypes field access per trial costs ~20 us, and a thousand trials take 60 ms of device time)
        a = np.frombuffer(res, dtype=_TRIAL_DTYPE, count=len(sd))
        nb, nc, nq, bl, bi, bp = (a["n_bases"].tolist(), a["n_candidates"].tolist(), a["n_quads"].tolist(), a["best_lcp"].tolist(), a["best_index"].tolist(),
                                  a["best_pose16"].copy())
        return [dict(n_bases=nb[t], n_candidates=nc[t], n_quads=nq[t], best_lcp=bl[t], best_index=bi[t], best_pose=bp[t]) for t in range(len(sd))]

    def trial_bases(self, trial):
        n = C.c_int(0)
        capi.check(self.L.stocs_trials_get_bases(self.h, trial, None, None, None, 0, C.byref(n)))
        ids = np.zeros((n.value, 4), np.int32); inv = np.zeros((n.value, 2), np.float32); valid = np.zeros(n.value, np.int32)
        capi.check(self.L.stocs_trials_get_bases(self.h, trial, ids.ctypes.data_as(capi._ip), inv.ctypes.data_as(capi._fp), valid.ctypes.data_as(capi._ip),
                                                 n.value, C.byref(n)))
        return valid.astype(bool), ids, inv

    def trial_quad_counts(self, trial):
        n = C.c_int(0)
        capi.check(self.L.stocs_trials_get_quad_counts(self.h, trial, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int64)
        if n.value:
            capi.check(self.L.stocs_trials_get_quad_counts(self.h, trial, out.ctypes.data_as(capi._i64p), n.value, C.byref(n)))
        return out

    def trials_get_hypotheses(self, trial):
        """-> the trial's kept hypotheses of the last post-processed batch, in cluster order: a structured array with the fields of
        stocs_trial_hypothesis (candidate_index, base_index, lcp, pose16, refined_lcp, refined_pose16, n_correspondences, iterations)."""
        n = C.c_int(0)
        capi.check(self.L.stocs_trials_get_hypotheses(self.h, trial, None, 0, C.byref(n)))
        buf = (capi.TrialHypothesis * max(n.value, 1))()
        if n.value:
            capi.check(self.L.stocs_trials_get_hypotheses(self.h, trial, buf, n.value, C.byref(n)))
        return np.frombuffer(buf, dtype=_HYP_DTYPE, count=n.value).copy()

    def trial_candidates(self, trial):
        n = C.c_int(0)
        capi.check(self.L.stocs_trials_get_candidates(self.h, trial, None, None, None, None, 0, C.byref(n)))
        T = np.zeros((n.value, 16), np.float32); P = np.zeros((n.value, 16), np.float32)
        l = np.zeros(n.value, np.float32); b = np.zeros(n.value, np.int32)
        if n.value:
            capi.check(self.L.stocs_trials_get_candidates(self.h, trial, T.ctypes.data_as(capi._fp), P.ctypes.data_as(capi._fp), l.ctypes.data_as(capi._fp),
                                                          b.ctypes.data_as(capi._ip), n.value, C.byref(n)))
        return T, P, l, b

    # ---- device-resident scoring for the benchmark ----
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        capi.check(self.L.stocs_dev_alloc(self.h, nbytes, C.byref(p)))
        return p

    def dev_free(self, p):
        capi.check(self.L.stocs_dev_free(self.h, p))

    def dev_upload(self, p, arr):
        arr = np.ascontiguousarray(arr)
        capi.check(self.L.stocs_dev_upload(self.h, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def dev_download(self, p, arr):
        capi.check(self.L.stocs_dev_download(self.h, arr.ctypes.data_as(C.c_void_p), p, arr.nbytes))

    def score_device(self, dT, n, dL):
        capi.check(self.L.stocs_score_transforms_device(self.h, dT, n, dL))

    def get_scene(self):
        """The scene as the context holds it (stocs_get_scene): centred positions, unit normals, CURRENT class
        probabilities (instance-mode sampling decays them, Q8), pixels."""
        pos = np.zeros((self.nS, 3), np.float32); nrm = np.zeros((self.nS, 3), np.float32)
        prob = np.zeros(self.nS, np.float32); pix = np.zeros((self.nS, 2), np.int32)
        capi.check(self.L.stocs_get_scene(self.h, pos.ctypes.data_as(capi._fp), nrm.ctypes.data_as(capi._fp), prob.ctypes.data_as(capi._fp),
                                          pix.ctypes.data_as(capi._ip)))
        return pos, nrm, prob, pix

    def get_segment(self):
        """`segment` of the last instance-mode attempt (stocs_get_segment): scene indices."""
        n = C.c_int(0)
        capi.check(self.L.stocs_get_segment(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        if n.value:
            capi.check(self.L.stocs_get_segment(self.h, out.ctypes.data_as(capi._ip), n.value, C.byref(n)))
        return out

    def cull_state(self, with_field=True):
        """(patches (n,4), perm (|M|,), geom dict, dist (nz,ny,nx) or None) of the scoring kernels' patch test (diagnostics)."""
        npat = C.c_int(0); nd = C.c_int64(0)
        capi.check(self.L.stocs_get_cull_state(self.h, None, None, C.byref(npat), None, None, 0, C.byref(nd)))
        patches = np.zeros((max(npat.value, 1), 4), np.float32); perm = np.zeros(self.nM, np.int32); geom = np.zeros(8, np.float32)
        dist = np.zeros(max(nd.value, 1), np.float32) if with_field else None
        capi.check(self.L.stocs_get_cull_state(self.h, patches.ctypes.data_as(capi._fp), perm.ctypes.data_as(capi._ip), C.byref(npat), geom.ctypes.data_as(capi._fp),
                                               dist.ctypes.data_as(capi._fp) if with_field else None, nd.value, C.byref(nd)))
        g = dict(origin=geom[:3].copy(), g=float(geom[3]), cap=float(geom[4]), dims=(int(geom[5]), int(geom[6]), int(geom[7])))
        if with_field and nd.value:
            dist = dist[:nd.value].reshape(g["dims"][2], g["dims"][1], g["dims"][0])
        else:
            dist = None
        return patches[:npat.value], perm, g, dist

    def grid_info(self):
        """The scene grid as it was built (stocs_get_grid_info; diagnostics): a dict of the struct's fields, the per-axis ones as
        tuples, origin / h / inv_h as numpy float32."""
        gi = capi.GridInfo()
        capi.check(self.L.stocs_get_grid_info(self.h, C.byref(gi)))
        d = {}
        for name, _ in capi.GridInfo._fields_:
            v = getattr(gi, name)
            d[name] = v
        d["origin"] = np.array(list(gi.origin), np.float32)
        d["h"] = np.float32(gi.h); d["inv_h"] = np.float32(gi.inv_h)
        d["cells"] = tuple(gi.cells); d["bricks"] = tuple(gi.bricks)
        del d["reserved"]
        # the octant lines of the grid (stocs_get_grid_octants): cells with more than a line of entries, those that got octant lines, their entries
        oc = (C.c_int64 * 3)()
        capi.check(self.L.stocs_get_grid_octants(self.h, oc))
        d["long_cells"], d["octant_cells"], d["octant_entries"] = int(oc[0]), int(oc[1]), int(oc[2])
        return d

    def set_option(self, key, value):
        capi.check(self.L.stocs_set_option(self.h, key.encode(), int(value)))

    def last_tie_counts(self):
        """(flagged, changed) of the last scoring call in exact_ties mode: queries the reference-order kd-tree answered, and those
        whose answer differs from the default largest-index rule.  (0, 0) after a default-mode call."""
        f = C.c_int64(0); ch = C.c_int64(0)
        capi.check(self.L.stocs_last_tie_counts(self.h, C.byref(f), C.byref(ch)))
        return int(f.value), int(ch.value)

    def best_device(self, dL, n, id_offset=0):
        """(best_lcp, global id) of n device-resident scores; (0.0, -1) when none is positive."""
        key = C.c_uint64(0)
        capi.check(self.L.stocs_best_device(self.h, dL, n, id_offset, C.byref(key)))
        if key.value == 0:
            return 0.0, -1, 0
        s = C.c_float(0); i = C.c_uint32(0)
        self.L.stocs_unpack_best(key.value, C.byref(s), C.byref(i))
        return s.value, int(i.value), int(key.value)

    def score_best_device(self, dT, n, dL, id_offset=0):
        key = C.c_uint64(0)
        capi.check(self.L.stocs_score_best_device(self.h, dT, n, dL, id_offset, C.byref(key)))
        if key.value == 0:
            return 0.0, -1
        s = C.c_float(0); i = C.c_uint32(0)
        self.L.stocs_unpack_best(key.value, C.byref(s), C.byref(i))
        return s.value, int(i.value)

    def set_stream(self, hip_stream):
        capi.check(self.L.stocs_set_stream(self.h, C.c_void_p(hip_stream)))

    def score_best_device_async(self, dT, n, dL, id_offset, d_key8):
        """Scores + arg-max key in ONE launch (the arg-max is the scoring kernel's epilogue), nothing synchronised."""
        capi.check(self.L.stocs_score_best_device_async(self.h, dT, n, dL, id_offset, C.c_void_p(d_key8)))

    def best_device_async(self, dL, n, id_offset, d_key8):
        capi.check(self.L.stocs_best_device_async(self.h, dL, n, id_offset, C.c_void_p(d_key8)))

    def sync(self):
        capi.check(self.L.stocs_sync(self.h))

    def last_call_timing(self, which):
        """[(step, milliseconds)] of the last find_congruent_all (0), make_transforms (1) or compute_best_transform (2):
        host wall clock between the call's own synchronisation points, always recorded by the library."""
        labels = (C.c_char_p * 18)()   # which = 3: the phases of the last run_trials; 4: the last pose_errors
        ms = (C.c_double * 18)()
        n = C.c_int(0)
        capi.check(self.L.stocs_last_call_timing(self.h, which, labels, ms, 18, C.byref(n)))
        return [(labels[i].decode(), float(ms[i])) for i in range(n.value)]

    def time_score_kernel(self, dT, n, dL, reps):
        ms = C.c_float(0)
        capi.check(self.L.stocs_time_score_kernel(self.h, dT, n, dL, reps, C.byref(ms)))
        return ms.value


def scene_row_words(shape):
    """uint32 words of one pixel row of a frame of shape (height, width) (stocs_scene_row_words)"""
    return int(capi.load().stocs_scene_row_words(int(shape[1]), int(shape[0])))


def select_scene(estimators, poses_per_object, scores_per_object=None, max_per_object=None, labels=False, surface=None, **params):
    """Which hypotheses of several objects form one consistent explanation of the frame: estimators[k] holds object k's model and the
    frame (set_frame, the same size everywhere), poses_per_object[k] its camera-frame hypotheses (m_k, 16).  The pool of pixel rows is
    allocated on the first estimator, every estimator writes its footprints into consecutive slots (group = object index), and the
    first estimator walks the pool (scene_select).  scores_per_object: one score array per object; default
    float32(agree) / float32(footprint), 0 where the footprint is empty -- visible-surface agreement, comparable across objects (LCP is
    not: its weights are per-object class probabilities).  max_per_object: an int or one cap per object.  surface: "points" or "mesh"
    per object (None: all points) -- a "mesh" object's footprints, and its masks under labels=True, come from the mesh of its
    estimator's set_mesh (scene_footprints_mesh, render_poses_mesh, render_resolve_mesh); both kinds share the pool.  params: fields of
    stocs_scene_params, of stocs_render_params, and claim.  -> dict(records, selected, footprints, score, group, index) over the slots
    (group / index: the object and the hypothesis of it a slot holds); with labels=True the selected poses of every object are rendered
    into one key buffer with id = slot (render_poses, render_resolve, render_labels) and the dict also holds render (records of the
    selected, in rank order), labels and state (the class image behind state's on_mask bit is the first estimator's)."""
    if len(estimators) != len(poses_per_object) or not estimators:
        raise ValueError("select_scene: %d estimators for %d pose sets" % (len(estimators), len(poses_per_object)))
    render_keys, scene_keys = dict(capi.RenderParams._fields_), dict(capi.SceneParams._fields_)
    claim = params.pop("claim", "agree")
    rprm = {k: v for k, v in params.items() if k in render_keys}
    sprm = {k: v for k, v in params.items() if k in scene_keys}
    for k in params:
        if k not in render_keys and k not in scene_keys:
            raise TypeError("select_scene: unknown parameter %r" % k)
    surface = ["points"] * len(estimators) if surface is None else list(surface)
    if len(surface) != len(estimators) or any(s not in ("points", "mesh") for s in surface):
        raise ValueError("select_scene: surface is one of 'points' / 'mesh' per object, got %r" % (surface,))
    mprm = {k: v for k, v in rprm.items() if k not in ("point_radius", "max_splat_px")}   # what a mesh reads of them
    first = estimators[0]
    shape = first._frame_shape("select_scene")
    if any(e._frame_shape("select_scene") != shape for e in estimators):
        raise ValueError("select_scene: the estimators' frames differ in size")
    P = [np.ascontiguousarray(p, np.float32).reshape(-1, 16) for p in poses_per_object]
    n = sum(len(p) for p in P)
    group = np.concatenate([np.full(len(p), k, np.int32) for k, p in enumerate(P)])
    index = np.concatenate([np.arange(len(p), dtype=np.int32) for p in P])
    cap = None if max_per_object is None else np.ascontiguousarray(np.broadcast_to(np.asarray(max_per_object, np.int32), (len(P),)))
    out = dict(group=group, index=index)
    rows = first.dev_alloc(max(n, 1) * scene_row_words(shape) * 4)
    zkey = None
    try:
        foot, base = [], 0
        for est, p, kind in zip(estimators, P, surface):
            foot.append(est.scene_footprints_mesh(p, rows, base, n, claim, **mprm) if kind == "mesh" else est.scene_footprints(p, rows, base, n, claim, **rprm))
            base += len(p)
        foot = np.concatenate(foot)
        if scores_per_object is None:
            score = np.zeros(n, np.float32)
            some = foot["footprint"] > 0
            score[some] = foot["agree"][some].astype(np.float32) / foot["footprint"][some].astype(np.float32)
        else:
            score = np.concatenate([np.asarray(s, np.float32).reshape(-1) for s in scores_per_object]).astype(np.float32)
            if score.size != n:
                raise ValueError("select_scene: %d scores for %d hypotheses" % (score.size, n))
        rec, sel = first.scene_select(rows, shape, score, group, foot, cap, n_groups=len(P), **sprm)
        out.update(records=rec, selected=sel, footprints=foot, score=score)
        if labels:
            if len(sel) == 0:
                out.update(render=np.zeros(0, _RENDER_DTYPE), labels=np.full(shape, -1, np.int32), state=np.zeros(shape, np.uint8))
            else:
                zkey = first.dev_alloc(shape[0] * shape[1] * 8)
                for i, s in enumerate(sel.tolist()):
                    if surface[group[s]] == "mesh":
                        estimators[group[s]].render_poses_mesh(P[group[s]][index[s]], zkey, s, i == 0)
                    else:
                        estimators[group[s]].render_poses(P[group[s]][index[s]], zkey, s, i == 0, **rprm)
                out["render"] = np.concatenate([estimators[group[s]].render_resolve_mesh(P[group[s]][index[s]], zkey, s, **mprm) if surface[group[s]] == "mesh"
                                                else estimators[group[s]].render_resolve(P[group[s]][index[s]], zkey, s, **rprm) for s in sel.tolist()])
                out["labels"], out["state"] = first.render_labels(zkey, **rprm)
    finally:
        first.dev_free(rows)
        if zkey is not None:
            first.dev_free(zkey)
    return out


def pose_recall(errors, diameter, k=0.1):
    """Share of the valid records of pose_errors whose ADD, and whose ADD-S, is below k * diameter -> (recall_add, recall_adds, n_valid);
    (nan, nan, 0) when no record is valid.  Invalid records ("no pose") are left out, not counted as misses."""
    errors = np.asarray(errors)
    ok = errors["valid"] != 0
    nv = int(ok.sum())
    if nv == 0:
        return float("nan"), float("nan"), 0
    thr = np.float32(k) * np.float32(diameter)
    return float((errors["add"][ok] < thr).mean()), float((errors["adds"][ok] < thr).mean()), nv


def symmetry_set(sym3, n_continuous=72, center=None):
    """The symmetry transforms that a clustering descriptor stands for (stocs_symmetry_set): sym3 holds 0, 90, 180 or 360 per axis, a
    continuous axis (360) is sampled at n_continuous steps, center is the point the rotations turn about (None: the origin) ->
    (K, 16) float32, column-major 4x4, entry 0 the identity."""
    L = capi.load()
    s3 = (C.c_float * 3)(*[float(x) for x in sym3])
    c3 = None if center is None else (C.c_float * 3)(*[float(x) for x in center])
    K = C.c_int(0)
    rc = L.stocs_symmetry_set(s3, int(n_continuous), c3, None, 0, C.byref(K))    # the count alone: no room is offered
    if K.value < 1:
        capi.check(rc)
    out = np.empty((K.value, 16), np.float32)
    capi.check(L.stocs_symmetry_set(s3, int(n_continuous), c3, out.ctypes.data_as(capi._fp), K.value, C.byref(K)))
    return out


def symmetry_search(**kw):
    """stocs_symmetry_search with its defaults (stocs_default_symmetry_search), fields overridden by keyword"""
    prm = capi.SymmetrySearch()
    capi.load().stocs_default_symmetry_search(C.byref(prm))
    for k, v in kw.items():
        if k not in dict(prm._fields_):
            raise TypeError("symmetry_search: unknown field %r" % k)
        setattr(prm, k, v)
    return prm


def symmetry_axes(n_axes=2048):
    """The candidate directions of the symmetry search (stocs_symmetry_axes) -> (n_axes, 3) float32: x, y, z, then a Fibonacci lattice on
    the hemisphere z > 0."""
    L = capi.load()
    out = np.empty((max(int(n_axes), 1), 3), np.float32)
    n = C.c_int(0)
    capi.check(L.stocs_symmetry_axes(int(n_axes), out.ctypes.data_as(capi._fp), int(n_axes), C.byref(n)))
    return out[:n.value]


def symmetry_rotation(axis, angle_deg, center=None):
    """The rotation by angle_deg about axis through center (stocs_symmetry_rotation; None: the origin) -> 16 float32, column-major"""
    a3 = (C.c_float * 3)(*[float(x) for x in axis])
    c3 = None if center is None else (C.c_float * 3)(*[float(x) for x in center])
    out = np.empty(16, np.float32)
    capi.check(capi.load().stocs_symmetry_rotation(a3, float(angle_deg), c3, out.ctypes.data_as(capi._fp)))
    return out


def symmetry_close(generators, same_deg=1.25, cap=capi.POSE_SYM_MAX):
    """The closure of generators (n, 16) under composition (stocs_symmetry_close) -> ((K, 16) float32 with the identity first, truncated)"""
    G, pG = capi.f32(generators)
    if G.size % 16:
        raise ValueError("symmetry_close: generators are 16 floats each")
    out = np.empty((max(int(cap), 1), 16), np.float32)
    K, tr = C.c_int(0), C.c_int(0)
    capi.check(capi.load().stocs_symmetry_close(pG, G.size // 16, float(same_deg), out.ctypes.data_as(capi._fp), int(cap), C.byref(K), C.byref(tr)))
    return out[:K.value].copy(), bool(tr.value)


BOP_MSSD_THRESHOLDS = tuple(0.05 * i for i in range(1, 11))     # of the diameter
BOP_MSPD_THRESHOLDS = tuple(5.0 * i for i in range(1, 11))      # pixels at an image width of 640


def pose_recall_sym(records, diameter, image_width=None):
    """BOP's average recalls over the valid records of pose_errors_sym -> (ar_mssd, ar_mspd, recall_add, n_valid): the mean over the
    thresholds 0.05, 0.10 .. 0.50 diameters of the share with mssd below the threshold; the mean over 5, 10 .. 50 pixels x
    image_width / 640 of the share with mspd below it (nan without a width); the share with the symmetric add below 0.1 diameter.
    (nan, nan, nan, 0) when no record is valid; invalid records are left out, as in pose_recall."""
    records = np.asarray(records)
    ok = records["valid"] != 0
    nv = int(ok.sum())
    if nv == 0:
        return float("nan"), float("nan"), float("nan"), 0
    d = np.float32(diameter)
    mssd, mspd, add = records["mssd"][ok], records["mspd"][ok], records["add"][ok]
    ar_mssd = float(np.mean([(mssd < np.float32(t) * d).mean() for t in BOP_MSSD_THRESHOLDS]))
    ar_mspd = float("nan")
    if image_width is not None:
        r = np.float32(image_width) / np.float32(640)
        ar_mspd = float(np.mean([(mspd < np.float32(t) * r).mean() for t in BOP_MSPD_THRESHOLDS]))
    return ar_mssd, ar_mspd, float((add < np.float32(0.1) * d).mean()), nv


BOP_VSD_TAUS = tuple(0.05 * i for i in range(1, 11))            # of the diameter: the misalignment tolerances
BOP_VSD_THRESHOLDS = tuple(0.05 * i for i in range(1, 11))      # of 1: the correctness thresholds on the error


def pose_recall_vsd(records, n_tau=None):
    """BOP's average recall of VSD over the records of pose_errors_vsd -> (ar_vsd, n_valid): the mean over the taus (the first n_tau
    entries of `e`; None: 10, the BOP set pose_errors_vsd fills by default) and over the correctness thresholds 0.05, 0.10 .. 0.50 of
    the share of records with e[t] below the threshold.  Unlike pose_recall_sym, which leaves invalid records out, an invalid record
    counts as WRONG here: VSD is defined for it (an estimate that renders nothing has e = 1), so the share is of all records.  (nan, 0)
    for no records."""
    records = np.asarray(records)
    if records.size == 0:
        return float("nan"), 0
    nt = 10 if n_tau is None else int(n_tau)
    if nt < 1 or nt > 16:
        raise ValueError("pose_recall_vsd: n_tau %d outside 1..16" % nt)
    ok = records["valid"].reshape(-1) != 0
    e = records["e"].reshape(-1, 16)[:, :nt]
    hit = [(ok[:, None] & (e < np.float32(th))).mean() for th in BOP_VSD_THRESHOLDS]
    return float(np.mean(hit)), int(ok.sum())


def kdtree_nn_host(pos3, queries3, sqdist):
    """The reference-order kd-tree of the exact_ties option on the host (stocs_kdtree_nn_host): built over pos3 (n, 3), one radius
    query per row of queries3 (q, 3); returns the scene indices (-1: nothing within sqdist)."""
    L = capi.load()
    p, pp = capi.f32(np.asarray(pos3, np.float32).reshape(-1, 3))
    q, pq = capi.f32(np.asarray(queries3, np.float32).reshape(-1, 3))
    out = np.zeros(max(len(q), 1), np.int32)
    capi.check(L.stocs_kdtree_nn_host(pp, len(p), pq, len(q), float(sqdist), out.ctypes.data_as(capi._ip)))
    return out[:len(q)]


def trial_post(acceptable_fraction=0.8, maximum_pose_count=10, min_distance=0.02, min_angle=15.0, sym3=(0.0, 0.0, 0.0), refine_iterations=0,
               max_correspondence_distance=0.035):
    """stocs_trial_post; the defaults are stocs_single's clustering (0.8, 10, 2 cm, 15 degrees, no symmetry) and the reference's ICP distance"""
    return capi.TrialPost(acceptable_fraction, maximum_pose_count, min_distance, min_angle, (C.c_float * 3)(*sym3), refine_iterations,
                          max_correspondence_distance)


def cluster_poses(poses16, lcp, acceptable_fraction, best_score, maximum_pose_count, min_distance, min_angle, sym):
    L = capi.load()
    p, pp = capi.f32(poses16); l, pl = capi.f32(lcp); s, ps = capi.f32(sym)
    out = np.zeros(max(len(l), 1), np.int32)
    n = C.c_int(0)
    capi.check(L.stocs_cluster_poses(pp, pl, len(l), acceptable_fraction, best_score, maximum_pose_count, min_distance,
                                     min_angle, ps, out.ctypes.data_as(capi._ip), len(out), C.byref(n)))
    return out[:n.value]


def ingest_scene(depth_u16, prob_u16, K, depth_scale, voxel_size=0.005, class_threshold=0.10, device=-1, normal_method=0):
    """GPU scene ingest (stocs_ingest_scene): returns pos, nrm, prob, pixel arrays.  normal_method 0: depth-gradient normals (the
    published LINEMOD method, what the reference asks OpenCV for), 1: the 5x5 plane fit of rounds 1-2 (the golden fixtures)."""
    L = capi.load()
    d = np.ascontiguousarray(depth_u16, np.uint16); p = np.ascontiguousarray(prob_u16, np.uint16)
    H, W = d.shape
    cam = capi.Camera(K[0], K[1], K[2], K[3], depth_scale, W, H, normal_method)
    cap = W * H
    pos = np.zeros((cap, 3), np.float32); nrm = np.zeros((cap, 3), np.float32); pr = np.zeros(cap, np.float32); px = np.zeros((cap, 2), np.int32)
    n = C.c_int(0)
    capi.check(L.stocs_ingest_scene(C.byref(cam), d.ctypes.data_as(C.POINTER(C.c_uint16)), p.ctypes.data_as(C.POINTER(C.c_uint16)), voxel_size,
                                    class_threshold, device, pos.ctypes.data_as(capi._fp), nrm.ctypes.data_as(capi._fp), pr.ctypes.data_as(capi._fp),
                                    px.ctypes.data_as(capi._ip), cap, C.byref(n)))
    k = n.value
    return pos[:k].copy(), nrm[:k].copy(), pr[:k].copy(), px[:k].copy()


def ingest_scene_multi(depth_u16, probs_u16, K, depth_scale, voxel_size=0.005, class_thresholds=0.10, device=-1, normal_method=0):
    """Every object of one frame from one GPU ingest (stocs_ingest_scene_multi): probs_u16 holds one class-probability image per object
    (n_objects x H x W, or a list of H x W images), class_thresholds one threshold for all or one per object.  Returns a list of
    (pos, nrm, prob, pixel), one per object, each bit for bit what ingest_scene(depth_u16, probs_u16[k], ..., class_thresholds[k]) returns."""
    L = capi.load()
    d = np.ascontiguousarray(depth_u16, np.uint16)
    H, W = d.shape
    p = np.ascontiguousarray(np.stack([np.asarray(x, np.uint16) for x in probs_u16]) if isinstance(probs_u16, (list, tuple)) else probs_u16, np.uint16)
    n_obj = p.shape[0]
    if p.shape[1:] != (H, W):
        raise ValueError("class-probability images are %s, the depth image %s" % (p.shape[1:], (H, W)))
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(class_thresholds, np.float32), (n_obj,)), np.float32)
    cam = capi.Camera(K[0], K[1], K[2], K[3], depth_scale, W, H, normal_method)
    off = np.zeros(n_obj + 1, np.int32)
    cap = W * H   # one frame's worth of points; grown once when the objects need more
    for attempt in range(2):
        pos = np.zeros((cap, 3), np.float32); nrm = np.zeros((cap, 3), np.float32); pr = np.zeros(cap, np.float32); px = np.zeros((cap, 2), np.int32)
        rc = L.stocs_ingest_scene_multi(C.byref(cam), d.ctypes.data_as(C.POINTER(C.c_uint16)), n_obj, p.ctypes.data_as(C.POINTER(C.c_uint16)),
                                        thr.ctypes.data_as(capi._fp), voxel_size, device, pos.ctypes.data_as(capi._fp), nrm.ctypes.data_as(capi._fp),
                                        pr.ctypes.data_as(capi._fp), px.ctypes.data_as(capi._ip), cap, off.ctypes.data_as(capi._ip))
        if rc == capi.ERR_CAPACITY and attempt == 0:
            cap = int(off[-1])
            continue
        capi.check(rc)
        break
    return [(pos[a:b].copy(), nrm[a:b].copy(), pr[a:b].copy(), px[a:b].copy()) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]


def _params(struct, default_fn, check_fn, kw, what):
    """A parameter struct with the library's defaults and kw on top; `what` names the kind of parameter in the TypeError."""
    p = struct()
    default_fn(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("segment_frame: no %s %r" % (what, k))
        setattr(p, k, v)
    capi.check(check_fn(C.byref(p)))
    return p


def segment_params(**kw):
    """stocs_segment_params with the library's defaults and kw on top; a value outside its range raises (stocs_check_segment_params)."""
    L = capi.load()
    return _params(capi.SegmentParams, L.stocs_default_segment_params, L.stocs_check_segment_params, kw, "parameter")


def segment_convex_params(**kw):
    """stocs_segment_convex_params with the library's defaults and kw on top; a value outside its range raises."""
    L = capi.load()
    return _params(capi.SegmentConvexParams, L.stocs_default_segment_convex_params, L.stocs_check_segment_convex_params, kw, "convex parameter")


def segment_frame(depth_u16, K, depth_scale, device=-1, cap_records=None, images=("class_prob", "labels", "edge"), convex=None, **params):
    """A depth-only frame's class image from its geometry (stocs_segment_frame): the support plane is found and removed, what stands on it
    is split into depth-connected segments.  Returns (result dict, records, images dict): the records as a structured array (root, pixels,
    c0, r0, c1, r1, zmin, zmax), images["class_prob"] (uint16: 10000 in a kept segment, what ingest_scene and set_frame take),
    images["labels"] (int32, 1 .. n_segments) and images["edge"] (uint8, 255 = interior, what set_edge_map takes).  params: the fields of
    stocs_segment_params.  cap_records None: as many as the frame can hold (pixels // min_pixels).  convex: None, or True (the defaults) or a
    dict of the fields of stocs_segment_convex_params: touching objects are cut apart at concave creases before the labelling
    (stocs_segment_frame_convex); the result dict then holds n_tested_h, n_tested_v, n_cut_h, n_cut_v and n_cut too, and `images` may name
    "cut" (uint8: bit 0 horizontal, bit 1 vertical) and "smoothed" (float32, NaN off the foreground)."""
    L = capi.load()
    d = np.ascontiguousarray(depth_u16, np.uint16)
    H, W = d.shape
    p = segment_params(**params)
    cam = capi.Camera(K[0], K[1], K[2], K[3], depth_scale, W, H, 0)
    cap = (W * H) // p.min_pixels if cap_records is None else int(cap_records)
    rec = (capi.SegmentRecord * max(cap, 1))()
    out = capi.SegmentResult()
    with_cut = convex is not None and convex is not False
    kinds = {"class_prob": (np.uint16, C.POINTER(C.c_uint16)), "labels": (np.int32, capi._ip), "edge": (np.uint8, capi._u8p)}
    if with_cut:
        kinds.update({"cut": (np.uint8, capi._u8p), "smoothed": (np.float32, capi._fp)})
    img = {k: np.zeros((H, W), t) for k, (t, _) in kinds.items() if k in images}
    ptr = {k: img[k].ctypes.data_as(t) if k in img else None for k, (_, t) in kinds.items()}
    front = (C.byref(cam), d.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(p))
    back = (rec if cap > 0 else None, cap, C.byref(out))
    res = {}
    if with_cut:
        cp = segment_convex_params(**({} if convex is True else dict(convex)))
        cout = capi.SegmentConvexResult()
        capi.check(L.stocs_segment_frame_convex(*front, C.byref(cp), device, ptr["class_prob"], ptr["labels"], ptr["edge"], ptr["cut"], ptr["smoothed"], *back, C.byref(cout)))
        res = {f: getattr(cout, f) for f, _ in capi.SegmentConvexResult._fields_ if f != "reserved"}
    else:
        capi.check(L.stocs_segment_frame(*front, device, ptr["class_prob"], ptr["labels"], ptr["edge"], *back))
    res = dict({f: getattr(out, f) for f, _ in capi.SegmentResult._fields_ if f not in ("plane", "reserved")}, **res)
    res["plane"] = np.array(list(out.plane), np.float32)
    records = np.frombuffer(rec, dtype=np.dtype([(f, np.float32 if f in ("zmin", "zmax") else np.int32) for f, _ in capi.SegmentRecord._fields_]))[:out.n_segments].copy()
    return res, records, img


def segment_class_images(labels, ids=None):
    """The object-major uint16 stack ingest_scene_multi takes, from a label image: image k is 10000 where labels == ids[k] (ids None: every
    segment 1 .. labels.max(), one image each; an entry of ids may be a list of segment numbers that make up one object)."""
    lab = np.asarray(labels)
    ids = list(range(1, int(lab.max()) + 1)) if ids is None else list(ids)
    out = np.zeros((len(ids),) + lab.shape, np.uint16)
    for k, i in enumerate(ids):
        out[k][np.isin(lab, np.atleast_1d(np.asarray(i)))] = 10000
    return out


def segment_gate_params(**kw):
    """stocs_segment_gate_params with the library's defaults (slack 0.25, min_ratio 0.5, min_used 3: from the geometry of a view, not fitted
    to data) and kw on top; a value outside its range raises."""
    L = capi.load()
    return _params(capi.SegmentGateParams, L.stocs_default_segment_gate_params, L.stocs_check_segment_gate_params, kw, "gate parameter")


def _shape_call(depth_u16, labels, K, depth_scale, n_labels):
    d = np.ascontiguousarray(depth_u16, np.uint16)
    lab = np.ascontiguousarray(labels, np.int32)
    if lab.shape != d.shape or d.ndim != 2:
        raise ValueError("label image %s, depth image %s" % (lab.shape, d.shape))
    n = int(max(int(lab.max()), 0)) if n_labels is None else int(n_labels)
    cam = capi.Camera(K[0], K[1], K[2], K[3], depth_scale, d.shape[1], d.shape[0], 0)
    return d, lab, n, cam


def _shape_counts(res):
    return {f: getattr(res, f) for f, _ in capi.SegmentShapesResult._fields_ if f != "reserved"}


def segment_shapes(depth_u16, labels, K, depth_scale, n_labels=None, max_depth=2.0, device=-1, moments=False):
    """The 3-D shape of every labelled region of a depth frame (stocs_segment_shapes): labels is an int32 image, 0 = none, 1 .. n_labels
    (None: labels.max()), from segment_frame or from anywhere else.  Returns (shapes, counts): shapes a structured array (capi.SHAPE_DTYPE:
    n_used, flags, centroid, eigenvalue, axis, lo, hi, extent), counts the dict of n_labelled, n_used, n_invalid, n_far, n_out_of_range;
    with moments=True the (n_labels, 10) int64 moments as a third value."""
    L = capi.load()
    d, lab, n, cam = _shape_call(depth_u16, labels, K, depth_scale, n_labels)
    shapes = np.zeros(n, capi.SHAPE_DTYPE)
    mom = np.zeros((n, 10), np.int64) if moments else None
    res = capi.SegmentShapesResult()
    capi.check(L.stocs_segment_shapes(C.byref(cam), d.ctypes.data_as(C.POINTER(C.c_uint16)), lab.ctypes.data_as(capi._ip), n, max_depth, device,
                                      shapes.ctypes.data_as(C.POINTER(capi.SegmentShape)) if n else None, mom.ctypes.data_as(capi._i64p) if moments and n else None, C.byref(res)))
    return (shapes, _shape_counts(res), mom) if moments else (shapes, _shape_counts(res))


def points_shape(pos, device=-1, moments=False):
    """The same descriptor for a point cloud (stocs_points_shape), e.g. a preprocessed model: one record of capi.SHAPE_DTYPE."""
    L = capi.load()
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    shape = np.zeros(1, capi.SHAPE_DTYPE)
    mom = np.zeros(10, np.int64)
    capi.check(L.stocs_points_shape(p.ctypes.data_as(capi._fp) if len(p) else None, len(p), device, shape.ctypes.data_as(C.POINTER(capi.SegmentShape)), mom.ctypes.data_as(capi._i64p)))
    return (shape[0], mom) if moments else shape[0]


def object_size(model_pos, diameter=None, device=-1):
    """An object's size for the gate, a record of capi.OBJECT_DTYPE: the extents are points_shape's of the model cloud; the diameter is the
    caller's exact one (StocsEstimator.model_diameter()) or, with None, the diagonal sqrt(m1^2 + m2^2 + m3^2) of the extents, formed in
    double and cast once: an upper bound of the diameter, so the gate's TOO_LARGE stays sound."""
    ext = points_shape(model_pos, device=device)["extent"]
    out = np.zeros((), capi.OBJECT_DTYPE)
    out["extent"] = ext
    out["diameter"] = np.float32(np.sqrt(np.sum(ext.astype(np.float64) ** 2))) if diameter is None else np.float32(diameter)
    return out


def _objects(objects):
    o = np.ascontiguousarray(np.atleast_1d(np.asarray(objects, capi.OBJECT_DTYPE)))
    return o, o.ctypes.data_as(C.POINTER(capi.ObjectSize)) if len(o) else None


def segment_gate(shapes, objects, **gate):
    """The size gate on the host (stocs_segment_gate): the (n_objects, n_labels) uint8 reason bits (capi.GATE_TOO_LARGE, GATE_TOO_SMALL,
    GATE_NO_SHAPE); 0: the segment is compatible with the object.  The gate is not exclusive.  gate: the fields of stocs_segment_gate_params."""
    L = capi.load()
    s = np.ascontiguousarray(np.atleast_1d(np.asarray(shapes, capi.SHAPE_DTYPE)))
    o, op = _objects(objects)
    g = segment_gate_params(**gate)
    reasons = np.zeros((len(o), len(s)), np.uint8)
    capi.check(L.stocs_segment_gate(s.ctypes.data_as(C.POINTER(capi.SegmentShape)) if len(s) else None, len(s), op, len(o), C.byref(g),
                                    reasons.ctypes.data_as(capi._u8p) if reasons.size else None))
    return reasons


def segment_assign(depth_u16, labels, K, depth_scale, objects, n_labels=None, max_depth=2.0, device=-1, **gate):
    """Shapes, the gate and the per-object class images of a labelled depth frame in one call (stocs_segment_assign).  objects: records of
    capi.OBJECT_DTYPE (object_size).  Returns (shapes, reasons, stack, counts): reasons (n_objects, n_labels) uint8, stack the
    (n_objects, H, W) uint16 images that ingest_scene_multi takes, 10000 where the pixel's label is compatible with the object."""
    L = capi.load()
    d, lab, n, cam = _shape_call(depth_u16, labels, K, depth_scale, n_labels)
    o, op = _objects(objects)
    g = segment_gate_params(**gate)
    shapes = np.zeros(n, capi.SHAPE_DTYPE)
    reasons = np.zeros((len(o), n), np.uint8)
    stack = np.zeros((len(o),) + d.shape, np.uint16)
    res = capi.SegmentShapesResult()
    capi.check(L.stocs_segment_assign(C.byref(cam), d.ctypes.data_as(C.POINTER(C.c_uint16)), lab.ctypes.data_as(capi._ip), n, max_depth, op, len(o), C.byref(g), device,
                                      shapes.ctypes.data_as(C.POINTER(capi.SegmentShape)) if n else None, None,
                                      reasons.ctypes.data_as(capi._u8p) if reasons.size else None, stack.ctypes.data_as(C.POINTER(C.c_uint16)) if len(o) else None, C.byref(res)))
    return shapes, reasons, stack, _shape_counts(res)


def segment_shapes_last_device_ms():
    """The kernels' HIP-event time of the calling thread's last segment_shapes / points_shape / segment_assign under STOCS_SEGMENT_CLOCK=1."""
    a = C.c_float(0)
    capi.check(capi.load().stocs_segment_shapes_last_device_ms(C.byref(a)))
    return a.value


def segment_last_device_ms():
    """(score_ms, label_ms) of the calling thread's last segment_frame under STOCS_SEGMENT_CLOCK=1."""
    a, b = C.c_float(0), C.c_float(0)
    capi.check(capi.load().stocs_segment_last_device_ms(C.byref(a), C.byref(b)))
    return a.value, b.value


def segment_last_bend_ms():
    """The bend step's time in the calling thread's last segment_frame(convex=...) under STOCS_SEGMENT_CLOCK=1."""
    a = C.c_float(0)
    capi.check(capi.load().stocs_segment_last_bend_ms(C.byref(a)))
    return a.value


def segment_last_moments():
    """The refit's count and nine int64 moments of the calling thread's last segment_frame."""
    m = np.zeros(10, np.int64)
    capi.check(capi.load().stocs_segment_last_moments(m.ctypes.data_as(capi._i64p)))
    return m


def estimate_objects(scenes, models, seeds, n_attempts=100, mode=0, dispersion=0.9, max_per_base=200, edge_map=None, options=None,
                     params=None, max_workers=4, device=-1, post=None, robust=None):
    """One estimator per object of a frame, run concurrently on a pool of at most max_workers host threads (each context owns its
    streams; the library calls release the GIL).  scenes[k] = (pos, nrm, prob, pixel) -- e.g. from ingest_scene_multi --, models[k] =
    (pos, nrm).  seeds: an int runs one trial (sample_bases, find_congruent_all, make_transforms, compute_best_transform), a sequence
    runs run_trials over it.  edge_map (instance mode) and options (set_option) apply to every object.  Each context is closed when its
    object is done, so at most max_workers hold trial memory at a time.  Returns, in object order, (best_lcp, best_index, best_pose)
    for one trial and run_trials' list of dicts otherwise.  post / robust (a sequence of seeds only): run_trials' arguments of the same
    names; every dict then also carries "hypotheses", the trial's trials_get_hypotheses array (the context is closed on return)."""
    from concurrent.futures import ThreadPoolExecutor
    if len(scenes) != len(models):
        raise ValueError("%d scenes for %d models" % (len(scenes), len(models)))

    def one(k):
        (sp, sn, spr, spx), (mp, mn) = scenes[k], models[k]
        est = StocsEstimator(sp, sn, spr, spx, mp, mn, params=params, build_index=True, device=device)
        try:
            for key, v in (options or {}).items():
                est.set_option(key, v)
            if edge_map is not None:
                est.set_edge_map(edge_map)
            if np.ndim(seeds) == 0:
                est.sample_bases(int(seeds), n_attempts, mode=mode, dispersion=dispersion)
                est.find_congruent_all()
                est.make_transforms(max_per_base, int(seeds))
                lcp, idx, pose = est.compute_best_transform()
                return float(lcp), int(idx), pose
            if post is None and robust is None:
                return est.run_trials(seeds, n_attempts, mode=mode, dispersion=dispersion, max_per_base=max_per_base)
            res = est.run_trials(seeds, n_attempts, mode=mode, dispersion=dispersion, max_per_base=max_per_base, post=post, robust=robust)
            for t, r in enumerate(res):
                r["hypotheses"] = est.trials_get_hypotheses(t)
            return res
        finally:
            est.close()

    with ThreadPoolExecutor(max(1, min(max_workers, len(scenes)))) as ex:
        return list(ex.map(one, range(len(scenes))))


def preprocess_model(raw_pos, normal_radius, voxel_size, model_scale=1.0, device=-1):
    """GPU model preprocessing (stocs_preprocess_model): returns voxelised pos, unit nrm."""
    L = capi.load()
    raw, pr = capi.f32(raw_pos)
    cap = len(raw)
    pos = np.zeros((cap, 3), np.float32); nrm = np.zeros((cap, 3), np.float32)
    n = C.c_int(0)
    capi.check(L.stocs_preprocess_model(pr, len(raw), normal_radius, voxel_size, model_scale, device, pos.ctypes.data_as(capi._fp),
                                        nrm.ctypes.data_as(capi._fp), cap, C.byref(n)))
    return pos[:n.value].copy(), nrm[:n.value].copy()


def mesh_sample_counts(verts, tris, spacing, seed=0, device=-1):
    """The sizes of mesh_sample (stocs_mesh_sample_counts): returns (counts (nt,) int32, area_total, n_total, n_skipped)."""
    L = capi.load()
    v, pv = capi.f32(verts); t, pt = capi.i32(tris)
    counts = np.zeros(len(t), np.int32)
    area, total, skipped = C.c_double(0.0), C.c_int64(0), C.c_int(0)
    capi.check(L.stocs_mesh_sample_counts(pv, len(v), pt, len(t), spacing, int(seed) & (2 ** 64 - 1), device, counts.ctypes.data_as(capi._ip), C.byref(area),
                                          C.byref(total), C.byref(skipped)))
    return counts, area.value, total.value, skipped.value


def mesh_sample(verts, tris, spacing, seed=0, orient=0, device=-1):
    """A triangle mesh sampled at one point per spacing^2 of area (stocs_mesh_sample): returns (pos (n, 3), unit nrm (n, 3), triangle
    index (n,) int32) in (triangle, sample) order.  orient 0: the normal of the winding, 1: turned away from the origin."""
    L = capi.load()
    v, pv = capi.f32(verts); t, pt = capi.i32(tris)
    n = C.c_int(0)
    seed = int(seed) & (2 ** 64 - 1)
    rc = L.stocs_mesh_sample(pv, len(v), pt, len(t), spacing, seed, orient, device, None, None, None, 0, C.byref(n))   # the size
    if rc != capi.ERR_CAPACITY or n.value == 0:   # (a mesh above stocs_mesh_check's limits is a capacity answer too, with no size)
        capi.check(rc)
    cap = n.value
    pos = np.zeros((cap, 3), np.float32); nrm = np.zeros((cap, 3), np.float32); tri = np.zeros(cap, np.int32)
    if cap:
        capi.check(L.stocs_mesh_sample(pv, len(v), pt, len(t), spacing, seed, orient, device, pos.ctypes.data_as(capi._fp), nrm.ctypes.data_as(capi._fp),
                                       tri.ctypes.data_as(capi._ip), cap, C.byref(n)))
    return pos, nrm, tri


def preprocess_model_mesh(verts, tris, voxel_size, spacing=0.0, seed=0, orient=0, model_scale=1.0, device=-1):
    """GPU model preprocessing from a mesh (stocs_preprocess_model_mesh): the surface sampled at `spacing` (0: voxel_size / 4), facet
    normals, voxel grid -> voxelised pos, unit nrm."""
    L = capi.load()
    v, pv = capi.f32(verts); t, pt = capi.i32(tris)
    n = C.c_int(0)
    seed = int(seed) & (2 ** 64 - 1)
    cap = 1 << 16
    for attempt in range(2):
        pos = np.zeros((cap, 3), np.float32); nrm = np.zeros((cap, 3), np.float32)
        rc = L.stocs_preprocess_model_mesh(pv, len(v), pt, len(t), spacing, seed, orient, voxel_size, model_scale, device, pos.ctypes.data_as(capi._fp),
                                           nrm.ctypes.data_as(capi._fp), cap, C.byref(n))
        if rc == capi.ERR_CAPACITY and attempt == 0:
            cap = n.value
            continue
        capi.check(rc)
        break
    return pos[:n.value].copy(), nrm[:n.value].copy()


def icp_point_to_plane(src_pos, tgt_pos, tgt_nrm, max_iterations=5, max_correspondence_distance=0.035, device=-1):
    """GPU point-to-plane ICP (stocs_icp_point_to_plane): returns (T 4x4 float32 source->target, n_correspondences)."""
    L = capi.load()
    s, ps = capi.f32(src_pos); t, pt = capi.f32(tgt_pos); n, pn = capi.f32(tgt_nrm)
    T = np.zeros(16, np.float32)
    nc = C.c_int(0)
    capi.check(L.stocs_icp_point_to_plane(ps, len(s), pt, pn, len(t), max_iterations, max_correspondence_distance, device,
                                          T.ctypes.data_as(capi._fp), C.byref(nc)))
    return T.reshape(4, 4).T.copy(), nc.value
