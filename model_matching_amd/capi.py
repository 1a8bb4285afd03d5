"""ctypes binding of libstocs_hip.so (include/stocs_hip.h).  Fails loudly when the library is
missing -- there is no CPU fallback in the product path."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libstocs_hip.so")

STOCS_OK = 0
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -4, -5
FORM_NAMES = {0: "lean", 1: "full_lds", 2: "full_device_memory", 3: "nine_launch", 4: "instance_lds", 5: "instance_device_memory"}   # STOCS_FORM_* of include/stocs_hip.h
ERR_NAMES = {0: "OK", -1: "INVALID", -2: "NO_DEVICE", -3: "HIP", -4: "CAPACITY", -5: "STATE", -6: "NOMEM"}


class StocsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("stocs_hip error %s: %s" % (ERR_NAMES.get(code, code), msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [("distance_threshold", C.c_float), ("ppf_tr_discretization", C.c_int),
                ("ppf_rot_discretization", C.c_int), ("plane_threshold", C.c_float),
                ("min_distance_base", C.c_float), ("internal_angle_threshold", C.c_float),
                ("lcp_normal_angle", C.c_float), ("image_width", C.c_int), ("image_height", C.c_int),
                ("number_of_bases", C.c_int), ("maximum_congruent_sets", C.c_int)]


class TrialResult(C.Structure):
    _fields_ = [("n_bases", C.c_int32), ("n_candidates", C.c_int32), ("n_quads", C.c_int64), ("best_lcp", C.c_float), ("best_index", C.c_int32),
                ("best_pose16", C.c_float * 16)]


class TrialPost(C.Structure):
    _fields_ = [("acceptable_fraction", C.c_float), ("maximum_pose_count", C.c_int32), ("min_distance", C.c_float), ("min_angle", C.c_float),
                ("sym3", C.c_float * 3), ("refine_iterations", C.c_int32), ("max_correspondence_distance", C.c_float)]


class TrialHypothesis(C.Structure):
    _fields_ = [("candidate_index", C.c_int32), ("base_index", C.c_int32), ("lcp", C.c_float), ("pose16", C.c_float * 16),
                ("refined_lcp", C.c_float), ("refined_pose16", C.c_float * 16), ("n_correspondences", C.c_int32), ("iterations", C.c_int32)]


class TrackParams(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("samples", C.c_int32), ("max_translation", C.c_float), ("max_rotation_deg", C.c_float), ("shrink", C.c_float),
                ("seed", C.c_uint64), ("refine_iterations", C.c_int32), ("max_correspondence_distance", C.c_float), ("keep_details", C.c_int32)]


class TrackResult(C.Structure):
    _fields_ = [("prior_lcp", C.c_float), ("lcp", C.c_float), ("pose16", C.c_float * 16), ("refined_lcp", C.c_float), ("refined_pose16", C.c_float * 16),
                ("n_correspondences", C.c_int32), ("iterations", C.c_int32)]


class RefineRobustParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("max_correspondence_distance", C.c_float), ("keep_ratio", C.c_float), ("min_normal_cos", C.c_float)]


class DepthParams(C.Structure):
    _fields_ = [("tolerance", C.c_float), ("class_threshold", C.c_float), ("self_occlusion", C.c_int32), ("cell_px", C.c_int32),
                ("occlusion_margin", C.c_float)]


class DepthResult(C.Structure):
    _fields_ = [("facing", C.c_int32), ("in_image", C.c_int32), ("self_occluded", C.c_int32), ("no_depth", C.c_int32), ("agree", C.c_int32),
                ("in_front", C.c_int32), ("behind", C.c_int32), ("on_mask", C.c_int32), ("score", C.c_float), ("violation", C.c_float)]


class PoseError(C.Structure):
    _fields_ = [("add_fix", C.c_uint64), ("adds_fix", C.c_uint64), ("add", C.c_float), ("add_max", C.c_float), ("adds", C.c_float),
                ("adds_max", C.c_float), ("valid", C.c_int32), ("reserved", C.c_int32)]


class PoseErrorSym(C.Structure):
    _fields_ = [("add_fix", C.c_uint64), ("add", C.c_float), ("mssd", C.c_float), ("mspd", C.c_float), ("reserved_f", C.c_float),
                ("k_add", C.c_int32), ("k_mssd", C.c_int32), ("k_mspd", C.c_int32), ("valid", C.c_int32)]


class SymmetryParams(C.Structure):
    _fields_ = [("reach", C.c_float), ("cos_normal", C.c_float), ("reserved", C.c_int32 * 2)]


class SymmetryError(C.Structure):
    _fields_ = [("sum_fix", C.c_uint64), ("mean", C.c_float), ("max", C.c_float), ("n_far", C.c_int32), ("n_normal_bad", C.c_int32),
                ("valid", C.c_int32), ("reserved", C.c_int32)]


class SymmetrySearch(C.Structure):
    _fields_ = [("tol_max", C.c_float), ("cos_normal", C.c_float), ("max_normal_bad", C.c_float), ("n_axes", C.c_int32), ("max_order", C.c_int32),
                ("n_continuous", C.c_int32), ("n_refine", C.c_int32), ("n_local", C.c_int32), ("rounds", C.c_int32), ("same_deg", C.c_float)]


class SymmetryAxis(C.Structure):
    _fields_ = [("axis", C.c_float * 3), ("order", C.c_int32), ("max", C.c_float), ("mean", C.c_float), ("n_normal_bad", C.c_int32),
                ("reserved", C.c_int32)]


SYMMETRY_DESCRIPTOR_INEXACT, SYMMETRY_SET_TRUNCATED, SYMMETRY_NOTHING_FOUND = 1, 2, 4
POSE_SYM_MAX = 4096


class InstanceParams(C.Structure):
    _fields_ = [("max_instances", C.c_int32), ("min_points", C.c_int32), ("min_exclusive_fraction", C.c_float)]


class InstanceResult(C.Structure):
    _fields_ = [("rank", C.c_int32), ("own", C.c_int32), ("exclusive", C.c_int32), ("lcp", C.c_float)]


class RenderParams(C.Structure):
    _fields_ = [("point_radius", C.c_float), ("max_splat_px", C.c_int32), ("tolerance", C.c_float), ("class_threshold", C.c_float)]


class VsdParams(C.Structure):
    _fields_ = [("surfel_radius", C.c_float), ("max_splat_px", C.c_int32), ("delta", C.c_float), ("n_tau", C.c_int32), ("tau", C.c_float * 16)]


class VsdRecord(C.Structure):
    _fields_ = [("px_est", C.c_int32), ("px_gt", C.c_int32), ("vis_est", C.c_int32), ("vis_gt", C.c_int32), ("inter", C.c_int32), ("uni", C.c_int32),
                ("far", C.c_int32 * 16), ("e", C.c_float * 16), ("valid", C.c_int32), ("reserved", C.c_int32)]


class RenderResult(C.Structure):
    _fields_ = [("footprint", C.c_int32), ("visible", C.c_int32), ("hidden", C.c_int32), ("no_depth", C.c_int32), ("agree", C.c_int32),
                ("in_front", C.c_int32), ("behind", C.c_int32), ("on_mask", C.c_int32)]


class RefineVisibleParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("max_distance", C.c_float), ("min_view_cos", C.c_float), ("class_threshold", C.c_float)]


class RefineVisibleResult(C.Structure):
    _fields_ = [("present", C.c_int32), ("no_depth", C.c_int32), ("off_class", C.c_int32), ("too_far", C.c_int32), ("grazing", C.c_int32),
                ("counted", C.c_int32), ("iterations", C.c_int32), ("frozen", C.c_int32), ("rms", C.c_float), ("reserved", C.c_int32)]


class RefineVisibleDampedParams(C.Structure):
    _fields_ = [("base", RefineVisibleParams), ("lambda0", C.c_float), ("lambda_down", C.c_float), ("lambda_up", C.c_float),
                ("max_step_rotation", C.c_float), ("max_step_translation", C.c_float), ("pivot", C.c_int32), ("pivot_model", C.c_float * 3)]


class RefineVisibleDampedResult(C.Structure):
    _fields_ = [("base", RefineVisibleResult), ("evaluations", C.c_int32), ("rejected", C.c_int32), ("cost", C.c_float), ("lambda_", C.c_float)]


class RefineVisibleTrace(C.Structure):
    _fields_ = [("pose", C.c_float * 16), ("cost", C.c_double), ("lambda_", C.c_double), ("accepted", C.c_int32), ("state", C.c_int32)]


class RefineVisibleContourParams(C.Structure):
    _fields_ = [("damped", RefineVisibleDampedParams), ("contour_weight", C.c_float), ("pull_radius_px", C.c_int32), ("pull_distance", C.c_float)]


class RefineVisibleContourResult(C.Structure):
    _fields_ = [("damped", RefineVisibleDampedResult), ("object_px", C.c_int32), ("uncovered", C.c_int32), ("unreached", C.c_int32), ("beyond", C.c_int32),
                ("pulled", C.c_int32), ("pull_rms", C.c_float)]


class SegmentParams(C.Structure):
    _fields_ = [("max_depth", C.c_float), ("plane_hypotheses", C.c_int32), ("score_stride", C.c_int32), ("plane_tolerance", C.c_float),
                ("plane_min_share", C.c_float), ("max_height", C.c_float), ("jump_abs", C.c_float), ("jump_rel", C.c_float), ("min_pixels", C.c_int32),
                ("seed", C.c_uint64)]


class SegmentResult(C.Structure):
    _fields_ = [("plane", C.c_float * 4), ("plane_found", C.c_int32), ("winner", C.c_int32), ("winner_count", C.c_int32), ("n_valid", C.c_int32),
                ("n_scored", C.c_int32), ("n_refit", C.c_int32), ("n_on_plane", C.c_int32), ("n_above", C.c_int32), ("n_below", C.c_int32),
                ("n_components", C.c_int32), ("n_segments", C.c_int32), ("reserved", C.c_int32)]


class SegmentRecord(C.Structure):
    _fields_ = [("root", C.c_int32), ("pixels", C.c_int32), ("c0", C.c_int32), ("r0", C.c_int32), ("c1", C.c_int32), ("r1", C.c_int32),
                ("zmin", C.c_float), ("zmax", C.c_float)]


class SegmentConvexParams(C.Structure):
    _fields_ = [("bend_radius", C.c_int32), ("smooth_radius", C.c_int32), ("bend_cos", C.c_float), ("reserved", C.c_int32)]


class SegmentConvexResult(C.Structure):
    _fields_ = [("n_tested_h", C.c_int32), ("n_tested_v", C.c_int32), ("n_cut_h", C.c_int32), ("n_cut_v", C.c_int32), ("n_cut", C.c_int32),
                ("reserved", C.c_int32 * 3)]


SHAPE_EMPTY, SHAPE_NONFINITE = 1, 2
GATE_TOO_LARGE, GATE_TOO_SMALL, GATE_NO_SHAPE = 1, 2, 4
MAX_FRAME_OBJECTS = 64


class SegmentShape(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("flags", C.c_int32), ("centroid", C.c_float * 3), ("eigenvalue", C.c_float * 3), ("axis", (C.c_float * 3) * 3),
                ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("extent", C.c_float * 3), ("reserved", C.c_int32 * 6)]


SHAPE_DTYPE = np.dtype([("n_used", np.int32), ("flags", np.int32), ("centroid", np.float32, (3,)), ("eigenvalue", np.float32, (3,)), ("axis", np.float32, (3, 3)),
                        ("lo", np.float32, (3,)), ("hi", np.float32, (3,)), ("extent", np.float32, (3,)), ("reserved", np.int32, (6,))])


class SegmentShapesResult(C.Structure):
    _fields_ = [("n_labelled", C.c_int32), ("n_used", C.c_int32), ("n_invalid", C.c_int32), ("n_far", C.c_int32), ("n_out_of_range", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class ObjectSize(C.Structure):
    _fields_ = [("diameter", C.c_float), ("extent", C.c_float * 3)]


OBJECT_DTYPE = np.dtype([("diameter", np.float32), ("extent", np.float32, (3,))])


class SegmentGateParams(C.Structure):
    _fields_ = [("slack", C.c_float), ("min_ratio", C.c_float), ("min_used", C.c_int32), ("reserved", C.c_int32)]


class SceneRecord(C.Structure):
    _fields_ = [("footprint", C.c_int32), ("no_depth", C.c_int32), ("agree", C.c_int32), ("in_front", C.c_int32), ("behind", C.c_int32),
                ("on_mask", C.c_int32), ("claimed", C.c_int32)]


class SceneParams(C.Structure):
    _fields_ = [("max_selected", C.c_int32), ("min_pixels", C.c_int32), ("min_exclusive_fraction", C.c_float), ("max_violation_fraction", C.c_float)]


class SceneResult(C.Structure):
    _fields_ = [("rank", C.c_int32), ("own", C.c_int32), ("exclusive", C.c_int32), ("reason", C.c_int32)]


GRID_SORT_ROCPRIM, GRID_SORT_OWN = 1, 2


class GridInfo(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("h", C.c_float), ("inv_h", C.c_float), ("div", C.c_int32), ("cells", C.c_int32 * 3),
                ("bricks", C.c_int32 * 3), ("centre_sorted", C.c_int32), ("pruned", C.c_int32), ("has_nearest", C.c_int32),
                ("has_cones", C.c_int32), ("has_flat", C.c_int32), ("sort", C.c_int32), ("prune_group", C.c_int32), ("prune_k", C.c_int32),
                ("longest_list", C.c_int32), ("reserved", C.c_int32), ("n_incidences", C.c_int64), ("n_cells", C.c_int64),
                ("n_bricks", C.c_int64), ("n_entries", C.c_int64)]


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("cx", C.c_float), ("fy", C.c_float), ("cy", C.c_float), ("depth_scale", C.c_float),
                ("width", C.c_int), ("height", C.c_int), ("normal_method", C.c_int)]


# name -> (restype, argtypes); every symbol declared in include/stocs_hip.h
_fp, _ip, _u8p, _vp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_void_p
_i64p = C.POINTER(C.c_int64)
_intp = C.POINTER(C.c_int)
SIGNATURES = {
    "stocs_default_params": (None, [C.POINTER(Params)]),
    "stocs_last_error": (C.c_char_p, []),
    "stocs_version": (C.c_char_p, []),
    "stocs_ctx_create": (C.c_int, [C.POINTER(Params), _fp, _fp, _fp, _ip, C.c_int, _fp, _fp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "stocs_ctx_destroy": (C.c_int, [_vp]),
    "stocs_ctx_set_scene": (C.c_int, [_vp, _fp, _fp, _fp, _ip, C.c_int]),
    "stocs_get_centroids": (C.c_int, [_vp, _fp, _fp]),
    "stocs_get_sizes": (C.c_int, [_vp, _intp, _intp]),
    "stocs_set_edge_map": (C.c_int, [_vp, _u8p]),
    "stocs_reset_trial": (C.c_int, [_vp]),
    "stocs_ppf_compute_host": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int, C.c_int, _ip]),
    "stocs_index_exists": (C.c_int, [_vp, _ip, _intp]),
    "stocs_index_lookup": (C.c_int, [_vp, _ip, _ip, C.c_int64, _i64p]),
    "stocs_index_stats": (C.c_int, [_vp, _i64p, _i64p, _i64p]),
    "stocs_index_save": (C.c_int, [_vp, C.c_char_p]),
    "stocs_index_load": (C.c_int, [_vp, C.c_char_p]),
    "stocs_sample_bases": (C.c_int, [_vp, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_float, _ip, _fp, _ip]),
    "stocs_get_segment": (C.c_int, [_vp, _ip, C.c_int, _intp]),
    "stocs_get_scene": (C.c_int, [_vp, _fp, _fp, _fp, _ip]),
    "stocs_png_read": (C.c_int, [C.c_char_p, _intp, _intp, _intp, _intp, _vp, C.c_int64]),
    "stocs_ply_read": (C.c_int, [C.c_char_p, _fp, _fp, C.c_int, _intp, _intp]),
    "stocs_ply_write": (C.c_int, [C.c_char_p, _fp, _fp, C.c_int, C.c_float]),
    "stocs_ply_read_mesh": (C.c_int, [C.c_char_p, _fp, C.c_int, _intp, _ip, C.c_int, _intp]),
    "stocs_ply_write_mesh": (C.c_int, [C.c_char_p, _fp, C.c_int, _ip, C.c_int]),
    "stocs_set_bases": (C.c_int, [_vp, C.c_int, _ip, _fp]),
    "stocs_clear_bases": (C.c_int, [_vp]),
    "stocs_num_bases": (C.c_int, [_vp]),
    "stocs_class_pass": (C.c_int, [_vp, C.c_int, _ip, _fp, _fp]),
    "stocs_ppf_filter_check": (C.c_int, [_vp, C.c_uint64, C.c_int64, _i64p, _i64p, _i64p]),
    "stocs_weight_fix_check": (C.c_int, [_vp, _i64p]),
    "stocs_try_sampled_base": (C.c_int, [_vp, _ip, _fp, _intp]),
    "stocs_draw": (C.c_int, [_vp, _fp, C.c_int, C.c_uint64, _intp]),
    "stocs_last_sampling_form": (C.c_int, [_vp, _intp, _intp, _i64p, _intp, _intp, _intp]),
    "stocs_last_instance_attempts": (C.c_int, [_vp, _ip, C.c_int, _intp]),
    "stocs_debug_draw_point1": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.c_int, _ip]),
    "stocs_find_congruent_all": (C.c_int, [_vp, _i64p]),
    "stocs_get_quads": (C.c_int, [_vp, C.c_int, _ip, C.c_int64, _i64p]),
    "stocs_get_quads_at": (C.c_int, [_vp, C.c_int, _i64p, C.c_int, _ip]),
    "stocs_cone_cells_host": (C.c_int, [_fp, C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _intp, _intp]),
    "stocs_cone_cells_device": (C.c_int, [C.c_int, _fp, _fp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _ip, _ip, _fp, _ip, _ip, _fp]),
    "stocs_make_transforms": (C.c_int, [_vp, C.c_int, C.c_uint64, _intp]),
    "stocs_rigid_transform": (C.c_int, [_vp, _ip, _ip, _fp, _fp, _intp]),
    "stocs_get_candidates": (C.c_int, [_vp, _fp, _fp, _fp, _ip, C.c_int, _intp]),
    "stocs_score_transforms": (C.c_int, [_vp, _fp, C.c_int, _fp]),
    "stocs_score_transforms_device": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "stocs_score_best_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_uint32, C.POINTER(C.c_uint64)]),
    "stocs_lcp_detail": (C.c_int, [_vp, _fp, _ip, _u8p]),
    "stocs_lcp_hit_count": (C.c_int, [_vp, _vp, C.c_int, _i64p, _i64p]),
    "stocs_lcp_gate_count": (C.c_int, [_vp, _vp, C.c_int, _i64p]),
    "stocs_verify_all": (C.c_int, [_vp, _fp, _intp, _fp]),
    "stocs_run_trials": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_int, C.c_float, C.c_int, C.c_int, C.POINTER(TrialResult)]),
    "stocs_trials_get_bases": (C.c_int, [_vp, C.c_int, _ip, _fp, _ip, C.c_int, _intp]),
    "stocs_trials_get_quad_counts": (C.c_int, [_vp, C.c_int, _i64p, C.c_int, _intp]),
    "stocs_trials_get_candidates": (C.c_int, [_vp, C.c_int, _fp, _fp, _fp, _ip, C.c_int, _intp]),
    "stocs_run_trials_post": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_int, C.c_float, C.c_int, C.c_int, C.POINTER(TrialPost),
                                        C.POINTER(TrialResult)]),
    "stocs_run_trials_post_robust": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_int, C.c_float, C.c_int, C.c_int, C.POINTER(TrialPost),
                                               C.c_float, C.c_float, C.POINTER(TrialResult)]),
    "stocs_trials_get_hypotheses": (C.c_int, [_vp, C.c_int, C.POINTER(TrialHypothesis), C.c_int, _intp]),
    "stocs_best_device": (C.c_int, [_vp, _vp, C.c_int, C.c_uint32, C.POINTER(C.c_uint64)]),
    "stocs_pack_best": (C.c_uint64, [C.c_float, C.c_uint32]),
    "stocs_unpack_best": (None, [C.c_uint64, _fp, C.POINTER(C.c_uint32)]),
    "stocs_comm_unique_id": (C.c_int, [_vp]),
    "stocs_comm_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "stocs_comm_destroy": (C.c_int, [_vp]),
    "stocs_allreduce_best": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint64), _fp, C.c_uint32]),
    "stocs_cluster_poses": (C.c_int, [_fp, _fp, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, _fp, _ip, C.c_int, _intp]),
    "stocs_cluster_trials_device": (C.c_int, [_vp, _fp, _fp, _ip, _fp, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, _fp, _ip, _ip, _ip, C.c_int, _ip]),
    "stocs_ingest_scene": (C.c_int, [C.POINTER(Camera), C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.c_float, C.c_float, C.c_int, _fp, _fp, _fp, _ip, C.c_int, _intp]),
    "stocs_ingest_scene_multi": (C.c_int, [C.POINTER(Camera), C.POINTER(C.c_uint16), C.c_int, C.POINTER(C.c_uint16), _fp, C.c_float, C.c_int, _fp, _fp, _fp, _ip,
                                           C.c_int, _ip]),
    "stocs_preprocess_model": (C.c_int, [_fp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, _fp, _fp, C.c_int, _intp]),
    "stocs_trim": (C.c_int, []),
    "stocs_default_segment_params": (None, [C.POINTER(SegmentParams)]),
    "stocs_check_segment_params": (C.c_int, [C.POINTER(SegmentParams)]),
    "stocs_segment_frame": (C.c_int, [C.POINTER(Camera), C.POINTER(C.c_uint16), C.POINTER(SegmentParams), C.c_int, C.POINTER(C.c_uint16), _ip, _u8p,
                                      C.POINTER(SegmentRecord), C.c_int, C.POINTER(SegmentResult)]),
    "stocs_segment_tile": (C.c_int, [_intp, _intp]),
    "stocs_segment_last_device_ms": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "stocs_segment_last_moments": (C.c_int, [_i64p]),
    "stocs_default_segment_convex_params": (None, [C.POINTER(SegmentConvexParams)]),
    "stocs_check_segment_convex_params": (C.c_int, [C.POINTER(SegmentConvexParams)]),
    "stocs_segment_frame_convex": (C.c_int, [C.POINTER(Camera), C.POINTER(C.c_uint16), C.POINTER(SegmentParams), C.POINTER(SegmentConvexParams), C.c_int,
                                             C.POINTER(C.c_uint16), _ip, _u8p, _u8p, _fp, C.POINTER(SegmentRecord), C.c_int, C.POINTER(SegmentResult),
                                             C.POINTER(SegmentConvexResult)]),
    "stocs_segment_last_bend_ms": (C.c_int, [C.POINTER(C.c_float)]),
    "stocs_default_segment_gate_params": (None, [C.POINTER(SegmentGateParams)]),
    "stocs_check_segment_gate_params": (C.c_int, [C.POINTER(SegmentGateParams)]),
    "stocs_segment_gate": (C.c_int, [C.POINTER(SegmentShape), C.c_int, C.POINTER(ObjectSize), C.c_int, C.POINTER(SegmentGateParams), _u8p]),
    "stocs_segment_shapes": (C.c_int, [C.POINTER(Camera), C.POINTER(C.c_uint16), _ip, C.c_int, C.c_float, C.c_int, C.POINTER(SegmentShape), _i64p,
                                       C.POINTER(SegmentShapesResult)]),
    "stocs_points_shape": (C.c_int, [_fp, C.c_int, C.c_int, C.POINTER(SegmentShape), _i64p]),
    "stocs_segment_assign": (C.c_int, [C.POINTER(Camera), C.POINTER(C.c_uint16), _ip, C.c_int, C.c_float, C.POINTER(ObjectSize), C.c_int, C.POINTER(SegmentGateParams),
                                       C.c_int, C.POINTER(SegmentShape), _i64p, _u8p, C.POINTER(C.c_uint16), C.POINTER(SegmentShapesResult)]),
    "stocs_segment_shapes_table": (C.c_int, [_intp]),
    "stocs_segment_shapes_last_device_ms": (C.c_int, [C.POINTER(C.c_float)]),
    "stocs_icp_point_to_plane": (C.c_int, [_fp, C.c_int, _fp, _fp, C.c_int, C.c_int, C.c_float, C.c_int, _fp, _intp]),
    "stocs_refine_poses": (C.c_int, [_vp, _fp, C.c_int, _ip, C.c_int, C.c_int, C.c_float, _fp, _fp, _fp, _ip, _ip]),
    "stocs_refine_detail": (C.c_int, [_vp, _fp, _ip, C.c_int, C.c_float, _ip, _u8p, C.POINTER(C.c_double)]),
    "stocs_refine_poses_robust": (C.c_int, [_vp, _fp, C.c_int, _ip, C.c_int, C.POINTER(RefineRobustParams), _fp, _fp, _fp, _ip, _ip, _ip]),
    "stocs_refine_robust_detail": (C.c_int, [_vp, _fp, _ip, C.c_int, C.POINTER(RefineRobustParams), _ip, _u8p, _u8p, C.POINTER(C.c_uint32), _ip, _ip,
                                             C.POINTER(C.c_double)]),
    "stocs_refine_robust_workspace": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "stocs_track_poses": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(TrackParams), C.POINTER(TrackResult)]),
    "stocs_track_poses_robust": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(TrackParams), C.c_float, C.c_float, C.POINTER(TrackResult)]),
    "stocs_track_get_round": (C.c_int, [_vp, C.c_int, C.c_int, _fp, _fp, C.c_int, _intp]),
    "stocs_ctx_set_frame": (C.c_int, [_vp, C.POINTER(Camera), C.POINTER(C.c_uint16), C.POINTER(C.c_uint16)]),
    "stocs_default_depth_params": (None, [C.POINTER(DepthParams)]),
    "stocs_depth_check_poses": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(DepthParams), C.POINTER(DepthResult)]),
    "stocs_default_vsd_params": (None, [C.POINTER(VsdParams)]),
    "stocs_check_vsd_params": (C.c_int, [C.POINTER(VsdParams)]),
    "stocs_render_depth": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(VsdParams), _fp]),
    "stocs_pose_errors_vsd": (C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, C.POINTER(VsdParams), C.POINTER(VsdRecord)]),
    "stocs_mesh_small_px": (C.c_int, []),
    "stocs_mesh_check": (C.c_int, [_fp, C.c_int, _ip, C.c_int]),
    "stocs_ctx_set_mesh": (C.c_int, [_vp, _fp, C.c_int, _ip, C.c_int]),
    "stocs_ctx_mesh_info": (C.c_int, [_vp, _intp, _intp]),
    "stocs_render_depth_mesh": (C.c_int, [_vp, _fp, C.c_int, _fp]),
    "stocs_pose_errors_vsd_mesh": (C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, C.POINTER(VsdParams), C.POINTER(VsdRecord)]),
    "stocs_mesh_last_call_timing": (C.c_int, [_vp, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_int, _intp]),
    "stocs_render_poses_mesh": (C.c_int, [_vp, _fp, C.c_int, C.c_int, _vp, C.c_int]),
    "stocs_render_resolve_mesh": (C.c_int, [_vp, _fp, C.c_int, C.c_int, C.POINTER(RenderParams), _vp, C.POINTER(RenderResult)]),
    "stocs_explain_poses_mesh": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(RenderParams), C.POINTER(RenderResult), _ip, _u8p]),
    "stocs_scene_footprints_mesh": (C.c_int, [_vp, _fp, C.c_int, C.c_int, C.c_int, C.POINTER(RenderParams), C.c_int, _vp, C.POINTER(SceneRecord)]),
    "stocs_render_mesh_last_device_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "stocs_default_refine_visible_params": (None, [C.POINTER(RefineVisibleParams)]),
    "stocs_check_refine_visible_params": (C.c_int, [C.POINTER(RefineVisibleParams)]),
    "stocs_refine_visible_groups": (C.c_int, [C.c_int, C.c_int]),
    "stocs_refine_poses_visible": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(RefineVisibleParams), _fp, C.POINTER(RefineVisibleResult)]),
    "stocs_refine_visible_detail": (C.c_int, [_vp, _fp, C.POINTER(RefineVisibleParams), C.POINTER(C.c_uint64), _u8p, C.POINTER(C.c_double)]),
    "stocs_refine_visible_last_device_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "stocs_default_refine_visible_damped_params": (None, [C.POINTER(RefineVisibleDampedParams)]),
    "stocs_check_refine_visible_damped_params": (C.c_int, [C.POINTER(RefineVisibleDampedParams)]),
    "stocs_refine_poses_visible_damped": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(RefineVisibleDampedParams), _fp, C.POINTER(RefineVisibleDampedResult),
                                                    C.POINTER(RefineVisibleTrace)]),
    "stocs_default_refine_visible_contour_params": (None, [C.POINTER(RefineVisibleContourParams)]),
    "stocs_check_refine_visible_contour_params": (C.c_int, [C.POINTER(RefineVisibleContourParams)]),
    "stocs_refine_poses_visible_contour": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(RefineVisibleContourParams), _fp, C.POINTER(RefineVisibleContourResult),
                                                     C.POINTER(RefineVisibleTrace)]),
    "stocs_refine_visible_contour_detail": (C.c_int, [_vp, _fp, C.POINTER(RefineVisibleContourParams), _u8p, _ip, C.POINTER(C.c_double)]),
    "stocs_refine_visible_contour_last_device_ms": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "stocs_mesh_sample_counts": (C.c_int, [_fp, C.c_int, _ip, C.c_int, C.c_float, C.c_uint64, C.c_int, _ip, C.POINTER(C.c_double), _i64p, _intp]),
    "stocs_mesh_sample": (C.c_int, [_fp, C.c_int, _ip, C.c_int, C.c_float, C.c_uint64, C.c_int, C.c_int, _fp, _fp, _ip, C.c_int, _intp]),
    "stocs_preprocess_model_mesh": (C.c_int, [_fp, C.c_int, _ip, C.c_int, C.c_float, C.c_uint64, C.c_int, C.c_float, C.c_float, C.c_int, _fp, _fp, C.c_int, _intp]),
    "stocs_pose_errors": (C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, C.POINTER(PoseError)]),
    "stocs_pose_errors_detail": (C.c_int, [_vp, _fp, _fp, _fp, _fp, _ip]),
    "stocs_model_diameter": (C.c_int, [_vp, _fp]),
    "stocs_pose_errors_sym": (C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, C.POINTER(Camera), C.POINTER(PoseErrorSym)]),
    "stocs_pose_errors_sym_detail": (C.c_int, [_vp, _fp, _fp, _fp, C.c_int, C.POINTER(Camera), C.POINTER(C.c_uint64), _fp, _fp]),
    "stocs_symmetry_set": (C.c_int, [_fp, C.c_int, _fp, _fp, C.c_int, _intp]),
    "stocs_symmetry_errors": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(SymmetryParams), C.POINTER(SymmetryError)]),
    "stocs_symmetry_errors_detail": (C.c_int, [_vp, _fp, C.POINTER(SymmetryParams), _fp, _ip, _fp]),
    "stocs_symmetry_axes": (C.c_int, [C.c_int, _fp, C.c_int, _intp]),
    "stocs_symmetry_rotation": (C.c_int, [_fp, C.c_double, _fp, _fp]),
    "stocs_symmetry_close": (C.c_int, [_fp, C.c_int, C.c_float, _fp, C.c_int, _intp, _intp]),
    "stocs_default_symmetry_search": (None, [C.POINTER(SymmetrySearch)]),
    "stocs_find_symmetries": (C.c_int, [_vp, C.POINTER(SymmetrySearch), _fp, C.POINTER(SymmetryAxis), C.c_int, _intp, _fp, C.c_int, _intp, _fp, _intp]),
    "stocs_default_render_params": (None, [C.POINTER(RenderParams)]),
    "stocs_render_poses": (C.c_int, [_vp, _fp, C.c_int, C.c_int, C.POINTER(RenderParams), _vp, C.c_int]),
    "stocs_render_resolve": (C.c_int, [_vp, _fp, C.c_int, C.c_int, C.POINTER(RenderParams), _vp, C.POINTER(RenderResult)]),
    "stocs_render_labels": (C.c_int, [_vp, _vp, C.POINTER(RenderParams), _ip, _u8p]),
    "stocs_explain_poses": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(RenderParams), C.POINTER(RenderResult), _ip, _u8p]),
    "stocs_default_instance_params": (None, [C.POINTER(InstanceParams)]),
    "stocs_select_instances": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(InstanceParams), C.POINTER(InstanceResult), _ip, _intp]),
    "stocs_select_instances_rows": (C.c_int, [_vp, _ip, _u8p, _fp, C.c_int, C.c_int, C.c_int, C.POINTER(InstanceParams), C.POINTER(InstanceResult), _ip, _intp]),
    "stocs_default_scene_params": (None, [C.POINTER(SceneParams)]),
    "stocs_scene_row_words": (C.c_int, [C.c_int, C.c_int]),
    "stocs_scene_footprints": (C.c_int, [_vp, _fp, C.c_int, C.c_int, C.c_int, C.POINTER(RenderParams), C.c_int, _vp, C.POINTER(SceneRecord)]),
    "stocs_scene_select": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _fp, _ip, C.POINTER(SceneRecord), C.c_int, _ip, C.POINTER(SceneParams),
                                     C.POINTER(SceneResult), _ip, _intp]),
    "stocs_device_alloc_count": (C.c_int64, []),
    "stocs_debug_stream_audit_selftest": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "stocs_debug_streams_overlap": (C.c_int, [_vp]),
    "stocs_debug_sort_pairs": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _fp, C.POINTER(C.c_uint32), C.c_int]),
    "stocs_last_call_timing": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_int, _intp]),
    "stocs_set_option": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "stocs_get_cull_state": (C.c_int, [_vp, _fp, _ip, _intp, _fp, _fp, C.c_int64, _i64p]),
    "stocs_get_grid_info": (C.c_int, [_vp, C.POINTER(GridInfo)]),
    "stocs_get_grid_octants": (C.c_int, [_vp, _i64p]),
    "stocs_model_patch_order": (C.c_int, [_fp, C.c_int, _ip, _fp]),
    "stocs_model_subpatches": (C.c_int, [_fp, C.c_int, _ip, _fp]),
    "stocs_model_subpatch_normals": (C.c_int, [_fp, _fp, C.c_int, _ip, _fp]),
    "stocs_patch_normal_bound_host": (C.c_float, [C.c_uint32, _fp, C.c_float, C.c_float, _intp, _fp]),
    "stocs_lcp_patch_normal_count": (C.c_int, [_vp, _vp, C.c_int, _i64p]),
    "stocs_patch_normal_info": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "stocs_kdtree_nn_host": (C.c_int, [_fp, C.c_int, _fp, C.c_int, C.c_float, _ip]),
    "stocs_last_tie_counts": (C.c_int, [_vp, _i64p, _i64p]),
    "stocs_set_stream": (C.c_int, [_vp, _vp]),
    "stocs_best_device_async": (C.c_int, [_vp, _vp, C.c_int, C.c_uint32, _vp]),
    "stocs_score_best_device_async": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_uint32, _vp]),
    "stocs_sync": (C.c_int, [_vp]),
    "stocs_stream": (_vp, [_vp]),
    "stocs_time_score_kernel": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _fp]),
    "stocs_dev_alloc": (C.c_int, [_vp, C.c_int64, C.POINTER(_vp)]),
    "stocs_dev_free": (C.c_int, [_vp, _vp]),
    "stocs_dev_upload": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "stocs_dev_download": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
}

_LIB = None


def load():
    """Load libstocs_hip.so; raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(make -C model_matching_amd/csrc).  There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def check(rc):
    if rc != STOCS_OK:
        raise StocsError(rc, load().stocs_last_error().decode())


def default_params(**kw) -> Params:
    p = Params()
    load().stocs_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(_fp)


def i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)
