/*
 * stocs_hip.h -- C ABI of libstocs_hip.so: the MI355X (gfx950) implementation of the StoCS hot path
 * of kuwt/model_matching (congruent-set sampling + rigid-transform estimation + LCP verification).
 *
 * The reference has no plugin/FFI interface: its boundary is the C++ class stocs::stocs_estimator
 * (reference include/stocs.hpp:16-180) statically linked into stocs_single
 * (reference src/stocs_match_one_object.cpp:51-185).  Each entry point below replaces one method
 * (or a batch of calls to one method) of that class; include/stocs.hpp of THIS repo is the façade
 * with the reference's method names on top of these calls, INTEGRATION.md shows the binding a
 * maintainer of the reference would add.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returns 0 on success or
 * a negative stocs_status; nothing throws across the boundary; output buffers are caller-owned with
 * explicit capacities; 4x4 matrices are 16 floats COLUMN-major (Eigen::Matrix4f::data() layout);
 * one context is bound to one HIP device and one stream, is not thread-safe, distinct contexts are
 * independent.  There is no CPU fallback: without a usable HIP device stocs_ctx_create fails with
 * STOCS_ERR_NO_DEVICE.
 */
#ifndef STOCS_HIP_H
#define STOCS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct stocs_ctx stocs_ctx;

typedef enum stocs_status {
    STOCS_OK = 0,
    STOCS_ERR_INVALID = -1,    /* bad argument */
    STOCS_ERR_NO_DEVICE = -2,  /* no HIP device / HIP runtime error at init */
    STOCS_ERR_HIP = -3,        /* HIP runtime error (see stocs_last_error) */
    STOCS_ERR_CAPACITY = -4,   /* caller buffer too small; required count is returned */
    STOCS_ERR_STATE = -5,      /* call order violated (e.g. no index, no bases) */
    STOCS_ERR_NOMEM = -6
} stocs_status;

/* Parameters: the file-scope constants of reference src/stocs_match_one_object.cpp:7-17 and the
 * hard-coded thresholds of reference src/stocs.cpp:368-370. */
typedef struct stocs_params {
    float distance_threshold;        /* 0.005  (:8)  epsilon of congruent-set matching and LCP   */
    int   ppf_tr_discretization;     /* 5 mm   (:9)                                               */
    int   ppf_rot_discretization;    /* 5 deg  (:10)                                              */
    float plane_threshold;           /* 0.015  (stocs.cpp:368)                                    */
    float min_distance_base;         /* 0.01   (stocs.cpp:369)                                    */
    float internal_angle_threshold;  /* 30     (stocs.cpp:370)                                    */
    float lcp_normal_angle;          /* 30     (stocs.cpp:1032)                                   */
    int   image_width, image_height; /* 640x480 (:23-24); only used by instance-mode sampling     */
    int   number_of_bases;           /* 100    (:16)                                              */
    int   maximum_congruent_sets;    /* 200    (:17)                                              */
} stocs_params;

void stocs_default_params(stocs_params* p);
const char* stocs_last_error(void);
const char* stocs_version(void);

/* ---- construction: replaces stocs_estimator::stocs_estimator (stocs.hpp:18-61):
 * load_object_info + load_scene_info (clouds are handed over as flat arrays instead of PLY/PNG
 * files), centroid_shift (stocs.cpp:943-964), kdtree_initialize (stocs.cpp:966-980; here a brick
 * grid over the centred scene).  Normals are normalised as Point3D::set_normal does.  When
 * build_index != 0 the model PPF index (reference PPFMapType, built offline by
 * stocs::pre_process_model, stocs.cpp:63-78 + rgbd.cpp:123-154) is built on the device.
 * scene_pixel2 (row,col per point) may be NULL.  device < 0 selects the current device. ---- */
int stocs_ctx_create(const stocs_params* prm,
                     const float* scene_pos3, const float* scene_nrm3, const float* scene_prob,
                     const int32_t* scene_pixel2, int nS,
                     const float* model_pos3, const float* model_nrm3, int nM,
                     int build_index, int device, stocs_ctx** out);
int stocs_ctx_destroy(stocs_ctx* ctx);
/* A new scene (the next camera frame) against the same model: load_scene_info + centroid_shift +
 * kdtree_initialize (stocs.hpp:36-60, stocs.cpp:943-980) for the scene only.  The model clouds and the PPF
 * index are kept; bases, candidates, edge map and instance-mode segments of the old scene are dropped.
 * Equivalent to destroying the context and creating it again with the same model, minus the index build. */
int stocs_ctx_set_scene(stocs_ctx* ctx, const float* scene_pos3, const float* scene_nrm3, const float* scene_prob,
                        const int32_t* scene_pixel2, int nS);

/* getters: stocs.hpp:115-116 get_scene_centroid (+ model centroid) */
int stocs_get_centroids(const stocs_ctx* ctx, float* scene3, float* model3);
int stocs_get_sizes(const stocs_ctx* ctx, int* nS, int* nM);
/* edge map (png values, image_height*image_width bytes): presence switches the driver to
 * sample_instance_base, as the stat() of probability_maps/edge.png does (stocs_match_one_object.cpp:90) */
int stocs_set_edge_map(stocs_ctx* ctx, const uint8_t* edge);
/* start a new trial stream on the same scene: restores the class probabilities given at construction
 * (instance-mode sampling decays them in place, stocs.cpp:572-580) and clears the segmentation state,
 * bases, quads and candidates.  Equivalent to constructing a new estimator, without rebuilding the grid
 * and the index. */
int stocs_reset_trial(stocs_ctx* ctx);

/* ---- PPF index queries: replace ppf_map.find (call sites stocs.cpp:403,438,487,780,784) ---- */
int stocs_ppf_compute_host(const float* p1, const float* n1, const float* p2, const float* n2,
                           int tr, int rot, int32_t* key4);       /* rgbd.cpp:99-121 */
int stocs_index_exists(const stocs_ctx* ctx, const int32_t* key4, int* exists);
/* pairs of lookup(key) in lexicographic (id1,id2) order == the reference's insertion order */
int stocs_index_lookup(stocs_ctx* ctx, const int32_t* key4, int32_t* pairs2, int64_t cap, int64_t* n);
int stocs_index_stats(const stocs_ctx* ctx, int64_t* n_pairs, int64_t* n_buckets, int64_t* n_keys);
/* on-disk form of the index: replaces rgbd::save_ppf_map / load_ppf_map (rgbd.cpp:156-177; a Boost
 * binary archive of the std::map there, compiler/Boost-version specific) by a flat, versioned,
 * little-endian CSR file.  load requires a context created with build_index = 0 for the SAME model
 * cloud and discretisation (checked through a hash stored in the file). */
int stocs_index_save(stocs_ctx* ctx, const char* path);
int stocs_index_load(stocs_ctx* ctx, const char* path);

/* ---- base sampling: batched form of the loop stocs_match_one_object.cpp:81-101 over
 * sample_class_base (stocs.cpp:363-519) / sample_instance_base (stocs.cpp:559-751).
 * mode 0 = class, 1 = instance.  Attempt i uses the seeded draws rng(seed, first_attempt+i, k).
 * Outputs per attempt: ids (permuted by try_sampled_base, stocs.cpp:224-268), the two invariants,
 * valid flag.  Valid bases are appended to the context's base set in attempt order. ---- */
int stocs_sample_bases(stocs_ctx* ctx, int mode, uint64_t seed, int first_attempt, int n_attempts,
                       float dispersion, int32_t* base_ids4, float* inv2, int32_t* valid);
/* `segment` of the last instance-mode attempt (the out-parameter of sample_instance_base, filled at stocs.cpp:628-638):
 * indices of the scene points that survived pass 1 inside the segmentation mask, in scene order */
int stocs_get_segment(const stocs_ctx* ctx, int32_t* scene_idx, int cap, int* n);
/* the context's scene as the estimator holds it: centred positions (centroid_shift), unit normals, CURRENT class
 * probabilities (instance-mode sampling decays them, Q8) and pixels; any pointer may be NULL */
int stocs_get_scene(const stocs_ctx* ctx, float* pos3_centred, float* nrm3, float* class_prob, int32_t* pixel2);
/* inject bases (already ordered, with their invariants) -- used by the parity tests and by callers
 * that sample elsewhere; replaces the context's base set */
int stocs_set_bases(stocs_ctx* ctx, int n, const int32_t* base_ids4, const float* inv2);
int stocs_clear_bases(stocs_ctx* ctx);
int stocs_num_bases(const stocs_ctx* ctx);
/* one pass of the weight update for fixed base points (kernel-level parity with the oracle):
 * pass k in 1..3, b3 = {P1,P2,P3} scene indices, w_in/w_out host arrays of nS floats */
int stocs_class_pass(stocs_ctx* ctx, int pass, const int32_t* b3, const float* w_in, float* w_out);
/* device self-check of the float filter that sits in front of the PPF arithmetic in the pass kernels: n_pairs seeded pairs
 * of scene points keyed both ways; *n_mismatch must come back 0, *n_undecided counts the pairs the filter handed to the
 * reference's double arithmetic */
int stocs_ppf_filter_check(stocs_ctx* ctx, uint64_t seed, int64_t n_pairs, int64_t* n_tested, int64_t* n_undecided, int64_t* n_mismatch);
/* device self-check of the fixed-point weight of the seeded draws: the kernels read trunc(w * 2^32) off the bits of w; all
 * 2^32 float patterns are compared with (uint64_t)((double)w * 4294967296.0) (0 for w <= 0 / NaN, saturating);
 * *n_mismatch must come back 0 */
int stocs_weight_fix_check(stocs_ctx* ctx, int64_t* n_mismatch);
/* try_sampled_base on four scene indices (stocs.cpp:224-268) */
int stocs_try_sampled_base(stocs_ctx* ctx, int32_t* ids4_inout, float* inv2, int* valid);
/* the seeded weighted draw itself (stocs.cpp:133-148 replacement): index or -1 */
int stocs_draw(stocs_ctx* ctx, const float* w, int n, uint64_t r64, int* index);
/* Which kernel form the last stocs_sample_bases or stocs_run_trials* call on the context ran, class mode or instance mode (tests only;
 * no device work, no synchronisation, no allocation; any output pointer may be NULL).  STOCS_ERR_STATE: no sampling call on the
 * context yet.
 *   *kernel     one of the STOCS_FORM_* values below
 *   *threads    threads per workgroup of the attempts kernel
 *   *lds_bytes  its dynamic LDS per workgroup
 *   *cap        survivors of pass 1 the lean kernel's list holds (an attempt with more is redone by the full-size kernel)
 *   *launches   launches of the attempts kernel (the redo of overflowed attempts not counted)
 *   *redone     attempts redone after a lean overflow
 * The rule, for a scene of S points (a16(x) = x rounded up to a multiple of 16):
 *   STOCS_CLASS_MULTI_KERNEL set: NINE_LAUNCH (stocs_sample_bases only); threads = lds_bytes = cap = launches = 0.
 *   The lean kernel is taken when 64 <= S <= 26000, neither STOCS_CLASS_FULL_KERNEL nor STOCS_INSTANCE_NO_LDS is set, and the call
 *   is a trial batch, or has more than 256 attempts, or finds the prior's prefix sums current (an earlier lean call since the last
 *   stocs_ctx_set_scene / stocs_reset_trial), or STOCS_CLASS_LEAN_KERNEL is set.  Then
 *     threads   = 256 for S <= 8000, 512 for S <= 24000, else 1024; STOCS_CLASS_LEAN_512 makes 256 into 512 and
 *                 STOCS_CLASS_LEAN_1024 makes both into 1024;
 *     lds_bytes = max(a16(2 S), min(top, a16(6 S + 16))) with top = 16384, 36864, 76800 for 256, 512, 1024 threads;
 *     cap       = min(S + 1, (lds_bytes - 8) / 6) rounded down to an even number; STOCS_CLASS_LEAN_CAP = v lowers it to
 *                 max(2, v rounded down to an even number);
 *     launches  = 1.
 *   Otherwise the full-size kernel, 1024 threads, cap = 0:
 *     S <= 26000 and STOCS_INSTANCE_NO_LDS unset: FULL_LDS, lds_bytes = a16(4 S) + 2 S + 16, launches = 1;
 *     else FULL_DEVICE_MEMORY, lds_bytes = 0; stocs_sample_bases: launches = 1; a trial batch of n attempts in all runs
 *     p = max(1, min(n, floor(2^30 / (8 S)))) attempts per launch (at most 1 GiB of working set): launches = ceil(n / p).
 * Instance mode (mode 1) has one kernel, a pair of 1024-thread workgroups per trial, in two forms of the attempt's working set:
 *   S <= 16000 and STOCS_INSTANCE_NO_LDS unset: INSTANCE_LDS, lds_bytes = 65552 + a16(4 S) + 2 S + 16 (65552 = a16(4 * 16385): the
 *   union-find parents of a disc of up to 16384 runs, which both forms keep in LDS); else INSTANCE_DEVICE_MEMORY, lds_bytes = 65552.
 *   threads = 1024, cap = 0, redone = 0; launches = 1 for stocs_sample_bases, ceil(n_trials / max(1, n_cu / 2)) for a trial batch on a
 *   device of n_cu compute units. */
enum { STOCS_FORM_LEAN = 0, STOCS_FORM_FULL_LDS = 1, STOCS_FORM_FULL_DEVICE_MEMORY = 2, STOCS_FORM_NINE_LAUNCH = 3, STOCS_FORM_INSTANCE_LDS = 4,
       STOCS_FORM_INSTANCE_DEVICE_MEMORY = 5 };
int stocs_last_sampling_form(const stocs_ctx* ctx, int* kernel, int* threads, int64_t* lds_bytes, int* cap, int* launches, int* redone);
/* What every attempt of the last stocs_sample_bases(mode 1) call on the context did in its first workgroup (tests only; copies from the
 * device and may synchronise; not kept for trial batches).  rec4[4 a ..]: the survivors of pass 1 inside the mask, point 1 (-1 when the
 * first draw failed), 1 when the attempt got as far as its mask, and the path of the mask: the number of passable runs in the image rows
 * of the disc for a new flood fill (up to 16384 the union-find parents are in LDS, beyond that in device memory), -1 when the seed pixel
 * was labelled already and the mask of that earlier attempt was taken, 0 when the first draw failed.  *n = attempts of that call; at most
 * cap records are written (STOCS_ERR_CAPACITY when there are more; rec4 may be NULL to ask for *n).  STOCS_ERR_STATE before the first
 * such call. */
int stocs_last_instance_attempts(stocs_ctx* ctx, int32_t* rec4, int cap, int* n);
/* Point 1 of the lean class kernel on its own (tests only): index[k] = the point the lean kernel draws first for the 64-bit word
 * r64[k] against the context's current prior -- the first scene index whose inclusive prefix sum of the 2^32 fixed-point prior
 * weights exceeds mulhi64(r64[k], total) -- or -1 when the total is zero.  Brings the prior's prefix sums up to date as a lean call
 * would, then runs the kernel's own search, one wavefront per word.  STOCS_ERR_STATE without a scene, STOCS_ERR_INVALID for a
 * scene outside 64 <= S <= 32768 (the sizes the lean kernel is compiled for). */
int stocs_debug_draw_point1(stocs_ctx* ctx, const uint64_t* r64, int n, int32_t* index);

/* ---- congruent sets: find_congruent_sets_on_model (stocs.cpp:753-869) for every base of the base
 * set at once (per-base COUNTS; quads are produced on demand); then per-base read-back:
 * stocs_get_quads -- all quads of a base, sorted as the reference's std::set orders them (stocs.cpp:860-866);
 * stocs_get_quads_at -- the quads at given ranks of the base's WALK order: by position cell of the Q pair's query
 * point, then index position of the Q pair, then index position of the P pair (index position of a model pair = its
 * quantised feature, then (id1, id2)) -- the enumeration stocs_make_transforms samples from for a base with >= max
 * quads (the reference shuffles with an unseeded generator there, so any fixed enumeration serves). ---- */
int stocs_find_congruent_all(stocs_ctx* ctx, int64_t* total_quads);
int stocs_get_quads(stocs_ctx* ctx, int base_slot, int32_t* quads4, int64_t cap, int64_t* n);
int stocs_get_quads_at(stocs_ctx* ctx, int base_slot, const int64_t* ranks, int n, int32_t* quads4);

/* one cone query of the normal set (normalset.hpp:166-214) evaluated on the host, for tests: the 343-bit direction-cell set
 * from the reference's float arithmetic alone and the one the kernels build (a cheap filtered evaluation, the
 * reference's arithmetic where the filter cannot decide; cone_cells.h); the two must be equal.  n3 = query direction. */
int stocs_cone_cells_host(const float* n3, float cos_alpha, uint32_t* exact_bits11, uint32_t* kernel_bits11, int* n_samples,
                          int* n_undecided);
/* n such queries on the device, for tests: what the join kernels compute for a sample.  The cone fields of every query (number of
 * samples, sin alpha, the shared (cos, sin) table) are filled on the host exactly as stocs_cone_cells_host and the count pass fill
 * them; ONE kernel, one lane per query, then evaluates the shared functions of cone_cells.h in the order of the join: the
 * quaternion, the filter's constants, and per sample (sin_alpha * table entry) the filtered cell and the exact cell.
 * n3 = n x 3 query directions, cos_alpha = n values; device < 0: the current device.  Per query:
 *   exact_bits11 [11 n]  the direction-cell set from the reference's arithmetic alone;
 *   kernel_bits11[11 n]  the set the join builds (filter first, exact where the filter is undecided);
 *   n_samples[n], n_undecided[n] (samples whose filtered cell was -1);  q4[4 n] the quaternion (x, y, z, w).
 * Per sample a of query i, at i * 64 + a (64 = the most samples a cone can have; slots beyond n_samples[i] hold -1, -1, 0):
 *   filtered_id  the filter's cell, or -1 when it cannot decide;  exact_id  the exact cell, or -1 for a direction that is not finite;
 *   t3[3 ..]     the filter's cell coordinates (tx, ty, tz) before truncation.
 * Synchronous; allocates and frees its own device memory. */
int stocs_cone_cells_device(int device, const float* n3, const float* cos_alpha, int n, uint32_t* exact_bits11, uint32_t* kernel_bits11,
                            int32_t* n_samples, int32_t* n_undecided, float* q4, int32_t* filtered_id, int32_t* exact_id, float* t3);

/* ---- candidate transforms: the loop stocs_match_one_object.cpp:120-147 over
 * get_rigid_transform_from_congruent_pair (stocs.cpp:871-941 -> ComputeRigidTransformation :270-361):
 * at most max_per_base quads per base (all when fewer; a seeded subset otherwise). ---- */
int stocs_make_transforms(stocs_ctx* ctx, int max_per_base, uint64_t seed, int* n_candidates);
/* single (base ids, quad) -> transform; ok=0 when the reference would not append a candidate */
int stocs_rigid_transform(stocs_ctx* ctx, const int32_t* ids4, const int32_t* quad4,
                          float* T16_centred, float* pose16_camera, int* ok);
int stocs_get_candidates(stocs_ctx* ctx, float* T16_centred, float* pose16_camera, float* lcp,
                         int32_t* base_index, int cap, int* n);

/* ---- verification: compute_alignment_score_for_rigid_transform (stocs.cpp:1006-1041), batched.
 * THE METRIC KERNEL: one candidate pose verified per transform. ---- */
int stocs_score_transforms(stocs_ctx* ctx, const float* T16_centred_host, int n, float* lcp_host);
/* device-resident variant: d_T16 and d_lcp are device pointers on the context's device; the call is
 * asynchronous on the context's stream (use stocs_sync) */
int stocs_score_transforms_device(stocs_ctx* ctx, const void* d_T16, int n, void* d_lcp);
/* score + device arg-max in one call (one host round trip): key as stocs_best_device.  The arg-max is taken in the epilogue of
 * the scoring kernel (one 64-bit atomic max per candidate: order independent), not by a second kernel */
int stocs_score_best_device(stocs_ctx* ctx, const void* d_T16, int n, void* d_lcp, uint32_t id_offset, uint64_t* key);
/* the same without any host synchronisation: scores into d_lcp, the packed key of the first maximum (0: no positive score) into
 * the 8 bytes at d_key8 (device memory), everything on the context's stream -- what bench.py times per step */
int stocs_score_best_device_async(stocs_ctx* ctx, const void* d_T16, int n, void* d_lcp, uint32_t id_offset, void* d_key8);
/* per model point: index of the matched scene point (-1 none) and whether it was counted */
int stocs_lcp_detail(stocs_ctx* ctx, const float* T16_centred_host, int32_t* hit, uint8_t* counted);
/* measurement aid (bench.py's `needed_bytes_per_launch`; no reference counterpart): over n device-resident transforms, the number of
 * (candidate, model point) queries of stocs.cpp:1016-1024 that found a scene point within epsilon (*hits: the nearest-neighbour
 * records a pose really needs, 28 bytes each) and how many of those passed the normal test of :1028-1032 (*counted, may be NULL).
 * Runs the per-point detail form of the scoring kernel in chunks; synchronises. */
int stocs_lcp_hit_count(stocs_ctx* ctx, const void* d_T16, int n, int64_t* hits, int64_t* counted);
/* test aid for the normal-cone gate of the queue-fed scoring kernel ("lcp_normal_gate"; no reference counterpart): over n
 * device-resident transforms, out[0] = the (candidate, model point) queries that land in a non-empty cell of the scene grid and
 * survive its sub-cell mask, out[1] = those of them the gate rules out, out[2] = the ruled-out ones that the per-point detail form
 * of the scoring kernel reports as counted -- 0, or the gate is wrong.  A plain counting kernel, one lane per query, that calls
 * the scoring kernel's own gate function; on a grid without cones out[1] is 0.  Runs the detail form in chunks; synchronises. */
int stocs_lcp_gate_count(stocs_ctx* ctx, const void* d_T16, int n, int64_t out[3]);
/* compute_best_transform (stocs.cpp:982-1004): score every stored candidate, arg-max with first
 * maximum winning; best_idx = -1 and best_lcp = 0 when every score is 0 */
int stocs_verify_all(stocs_ctx* ctx, float* best_lcp, int* best_idx, float* best_pose16_camera);
/* ---- trial batches: N independent StoCS trials in ONE set of launches.  The reference runs one trial per process
 * (stocs_match_one_object.cpp:81-165: 100 base attempts -> congruent sets -> <= 200 candidates per base -> best candidate);
 * BASELINE config 4 runs 64 of them.  Trial t of the batch is, bit for bit (bases, congruent sets, candidates, scores, winner),
 *     stocs_reset_trial; stocs_sample_bases(mode, seeds[t], 0, n_attempts, dispersion); stocs_find_congruent_all;
 *     stocs_make_transforms(max_per_base, seeds[t]); stocs_verify_all
 * but the trials share every launch: one sampling launch (class mode: a workgroup per attempt of every trial; instance mode: a
 * workgroup pair per trial on its own copy of the image-space state), one congruent-set pass over the concatenated base sets, one
 * transform pass, one scoring launch with a per-trial arg-max.  Batches beyond what one set of launches can key or hold are cut
 * into pieces of consecutive trials (environment STOCS_TRIALS_MAX_MB: device-memory ceiling of a piece, default 16384).
 * The context is left as stocs_reset_trial leaves it (no bases, no candidates); the batch's record stays readable through the
 * getters below until the next batch.  keep_details != 0 also keeps every trial's candidate list (tests; costs a download). ---- */
typedef struct stocs_trial_result {
    int32_t n_bases;          /* valid bases among the trial's attempts                                   */
    int32_t n_candidates;     /* candidates its stocs_make_transforms produced                            */
    int64_t n_quads;          /* congruent sets over all its bases                                        */
    float   best_lcp;         /* compute_best_transform of the trial alone (stocs.cpp:982-1004)           */
    int32_t best_index;       /* index into the trial's own candidate list; -1 (and best_lcp 0): no pose  */
    float   best_pose16[16];  /* camera frame, column-major; zeros when there is no pose                  */
} stocs_trial_result;
int stocs_run_trials(stocs_ctx* ctx, int mode, int n_trials, const uint64_t* seeds, int n_attempts, float dispersion, int max_per_base,
                     int keep_details, stocs_trial_result* out /* n_trials, may be NULL */);
/* attempts of one trial of the last batch, as stocs_sample_bases returns them (ids permuted by try_sampled_base, invariants, valid) */
int stocs_trials_get_bases(stocs_ctx* ctx, int trial, int32_t* base_ids4, float* inv2, int32_t* valid, int cap_attempts, int* n_attempts);
/* congruent sets of each valid base of the trial (what stocs_get_quads reports as *n for that base slot) */
int stocs_trials_get_quad_counts(stocs_ctx* ctx, int trial, int64_t* counts, int cap, int* n);
/* the trial's candidates as stocs_get_candidates returns them after stocs_verify_all (needs keep_details; base_index counts the
 * trial's own valid bases) */
int stocs_trials_get_candidates(stocs_ctx* ctx, int trial, float* T16_centred, float* pose16_camera, float* lcp, int32_t* base_index, int cap, int* n);
/* ---- post-processing inside a trial batch: clustering::greedy_clustering (pose_clustering.cpp:79-121) of every trial's candidates
 * and clustering::point_to_plane_icp (:123-140) of the kept hypotheses, on the device, per piece of the batch; only the kept
 * hypotheses come back (with the per-trial results: one read-back, one synchronisation per piece).  Trial t's hypotheses are, bit
 * for bit, stocs_cluster_poses(its candidates' camera poses, their lcp, n, acceptable_fraction, best_score = its best_lcp, ...) --
 * candidate_index in that order, i.e. descending lcp -- and, with refine_iterations > 0, stocs_refine_poses(the kept candidates'
 * centred T16, n, NULL, 0, refine_iterations, max_correspondence_distance) run on the same context right after that trial alone
 * (instance mode: rescored against the trial's own decayed class probabilities).  stocs_run_trials(...) is
 * stocs_run_trials_post(..., post = NULL, ...): the batch runs exactly as without post-processing.  A negative count or iteration
 * number, a NaN fraction, a min_distance / min_angle / max_correspondence_distance that is <= 0 or not finite: STOCS_ERR_INVALID. ---- */
typedef struct stocs_trial_post {
    float   acceptable_fraction;          /* candidates with lcp > fraction * best_lcp take part (the driver uses 0.8)            */
    int32_t maximum_pose_count;           /* >= 0; up to count + 1 hypotheses per trial (the reference's size() > count break)    */
    float   min_distance, min_angle;      /* metres, degrees: a candidate within both of a kept one is dropped (0.02, 15)        */
    float   sym3[3];                      /* sym_info: 0 / 90 / 180 / 360 degrees per Euler axis                                 */
    int32_t refine_iterations;            /* 0: cluster only (refined fields = the candidate's, counts 0)                        */
    float   max_correspondence_distance;  /* metres (0.035)                                                                      */
} stocs_trial_post;
int stocs_run_trials_post(stocs_ctx* ctx, int mode, int n_trials, const uint64_t* seeds, int n_attempts, float dispersion, int max_per_base,
                          int keep_details, const stocs_trial_post* post /* may be NULL */, stocs_trial_result* out /* n_trials, may be NULL */);
typedef struct stocs_trial_hypothesis {
    int32_t candidate_index, base_index;  /* into the trial's own lists, as stocs_trials_get_candidates                          */
    float   lcp, pose16[16];              /* the candidate as scored (camera frame, column-major)                                */
    float   refined_lcp, refined_pose16[16];
    int32_t n_correspondences, iterations;   /* stocs_refine_poses's; == the candidate's lcp / pose and 0, 0 without refinement */
} stocs_trial_hypothesis;
/* the hypotheses of one trial of the last batch, in cluster order (descending lcp); a trial without a pose has none.  The batch ran
 * without post: STOCS_ERR_STATE; out != NULL and cap < the count: STOCS_ERR_CAPACITY (*n is the count either way) */
int stocs_trials_get_hypotheses(stocs_ctx* ctx, int trial, stocs_trial_hypothesis* out, int cap, int* n);
/* ---- stocs_run_trials_post with the kept hypotheses refined by the trimmed, normal-gated form (stocs_refine_poses_robust, below)
 * instead of the plain one.  Iterations and correspondence distance are post's (refine_iterations, max_correspondence_distance);
 * keep_ratio and min_normal_cos mean what they mean in stocs_refine_robust_params, under the same rules: keep_ratio in (0, 1] and
 * not NaN; min_normal_cos <= 1 and not NaN, below -1 turns the gate off.  Outside them, or post == NULL: STOCS_ERR_INVALID; every
 * other argument is checked as stocs_run_trials_post checks it.  The contract:
 *   - everything up to and including the clustering is stocs_run_trials_post's, bit for bit;
 *   - with refine_iterations > 0, trial t's refined fields are bitwise what
 *         stocs_refine_poses_robust(the kept candidates' centred T16, n, NULL, 0,
 *                                   {refine_iterations, max_correspondence_distance, keep_ratio, min_normal_cos}, ...)
 *     gives when run on the same context right after that trial alone; in instance mode the pose is rescored against the trial's own
 *     decayed class probabilities, as in stocs_run_trials_post, and the gate reads the base scene's normals (the decay changes the
 *     weights, never a normal);
 *   - n_correspondences is k of the last evaluated iteration (the kept pairs); n_cand is not reported (the record is ABI);
 *   - the hypotheses are read with stocs_trials_get_hypotheses, unchanged;
 *   - with keep_ratio == 1 and the gate off, every byte of every record and result equals stocs_run_trials_post's.
 * The robust workspace takes 8 bytes per (hypothesis, scene point), and a piece's slots are an upper bound (min(count + 1,
 * candidates) per trial) on the whole scene: a piece refines its slots in GROUPS of consecutive slots that share the workspace, a
 * group being the largest run whose demand (group x scene points x 8 bytes) stays within STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES,
 * and at least one slot.  Only a scene too large for ONE slot (scene points x 8 bytes above the limit, where rank words are stored:
 * keep_ratio < 1) is STOCS_ERR_INVALID.  The
 * environment variable STOCS_REFINE_ROBUST_GROUP_BYTES, read per call, lowers the limit (tests: forces several groups).  Results
 * are bitwise independent of the grouping and of the pieces.  The workspace is grow-only (stocs_refine_robust_workspace): a repeated
 * call of the same size allocates nothing.  One read-back and one synchronisation per piece, as stocs_run_trials_post.
 * stocs_last_call_timing(which = 3) reports the groups of the last call next to its pieces. ---- */
int stocs_run_trials_post_robust(stocs_ctx* ctx, int mode, int n_trials, const uint64_t* seeds, int n_attempts, float dispersion, int max_per_base,
                                 int keep_details, const stocs_trial_post* post /* not NULL */, float keep_ratio, float min_normal_cos,
                                 stocs_trial_result* out /* n_trials, may be NULL */);

/* arg-max of n device-resident scores on the device: *key = max over i of
 * stocs_pack_best(lcp[i], id_offset + i), 0 when no score is positive (first maximum wins, as the
 * strict > of stocs.cpp:994).  Synchronises the context's stream; 8 bytes cross PCIe. */
int stocs_best_device(stocs_ctx* ctx, const void* d_lcp, int n, uint32_t id_offset, uint64_t* key);
/* order-preserving key for the cross-GPU arg-max (max wins; lowest global id wins ties); 0 = "no pose" when the score
 * is not positive (stocs.cpp:987-998), so a rank whose candidates all scored 0 never wins */
uint64_t stocs_pack_best(float lcp, uint32_t global_candidate_id);
void stocs_unpack_best(uint64_t key, float* lcp, uint32_t* global_candidate_id);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI (librccl is opened lazily).  The path has a single
 * exchange: the arg-max of compute_best_transform across ranks. ---- */
typedef struct stocs_comm stocs_comm;
int stocs_comm_unique_id(void* id128);                       /* rank 0: 128-byte ncclUniqueId to hand to the others */
int stocs_comm_create(const void* id128, int nranks, int rank, int device, stocs_comm** out);
int stocs_comm_destroy(stocs_comm* comm);
/* in: this rank's packed key (0 = none) and pose; out: the global maximum and the winner's pose.
 * Global ids must satisfy id / ids_per_rank == owning rank.  Status: exercised with a one-rank communicator on a
 * one-GPU box and by world-size-2 gloo tests of the same reduction; the 2+ rank RCCL path is unmeasured so far. */
int stocs_allreduce_best(stocs_comm* comm, void* hip_stream, uint64_t* key_inout, float* pose16_inout, uint32_t ids_per_rank);

/* ---- pose post-processing: clustering::greedy_clustering (pose_clustering.cpp:79-121), host ---- */
int stocs_cluster_poses(const float* poses16, const float* lcp, int n, float acceptable_fraction,
                        float best_score, int maximum_pose_count, float min_distance, float min_angle,
                        const float* sym3, int32_t* out_idx, int cap, int* n_out);
/* ---- the device clustering of trial batches (csrc/cluster.hip, trial_cluster_kernel) on candidates the caller gives: the kernel
 * stocs_run_trials_post runs, through the same launcher, without the rest of a batch.  poses16: N x 16 camera-frame, column-major;
 * lcp: N scores; cand_off: n_trials + 1 offsets into both, cand_off[0] = 0, not decreasing, N = cand_off[n_trials]; best_score[t]:
 * trial t's best_lcp as the batch's arg-max leaves it (its largest positive score, 0 when it has none).  Trial t's result is, bit for
 * bit, stocs_cluster_poses(its poses, its lcp, n_t, acceptable_fraction, best_score[t], ...): out_cnt[t] indices (local to the trial)
 * at out_idx[out_off[t] ..], in cluster order.  out_off[t + 1] - out_off[t] = min(maximum_pose_count + 1, n_t) slots as in
 * stocs_run_trials_post; slots past the count keep the -1 they are filled with before the launch.  out_cap: entries out_idx holds
 * (too few: STOCS_ERR_CAPACITY, out_off is valid).  round0_survivors (n_trials, may be NULL): per trial, how many candidates the
 * kernel's first pass let through (lcp > acceptable_fraction * best_score[t]) -- at most 2048 and the later rounds walk the list in
 * LDS, above it the flags in global memory.  Taken from the flags of a launch with count 0 in front of the real one.
 * DOMAIN: every lcp and best_score is +0 or above, or NaN (never a survivor).  Negative scores and -0.0 are STOCS_ERR_INVALID: the
 * pipeline cannot produce them, and the arg-max key orders the scores' bits as unsigned integers.  Also STOCS_ERR_INVALID, with a
 * message: a NULL argument, n_trials < 0, maximum_pose_count < 0, a NaN fraction, a min_distance / min_angle that is <= 0 or not
 * finite, offsets that decrease or do not start at 0.  n_trials = 0 is STOCS_OK (out_off[0] = 0).  Synchronises once; a test and
 * diagnosis facility (pageable copies). ---- */
int stocs_cluster_trials_device(stocs_ctx* ctx, const float* poses16, const float* lcp, const int32_t* cand_off, const float* best_score, int n_trials,
                                float acceptable_fraction, int maximum_pose_count, float min_distance, float min_angle, const float* sym3,
                                int32_t* out_off, int32_t* out_cnt, int32_t* out_idx, int out_cap, int32_t* round0_survivors);

/* ---- upstream rows, GPU implementations.  PARITY WITH THE REFERENCE IS UNPINNED:
 * their arithmetic lives in PCL / OpenCV-contrib, absent here; these are pinned against this repo's
 * numpy restatement (oracle/ingest_oracle.py).  Stand-alone calls (no context). ---- */
enum {
    /* surface normals of the depth image, rgbd.cpp:199-205 (cv::rgbd::RgbdNormals, RGBD_NORMALS_METHOD_LINEMOD on the raw
     * 16-bit depth image).  0: the published method restated -- Hinterstoisser et al., "Gradient Response Maps for Real-Time
     * Detection of Texture-Less Objects", PAMI 2012, section 2.4: least-squares depth gradient over the 8 neighbours at
     * +-5 pixels whose depth differs from the centre by less than 50 raw units, normal of the tangent plane through the three
     * back-projected points X, X(x+1), X(y+1), oriented toward the camera; integer sums, float normal.  Parity with OpenCV's
     * implementation is UNPINNED (library absent): patch, threshold and arithmetic follow the paper and the library's
     * documented defaults.  1: the least-squares plane over the 5x5 window of rounds 1-2 (tests/golden/example_*.npz hold its clouds) */
    STOCS_NORMALS_DEPTH_GRADIENT = 0,
    STOCS_NORMALS_PLANE_FIT = 1
};
typedef struct stocs_camera {
    float fx, cx, fy, cy;      /* stocs_match_one_object.cpp:20 */
    float depth_scale;         /* :21 */
    int width, height;         /* :23-24 */
    int normal_method;         /* STOCS_NORMALS_* */
} stocs_camera;
/* rgbd::load_rgbd_data_sampled (rgbd.cpp:179-281): depth + class-probability images (uint16) -> voxelised,
 * outlier-filtered, oriented scene cloud with class probability and (row, col) pixel per point.  Any depth is accepted (far
 * background and saturated 65 535 included): the voxel grid covers the whole frame, and the outlier-removal search grid only the
 * leaves that can hold a centroid with z in [-r, 2 m + r] (r = 2*voxel_size + 5 mm) -- every other centroid lies beyond the
 * reach of a point the z <= 2 m cut keeps, and is given no neighbours.  STOCS_ERR_INVALID when that near part of the frame needs
 * more than 2^28 search cells of r, i.e. spans kilometres: intrinsics no camera has (a focal length of a pixel or less). */
int stocs_ingest_scene(const stocs_camera* cam, const uint16_t* depth, const uint16_t* class_prob, float voxel_size,
                       float class_threshold, int device, float* pos3, float* nrm3, float* prob, int32_t* pixel2,
                       int cap, int* n_out);
/* Several objects of one frame: one depth image, n_objects class-probability images (n_objects*height*width uint16, object-major)
 * and n_objects class thresholds -> n_objects scene clouds, concatenated in object order; object k owns points
 * offsets[k] .. offsets[k+1]-1 (offsets: n_objects+1 entries, offsets[0] = 0).  The stages that never read a class-probability
 * image (back-projection, normals, voxel grid, outlier removal; rgbd.cpp:227-237) run once for the frame; per object, the cloud is
 * bitwise what stocs_ingest_scene(cam, depth, class_probs + k*height*width, voxel_size, class_thresholds[k], ...) returns.  An
 * empty cloud is not an error (offsets[k] == offsets[k+1]).  cap counts points over all objects: when offsets[n_objects] > cap
 * the call returns STOCS_ERR_CAPACITY with offsets filled and writes no point.  1 <= n_objects <= STOCS_MAX_FRAME_OBJECTS; NULL
 * images / thresholds / offsets, a non-finite threshold or voxel_size <= 0: STOCS_ERR_INVALID.  Same cached workspace and pinned
 * block as stocs_ingest_scene (the block grows to (2 + 2*n_objects) bytes per pixel in, 36 bytes per point out). */
#define STOCS_MAX_FRAME_OBJECTS 64
int stocs_ingest_scene_multi(const stocs_camera* cam, const uint16_t* depth, int n_objects, const uint16_t* class_probs,
                             const float* class_thresholds, float voxel_size, int device, float* pos3, float* nrm3, float* prob,
                             int32_t* pixel2, int cap, int32_t* offsets);
/* cloud part of stocs::pre_process_model (stocs.cpp:43-60): raw vertices -> radius normals pointing away
 * from the model origin -> voxel grid (positions and normals averaged per leaf) -> scale */
int stocs_preprocess_model(const float* raw_pos3, int n_raw, float normal_radius, float voxel_size, float model_scale,
                           int device, float* pos3, float* nrm3, int cap, int* n_out);
/* stocs_ingest_scene(_multi) / stocs_preprocess_model keep their device workspace cached per calling thread and device
 * (a stream of frames does no hipMalloc / hipFree after the first one), and stocs_ingest_scene(_multi) a pinned host block per calling thread
 * (40 bytes per pixel: the frame's two images go up and its cloud comes down through it, so the caller's arrays may be ordinary
 * pageable memory at no cost); this gives the calling thread's cache and block back. */
int stocs_trim(void);

/* ---- depth-only frames: support-plane removal and depth-connected segments (no reference counterpart; csrc/segment.hip, restated in
 * float32 numpy in tests/segment_ref.py, equal bit for bit).  In the reference the class-probability image and the edge image come from
 * a network; a caller with a depth camera and no network gets both from the frame's geometry here, in the formats the existing entry
 * points take: a uint16 class image (stocs_ingest_scene, stocs_ctx_set_frame), a uint8 edge image (stocs_set_edge_map), a label image
 * and one record per segment.  Stand-alone like stocs_ingest_scene: `device` (-1: the current one), no context; a per-thread cached
 * workspace and pinned block of its own that stocs_trim gives back; one read-back and one synchronisation per call; a second call of
 * the same size allocates nothing (stocs_device_alloc_count).  Every step is float, one IEEE operation at a time, no contraction;
 * 3-term sums are e0 + (e1 + e2); a comparison with NaN is false.  Pixel (row i, col j) has linear index i * width + j.
 *
 *   1. Points.  z = (float)raw * depth_scale; x = (float)(((double)j - (double)cx) * (double)z / (double)fx), y likewise with i, cy,
 *      fy (as the ingest forms them).  A pixel is VALID when raw != 0 and z <= max_depth.  cam->normal_method is ignored.
 *   2. Hypotheses.  Hypothesis h (0 .. plane_hypotheses - 1) draws the pixels i_k = ((rng64(seed, h, k) >> 32) * npix) >> 32, k = 0, 1, 2
 *      (rng64 of csrc/stocs_math.h, npix = width * height, 64-bit unsigned arithmetic), with points A, B, C.  e1 = B - A, e2 = C - A,
 *      m = e1 x e2 (each component a * b - c * d), mm = m0 m0 + (m1 m1 + m2 m2).  It is DEAD when one of the pixels is not valid, two
 *      indices are equal, or mm is not > 0 and finite.  The SCORED pixels are the valid ones with i % score_stride == 0 and
 *      j % score_stride == 0 (n_scored of them).  A pixel X is an inlier of h when, with d = X - A, s = m0 dx + (m1 dy + m2 dz),
 *      s * s <= (tol * tol) * mm.  count(h) = the inliers among the scored pixels.  The winner is the live h of count > 0 with the
 *      largest (count << 32) | ~h: the largest count, the lowest h on a tie; `winner` and `winner_count` report it (-1 and 0 without
 *      one).  plane_found = 0 when plane_hypotheses == 0, when there is no winner, or when (double)count < (double)plane_min_share *
 *      (double)n_scored -- then plane is zero, n_refit, n_on_plane, n_above and n_below are 0.
 *   3. Refit.  Over EVERY valid pixel (unstrided) that is an inlier of the winner and has |x|, |y|, |z| < 16: q = llrint((double)v *
 *      65536) per coordinate (exact: the product is a double, rounded to nearest even), and the int64 sums n_refit = sum 1, Sx, Sy, Sz,
 *      Sxx, Sxy, Sxz, Syy, Syz, Szz of q and their products (stocs_segment_last_moments gives the ten).  |q| < 2^20, a product < 2^40,
 *      and a frame holds at most 2^22 pixels (more: STOCS_ERR_CAPACITY), so every sum stays below 2^62: exact, whatever the order.
 *      In double: c = S / n / 65536, cov_ab = Sab / n / 2^32 - c_a c_b; the eigenvector of the smallest eigenvalue by cyclic Jacobi
 *      (pairs (0,1), (0,2), (1,2), 12 sweeps), normalised; d = -(n . c); n and d negated when d < 0; one cast to float each.  With
 *      n_refit < 3 or a non-finite result the winner's own plane is used the same way: n = m / |m|, d = -(n . A).  plane is
 *      (n0, n1, n2, d): n . X + d = 0, d >= 0 (the normal faces the camera).
 *   4. Heights.  h = (n0 x + (n1 y + n2 z)) + d on the float plane of `out`.  Among the valid pixels: on the plane when
 *      fabsf(h) <= tol (n_on_plane), above when h > tol (n_above), below when h < -tol (n_below).  FOREGROUND: valid, h > tol and
 *      h <= max_height.  Without a plane every valid pixel is foreground.
 *   5. Components.  4-neighbourhood; two foreground neighbours a, b join when fabsf(za - zb) <= jump_abs + jump_rel * fminf(za, zb).
 *      A component's root is the lowest linear index among its pixels.  n_components counts all of them; those of fewer than
 *      min_pixels pixels are dropped; the others are the segments, numbered 1 .. n_segments in the order of their roots.
 *      n_segments > cap_records: STOCS_ERR_CAPACITY with `out` filled, no record and no image written.
 *   6. Images (each height * width, or NULL).  labels: the segment's number, 0 elsewhere.  class_prob: 10000 in a segment, 0 elsewhere.
 *      edge: 255 where the pixel has a label and every 4-neighbour inside the image has the same label, 0 elsewhere (the png
 *      convention of stocs_set_edge_map: 255 = not an edge).
 *   7. Records.  root, pixels, the box c0 <= col <= c1, r0 <= row <= r1, and zmin / zmax, the extremes of the float z.
 *   8. Checked in this order: NULL cam / depth / p / out; width or height < 1; a parameter outside its range
 *      (stocs_check_segment_params; plane_hypotheses at most 2^20); cap_records < 0 or records == NULL with cap_records > 0: all
 *      STOCS_ERR_INVALID.  Then more than 2^22 pixels: STOCS_ERR_CAPACITY; a STOCS_SEGMENT_FORM other than 0, 1, 2: STOCS_ERR_INVALID.
 *      A frame with no valid pixel is not an error: zero result, empty images.
 * STOCS_SEGMENT_FORM in the environment forces the label kernel's form (1: union-find in device memory; 2: tiles of
 * stocs_segment_tile in LDS, then the tile borders; 0 or unset: the default); both end at the same roots.  With STOCS_SEGMENT_CLOCK=1
 * stocs_segment_last_device_ms gives the HIP-event times of the calling thread's last call: hypotheses + scoring + winner, and the
 * label kernels up to the flattened roots (STOCS_ERR_STATE without such a call). ---- */
typedef struct stocs_segment_params {
    float    max_depth;         /* m, > 0 finite: farther pixels are not valid (default 2.0, the ingest's cut)       */
    int32_t  plane_hypotheses;  /* >= 0; 0: no plane search, every valid pixel is foreground (default 1024)          */
    int32_t  score_stride;      /* >= 1: hypotheses are scored on pixels with row % s == 0 and col % s == 0 (4)      */
    float    plane_tolerance;   /* m, > 0 finite (0.01)                                                               */
    float    plane_min_share;   /* [0, 1]: least share of the scored pixels on the winning plane (0.15)              */
    float    max_height;        /* m, > 0 finite: foreground stands at most this far off the plane (0.5)             */
    float    jump_abs, jump_rel;/* >= 0 finite: neighbours join when |za - zb| <= jump_abs + jump_rel * min(za, zb) (0.005, 0.01) */
    int32_t  min_pixels;        /* >= 1: smaller components are dropped (200)                                         */
    uint64_t seed;              /* (1)                                                                                */
} stocs_segment_params;
typedef struct stocs_segment_result {
    float   plane[4];           /* unit normal facing the camera and offset: n.X + d = 0, d > 0; zeros without one   */
    int32_t plane_found, winner, winner_count, n_valid, n_scored, n_refit, n_on_plane, n_above, n_below,
            n_components, n_segments, reserved;
} stocs_segment_result;
typedef struct stocs_segment_record { int32_t root, pixels, c0, r0, c1, r1; float zmin, zmax; } stocs_segment_record; /* 32 bytes */
void stocs_default_segment_params(stocs_segment_params*);
int  stocs_check_segment_params(const stocs_segment_params*);                 /* host only */
int  stocs_segment_frame(const stocs_camera* cam, const uint16_t* depth, const stocs_segment_params* p, int device,
                         uint16_t* class_prob /* H W or NULL */, int32_t* labels /* H W or NULL */, uint8_t* edge /* H W or NULL */,
                         stocs_segment_record* records, int cap_records, stocs_segment_result* out);
int  stocs_segment_tile(int* width, int* height);                             /* host only: the label kernel's tile */
int  stocs_segment_last_device_ms(float* score_ms, float* label_ms);          /* with STOCS_SEGMENT_CLOCK=1         */
int  stocs_segment_last_moments(int64_t* moments10);                          /* n_refit, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz of the thread's last call */

/* ---- the concavity cut in front of the labelling (opt-in; no reference counterpart; restated in tests/segment_convex_ref.py, equal bit
 * for bit).  Two touching objects have no depth jump between them, so step 5 joins them; they have a concave crease.  This entry point is
 * stocs_segment_frame with two more steps between its steps 4 and 5, under step 1's conventions (float, one IEEE operation at a time, no
 * contraction, 3-term sums e0 + (e1 + e2), a comparison with NaN false).  It follows the local-convexity idea of LCCP (Stein et al. 2014)
 * on the image grid: three smoothed points a fixed pixel distance apart stand in for the two normals, and the angle test is on squared
 * quantities, so there is no normal and no square root.
 *
 *   4a. Smoothed depth.  For a FOREGROUND pixel c (raw depth q_c, float depth z_c), over the (2s+1)^2 window around it (s =
 *       smooth_radius) clipped to the image, a window pixel w COUNTS when it is foreground and fabsf(z_c - z_w) <= jump_abs + jump_rel *
 *       fminf(z_c, z_w) (step 5's rule between the centre and w directly; the centre always counts).  S = the integer sum of the raw
 *       depths that count, N their number; zs = ((float)S / (float)N) * depth_scale; xs, ys from zs as step 1 forms x, y from z, through
 *       double.  S <= 81 * 65535 < 2^24: exact as a float, whatever the order.  With s = 0 zs is step 1's z.  Off the foreground zs is NaN.
 *   4b. Bend test, per axis, r = bend_radius.  The horizontal triple at (i, j) is L = (i, j - r), C = (i, j), R = (i, j + r); the
 *       vertical one uses rows.  A triple is TESTED when all three pixels are inside the image and foreground and, for X in {L, R},
 *       fabsf(zs_X - zs_C) <= (float)r * (jump_abs + jump_rel * fminf(zs_C, zs_X)).  On the smoothed points, component-wise: a = C - L,
 *       b = R - C, m = (L + R) - (C + C); ab = a.b, aa = a.a, bb = b.b; toward = m.C < 0 (the chord's midpoint lies nearer the camera
 *       than C: the bend opens towards the viewer); bend = ab <= 0 || ab * ab < (bend_cos * bend_cos) * (aa * bb).  The pixel is CUT on
 *       that axis when the triple is tested and toward and bend hold.  A pixel cut on either axis leaves the foreground for step 5 only:
 *       it joins nothing, has label 0 and class 0 and is no component; n_on_plane, n_above and n_below stay step 4's.  Steps 5 - 7 run
 *       on what is left, unchanged, so the edge image marks the neighbours of a cut pixel as edges.
 *
 * cut (uint8 H W or NULL): bit 0 the horizontal cut, bit 1 the vertical.  smoothed (float H W or NULL): zs, NaN off the foreground;
 * copied back only when asked for.  cout: the triples tested and the pixels cut per axis, and the pixels cut on either.  Everything else
 * is stocs_segment_frame's, checked in its order: NULL cp / cout with the other NULLs, cp (stocs_check_segment_convex_params) right
 * after p; a STOCS_SEGMENT_BEND_FORM other than 0, 1, 2 after STOCS_SEGMENT_FORM.  On STOCS_ERR_CAPACITY `out` and `cout` are filled
 * and nothing else is written.  With bend_radius == 0 every output is stocs_segment_frame's bit for bit, cut is zero and so are the
 * counts (smoothed is still 4a's).  STOCS_SEGMENT_BEND_FORM forces the step's form (1: a lane per pixel, every read from device memory;
 * 2: a workgroup per stocs_segment_tile, depths and smoothed points in LDS; 0 or unset: the default); both end at the same bits.  With
 * STOCS_SEGMENT_CLOCK=1 stocs_segment_last_bend_ms gives the HIP-event time of steps 4a + 4b of the thread's last call
 * (STOCS_ERR_STATE when that was not a stocs_segment_frame_convex under the clock); stocs_segment_last_device_ms keeps its two values. ---- */
typedef struct stocs_segment_convex_params {
    int32_t bend_radius;        /* 0 .. 8 pixels between the points of a triple; 0: no cut (default 4)               */
    int32_t smooth_radius;      /* 0 .. 4: the window of 4a is (2s+1)^2 pixels (2)                                    */
    float   bend_cos;           /* [0, 1]: a bend of more than acos(bend_cos) is cut (0.90630779f, cos 25 degrees)   */
    int32_t reserved;           /* 0                                                                                  */
} stocs_segment_convex_params;
typedef struct stocs_segment_convex_result { int32_t n_tested_h, n_tested_v, n_cut_h, n_cut_v, n_cut, reserved[3]; } stocs_segment_convex_result; /* 32 bytes */
void stocs_default_segment_convex_params(stocs_segment_convex_params*);
int  stocs_check_segment_convex_params(const stocs_segment_convex_params*);   /* host only */
int  stocs_segment_frame_convex(const stocs_camera* cam, const uint16_t* depth, const stocs_segment_params* p, const stocs_segment_convex_params* cp,
                                int device, uint16_t* class_prob /* H W or NULL */, int32_t* labels /* H W or NULL */, uint8_t* edge /* H W or NULL */,
                                uint8_t* cut /* H W or NULL */, float* smoothed /* H W or NULL */, stocs_segment_record* records, int cap_records,
                                stocs_segment_result* out, stocs_segment_convex_result* cout);
int  stocs_segment_last_bend_ms(float* bend_ms);                              /* with STOCS_SEGMENT_CLOCK=1         */

/* ---- 3-D shape of every labelled region of a depth frame, and a size gate between segments and objects (no reference counterpart;
 * csrc/segment_shapes.hip and csrc/segment_gate.h, restated in numpy in tests/segment_shapes_ref.py).  The label image (int32, 0 = none,
 * 1 .. n_labels) may be stocs_segment_frame's, stocs_segment_frame_convex's or anybody's (a network's instance mask): nothing here depends
 * on how it was made.  Stand-alone like stocs_segment_frame: `device` (-1: the current one), no context, one stream, one pinned read-back
 * and one synchronisation per call, a per-thread cached workspace of its own that stocs_trim gives back; a second call of the same or a
 * smaller size allocates nothing (stocs_device_alloc_count).  Conventions of stocs_segment_frame: float, one IEEE operation at a time, no
 * contraction, 3-term sums e0 + (e1 + e2).
 *
 *   1. Used pixels.  A label outside [0, n_labels] is counted (n_out_of_range) and treated as 0.  A LABELLED pixel (label 1 .. n_labels,
 *      n_labelled) is USED (n_used) when raw != 0 and z = (float)raw * depth_scale <= max_depth (else n_invalid) and its point, step 1 of
 *      stocs_segment_frame, has |x|, |y|, |z| < 16 (else n_far).  n_labelled = n_used + n_invalid + n_far.
 *   2. Moments, per label: n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz of q = llrint((double)v * 65536) in int64, over the used pixels,
 *      under the refit's overflow argument (|q| < 2^20, at most 2^22 pixels, every sum below 2^62): exact whatever the order.  `moments`
 *      (n_labels x 10, or NULL) returns them.
 *   3. Centroid, covariance, axes, per label in double from the moments as step 3 of stocs_segment_frame forms them (c = S / n / 65536,
 *      cov_ab = Sab / n / 2^32 - c_a c_b), all three eigenpairs by the same cyclic Jacobi (pairs (0,1), (0,2), (1,2), 12 sweeps).
 *      Eigenvalues descending, on equal values the lower column first; each axis normalised and signed so that its component of largest
 *      magnitude is positive (the lowest index on equal magnitudes); one cast to float each.  axis[k] is the k-th axis.  A non-finite
 *      value: identity axes, zero eigenvalues, flag STOCS_SHAPE_NONFINITE.  n_used == 0: a zero record, flag STOCS_SHAPE_EMPTY.
 *   4. Extents, a second pass over the used pixels, in float on the record's float centroid and axes: d = p - c,
 *      t_k = a_k0 * d.x + (a_k1 * d.y + a_k2 * d.z); lo[k], hi[k] the minimum and maximum of t_k under the order of the bits (as signed
 *      integers, negative floats with their low 31 bits inverted: -0 < +0), extent[k] = hi[k] - lo[k].
 * stocs_points_shape: the same kernels on n points (pos3, n x 3 float) as one label, every point "labelled" and used when all three of
 * |x|, |y|, |z| < 16: a model cloud's descriptor.  n == 0 is the EMPTY record; NULL pos3 (with n > 0) or shape, n < 0: STOCS_ERR_INVALID;
 * n > 2^22: STOCS_ERR_CAPACITY.
 *
 * The gate (csrc/segment_gate.h, one rule for host and device).  e1 >= e2 >= e3 the shape's extents sorted by value, m1 >= m2 >= m3 the
 * object's.  Reason bits, float, one operation each: TOO_LARGE e1 > (1 + slack) * diameter (no view of a body is wider than its diameter);
 * TOO_SMALL e1 < min_ratio * m2 (an unoccluded view of a box shows at least its middle extent; min_ratio is the room left for
 * occlusion); NO_SHAPE n_used < min_used or flags != 0.  A segment is compatible with an object when no bit is set.  The gate is not
 * exclusive: two objects of like size keep the same segments.  Defaults slack 0.25, min_ratio 0.5, min_used 3: chosen from the geometry
 * argument above, not fitted to data.  stocs_check_segment_gate_params: slack finite and >= 0, min_ratio in [0, 1], min_used >= 1,
 * reserved 0.  stocs_segment_gate is host only: reasons[k * n_labels + l] for object k and label l + 1.
 *
 * stocs_segment_assign: shapes, the gate (on the device, one lane per (object, label) pair) and the class stack in one launch sequence.
 * class_stack: n_objects images of height * width uint16, object-major, what stocs_ingest_scene_multi takes: image k holds 10000 where
 * the pixel's label is compatible with object k (used or not), else 0.  Checked in this order: (1) NULL cam, depth, labels or result:
 * STOCS_ERR_INVALID; (2) n_labels < 0 or above 2^22, width or height < 1: STOCS_ERR_INVALID; more than 2^22 pixels: STOCS_ERR_CAPACITY;
 * (3) n_objects outside 0 .. STOCS_MAX_FRAME_OBJECTS: STOCS_ERR_INVALID; (4) NULL shapes with n_labels > 0; with n_objects > 0 NULL objects,
 * class_stack, or reasons with n_labels > 0: STOCS_ERR_INVALID; (5) max_depth not finite or not above 0, gate parameters outside their range
 * (NULL with n_objects > 0: the defaults), an object's diameter or extent negative or not finite: STOCS_ERR_INVALID.  n_labels == 0 is not an
 * error: the stack comes back zero.  n_objects == 0 (objects, gate, reasons, class_stack ignored) is the shapes call alone, and
 * stocs_segment_shapes is that. ---- */
#define STOCS_SHAPE_EMPTY     1
#define STOCS_SHAPE_NONFINITE 2
#define STOCS_GATE_TOO_LARGE  1
#define STOCS_GATE_TOO_SMALL  2
#define STOCS_GATE_NO_SHAPE   4
typedef struct stocs_segment_shape {
    int32_t n_used, flags;      /* STOCS_SHAPE_*                                                                      */
    float   centroid[3];
    float   eigenvalue[3];      /* of the covariance, m^2, descending                                                 */
    float   axis[3][3];         /* axis[k]: the unit eigenvector of eigenvalue[k]                                     */
    float   lo[3], hi[3];       /* the range of (p - centroid) . axis[k] over the used pixels                         */
    float   extent[3];          /* hi - lo                                                                            */
    int32_t reserved[6];
} stocs_segment_shape;          /* 128 bytes */
typedef struct stocs_segment_shapes_result { int32_t n_labelled, n_used, n_invalid, n_far, n_out_of_range, reserved[3]; } stocs_segment_shapes_result; /* 32 bytes */
typedef struct stocs_object_size { float diameter; float extent[3]; } stocs_object_size;                    /* 16 bytes */
typedef struct stocs_segment_gate_params { float slack, min_ratio; int32_t min_used, reserved; } stocs_segment_gate_params; /* 16 bytes */
void stocs_default_segment_gate_params(stocs_segment_gate_params*);
int  stocs_check_segment_gate_params(const stocs_segment_gate_params*);       /* host only */
int  stocs_segment_gate(const stocs_segment_shape* shapes, int n_labels, const stocs_object_size* objects, int n_objects,
                        const stocs_segment_gate_params* params /* NULL: the defaults */, uint8_t* reasons /* n_objects x n_labels */);   /* host only */
int  stocs_segment_shapes(const stocs_camera* cam, const uint16_t* depth, const int32_t* labels, int n_labels, float max_depth, int device,
                          stocs_segment_shape* shapes /* n_labels */, int64_t* moments /* n_labels x 10 or NULL */, stocs_segment_shapes_result* result);
int  stocs_points_shape(const float* pos3, int n, int device, stocs_segment_shape* shape, int64_t* moments10 /* or NULL */);
int  stocs_segment_assign(const stocs_camera* cam, const uint16_t* depth, const int32_t* labels, int n_labels, float max_depth,
                          const stocs_object_size* objects, int n_objects, const stocs_segment_gate_params* gate_params, int device,
                          stocs_segment_shape* shapes, int64_t* moments, uint8_t* reasons, uint16_t* class_stack, stocs_segment_shapes_result* result);
int  stocs_segment_shapes_table(int* slots);                                  /* host only: labels a tile's LDS table holds */
/* with STOCS_SEGMENT_CLOCK=1: the HIP-event time of the calling thread's last shapes / points / assign call, every kernel of it, without
 * the copies up and down (STOCS_ERR_STATE without such a call) */
int  stocs_segment_shapes_last_device_ms(float* shapes_ms);

/* ---- files either side of the path (host code; zlib only): what the reference's constructor and driver read and
 * write through OpenCV / PCL.  stocs_png_read: 8/16-bit grey / RGB (+alpha), non-interlaced; pixels = height rows of
 * width*channels samples of bit_depth/8 bytes, 16-bit in host byte order; pixels == NULL queries the sizes.
 * stocs_ply_read: ascii or binary_little_endian vertices, x y z (+ normal_x/nx ...); pos3 == NULL queries the count.
 * stocs_ply_write: ascii, positions multiplied by `scale` as rgbd::save_as_ply does (rgbd.cpp:35-56). ---- */
int stocs_png_read(const char* path, int* width, int* height, int* channels, int* bit_depth, void* pixels, int64_t cap_bytes);
int stocs_ply_read(const char* path, float* pos3, float* nrm3, int cap, int* n, int* has_normals);
int stocs_ply_write(const char* path, const float* pos3, const float* nrm3, int n, float scale);
/* stocs_ply_read_mesh: the vertex element, then the face element of an ascii or binary_little_endian file: `property list <count type>
 * <index type> vertex_indices` (or vertex_index), any integer types; other face properties are skipped.  A polygon of k >= 3 corners
 * becomes the k - 2 triangles (0, i, i + 1) of a fan from its corner 0; one of fewer corners is STOCS_ERR_INVALID.  pos3 == NULL or
 * tris3 == NULL queries the counts (*nt then counts triangles, after the fans).  `element face 0`, or no face element, gives *nt = 0
 * and is no error.  Indices are handed on as they stand: stocs_mesh_check judges them.
 * stocs_ply_write_mesh: ascii, 9 significant digits (floats round-trip), faces as `property list uchar int vertex_indices`. */
int stocs_ply_read_mesh(const char* path, float* pos3, int cap_v, int* nv, int32_t* tris3, int cap_t, int* nt);
int stocs_ply_write_mesh(const char* path, const float* pos3, int nv, const int32_t* tris3, int nt);

/* clustering::point_to_plane_icp (pose_clustering.cpp:123-140: PCL IterativeClosestPointWithNormals, 5
 * iterations, 3.5 cm): own linearised point-to-plane ICP; T16_out maps the source cloud onto the target
 * (column-major).  Stand-alone; parity with PCL unpinned. */
int stocs_icp_point_to_plane(const float* src_pos3, int nsrc, const float* tgt_pos3, const float* tgt_nrm3, int ntgt,
                             int max_iterations, float max_correspondence_distance, int device, float* T16_out,
                             int* n_correspondences);

/* ---- pose refinement on the context: clustering::point_to_plane_icp (pose_clustering.cpp:123-140: PCL ICP with normals, 5
 * iterations, 3.5 cm; scene segment aligned onto the model) applied to n hypotheses in one call and rescored.  T16_centred_in:
 * n column-major 4x4 in the centred frame of stocs_score_transforms (centred model -> centred scene).  Source: the context's
 * centred scene points, restricted to src_idx[0 .. n_src) when src_idx != NULL (e.g. stocs_get_segment's indices in instance
 * mode; NULL: every scene point); target: the centred model with its unit normals.  Per hypothesis, exactly max_iterations
 * iterations of: nearest model point within max_correspondence_distance (lowest model index on equal distance), linearised
 * point-to-plane least squares in double, U <- [Rz Ry Rx | t] U; a hypothesis with < 6 correspondences or a singular system
 * stops and keeps its U.  Out (any pointer may be NULL): T16_centred_out = T U^-1, pose16_camera_out its camera form (as
 * stocs_get_candidates forms it), lcp_out = bitwise what stocs_score_transforms returns for T16_centred_out, n_corr_out the
 * last evaluated iteration's correspondences, iterations_out the updates applied.  Results are bitwise independent of the
 * batch a hypothesis shares.  n == 0: no-op; max_iterations == 0: inputs returned unchanged and scored; negative sizes or
 * iterations, a distance <= 0 or not finite, an index outside the scene: STOCS_ERR_INVALID; no scene: STOCS_ERR_STATE.
 * The model's correspondence grid is built at the first call and kept per distance.  One synchronisation per call.
 * Parity with PCL unpinned (pinned against oracle/ingest_oracle.py::icp). ---- */
int stocs_refine_poses(stocs_ctx* ctx, const float* T16_centred_in, int n, const int32_t* src_idx, int n_src, int max_iterations,
                       float max_correspondence_distance, float* T16_centred_out, float* pose16_camera_out, float* lcp_out,
                       int32_t* n_corr_out, int32_t* iterations_out);

/* Test and diagnosis facility of the refinement (as stocs_lcp_detail is of the scoring): the FIRST evaluation (U = I) of ONE
 * hypothesis, by the walk, the grid, the staging (LDS or global memory), the octant switch and the margins stocs_refine_poses uses
 * for that distance on this context.  Source point i = src_idx[i] (NULL: every scene point, n_src ignored), taken to the model frame
 * by T^-1 and rounded to float.  match[i]: the model index the walk chose -- the nearest centred model point by the float squared
 * distance fma(dz, dz, fma(dy, dy, dx dx)) among those below the search bound (float)(d^2 (1 + 1e-5)), THE LOWEST MODEL INDEX ON
 * EQUAL DISTANCE -- or -1 when there is none or the point lies outside the model's box widened by the distance.  counted[i]: 1 when
 * that pair passed the double test |s - t|^2 <= (double)d (double)d and entered the sums.  sums28 (may be NULL): the 21 entries of
 * the upper triangle of A^T A (row by row), the 6 of A^T b and the count, in double, summed as the solve step sums them.  A
 * hypothesis whose linear part is singular or not finite matches nothing: match -1, counted 0, sums 0.  Argument checking as
 * stocs_refine_poses (one hypothesis, never NULL; match and counted must not be NULL when there are source points).  Changes no
 * state but the refinement's workspace; synchronises. */
int stocs_refine_detail(stocs_ctx* ctx, const float* T16_centred, const int32_t* src_idx, int n_src, float max_correspondence_distance,
                        int32_t* match, uint8_t* counted, double* sums28);

/* ---- robust pose refinement on the context: stocs_refine_poses with two rejectors, a trim (keep the nearest share of the pairs)
 * and a normal gate (drop a pair whose normals disagree).  No reference counterpart: pose_clustering.hpp:24-28 declares
 * clustering::trimmed_icp and never defines it.  Everything not named here is exactly stocs_refine_poses: the source, the walk and
 * its tie rule, the double threshold test, the linearised system, the update and the freeze rules, T U^-1, the camera form, the LCP
 * rescoring, one synchronisation per call.  Per hypothesis and iteration:
 *   match      the plain walk's model index, -1 when there is none.
 *   candidate  a matched pair that passes the double distance test and, with the gate on, the normal test: ns the scene point's unit
 *              normal as the context holds it (the base scene's, never an instance-mode override), n the matched model normal; in
 *              double, one operation at a time, left to right: q = Tinv_R ns, g = U_R q, c = (g.x n.x + g.y n.y) + g.z n.z; the
 *              pair passes iff c >= (double)min_normal_cos.  g is not normalised (unit to rounding for a rigid hypothesis).
 *   rank       a candidate's rank word is the bit pattern of the float squared distance the walk minimised; any other source
 *              position has 0xFFFFFFFF.
 *   trim       n_cand = the number of candidates, k = floor((double)keep_ratio * n_cand) (exact).  KEPT are the k candidates smallest
 *              by (rank word, position i in the source list): on equal distance the lowest source position wins.  Integer set logic,
 *              independent of batch, launch shape and reduction order.
 *   sums       over the kept pairs only, by the plain kernel's expressions in the plain kernel's reduction order; the count that
 *              decides the freeze (< 6) is k.  With keep_ratio == 1 and the gate off every output is BITWISE stocs_refine_poses's.
 * Out (any pointer may be NULL): as stocs_refine_poses; n_corr_out = k of the last evaluated iteration, n_cand_out its n_cand.
 * Results are bitwise independent of the batch.  n == 0: no-op; max_iterations == 0: inputs returned unchanged and scored, counts 0.
 * STOCS_ERR_INVALID: as stocs_refine_poses, and a NULL params pointer, a keep_ratio outside (0, 1] or NaN, a min_normal_cos > 1 or
 * NaN, and a workspace demand of n * n_src * 8 bytes above STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES (n_src: the source size, every
 * scene point without src_idx; checked for every keep_ratio, though keep_ratio == 1 stores no rank words).  The workspace is grow-only
 * and freed with the context: a repeated call allocates nothing.  No host round trip between iterations. ---- */
#define STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES 1073741824 /* 1 GiB */
typedef struct stocs_refine_robust_params {
    int32_t max_iterations;               /* >= 0 */
    float   max_correspondence_distance;  /* m, > 0 and finite */
    float   keep_ratio;                   /* in (0, 1]: share of the candidate pairs kept, nearest first */
    float   min_normal_cos;               /* in [-1, 1]: gate on; < -1: gate off; > 1 or NaN: invalid */
} stocs_refine_robust_params;

int stocs_refine_poses_robust(stocs_ctx* ctx, const float* T16_centred_in, int n, const int32_t* src_idx, int n_src,
                              const stocs_refine_robust_params* params, float* T16_centred_out, float* pose16_camera_out, float* lcp_out,
                              int32_t* n_corr_out, int32_t* n_cand_out, int32_t* iterations_out);

/* Test and diagnosis facility of the robust refinement, as stocs_refine_detail is of the plain one: the FIRST evaluation (U = I) of
 * ONE hypothesis, always by the match, select and kept-accumulation kernels (keep_ratio == 1 included).  Per source position i:
 * match[i] as stocs_refine_detail; rank[i] the rank word; candidate[i] = (rank[i] != 0xFFFFFFFF); kept[i]: 1 when the pair entered
 * the sums.  *k_out, *n_cand_out: as defined above.  sums28 (k_out, n_cand_out, sums28 may be NULL): the 28 sums over the kept pairs
 * as the solve step forms them; no solve.  A hypothesis whose linear part is singular or not finite: match -1, rank 0xFFFFFFFF,
 * flags, counts and sums 0.  Argument checking as stocs_refine_poses_robust (match, candidate, kept and rank must not be NULL when
 * there are source points; max_iterations is checked and not used).  Changes no state but the workspace; synchronises. */
int stocs_refine_robust_detail(stocs_ctx* ctx, const float* T16_centred, const int32_t* src_idx, int n_src,
                               const stocs_refine_robust_params* params, int32_t* match, uint8_t* candidate, uint8_t* kept, uint32_t* rank,
                               int32_t* k_out, int32_t* n_cand_out, double* sums28);

/* The robust refinement's device workspace as it stands (address NULL and 0 bytes before the first call): a repeated call of the same
 * or a smaller size must leave both unchanged.  Either pointer may be NULL.  No device work. */
int stocs_refine_robust_workspace(stocs_ctx* ctx, void** address, uint64_t* bytes);

/* ---- pose tracking across frames: a local search around n prior poses on the context's current scene (no reference counterpart;
 * the reference detects from scratch on every frame).  Priors are CAMERA-frame poses (column-major, as stocs_get_candidates and the
 * pose file give them: only the camera frame carries over from frame to frame).  Each is taken to the centred frame on the host, in
 * float: R is kept, Rcm_r = R_r0 cm_x + (R_r1 cm_y + R_r2 cm_z), t_r = (tc_r - cs_r) + Rcm_r (cs / cm: stocs_get_centroids).
 * Round r = 0 .. rounds-1, prior p, slot j = 0 .. samples-1: slot 0 is the incumbent as it stands; slot j >= 1 is the incumbent
 * perturbed about the model centroid (the origin of the centred model): R' = R dR, t' = t + dt.  Its six draws are
 *     u_k = (rng64(seed, p * rounds + r, 8 * j + k) >> 40) * 2^-24,  k = 0 .. 5   (csrc/stocs_math.h; exact floats in [0, 1))
 *     dt_k = tau_r * (2 u_k - 1)  (k = 0, 1, 2),   v_k = h_r * (2 u_{k+3} - 1)  (k = 0, 1, 2)
 * with b_r = shrink^r (a double product, b_0 = 1), tau_r = (float)(max_translation * b_r), h_r = (float)tan(max_rotation_deg * b_r * pi
 * / 360), both in double on the host.  dR is the rotation of the unit quaternion (1, v) / sqrt(1 + |v|^2):
 *     d = 1 + (v0 v0 + (v1 v1 + v2 v2)),  s = 1 / sqrt(d),  w = s, x = v0 s, y = v1 s, z = v2 s,
 *     dR = [[1 - 2 (y y + z z), 2 (x y - w z), 2 (x z + w y)], [2 (x y + w z), 1 - 2 (x x + z z), 2 (y z - w x)],
 *           [2 (x z - w y), 2 (y z + w x), 1 - 2 (x x + y y)]]
 *     R'_ab = R_a0 dR_0b + (R_a1 dR_1b + R_a2 dR_2b),   t'_a = t_a + dt_a
 * (float, IEEE division and square root, no contraction: a float32 restatement reproduces every candidate bit for bit).  v is drawn
 * from a cube, not a ball: a sample turns by at most 2 atan(sqrt(3) h_r), i.e. up to ~1.7x the nominal bound at a corner.
 * Every candidate is scored by the context's LCP path as it stands (exact_ties included): bitwise stocs_score_transforms of its T16.
 * The next incumbent is the first maximum of the prior's slots, key (lcp bits << 32) | ~slot: ties keep the incumbent, so the lcp
 * never decreases over the rounds and lcp >= prior_lcp.  Rounds chain on the device (no host wait between them).  With
 * refine_iterations > 0 the final incumbents go through the refinement of stocs_refine_poses: refined_* are bitwise
 * stocs_refine_poses(incumbent T16, n, NULL, 0, refine_iterations, max_correspondence_distance) on the same context; without it they
 * repeat lcp / pose16 with counts 0.  A prior's results are bitwise independent of the other priors of the call (its draws depend on
 * its index p).  The context's bases, candidates and last trial batch are left as they were; tracking has its own grow-only
 * workspace (a repeated call of the same size allocates nothing) and does one pinned read-back and one synchronisation per call.
 * Limits: 1 <= rounds <= STOCS_TRACK_MAX_ROUNDS; n_priors * samples <= STOCS_TRACK_MAX_CANDIDATES per round (2^20: one round's
 * candidates stay within 64 MiB of workspace, or rounds x that with keep_details; a wider search is a detection, stocs_run_trials).
 * n_priors == 0: no-op.  A NULL pointer, a non-finite prior or one whose rotation is not orthonormal within 1e-3 (max |R^T R - I|),
 * a parameter outside its range below, or a batch over the limits: STOCS_ERR_INVALID; no scene: STOCS_ERR_STATE. ---- */
#define STOCS_TRACK_MAX_ROUNDS 64
#define STOCS_TRACK_MAX_CANDIDATES (1 << 20)
typedef struct stocs_track_params {
    int32_t  rounds;                      /* 1 .. STOCS_TRACK_MAX_ROUNDS search rounds                                 */
    int32_t  samples;                     /* >= 1 candidates per prior per round; slot 0 is the incumbent, unperturbed */
    float    max_translation;             /* m, round-0 half-edge of the translation cube (> 0, finite)                */
    float    max_rotation_deg;            /* round-0 rotation bound, degrees, in (0, 180): h_0 = tan(bound / 2)        */
    float    shrink;                      /* (0, 1]: both bounds are multiplied by it after every round                */
    uint64_t seed;
    int32_t  refine_iterations;           /* >= 0; 0: no refinement                                                    */
    float    max_correspondence_distance; /* m, > 0 and finite, as stocs_refine_poses                                  */
    int32_t  keep_details;                /* != 0: keep every round's candidates and scores for stocs_track_get_round */
} stocs_track_params;
typedef struct stocs_track_result {
    float   prior_lcp;                    /* the prior's own score (round 0, slot 0)                                   */
    float   lcp, pose16[16];              /* best after the rounds, camera frame, column-major                         */
    float   refined_lcp, refined_pose16[16];
    int32_t n_correspondences, iterations;/* stocs_refine_poses's; == lcp / pose16 and 0, 0 without refinement        */
} stocs_track_result;
int stocs_track_poses(stocs_ctx* ctx, const float* prior_pose16_camera, int n_priors, const stocs_track_params* p, stocs_track_result* out);
/* stocs_track_poses with the final incumbents refined by the trimmed, normal-gated form.  The rounds are stocs_track_poses's, bit
 * for bit (candidates, scores, incumbents, stocs_track_get_round); with refine_iterations > 0, refined_*, n_correspondences (k of
 * the last evaluated iteration) and iterations are bitwise stocs_refine_poses_robust(incumbent T16, n, NULL, 0, {refine_iterations,
 * max_correspondence_distance, keep_ratio, min_normal_cos}) on the same context; with keep_ratio == 1 and the gate off every byte of
 * every record equals stocs_track_poses's.  A prior's results stay independent of the other priors of the call; one pinned
 * read-back and one synchronisation per call.  keep_ratio / min_normal_cos: the rules of stocs_refine_robust_params (outside them:
 * STOCS_ERR_INVALID); everything else is checked as stocs_track_poses checks it.  The priors are refined in groups by the rule of
 * stocs_run_trials_post_robust (same limit, same environment variable, same independence); the workspace is grow-only. */
int stocs_track_poses_robust(stocs_ctx* ctx, const float* prior_pose16_camera, int n_priors, const stocs_track_params* p, float keep_ratio,
                             float min_normal_cos, stocs_track_result* out);
/* round `round` of prior `prior` of the last stocs_track_poses: its samples candidates (centred T16, slot order) and their scores.
 * *n = samples.  The last call did not keep details (or there was none): STOCS_ERR_STATE; prior / round out of range: STOCS_ERR_INVALID;
 * an output given and cap < samples: STOCS_ERR_CAPACITY (*n set; NULL outputs query the count). */
int stocs_track_get_round(stocs_ctx* ctx, int prior, int round, float* T16_centred, float* lcp, int cap, int* n);

/* ---- depth-image verification of pose hypotheses (no reference counterpart: the reference scores by LCP alone, which only rewards;
 * the host restatement this replaces is tools/pose_check.py::depth_agreement).  stocs_ctx_set_frame hands over the camera frame the
 * context's scene came from: depth (height*width uint16, row-major) and, optionally, the object's class-probability image (may be
 * NULL), copied to the device and kept until the next stocs_ctx_set_frame / stocs_ctx_destroy.  Independent of stocs_ctx_set_scene
 * (the caller keeps the two in step).  cam->normal_method is ignored.  NULL ctx / cam / depth, width or height < 1:
 * STOCS_ERR_INVALID.  Synchronises once.
 * stocs_depth_check_poses scores n CAMERA-frame poses (column-major, as stocs_get_candidates, stocs_trial_hypothesis::pose16 /
 * refined_pose16 and stocs_track_result::pose16 give them) against that frame in one launch.  A pose acts on the model positions as
 * handed to stocs_ctx_create and on the context's unit normals (normalised as Point3D::set_normal does).  Per hypothesis P and
 * model point m with normal k, all in float, every operation a single IEEE add / sub / mul / div / floor, no contraction
 * (R_ab = P[4b + a], t_a = P[12 + a]):
 *   1. p_a = (R_a0 m_x + (R_a1 m_y + R_a2 m_z)) + t_a,   q_a = R_a0 k_x + (R_a1 k_y + R_a2 k_z)
 *   2. facing <=> (q_0 p_0 + (q_1 p_1 + q_2 p_2)) < 0 and p_2 > 1e-6f (comparisons with NaN are false).  A pose with a non-finite
 *      entry among the twelve R_ab, t_a gives an all-zero record; so does an all-zero pose (a "no pose" record of a trial batch):
 *      neither is an error.
 *   3. a = floorf(((fx p_0) / p_2 + cx) + 0.5f), b = floorf(((fy p_1) / p_2 + cy) + 0.5f);
 *      in_image <=> facing and 0 <= a < (float)width and 0 <= b < (float)height, tested on the floats; then col = (int)a, row = (int)b.
 *   4. self_occlusion == 1: over the in_image points c0 / c1 / r0 / r1 are the min and max of col and row; the stride is
 *      s = max(cell_px, ceil(max(c1 - c0 + 1, r1 - r0 + 1) / 64)) in integers, a point's cell ((row - r0) / s) * 64 + (col - c0) / s
 *      on a 64 x 64 grid, zmin[cell] the minimum p_2 of the cell's points; self_occluded <=> p_2 > zmin[cell] + occlusion_margin.
 *      self_occlusion == 0: nothing is self-occluded.
 *   5. for the remaining in_image points: raw = depth[row * width + col]; no_depth <=> raw == 0; otherwise zo = (float)raw * depth_scale
 *      (the expression of the scene ingest's back-projection) and d = p_2 - zo:  agree <=> fabsf(d) <= tolerance;  in_front <=> d <
 *      -tolerance (the camera measured a surface BEHIND where the model should have been: a free-space violation);  behind <=> d >
 *      tolerance (hidden by something else: neutral).
 *   6. on_mask <=> agree, a class image is present and !(cp < class_threshold), cp = (float)((double)class_prob[row * width + col] *
 *      (1.0 / 10000)) as stocs_ingest_scene forms it.
 * Hence facing >= in_image == self_occluded + no_depth + agree + in_front + behind.  All counts are integer sums and the z-buffer is
 * a minimum: a hypothesis's record is bitwise independent of the batch it shares and of its position in it, and a float32
 * restatement of the six steps reproduces every count (tests/depth_check_ref.py).
 * n == 0: no-op.  NULL ctx / p / out / poses with n > 0, n < 0, a parameter outside the ranges below, a camera width or height
 * < 1: STOCS_ERR_INVALID; no frame set, or a frame whose width * height differs from what was uploaded: STOCS_ERR_STATE.  Its own
 * grow-only workspace on the context (a second call of the same size allocates nothing); one pinned read-back and one
 * synchronisation per call.  Known limit: one workgroup per hypothesis, so with n far below the number of compute units a call is
 * latency-bound. ---- */
int stocs_ctx_set_frame(stocs_ctx* ctx, const stocs_camera* cam, const uint16_t* depth, const uint16_t* class_prob);
typedef struct stocs_depth_params {
    float   tolerance;          /* m, > 0 finite: |model z - observed z| <= tolerance agrees (default 0.01)          */
    float   class_threshold;    /* finite, as stocs_ingest_scene's (default 0.10); unused without a class image      */
    int32_t self_occlusion;     /* 0: off; 1: per-hypothesis z-buffer (default 1)                                    */
    int32_t cell_px;            /* >= 1: smallest z-buffer cell edge in pixels (default 8)                           */
    float   occlusion_margin;   /* m, >= 0 finite: a point farther than its cell's nearest + margin is hidden (0.01) */
} stocs_depth_params;
typedef struct stocs_depth_result {
    int32_t facing, in_image, self_occluded, no_depth, agree, in_front, behind, on_mask;
    float   score, violation;   /* (float)agree / (float)facing, (float)in_front / (float)facing; 0 when facing == 0 */
} stocs_depth_result;
void stocs_default_depth_params(stocs_depth_params* p);
int stocs_depth_check_poses(stocs_ctx* ctx, const float* pose16_camera, int n, const stocs_depth_params* p, stocs_depth_result* out);

/* ---- pose errors against ground truth: ADD, ADD-S, model diameter (no reference counterpart; the host method this replaces is a
 * kd-tree query plus float64 products per pose).  stocs_pose_errors compares n estimated CAMERA-frame poses (column-major, as
 * stocs_depth_check_poses takes them) with ground-truth poses of the same kind: n_gt == 1, every estimate against the one ground
 * truth; n_gt == n, estimate k against ground truth k; any other n_gt is STOCS_ERR_INVALID.  Poses act on the model positions as
 * handed to stocs_ctx_create (M of them).  Per pair, all in float, every operation a single IEEE add / sub / mul / sqrt, no
 * contraction (R_ab = P[4b + a], t_a = P[12 + a]):
 *   1. p_a(i) = (R_a0 m_x + (R_a1 m_y + R_a2 m_z)) + t_a under the estimate, g_a(j) the same expression under the ground truth
 *      (step 1 of the depth check).
 *   2. D(i, j) = (dx dx) + ((dy dy) + (dz dz)),  d = p(i) - g(j).
 *   3. e_i = r(D(i, i)),  s_i = r(min_j D(i, j)); the minimum starts at +inf and is replaced only on `<`, so a NaN never wins it;
 *      r(x) = +inf for NaN, else the correctly rounded float square root; nn_i = the lowest j that attains the minimum, -1 when
 *      none does.  j = i is among the candidates with the identical expression: s_i <= e_i holds bit for bit.
 *   4. q(x) = (uint64) floor(min(x, 32768.f) * 2^32) (exact);  add_fix = sum_i q(e_i),  adds_fix = sum_i q(s_i);
 *      add = (float)((double)add_fix / 2^32 / (double)M), adds likewise;  add_max = max_i e_i,  adds_max = max_i s_i.
 *      Integer sums and maxima: a record is bitwise independent of the batch it shares, of its position there and of any reduction
 *      order, and a float32 numpy restatement reproduces every field (tests/pose_error_ref.py).
 *   5. valid = 0, zero sums and four +inf when one of the pair's two poses has a non-finite entry among the twelve R_ab, t_a, or
 *      when all sixteen entries of the estimate are zero (a trial batch's "no pose" record).  Neither is an error.
 *   6. stocs_model_diameter: max over i < j of r(D(i, j)) with both points untransformed (p = m_i, g = m_j) and step 2's expression
 *      as it stands; 0 for M == 1.  Computed on the device at the first call and kept on the context (the model is fixed per context).
 * stocs_pose_errors_detail gives e, s and nn (M entries each, any may be NULL) of ONE pair; it applies steps 1-3 to the poses as
 * given (step 5 does not apply: a non-finite pose yields +inf and -1 by the arithmetic alone).
 * Checked in this order: a NULL ctx (whatever n) and n < 0 are STOCS_ERR_INVALID; n == 0 is then a no-op that looks at no other
 * argument; with n > 0 a NULL out or pose pointer, and an n_gt other than 1 or n, are STOCS_ERR_INVALID.  stocs_pose_errors_detail:
 * a NULL ctx or pose; stocs_model_diameter: a NULL ctx or result.  Its own grow-only workspace on the context (a second
 * call of the same or a smaller size allocates nothing, stocs_device_alloc_count); on the context's stream, one pinned read-back and
 * one synchronisation per call.  stocs_last_call_timing(which = 4) gives the host steps of the last stocs_pose_errors and, with the
 * "device_clock" option on, the HIP-event time of its launches.
 * The kernel (csrc/pose_error.hip) is exact brute force: workgroups of STOCS_POSE_ERROR_THREADS threads on a grid (query chunks,
 * pairs); a chunk is STOCS_POSE_ERROR_CHUNK query points (four rows of one per thread; a chunk with fewer rows runs a loop
 * instantiated for 1, 2 or 3), and the targets pass through LDS in tiles of STOCS_POSE_ERROR_TILE points.  A call of more than
 * 65 535 pairs is several launches.  Known limit: few pairs on a small model leave most compute units idle. ---- */
#define STOCS_POSE_ERROR_THREADS 256
#define STOCS_POSE_ERROR_CHUNK 1024
#define STOCS_POSE_ERROR_TILE 1024
typedef struct stocs_pose_error {
    uint64_t add_fix, adds_fix;              /* sums of step 4 */
    float    add, add_max, adds, adds_max;   /* metres */
    int32_t  valid, reserved;
} stocs_pose_error;
int stocs_pose_errors(stocs_ctx* ctx, const float* est_pose16_camera, int n, const float* gt_pose16_camera, int n_gt, stocs_pose_error* out);
int stocs_pose_errors_detail(stocs_ctx* ctx, const float* est_pose16_camera, const float* gt_pose16_camera,
                             float* e /*M*/, float* s /*M*/, int32_t* nn /*M*/);   /* one pair; any output may be NULL */
int stocs_model_diameter(stocs_ctx* ctx, float* diameter);

/* ---- pose errors under model symmetries: MSSD, MSPD, symmetric ADD (the measures of the BOP benchmark; no reference counterpart).
 * ADD calls every pose turned about a symmetry axis wrong and ADD-S calls nearly anything that overlaps right; these take an EXPLICIT
 * set of K symmetry transforms of the model and keep the point-to-same-point distance.  stocs_pose_errors_sym compares n estimated
 * CAMERA-frame poses with ground truth (n_gt == 1 or n, as stocs_pose_errors) under K symmetries: column-major 4x4 in the MODEL frame
 * handed to stocs_ctx_create, S_ab = S[4b + a], s_a = S[12 + a]; likewise the ground truth G with t_a = G[12 + a].  Per pair and per
 * symmetry k, all in float, every operation a single IEEE add / sub / mul / div / sqrt, no contraction:
 *   0. Compose as BOP does (R_gt R_sym, R_gt t_sym + t_gt), once per (pair, k):
 *        C_ab = G_a0 S_0b + (G_a1 S_1b + G_a2 S_2b),   u_a = (G_a0 s_0 + (G_a1 s_1 + G_a2 s_2)) + t_a.
 *   1. p(i) under the estimate by step 1 of stocs_pose_errors; g^k(i) by the same expression under (C, u).
 *   2. D_k(i) by step 2 there with d = p(i) - g^k(i).
 *   3. e^k_i = r(D_k(i));  add_fix_k = sum_i q(e^k_i);  max3_k = max_i e^k_i  (r and q of stocs_pose_errors; the maximum may be taken
 *      on D with a NaN counted as +inf and rooted once: the correctly rounded root is monotone).
 *   4. Projection, only with a camera.  For a transformed point x: a = (fx x_0) / x_2 + cx,  b = (fy x_1) / x_2 + cy (the depth
 *      check's projection before its + 0.5 and floor).  P_k(i) = (da da) + (db db) with da, db the differences estimate minus
 *      ground truth; P_k(i) = +inf when !(x_2 > 1e-6f) for the point under either pose or when P is NaN.  max2_k = r(max_i P_k(i)),
 *      in pixels.  Without a camera max2_k = +inf.
 *   5. Minimum over k in index order, starting at +inf and replaced only on `<`:  mssd = min_k max3_k,  mspd = min_k max2_k;
 *      add_fix = min_k add_fix_k as integers (the start is above every sum, so k_add >= 0 for every valid pair);
 *      add = (float)((double)add_fix / 2^32 / (double)M).  k_mssd, k_mspd, k_add: the LOWEST k that attains the minimum, -1 when no
 *      k is below +inf.  Integer sums, maxima and index-ordered minima: a record is bitwise independent of the batch it shares and
 *      of any reduction order, and a float32 numpy restatement reproduces every field (tests/pose_error_sym_ref.py).
 *   6. valid = 0, a zero sum, three +inf and three -1 for the pairs that step 5 of stocs_pose_errors calls invalid.  Not an error.
 * With K = 1 and the identity, add_fix and add equal stocs_pose_errors's and mssd its add_max bit for bit for every valid pair: the
 * composition can only change signs of zero, which the squares of step 2 remove.
 * stocs_pose_errors_sym_detail gives add_fix_k, max3_k and max2_k (K entries each, any may be NULL) of ONE pair by the same kernel;
 * as in stocs_pose_errors_detail step 6 does not apply.
 * Checked in this order: a NULL ctx (whatever n) and n < 0 are STOCS_ERR_INVALID; n == 0 is then a no-op that looks at no other
 * argument; then K < 1 or K > STOCS_POSE_SYM_MAX, a NULL out, pose or symmetry pointer, an n_gt other than 1 or n, a non-finite
 * entry among a symmetry's twelve used entries, a non-finite fx, fy, cx or cy of a given camera (its other fields are not read), and a
 * workspace demand above STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES (64 n_gt K + 16 n K bytes and the poses) are STOCS_ERR_INVALID.
 * Its own grow-only workspace on the context (a second call of the same or a smaller size allocates nothing); on the context's
 * stream, poses and symmetries up through the pinned block, one read-back of n records and one synchronisation per call.
 * stocs_last_call_timing(which = 5) gives the host steps of the last stocs_pose_errors_sym and, with "device_clock" on, the
 * HIP-event time of its launches.
 * The kernels (csrc/pose_error_sym.hip): one thread per (ground truth, k) composes step 0 into device memory; a workgroup of
 * STOCS_POSE_SYM_THREADS threads owns one pair and a block of STOCS_POSE_SYM_BLOCK symmetries, whose composed poses it reads as
 * wave-uniform scalars, and walks the whole model with per-lane accumulators (grid: pairs in x, symmetry blocks in y), then stores
 * the block's per-k values: no atomics, no memset; one wavefront per pair takes step 5.
 *
 * stocs_symmetry_set (host code, no device work) writes the rotations that the clustering's symmetry descriptor names (the
 * reference's sym_info, folded into stocs_cluster_poses's rotation error).  For a descriptor on x or z the smallest plain rotation
 * error over the set equals the clustering's folded error for every turn about that axis.  For y that holds only for turns of LESS
 * than 90 degrees: the clustering takes the pitch by asin, which folds it into +-90 degrees before any symmetry is folded, so beyond
 * a quarter turn about y its error is 180 degrees whatever the descriptor, while the set holds the true rotations (Ry(100) under
 * (0, 360, 0): 180 degrees there, 0 here).  A clustering with a y descriptor and these errors can disagree beyond that.  Per axis d the angle list is the multiples of 90 degrees
 * for sym3[d] == 90, {0, 180} for 180, 360 j / n_continuous (j = 0 .. n_continuous - 1; n_continuous < 1 is invalid there) for 360,
 * {0} otherwise.  The set is T(c) Rz(gamma) Ry(beta) Rx(alpha) T(-c) over the three lists -- the Euler order of the clustering's
 * quaternion_to_euler -- with the x angle running fastest, so entry 0 is the identity; c = center3 (NULL: the origin).  Entries are
 * computed in double and rounded once; angles that are multiples of 90 degrees give exactly 0 and +-1.  *K always receives the count;
 * cap < K (or a NULL out16) is STOCS_ERR_INVALID and writes nothing.  With more than one non-trivial axis the product list need NOT
 * be a group (it is not closed under composition in general, and may name one rotation twice); pass an explicit list to
 * stocs_pose_errors_sym instead where that matters. ---- */
#define STOCS_POSE_SYM_MAX 4096
#define STOCS_POSE_SYM_THREADS 256
#define STOCS_POSE_SYM_BLOCK 4
typedef struct stocs_pose_error_sym {
    uint64_t add_fix;                       /* min over k of the step-3 sum */
    float    add, mssd, mspd, reserved_f;   /* metres, metres, pixels, 0 */
    int32_t  k_add, k_mssd, k_mspd, valid;  /* the lowest k that attains each minimum; -1: none */
} stocs_pose_error_sym;                     /* 40 bytes */
int stocs_pose_errors_sym(stocs_ctx* ctx, const float* est_pose16_camera, int n, const float* gt_pose16_camera, int n_gt,
                          const float* sym16_model, int K, const stocs_camera* cam /* NULL: no MSPD */, stocs_pose_error_sym* out);
int stocs_pose_errors_sym_detail(stocs_ctx* ctx, const float* est_pose16_camera, const float* gt_pose16_camera, const float* sym16_model, int K,
                                 const stocs_camera* cam, uint64_t* add_fix /*K*/, float* max3 /*K*/, float* max2 /*K*/);
int stocs_symmetry_set(const float sym3[3], int n_continuous, const float* center3 /* NULL: origin */, float* out16, int cap, int* K);

/* ---- finding a model's symmetries: self-distance of the model under K transforms, candidate axes, closure, the search (no
 * reference counterpart).  stocs_symmetry_errors scores K transforms of the MODEL frame (column-major 4x4 as sym16_model of
 * stocs_pose_errors_sym, S_ab = S[4b + a], s_a = S[12 + a]) by how well the transformed model lies on the untransformed one.  The
 * points m_i are those handed to stocs_ctx_create, the normals n_i those normals as the context keeps them: divided by their float
 * length (x x + (y y + z z), correctly rounded root, three divisions) where that length's square is > 0, else as given.  Per transform,
 * all in float, every operation a single IEEE add / sub / mul / sqrt, no contraction (r and q of stocs_pose_errors):
 *   1. p(i) = step 1 of stocs_pose_errors under S;  D(i, j) = step 2 there with d = p(i) - m_j (the target is NOT transformed).
 *   2. Dmin_i = min_j D(i, j), starting at +inf and replaced only on `<`; nn_i the lowest j that attains it.  Point i is MATCHED iff
 *      Dmin_i <= reach * reach (one float product, inclusive) and Dmin_i < +inf, else FAR.  Detail of a far point: nn_i = -1, s_i = +inf, dot_i = 0.
 *   3. s_i = r(Dmin_i) for matched points;  c_i = s_i if matched, else reach;  sum_fix = sum over ALL i of q(c_i);
 *      mean = (float)((double)sum_fix / 2^32 / (double)M);  max = max of s_i over matched points, 0 when there are none;
 *      n_far = the count of far points.
 *   4. n'_a = S_a0 n_x + (S_a1 n_y + S_a2 n_z) of point i's normal, t the normal of target nn_i:
 *      dot_i = n'_x t_x + (n'_y t_y + n'_z t_z);  n_normal_bad counts the matched points with !(dot_i >= cos_normal): a NaN is bad.
 *   Integer sums, maxima taken on bits: a record is bitwise independent of the batch it shares, of its position there and of any
 *   reduction order; valid = 1, reserved = 0.  tests/symmetry_ref.py restates it in float32 numpy.
 * Identity with stocs_pose_errors_detail: with the identity as ground truth g(j) there is m_j up to the sign of zero, which the squares
 * of step 2 remove, so stocs_pose_errors_detail(S, I) yields s and nn from the identical expressions: wherever a point is matched this
 * call's s_i and nn_i equal them bit for bit.
 * stocs_symmetry_errors_detail gives s, nn and dot (M entries each, any may be NULL) of ONE transform.
 * Checked in this order: a NULL ctx and K < 0 are STOCS_ERR_INVALID; K == 0 is then a no-op that looks at no other argument; a NULL
 * transform, parameter or result pointer, a non-finite entry among a transform's twelve used entries, !(reach > 0), a non-finite
 * reach or one whose float square is below the smallest normal float (about 1.1e-19 m: the squares of step 1 would underflow), and a workspace demand (96 K bytes) above STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES are STOCS_ERR_INVALID (the detail form: a
 * NULL ctx, transform or parameters, the same value checks).  cos_normal is not checked: NaN calls every matched point bad.
 * The grid.  The target never moves, so it is binned once per (context, reach) on the host into a uniform grid over the model's
 * bounding box: cell starts plus the points sorted by cell, uploaded into a grow-only block of this feature's own; another reach
 * rebuilds it.  A second call at the same reach and the same or a smaller K allocates nothing (stocs_device_alloc_count).
 * Cell edge h = (float) max(reach * 65 / 64, largest box extent / STOCS_SYMMETRY_GRID_SPAN) in double, inv = 1.f / h; the cell of x
 * along axis a is floorf((x_a - o_a) * inv), o the box minimum: ONE float expression (csrc/symmetry.h) that the host runs on the
 * targets and the device on the queries.  The walk over the 27 cells about a query's cell misses no target with D <= reach * reach:
 * the comment in csrc/symmetry.h gives the argument.  Cells are visited in no index order, so the running minimum is kept on (D, j)
 * keys.  A query outside the box finds fewer cells or none; the normals are read once per query by index.
 * The kernel (csrc/symmetry.hip): a workgroup of STOCS_SYMMETRY_THREADS threads owns one transform, read as wave-uniform scalars; a
 * lane takes the queries tid, tid + STOCS_SYMMETRY_THREADS, ...; per-lane accumulators are reduced once (shuffles, LDS) and stored
 * plainly: no atomics, no memset.  A call of more than STOCS_SYMMETRY_MAX_LAUNCH transforms is several launches.  On the context's
 * stream: one upload through the pinned block, one read-back of K records, one synchronisation.  stocs_last_call_timing(which = 6)
 * gives the host steps of the last stocs_symmetry_errors and, with "device_clock" on, the HIP-event time of its launches.
 *
 * Host helpers (no device work):
 * stocs_symmetry_axes writes n_axes >= 3 candidate directions: entries 0, 1, 2 are exactly x, y, z; entry 3 + k (k = 0 .. L - 1,
 * L = n_axes - 3) is the Fibonacci lattice point of the hemisphere z > 0:  z = 1 - (k + 0.5) / L,  phi = k * pi * (3 - sqrt(5)),
 * (sqrt(1 - z z) cos phi, sqrt(1 - z z) sin phi, z), normalised, all in double, rounded once.  The lattice's spacing is taken as
 * sqrt(2 pi / L) radians (the square root of the area per point).  n_axes < 3 is STOCS_ERR_INVALID with *n = 0; otherwise *n always
 * receives n_axes, and cap < n_axes or a NULL axes3 is STOCS_ERR_INVALID and writes nothing else.
 * stocs_symmetry_rotation writes T(c) R T(-c), R the Rodrigues rotation c I + s [a]x + (1 - c) a a^T by angle_deg about axis3
 * normalised in double (a zero or non-finite axis or angle or centre: STOCS_ERR_INVALID), c = center3 (NULL: origin); computed in double
 * and rounded once, no -0 entries; an angle that is a multiple of 90 degrees takes cos and sin exactly from {0, +-1}, so about a
 * coordinate axis the entries are exactly 0 and +-1 as stocs_symmetry_set's are.
 * stocs_symmetry_close closes n_gen generators under composition, breadth first: the list starts with the identity; for every kept
 * entry g in list order and every generator h in the order given, the product h g (in double, on the generators widened once) is
 * appended when it is NEW.  NEW: against every kept entry either the relative rotation exceeds same_deg (its trace is below
 * 1 + 2 cos same_deg) or the translations differ by more than same_deg in radians times the largest translation norm among the
 * generators.  Entries are rounded once on output, entry 0 is the identity, the order is deterministic.  It stops at cap
 * (1 .. STOCS_POSE_SYM_MAX; outside: STOCS_ERR_INVALID) with *truncated = 1 when a new entry found no room -- two continuous axes, as
 * on a sphere, do that; not an error.  *K receives the count written.  n_gen == 0 gives the identity alone.
 *
 * stocs_find_symmetries: deterministic host logic around batched stocs_symmetry_errors calls with reach = tol_max and the search's
 * cos_normal.  c = center3, or with NULL the centroid of the model points summed in double in index order, rounded once to float.
 * G(a, n) is stocs_symmetry_rotation(a, 360 / n (double), c).  tol_max <= 0 stands for 0.1f * stocs_model_diameter.
 *   1. Coarse pass.  Every direction d of stocs_symmetry_axes(n_axes) with every order n = 2 .. max_order, candidate index
 *      d * (max_order - 1) + (n - 2), scored in ONE call; ranked by (mean, index) ascending.
 *   2. Refinement.  Walk the ranking and keep a candidate when its axis is more than same_deg from every kept axis, up to sign, until
 *      n_refine are kept.  Then `rounds` rounds, each ONE scoring call for all kept candidates: round r = 0 .. rounds - 1 has the
 *      half-angle theta = spacing / 2^r (spacing of the lattice as above; n_axes == 3: pi / 4).  About the current axis a (float,
 *      widened): e = the coordinate axis of smallest |a_e| (lowest index on ties), u = normalise(e - (e . a) a), v = a x u; direction
 *      k = 0 .. n_local - 1 is normalise(a + tan(theta sqrt((k + 0.5) / n_local)) (cos(k g) u + sin(k g) v)), g = pi (3 - sqrt 5),
 *      in double, rounded once; each is scored at the candidate's own order.  The candidate moves to the direction of lowest mean when
 *      that is `<` its current mean (lowest k on ties).
 *   3. Decision.  Every kept axis with every order 2 .. max_order in ONE call.  Order n PASSES iff n_far == 0, max <= tol_max and
 *      (float)n_normal_bad <= max_normal_bad * (float)M.  The axis's order is the largest passing n, 0 (continuous) when every n
 *      passes; an axis where none passes is dropped.  Its max, mean and n_normal_bad are those of that n (continuous: of max_order).
 *      Axes sorted by (mean, kept rank); one nearer than same_deg, up to sign, to an axis before it is dropped.
 *   4. Output.  The axes best first (*n_axes receives their count; at most cap_axes are written).  The set is stocs_symmetry_close of
 *      the generators G(a, order), a continuous axis giving G(a, n_continuous), whose powers are its n_continuous steps, with the
 *      tolerance min(same_deg, 90 / n_continuous) and cap min(cap_set, STOCS_POSE_SYM_MAX).  sym3 is the clustering descriptor when
 *      every axis lies within same_deg of a coordinate axis, up to sign, and has an order the descriptor names (2 -> 180, 4 -> 90,
 *      continuous -> 360) and no two axes lie that near the SAME coordinate axis (two axes more than same_deg apart can); otherwise sym3 is zeros and flags carries
 *      STOCS_SYMMETRY_DESCRIPTOR_INEXACT.  For a y descriptor the caveat at stocs_symmetry_set applies.  STOCS_SYMMETRY_SET_TRUNCATED:
 *      the closure stopped at its cap.  STOCS_SYMMETRY_NOTHING_FOUND: no axis; then K = 1, the identity, sym3 zeros.
 * Defaults (stocs_default_symmetry_search): tol_max 0, cos_normal cos 30 degrees (the LCP's), max_normal_bad 1 (the count is reported,
 * not used), n_axes 2048, max_order 6, n_continuous 72, n_refine 16, n_local 32, rounds 4, same_deg 6 (2 sin 6 degrees x half a diameter is 0.1 diameter: an axis farther off than that moves
 * the model's rim by more than the default tolerance under a half turn).  Refused (STOCS_ERR_INVALID):
 * NULL ctx, search, n_axes, K, sym3 or flags pointer; axes NULL with cap_axes > 0; set16 NULL or cap_set < 1; n_axes < 3, max_order
 * < 2, n_continuous < 1, n_refine < 1, n_local < 1, rounds < 0, !(same_deg > 0), a non-finite tol_max or centre. ---- */
#define STOCS_SYMMETRY_THREADS 256
#define STOCS_SYMMETRY_MAX_LAUNCH 65535
#define STOCS_SYMMETRY_GRID_SPAN 60
#define STOCS_SYMMETRY_DESCRIPTOR_INEXACT 1
#define STOCS_SYMMETRY_SET_TRUNCATED 2
#define STOCS_SYMMETRY_NOTHING_FOUND 4
typedef struct stocs_symmetry_params { float reach; float cos_normal; int32_t reserved[2]; } stocs_symmetry_params;
typedef struct stocs_symmetry_error {
    uint64_t sum_fix;          /* sum over ALL i of q(c_i) */
    float    mean, max;        /* metres */
    int32_t  n_far, n_normal_bad;
    int32_t  valid, reserved;
} stocs_symmetry_error;        /* 32 bytes */
int stocs_symmetry_errors(stocs_ctx* ctx, const float* sym16_model, int K, const stocs_symmetry_params* p, stocs_symmetry_error* out);
int stocs_symmetry_errors_detail(stocs_ctx* ctx, const float* sym16_model /* one */, const stocs_symmetry_params* p,
                                 float* s /*M*/, int32_t* nn /*M*/, float* dot /*M*/);   /* any output may be NULL */
int stocs_symmetry_axes(int n_axes, float* axes3, int cap, int* n);
int stocs_symmetry_rotation(const float axis3[3], double angle_deg, const float* center3 /* NULL: origin */, float out16[16]);
int stocs_symmetry_close(const float* gen16, int n_gen, float same_deg, float* out16, int cap, int* K, int* truncated);
typedef struct stocs_symmetry_search {
    float tol_max;          /* metres; <= 0: 0.1 x stocs_model_diameter, the project's recall threshold */
    float cos_normal;       /* gate of the count */
    float max_normal_bad;   /* accepted share of the model's points failing the gate */
    int32_t n_axes;         /* coarse directions */
    int32_t max_order;      /* discrete orders 2 .. max_order */
    int32_t n_continuous;   /* steps of a continuous axis in the set */
    int32_t n_refine, n_local, rounds;   /* axes refined, directions per cone, halvings */
    float same_deg;         /* axes / transforms nearer than this are one */
} stocs_symmetry_search;
typedef struct stocs_symmetry_axis { float axis[3]; int32_t order; /* 0: continuous */ float max, mean; int32_t n_normal_bad, reserved; } stocs_symmetry_axis;
void stocs_default_symmetry_search(stocs_symmetry_search* s);
int stocs_find_symmetries(stocs_ctx* ctx, const stocs_symmetry_search* s, const float* center3 /* NULL: centroid */,
                          stocs_symmetry_axis* axes, int cap_axes, int* n_axes, float* set16, int cap_set, int* K, float sym3[3], int* flags);

/* ---- multi-instance selection (no reference counterpart: the reference returns one pose per object).  Of n hypotheses, which are
 * distinct instances and which are one instance found twice: walk them best first and keep one only if enough of the scene points it
 * explains are not explained by one kept before it.  stocs_select_instances takes n CENTRED-frame hypotheses (column-major, as
 * stocs_score_transforms and stocs_refine_poses take them).  Integer set logic over the scoring kernel's match records; csrc/instances.hip,
 * restated in numpy in tests/instances_ref.py, equal bit for bit:
 *   1. Explained set.  E_h = { hit[i] : counted[i] != 0 } over the model points i, hit / counted being the records stocs_lcp_detail(T_h)
 *      returns (exact_ties honoured): the distinct scene indices the context's own LCP launch counts for T_h.  Several model points
 *      on one scene point count once; a hit that fails the normal test does not count.  own_h = |E_h|; lcp_h is that launch's score.
 *   2. Invalid hypotheses.  One with a non-finite entry among its 16, or with all 16 zero (the "no pose" record of a trial batch), has
 *      own = 0, lcp = 0 and is never selected.  It is not scored as a transform (the zero matrix maps the model onto the centroid).
 *   3. Order.  Descending stocs_pack_best(lcp_h, h): higher score first, lower index first on equal score.  Scores that are not
 *      positive (or NaN) all pack to 0 and come last, lower index first.
 *   4. Walk.  In that order, covered = {} at the start, excl = |E_h \ covered|.  h is selected when excl >= min_points, and
 *      (float)excl >= min_exclusive_fraction * (float)own_h (one IEEE float multiply, one compare, no contraction), and fewer than
 *      max_instances are selected so far.  On selection covered |= E_h and h takes the next rank (0, 1, ...).
 *   5. Output.  out[h] = { rank (-1: not selected), own, exclusive, lcp }.  exclusive of a selected hypothesis is excl at its selection;
 *      of an unselected one |E_h \ covered_final|, what the chosen set leaves unexplained.  *n_selected (<= min(max_instances, n)) and
 *      their indices in rank order in selected[] (capacity max_instances, or n if that is smaller).
 * covered only grows, so a hypothesis that fails against the cover of some of its predecessors fails for good: the kernel tests
 * sixteen pending hypotheses per round and the results above do not depend on that.  A hypothesis's own and lcp are bitwise independent
 * of the batch it shares.
 * n == 0: STOCS_OK, nothing selected.  NULL ctx / p / n_selected, NULL T16 / out / selected with n > 0, n < 0 or n > 16 384,
 * max_instances < 1, min_points < 1, a fraction that is NaN, <= 0 or > 1: STOCS_ERR_INVALID.  No scene or no model on the context:
 * STOCS_ERR_STATE.  A scene of more than 2^18 points: STOCS_ERR_CAPACITY (the explained sets are 32 KB bitsets in LDS).
 * The detail rows are produced in chunks of hypotheses (256 MB of rows, as stocs_lcp_hit_count; STOCS_INSTANCES_CHUNK=<hypotheses> in
 * the environment forces a chunk size).  Poses go up through the context's pinned block, everything runs on the context's stream,
 * one pinned read-back and one synchronisation per call; own grow-only workspace on the context (a second call of the same or a
 * smaller size allocates nothing).
 * stocs_select_instances_rows runs steps 1 (the set arithmetic), 3, 4 and 5 on GIVEN detail rows: host arrays hit[n * nM],
 * counted[n * nM], lcp[n] over nS scene points (nM, nS >= 1); step 2 does not apply.  It needs a context for the device and the
 * workspace only, not its scene.  A counted row whose hit is negative or >= nS is STOCS_ERR_INVALID, checked on the host before
 * anything is uploaded.  nS > 2^18: STOCS_ERR_CAPACITY.  A test and diagnosis facility (pageable copies). ---- */
typedef struct stocs_instance_params {
    int32_t max_instances;            /* >= 1: stop after this many (default 16)                                              */
    int32_t min_points;               /* >= 1: scene points a hypothesis must explain that no selected one explains (default 20) */
    float   min_exclusive_fraction;   /* in (0, 1]: ... as a share of all it explains (default 0.5)                           */
} stocs_instance_params;
typedef struct stocs_instance_result {
    int32_t rank, own, exclusive;
    float   lcp;
} stocs_instance_result;
void stocs_default_instance_params(stocs_instance_params* p);
int stocs_select_instances(stocs_ctx* ctx, const float* T16_centred, int n, const stocs_instance_params* p, stocs_instance_result* out,
                           int32_t* selected, int* n_selected);
int stocs_select_instances_rows(stocs_ctx* ctx, const int32_t* hit, const uint8_t* counted, const float* lcp, int n, int nM, int nS,
                                const stocs_instance_params* p, stocs_instance_result* out, int32_t* selected, int* n_selected);

/* ---- joint rendering of poses: instance masks, visibility, depth agreement (no reference counterpart).  stocs_depth_check_poses judges
 * every hypothesis alone; these entry points splat the model points of many poses -- of one context, or of several contexts one call
 * after another -- into ONE frame-sized key buffer, so that a pose standing in front of another hides it, and read the result back per
 * instance and per pixel.  The frame is the one stocs_ctx_set_frame uploaded; poses are CAMERA-frame and column-major, as for
 * stocs_depth_check_poses.  csrc/render.hip, restated in float32 numpy in tests/render_ref.py, equal bit for bit.
 * The key buffer: width*height uint64_t on the device, row-major; empty is all ones.  The caller allocates it (stocs_dev_alloc of any
 * context on the same device serves).  Several contexts, one per object, may render into the same buffer one call after another.
 * The splat rule, used by every entry point below.  Hypothesis h has id = id_base + h (id_base >= 0, id_base + n <= 2^31 - 1).  Each
 * model point goes through steps 1-3 of the depth-check contract above, unchanged.  If the point is in_image:
 *   s = (int)fminf(floorf((fx * point_radius) / p_2 + 0.5f), (float)max_splat_px)   (float, one IEEE operation at a time; fx serves both axes)
 * and the point touches every pixel (row + dy, col + dx) with |dy|, |dx| <= s that lies inside the image (tested on integers).  A pose
 * with a non-finite entry among its twelve used entries, or the all-zero "no pose" record, touches nothing and is no error.
 *   1. stocs_render_poses: with clear != 0 the buffer is filled with empty first; then every touched pixel gets
 *      key = min(key, (uint64_t)bits(p_2) << 32 | id).  p_2 > 1e-6, so the float's bits keep its order: the nearest surface wins and on
 *      an equal depth the lower id.  A minimum: the result does not depend on execution order, on the batch, or on the order of calls.
 *      Synchronises its stream before it returns, so that another context may continue on the buffer.
 *   2. stocs_render_resolve: called with the same poses and ids after every render into the buffer is done.  C_h is the set of distinct
 *      pixels h touches, footprint = |C_h|.  A pixel of C_h whose key's low word is not h's id is hidden (an empty key too); otherwise it is
 *      visible and, with z = the float in the key's high word, classified by steps 5-6 of the depth-check contract with p_2 := z:
 *      no_depth, agree, in_front, behind, on_mask.  footprint == visible + hidden, visible == no_depth + agree + in_front + behind.
 *   3. stocs_render_labels: per pixel, labels (host, width*height int32) = -1 for an empty key, else its id; state (host, width*height
 *      uint8, may be NULL) = 0 empty, 1 no_depth, 2 agree, 3 in_front, 4 behind, plus 16 when on_mask, classified as in 2.
 *   4. stocs_explain_poses, the single-object form: the context's own key buffer, id_base 0; clear, render, resolve, and labels / state when
 *      `labels` is given (state alone is ignored).  One pinned read-back and one synchronisation; a second call of the same size
 *      allocates nothing.
 * n == 0: no-op (nothing is cleared either); stocs_explain_poses with n == 0 and labels given still returns the all-empty label image
 * (it needs the frame for its size, nothing else).  NULL ctx; NULL poses / p / key buffer / out with n > 0; NULL key buffer / p / labels
 * for stocs_render_labels; n < 0; a parameter outside the ranges below; an id outside 0 .. 2^31 - 2: STOCS_ERR_INVALID.  No frame set, or
 * a frame whose width * height differs from what was uploaded: STOCS_ERR_STATE.  stocs_render_resolve or stocs_explain_poses (n > 0) on a
 * frame of more than 2^19 pixels: STOCS_ERR_CAPACITY (the footprint is a 64 KB bitset in LDS); render and labels take any frame.  Poses go
 * up and results come back through the context's pinned block, everything runs on the context's stream, every call synchronises once;
 * own grow-only workspace on the context.  Known limits: a point's whole splat is written by one lane; resolve is one workgroup per
 * hypothesis, so with n far below the number of compute units it is latency-bound. ---- */
typedef struct stocs_render_params {
    float   point_radius;      /* m, >= 0 finite: radius of the disc a model point stands for (default 0.005)                  */
    int32_t max_splat_px;      /* 0..16: largest splat half-width in pixels (default 8)                                        */
    float   tolerance;         /* m, > 0 finite: |rendered z - observed z| <= tolerance agrees (default 0.01)                  */
    float   class_threshold;   /* finite, as stocs_ingest_scene's (default 0.10); unused without a class image                 */
} stocs_render_params;
typedef struct stocs_render_result {
    int32_t footprint, visible, hidden, no_depth, agree, in_front, behind, on_mask;
} stocs_render_result;
void stocs_default_render_params(stocs_render_params* p);
int stocs_render_poses(stocs_ctx* ctx, const float* pose16_camera, int n, int id_base, const stocs_render_params* p, void* d_zkey, int clear);
int stocs_render_resolve(stocs_ctx* ctx, const float* pose16_camera, int n, int id_base, const stocs_render_params* p, const void* d_zkey,
                         stocs_render_result* out);
int stocs_render_labels(stocs_ctx* ctx, const void* d_zkey, const stocs_render_params* p, int32_t* labels, uint8_t* state);
int stocs_explain_poses(stocs_ctx* ctx, const float* pose16_camera, int n, const stocs_render_params* p, stocs_render_result* out,
                        int32_t* labels, uint8_t* state);

/* ---- scene-level selection across objects on the pixels of the depth image (no reference counterpart).  stocs_select_instances works on
 * scene-point indices, which every context numbers for itself; stocs_depth_check_poses and stocs_render_resolve judge poses somebody chose.
 * The one index space all contexts of a frame share is its pixels: these entry points give every hypothesis of every object the set of
 * depth pixels it claims, and walk the pool best first, keeping a hypothesis only if enough of its pixels are claimed by none kept before
 * it.  csrc/scene.hip, restated in float32 numpy and integer set logic in tests/scene_ref.py, equal bit for bit.
 * Pixel rows.  A frame of W x H has npix = W*H pixels; a row is Wr = ceil(npix / 32) rounded up to a multiple of 4 uint32_t words; pixel
 * i = row*W + col is bit i & 31 of word i >> 5; padding bits are zero.  stocs_scene_row_words(width, height) returns Wr (0 when either is
 * < 1).  A pool is n_slots * Wr words of device memory the caller allocates (stocs_dev_alloc of any context on the device); several
 * contexts write into one pool, one call after another.
 *   1. stocs_scene_footprints: n CAMERA-frame poses (column-major, as for stocs_depth_check_poses) of this context's model against the frame
 *      of stocs_ctx_set_frame; hypothesis h goes to slot slot_base + h.  Every model point goes through steps 1-3 of the depth-check contract,
 *      then the splat rule of the render contract, unchanged.  Z_h(pixel) = the minimum p_2 over the points of pose h ALONE that touch the
 *      pixel: the float in the key stocs_render_poses leaves when this one pose is rendered into a cleared buffer.  Every touched pixel is
 *      classified by steps 5-6 of the depth-check contract with p_2 := Z_h.  out[h] = { footprint, no_depth, agree, in_front, behind, on_mask,
 *      claimed }: footprint == no_depth + agree + in_front + behind, claimed = the popcount of the row.  The row holds the agree pixels
 *      (claim == 0) or the on_mask pixels (claim == 1).  The whole row, padding included, is always written: the pool need not be cleared,
 *      and slots outside [slot_base, slot_base + n) are not touched.  A pose with a non-finite entry among its twelve used entries, or the
 *      all-zero "no pose" record, gives an all-zero record and an all-zero row and is no error.  The record of h equals the record
 *      stocs_explain_poses returns for that pose alone (hidden == 0, visible == footprint).  Bitwise independent of the batch, of the
 *      position in it and of the chunking (hypotheses are processed in chunks of 256 MB of z-buffers; STOCS_SCENE_CHUNK=<hypotheses> in the
 *      environment forces a size).
 *      n == 0: no-op.  NULL ctx; NULL poses / p / rows / out with n > 0; n < 0; claim other than 0 or 1; slot_base < 0;
 *      slot_base + n > n_slots; a parameter outside the ranges of stocs_render_params: STOCS_ERR_INVALID.  No frame set, or a frame whose
 *      width * height differs from what was uploaded: STOCS_ERR_STATE.  npix > 2^19: STOCS_ERR_CAPACITY (so that step 2 can walk every pool).
 *      Poses go up and records come back through the context's pinned block, everything runs on the context's stream, one
 *      synchronisation; own grow-only workspace on the context (a second call of the same or a smaller size allocates nothing).
 *   2. stocs_scene_select: slots 0 .. n-1 of the pool, host arrays score[n], group[n] (0 .. n_groups-1, e.g. the object), rec[n] (step 1's
 *      records), group_cap[n_groups] (>= 1 each; NULL: no cap).  It needs a context for the device and the workspace only, neither its
 *      scene nor its frame.  own_h = the popcount of row h, counted on the device and not trusted from rec.
 *      Eligible: score_h > 0 (NaN is not), own_h >= min_pixels, and (float)rec[h].in_front <= max_violation_fraction * (float)rec[h].footprint
 *      (one IEEE float multiply, one compare, no contraction).
 *      Order: descending stocs_pack_best(score_h, h): higher score first, lower slot first on equal score; scores that are not positive
 *      (or NaN) pack to 0 and come last, lower slot first.
 *      Walk: in that order, covered = {} and cnt[g] = 0 at the start, excl = |A_h \ covered|.  h is selected when it is eligible,
 *      cnt[group_h] < group_cap[group_h], fewer than max_selected are selected so far, excl >= min_pixels and
 *      (float)excl >= min_exclusive_fraction * (float)own_h.  On selection covered |= A_h, ++cnt[group_h], and h takes the next rank.
 *      Output: out[h] = { rank (-1: not selected), own, exclusive, reason }.  exclusive of a selected slot is excl at its selection, of an
 *      unselected one |A_h \ covered_final|.  reason, decided from the FINAL state, the first that applies: 0 selected, 1 not eligible,
 *      2 exclusive fails min_pixels or the fraction against the final cover, 3 its group is full at the end, 4 max_selected was reached.
 *      selected[] (capacity max_selected, or n if that is smaller) lists the slots in rank order, *n_selected their count.
 *      The cover and the counts only grow, so a slot that fails at its turn fails for good: the kernel tests sixteen pending slots per
 *      round and the results above do not depend on that.
 *      NULL ctx / p / n_selected; NULL rows / score / group / rec / out / selected with n > 0; n < 0 or n > 16 384; width or height < 1;
 *      n_groups < 1 or > 1024; a group id outside 0 .. n_groups-1; a cap < 1; a negative count in rec; max_selected < 1; min_pixels < 1;
 *      a min_exclusive_fraction that is NaN, <= 0 or > 1; a max_violation_fraction that is NaN, < 0 or > 1: STOCS_ERR_INVALID.
 *      npix > 2^19: STOCS_ERR_CAPACITY (the cover is a 64 KB bitset in LDS).  n == 0 (after those checks): STOCS_OK, nothing selected.
 *      One pinned read-back and one synchronisation per call; a second call of the same or a smaller size allocates nothing.
 * Known limits: the classification walks the whole frame of every hypothesis; the walk is one workgroup, so its time grows with
 * rounds x Wr. ---- */
typedef struct stocs_scene_record {
    int32_t footprint, no_depth, agree, in_front, behind, on_mask, claimed;
} stocs_scene_record;
typedef struct stocs_scene_params {
    int32_t max_selected;             /* >= 1: stop after this many (default 64)                                              */
    int32_t min_pixels;               /* >= 1: pixels a hypothesis must claim that no selected one claims (default 50)        */
    float   min_exclusive_fraction;   /* in (0, 1]: ... as a share of all it claims (default 0.5)                             */
    float   max_violation_fraction;   /* in [0, 1]: largest in_front / footprint of an eligible hypothesis (default 0.2)      */
} stocs_scene_params;
typedef struct stocs_scene_result {
    int32_t rank, own, exclusive, reason;
} stocs_scene_result;
void stocs_default_scene_params(stocs_scene_params* p);
int stocs_scene_row_words(int width, int height);
int stocs_scene_footprints(stocs_ctx* ctx, const float* pose16_camera, int n, int slot_base, int n_slots, const stocs_render_params* p, int claim,
                           void* d_rows, stocs_scene_record* out);
int stocs_scene_select(stocs_ctx* ctx, const void* d_rows, int n, int width, int height, const float* score, const int32_t* group,
                       const stocs_scene_record* rec, int n_groups, const int32_t* group_cap, const stocs_scene_params* p, stocs_scene_result* out,
                       int32_t* selected, int* n_selected);

/* ---- visible-surface discrepancy (VSD, the third measure of the BOP benchmark) and the surfel depth renderer under it (no reference
 * counterpart).  MSSD, MSPD and ADD compare model points; VSD compares what the camera would see: the rendered surface of the estimate
 * and of the ground truth, each only where it is visible in the frame's depth image.  It needs no symmetry set.  The splats of the render
 * contract above are screen-aligned squares at the constant depth of their centre: masks, not a surface.  Here a model point is an
 * oriented disc (a surfel) of radius surfel_radius, ray-cast per pixel.  The frame is the one stocs_ctx_set_frame uploaded; poses are
 * CAMERA-frame, column-major, and act on the model as in the depth check.  csrc/vsd.hip, restated in float32 numpy in tests/vsd_ref.py,
 * equal bit for bit.  All in float, every operation one IEEE add / sub / mul / div / floor / correctly rounded sqrt, no contraction.
 * The surfel rule.  A model point goes through steps 1-3 of the depth-check contract, unchanged: p, q, facing, in_image, col, row, and
 * f = q_0 p_0 + (q_1 p_1 + q_2 p_2), the facing expression itself.  For an in_image point:
 *   s = (int)fminf(floorf((fx * surfel_radius) / p_2 + 0.5f), (float)max_splat_px)   (the splat rule's s with surfel_radius)
 * and for every pixel (r, c) with |r - row|, |c - col| <= s inside the image (tested on integers):
 *   xn = ((float)c - cx) / fx,  yn = ((float)r - cy) / fy                 the pixel's ray (xn, yn, 1)
 *   dn = q_0 xn + (q_1 yn + q_2);                  hit only if dn < 0     the ray meets the disc's front
 *   z  = f / dn;                                   hit only if z > 1e-6f  where the ray meets the disc's plane
 *   ex = xn z - p_0,  ey = yn z - p_1,  ez = z - p_2
 *   hit only if (ex ex) + ((ey ey) + (ez ez)) <= surfel_radius * surfel_radius      inside the disc
 *   a hit pixel gets zbuf = min(zbuf, bits(z)); empty is all ones.  z > 1e-6, so the bits keep the order of the floats.
 * The z-buffer is a minimum: a render depends neither on the batch, nor on the order, nor on the chunk.  A pose with a non-finite entry
 * among its twelve used entries, or the all-zero "no pose" record, renders nothing and is no error.
 * stocs_render_depth: the z image of each of n poses (n * height * width floats, host, row-major), 0.0f where empty.
 * stocs_pose_errors_vsd: n estimates against ground truth, n_gt == 1 or n as for stocs_pose_errors (with n_gt == 1 the ground truth is
 * rendered once).  Each pair renders ZE and ZG.  Per pixel, with xn, yn as above, k = sqrtf((xn xn + yn yn) + 1.0f): BOP compares
 * distances from the camera centre, not z.  dE = ZE k, dG = ZG k, and with raw = depth[pixel], dS = ((float)raw * depth_scale) * k.
 * Then, as bop_toolkit's `bop19` visibility mode:
 *   visG  = G present and (raw == 0 or dG - dS <= delta)
 *   visE  = E present and (raw == 0 or dE - dS <= delta or visG)
 *   inter = visG and visE,  uni = visG or visE
 *   on inter: dd = fabsf(dG - dE); for every t < n_tau, far[t] += (dd >= tau[t]).
 * The record: the integer counts px_est, px_gt (pixels present), vis_est, vis_gt, inter, uni, far[t];
 * e[t] = (float)(far[t] + (uni - inter)) / (float)uni, 1.0f when uni == 0 (t >= n_tau: far 0, e 0); valid = 0 for the pairs that step 5
 * of stocs_pose_errors calls invalid -- the arithmetic still runs, so such an estimate scores 1.  Every field is an integer sum: a
 * record is bitwise independent of the batch it shares and of its position in it.
 * Checked in this order: a NULL ctx (whatever n) and n < 0 are STOCS_ERR_INVALID; n == 0 is then a no-op; a NULL pose, parameter or
 * result pointer, an n_gt other than 1 or n (stocs_pose_errors_vsd), a parameter outside the ranges below (stocs_check_vsd_params:
 * host code, the same check on its own; stocs_render_depth ignores delta, n_tau and tau): STOCS_ERR_INVALID; a context without a model,
 * no frame set, or a frame whose width * height differs from what was uploaded: STOCS_ERR_STATE.
 * Own grow-only workspace on the context (a second call of the same or a smaller size allocates nothing); on the context's stream;
 * stocs_pose_errors_vsd has one pinned read-back and one synchronisation per call, stocs_render_depth one per piece of at most 32 MB
 * of images.  stocs_last_call_timing(which = 7) gives the host steps of the last stocs_pose_errors_vsd and, with "device_clock" on, the
 * HIP-event time of its launches.
 * The kernels (csrc/vsd.hip): a z-buffer of float bits per rendered pose in a chunk of workspace (256 MB; STOCS_VSD_CHUNK=<poses> in
 * the environment forces a size; a chunk holds whole pairs, and with n_gt == 1 the ground truth's buffer stays beside the chunks).
 * Render: a workgroup of four wavefronts per (pose, STOCS_VSD_POINTS model points); a wavefront projects 64 points, one per lane, then
 * takes the in_image ones in turn: the surfel goes into scalar registers and all 64 lanes sweep its square, one 32-bit atomicMin per hit
 * pixel -- in large calls on dense models only where the stored depth, read first, is not already nearer.  Compare: one pass per pair
 * over the union of the two poses' bounding rectangles in both z-buffers and the frame, counts by __ballot and popcount in scalar
 * registers, one integer atomicAdd per counter and workgroup.  STOCS_VSD_FORM=<bits> in the environment forces a form for measurements
 * and tests (1: compare whole frames; 2: never read first; 4: always read first); no bit changes a result. ---- */
#define STOCS_VSD_MAX_TAU 16
#define STOCS_VSD_POINTS 256
typedef struct stocs_vsd_params {
    float   surfel_radius;           /* m, > 0 finite: radius of the disc a model point stands for (default 0.006)   */
    int32_t max_splat_px;            /* 0..16: largest half-width in pixels of the square a surfel is tested on (16) */
    float   delta;                   /* m, > 0 finite: visibility tolerance (default 0.015, BOP's)                   */
    int32_t n_tau;                   /* 1..16 (default 0: the caller sets the taus, they depend on the diameter)     */
    float   tau[STOCS_VSD_MAX_TAU];  /* m, each of the first n_tau > 0 finite: misalignment tolerances               */
} stocs_vsd_params;                  /* 80 bytes */
typedef struct stocs_vsd_record {
    int32_t px_est, px_gt, vis_est, vis_gt, inter, uni;
    int32_t far[STOCS_VSD_MAX_TAU];
    float   e[STOCS_VSD_MAX_TAU];
    int32_t valid, reserved;
} stocs_vsd_record;                  /* 160 bytes */
void stocs_default_vsd_params(stocs_vsd_params* p);
int stocs_check_vsd_params(const stocs_vsd_params* p);
int stocs_render_depth(stocs_ctx* ctx, const float* pose16_camera, int n, const stocs_vsd_params* p, float* depth /* n*height*width */);
int stocs_pose_errors_vsd(stocs_ctx* ctx, const float* est_pose16_camera, int n, const float* gt_pose16_camera, int n_gt,
                          const stocs_vsd_params* p, stocs_vsd_record* out);

/* ---- triangle meshes: a second model representation on the context, an exact, watertight depth rasteriser for it and VSD on that
 * (no reference counterpart).  BOP, YCB-Video and LINEMOD ship their objects as meshes and bop_toolkit's VSD is defined on the rendered
 * mesh; a surfel image depends on a radius chosen per model and pads the silhouette by up to that radius.  csrc/mesh.hip, restated in
 * float32 numpy in tests/mesh_ref.py, equal bit for bit.  All in float, every operation one IEEE add / sub / mul / div / floor, no
 * contraction.
 * The mesh: nv vertices (float[3]) and nt triangles (int32[3], indices into the vertices), in the frame of the model points handed to
 * stocs_ctx_create; keeping the two in step is the caller's job, as it is for the frame and the scene.
 * A vertex v under a pose (R, t): p_a = (R_a0 v_0 + (R_a1 v_1 + R_a2 v_2)) + t_a, step 1 of the depth-check contract.
 * A triangle (i0, i1, i2) with camera points A, B, C:
 *   1. skipped unless all nine coordinates are finite and A_2, B_2, C_2 > 1e-6f.  There is NO near-plane clipping: a triangle that
 *      reaches the camera plane renders nothing.
 *   2. per vertex a = (fx * p_0) / p_2 + cx, b = (fy * p_1) / p_2 + cy;  c_lo = fmaxf(floorf(min a) - 1, 0),
 *      c_hi = fminf(floorf(max a) + 2, W - 1), r_lo and r_hi likewise from b and H; skipped unless c_lo <= c_hi and r_lo <= r_hi, tested
 *      in float; only then converted to int.  No size cap.
 *   3. edge normals nA = B x C, nB = C x A, nC = A x B, a cross product written n_x = u_y v_z - u_z v_y, n_y = u_z v_x - u_x v_z,
 *      n_z = u_x v_y - u_y v_x.
 *   4. per pixel (r, c) of the box, with the ray of the surfel rule, xn = ((float)c - cx) / fx, yn = ((float)r - cy) / fy:
 *        u = xn nA_0 + (yn nA_1 + nA_2), v and w likewise from nB and nC;  det = u + (v + w)
 *        hit only if det != 0 and (u, v, w >= 0 or u, v, w <= 0): edges are inclusive, and there is no back-face culling, so winding
 *        does not matter and open meshes render
 *        z = (u A_2 + (v B_2 + w C_2)) / det;  hit only if z > 1e-6f
 *        a hit pixel gets zbuf = min(zbuf, bits(z)); empty is all ones.
 * B x A is exactly -(A x B) in IEEE arithmetic and the dot with the ray negates exactly too, so two triangles that share an edge see
 * the same edge value with opposite sign: a ray is inside at least one of them and a ray exactly on the edge is inside both -- no
 * pinholes.  The z-buffer is a minimum of float bits: a render depends on neither triangle order, winding, batch nor chunk.  The
 * reversed triangle (i0, i2, i1) turns u, v, w into -u, -w, -v exactly, and det and z come out the same bits (v + w is w + v).  Which
 * corner comes first is not winding: (i1, i2, i0) permutes u, v, w, hits the same pixels, and sums det and z in another order, so their
 * last bits may differ (2 ulp measured).  A pose with a non-finite used entry, or the all-zero record, renders nothing, as for surfels.
 * stocs_mesh_check: the host check of a mesh on its own (no context, no device): STOCS_ERR_INVALID for a negative count, a NULL array
 * of a non-zero count, an index outside [0, nv) or a non-finite vertex; STOCS_ERR_CAPACITY above nv <= 2^24, nt <= 2^22.
 * stocs_ctx_set_mesh: copies the mesh to the device, where it stays until the next call or stocs_ctx_destroy; nt == 0 drops it (and
 * looks at nothing else).  stocs_mesh_check's answers; synchronises once; grow-only (a second mesh of the same or a smaller size
 * allocates nothing).  stocs_ctx_mesh_info: the counts on the context (0, 0 without a mesh).
 * stocs_render_depth_mesh: the images of stocs_render_depth from the mesh.  stocs_pose_errors_vsd_mesh: stocs_pose_errors_vsd with the
 * mesh rendered in place of the surfels: the same compare pass, the same stocs_vsd_params (surfel_radius and max_splat_px are ignored,
 * whatever they hold) and the same stocs_vsd_record.  Checked in the order of their surfel counterparts, with "no mesh" where those
 * have "no model": STOCS_ERR_STATE.  stocs_mesh_last_call_timing gives the steps of the last stocs_pose_errors_vsd_mesh as
 * stocs_last_call_timing does for the calls it knows.
 * The kernel (csrc/mesh.hip): a workgroup of four wavefronts per (pose, 256 triangles), one triangle per lane for the set-up; a box of
 * at most STOCS_MESH_SMALL_PX pixels is walked by its lane, a larger one swept by the wavefront from scalar registers, the largest by
 * the workgroup.  STOCS_MESH_FORM=<bits> in the environment forces forms for measurements and tests (1: lanes walk their own boxes;
 * 2: none does; 4: read the stored depth before every atomicMin, 8: never, the default; 16: no box goes to the workgroup); no bit changes a result.
 * STOCS_VSD_CHUNK keeps its meaning.  stocs_mesh_small_px returns STOCS_MESH_SMALL_PX as the library was built; STOCS_MESH_SMALL_PX=<pixels>
 * in the environment overrides it for measurements (tools/mesh_time.py --forms) and changes no result either. ---- */
#define STOCS_MESH_SMALL_PX 120
int stocs_mesh_small_px(void);
int stocs_mesh_check(const float* pos3, int nv, const int32_t* tris3, int nt);
int stocs_ctx_set_mesh(stocs_ctx* ctx, const float* pos3, int nv, const int32_t* tris3, int nt);
int stocs_ctx_mesh_info(const stocs_ctx* ctx, int* nv, int* nt);
int stocs_render_depth_mesh(stocs_ctx* ctx, const float* pose16_camera, int n, float* depth /* n*height*width */);
int stocs_pose_errors_vsd_mesh(stocs_ctx* ctx, const float* est_pose16_camera, int n, const float* gt_pose16_camera, int n_gt,
                               const stocs_vsd_params* p, stocs_vsd_record* out);
int stocs_mesh_last_call_timing(const stocs_ctx* ctx, const char** labels, double* ms, int cap, int* n);

/* ---- the mesh in the joint renderer and in scene selection: exact masks (no reference counterpart).  The splats of the render contract
 * pad a silhouette by up to point_radius, stand at the constant depth of their centre, let a far-side point of a sparse model through
 * between near-side ones and need a radius chosen per model.  These entry points make the same judgements -- instance masks, what hides
 * what, agreement with the depth image, the pixel rows stocs_scene_select walks -- on the mesh of stocs_ctx_set_mesh.  csrc/render_mesh.hip,
 * restated in float32 numpy in tests/render_mesh_ref.py as a composition of tests/mesh_ref.py, render_ref.py and scene_ref.py, equal bit
 * for bit.
 * Z_h: the image of float bits that stocs_render_depth_mesh defines for pose h ALONE against the frame of stocs_ctx_set_frame: steps 1-4
 * of the mesh contract above, unchanged; empty is all ones.  Everything below is defined through Z_h.  Poses are CAMERA-frame and
 * column-major; a pose with a non-finite entry among its twelve used entries, or the all-zero "no pose" record, renders nothing, gets a
 * zero record (and a zero row) and is no error.  The key buffer, the ids (id = id_base + h, id_base >= 0, id_base + n <= 2^31 - 1) and
 * the `clear` rule are those of stocs_render_poses.
 *   1. stocs_render_poses_mesh: every pixel where Z_h is not empty gets key = min(key, (uint64_t)Z_h << 32 | (id_base + h)).  The nearest
 *      surface wins and on an equal depth the lower id; a minimum: the result depends on neither order, batch, kernel form nor the
 *      sequence of calls.  Splat renders and mesh renders, of this or of other contexts, may share one buffer.  Synchronises its stream
 *      before it returns.  It takes no stocs_render_params: nothing in the mesh rule has a radius.
 *   2. stocs_render_resolve_mesh: called with the same poses and ids after every render into the buffer is done.  C_h is the set of
 *      non-empty pixels of Z_h, footprint = |C_h|.  A pixel of C_h whose key's low word is not h's id is hidden (an empty key too);
 *      otherwise it is visible and classified by steps 5-6 of the depth-check contract with p_2 := the float in the key's high word.
 *      The record is stocs_render_result with the identities stated there.  Of p only tolerance and class_threshold are read and checked;
 *      point_radius and max_splat_px are ignored, whatever they hold (as stocs_pose_errors_vsd_mesh ignores the surfel fields).  There is
 *      no 2^19-pixel cap: the footprint is no bitset in LDS.
 *   3. stocs_explain_poses_mesh, the single-object form, exactly as stocs_explain_poses: the context's own key buffer, id_base 0; clear,
 *      render, resolve, and labels / state when `labels` is given.  One pinned read-back and one synchronisation per call.  n == 0 with
 *      labels given returns the all-empty image (it needs the frame for its size, neither a mesh nor anything else).
 *   4. stocs_scene_footprints_mesh: stocs_scene_footprints with Z_h from the mesh in place of the splat minimum: the same classification,
 *      rows (the whole row is always written) and stocs_scene_record, the 2^19 cap, the chunk rule and STOCS_SCENE_CHUNK.  The record of h
 *      equals the record stocs_explain_poses_mesh gives for that pose alone (hidden == 0, visible == footprint).  A pool may hold splat
 *      slots and mesh slots side by side; stocs_scene_select does not know the difference.
 * stocs_render_labels serves both kinds of buffer, unchanged.
 * Checked in the order of the splat counterparts: NULL ctx and n < 0 (STOCS_ERR_INVALID); n == 0 is a no-op (stocs_explain_poses_mesh:
 * unless labels are given); NULL poses / p / key buffer / rows / out; claim, slots; tolerance and class_threshold outside the ranges of
 * stocs_render_params; an id outside 0 .. 2^31 - 2: STOCS_ERR_INVALID.  Then a context without a mesh: STOCS_ERR_STATE; then the frame
 * (STOCS_ERR_STATE) and, for stocs_scene_footprints_mesh, npix > 2^19: STOCS_ERR_CAPACITY.
 * Every entry point has its own grow-only workspace on the context (a second call of the same or a smaller size allocates nothing);
 * poses go up and results come back through the context's pinned block, everything runs on the context's stream.
 * The kernels.  Render: mesh.hip's rasteriser (one triangle per lane for the set-up; lane, wavefront and workgroup tiers; the same
 * STOCS_MESH_FORM bits) with a 64-bit sink: all poses of the launch write the one buffer, one 64-bit atomicMin per hit pixel, the id in a
 * scalar register.  Resolve: every pose of a chunk is rendered alone into a z-buffer of its own by the depth form of the rasteriser
 * (chunks of 256 MB of z-buffers; STOCS_RENDER_MESH_CHUNK=<poses> in the environment forces a size), then one kernel walks the rows of
 * each pose's bounding rectangle in runs of 64 pixels: a 4-byte load of the pose's own depth, where present an 8-byte load of the key,
 * counts by __ballot and popcount, one integer atomicAdd per counter and workgroup; several workgroups per pose.  Scene footprints: the
 * depth form into the chunk's z-buffers, then stocs_scene_footprints' classify kernel as it stands.
 * stocs_render_mesh_last_device_ms: with the option "device_clock" on, the HIP-event time in ms of the key render and of the (last
 * chunk's) resolve kernel of the last call of 1-3 on this context; -1 for what that call did not run or did not time.
 * Known limits: resolve rasterises every pose a second time (the key buffer keeps only the winners' depths); the depth check
 * (stocs_depth_check_poses), trial batches and the tracker still see the model as points (a pose can be refined on the mesh by
 * stocs_refine_poses_visible below, as a step of its own). ---- */
int stocs_render_poses_mesh(stocs_ctx* ctx, const float* pose16_camera, int n, int id_base, void* d_zkey, int clear);
int stocs_render_resolve_mesh(stocs_ctx* ctx, const float* pose16_camera, int n, int id_base, const stocs_render_params* p, const void* d_zkey,
                              stocs_render_result* out);
int stocs_explain_poses_mesh(stocs_ctx* ctx, const float* pose16_camera, int n, const stocs_render_params* p, stocs_render_result* out,
                             int32_t* labels, uint8_t* state);
int stocs_scene_footprints_mesh(stocs_ctx* ctx, const float* pose16_camera, int n, int slot_base, int n_slots, const stocs_render_params* p,
                                int claim, void* d_rows, stocs_scene_record* out);
int stocs_render_mesh_last_device_ms(const stocs_ctx* ctx, float* key_ms, float* resolve_ms);

/* ---- refinement on the visible surface: projective, point-to-plane refinement of n CAMERA-frame poses of the mesh of stocs_ctx_set_mesh
 * against the frame of stocs_ctx_set_frame (no reference counterpart).  stocs_refine_poses pairs a voxel-sampled scene segment with the
 * nearest point of the whole model cloud, far side included; this one needs no segment, uses every depth pixel under the rendered
 * silhouette and pairs it with the surface the camera sees there at the current hypothesis, under the exact normal of the facet.
 * csrc/refine_visible.hip, restated in numpy in tests/refine_visible_ref.py: keys and states equal bit for bit, sums and poses within the
 * rounding of the double sums.
 * Per iteration and pose P: render, accumulate, solve.
 *   The render is the mesh contract above with one addition: a hit pixel gets key = min(key, (uint64_t)bits(z) << 32 | t), t the index of
 *   the triangle; empty is all ones.  The nearest surface wins and on equal depth bits the lowest triangle index; a minimum: independent of
 *   order, batch, chunk and kernel form (STOCS_MESH_FORM).
 * Steps 1-3 in float, every operation one IEEE operation, no contraction; step 4 in double from those floats.  For pixel (r, c) with a
 * non-empty key (z the float in the high word, t the low word):
 *   1. xn = ((float)c - cx) / fx, yn = ((float)r - cy) / fy (the mesh rule's ray); model point p = (xn z, yn z, z).
 *      raw = depth[r W + c]; raw == 0: no_depth.  d = (float)raw * depth_scale, q = (xn d, yn d, d).  With a class image:
 *      cp = (float)((double)prob[r W + c] * (1.0 / 10000)) (step 6 of the depth-check contract); cp < class_threshold: off_class.
 *   2. e = p - q, D = e_x e_x + (e_y e_y + e_z e_z); D > max_distance * max_distance (the product in float): too_far; equality is not.
 *      This is what drops occluders and background.
 *   3. A, B, C: the triangle's camera points (the mesh contract's vertex rule).  u = B - A, w = C - A,
 *      m = (u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x);  s = m_x p_x + (m_y p_y + m_z p_z), mm and pp likewise from m, m and
 *      p, p.  m.m == 0 (a degenerate facet), or s s < (min_view_cos * min_view_cos) * (mm * pp): grazing.  min_view_cos == 0: only
 *      degenerate facets are.
 *   4. a pixel that passes 1-3 is counted.  In double: len = sqrt(m_x m_x + (m_y m_y + m_z m_z)), n = (g m) / len per component with
 *      g = -1 when s > 0 (the float of step 3), else 1: the normal faces the camera, whatever the winding.
 *      a = (q x n, n) = (q_y n_z - q_z n_y, q_z n_x - q_x n_z, q_x n_y - q_y n_x, n_x, n_y, n_z),
 *      b = (n_x (q_x - p_x) + n_y (q_y - p_y)) + n_z (q_z - p_z).
 *      The row linearises n'.(p' - q) for a small motion Delta = (Rz(gamma) Ry(beta) Rx(alpha), t) applied ON THE LEFT, in the camera frame;
 *      the normal turns with the point: r ~ n.(p - q) + omega.(q x n) + t.n.
 *   5. the 29 sums over the counted pixels, in double: [0..20] the upper triangle of A^T A row by row, [21..26] A^T b, [27] the count,
 *      [28] b^T b.
 *   6. count < 6, or a pivot of the 6x6 elimination (partial pivoting) below 1e-300: the pose is frozen, keeps its current value and is
 *      evaluated no more.  Otherwise x = (alpha, beta, gamma, t) solves A^T A x = A^T b, R = Rz Ry Rx, and P <- (float)(Delta P): entry
 *      (r, c), r < 3, is (R_r0 P_0c + R_r1 P_1c) + R_r2 P_2c, plus t_r for c = 3, in double, rounded to float; the last row stays.  The
 *      pose is a float pose between iterations: an iteration is a pure function of 16 floats.
 *   7. a pose with a non-finite used entry, or the all-zero record, renders nothing, comes back bit for bit with a zero record and is no
 *      error.
 * max_iterations == 0 evaluates once and updates nothing: the pose comes back bit for bit and the record is a dense depth score of it.
 * The record describes the LAST EVALUATION, the pose before the last update (n_corr of stocs_refine_poses has the same convention):
 * present = no_depth + off_class + too_far + grazing + counted is the number of non-empty keys; iterations the updates applied; frozen 1
 * when step 6 froze the pose.
 * stocs_refine_visible_detail: ONE pose, one evaluation, no update (max_iterations is checked and not used): the keys (H W, or NULL),
 * per pixel state 0 empty, 1 no_depth, 2 off_class, 3 too_far, 4 grazing, 5 counted (H W, or NULL; the tests in the order of the steps)
 * and the 29 sums.  A synchronous diagnosis path with pageable copies.
 * Checked in the order of the mesh entry points: NULL ctx, n < 0 (STOCS_ERR_INVALID); n == 0 is a no-op; NULL pointers, parameters out of
 * range (STOCS_ERR_INVALID); no mesh (STOCS_ERR_STATE); no frame or a frame whose size does not match (STOCS_ERR_STATE).
 * Its own grow-only workspace on the context (a second call of the same or a smaller size allocates nothing; stocs_ctx_destroy frees
 * it); poses go up and poses and records come back through the pinned block: one read-back and one synchronisation per call of
 * stocs_refine_poses_visible.  Everything between runs on the context's stream.
 * The kernels (csrc/refine_visible.hip).  Key buffers live in chunks of 256 MB (STOCS_REFINE_VISIBLE_CHUNK=<poses> in the environment
 * forces a size); all iterations of a chunk run before the next chunk starts.  Accumulate: a grid of (G, pose), G =
 * stocs_refine_visible_groups(width, height) = min(64, max(1, pixels / 2048)); workgroup g walks rows r0 + g, r0 + g + G, ... of the
 * pose's rectangle in runs of 64 pixels per wavefront; 29 double sums per lane, a butterfly, the four waves in order, one partial per
 * workgroup, no float atomics; it puts the empty key back where it found one, so only what a render wrote is cleared between
 * iterations.  Solve: one wavefront per pose.  A pose's result is bitwise independent of the batch, of its position in it and of the
 * chunk.  stocs_refine_visible_last_device_ms: with the option "device_clock" on, the HIP-event time in ms of the render, the
 * accumulation and the solve of the last iteration of the last chunk of the last call; -1 otherwise.
 * Known limits: same-pixel association has no pull from frame pixels outside the rendered silhouette, so a pose that is off by more
 * than max_distance along the rays, or by more than the object's width across them, does not come back; the step of 6 is undamped and
 * its rotation is about the camera's origin: where the visible surface constrains a motion weakly (a solid of revolution, the Cm solid
 * of this project's benchmarks) it can be large and leave the pose worse than it came (measured: DESIGN.md 7.19).  For such a solid use
 * stocs_refine_poses_visible_damped below: the same evaluation, a damped and bounded step about a point of the object that is taken
 * only when it lowers the cost.  No trimming by rank; the float pose is not re-orthonormalised between iterations;
 * not part of trial batches or the tracker. ---- */
typedef struct stocs_refine_visible_params {
    int32_t max_iterations;     /* >= 0 (default 5)                                            */
    float   max_distance;       /* m, > 0 finite (default 0.02)                                */
    float   min_view_cos;       /* 0 <= . < 1 (default 0: off)                                 */
    float   class_threshold;    /* finite (default 0.10); unused without a class image         */
} stocs_refine_visible_params;     /* 16 bytes */
typedef struct stocs_refine_visible_result {
    int32_t present, no_depth, off_class, too_far, grazing, counted;  /* present = their sum  */
    int32_t iterations, frozen;
    float   rms;                /* sqrtf((float)(btb / count)), 0 when count == 0              */
    int32_t reserved;
} stocs_refine_visible_result;     /* 40 bytes */
void stocs_default_refine_visible_params(stocs_refine_visible_params* p);
int stocs_check_refine_visible_params(const stocs_refine_visible_params* p);   /* host only */
int stocs_refine_visible_groups(int width, int height);                        /* host only; 0 for a size below 1 */
int stocs_refine_poses_visible(stocs_ctx* ctx, const float* pose16_camera, int n, const stocs_refine_visible_params* p, float* pose16_out,
                               stocs_refine_visible_result* out);
int stocs_refine_visible_detail(stocs_ctx* ctx, const float* pose16_camera /* one */, const stocs_refine_visible_params* p,
                                uint64_t* keys /* H*W or NULL */, uint8_t* state /* H*W or NULL */, double* sums29);
int stocs_refine_visible_last_device_ms(const stocs_ctx* ctx, float* render_ms, float* accumulate_ms, float* solve_ms);

/* ---- damped refinement on the visible surface: Levenberg-Marquardt steps on the evaluation of stocs_refine_poses_visible, accepted or
 * rejected on the device, bounded, and applied about a point of the object (no reference counterpart).  csrc/refine_visible.hip, restated
 * in numpy in tests/refine_visible_damped_ref.py.  The plain form, its kernels and its results are what they were.
 * An evaluation is exactly one evaluation of the plain contract above: the render, steps 1-5, the 29 sums S and the five counts, by the
 * same kernels on a float pose.  With K = base.max_iterations a call makes K + 1 evaluations per pose, e = 0 .. K; K = 0 makes one, and
 * then the pose comes back bit for bit with the plain form's record.  Everything below is in double, from the float pose and the sums.
 *   Cost.  C = (S[28] + (double)max_d2 too_far) / (counted + too_far), max_d2 the float product max_distance * max_distance of step 2;
 *     C = +inf when counted < 6.  A truncated quadratic over the silhouette pixels with a measurement: a pose that merely sheds pixels
 *     past max_distance does not look better for it.
 *   e = 0.  The start is accepted: the accepted state is the pose Pa, its sums Sa and counts, its cost Ca; lambda = lambda0.  With K > 0,
 *     counted < 6 freezes the pose as in the plain form (frozen = 1, the pose as it came).
 *   e > 0, the trial Pt.  Accepted if and only if C < Ca: then the accepted state is the trial's, lambda = max(lambda / lambda_down, 1e-9)
 *     and iterations grows by 1.  Otherwise lambda = min(lambda lambda_up, 1e9) and rejected grows by 1.  A trial that shows fewer than 6
 *     counted pixels (or nothing) has C = +inf and is rejected.
 *   After evaluation e < K, the next trial from (Pa, Sa, lambda):
 *     1. the pivot c = 0 (pivot 0), or c_r = ((Pa_r0 m_0 + Pa_r1 m_1) + Pa_r2 m_2) + Pa_r3 with m = pivot_model (pivot 1).
 *     2. the sums about c, without a second accumulation: the row about c is a' = ((q - c) x n, n) = T a with T = [[I, -[c]x], [0, I]],
 *        so M' = (T M) T^T and v' = T v from the 21 + 6 sums.
 *     3. M'' = M' with every diagonal entry multiplied by (1 + lambda).
 *     4. x = the 6x6 elimination of step 6 above on (M'', v'); a pivot below 1e-300 freezes the pose at Pa.
 *     5. s = min(1, max_step_rotation / |x[0..2]|, max_step_translation / |x[3..5]|), |.| = sqrt(a a + (b b + c c)); a zero norm sets no
 *        bound; x <- s x.
 *     6. Delta = (R(x), t) with R = Rz Ry Rx as above and t_r = (x[3 + r] + c_r) - ((R_r0 c_0 + R_r1 c_1) + R_r2 c_2): the rotation is
 *        about c.
 *     7. Pt = (float)(Delta Pa), composed and rounded as in step 6 above.
 *   Returned: Pa; base describes Pa's evaluation (iterations: the accepted updates), evaluations and rejected count what was done, cost
 *   and lambda are (float) of Ca and of the last lambda.  The cost of the returned pose is never above that of the pose that came in;
 *   evaluations are deterministic, so two K = 0 calls show it exactly.
 * As in the plain form: a non-finite or all-zero pose comes back bit for bit with a zero record; the order of the refusals, the new
 * parameters checked behind the base ones; one grow-only workspace, one read-back and one synchronisation per call; chunks of key
 * buffers and STOCS_REFINE_VISIBLE_CHUNK; a pose's result is bitwise independent of batch, position and chunk.
 * trace (n (K + 1) rows, row h (K + 1) + e, or NULL): the pose that was evaluated, its cost, whether it was accepted (1 at e = 0), the
 * lambda after the decision, state 1: evaluated, 3: evaluated and the pose froze behind it; a row that was not evaluated (an invalid or
 * frozen pose) is zero.
 * The kernel: refine_visible_damped_solve_kernel, one wavefront per pose, the fixed-order reduction of the plain solve, then lane 0; the
 * accepted pose, sums, cost and lambda of a pose live in the workspace between evaluations.
 * Measured: DESIGN.md 7.21 and profiles/refine_visible_damped.md.  Not here: re-orthonormalising the pose, trimming by rank, use inside
 * trial batches or the tracker. ---- */
typedef struct stocs_refine_visible_damped_params {
    stocs_refine_visible_params base;   /* as above; max_iterations = K                                        */
    float   lambda0;                    /* >= 0 finite (default 1)                                             */
    float   lambda_down, lambda_up;     /* >= 1 finite (defaults 4, 16)                                        */
    float   max_step_rotation;          /* rad, > 0 (default 5 degrees); +inf: no bound                        */
    float   max_step_translation;       /* m, > 0 (default 0.01); +inf: no bound                               */
    int32_t pivot;                      /* 0: the camera's origin (the plain form's); 1: pivot_model (default) */
    float   pivot_model[3];             /* a point in the MODEL frame, finite (default 0, 0, 0)                */
} stocs_refine_visible_damped_params;   /* 52 bytes */
typedef struct stocs_refine_visible_damped_result {
    stocs_refine_visible_result base;   /* the evaluation of the RETURNED pose; iterations = accepted updates  */
    int32_t evaluations, rejected;
    float   cost, lambda;               /* (float) of the accepted cost and of the last lambda                 */
} stocs_refine_visible_damped_result;   /* 56 bytes */
typedef struct stocs_refine_visible_trace {
    float   pose[16];
    double  cost, lambda;
    int32_t accepted, state;
} stocs_refine_visible_trace;           /* 88 bytes */
void stocs_default_refine_visible_damped_params(stocs_refine_visible_damped_params* p);
int stocs_check_refine_visible_damped_params(const stocs_refine_visible_damped_params* p);   /* host only */
int stocs_refine_poses_visible_damped(stocs_ctx* ctx, const float* pose16_camera, int n, const stocs_refine_visible_damped_params* p,
                                      float* pose16_out, stocs_refine_visible_damped_result* out,
                                      stocs_refine_visible_trace* trace /* n * (K + 1) or NULL */);

/* ---- contour pull for the damped refinement on the visible surface: the frame's object pixels that the render leaves uncovered pull the
 * pose towards them (no reference counterpart).  csrc/refine_visible.hip, restated in numpy in tests/refine_visible_contour_ref.py.  The
 * plain and the damped form, their kernels and their results are what they were.  The frame must carry a class image.
 *   Object pixels.  O = the pixels with raw != 0 and cp >= class_threshold, cp as in step 1 of the plain contract; N_O = |O| does not
 *     depend on the pose and is counted once per call.
 *   Evaluation.  One evaluation of the damped contract (the render, steps 1-5, the 29 sums S, the five counts) plus the contour pass
 *     below on the same keys.  Let (r0..r1, c0..c1) be the pose's rectangle (the union of its triangles' clamped boxes), grown by
 *     R = pull_radius_px on every side and clamped to the frame.  For every pixel u = (r, c) of the grown rectangle that is in O and has
 *     an empty key:
 *     1. the nearest silhouette pixel: among the pixels s = (r_s, c_s) with a non-empty key, |r_s - r| <= R and |c_s - c| <= R, the one
 *        with the minimum of (d2 = dr dr + dc dc, r_s W + c_s): the exact Euclidean nearest inside the square window, on equal d2 the
 *        lowest linear index.  None: u is unreached (state 1).
 *     2. in float, every operation one IEEE operation, no contraction: z_s the float in the high word of s's key,
 *        p = (xn_s z_s, yn_s z_s, z_s) on the mesh rule's ray of s; d = (float)raw_u * depth_scale, q = (xn_u d, yn_u d, d) on the ray of
 *        u; e = q - p; D = e_x e_x + (e_y e_y + e_z e_z).
 *     3. D > pull_distance * pull_distance (the product in float): u is beyond (state 2) and gives no row; equality is not beyond.  This
 *        is what drops the table and the neighbours.
 *     4. otherwise u is pulled (state 3) and gives three point-to-point rows, in double from those floats: for k = 0, 1, 2
 *        a_k = (p x u_k, u_k) with u_k the k-th unit vector, b_k = e[k]:
 *        a_0 = (0, p_z, -p_y, 1, 0, 0), a_1 = (-p_z, 0, p_x, 0, 1, 0), a_2 = (p_y, -p_x, 0, 0, 0, 1).
 *        The rows linearise p' - q for the same left, camera-frame motion as the plain row: p' ~ p + omega x p + t and
 *        u_k.(omega x p) = omega.(p x u_k).  Each row adds its products to the 29 contour sums Sc as a counted pixel's row does to S, row
 *        0 first; Sc[27] counts pulled pixels, one per pixel; Sc[28] = the sum of b_k b_k.
 *   Counts.  uncovered = N_O - (too_far + grazing + counted): the object pixels without a key.  unreached, beyond and pulled are counted
 *     over the grown rectangle; uncovered pixels outside it are unreached by definition, are not walked and are not in `unreached`.
 *   System, in double, with w = (double)contour_weight:  M = S[0..20] + w Sc[0..20], v = S[21..26] + w Sc[21..26], entry by entry.
 *     Everything behind them is the damped contract verbatim on these totals (the sums about the pivot, (1 + lambda) on the diagonal,
 *     the elimination, the common bound, the composition).
 *   Cost.  C = ((S[28] + max_d2 too_far) + w (Sc[28] + pull_d2 (uncovered - pulled))) / ((double)(counted + too_far) + w uncovered),
 *     max_d2 and pull_d2 the (double) of the float products; C = +inf when counted + 3 pulled < 6, and with K > 0 that freezes the pose
 *     at e = 0 in place of the damped form's counted < 6.  A truncated quadratic over a pixel set that does not depend on the pose: a
 *     pose that sheds an object pixel pays pull_d2 for it.  An empty render stays rejected or frozen; a silhouette that has slid off the
 *     object but still reaches it within R is no longer frozen.
 *   contour_weight == 0: the contour pass is not run; poses, the damped part of the records and the trace are those of
 *     stocs_refine_poses_visible_damped bit for bit (pulled, unreached, beyond and pull_rms are 0).  N_O == 0 with w > 0: the same,
 *     every added term is an exact zero.
 * Returned per pose: the damped record of the RETURNED pose and, of the same evaluation, object_px, uncovered, unreached, beyond, pulled
 * and pull_rms; an invalid or all-zero pose comes back bit for bit with a zero record.  trace: as in the damped form.
 * stocs_refine_visible_contour_detail: ONE pose, one evaluation, no update (max_iterations is checked and not used; contour_weight
 * likewise, the pass runs): per pixel the contour state (H W, or NULL: 0 for a pixel that was not walked, is not in O or has a key, else
 * 1, 2, 3), the linear index of the nearest silhouette pixel (H W, or NULL; -1 where there is none) and the 29 contour sums.
 * Checked in the order of the damped form, the new parameters behind the damped ones, and behind "no frame": a frame without a class
 * image (STOCS_ERR_STATE).  One grow-only workspace, one read-back and one synchronisation per call; chunks of key buffers and
 * STOCS_REFINE_VISIBLE_CHUNK; a pose's result is bitwise independent of batch, position and chunk.
 * The kernels: refine_visible_object_count_kernel once per call; per evaluation refine_visible_contour_kernel between
 * the render and the accumulation (which clears the keys): the accumulation's grid, tiles of 16 rows x 64 columns of the grown
 * rectangle, "key present" as bit rows in LDS built with __ballot, the nearest set bit of a row by count-leading/trailing-zeros, the
 * minimum over the window's rows nearest first; one partial per workgroup in a fixed order; refine_visible_contour_solve_kernel in the
 * damped solve's place.  stocs_refine_visible_contour_last_device_ms: with "device_clock" on, the contour kernel's HIP-event time of the
 * last evaluation of the last chunk of the last call; -1 otherwise.
 * Not here: the opposite push (silhouette pixels whose measurement lies far behind), weights per pixel, the term inside trial batches or
 * the tracker, frames without a class image. ---- */
typedef struct stocs_refine_visible_contour_params {
    stocs_refine_visible_damped_params damped;   /* as above                                                   */
    float   contour_weight;             /* w >= 0 finite (default 1); 0: the damped form, bit for bit          */
    int32_t pull_radius_px;             /* R, 1 .. 64 (default 16)                                             */
    float   pull_distance;              /* m, > 0 finite (default 0.03): the 3-D gate of a pull                */
} stocs_refine_visible_contour_params;  /* 64 bytes */
typedef struct stocs_refine_visible_contour_result {
    stocs_refine_visible_damped_result damped;
    int32_t object_px;                  /* N_O                                                                 */
    int32_t uncovered, unreached, beyond, pulled;   /* of the returned pose's evaluation                      */
    float   pull_rms;                   /* sqrtf((float)(Sc[28] / pulled)), 0 when pulled == 0                 */
} stocs_refine_visible_contour_result;  /* 80 bytes */
void stocs_default_refine_visible_contour_params(stocs_refine_visible_contour_params* p);
int stocs_check_refine_visible_contour_params(const stocs_refine_visible_contour_params* p);   /* host only */
int stocs_refine_poses_visible_contour(stocs_ctx* ctx, const float* pose16_camera, int n, const stocs_refine_visible_contour_params* p,
                                       float* pose16_out, stocs_refine_visible_contour_result* out,
                                       stocs_refine_visible_trace* trace /* n * (K + 1) or NULL */);
int stocs_refine_visible_contour_detail(stocs_ctx* ctx, const float* pose16_camera /* one */, const stocs_refine_visible_contour_params* p,
                                        uint8_t* state /* H*W or NULL */, int32_t* nearest /* H*W or NULL */, double* sums29);
int stocs_refine_visible_contour_last_device_ms(const stocs_ctx* ctx, float* contour_ms);

/* ---- mesh models: a triangle mesh sampled into the oriented model cloud the search needs (no reference counterpart).  Stand-alone like
 * stocs_preprocess_model: no context; the same cached per-thread workspace and pinned block (stocs_trim gives them back; a second call of
 * the same or a smaller size allocates nothing).  csrc/mesh_sample.hip, restated in numpy in tests/mesh_sample_ref.py, equal bit for bit.
 * The mesh is stocs_ctx_set_mesh's; spacing h > 0 in the mesh's units: one sample per h^2 of area in expectation; seed: any 64 bits.
 * Per triangle t = (A, B, C), in double from the float coordinates, every operation one IEEE operation in this order:
 *   e1 = B - A, e2 = C - A, c = e1 x e2 (each component a difference of two rounded products), len = sqrt(cx cx + (cy cy + cz cz)),
 *   area = 0.5 len, x = area / (hd hd) with hd = (double)h;   n_t = floor(x) + (d_t < x - floor(x)),
 *   d_t = (key_t >> 40) 2^-24, key_t = mix64(mix64(seed + 0x9E3779B97F4A7C15) ^ (t 0xD1B54A32D192ED03 + 0x8CB92BA72F3D8DD7)) modulo 2^64,
 *   mix64(z): z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) 0x94D049BB133111EB; z ^ (z >> 31).
 *   A triangle with a non-finite corner or len == 0 has no sample and counts as skipped.  x >= 2^32 - 1 on any triangle, or a total above
 *   2^31 - 1, is STOCS_ERR_INVALID ("spacing too small for the mesh").
 * Per sample j < n_t: w = mix64(key_t ^ ((j + 1) 0xDB4F0B9175AE2165)), iu = w >> 40, iv = (w >> 16) & 0xFFFFFF; when iu + iv >= 2^24 both
 *   are reflected (2^24 - 1 - i); u = iu 2^-24, v = iv 2^-24 (exact floats); in float, per component, position = A + (u (B - A) + v (C - A));
 *   normal = (float)(c / len) per component.  orient 0: that normal, the winding's (B - A) x (C - A).  orient 1: negated when
 *   n.x p.x + (n.y p.y + n.z p.z) < 0 in float, p the sample's position: away from the origin, stocs_preprocess_model's convention, for meshes
 *   whose winding is not consistent.
 * Samples come in (t, j) order.  A triangle's samples depend on the seed, its index and its corners only.
 * stocs_mesh_sample_counts: the sizes, and the per-triangle detail.  Checked in this order, all before a device is looked for:
 *   stocs_mesh_check's answers except the finite-vertex test (a non-finite corner is a skipped triangle here); a spacing that is not
 *   finite or not above 0: STOCS_ERR_INVALID.  nt == 0: all zero, STOCS_OK.  counts (nt) and every other output may be NULL.
 *   *area_total: the areas of the triangles that are not skipped, added in triangle order in double.
 * stocs_mesh_sample: in this order, before a device is looked for: NULL n_out; stocs_mesh_check's answers (a non-finite vertex included); the
 *   spacing as above; orient outside {0, 1}; cap < 0: STOCS_ERR_INVALID (STOCS_ERR_CAPACITY where stocs_mesh_check says so).  nt == 0 or a
 *   total of 0: STOCS_OK, *n_out = 0.  A total above cap: STOCS_ERR_CAPACITY, *n_out = the total, nothing else is written.  Any of
 *   out_pos3, out_nrm3 (total x 3) and out_tri (total) may be NULL.
 * stocs_preprocess_model_mesh: the samples go through the voxel grid of stocs_preprocess_model on the device (positions and normals
 *   averaged per leaf; no host round trip between the sample kernel and the grid), then its tail: a leaf whose averaged normal has no
 *   length is dropped, the others are normalised in double, positions times model_scale.  spacing == 0: voxel_size / 4, about 16 samples
 *   per leaf face.  Checks as stocs_mesh_sample (spacing 0 allowed), then voxel_size not finite or not above 0, a non-finite
 *   model_scale, cap < 0: STOCS_ERR_INVALID.  More leaves than cap: STOCS_ERR_CAPACITY with *n_out the count and the first cap written,
 *   as stocs_preprocess_model.
 * STOCS_MESH_SAMPLE_FORM=<n> in the environment forces the sample kernel's search form for measurements and tests (1: every lane searches
 * the whole offset array, the default; 2: a workgroup finds its triangle range once and searches a window of it in LDS); no value changes a
 * result. ---- */
#define STOCS_MESH_ORIENT_WINDING 0
#define STOCS_MESH_ORIENT_ORIGIN 1
int stocs_mesh_sample_counts(const float* pos3, int nv, const int32_t* tris3, int nt, float spacing, uint64_t seed, int device,
                             int32_t* counts /* nt or NULL */, double* area_total, int64_t* n_total, int* n_skipped);
int stocs_mesh_sample(const float* pos3, int nv, const int32_t* tris3, int nt, float spacing, uint64_t seed, int orient, int device,
                      float* out_pos3, float* out_nrm3, int32_t* out_tri, int cap, int* n_out);
int stocs_preprocess_model_mesh(const float* pos3, int nv, const int32_t* tris3, int nt, float spacing, uint64_t seed, int orient,
                                float voxel_size, float model_scale, int device, float* pos3_out, float* nrm3_out, int cap, int* n_out);

/* ---- tuning knobs (never change results beyond float summation order).
 * "lcp_variant": 99 = automatic (default): the scan fed from a per-wavefront LDS queue of the queries that have a list -- over
 *   index-ordered lists at cell edge epsilon (24, sparse scenes), over centre-sorted lists with triangle-inequality early exit
 *   at epsilon/2 or epsilon/4 (39, dense scenes); selectable cross-checks: 31 (the per-step cooperative scan of round 2 over the
 *   centre-sorted lists) and 0 (plain lane-per-query scan).  Every selectable kernel returns the reference's scores; any other
 *   value is STOCS_ERR_INVALID (the variants that lost their A/B runs are no longer in the code: DESIGN_HISTORY.md lists them).
 * "device_clock": 1 = stocs_find_congruent_all records HIP events between its kernel groups and stocs_last_call_timing reports them as
 *   "device: ..." steps; 0 (default; STOCS_DEVICE_CLOCK=1 in the environment turns it on at context creation) = the host's steps only --
 *   an event between two kernels of a stream costs ~5 us of idle queue on this runtime, nine of them 45 us of a 600 us call.
 * "lcp_flat": 1 (default) = sparse scenes address a flat copy of the cell table (one look-up per query), 0 = brick look-ups.
 * "lcp_normal_gate": 1 (default) = the cell words of the scene grid carry a cone of their list's scene normals, and on sparse
 *   lists the queue-fed scoring kernel drops a query before its list is touched when no normal
 *   inside the cell's cone can pass the 30-degree test against the rotated model normal; 0 = the forms without the gate; any
 *   other value is STOCS_ERR_INVALID.  A dropped query is one the ungated kernel would not count: same scores, bitwise.  The
 *   per-point detail forms and the cross-check kernels (lcp_variant 0, 31, exact_ties) never gate.
 * "lcp_patch_normals": 1 (default; STOCS_LCP_PATCH_NORMALS=0 in the environment turns it off at context creation) = the patch test
 *   of the shared-list forms ("lcp_split" 1, "lcp_cull_unit" 16, models of 512 to 8 192 points -- from 64 points on dense grids, which
 *   split every model) also drops a 16-point sub-patch when no scene normal within reach of it can pass the 30-degree test against
 *   any of its rotated normals: a cone of the scene normals per cell of the distance field against a cone per sub-patch
 *   (csrc/patch_normals.h); 0 = the sphere test alone; any other value is STOCS_ERR_INVALID.  A dropped sub-patch holds no point the
 *   kernel would count: same scores, bitwise.  Every other kernel form never runs the test, and a context that runs none of those
 *   forms never fills the field: the first launch of a shared-list form with the option on does (once per scene).  Its memory is
 *   taken with the scene's grid, when the option is on and the model's size allows such a form; turned on later, the option takes
 *   effect from the next scene.
 * "lcp_split": 1 (default) = four wavefronts share a candidate's model points, 0 = one wavefront per candidate.  Scores are
 *   accumulated as integers, so neither option changes a single bit of them.
 * "lcp_order": 0 = candidates in batch order, 1 (default) = big batches against scenes whose lists do not stay in the caches
 *   are processed in a spatial order of their translations (scores are bitwise independent of it), >= 2 = always ordered, in
 *   XCD-blocked variants of that order (k > 2: runs of k consecutive slots per XCD).
 * "lcp_cull": the patch test of the queue-fed scoring kernels.  The reference walks every model point of every candidate
 *   (stocs.cpp:1016-1035); a 64-point step of the model whose bounding sphere, under the candidate transform, is farther
 *   than epsilon from every scene point cannot add to the score and is skipped after one look-up in a distance field of
 *   the scene.  0 = off, 1 (default) = on once the field pays (1e9 candidates x model points scored against the scene so
 *   far: the field costs ~0.25 ms per scene and takes ~6 % off a launch), 2 = from the first call.  Same scores, bitwise.
 * "lcp_cull_unit": the points per bounding sphere of that test: 16 (default) = every 64-point step is tested as four 16-point
 *   sub-patches and the wavefront walks only the live ones, four to a step; 64 = whole steps.  Same scores, bitwise.
 * "lcp_cull_after": that threshold of "lcp_cull" = 1 in MILLIONS of point queries (candidates x model points scored against
 *   the current scene); default 1000, 0 = from the first call.  One trial of a 640x480 frame is 1-40 million: a caller that
 *   scores a single trial per frame never fills the field, a trial batch (stocs_run_trials) or a stream of candidate batches
 *   crosses the threshold within a call or two.  When the scene BEFORE the current one crossed it, stocs_ctx_set_scene fills
 *   the new scene's field at once, on the context's auxiliary stream (a frame stream on a fixed camera will cross it again).
 * "lcp_group": lanes that verify one queued query together in the queue-fed kernels: 4 (two entries of a 128-byte list line per
 *   lane, sixteen queries per trip).  The only value, in every build: anything else is STOCS_ERR_INVALID (8, one entry per lane,
 *   was the form of rounds 1-3a; DESIGN_HISTORY.md).
 * "exact_ties": 0 (default) = a query whose nearest scene points lie at exactly the same float32 distance takes the one with the
 *   largest scene index (divergence Q11: every other integer result already equals the reference's).  1 = it takes the point the
 *   reference's kd-tree (kdtree.h:394-459) returns -- the one its visiting order reaches last -- so that every (candidate, model
 *   point) query of every scoring entry point (stocs_score_transforms(_device), stocs_score_best_device(_async), stocs_verify_all,
 *   stocs_lcp_detail, stocs_lcp_hit_count, stocs_run_trials) returns exactly the reference's scene index, and scores and arg-max
 *   keys follow from those answers.  Costs: a host build of the reference-order tree per scene (at the first exact-mode scoring
 *   call after a scene change, or in stocs_ctx_set_scene when the option is already on; that call synchronises) and a slower
 *   scoring kernel (a lane per query, whole cell lists, no patch test; see DESIGN.md 2 for measured figures).  Default-mode
 *   kernels are untouched.  Other values are STOCS_ERR_INVALID.  This one option changes results (on exact ties only). ---- */
int stocs_set_option(stocs_ctx* ctx, const char* key, int value);
/* exact_ties counters of the context's last scoring entry point: *flagged = queries answered by the kd-tree (exact distance ties,
 * and single answers lying exactly at epsilon^2), *changed = those whose answer differs from the largest-index rule.  Both 0 when that
 * call ran in default mode.  Synchronises the context's stream. */
int stocs_last_tie_counts(stocs_ctx* ctx, int64_t* flagged, int64_t* changed);
/* Diagnostics of that patch test (tests only; no reference counterpart).  patches4: n_patches x (centre x, y, z, radius) in the
 * centred model frame, one per 64 consecutive slots of the sorted model; perm: sorted slot -> model index (|M| entries);
 * geom8: origin x, y, z, cell edge, cap, nx, ny, nz of the scene's distance field; dist: its nx*ny*nz values (x fastest;
 * the field is filled by this call if it was not yet): distance from a cell's centre to the nearest scene point, rounded
 * down, capped.  NULL outputs are skipped; *n_patches and *n_dist are always set (0 when the context has no field). */
int stocs_get_cull_state(stocs_ctx* ctx, float* patches4, int32_t* perm, int* n_patches, float* geom8, float* dist,
                         int64_t dist_cap, int64_t* n_dist);
/* The scene grid as the last stocs_ctx_create / stocs_ctx_set_scene built it (tests and diagnostics; no reference counterpart; host
 * records only: no device work, no synchronisation).  The scoring kernels locate a query q in cell floor((q - origin) * inv_h) per
 * axis, in float; a cell's list holds scene points within r of its box, r = 1.001 epsilon, or epsilon + 2^-21 of the grid's span on
 * scenes wider than about 2 100 epsilons (where the float rounding of that cell computation would use the thousandth up). */
#define STOCS_GRID_SORT_ROCPRIM 1
#define STOCS_GRID_SORT_OWN 2
typedef struct stocs_grid_info {
    float origin[3];        /* the float origin the kernels subtract */
    float h, inv_h;         /* cell edge (epsilon / div) and the float the kernels multiply by */
    int32_t div;            /* 1..4 */
    int32_t cells[3];       /* cells per axis */
    int32_t bricks[3];      /* bricks of 8x8x8 cells per axis (the top table has their product) */
    int32_t centre_sorted;  /* lists ordered by distance from the cell centre, with chunk bounds (else ascending scene index) */
    int32_t pruned;         /* lists hold only points that can win somewhere in their cell */
    int32_t has_nearest;    /* the z word of a cell is a distance bound (div > 1), not half of the sub-cell mask */
    int32_t has_cones;      /* the count word carries the cell's normal cone */
    int32_t has_flat;       /* the flat cell table exists */
    int32_t sort;           /* STOCS_GRID_SORT_*: which sort ordered the (cell, point) incidences */
    int32_t prune_group;    /* lanes per cell of the prune kernel, 16 or 64; 0 when not pruned */
    int32_t prune_k;        /* dominators tried per entry, 4, 8 or 16; 0 when not pruned */
    int32_t longest_list;   /* entries of the longest stored list, before padding to 8 */
    int32_t reserved;
    int64_t n_incidences;   /* (cell, point) pairs with the point within r of the cell's box */
    int64_t n_cells;        /* non-empty cells */
    int64_t n_bricks;       /* bricks with a non-empty cell */
    int64_t n_entries;      /* stored list entries, padding included */
} stocs_grid_info;
/* STOCS_ERR_INVALID for a NULL argument; STOCS_ERR_STATE ("no scene") for a context whose last scene was refused -- *info is zeroed. */
int stocs_get_grid_info(stocs_ctx* ctx, stocs_grid_info* info);
/* The octant lines of that grid (sparse pruned grids at cell edge epsilon with a flat table; STOCS_GRID_OCTANTS=0, read per build,
 * leaves them out), beside the struct above, whose layout is fixed: counts3[0] = cells whose stored list is longer
 * than one 128-byte line of 8 entries, [1] = those of them whose eight octants each fit one line (their flat-table word names the block
 * of octant lines; the rest stay plain), [2] = the entries of those cells' octant lines before padding.  [1] and [2] are 0 until the
 * scene has been scored for "lcp_cull_after" point queries: the launch that passes the threshold writes the lines.  n_entries above
 * counts the plain lists only.  Errors as above; the counts are zeroed. */
int stocs_get_grid_octants(stocs_ctx* ctx, int64_t* counts3);
/* The model-side half of that test without a context or a device (host code: what stocs_ctx_create computes): the order in
 * which the scoring kernels walk the model -- perm[slot] = model index, 64 consecutive slots = one compact surface patch --
 * and the bounding sphere of every patch (centre x, y, z in the CENTRED model frame, radius), ceil(nM / 64) of them. */
int stocs_model_patch_order(const float* model_pos3, int nM, int32_t* perm, float* patches4);
/* The unit of that test at "lcp_cull_unit" = 16, on the host likewise: the same perm (every 64-slot patch above is the union of four
 * 16-slot runs) and the bounding sphere of every run of 16 consecutive slots (centre x, y, z in the centred frame, radius),
 * ceil(nM / 16) of them. */
int stocs_model_subpatches(const float* model_pos3, int nM, int32_t* perm, float* spheres4);
/* The normal cone of each of those runs ("lcp_patch_normals"), on the host likewise: the same perm, and per run of 16 slots the unit
 * axis of its normals (x, y, z) and sb >= sin(beta), beta the largest angle of a member normal (model_nrm3 normalised in float, as
 * stocs_ctx_create does) against that axis, rounded outwards; sb < 0: the run takes no part in the test (beta above 45 degrees, a
 * normal that is not finite or has no direction).  ceil(nM / 16) records. */
int stocs_model_subpatch_normals(const float* model_pos3, const float* model_nrm3, int nM, int32_t* perm, float* records4);
/* The left-hand side of that test on the host (csrc/patch_normals.h, the function the kernel runs): for the field word `cone_word`
 * (octahedral axis of 2 x 12 bits, class k in bits 24..31), the rotated model axis v3, the model record's sb and the norm bound s of the
 * matrix.  *outside = 1 when v3 lies outside the scene cone (only then is a sub-patch ruled out).  axis3 (may be NULL) receives the axis
 * of the word as the kernel decodes it, not normalised. */
float stocs_patch_normal_bound_host(uint32_t cone_word, const float* v3, float sb, float s, int* outside, float* axis3);
/* Test aid for "lcp_patch_normals" (no reference counterpart): over n candidate transforms (device, column-major 4x4) and every
 * sub-patch of the model, out[0] = the sub-patches the sphere test leaves alive, out[1] = those of them that the normal-cone test rules
 * out, out[2] = those of out[1] that hold a point which the per-point detail form counts (must be 0).  Fills the distance field and
 * the cone field of the scene if need be.  All zero when the scene has no cone field (a model no shared-list form can
 * score: more than 8 192 points, or fewer than 512 on a sparse grid; the option off when the scene was set; an empty scene). */
int stocs_lcp_patch_normal_count(stocs_ctx* ctx, const void* d_T16, int n, int64_t out[3]);
/* What the context holds for "lcp_patch_normals" (host records, no device work): out[0] = the reach of the current scene's cone field
 * as the kernels are given it, in the units of the clouds (at most 5.9 cells of the distance field: csrc/patch_normals.h), 0 without
 * a field; out[1] = cells a scene point reaches on either side when the field is filled; out[2] = 1 when the field has been filled;
 * out[3] = the scoring launches of this context so far that ran a shared-list form WITH the cone test (counted over all scenes). */
int stocs_patch_normal_info(stocs_ctx* ctx, double out[4]);
/* The reference-order kd-tree of the "exact_ties" option on the host, for tests: builds the tree over n points pos3 as the reference
 * builds it (64 points per leaf, depth 32, widest axis split at the box midpoint, the same in-place partition) and answers nq
 * radius queries q3 with the query function the device runs: idx[i] = the reference's doQueryRestrictedClosestIndex(q3[i], sqdist),
 * -1 when no point lies within sqdist. */
int stocs_kdtree_nn_host(const float* pos3, int n, const float* q3, int nq, float sqdist, int32_t* idx);

/* ---- stream / timing plumbing ---- */
/* run the context's work on a caller-owned HIP stream (e.g. PyTorch's current stream, so that RCCL
 * collectives issued through torch.distributed are ordered after the kernels without a host sync);
 * NULL restores the context's own stream.  The caller keeps the stream alive. */
int stocs_set_stream(stocs_ctx* ctx, void* hip_stream);
/* asynchronous arg-max: writes the packed key (see stocs_best_device) to the 8 bytes at d_key8 on the
 * context's stream; no synchronisation */
int stocs_best_device_async(stocs_ctx* ctx, const void* d_lcp, int n, uint32_t id_offset, void* d_key8);
int   stocs_sync(stocs_ctx* ctx);
void* stocs_stream(stocs_ctx* ctx);          /* hipStream_t */
/* times `reps` back-to-back launches of the LCP kernel on n device-resident transforms with HIP
 * events on the context's stream; returns the average milliseconds per launch */
int stocs_time_score_kernel(stocs_ctx* ctx, const void* d_T16, int n, void* d_lcp, int reps,
                            float* avg_ms);
/* Debug aid: with STOCS_DEBUG_STREAMS=1 in the environment stocs_find_congruent_all and stocs_make_transforms -- the two entry
 * points that use the context's auxiliary stream -- check on the host, step by step, that every buffer used on both streams is
 * ordered by an event edge (main -> aux before its first use there, aux -> main before its next use or before its arena is
 * recycled) and return STOCS_ERR_STATE naming buffer and step otherwise.  The launches are the same with and without it.  This
 * runs the checker itself on canned sequences (no device): scenario 0 = the library's fork / join pattern (returns 0), 1-4 = one
 * missing edge each (return >= 1; first_msg receives the report). */
int stocs_debug_stream_audit_selftest(int scenario, char* first_msg, int cap);
/* Do the context's two streams run side by side?  1 = a kernel on the auxiliary stream ran WHILE one on the main stream was waiting
 * for it, 0 = it did not (both streams sit on one hardware queue of the runtime, GPU_MAX_HW_QUEUES: the two-stream sections of
 * stocs_find_congruent_all / stocs_make_transforms then run one after the other -- correct, ~13 % slower at Cm), < 0 = error.
 * stocs_ctx_create asks the same question and takes another auxiliary stream (up to four candidates) until the answer is 1;
 * STOCS_NO_STREAM_PROBE=1 in the environment skips that.  The context must be idle. */
int stocs_debug_streams_overlap(stocs_ctx* ctx);
/* Diagnostics of the library's own stable radix sort of (u32 key, u32 value) pairs (csrc/sort32.hip; the sort of the congruent-set
 * phase's pair lists -- in the reference a pointer grid of per-cell vectors, include/super4pcs/accelerators/normalset.hpp:114-131):
 * sorts n host pairs by key bits [0, end_bit) on `device` (-1: the current one), which = 1 with the library's sort, 0 with rocPRIM's;
 * `reps` timed runs after one warm-up; sorted pairs and the average device time of one sort come back.  seg_off (host, n_seg + 1 ascending
 * offsets; own sort only; NULL: the whole list): every segment is sorted on its own and stays where it is -- the form the congruent-set
 * phase uses, one segment per base. */
int stocs_debug_sort_pairs(int device, const uint32_t* keys, const uint32_t* vals, int64_t n, int end_bit, int which, int reps,
                           uint32_t* keys_out, uint32_t* vals_out, float* ms_per_sort, const uint32_t* seg_off, int n_seg);
/* number of device (hipMalloc) and pinned-host (hipHostMalloc) allocations the library has made in this process so far.
 * A warm context -- one that has run a trial of the current scene -- runs further trials without allocating: the
 * difference across them is 0. */
int64_t stocs_device_alloc_count(void);
/* host wall clock, in milliseconds, of the steps of the context's LAST stocs_find_congruent_all (which = 0),
 * stocs_make_transforms (1), stocs_verify_all (2), stocs_run_trials (3: its phases summed over the pieces of the batch), stocs_pose_errors
 * (4; with "device_clock" 1 also "device: kernel", the HIP-event time of its launches) stocs_pose_errors_sym (5; likewise), stocs_symmetry_errors (6; likewise) or stocs_pose_errors_vsd (7; likewise): always recorded (a few clock reads per call, no synchronisation of its
 * own), so that a call that stalls -- tens of milliseconds instead of one -- names the step it stalled in.  Steps are host
 * intervals between the call's existing synchronisation points: "wait for the device" steps hold the GPU work, the others
 * host work and runtime calls; entries whose label starts with "device:" are HIP-event times of the kernel groups that
 * wait covered.  At most 18 entries.  labels[i] point to static strings.  STOCS_ERR_CAPACITY when cap is too small (*n is set). */
int stocs_last_call_timing(const stocs_ctx* ctx, int which, const char** labels, double* ms, int cap, int* n);
/* device memory helpers so that callers without a HIP binding (ctypes) can keep inputs resident */
int stocs_dev_alloc(stocs_ctx* ctx, int64_t bytes, void** dptr);
int stocs_dev_free(stocs_ctx* ctx, void* dptr);
int stocs_dev_upload(stocs_ctx* ctx, void* dptr, const void* host, int64_t bytes);
int stocs_dev_download(stocs_ctx* ctx, void* host, const void* dptr, int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif
