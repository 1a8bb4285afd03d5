// stocs_single -- the repo's equivalent of the reference driver (reference src/stocs_match_one_object.cpp:51-215): same
// command line (scene directory + object name), same input files (depth.png, probability_maps/<object>.png, optional
// probability_maps/edge.png, models/<object>/model_search.ply + ppf_map), same four phases, same three timed spans printed
// in microseconds, same constants (:7-17), same output file (12 floats, 3x4 row-major, space separated, default ostream
// precision, :171-180), best_pose.ply / scene.ply in <scene>/dbg (stocs.hpp:136-149).  Host code is C++ on the façade
// include/stocs.hpp; all hot-path work runs in libstocs_hip.so on the GPU.
//
// The loops of the reference's caller (one call per base, :81-147) are taken through the façade's batched methods: all
// 100 attempts, all bases' congruent sets and all <= 200-per-base transforms are one GPU pass each, and the subset of a
// base with >= 200 congruent sets is the library's seeded rule (stocs_make_transforms).  The per-call spelling of the same
// sequence is tests/cpp/reference_call_sequence.cpp.
//
//   stocs_single <scene_path> <object_name> [--repo DIR] [--intrinsics fx,cx,fy,cy] [--depth-scale S] [--voxel V] ...
//   stocs_single --clouds <scene.stcl> <model.stcl> [--edge edge.u8] ...       (flat clouds, e.g. the synthetic workloads)
//   stocs_single <scene_path> <object_a,object_b,...> [options]   (several objects of the frame: one ingest, one context per object)
// common options: --seed N --bases 100 --max-sets 200 --out FILE --dbg DIR --cluster 1 --exact-ties 1
// --refine N (with --cluster 1): N point-to-plane iterations on every clustered hypothesis (clustering::point_to_plane_icp,
// pose_clustering.cpp:123-140, batched: stocs_refine_poses); the best refined pose goes to <out>.refined in the same format.
// --trim r [--normal-gate deg] (with --cluster 1 --refine N, without --trials): the robust refinement (stocs_refine_poses_robust): per
// iteration the nearest share r in (0, 1] of the pairs is kept, and a pair whose normals differ by more than deg is dropped (without
// --normal-gate: no gate).  Recommended: --trim 0.7 --normal-gate 30 -- on cluttered frames the plain refinement is pulled off the
// object; either rejector alone helps, only both hold on sparse clouds.  Without --trim the output is the plain one's.
// --trials N --cluster 1 [--refine K]: the clustering (and refinement) of every trial runs inside the batch, on the device
// (stocs_run_trials_post); per-trial cluster / refined lines, the best refined pose of the best trial to <out>.refined.
// --robust keep[,deg] (with --trials N --cluster 1 --refine K, the multi-instance forms included, or with --track <file> --cluster 1
// --refine K): the refinement inside the batch is the robust one (stocs_run_trials_post_robust): keep in (0, 1] and deg in [0, 180]
// as --trim and --normal-gate (without deg: no gate).  With --track it applies wherever that path refines: the detection the run
// falls back to (the batch with --trials, else the single run's refinement).  --robust 1 prints what the run prints without it.
// Refused, with a message naming --robust, when the values are out of range or there is nothing to refine.
// --track <pose file> [--track-min-lcp x] (single object): track from a prior pose in the format this driver writes (12 floats, 3x4
// row-major) -- a local search around it on this frame (stocs_track_poses, the façade's default parameters); when the tracked lcp is
// below x (default 0.02: a prior that has lost the object scores ~0) the usual detection runs instead.  Prints which route produced
// the pose ("track: route=tracked ..." / "track: route=detection ...") and writes <out> as detection does.
// --gt <pose file> (single object): a ground-truth pose in the same format.  After the run, "gt <object>: add=... add_max=... adds=...
// adds_max=... diameter=... adds_over_diameter=... valid=..." (metres; stocs_pose_errors on the pose file this run wrote, read back as the
// ground truth is) and, with --trials N, "gt <object> recall: trials=N valid=... threshold=... add=... adds=...": the share of the trials'
// winners whose ADD / ADD-S is below 0.1 diameter (with --track only when the run fell back to detection: a tracked pose ran no trials).
// A pose file left at <out> by an earlier run is removed first; when this run finds no pose the line reads "gt <object>: no pose".
// --sym a,b,c [--sym-steps n] [--sym-file <K x 16 floats>] (with --gt): the errors under the model's symmetries as well (stocs_pose_errors_sym).
// a,b,c is the clustering's descriptor (0, 90, 180 or 360 per axis; stocs_symmetry_set, a continuous axis in n steps, default 72);
// --sym-file replaces the generated set by an explicit one (text, 16 floats per transform, column-major).  After the gt line,
// "gt <object> sym: symmetries=K mssd=... k_mssd=... add=... k_add=... [mspd=... k_mspd=...] valid=..." (mspd when the run has a
// camera: a scene directory) and, with --trials N, one "gt <object> sym trial t: mssd=... add=... [mspd=...] valid=..." line per trial's
// winner and "gt <object> sym recall: trials=N valid=... mssd=... add=... [mspd=...]": BOP's average
// recall of MSSD over 0.05 .. 0.50 diameters, the share with the symmetric ADD below 0.1 diameter, and the average recall of MSPD over
// 5 .. 50 pixels x image width / 640.  Without --sym the output is what it is without these options.
// --vsd [--vsd-delta m] [--surfel-radius m] (with --gt, a scene directory, a single object): BOP's visible-surface discrepancy on the
// frame's own depth image as well (stocs_pose_errors_vsd; the library's delta 0.015 and surfel radius 0.006 unless given).  After the gt
// lines, "gt <object> vsd: taus=10 delta=... surfel_radius=... e0=... .. e9=... mean=... px_est=... px_gt=... vis_est=... vis_gt=...
// inter=... uni=... valid=...": the errors at the misalignment tolerances 0.05, 0.10 .. 0.50 model diameters and their mean; with
// --trials N one "gt <object> vsd trial t: e0=... .. e9=... valid=..." line per trial's winner and "gt <object> vsd recall: trials=N
// valid=... vsd=...": BOP's average recall of VSD, the mean over the ten taus and the correctness thresholds 0.05 .. 0.50 of the share of
// ALL trials with e below the threshold (a trial without a pose counts as wrong: VSD is defined for it).  Without --vsd the output is
// what it is without these options.  --mesh <ply> (with --vsd): the model as a triangle mesh, in the frame of the model cloud; the VSD
// lines then come from the exact rasteriser (stocs_pose_errors_vsd_mesh) and say "mesh=<triangles>" where they said "surfel_radius=...".
// --depth-check (with --trials N --cluster 1 [--refine K], a scene directory): every trial's hypotheses -- the refined poses when
// refinement ran -- scored against the frame's own depth image and class-probability map (stocs_depth_check_poses); one "depth t.i:"
// line per hypothesis, and <out> is written from the first maximum of score - violation (ties: the higher lcp, then the lower trial
// and hypothesis index) instead of the LCP winner.  Every other line is what the run prints without the flag.
// --instances M [--instance-min-fraction f] [--instance-min-points p] (with --trials N --cluster 1 [--refine K]): the hypotheses of all
// trials -- the refined poses when refinement ran -- go through stocs_select_instances in one call (at most M instances; f and p default
// to the library's 0.5 and 20); one "instance r: trial.hyp own exclusive lcp" line per selected instance, and their poses, 3x4 row-major,
// one per line in rank order, to pose_instances_<object>.txt next to <out> (<object>: the object name, with --clouds the model file's
// name without its extension).  Every other line and file is what the run writes without the flag.
// --scene-select [--scene-max-per-object K] [--masks] (several objects, --trials N): once every object is searched, the N trial winners of
// every object -- camera-frame poses, one pool over all objects -- are judged together on the pixels of the depth image
// (stocs::select_scene): walked best first, a pose is kept only if enough of the depth pixels that agree with it are claimed by none
// kept before it, whatever object it belongs to.  One "scene r: object .. trial .. score .. own .. exclusive .. reason .." line per pool
// entry, the selected ones first in rank order (r = rank), then the others in pool order (r = -1), and the same entries with their poses
// to <scene>/scene_selection.txt.  With --masks the selected poses of all objects are rendered into one key buffer and the label image
// goes to <scene>/labels_scene.pgm (value = pool slot + 1, 0 = nobody; the format of labels_<object>.pgm).
// --surface points|mesh (default points; mesh needs --mesh <ply> and --masks with --instances M, refused before any search otherwise): with
// mesh the "mask r:" lines and the label image come from the exact rasteriser on that mesh (stocs_explain_poses_mesh) and every line ends
// in " mesh=<triangles>".  --mesh then needs no --vsd.  Several objects with --scene-select stay on points: one mesh file names one object.
// --refine-visible K[,dist[,cos]] (needs --mesh <ply>, a scene directory, a single object; --mesh then needs no --vsd): after every other
// step, the pose this run wrote to <out> is refined on the mesh against the frame's own depth image and class-probability map
// (stocs_refine_poses_visible: K iterations, max_distance dist and min_view_cos cos, the library's defaults unless given) and <out> is
// written again from the result; K = 0 scores the pose and leaves the file.  One "refine-visible <object>: iterations=.. frozen=..
// present=.. no_depth=.. off_class=.. too_far=.. grazing=.. counted=.. rms=.. mesh=<triangles>" line and the refined "pose:" line; with
// --gt a "refine-visible <object> before: add=.. adds=.." and an "after" line (stocs_pose_errors), and the gt lines score the refined file.
// --contour [w[,radius_px[,dist_m]]] (with --refine-visible and --damped; without --damped an error naming it): the damped form with the
// contour term (stocs_refine_poses_visible_contour: uncovered object pixels of the class image pull the pose); the line then reads
// "refine-visible <object>: contour iterations=.. .. rms=.. object_px=.. uncovered=.. unreached=.. beyond=.. pulled=.. pull_rms=.. mesh=..".
// --damped [lambda0[,rot_deg[,trans_m]]] (with --refine-visible): the damped form (stocs_refine_poses_visible_damped: K + 1 evaluations, steps
// bounded by rot_deg degrees and trans_m metres, taken only when they lower the cost, about the mean of the mesh's vertices; the library's
// defaults unless given); the line then reads "refine-visible <object>: damped iterations=.. rejected=.. evaluations=.. cost=.. lambda=..
// frozen=.. present=.. .. mesh=<triangles>" and describes the pose that is written.
// --masks (with --instances M, a scene directory): the selected instances, in rank order, rendered together against the frame's depth image
// and class-probability map (stocs_explain_poses); one "mask r: footprint .. visible .. hidden .. agree .. in_front .. behind .. no_depth ..
// on_mask .." line per instance, and the label image to labels_<object>.pgm next to <out>: binary 16-bit PGM (P5, maxval 65535, most
// significant byte first), value = rank + 1, 0 = no instance.  Every other line and file is what the run writes without the flag.
// --segment [tol[,min_pixels]] (a scene directory, a single object): a depth-only frame.  probability_maps is not read: the class image is made
// from depth.png (stocs_segment_frame: the support plane within tol metres removed, what stands on it split into depth-connected segments of
// min_pixels or more; the library's defaults unless given) and goes to the ingest and, where a frame is set, to set_frame; one "segment: plane
// found (n0 n1 n2 d), .. pixels on it, .. components, .. segments kept" line.  --segment-edges (with --segment, refused without it): the edge
// image of the same call goes to stocs_set_edge_map, so sampling runs in instance mode.  --segment-convex [r[,s[,deg]]] (with --segment,
// refused without it): touching objects are cut apart at concave creases before the labelling (stocs_segment_frame_convex: bend radius and
// smoothing radius in pixels, the bend angle in degrees, which becomes bend_cos here; the library's defaults unless given), and a
// "segment convex: .. triples tested, .. cut, .. pixels cut" line follows.
// <scene> a,b,c --segment [...] [--segment-gate slack[,min_ratio]]: several objects of a depth-only frame.  One stocs_segment_frame, one
// stocs_segment_assign (each segment's 3-D shape against each object's size, from its model cloud: the extents of stocs_points_shape and
// their diagonal as the diameter; the library's gate defaults unless given), the per-object class stack into the multi-object ingest; one
// "segment assign: <object>: k of n segments" line per object.  The gate is not exclusive: objects of like size keep the same segments
// (--scene-select chooses among them).  --segment-gate without --segment is refused; with a single object it takes the same path.
// The reference edits its per-data-set constants in the source (README.md:42-66); here they are options with the
// reference's YCB values as defaults.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pose_clustering.hpp"
#include "../../include/stocs.hpp"

// reference stocs_match_one_object.cpp:4-24
static std::string repo_path = ".";
static float voxel_size = 0.005f;
static float distance_threshold = 0.005f;
static int ppf_tr_discretization = 5;
static int ppf_rot_discretization = 5;
static float edge_threshold = 0;
static float class_threshold = 0.10f;
static float sample_dispersion = 0.9f;
static int number_of_bases = 100;
static int maximum_congruent_sets = 200;
static std::vector<float> cam_intrinsics = {1066.778f, 312.986f, 1067.487f, 241.310f};  // YCB
static float depth_scale = 1 / 10000.0f;
static int image_width = 640, image_height = 480;
static bool g_robust = false;                       // --robust keep[,deg]: the batched refinement is the robust one
static float g_robust_keep = 1.0f, g_robust_deg = -1.0f;   // (< 0: no gate)
static float g_trim = 0.0f, g_gate_deg = -1.0f;   // --trim r [--normal-gate deg]: the robust refinement (0: the plain one; < 0: no gate)

static bool read_stcl(const std::string& path, std::vector<float>& pos, std::vector<float>& nrm, std::vector<float>* prob, std::vector<int32_t>* pixel) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char magic[8];
    int32_t n = 0, flags = 0;
    bool ok = fread(magic, 1, 8, f) == 8 && std::string(magic, 8) == "STOCSCL1" && fread(&n, 4, 1, f) == 1 && fread(&flags, 4, 1, f) == 1 && n >= 0;
    if (ok) {
        pos.resize((size_t)n * 3); nrm.resize((size_t)n * 3);
        ok = fread(pos.data(), 4, pos.size(), f) == pos.size() && fread(nrm.data(), 4, nrm.size(), f) == nrm.size();
        if (ok && (flags & 1)) { std::vector<float> p(n); ok = fread(p.data(), 4, n, f) == (size_t)n; if (prob) *prob = p; }
        else if (prob) prob->assign(n, 1.0f);
        if (ok && (flags & 2)) { std::vector<int32_t> px((size_t)n * 2); ok = fread(px.data(), 4, px.size(), f) == px.size(); if (pixel) *pixel = px; }
    }
    fclose(f);
    return ok;
}

// everything after the estimator is built (:79-185): one run, or n_trials in one batch; lines to os, the pose to out_path
static int g_mask_mesh_triangles = 0;   // --surface mesh: the triangles of the mesh set on the estimator; 0: the masks come from the model points

static int run_search(stocs::stocs_estimator& stocs_ptr, std::ostream& os, const std::string& out_path, const std::string& dbg_dir, uint64_t seed, int n_trials,
                      int exact_ties, int do_cluster, int n_refine, int depth_check = 0, const stocs_instance_params* instances = NULL,
                      const std::string& instances_path = std::string(), const std::string& labels_path = std::string(),
                      std::vector<stocs::stocs_estimator::TrialResult>* trial_results = NULL) {
    stocs_ptr.set_seed(seed);
    if (exact_ties) stocs_ptr.set_exact_ties(true);

    if (n_trials > 0) {
        // BASELINE config 4: N independent StoCS trials -- each the whole loop of run_stocs_estimation (:79-165) with its own seed --
        // in ONE set of launches (stocs_run_trials); the best pose over the trials is the result
        // --cluster 1 [--refine K]: every trial's candidates clustered (and the kept ones refined) inside the batch, on the device
        // (stocs_run_trials_post), with the single-trial block's clustering constants
        std::vector<stocs::stocs_estimator::TrialResult> res;
        std::vector<std::vector<PoseCandidate*> > hyps, refined;
        auto t0 = std::chrono::high_resolution_clock::now();
        int best;
        if (do_cluster) {
            stocs_trial_post post;
            post.acceptable_fraction = 0.8f; post.maximum_pose_count = 10; post.min_distance = 0.02f; post.min_angle = 15.0f;
            post.sym3[0] = post.sym3[1] = post.sym3[2] = 0.0f;
            post.refine_iterations = n_refine; post.max_correspondence_distance = 0.035f;
            best = g_robust ? stocs_ptr.run_trials(n_trials, seed, number_of_bases, maximum_congruent_sets, sample_dispersion, post, &res, &hyps, &refined,
                                                   g_robust_keep, g_robust_deg)
                            : stocs_ptr.run_trials(n_trials, seed, number_of_bases, maximum_congruent_sets, sample_dispersion, post, &res, &hyps, &refined);
        } else {
            best = stocs_ptr.run_trials(n_trials, seed, number_of_bases, maximum_congruent_sets, sample_dispersion, &res);
        }
        auto t1 = std::chrono::high_resolution_clock::now();
        long long cand = 0;
        for (size_t t = 0; t < res.size(); ++t) {
            cand += res[t].n_candidates;
            os << "trial " << t << ": bases " << res[t].n_bases << " congruent sets " << res[t].n_congruent_sets << " candidates " << res[t].n_candidates
               << " best lcp " << res[t].best_lcp << std::endl;
            if (do_cluster && t < hyps.size()) {
                os << "trial " << t << " clustered hypotheses: " << hyps[t].size() << std::endl;
                for (size_t i = 0; i < hyps[t].size(); ++i) os << "  cluster " << i << ": base " << hyps[t][i]->base_index << " lcp " << hyps[t][i]->lcp << std::endl;
                for (size_t i = 0; n_refine > 0 && i < refined[t].size(); ++i)
                    os << "  refined " << i << ": base " << refined[t][i]->base_index << " lcp " << hyps[t][i]->lcp << " -> " << refined[t][i]->lcp << std::endl;
            }
        }
        const long long us = (long long)std::chrono::duration_cast<micro>(t1 - t0).count();
        char tl[256];
        snprintf(tl, sizeof(tl), "trials: n=%d best_trial=%d best_lcp=%.9g candidates=%lld total_microseconds=%lld", n_trials, best,
                 best >= 0 ? (double)res[(size_t)best].best_lcp : 0.0, cand, us);
        if (PoseCandidate* bp = stocs_ptr.get_best_trial_pose()) {
            std::ofstream o(out_path, std::ofstream::out);
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) o << bp->transform(r, c) << (r == 2 && c == 3 ? "" : " ");
            o << std::endl;
            os << "pose:";
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) { char b[32]; snprintf(b, sizeof(b), " %.9g", (double)bp->transform(r, c)); os << b; }
            os << std::endl;
            // the best refined hypothesis (first maximum of the rescored lcp) of the best trial
            PoseCandidate* rb = NULL;
            for (size_t i = 0; n_refine > 0 && best >= 0 && (size_t)best < refined.size() && i < refined[(size_t)best].size(); ++i)
                if (!rb || refined[(size_t)best][i]->lcp > rb->lcp) rb = refined[(size_t)best][i];
            if (rb) {
                std::ofstream rf(out_path + ".refined", std::ofstream::out);
                for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) rf << rb->transform(r, c) << (r == 2 && c == 3 ? "" : " ");
                rf << std::endl;
                os << "refined pose:";
                for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) { char b[32]; snprintf(b, sizeof(b), " %.9g", (double)rb->transform(r, c)); os << b; }
                os << std::endl;
            }
        } else {
            os << "no pose found" << std::endl;
        }
        os << tl << std::endl;
        if (trial_results) *trial_results = res;
        if (depth_check) {
            const std::vector<std::vector<PoseCandidate*> >& src = n_refine > 0 ? refined : hyps;
            std::vector<PoseCandidate*> flat;
            std::vector<std::pair<int, int> > id;
            for (size_t t = 0; t < src.size(); ++t)
                for (size_t i = 0; i < src[t].size(); ++i) { flat.push_back(src[t][i]); id.push_back(std::make_pair((int)t, (int)i)); }
            const std::vector<stocs_depth_result> dr = stocs_ptr.depth_check_poses(flat);
            if (dr.size() != flat.size()) { std::cerr << "depth check failed: " << stocs_last_error() << std::endl; return 2; }
            int w = -1;
            for (size_t k = 0; k < dr.size(); ++k) {
                char b[384];
                snprintf(b, sizeof(b), "  depth %d.%d: facing %d in_image %d self_occluded %d no_depth %d agree %d in_front %d behind %d on_mask %d score %.9g violation %.9g lcp %.9g",
                         id[k].first, id[k].second, dr[k].facing, dr[k].in_image, dr[k].self_occluded, dr[k].no_depth, dr[k].agree, dr[k].in_front, dr[k].behind,
                         dr[k].on_mask, (double)dr[k].score, (double)dr[k].violation, (double)flat[k]->lcp);
                os << b << std::endl;
                // first maximum of score - violation; on a tie the higher lcp; then the lower (trial, hypothesis), i.e. the earlier k
                const float key = dr[k].score - dr[k].violation;
                if (w < 0 || key > dr[(size_t)w].score - dr[(size_t)w].violation ||
                    (key == dr[(size_t)w].score - dr[(size_t)w].violation && flat[k]->lcp > flat[(size_t)w]->lcp))
                    w = (int)k;
            }
            if (w >= 0) {
                const PoseCandidate* bp = flat[(size_t)w];
                std::ofstream o(out_path, std::ofstream::out);
                for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) o << bp->transform(r, c) << (r == 2 && c == 3 ? "" : " ");
                o << std::endl;
                os << "depth pose:";
                for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) { char b[32]; snprintf(b, sizeof(b), " %.9g", (double)bp->transform(r, c)); os << b; }
                os << std::endl;
                char b[256];
                snprintf(b, sizeof(b), "depth check: hypotheses=%d best_trial=%d best_hypothesis=%d score=%.9g violation=%.9g lcp=%.9g", (int)dr.size(), id[(size_t)w].first,
                         id[(size_t)w].second, (double)dr[(size_t)w].score, (double)dr[(size_t)w].violation, (double)bp->lcp);
                os << b << std::endl;
            } else {
                os << "depth check: hypotheses=0" << std::endl;
            }
        }
        if (instances) {
            const std::vector<std::vector<PoseCandidate*> >& src = n_refine > 0 ? refined : hyps;
            std::vector<PoseCandidate*> flat;
            std::vector<std::pair<int, int> > id;
            for (size_t t = 0; t < src.size(); ++t)
                for (size_t i = 0; i < src[t].size(); ++i) { flat.push_back(src[t][i]); id.push_back(std::make_pair((int)t, (int)i)); }
            std::vector<int> sel;
            const std::vector<stocs_instance_result> rec = stocs_ptr.select_instances(flat, &sel, *instances);
            if (rec.size() != flat.size()) { std::cerr << "instance selection failed: " << stocs_last_error() << std::endl; return 2; }
            std::ofstream o(instances_path, std::ofstream::out);
            for (size_t r = 0; r < sel.size(); ++r) {
                const size_t k = (size_t)sel[r];
                char b[192];
                snprintf(b, sizeof(b), "instance %d: %d.%d own %d exclusive %d lcp %.9g", (int)r, id[k].first, id[k].second, rec[k].own, rec[k].exclusive, (double)rec[k].lcp);
                os << b << std::endl;
                for (int rr = 0; rr < 3; ++rr) for (int c = 0; c < 4; ++c) { snprintf(b, sizeof(b), "%.9g", (double)flat[k]->transform(rr, c)); o << b << (rr == 2 && c == 3 ? "" : " "); }
                o << std::endl;
            }
            os << "instances: hypotheses=" << flat.size() << " selected=" << sel.size() << std::endl;
            if (!labels_path.empty()) {
                std::vector<PoseCandidate*> chosen;
                for (size_t r = 0; r < sel.size(); ++r) chosen.push_back(flat[(size_t)sel[r]]);
                std::vector<int32_t> labels;
                const std::vector<stocs_render_result> mr = g_mask_mesh_triangles > 0 ? stocs_ptr.explain_poses_mesh(chosen, &labels) : stocs_ptr.explain_poses(chosen, &labels);
                if (mr.size() != chosen.size() || labels.empty()) { std::cerr << "mask rendering failed: " << stocs_last_error() << std::endl; return 2; }
                for (size_t r = 0; r < mr.size(); ++r) {
                    char b[256];
                    int at = snprintf(b, sizeof(b), "mask %d: footprint %d visible %d hidden %d agree %d in_front %d behind %d no_depth %d on_mask %d", (int)r, mr[r].footprint,
                                      mr[r].visible, mr[r].hidden, mr[r].agree, mr[r].in_front, mr[r].behind, mr[r].no_depth, mr[r].on_mask);
                    if (g_mask_mesh_triangles > 0) snprintf(b + at, sizeof(b) - (size_t)at, " mesh=%d", g_mask_mesh_triangles);
                    os << b << std::endl;
                }
                std::vector<unsigned char> px(labels.size() * 2);
                for (size_t i = 0; i < labels.size(); ++i) { const unsigned v = (unsigned)(labels[i] + 1); px[2 * i] = (unsigned char)(v >> 8); px[2 * i + 1] = (unsigned char)(v & 255u); }
                std::ofstream pg(labels_path, std::ofstream::out | std::ofstream::binary);
                pg << "P5\n" << image_width << " " << image_height << "\n65535\n";
                pg.write((const char*)px.data(), (std::streamsize)px.size());
            }
        }
        return 0;
    }

    // Step 1: sample n bases on the scene (:79-105)
    auto start = std::chrono::high_resolution_clock::now();
    const int n_bases = stocs_ptr.sample_bases(number_of_bases, sample_dispersion);
    auto finish = std::chrono::high_resolution_clock::now();
    os << "Sampled " << n_bases << " bases in " << std::chrono::duration_cast<micro>(finish - start).count() << " microseconds\n";
    auto total_time = std::chrono::duration_cast<micro>(finish - start).count();

    // Step 2 + 3: congruent sets and rigid transforms (:107-153)
    start = std::chrono::high_resolution_clock::now();
    const long long total_congruent_set_found = stocs_ptr.find_congruent_sets_all();
    const int n_candidates = stocs_ptr.make_transforms(maximum_congruent_sets);
    finish = std::chrono::high_resolution_clock::now();
    os << "found " << total_congruent_set_found << " congruent sets in " << std::chrono::duration_cast<micro>(finish - start).count() << " microseconds\n";
    total_time += std::chrono::duration_cast<micro>(finish - start).count();

    // Step 4: verify all transforms to get the best pose (:155-165)
    start = std::chrono::high_resolution_clock::now();
    stocs_ptr.compute_best_transform();
    finish = std::chrono::high_resolution_clock::now();
    os << "evaluated transforms in " << std::chrono::duration_cast<micro>(finish - start).count() << " microseconds\n";
    total_time += std::chrono::duration_cast<micro>(finish - start).count();

    PoseCandidate* best_pose = stocs_ptr.get_best_pose();
    char line[256];
    snprintf(line, sizeof(line), "summary: bases=%d congruent_sets=%lld candidates=%d best_lcp=%.9g best_index=%d total_microseconds=%lld", n_bases,
             total_congruent_set_found, n_candidates, (double)stocs_ptr.get_best_score(), stocs_ptr.get_best_index(), (long long)total_time);
    if (!dbg_dir.empty()) stocs_ptr.visualize_best_pose();   // :167
    if (best_pose != NULL) {  // :171-180
        std::ofstream out_file_ptr;
        out_file_ptr.open(out_path, std::ofstream::out);
        out_file_ptr << best_pose->transform(0, 0) << " " << best_pose->transform(0, 1) << " " << best_pose->transform(0, 2) << " " << best_pose->transform(0, 3) << " "
                     << best_pose->transform(1, 0) << " " << best_pose->transform(1, 1) << " " << best_pose->transform(1, 2) << " " << best_pose->transform(1, 3) << " "
                     << best_pose->transform(2, 0) << " " << best_pose->transform(2, 1) << " " << best_pose->transform(2, 2) << " " << best_pose->transform(2, 3) << std::endl;
        out_file_ptr.close();
        // full-precision copy of the same 12 numbers for tools that compare poses
        os << "pose:";
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) { char b[32]; snprintf(b, sizeof(b), " %.9g", (double)best_pose->transform(r, c)); os << b; }
        os << std::endl;
        if (do_cluster) {  // clustering::greedy_clustering (pose_clustering.cpp:79-121; no caller in the reference): 0.8, best, 10, 2 cm, 15 deg, no symmetry
            std::vector<PoseCandidate*> all = stocs_ptr.get_pose_candidates(), kept;
            clustering::greedy_clustering(all, 0.8f, stocs_ptr.get_best_score(), 10, 0.02f, 15.0f, VectorType(0, 0, 0), kept);
            os << "clustered hypotheses: " << kept.size() << std::endl;
            for (size_t i = 0; i < kept.size(); ++i) os << "  cluster " << i << ": base " << kept[i]->base_index << " lcp " << kept[i]->lcp << std::endl;
            if (n_refine > 0) {
                const std::vector<PoseCandidate*> ref = g_trim > 0.0f ? stocs_ptr.refine_pose_candidates_robust(kept, n_refine, 0.035f, g_trim, g_gate_deg)
                                                                      : stocs_ptr.refine_pose_candidates(kept, n_refine);
                PoseCandidate* rb = NULL;
                for (size_t i = 0; i < ref.size(); ++i) {
                    os << "  refined " << i << ": base " << ref[i]->base_index << " lcp " << kept[i]->lcp << " -> " << ref[i]->lcp << std::endl;
                    if (!rb || ref[i]->lcp > rb->lcp) rb = ref[i];   // first maximum
                }
                if (rb) {
                    std::ofstream rf(out_path + ".refined", std::ofstream::out);
                    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) rf << rb->transform(r, c) << (r == 2 && c == 3 ? "" : " ");
                    rf << std::endl;
                    os << "refined pose:";
                    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) { char b[32]; snprintf(b, sizeof(b), " %.9g", (double)rb->transform(r, c)); os << b; }
                    os << std::endl;
                }
            }
        }
    } else {
        os << "no pose found" << std::endl;
    }
    os << line << std::endl;
    return 0;
}

// a pose file in the format this driver writes (12 floats, 3x4 row-major): the reader of --track and --gt
static bool read_pose_file(const std::string& path, MatrixType& m) {
    std::ifstream f(path);
    float v[12];
    for (int i = 0; i < 12; ++i)
        if (!(f >> v[i])) return false;
    m = MatrixType();   // identity; the bottom row stays 0 0 0 1
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) m(r, c) = v[r * 4 + c];
    return true;
}

// --gt: the pose this run wrote to out_path, read back with the reader the ground truth goes through (what is scored is what a reader of
// the file gets), against the ground truth: ADD, ADD-S, their maxima, the model's diameter (stocs_pose_errors, stocs_model_diameter); with
// --trials N also the share of the trials' winners (full precision, a trial without a pose left out) within 0.1 diameter
struct RefineVisibleOptions { bool on; int iterations; float distance, view_cos; int mesh_triangles; bool damped; float lambda0, rot_deg, trans_m, pivot[3]; bool contour; float weight; int radius_px; float pull_m; };   // --refine-visible K[,dist[,cos]]; a value < 0 leaves the library's default
struct VsdOptions { bool on; float delta, surfel_radius; int mesh_triangles; };   // --vsd; a value <= 0 leaves the library's default; mesh_triangles > 0: --mesh

// the ten errors of a VSD record as " e0=... .. e9=..." at b + at; returns the new end
static int print_vsd_errors(char* b, size_t cap, int at, const stocs_vsd_record& r, int n_tau) {
    for (int t = 0; t < n_tau; ++t) at += snprintf(b + at, cap - (size_t)at, " e%d=%.9g", t, (double)r.e[t]);
    return at;
}

// --refine-visible: the pose this run wrote to out_path, read back as --gt reads it, refined on the mesh against the frame; out_path is
// written again in the format the search writes it
// the parameters of --refine-visible .. --damped ..: the library's defaults unless given
static stocs_refine_visible_damped_params damped_params_of(const RefineVisibleOptions& rv) {
    stocs_refine_visible_damped_params prm = stocs::stocs_estimator::default_refine_visible_damped_params();
    prm.base.max_iterations = rv.iterations;
    if (rv.distance >= 0.0f) prm.base.max_distance = rv.distance;
    if (rv.view_cos >= 0.0f) prm.base.min_view_cos = rv.view_cos;
    if (rv.lambda0 >= 0.0f) prm.lambda0 = rv.lambda0;
    if (rv.rot_deg >= 0.0f) prm.max_step_rotation = (float)((double)rv.rot_deg * 3.14159265358979323846 / 180.0);
    if (rv.trans_m >= 0.0f) prm.max_step_translation = rv.trans_m;
    for (int k = 0; k < 3; ++k) prm.pivot_model[k] = rv.pivot[k];
    return prm;
}

// the parameters of --refine-visible .. --damped .. --contour ..: the library's defaults unless given
static stocs_refine_visible_contour_params contour_params_of(const RefineVisibleOptions& rv) {
    stocs_refine_visible_contour_params prm = stocs::stocs_estimator::default_refine_visible_contour_params();
    prm.damped = damped_params_of(rv);
    if (rv.weight >= 0.0f) prm.contour_weight = rv.weight;
    if (rv.radius_px >= 0) prm.pull_radius_px = rv.radius_px;
    if (rv.pull_m >= 0.0f) prm.pull_distance = rv.pull_m;
    return prm;
}

static int run_refine_visible(stocs::stocs_estimator& est, const RefineVisibleOptions& rv, const std::string& out_path, const std::string& object, const std::string& gt_path) {
    MatrixType p, g;
    if (!read_pose_file(out_path, p)) { std::cout << "refine-visible " << object << ": no pose" << std::endl; return 0; }
    stocs_refine_visible_params prm = stocs::stocs_estimator::default_refine_visible_params();
    prm.max_iterations = rv.iterations;
    if (rv.distance >= 0.0f) prm.max_distance = rv.distance;
    if (rv.view_cos >= 0.0f) prm.min_view_cos = rv.view_cos;
    PoseCandidate e(p, 0.0f, -1.0f);
    std::vector<MatrixType> refined;
    std::vector<stocs_refine_visible_result> r;
    char b[960];
    if (rv.contour) {
        const std::vector<stocs_refine_visible_contour_result> d = est.refine_poses_visible_contour(std::vector<PoseCandidate*>(1, &e), &refined, contour_params_of(rv));
        if (d.size() != 1 || refined.size() != 1) { std::cerr << "refine-visible failed: " << stocs_last_error() << std::endl; return 2; }
        r.push_back(d[0].damped.base);
        snprintf(b, sizeof(b), "refine-visible %s: contour iterations=%d rejected=%d evaluations=%d cost=%.9g lambda=%.9g frozen=%d present=%d no_depth=%d off_class=%d too_far=%d "
                 "grazing=%d counted=%d rms=%.9g object_px=%d uncovered=%d unreached=%d beyond=%d pulled=%d pull_rms=%.9g mesh=%d", object.c_str(), r[0].iterations,
                 d[0].damped.rejected, d[0].damped.evaluations, (double)d[0].damped.cost, (double)d[0].damped.lambda, r[0].frozen, r[0].present, r[0].no_depth, r[0].off_class,
                 r[0].too_far, r[0].grazing, r[0].counted, (double)r[0].rms, d[0].object_px, d[0].uncovered, d[0].unreached, d[0].beyond, d[0].pulled, (double)d[0].pull_rms,
                 rv.mesh_triangles);
    } else if (rv.damped) {
        const std::vector<stocs_refine_visible_damped_result> d = est.refine_poses_visible_damped(std::vector<PoseCandidate*>(1, &e), &refined, damped_params_of(rv));
        if (d.size() != 1 || refined.size() != 1) { std::cerr << "refine-visible failed: " << stocs_last_error() << std::endl; return 2; }
        r.push_back(d[0].base);
        snprintf(b, sizeof(b), "refine-visible %s: damped iterations=%d rejected=%d evaluations=%d cost=%.9g lambda=%.9g frozen=%d present=%d no_depth=%d off_class=%d too_far=%d "
                 "grazing=%d counted=%d rms=%.9g mesh=%d", object.c_str(), r[0].iterations, d[0].rejected, d[0].evaluations, (double)d[0].cost, (double)d[0].lambda, r[0].frozen,
                 r[0].present, r[0].no_depth, r[0].off_class, r[0].too_far, r[0].grazing, r[0].counted, (double)r[0].rms, rv.mesh_triangles);
    } else {
        r = est.refine_poses_visible(std::vector<PoseCandidate*>(1, &e), &refined, prm);
        if (r.size() != 1 || refined.size() != 1) { std::cerr << "refine-visible failed: " << stocs_last_error() << std::endl; return 2; }
        snprintf(b, sizeof(b), "refine-visible %s: iterations=%d frozen=%d present=%d no_depth=%d off_class=%d too_far=%d grazing=%d counted=%d rms=%.9g mesh=%d", object.c_str(),
                 r[0].iterations, r[0].frozen, r[0].present, r[0].no_depth, r[0].off_class, r[0].too_far, r[0].grazing, r[0].counted, (double)r[0].rms, rv.mesh_triangles);
    }
    std::cout << b << std::endl;
    if (r[0].iterations > 0) {
        std::ofstream f(out_path, std::ofstream::out);
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) f << refined[0](i, j) << (i == 2 && j == 3 ? "" : " ");
        f << std::endl;
    }
    std::cout << "pose:";
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) { char t[32]; snprintf(t, sizeof(t), " %.9g", (double)refined[0](i, j)); std::cout << t; }
    std::cout << std::endl;
    if (!gt_path.empty() && read_pose_file(gt_path, g)) {
        PoseCandidate gt(g, 0.0f, -1.0f), a(refined[0], 0.0f, -1.0f);
        std::vector<PoseCandidate*> both;
        both.push_back(&e); both.push_back(&a);
        const std::vector<stocs_pose_error> q = est.pose_errors(both, std::vector<PoseCandidate*>(1, &gt));
        if (q.size() != 2) { std::cerr << "pose errors failed: " << stocs_last_error() << std::endl; return 2; }
        for (int k = 0; k < 2; ++k) {
            snprintf(b, sizeof(b), "refine-visible %s %s: add=%.9g add_max=%.9g adds=%.9g adds_max=%.9g valid=%d", object.c_str(), k ? "after" : "before", (double)q[(size_t)k].add,
                     (double)q[(size_t)k].add_max, (double)q[(size_t)k].adds, (double)q[(size_t)k].adds_max, q[(size_t)k].valid);
            std::cout << b << std::endl;
        }
    }
    return 0;
}

static int report_gt(stocs::stocs_estimator& est, const std::string& gt_path, const std::string& out_path, const std::string& object,
                     const std::vector<stocs::stocs_estimator::TrialResult>& trials, const std::vector<float>& syms, const stocs_camera* cam,
                     const VsdOptions& vsd) {
    MatrixType g, p;
    if (!read_pose_file(gt_path, g)) { std::cerr << "cannot read a 3x4 pose from " << gt_path << std::endl; return 1; }
    PoseCandidate gt(g, 0.0f, -1.0f);
    const std::vector<PoseCandidate*> gts(1, &gt);
    const float diameter = est.model_diameter();
    if (diameter < 0.0f) { std::cerr << "model diameter failed: " << stocs_last_error() << std::endl; return 2; }
    char b[768];
    stocs_vsd_params vp;
    memset(&vp, 0, sizeof(vp));
    if (vsd.on) {
        vp = est.default_vsd_params();   // BOP's ten taus from the diameter
        if (vsd.delta > 0.0f) vp.delta = vsd.delta;
        if (vsd.surfel_radius > 0.0f) vp.surfel_radius = vsd.surfel_radius;
    }
    if (!read_pose_file(out_path, p)) {
        std::cout << "gt " << object << ": no pose" << std::endl;
    } else {
        PoseCandidate e(p, 0.0f, -1.0f);
        const std::vector<stocs_pose_error> r = est.pose_errors(std::vector<PoseCandidate*>(1, &e), gts);
        if (r.size() != 1) { std::cerr << "pose errors failed: " << stocs_last_error() << std::endl; return 2; }
        snprintf(b, sizeof(b), "gt %s: add=%.9g add_max=%.9g adds=%.9g adds_max=%.9g diameter=%.9g adds_over_diameter=%.9g valid=%d", object.c_str(), (double)r[0].add,
                 (double)r[0].add_max, (double)r[0].adds, (double)r[0].adds_max, (double)diameter, diameter > 0.0f ? (double)(r[0].adds / diameter) : 0.0, r[0].valid);
        std::cout << b << std::endl;
        if (!syms.empty()) {
            const std::vector<stocs_pose_error_sym> q = est.pose_errors_sym(std::vector<PoseCandidate*>(1, &e), gts, syms, cam);
            if (q.size() != 1) { std::cerr << "symmetric pose errors failed: " << stocs_last_error() << std::endl; return 2; }
            int at = snprintf(b, sizeof(b), "gt %s sym: symmetries=%d mssd=%.9g k_mssd=%d add=%.9g k_add=%d", object.c_str(), (int)(syms.size() / 16), (double)q[0].mssd,
                              q[0].k_mssd, (double)q[0].add, q[0].k_add);
            if (cam) at += snprintf(b + at, sizeof(b) - (size_t)at, " mspd=%.9g k_mspd=%d", (double)q[0].mspd, q[0].k_mspd);
            snprintf(b + at, sizeof(b) - (size_t)at, " valid=%d", q[0].valid);
            std::cout << b << std::endl;
        }
        if (vsd.on) {
            const std::vector<PoseCandidate*> es(1, &e);
            const std::vector<stocs_vsd_record> q = vsd.mesh_triangles > 0 ? est.pose_errors_vsd_mesh(es, gts, vp) : est.pose_errors_vsd(es, gts, vp);
            if (q.size() != 1) { std::cerr << "visible-surface discrepancy failed: " << stocs_last_error() << std::endl; return 2; }
            int at = snprintf(b, sizeof(b), "gt %s vsd: taus=%d delta=%.9g", object.c_str(), vp.n_tau, (double)vp.delta);
            if (vsd.mesh_triangles > 0) at += snprintf(b + at, sizeof(b) - (size_t)at, " mesh=%d", vsd.mesh_triangles);
            else at += snprintf(b + at, sizeof(b) - (size_t)at, " surfel_radius=%.9g", (double)vp.surfel_radius);
            at = print_vsd_errors(b, sizeof(b), at, q[0], vp.n_tau);
            double mean = 0.0;
            for (int t = 0; t < vp.n_tau; ++t) mean += (double)q[0].e[t];
            snprintf(b + at, sizeof(b) - (size_t)at, " mean=%.9g px_est=%d px_gt=%d vis_est=%d vis_gt=%d inter=%d uni=%d valid=%d", mean / vp.n_tau, q[0].px_est, q[0].px_gt,
                     q[0].vis_est, q[0].vis_gt, q[0].inter, q[0].uni, q[0].valid);
            std::cout << b << std::endl;
        }
    }
    if (!trials.empty()) {
        std::vector<PoseCandidate> w;
        for (size_t t = 0; t < trials.size(); ++t) w.push_back(PoseCandidate(trials[t].best_pose, trials[t].best_lcp, -1.0f));
        std::vector<PoseCandidate*> wp;
        for (size_t t = 0; t < w.size(); ++t) wp.push_back(&w[t]);
        const std::vector<stocs_pose_error> r = est.pose_errors(wp, gts);
        if (r.size() != wp.size()) { std::cerr << "pose errors failed: " << stocs_last_error() << std::endl; return 2; }
        const float thr = 0.1f * diameter;
        int valid = 0, hit_add = 0, hit_adds = 0;
        for (size_t t = 0; t < r.size(); ++t) {
            if (!r[t].valid) continue;
            ++valid; hit_add += r[t].add < thr; hit_adds += r[t].adds < thr;
        }
        snprintf(b, sizeof(b), "gt %s recall: trials=%d valid=%d threshold=%.9g add=%.9g adds=%.9g", object.c_str(), (int)r.size(), valid, (double)thr,
                 valid ? (double)hit_add / valid : 0.0, valid ? (double)hit_adds / valid : 0.0);
        std::cout << b << std::endl;
        if (!syms.empty()) {
            const std::vector<stocs_pose_error_sym> q = est.pose_errors_sym(wp, gts, syms, cam);
            if (q.size() != wp.size()) { std::cerr << "symmetric pose errors failed: " << stocs_last_error() << std::endl; return 2; }
            int nv = 0, hit_add = 0, hit3 = 0, hit2 = 0;   // hits summed over the ten thresholds of each average recall
            for (size_t t = 0; t < q.size(); ++t) {
                int at = snprintf(b, sizeof(b), "gt %s sym trial %d: mssd=%.9g add=%.9g", object.c_str(), (int)t, (double)q[t].mssd, (double)q[t].add);
                if (cam) at += snprintf(b + at, sizeof(b) - (size_t)at, " mspd=%.9g", (double)q[t].mspd);
                snprintf(b + at, sizeof(b) - (size_t)at, " valid=%d", q[t].valid);
                std::cout << b << std::endl;
                if (!q[t].valid) continue;
                ++nv; hit_add += q[t].add < thr;
                for (int i = 1; i <= 10; ++i) {
                    hit3 += q[t].mssd < (float)(0.05 * i) * diameter;
                    hit2 += q[t].mspd < (float)(5.0 * i) * ((float)image_width / 640.0f);
                }
            }
            int at = snprintf(b, sizeof(b), "gt %s sym recall: trials=%d valid=%d mssd=%.9g add=%.9g", object.c_str(), (int)q.size(), nv, nv ? (double)hit3 / (10.0 * nv) : 0.0,
                              nv ? (double)hit_add / nv : 0.0);
            if (cam) snprintf(b + at, sizeof(b) - (size_t)at, " mspd=%.9g", nv ? (double)hit2 / (10.0 * nv) : 0.0);
            std::cout << b << std::endl;
        }
        if (vsd.on) {
            const std::vector<stocs_vsd_record> q = vsd.mesh_triangles > 0 ? est.pose_errors_vsd_mesh(wp, gts, vp) : est.pose_errors_vsd(wp, gts, vp);
            if (q.size() != wp.size()) { std::cerr << "visible-surface discrepancy failed: " << stocs_last_error() << std::endl; return 2; }
            int nv = 0, hits = 0;   // hits summed over the taus and the ten correctness thresholds
            for (size_t t = 0; t < q.size(); ++t) {
                int at = snprintf(b, sizeof(b), "gt %s vsd trial %d:", object.c_str(), (int)t);
                at = print_vsd_errors(b, sizeof(b), at, q[t], vp.n_tau);
                snprintf(b + at, sizeof(b) - (size_t)at, " valid=%d", q[t].valid);
                std::cout << b << std::endl;
                if (!q[t].valid) continue;   // wrong under every threshold
                ++nv;
                for (int k = 0; k < vp.n_tau; ++k)
                    for (int i = 1; i <= 10; ++i) hits += q[t].e[k] < (float)(0.05 * i);
            }
            snprintf(b, sizeof(b), "gt %s vsd recall: trials=%d valid=%d vsd=%.9g", object.c_str(), (int)q.size(), nv, (double)hits / (10.0 * vp.n_tau * (double)q.size()));
            std::cout << b << std::endl;
        }
    }
    return 0;
}

// a symmetry set as text: 16 floats per transform, column-major; empty when the file holds no whole transform or something else
static std::vector<float> read_sym_file(const std::string& path) {
    std::ifstream f(path);
    std::vector<float> v;
    float x;
    while (f >> x) v.push_back(x);
    if (!f.eof() || v.size() % 16 != 0) v.clear();
    return v;
}

// --track: the prior from the pose file, tracked on this frame; the detection of run_search when the tracked lcp stays below min_lcp
static int run_track(stocs::stocs_estimator& est, const std::string& track_path, float min_lcp, const std::string& out_path, const std::string& dbg_dir,
                     uint64_t seed, int n_trials, int exact_ties, int do_cluster, int n_refine,
                     std::vector<stocs::stocs_estimator::TrialResult>* trial_results = NULL) {
    MatrixType m;
    if (!read_pose_file(track_path, m)) { std::cerr << "cannot read a 3x4 pose from " << track_path << std::endl; return 1; }
    PoseCandidate prior(m, 0.0f, -1.0f);
    if (exact_ties) est.set_exact_ties(true);
    std::vector<PoseCandidate*> priors(1, &prior);
    std::vector<stocs_track_result> res;
    auto t0 = std::chrono::high_resolution_clock::now();
    const std::vector<PoseCandidate*> got = est.track_poses(priors, stocs::stocs_estimator::default_track_params(), &res);
    auto t1 = std::chrono::high_resolution_clock::now();
    if (got.empty()) { std::cerr << "tracking failed: " << stocs_last_error() << std::endl; return 2; }
    const long long us = (long long)std::chrono::duration_cast<micro>(t1 - t0).count();
    char line[256];
    if (got[0]->lcp < min_lcp) {
        snprintf(line, sizeof(line), "track: route=detection prior_lcp=%.9g tracked_lcp=%.9g min_lcp=%.9g track_microseconds=%lld", (double)res[0].prior_lcp,
                 (double)got[0]->lcp, (double)min_lcp, us);
        std::cout << line << std::endl;
        return run_search(est, std::cout, out_path, dbg_dir, seed, n_trials, exact_ties, do_cluster, n_refine, 0, NULL, std::string(), std::string(), trial_results);
    }
    const PoseCandidate* bp = got[0];
    std::ofstream o(out_path, std::ofstream::out);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) o << bp->transform(r, c) << (r == 2 && c == 3 ? "" : " ");
    o << std::endl;
    std::cout << "pose:";
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) { char b[32]; snprintf(b, sizeof(b), " %.9g", (double)bp->transform(r, c)); std::cout << b; }
    std::cout << std::endl;
    snprintf(line, sizeof(line), "track: route=tracked prior_lcp=%.9g best_lcp=%.9g min_lcp=%.9g track_microseconds=%lld", (double)res[0].prior_lcp, (double)bp->lcp,
             (double)min_lcp, us);
    std::cout << line << std::endl;
    return 0;
}

// Several objects of one frame (<object_name> = a,b,c): every model, PPF index and probability map is read before any GPU work (a
// missing one ends the run, naming the object); the frame is ingested once for all of them (stocs::load_frame_scenes); then each
// object is searched on its own context, at most kMaxFrameThreads at a time (every context holds its own trial memory).  Each
// object writes <scene>/best_pose_candidate_<object>.txt and its block of lines, printed in the order given once all are done.
static const int kMaxFrameThreads = 4;

struct SceneSelectOptions { bool on, masks; int max_per_object; };

// --scene-select: the trial winners of every object, judged together; the estimators hold their frames
static int run_scene_select(const std::string& scene_path, const std::vector<std::string>& objects, std::vector<std::unique_ptr<stocs::stocs_estimator> >& ests,
                            const std::vector<std::vector<stocs::stocs_estimator::TrialResult> >& results, const SceneSelectOptions& opt) {
    std::vector<std::vector<std::unique_ptr<PoseCandidate> > > store(objects.size());
    std::vector<std::vector<PoseCandidate*> > poses(objects.size());
    std::vector<stocs::stocs_estimator*> ptrs;
    for (size_t k = 0; k < objects.size(); ++k) {
        ptrs.push_back(ests[k].get());
        for (size_t t = 0; t < results[k].size(); ++t) {
            store[k].emplace_back(new PoseCandidate(results[k][t].best_pose, results[k][t].best_lcp, -1.0f));
            poses[k].push_back(store[k].back().get());
        }
    }
    std::vector<int> caps;
    if (opt.max_per_object > 0) caps.push_back(opt.max_per_object);
    const stocs::SceneSelection sel = stocs::select_scene(ptrs, poses, caps, opt.masks);
    if (!sel.ok) { std::cerr << "scene selection failed: " << stocs_last_error() << std::endl; return 2; }
    std::vector<int> order(sel.selected);
    for (size_t h = 0; h < sel.records.size(); ++h) if (sel.records[h].rank < 0) order.push_back((int)h);
    std::ofstream o(scene_path + "/scene_selection.txt", std::ofstream::out);
    for (size_t i = 0; i < order.size(); ++i) {
        const size_t h = (size_t)order[i];
        const stocs_scene_result& r = sel.records[h];
        char b[256];
        snprintf(b, sizeof(b), "scene %d: object %s trial %d score %.9g own %d exclusive %d reason %d", r.rank, objects[(size_t)sel.group[h]].c_str(), sel.index[h],
                 (double)sel.score[h], r.own, r.exclusive, r.reason);
        std::cout << b << std::endl;
        o << r.rank << " " << objects[(size_t)sel.group[h]] << " " << sel.index[h];
        const PoseCandidate* pc = poses[(size_t)sel.group[h]][(size_t)sel.index[h]];
        for (int rr = 0; rr < 3; ++rr) for (int c = 0; c < 4; ++c) { snprintf(b, sizeof(b), " %.9g", (double)pc->transform(rr, c)); o << b; }
        o << std::endl;
    }
    std::cout << "scene: hypotheses=" << sel.records.size() << " selected=" << sel.selected.size() << std::endl;
    if (opt.masks) {
        std::vector<unsigned char> px(sel.labels.size() * 2);
        for (size_t i = 0; i < sel.labels.size(); ++i) { const unsigned v = (unsigned)(sel.labels[i] + 1); px[2 * i] = (unsigned char)(v >> 8); px[2 * i + 1] = (unsigned char)(v & 255u); }
        std::ofstream pg(scene_path + "/labels_scene.pgm", std::ofstream::out | std::ofstream::binary);
        pg << "P5\n" << image_width << " " << image_height << "\n65535\n";
        pg.write((const char*)px.data(), (std::streamsize)px.size());
    }
    return 0;
}

// --segment with several objects (or --segment-gate): the class images come from the depth image and the size gate, not from probability_maps
struct SegmentAssignOptions {
    bool on, convex;
    stocs_segment_params prm;
    stocs_segment_convex_params cvx;
    stocs_segment_gate_params gate;
};
static void print_segment_lines(std::ostream& os, const stocs::SegmentedFrame& seg, bool convex, const stocs_segment_convex_params& cvx) {
    const stocs_segment_result& sr = seg.result;
    if (convex)
        os << "segment convex: radius " << cvx.bend_radius << ", smoothing " << cvx.smooth_radius << ", cos " << cvx.bend_cos << ": " << seg.convex.n_tested_h
           << " + " << seg.convex.n_tested_v << " triples tested, " << seg.convex.n_cut_h << " + " << seg.convex.n_cut_v << " cut, " << seg.convex.n_cut
           << " pixels cut" << std::endl;
    os << "segment: plane " << (sr.plane_found ? "found" : "not found") << " (" << sr.plane[0] << " " << sr.plane[1] << " " << sr.plane[2] << " " << sr.plane[3]
       << "), " << sr.n_on_plane << " pixels on it, " << sr.n_components << " components, " << sr.n_segments << " segments kept" << std::endl;
}

static int run_frame_objects(const std::string& scene_path, const std::vector<std::string>& objects, uint64_t seed, int n_trials, int exact_ties,
                             const SceneSelectOptions& scene_opt, const SegmentAssignOptions& seg_opt) {
    const size_t n = objects.size();
    std::vector<stocs::ModelCloud> models(n);
    std::vector<PPFMapType> maps(n);
    std::vector<std::string> prob_paths(n);
    std::cout << "############# LOADING OBJECT MAPS ################" << std::endl;
    for (size_t k = 0; k < n; ++k) {
        const std::string& obj = objects[k];
        const std::string model_path = repo_path + "/models/" + obj + "/model_search.ply", map_path = repo_path + "/models/" + obj + "/ppf_map";
        prob_paths[k] = scene_path + "/probability_maps/" + obj + ".png";
        if (!seg_opt.on && !stocs::file_exists(prob_paths[k])) { std::cerr << "object " << obj << ": no class probability map " << prob_paths[k] << std::endl; return 1; }
        if (!stocs::file_exists(model_path)) { std::cerr << "object " << obj << ": no model " << model_path << std::endl; return 1; }
        rgbd::load_ppf_map(map_path, maps[k]);
        if (maps[k].location.empty()) { std::cerr << "object " << obj << ": no readable ppf_map " << map_path << std::endl; return 1; }
        try {
            stocs::read_ply(model_path, &models[k], true);
        } catch (const std::exception& e) {
            std::cerr << "object " << obj << ": " << e.what() << std::endl;
            return 1;
        }
        std::cout << "object " << obj << ": |M| = " << models[k].size() << ",  |map(M)| = " << maps[k].size() << std::endl;
    }
    std::cout << "############# LOADING OBJECT COMPLETE ################" << std::endl;
    std::vector<stocs::SceneCloud> scenes;
    std::vector<uint16_t> seg_depth, seg_stack;   // --segment: the frame and the gate's class stack (object-major), kept for --scene-select
    try {
        if (seg_opt.on) {
            stocs::read_image(scene_path + "/depth.png", 1, 16, image_width, image_height, &seg_depth);
            const stocs::SegmentedFrame seg = seg_opt.convex ? stocs::segment_frame(seg_depth.data(), cam_intrinsics, image_width, image_height, depth_scale, seg_opt.prm, seg_opt.cvx)
                                                             : stocs::segment_frame(seg_depth.data(), cam_intrinsics, image_width, image_height, depth_scale, seg_opt.prm);
            print_segment_lines(std::cout, seg, seg_opt.convex, seg_opt.cvx);
            std::vector<stocs_object_size> sizes(n);
            for (size_t k = 0; k < n; ++k) sizes[k] = stocs::object_size(models[k].pos);
            stocs::SegmentAssignment as = stocs::segment_assign(seg_depth.data(), seg.labels.data(), seg.result.n_segments, sizes, cam_intrinsics, image_width, image_height,
                                                                depth_scale, seg_opt.prm.max_depth, seg_opt.gate);
            for (size_t k = 0; k < n; ++k)
                std::cout << "segment assign: " << objects[k] << ": " << as.compatible((int)k) << " of " << as.n_labels << " segments" << std::endl;
            seg_stack.swap(as.class_stack);
            scenes = stocs::load_frame_scenes(seg_depth.data(), seg_stack.data(), std::vector<float>(n, class_threshold), NULL, cam_intrinsics, image_width, image_height,
                                              depth_scale, voxel_size);
        } else
        scenes = stocs::load_frame_scenes(scene_path + "/depth.png", prob_paths, std::vector<float>(n, class_threshold), scene_path + "/probability_maps/edge.png",
                                          cam_intrinsics, image_width, image_height, depth_scale, voxel_size);
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;   // no GPU => loud failure, never a CPU fallback
        return 2;
    }
    std::vector<std::ostringstream> blocks(n);
    std::vector<int> rcs(n, 0);
    std::atomic<size_t> next(0);
    // --scene-select: the contexts stay alive until all objects are done, each with the frame (the depth image and its own class image)
    std::vector<std::unique_ptr<stocs::stocs_estimator> > kept(n);
    std::vector<std::vector<stocs::stocs_estimator::TrialResult> > trial_results(n);
    std::vector<uint16_t> frame_depth;
    if (scene_opt.on) {
        try {
            stocs::read_image(scene_path + "/depth.png", 1, 16, image_width, image_height, &frame_depth);
        } catch (const std::exception& e) {
            std::cerr << e.what() << std::endl;
            return 1;
        }
    }
    auto worker = [&]() {
        for (size_t k; (k = next.fetch_add(1)) < n;) {
            std::ostringstream& os = blocks[k];
            os << "############# RUNNING STOCS for Scene: " << scene_path << ", Object: " << objects[k] << " ##############" << std::endl;
            try {
                std::unique_ptr<stocs::stocs_estimator> est(new stocs::stocs_estimator(models[k], maps[k], scenes[k], std::string(), image_width, image_height,
                                                                                       distance_threshold, ppf_tr_discretization, ppf_rot_discretization, edge_threshold,
                                                                                       class_threshold, -1, &os));
                rcs[k] = run_search(*est, os, scene_path + "/best_pose_candidate_" + objects[k] + ".txt", std::string(), seed, n_trials, exact_ties, 0, 0, 0, NULL, std::string(),
                                    std::string(), scene_opt.on ? &trial_results[k] : NULL);
                if (scene_opt.on) {
                    std::vector<uint16_t> prob;
                    if (seg_opt.on) prob.assign(seg_stack.begin() + (std::ptrdiff_t)(k * (size_t)image_width * image_height), seg_stack.begin() + (std::ptrdiff_t)((k + 1) * (size_t)image_width * image_height));
                    else stocs::read_image(prob_paths[k], 1, 16, image_width, image_height, &prob);
                    est->set_frame(frame_depth.data(), prob.data(), cam_intrinsics, depth_scale);
                    kept[k] = std::move(est);
                }
            } catch (const std::exception& e) {
                os << "object " << objects[k] << " failed: " << e.what() << std::endl;
                rcs[k] = 2;
            }
        }
    };
    std::vector<std::thread> pool;
    for (size_t t = 0; t < std::min<size_t>(n, kMaxFrameThreads); ++t) pool.emplace_back(worker);
    for (size_t t = 0; t < pool.size(); ++t) pool[t].join();
    int rc = 0;
    for (size_t k = 0; k < n; ++k) {
        std::cout << blocks[k].str();
        if (rcs[k] != 0 && rc == 0) rc = rcs[k];
    }
    std::cout << std::flush;
    if (scene_opt.on && rc == 0) rc = run_scene_select(scene_path, objects, kept, trial_results, scene_opt);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::cout << "Enter scene path and object name as arguments!" << std::endl;   // :190
        return -1;
    }
    const bool clouds = std::string(argv[1]) == "--clouds";
    if (clouds && argc < 4) { std::cout << "usage: stocs_single --clouds <scene.stcl> <model.stcl> [options]" << std::endl; return -1; }
    const std::string a1 = argv[clouds ? 2 : 1], a2 = argv[clouds ? 3 : 2];
    if (const char* e = getenv("STOCS_REPO_PATH")) repo_path = e;
    std::string edge_path, out_path, dbg_dir, track_path, gt_path, sym_path;
    float sym3[3] = {0.0f, 0.0f, 0.0f};
    int sym_steps = 72;
    bool have_sym = false;
    float track_min_lcp = 0.02f;
    int do_cluster = 0, n_trials = 0, exact_ties = 0, n_refine = 0, depth_check = 0;
    bool do_instances = false, do_masks = false, have_trim = false, have_gate = false;
    SceneSelectOptions scene_opt = {false, false, 0};
    VsdOptions vsd_opt = {false, 0.0f, 0.0f, 0};
    RefineVisibleOptions rv_opt = {false, 0, -1.0f, -1.0f, 0, false, -1.0f, -1.0f, -1.0f, {0.0f, 0.0f, 0.0f}, false, -1.0f, -1, -1.0f};
    bool damped_bad = false, contour_bad = false;
    bool do_segment = false, segment_edges = false, segment_bad = false;   // --segment [tol[,min_pixels]] [--segment-edges]
    stocs_segment_params seg_prm = stocs::default_segment_params();
    bool segment_convex = false;                                            // --segment-convex [r[,s[,deg]]]
    stocs_segment_convex_params seg_cvx = stocs::default_segment_convex_params();
    bool segment_gate = false, segment_gate_bad = false;                    // --segment-gate slack[,min_ratio]
    stocs_segment_gate_params seg_gate = stocs::default_segment_gate_params();
    std::string mesh_path, surface = "points";
    bool have_vsd_delta = false, have_surfel_radius = false;
    stocs_instance_params inst_prm = stocs::stocs_estimator::default_instance_params();
    uint64_t seed = 1;
    for (int i = clouds ? 4 : 3; i < argc; i += 2) {
        if (std::string(argv[i]) == "--depth-check") { depth_check = 1; --i; continue; }   // the options without a value
        if (std::string(argv[i]) == "--masks") { do_masks = true; --i; continue; }
        if (std::string(argv[i]) == "--scene-select") { scene_opt.on = true; --i; continue; }
        if (std::string(argv[i]) == "--segment-edges") { segment_edges = true; --i; continue; }
        if (std::string(argv[i]) == "--segment") {   // [tol[,min_pixels]]: the class image from the depth image; the value may be left out
            do_segment = true;
            if (i + 1 >= argc || std::string(argv[i + 1]).compare(0, 2, "--") == 0) { --i; continue; }
            const std::string sv = argv[i + 1];
            char tail = 0;
            const int got = sscanf(sv.c_str(), "%f,%d%c", &seg_prm.plane_tolerance, &seg_prm.min_pixels, &tail);
            if (got < 1 || got > 2 || (size_t)std::count(sv.begin(), sv.end(), ',') + 1 != (size_t)got || stocs_check_segment_params(&seg_prm) != STOCS_OK) segment_bad = true;
            continue;
        }
        if (std::string(argv[i]) == "--segment-convex") {   // [r[,s[,deg]]]: the concavity cut in front of the labelling; the value may be left out
            segment_convex = true;
            if (i + 1 >= argc || std::string(argv[i + 1]).compare(0, 2, "--") == 0) { --i; continue; }
            const std::string sv = argv[i + 1];
            char tail = 0;
            float deg = 25.0f;
            const int got = sscanf(sv.c_str(), "%d,%d,%f%c", &seg_cvx.bend_radius, &seg_cvx.smooth_radius, &deg, &tail);
            if (got < 1 || got > 3 || (size_t)std::count(sv.begin(), sv.end(), ',') + 1 != (size_t)got || !(deg >= 0.0f && deg <= 90.0f)) segment_bad = true;
            if (got == 3) seg_cvx.bend_cos = std::min(1.0f, std::max(0.0f, (float)std::cos((double)deg * 3.14159265358979323846 / 180.0)));   // degrees become bend_cos here
            if (stocs_check_segment_convex_params(&seg_cvx) != STOCS_OK) segment_bad = true;
            continue;
        }
        if (std::string(argv[i]) == "--segment-gate") {   // slack[,min_ratio]: the size gate between segments and objects
            segment_gate = true;
            const std::string sv = i + 1 < argc ? argv[i + 1] : "";
            char tail = 0;
            const int got = sscanf(sv.c_str(), "%f,%f%c", &seg_gate.slack, &seg_gate.min_ratio, &tail);
            if (got < 1 || got > 2 || (size_t)std::count(sv.begin(), sv.end(), ',') + 1 != (size_t)got || stocs_check_segment_gate_params(&seg_gate) != STOCS_OK) segment_gate_bad = true;
            continue;
        }
        if (std::string(argv[i]) == "--vsd") { vsd_opt.on = true; --i; continue; }   // with --gt: the visible-surface discrepancy too
        if (std::string(argv[i]) == "--damped") {   // [lambda0[,rot_deg[,trans_m]]]: the value may be left out
            rv_opt.damped = true;
            if (i + 1 >= argc || std::string(argv[i + 1]).compare(0, 2, "--") == 0) { --i; continue; }
            const std::string dv = argv[i + 1];
            char tail = 0;
            const int got = sscanf(dv.c_str(), "%f,%f,%f%c", &rv_opt.lambda0, &rv_opt.rot_deg, &rv_opt.trans_m, &tail);
            if (got < 1 || got > 3 || (size_t)std::count(dv.begin(), dv.end(), ',') + 1 != (size_t)got) damped_bad = true;
            if (!(rv_opt.lambda0 >= 0.0f) || (got >= 2 && !(rv_opt.rot_deg > 0.0f)) || (got == 3 && !(rv_opt.trans_m > 0.0f))) damped_bad = true;
            continue;
        }
        if (std::string(argv[i]) == "--contour") {   // [w[,radius_px[,dist_m]]]: the value may be left out
            rv_opt.contour = true;
            if (i + 1 >= argc || std::string(argv[i + 1]).compare(0, 2, "--") == 0) { --i; continue; }
            const std::string cv = argv[i + 1];
            char tail = 0;
            const int got = sscanf(cv.c_str(), "%f,%d,%f%c", &rv_opt.weight, &rv_opt.radius_px, &rv_opt.pull_m, &tail);
            if (got < 1 || got > 3 || (size_t)std::count(cv.begin(), cv.end(), ',') + 1 != (size_t)got) contour_bad = true;
            if (!(rv_opt.weight >= 0.0f) || (got >= 2 && rv_opt.radius_px < 1) || (got == 3 && !(rv_opt.pull_m > 0.0f))) contour_bad = true;
            continue;
        }
        if (i + 1 >= argc) break;
        const std::string k = argv[i], v = argv[i + 1];
        if (k == "--edge") edge_path = v;
        else if (k == "--seed") seed = strtoull(v.c_str(), NULL, 10);
        else if (k == "--out") out_path = v;
        else if (k == "--bases") number_of_bases = atoi(v.c_str());
        else if (k == "--max-sets") maximum_congruent_sets = atoi(v.c_str());
        else if (k == "--dbg") dbg_dir = v;
        else if (k == "--cluster") do_cluster = atoi(v.c_str());
        else if (k == "--refine") n_refine = atoi(v.c_str());   // iterations of the refinement of the clustered hypotheses (0: off)
        else if (k == "--trim") { g_trim = (float)atof(v.c_str()); have_trim = true; }   // robust refinement: share of the pairs kept per iteration
        else if (k == "--normal-gate") { g_gate_deg = (float)atof(v.c_str()); have_gate = true; }   // and the largest angle between a pair's normals
        else if (k == "--robust") {   // the robust refinement inside a trial batch or behind --track: keep[,deg]
            char tail = 0;
            const int got = sscanf(v.c_str(), "%f,%f%c", &g_robust_keep, &g_robust_deg, &tail);
            g_robust = true;
            if (got == 1 && v.find(',') == std::string::npos) g_robust_deg = -1.0f;
            else if (got != 2) g_robust_keep = -1.0f;   // not keep[,deg]: refused below
            else if (!(g_robust_deg >= 0.0f && g_robust_deg <= 180.0f)) g_robust_keep = -1.0f;
        }
        else if (k == "--trials") n_trials = atoi(v.c_str());   // N independent runs (seeds seed, seed + 1, ...) in one set of GPU launches; the best one is written
        else if (k == "--exact-ties") exact_ties = atoi(v.c_str());   // 1: the reference kd-tree's answer on exact distance ties (set_exact_ties)
        else if (k == "--track") track_path = v;   // track from this pose file; detection when the tracked lcp is below --track-min-lcp
        else if (k == "--track-min-lcp") track_min_lcp = (float)atof(v.c_str());
        else if (k == "--gt") gt_path = v;   // ground-truth pose file (the format of --track): ADD / ADD-S of the pose this run writes
        else if (k == "--sym") {   // with --gt: the errors under the symmetries this clustering descriptor stands for
            if (sscanf(v.c_str(), "%f,%f,%f", &sym3[0], &sym3[1], &sym3[2]) != 3) { std::cerr << "--sym a,b,c" << std::endl; return -1; }
            have_sym = true;
        } else if (k == "--sym-steps") sym_steps = atoi(v.c_str());
        else if (k == "--sym-file") sym_path = v;
        else if (k == "--vsd-delta") { vsd_opt.delta = (float)atof(v.c_str()); have_vsd_delta = true; }
        else if (k == "--surfel-radius") { vsd_opt.surfel_radius = (float)atof(v.c_str()); have_surfel_radius = true; }
        else if (k == "--surface") surface = v;   // points | mesh: what --masks renders
        else if (k == "--refine-visible") {   // K[,dist[,cos]]: the written pose refined on the mesh against the frame (needs --mesh)
            char tail = 0;
            const int got = sscanf(v.c_str(), "%d,%f,%f%c", &rv_opt.iterations, &rv_opt.distance, &rv_opt.view_cos, &tail);
            const size_t commas = (size_t)std::count(v.begin(), v.end(), ',');
            rv_opt.on = true;
            if (got < 1 || got > 3 || commas + 1 != (size_t)got) rv_opt.iterations = -1;   // not K[,dist[,cos]]: refused below
            if ((got >= 2 && !(rv_opt.distance > 0.0f)) || (got == 3 && !(rv_opt.view_cos >= 0.0f))) rv_opt.iterations = -1;   // (a value below 0 means "not given")
        }
        else if (k == "--mesh") mesh_path = v;   // with --vsd: the model as a triangle mesh, rasterised in place of the surfels
        else if (k == "--instances") { do_instances = true; inst_prm.max_instances = atoi(v.c_str()); }
        else if (k == "--instance-min-fraction") inst_prm.min_exclusive_fraction = (float)atof(v.c_str());
        else if (k == "--instance-min-points") inst_prm.min_points = atoi(v.c_str());
        else if (k == "--scene-max-per-object") scene_opt.max_per_object = atoi(v.c_str());
        else if (k == "--repo") repo_path = v;
        else if (k == "--voxel") voxel_size = (float)atof(v.c_str());
        else if (k == "--depth-scale") depth_scale = (float)atof(v.c_str());
        else if (k == "--class-threshold") class_threshold = (float)atof(v.c_str());
        else if (k == "--intrinsics") {
            if (sscanf(v.c_str(), "%f,%f,%f,%f", &cam_intrinsics[0], &cam_intrinsics[1], &cam_intrinsics[2], &cam_intrinsics[3]) != 4) { std::cerr << "--intrinsics fx,cx,fy,cy" << std::endl; return -1; }
        } else { std::cerr << "unknown option " << k << std::endl; return -1; }
    }

    if (!gt_path.empty()) {   // before any search: a ground truth that cannot be read ends the run here
        MatrixType g;
        if (!read_pose_file(gt_path, g)) { std::cerr << "cannot read a 3x4 pose from " << gt_path << std::endl; return 1; }
    }

    std::vector<float> syms;   // --sym: the set the report is taken under, settled before any search
    if (have_sym || !sym_path.empty()) {
        if (!have_sym || gt_path.empty()) { std::cerr << "--sym a,b,c [--sym-steps n] [--sym-file f] needs --gt" << std::endl; return -1; }
        syms = sym_path.empty() ? stocs::symmetry_set(sym3, sym_steps) : read_sym_file(sym_path);
        if (syms.empty() || syms.size() / 16 > (size_t)STOCS_POSE_SYM_MAX) {
            std::cerr << "no symmetry set of 1 .. " << STOCS_POSE_SYM_MAX << " transforms from " << (sym_path.empty() ? std::string("--sym / --sym-steps") : sym_path) << std::endl;
            return 1;
        }
    }

    const bool segment_assign = do_segment && !clouds && (segment_gate || a2.find(',') != std::string::npos);   // the multi-object path of --segment
    if (segment_gate && (!do_segment || segment_gate_bad || clouds)) {   // refused before any search
        std::cerr << "--segment-gate slack[,min_ratio] needs --segment, a scene directory, slack >= 0 and min_ratio in [0, 1]" << std::endl;
        return -1;
    }
    if (segment_bad || ((segment_edges || segment_convex) && !do_segment) || (do_segment && clouds) || (segment_assign && segment_edges)) {   // refused before any search
        std::cerr << "--segment [tol[,min_pixels]] needs a scene directory, tol > 0 and min_pixels >= 1; --segment-edges needs --segment and a single object without --segment-gate; "
                     "--segment-convex [r[,s[,deg]]] needs --segment, r in 0..8, s in 0..4 and 0 <= deg <= 90" << std::endl;
        return -1;
    }
    std::vector<float> mesh_v;
    std::vector<int32_t> mesh_t;
    if (surface != "points" && surface != "mesh") { std::cerr << "--surface takes points or mesh" << std::endl; return -1; }
    const bool surface_mesh = surface == "mesh";
    if (surface_mesh && (mesh_path.empty() || !do_masks || !do_instances || clouds || a2.find(',') != std::string::npos)) {   // refused before any search
        std::cerr << "--surface mesh needs --mesh <ply>, --masks with --instances M, a scene directory and a single object" << std::endl;
        return -1;
    }
    if (!mesh_path.empty()) {   // refused before any search
        if ((!vsd_opt.on && !surface_mesh && !rv_opt.on) || have_surfel_radius) { std::cerr << "--mesh <ply> needs --vsd and takes no --surfel-radius" << std::endl; return -1; }
        int nv = 0, nt = 0;
        if (stocs_ply_read_mesh(mesh_path.c_str(), NULL, 0, &nv, NULL, 0, &nt) != STOCS_OK) { std::cerr << "cannot read a mesh from " << mesh_path << ": " << stocs_last_error() << std::endl; return 1; }
        if (nt < 1) { std::cerr << mesh_path << " has no faces" << std::endl; return 1; }
        mesh_v.resize((size_t)nv * 3); mesh_t.resize((size_t)nt * 3);
        if (stocs_ply_read_mesh(mesh_path.c_str(), mesh_v.data(), nv, &nv, mesh_t.data(), nt, &nt) != STOCS_OK || stocs_mesh_check(mesh_v.data(), nv, mesh_t.data(), nt) != STOCS_OK) {
            std::cerr << "cannot read a mesh from " << mesh_path << ": " << stocs_last_error() << std::endl;
            return 1;
        }
        if (vsd_opt.on) vsd_opt.mesh_triangles = nt;
        if (surface_mesh) g_mask_mesh_triangles = nt;
        if (rv_opt.on) rv_opt.mesh_triangles = nt;
        double mean[3] = {0.0, 0.0, 0.0};   // --damped turns about the mean of the vertices
        for (int i = 0; i < nv; ++i) for (int k = 0; k < 3; ++k) mean[k] += (double)mesh_v[(size_t)i * 3 + (size_t)k];
        for (int k = 0; k < 3; ++k) rv_opt.pivot[k] = (float)(mean[k] / (double)nv);
    }
    if (rv_opt.damped) {   // refused before any search
        const stocs_refine_visible_damped_params dp = damped_params_of(rv_opt);
        if (!rv_opt.on || damped_bad || (rv_opt.iterations >= 0 && !mesh_path.empty() && stocs_check_refine_visible_damped_params(&dp) != STOCS_OK)) {
            std::cerr << "--damped [lambda0[,rot_deg[,trans_m]]] needs --refine-visible, lambda0 >= 0, rot_deg > 0 and trans_m > 0" << std::endl;
            return -1;
        }
    }
    if (rv_opt.contour) {   // refused before any search
        const stocs_refine_visible_contour_params cp = contour_params_of(rv_opt);
        if (!rv_opt.on || !rv_opt.damped) {
            std::cerr << "--contour [w[,radius_px[,dist_m]]] needs " << (!rv_opt.on ? "--refine-visible" : "--damped") << std::endl;
            return -1;
        }
        if (contour_bad || (rv_opt.iterations >= 0 && !mesh_path.empty() && !damped_bad && stocs_check_refine_visible_contour_params(&cp) != STOCS_OK)) {
            std::cerr << "--contour [w[,radius_px[,dist_m]]] needs w >= 0, radius_px in 1 .. 64 and dist_m > 0" << std::endl;
            return -1;
        }
    }
    if (rv_opt.on) {   // refused before any search
        stocs_refine_visible_params rp = stocs::stocs_estimator::default_refine_visible_params();
        rp.max_iterations = rv_opt.iterations;
        if (rv_opt.distance >= 0.0f) rp.max_distance = rv_opt.distance;
        if (rv_opt.view_cos >= 0.0f) rp.min_view_cos = rv_opt.view_cos;
        if (mesh_path.empty() || clouds || a2.find(',') != std::string::npos || stocs_check_refine_visible_params(&rp) != STOCS_OK || !(rv_opt.distance == rv_opt.distance) ||
            !(rv_opt.view_cos == rv_opt.view_cos)) {
            std::cerr << "--refine-visible K[,dist[,cos]] needs --mesh <ply>, a scene directory, a single object, K >= 0, dist > 0 and 0 <= cos < 1" << std::endl;
            return -1;
        }
    }
    if (vsd_opt.on || have_vsd_delta || have_surfel_radius) {   // refused before any search
        if (!vsd_opt.on || gt_path.empty() || clouds || a2.find(',') != std::string::npos) {
            std::cerr << "--vsd [--vsd-delta m] [--surfel-radius m] needs --gt, a scene directory and a single object" << std::endl;
            return -1;
        }
        if ((have_vsd_delta && !(vsd_opt.delta > 0.0f && std::isfinite(vsd_opt.delta))) ||
            (have_surfel_radius && !(vsd_opt.surfel_radius > 0.0f && std::isfinite(vsd_opt.surfel_radius)))) {
            std::cerr << "--vsd-delta and --surfel-radius need positive, finite metres" << std::endl;
            return -1;
        }
    }

    if (n_refine < 0 || (n_refine > 0 && !do_cluster)) { std::cerr << "--refine N needs N >= 0 and --cluster 1" << std::endl; return -1; }
    if ((have_trim || have_gate) && (!have_trim || !(g_trim > 0.0f && g_trim <= 1.0f) || (have_gate && !(g_gate_deg >= 0.0f && g_gate_deg <= 180.0f)) || n_refine <= 0 ||
                                     n_trials > 0 || !track_path.empty())) {
        std::cerr << "--trim r [--normal-gate deg] needs r in (0, 1], deg in [0, 180], --cluster 1 --refine N, and neither --trials nor --track" << std::endl;
        return -1;
    }

    if (g_robust) {
        if (!(g_robust_keep > 0.0f && g_robust_keep <= 1.0f)) { std::cerr << "--robust keep[,deg] needs keep in (0, 1] and deg in [0, 180]" << std::endl; return -1; }
        if (n_refine <= 0 || !do_cluster || (n_trials <= 0 && track_path.empty())) {
            std::cerr << "--robust keep[,deg] has nothing to refine: it needs --cluster 1 --refine K with --trials N or --track <file>" << std::endl;
            return -1;
        }
        if (n_trials <= 0) { g_trim = g_robust_keep; g_gate_deg = g_robust_deg; }   // --track without --trials: the single run's refinement
    }

    if (depth_check && (clouds || n_trials <= 0 || !do_cluster || !track_path.empty() || a2.find(',') != std::string::npos)) {
        std::cerr << "--depth-check needs a scene directory, a single object, --trials N and --cluster 1" << std::endl;
        return -1;
    }

    if (do_instances && (n_trials <= 0 || !do_cluster || !track_path.empty() || (!clouds && a2.find(',') != std::string::npos))) {
        std::cerr << "--instances needs a single object, --trials N and --cluster 1" << std::endl;
        return -1;
    }

    if ((scene_opt.on || scene_opt.max_per_object != 0) && (!scene_opt.on || clouds || a2.find(',') == std::string::npos || n_trials <= 0 || scene_opt.max_per_object < 0)) {
        std::cerr << "--scene-select needs several objects and --trials N (--scene-max-per-object K >= 1 goes with it)" << std::endl;
        return -1;
    }
    scene_opt.masks = scene_opt.on && do_masks;

    if (do_masks && !scene_opt.on && (clouds || !do_instances)) {
        std::cerr << "--masks needs a scene directory and --instances M" << std::endl;
        return -1;
    }

    if (!clouds && (a2.find(',') != std::string::npos || segment_assign)) {
        std::vector<std::string> objects;
        std::stringstream names(a2);
        for (std::string o; std::getline(names, o, ',');) objects.push_back(o);
        if (a2.back() == ',') objects.push_back(std::string());
        for (size_t k = 0; k < objects.size(); ++k) {
            if (objects[k].empty() || std::count(objects.begin(), objects.end(), objects[k]) > 1) { std::cerr << "object list " << a2 << ": empty or repeated name" << std::endl; return -1; }
        }
        if (do_cluster || n_refine || !out_path.empty() || !dbg_dir.empty() || !edge_path.empty() || !track_path.empty() || !gt_path.empty()) {
            std::cerr << (objects.size() > 1 ? "several objects" : "--segment-gate (the path of several objects, also with one)")
                      << ": --cluster, --refine, --out, --dbg, --edge, --track and --gt take a single object" << (objects.size() > 1 ? "" : " without --segment-gate") << std::endl;
            return -1;
        }
        const SegmentAssignOptions seg_opt = {segment_assign, segment_convex, seg_prm, seg_cvx, seg_gate};
        return run_frame_objects(a1, objects, seed, n_trials, exact_ties, scene_opt, seg_opt);
    }

    std::unique_ptr<stocs::stocs_estimator> est;
    try {
        if (clouds) {
            stocs::SceneCloud scene;
            stocs::ModelCloud model;
            if (!read_stcl(a1, scene.pos, scene.nrm, &scene.class_probability, &scene.pixel)) { std::cerr << "cannot read scene " << a1 << std::endl; return 1; }
            if (!read_stcl(a2, model.pos, model.nrm, NULL, NULL)) { std::cerr << "cannot read model " << a2 << std::endl; return 1; }
            if (!edge_path.empty()) {
                std::ifstream ef(edge_path, std::ios::binary);
                scene.edge_map.resize((size_t)image_width * image_height);
                if (!ef.read((char*)scene.edge_map.data(), (std::streamsize)scene.edge_map.size())) { std::cerr << "cannot read edge map" << std::endl; return 1; }
            }
            if (out_path.empty()) out_path = "best_pose_candidate.txt";
            std::cout << "|M| = " << model.size() << std::endl;
            est.reset(new stocs::stocs_estimator(model, scene, dbg_dir, image_width, image_height, distance_threshold, ppf_tr_discretization, ppf_rot_discretization,
                                                 edge_threshold, class_threshold));
        } else {
            // :56-62, :196-208
            const std::string scene_path = a1, object_name = a2;
            const std::string rgb_path = scene_path + "/rgb.png", depth_path = scene_path + "/depth.png";
            const std::string class_probability_path = scene_path + "/probability_maps/" + object_name + ".png";
            const std::string edge_probability_path = scene_path + "/probability_maps/edge.png";
            const std::string model_path = repo_path + "/models/" + object_name + "/model_search.ply";
            if (out_path.empty()) out_path = scene_path + "/best_pose_candidate_" + object_name + ".txt";
            const bool own_dbg = dbg_dir.empty();
            if (own_dbg) dbg_dir = scene_path + "/dbg";
            std::cout << "############# LOADING OBJECT MAPS ################" << std::endl;
            PPFMapType model_map;
            rgbd::load_ppf_map(repo_path + "/models/" + object_name + "/ppf_map", model_map);
            std::cout << "############# LOADING OBJECT COMPLETE ################" << std::endl;
            // :207-208 (only the reference's own <scene>/dbg is wiped; a directory named with --dbg is merely created)
            if (system(((own_dbg ? "rm -rf '" + dbg_dir + "' && " : std::string()) + "mkdir -p '" + dbg_dir + "'").c_str()) != 0) std::cerr << "cannot create " << dbg_dir << std::endl;
            std::cout << "############# RUNNING STOCS for Scene: " << scene_path << ", Object: " << object_name << " ##############" << std::endl;
            if (do_segment) {   // no probability_maps: the class image (and with --segment-edges the edge image) comes from the depth image
                std::vector<uint16_t> depth;
                stocs::read_image(depth_path, 1, 16, image_width, image_height, &depth);
                const stocs::SegmentedFrame seg = segment_convex ? stocs::segment_frame(depth.data(), cam_intrinsics, image_width, image_height, depth_scale, seg_prm, seg_cvx)
                                                                 : stocs::segment_frame(depth.data(), cam_intrinsics, image_width, image_height, depth_scale, seg_prm);
                const stocs_segment_result& sr = seg.result;
                if (segment_convex)
                    std::cout << "segment convex: radius " << seg_cvx.bend_radius << ", smoothing " << seg_cvx.smooth_radius << ", cos " << seg_cvx.bend_cos << ": " << seg.convex.n_tested_h
                              << " + " << seg.convex.n_tested_v << " triples tested, " << seg.convex.n_cut_h << " + " << seg.convex.n_cut_v << " cut, " << seg.convex.n_cut
                              << " pixels cut" << std::endl;
                std::cout << "segment: plane " << (sr.plane_found ? "found" : "not found") << " (" << sr.plane[0] << " " << sr.plane[1] << " " << sr.plane[2] << " " << sr.plane[3]
                          << "), " << sr.n_on_plane << " pixels on it, " << sr.n_components << " components, " << sr.n_segments << " segments kept" << std::endl;
                stocs::ModelCloud model;
                stocs::read_ply(model_path, &model, true);
                est.reset(new stocs::stocs_estimator(model, model_map, depth.data(), seg.class_prob.data(), segment_edges ? seg.edge.data() : NULL, dbg_dir, cam_intrinsics,
                                                     image_width, image_height, depth_scale, 1.0f, voxel_size, distance_threshold, ppf_tr_discretization,
                                                     ppf_rot_discretization, edge_threshold, class_threshold));
                if (depth_check || do_masks || vsd_opt.on || rv_opt.on) est->set_frame(depth.data(), seg.class_prob.data(), cam_intrinsics, depth_scale);
            } else {
            est.reset(new stocs::stocs_estimator(model_path, model_map, rgb_path, depth_path, class_probability_path, edge_probability_path, dbg_dir, cam_intrinsics,
                                                 image_width, image_height, depth_scale, 1.0f, voxel_size, distance_threshold, ppf_tr_discretization,
                                                 ppf_rot_discretization, edge_threshold, class_threshold));
            }
            if (!do_segment && (depth_check || do_masks || vsd_opt.on || rv_opt.on)) {   // the frame the scene was ingested from, for stocs_depth_check_poses / stocs_explain_poses / stocs_pose_errors_vsd
                std::vector<uint16_t> depth, prob;
                stocs::read_image(depth_path, 1, 16, image_width, image_height, &depth);
                stocs::read_image(class_probability_path, 1, 16, image_width, image_height, &prob);
                est->set_frame(depth.data(), prob.data(), cam_intrinsics, depth_scale);
            }
        }
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;  // no GPU => loud failure, never a CPU fallback
        return 2;
    }
    std::string instances_path, labels_path;
    std::string object = a2;
    if (clouds) {
        const size_t sl = object.find_last_of('/');
        if (sl != std::string::npos) object = object.substr(sl + 1);
        const size_t dot = object.find_last_of('.');
        if (dot != std::string::npos && dot > 0) object = object.substr(0, dot);
    }
    if (do_instances) {   // next to <out>
        const size_t sl = out_path.find_last_of('/');
        instances_path = (sl == std::string::npos ? std::string() : out_path.substr(0, sl + 1)) + "pose_instances_" + object + ".txt";
        if (do_masks) labels_path = (sl == std::string::npos ? std::string() : out_path.substr(0, sl + 1)) + "labels_" + object + ".pgm";
    }
    std::vector<stocs::stocs_estimator::TrialResult> trial_results;
    if (g_mask_mesh_triangles > 0 && !est->set_mesh(mesh_v, mesh_t)) { std::cerr << "set_mesh failed: " << stocs_last_error() << std::endl; return 2; }
    // --gt scores the pose file THIS run writes: one left at out_path by an earlier run must not stand in for it when this run finds no pose
    if (!gt_path.empty()) std::remove(out_path.c_str());
    const int rc = !track_path.empty() ? run_track(*est, track_path, track_min_lcp, out_path, dbg_dir, seed, n_trials, exact_ties, do_cluster, n_refine, &trial_results)
                                       : run_search(*est, std::cout, out_path, dbg_dir, seed, n_trials, exact_ties, do_cluster, n_refine, depth_check,
                                                    do_instances ? &inst_prm : NULL, instances_path, labels_path, &trial_results);
    if (rc == 0 && rv_opt.on) {   // after every other step, on the pose the run wrote
        if (!est->set_mesh(mesh_v, mesh_t)) { std::cerr << "set_mesh failed: " << stocs_last_error() << std::endl; return 2; }
        const int r2 = run_refine_visible(*est, rv_opt, out_path, object, gt_path);
        if (r2 != 0) return r2;
    }
    if (rc != 0 || gt_path.empty()) return rc;
    if (vsd_opt.mesh_triangles > 0 && !est->set_mesh(mesh_v, mesh_t)) { std::cerr << "set_mesh failed: " << stocs_last_error() << std::endl; return 2; }
    stocs_camera cam;   // a scene directory has a camera: MSPD is reported too
    memset(&cam, 0, sizeof(cam));
    cam.fx = cam_intrinsics[0]; cam.cx = cam_intrinsics[1]; cam.fy = cam_intrinsics[2]; cam.cy = cam_intrinsics[3];
    return report_gt(*est, gt_path, out_path, object, trial_results, syms, clouds ? NULL : &cam, vsd_opt);
}
