// trials.hip -- N independent StoCS trials in ONE set of launches (stocs_run_trials).
//
// The reference runs one trial per process: 100 base attempts, their congruent sets, <= 200 candidates per base, the best
// candidate (reference src/stocs_match_one_object.cpp:81-165).  A trial of a 640x480 frame is a few hundred microseconds of
// device work spread over ~40 launches, on a chip that could run a hundred of them side by side -- and BASELINE config 4 asks
// for 64 of them.  Here the trials of a batch share every launch:
//   phase 1  class mode: n_trials x n_attempts workgroups of class_attempts_kernel; instance mode: a pair of workgroups per
//            trial on its own copy of the mutable image-space state (sample.hip, sample_trials);
//   phase 2  the trials' base sets are concatenated and go through stocs_find_congruent_all as ONE base set: every structure
//            there is keyed by base (gather segments, (base, cell) sort keys, run tables, per-base quad counts), so a base neither
//            knows nor cares whose trial it belongs to;
//   phase 3  stocs_make_transforms over the concatenation -- each base draws its <= max subset with the seed of ITS trial and
//            under its slot in that trial (transform.hip), the candidates come out trial by trial;
//   phase 4  one scoring launch over all candidates, then compute_best_transform (stocs.cpp:982-1004) per trial
//            (trial_best_kernel); instance mode scores trial by trial, each against its own decayed class probabilities (Q8).
// A batch that would not fit -- 32-bit (base, cell) keys, 64-bit packed quads, the memory ceiling -- is cut into pieces of
// consecutive trials, each piece one set of launches.  Every trial's bases, congruent sets, candidates and winner are bit for
// bit what stocs_reset_trial + stocs_sample_bases + stocs_find_congruent_all + stocs_make_transforms + stocs_verify_all give
// for the same seed (tests/test_trials_gpu.py).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "stocs_ctx.h"

namespace stocs {

struct TrialBatch {
    int mode = 0, nT = 0, nA = 0, max_per_base = 0;
    bool keep = false;
    std::vector<uint64_t> seeds;
    std::vector<BaseOut> res;                                   // nT * nA attempts
    std::vector<stocs_trial_result> out;                        // nT
    std::vector<std::vector<long long> > quads;                 // per trial: congruent sets of each valid base
    std::vector<std::vector<float> > T, P, lcp;                 // per trial, when details are kept
    std::vector<std::vector<int32_t> > cbase;
    bool post = false;                                          // the batch ran with post-processing (stocs_run_trials_post)
    std::vector<std::vector<stocs_trial_hypothesis> > hyps;     // per trial: its kept hypotheses, in cluster order
    int pieces = 0;
    int robust_groups = 0;                                      // stocs_run_trials_post_robust: groups its pieces refined their slots in, all pieces
};

// compute_best_transform (stocs.cpp:982-1004) of every trial of a piece: the first maximum of the trial's positive scores (best_key,
// stocs_math.h; a trial whose scores are all 0 has no pose) over the trial's own stretch of the score array, and the winner's
// camera-frame pose next to it.  One workgroup per trial; out18[t] = (key lo, key hi, pose[16]) with the candidate index counted inside the trial.
__global__ __launch_bounds__(256) void trial_best_kernel(const float* __restrict__ lcp, const float* __restrict__ P, const int32_t* __restrict__ cand_off,
                                                         float* __restrict__ out18) {
    __shared__ unsigned long long sh[4];
    const int t = blockIdx.x;
    const int i0 = cand_off[t], i1 = cand_off[t + 1];
    unsigned long long k = 0;
    for (int i = i0 + (int)threadIdx.x; i < i1; i += 256) {
        const float s = lcp[i];
        if (s > 0.0f) { const unsigned long long key = best_key(s, (uint32_t)(i - i0)); k = key > k ? key : k; }
    }
    k = wg_max_key<4>(k, sh);
    float* o = out18 + (size_t)t * 18;
    if (threadIdx.x == 0) { o[0] = __uint_as_float((uint32_t)(k & 0xFFFFFFFFull)); o[1] = __uint_as_float((uint32_t)(k >> 32)); }
    if (threadIdx.x < 16) o[2 + threadIdx.x] = k ? P[((size_t)i0 + best_key_index(k)) * 16 + threadIdx.x] : 0.0f;
}

// candidate -> trial of the piece (candidates come out trial by trial: a binary search in the per-trial offsets)
__global__ __launch_bounds__(256) void cand_trial_kernel(const int32_t* __restrict__ cand_off, int n_trials, int first_trial, int n, int32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = n_trials - 1;           // last t with cand_off[t] <= i
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (cand_off[mid] <= i) lo = mid; else hi = mid - 1; }
    out[i] = first_trial + lo;
}

// slot s of the piece's hypotheses -> its trial (last t with hyp_off[t] <= s) and its rank k there.  A slot below the trial's count
// gets the kept candidate's record (refined fields = the candidate's; refine_trial_hyp_kernel overwrites them after a refinement);
// with Tin != NULL also the refinement's input: the candidate's centred T16, or for an unused slot a pose parked far outside the scene
// and the model (refine_init_kernel freezes it, every LCP query of it misses at the first bounds test) -- the slots are sized before
// the counts are known, and the piece keeps its one synchronisation
__global__ __launch_bounds__(256) void trial_hyp_gather_kernel(const float* __restrict__ T, const float* __restrict__ P, const float* __restrict__ lcp,
                                                               const int32_t* __restrict__ cbase, const int32_t* __restrict__ cand_off,
                                                               const int32_t* __restrict__ hyp_off, const int32_t* __restrict__ hyp_cnt,
                                                               const int32_t* __restrict__ hyp_idx, int n_trials, int first_trial, int H,
                                                               stocs_trial_hypothesis* __restrict__ rec, float* __restrict__ Tin, int32_t* __restrict__ live,
                                                               int32_t* __restrict__ slot_trial) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= H) return;
    int lo = 0, hi = n_trials - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (hyp_off[mid] <= s) lo = mid; else hi = mid - 1; }
    const int t = lo, k = s - hyp_off[t];
    const bool on = k < hyp_cnt[t];
    const int id = on ? hyp_idx[s] : 0;
    const size_t g = (size_t)cand_off[t] + (size_t)id;
    if (on) {
        stocs_trial_hypothesis& r = rec[s];
        r.candidate_index = id; r.base_index = cbase[g]; r.lcp = lcp[g]; r.refined_lcp = lcp[g];
        for (int i = 0; i < 16; ++i) { const float v = P[g * 16 + i]; r.pose16[i] = v; r.refined_pose16[i] = v; }
        r.n_correspondences = 0; r.iterations = 0;
    }
    if (Tin) {
        for (int i = 0; i < 16; ++i) Tin[(size_t)s * 16 + i] = on ? T[g * 16 + i] : (i % 5 == 0 ? 1.0f : (i >= 12 && i < 15 ? 1.0e4f : 0.0f));
        live[s] = on ? 1 : 0;
        slot_trial[s] = first_trial + t;
    }
}

__global__ __launch_bounds__(256) void refine_trial_hyp_kernel(const int32_t* __restrict__ live, int H, const float* __restrict__ Pout, const float* __restrict__ lcp_out,
                                                               const int32_t* __restrict__ nc, const int32_t* __restrict__ it, stocs_trial_hypothesis* __restrict__ rec) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= H || !live[s]) return;
    stocs_trial_hypothesis& r = rec[s];
    for (int i = 0; i < 16; ++i) r.refined_pose16[i] = Pout[(size_t)s * 16 + i];
    r.refined_lcp = lcp_out[s]; r.n_correspondences = nc[s]; r.iterations = it[s];
}

static double now_ms() { return CallTiming::now_s() * 1e3; }

static int check_post(const stocs_trial_post* p) {
    if (!p) return STOCS_OK;
    if (p->maximum_pose_count < 0) { set_error("stocs_run_trials_post: maximum_pose_count %d < 0", p->maximum_pose_count); return STOCS_ERR_INVALID; }
    if (p->refine_iterations < 0) { set_error("stocs_run_trials_post: refine_iterations %d < 0", p->refine_iterations); return STOCS_ERR_INVALID; }
    if (p->acceptable_fraction != p->acceptable_fraction) { set_error("stocs_run_trials_post: acceptable_fraction is NaN"); return STOCS_ERR_INVALID; }
    if (!(p->min_distance > 0.0f) || !isfinite(p->min_distance)) {
        set_error("stocs_run_trials_post: min_distance %g must be positive and finite", (double)p->min_distance);
        return STOCS_ERR_INVALID;
    }
    if (!(p->min_angle > 0.0f) || !isfinite(p->min_angle)) {
        set_error("stocs_run_trials_post: min_angle %g must be positive and finite", (double)p->min_angle);
        return STOCS_ERR_INVALID;
    }
    if (!(p->max_correspondence_distance > 0.0f) || !isfinite(p->max_correspondence_distance)) {
        set_error("stocs_run_trials_post: max_correspondence_distance %g must be positive and finite", (double)p->max_correspondence_distance);
        return STOCS_ERR_INVALID;
    }
    return STOCS_OK;
}

// ---- how many bases one set of launches can take (congruent.hip: 32-bit (base, cell) sort keys with the run table, packed 64-bit
//      quads with the base above the four model ids) ----
static long long max_bases_per_piece(const stocs_ctx* c, int nA) {
    long long max_bases = 1 << 20;
    const float eps_unit = c->prm.distance_threshold / c->ratio;
    const int gridDepth = (int)(-log2f(eps_unit));
    const int egSize = (int)pow(2.0, (double)gridDepth);
    const long long NC = (long long)egSize * egSize * egSize;
    int id_bits = 1, cell_bits = 1;
    while ((1 << id_bits) < c->nM) id_bits++;
    if (NC > 0 && NC < (1ll << 31)) {
        while (cell_bits < 40 && (((unsigned long long)1 << cell_bits) - 1ull) < (unsigned long long)NC) cell_bits++;
        if (cell_bits < 32) max_bases = std::min(max_bases, 1ll << (32 - cell_bits));
        max_bases = std::min(max_bases, std::max(1ll, (1ll << 27) / NC));
    }
    if (4 * id_bits < 64) max_bases = std::min(max_bases, 1ll << std::min(20, 64 - 4 * id_bits));
    return std::max(max_bases, (long long)std::max(nA, 1));     // a single trial always goes through (as it does alone)
}

// the context's base set = the valid bases of trials t0 .. t1 one behind the other, each with its trial's seed and its slot there
static void assemble_piece(stocs_ctx* c, const TrialBatch* B, int t0, int t1) {
    c->bases.clear(); c->base_seed.clear(); c->base_local.clear(); c->trial_first_base.clear(); c->trial_cand_off.clear();
    c->quad_off.clear(); clear_candidates(c);
    for (int t = t0; t < t1; ++t) {
        c->trial_first_base.push_back((int32_t)c->bases.size());
        int slot = 0;
        for (int a = 0; a < B->nA; ++a) {
            const BaseOut& r = B->res[(size_t)t * B->nA + a];
            if (!r.valid) continue;
            BaseRec br; br.inv1 = r.inv[0]; br.inv2 = r.inv[1];
            for (int k = 0; k < 4; ++k) br.ids[k] = r.ids[k];
            c->bases.push_back(br);
            c->base_seed.push_back(B->seeds[(size_t)t]);
            c->base_local.push_back(slot++);
        }
    }
    c->trial_first_base.push_back((int32_t)c->bases.size());
}

// One piece (trials first .. first + n_trials of the batch) between its transforms and its results.
struct Piece {
    int first = 0, n_trials = 0, n_cand = 0;
    const stocs_trial_post* post = NULL;     // NULL: no post-processing
    const char* who = NULL;                  // post: the entry point, for messages
    RefineSettings refine_s = {};            // post: how the slots are refined (stocs_run_trials_post: the plain form)
    int groups = 0;                          // ... the groups of slots the refinement ran
    const float4* trial_weights = NULL;      // != NULL (instance mode): every candidate scores against the weights of its own trial (Q8)
    int n_slots = 0; bool refine = false;    // post: hypothesis slots of the piece, per trial min(count + 1, its candidates); they are refined
    std::vector<int32_t> hyp_off;            // post: first slot of every trial (+ 1)
    std::vector<float> best18;               // per trial (key lo, key hi, pose[16]); all zero for a trial without a positive score
    // The scratch of the scoring step (the transform jobs of the piece are done with the area), one layout for the device block and the
    // pinned block: the regions up to hyp_off exist in both (h_* mirrors d_*), the rest on the device only.  best18 | hyp_count |
    // hyp_records come back in ONE copy of back_bytes.
    int32_t* d_cand_off; float* d_best18; int32_t* d_hyp_count; stocs_trial_hypothesis* d_hyp_records; int32_t* d_hyp_off;
    int32_t* d_cand_trial; uint8_t* d_alive; int32_t* d_hyp_index; int32_t* d_slot_trial; int32_t* d_slot_live;
    int32_t* h_cand_off; float* h_best18; int32_t* h_hyp_count; stocs_trial_hypothesis* h_hyp_records; int32_t* h_hyp_off; size_t back_bytes;
};

// sizes the hypothesis slots and lays the piece's scratch out (grows the context's scratch and pinned blocks when they are too small)
static int plan_piece(stocs_ctx* c, Piece& pc) {
    const size_t nT = (size_t)pc.n_trials, n_cand = (size_t)pc.n_cand; const bool post = pc.post != NULL;
    pc.hyp_off.assign(post ? nT + 1 : 0, 0);
    for (size_t t = 0; post && t < nT; ++t)   // (the counts come back with the read-back)
        pc.hyp_off[t + 1] = pc.hyp_off[t] + trial_hyp_slots(pc.post->maximum_pose_count, (long long)(c->trial_cand_off[t + 1] - c->trial_cand_off[t]));
    pc.n_slots = post ? pc.hyp_off[nT] : 0;
    pc.refine = post && pc.post->refine_iterations > 0 && pc.n_slots > 0;
    const size_t H = (size_t)pc.n_slots;
    Carve cv;
    const size_t cand_off = cv.take((nT + 1) * 4), best18 = cv.take(nT * 18 * 4), hyp_count = cv.take(post ? nT * 4 : 0),
                 hyp_records = cv.take(post ? H * sizeof(stocs_trial_hypothesis) : 0), hyp_off = cv.take(post ? (nT + 1) * 4 : 0), mirrored = cv.total;
    const size_t cand_trial = cv.take(pc.trial_weights ? n_cand * 4 : 0), alive = cv.take(post ? n_cand : 0), hyp_index = cv.take(post ? H * 4 : 0),
                 slot_trial = cv.take(pc.refine ? H * 4 : 0), slot_live = cv.take(pc.refine ? H * 4 : 0);
    if (int rc = ensure_scratch(c, cv.total + 256)) return rc;
    if (int rc = ensure_pinned(c, (size_t)PIN_VAR + mirrored + 256)) return rc;
    void* d = c->d_scratch; void* h = (char*)c->h_pin + PIN_VAR;
    pc.d_cand_off = Carve::at<int32_t>(d, cand_off); pc.h_cand_off = Carve::at<int32_t>(h, cand_off); pc.d_best18 = Carve::at<float>(d, best18); pc.h_best18 = Carve::at<float>(h, best18);
    pc.d_hyp_count = Carve::at<int32_t>(d, hyp_count); pc.h_hyp_count = Carve::at<int32_t>(h, hyp_count); pc.d_hyp_off = Carve::at<int32_t>(d, hyp_off); pc.h_hyp_off = Carve::at<int32_t>(h, hyp_off);
    pc.d_hyp_records = Carve::at<stocs_trial_hypothesis>(d, hyp_records); pc.h_hyp_records = Carve::at<stocs_trial_hypothesis>(h, hyp_records);
    pc.d_cand_trial = Carve::at<int32_t>(d, cand_trial); pc.d_alive = Carve::at<uint8_t>(d, alive); pc.d_hyp_index = Carve::at<int32_t>(d, hyp_index);
    pc.d_slot_trial = Carve::at<int32_t>(d, slot_trial); pc.d_slot_live = Carve::at<int32_t>(d, slot_live);
    pc.back_bytes = post ? (hyp_records - best18) + H * sizeof(stocs_trial_hypothesis) : nT * 18 * 4;
    return STOCS_OK;
}

// While it lives, the context's scoring launches take candidate i's scene normals + weights from trial cand_trial[i]'s copy
// (LcpArgs::cand_trial); nothing when the piece has no per-trial weights.
struct TrialWeightsScope {
    stocs_ctx* c;
    TrialWeightsScope(stocs_ctx* ctx, const float4* weights, const int32_t* d_cand_trial) : c(ctx) { if (weights) { c->snrmw_override = weights; c->lcp_cand_trial = d_cand_trial; } }
    ~TrialWeightsScope() { c->snrmw_override = NULL; c->lcp_cand_trial = NULL; }
};

// the offsets go up, every candidate of the piece is scored in ONE launch, then the arg-max of each trial
static int score_piece(stocs_ctx* c, const Piece& pc) {
    const size_t off_bytes = 4 * ((size_t)pc.n_trials + 1);
    memcpy(pc.h_cand_off, c->trial_cand_off.data(), off_bytes);
    STOCS_HIP_CHECK(hipMemcpyAsync(pc.d_cand_off, pc.h_cand_off, off_bytes, hipMemcpyHostToDevice, c->stream));
    if (pc.post) {
        memcpy(pc.h_hyp_off, pc.hyp_off.data(), off_bytes);
        STOCS_HIP_CHECK(hipMemcpyAsync(pc.d_hyp_off, pc.h_hyp_off, off_bytes, hipMemcpyHostToDevice, c->stream));
    }
    if (pc.trial_weights) {
        hipLaunchKernelGGL(cand_trial_kernel, dim3((unsigned)((pc.n_cand + 255) / 256)), dim3(256), 0, c->stream, (const int32_t*)pc.d_cand_off, pc.n_trials, pc.first,
                           pc.n_cand, pc.d_cand_trial);
        STOCS_HIP_CHECK(hipGetLastError());
    }
    int rc;
    { TrialWeightsScope weights(c, pc.trial_weights, pc.d_cand_trial); rc = launch_lcp(c, cand_T(c), pc.n_cand, cand_lcp(c), NULL, NULL, NULL, 0); }
    if (rc) return rc;
    hipLaunchKernelGGL(trial_best_kernel, dim3((unsigned)pc.n_trials), dim3(256), 0, c->stream, (const float*)cand_lcp(c), (const float*)cand_P(c),
                       (const int32_t*)pc.d_cand_off, pc.d_best18);
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

// post-processing of the piece: greedy_clustering of every trial, the kept candidates' records, then (refine_iterations > 0) the
// point-to-plane refinement of every kept hypothesis of the piece in one enqueue, on the whole scene, written back into the records
// (the trimmed form: in groups of slots that share the rows of the workspace)
static int post_piece(stocs_ctx* c, Piece& pc) {
    const stocs_trial_post* post = pc.post;
    const int H = pc.n_slots;
    TrialClusterArgs ca;
    ca.fraction = post->acceptable_fraction; ca.count = post->maximum_pose_count; ca.min_distance = post->min_distance; ca.min_angle = post->min_angle;
    for (int d = 0; d < 3; ++d) ca.sym[d] = post->sym3[d];
    int rc = enqueue_trial_cluster(c, pc.n_trials, cand_P(c), cand_lcp(c), pc.d_cand_off, pc.d_best18, ca, pc.d_alive, pc.d_hyp_off, pc.d_hyp_count, pc.d_hyp_index);
    if (rc) return rc;
    RefineWork w;
    if (pc.refine && (rc = refine_prepare(c, pc.who, H, c->nS, pc.refine_s, 0, &w))) return rc;
    if (H > 0) {
        hipLaunchKernelGGL(trial_hyp_gather_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, c->stream, (const float*)cand_T(c), (const float*)cand_P(c),
                           (const float*)cand_lcp(c), (const int32_t*)cand_base(c), (const int32_t*)pc.d_cand_off, (const int32_t*)pc.d_hyp_off,
                           (const int32_t*)pc.d_hyp_count, (const int32_t*)pc.d_hyp_index, pc.n_trials, pc.first, H, pc.d_hyp_records, pc.refine ? w.d_Tin : NULL,
                           pc.d_slot_live, pc.d_slot_trial);
        STOCS_HIP_CHECK(hipGetLastError());
    }
    if (!pc.refine) return STOCS_OK;
    {   // instance mode: hypothesis s rescored against the weights of its own trial, as the scoring launch
        TrialWeightsScope weights(c, pc.trial_weights, pc.d_slot_trial);
        rc = refine_enqueue(c, w, false, pc.d_slot_live, &pc.groups);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(refine_trial_hyp_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, c->stream, (const int32_t*)pc.d_slot_live, H, (const float*)w.d_Pout,
                       (const float*)w.d_lcp, (const int32_t*)w.d_nc, (const int32_t*)w.d_it, pc.d_hyp_records);
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

// the piece's one read-back and its one synchronisation: the per-trial results [, the hypothesis counts and records behind them]
static int fetch_piece(stocs_ctx* c, TrialBatch* B, Piece& pc) {
    STOCS_HIP_CHECK(hipMemcpyAsync(pc.h_best18, pc.d_best18, pc.back_bytes, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    memcpy(pc.best18.data(), pc.h_best18, (size_t)pc.n_trials * 18 * 4);
    for (int t = 0; pc.post && t < pc.n_trials; ++t) {
        const int m = std::min(pc.h_hyp_count[t], pc.hyp_off[(size_t)t + 1] - pc.hyp_off[(size_t)t]);
        B->hyps[(size_t)(pc.first + t)].assign(pc.h_hyp_records + pc.hyp_off[(size_t)t], pc.h_hyp_records + pc.hyp_off[(size_t)t] + std::max(m, 0));
    }
    c->cands_stale = true;
    return STOCS_OK;
}

// the per-trial results of the piece, and with keep_details every trial's candidates
static int collect_piece(stocs_ctx* c, TrialBatch* B, const Piece& pc) {
    const size_t n_cand = (size_t)pc.n_cand;
    std::vector<float> hT, hP, hL; std::vector<int32_t> hB;
    if (B->keep && n_cand > 0) {
        hT.resize(n_cand * 16); hP.resize(n_cand * 16); hL.resize(n_cand); hB.resize(n_cand);
        STOCS_HIP_CHECK(hipMemcpyAsync(hT.data(), cand_T(c), n_cand * 64, hipMemcpyDeviceToHost, c->stream));
        STOCS_HIP_CHECK(hipMemcpyAsync(hP.data(), cand_P(c), n_cand * 64, hipMemcpyDeviceToHost, c->stream));
        STOCS_HIP_CHECK(hipMemcpyAsync(hL.data(), cand_lcp(c), n_cand * 4, hipMemcpyDeviceToHost, c->stream));
        STOCS_HIP_CHECK(hipMemcpyAsync(hB.data(), cand_base(c), n_cand * 4, hipMemcpyDeviceToHost, c->stream));
        STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    for (int t = 0; t < pc.n_trials; ++t) {
        const size_t bt = (size_t)(pc.first + t);
        stocs_trial_result& R = B->out[bt];
        const int b0 = c->trial_first_base[(size_t)t], b1 = c->trial_first_base[(size_t)t + 1];
        const int o0 = c->trial_cand_off[(size_t)t], o1 = c->trial_cand_off[(size_t)t + 1];
        R.n_bases = b1 - b0; R.n_candidates = o1 - o0; R.n_quads = 0;
        std::vector<long long>& q = B->quads[bt];
        q.resize((size_t)(b1 - b0));
        for (int b = b0; b < b1; ++b) {
            const long long nq = (size_t)b + 1 < c->quad_off.size() ? (long long)(c->quad_off[(size_t)b + 1] - c->quad_off[(size_t)b]) : 0;
            q[(size_t)(b - b0)] = nq; R.n_quads += nq;
        }
        const float* r18 = &pc.best18[(size_t)t * 18];
        uint32_t lo, hi; memcpy(&lo, r18, 4); memcpy(&hi, r18 + 1, 4);
        const unsigned long long key = ((unsigned long long)hi << 32) | lo;
        R.best_lcp = 0.0f; R.best_index = -1; memset(R.best_pose16, 0, sizeof(R.best_pose16));
        if (key) {
            R.best_lcp = best_key_score(key);
            R.best_index = (int32_t)best_key_index(key);
            memcpy(R.best_pose16, r18 + 2, 64);
        }
        if (B->keep && o1 > o0) {
            B->T[bt].assign(hT.begin() + (size_t)o0 * 16, hT.begin() + (size_t)o1 * 16);
            B->P[bt].assign(hP.begin() + (size_t)o0 * 16, hP.begin() + (size_t)o1 * 16);
            B->lcp[bt].assign(hL.begin() + o0, hL.begin() + o1);
            B->cbase[bt].assign(hB.begin() + o0, hB.begin() + o1);
        }
    }
    return STOCS_OK;
}

}  // namespace stocs

using namespace stocs;

extern "C" {

void stocs_internal_free_trials(stocs_ctx* c) {
    if (c && c->trials) { delete (TrialBatch*)c->trials; c->trials = NULL; }
}

int stocs_run_trials(stocs_ctx* c, int mode, int n_trials, const uint64_t* seeds, int n_attempts, float dispersion, int max_per_base, int keep_details,
                     stocs_trial_result* out) {
    return stocs_run_trials_post(c, mode, n_trials, seeds, n_attempts, dispersion, max_per_base, keep_details, NULL, out);
}

// stocs_run_trials_post and stocs_run_trials_post_robust (who; robust: it reports its groups); rs: keep_ratio and min_normal_cos of the
// refinement, its iterations and distance are post's
static int run_trials_post(stocs_ctx* c, const char* who, int mode, int n_trials, const uint64_t* seeds, int n_attempts, float dispersion, int max_per_base, int keep_details,
                           const stocs_trial_post* post, RefineSettings rs, bool robust, stocs_trial_result* out) {
    if (!c || n_trials < 0 || n_attempts < 0 || max_per_base <= 0 || (mode != 0 && mode != 1) || (n_trials && !seeds)) return STOCS_ERR_INVALID;
    if (check_post(post)) return STOCS_ERR_INVALID;
    if (post) { rs.iterations = post->refine_iterations; rs.distance = post->max_correspondence_distance; }
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    const double t_entry = now_ms();
    if (!c->index.built) { set_error("stocs_run_trials: PPF index not built"); return STOCS_ERR_STATE; }
    if (mode == 1 && n_attempts > 254) { set_error("instance mode labels segments with a u8 (<= 254 attempts, Q14)"); return STOCS_ERR_INVALID; }
    if ((long long)n_trials * (long long)std::max(n_attempts, 1) > (1ll << 24)) { set_error("stocs_run_trials: more than 2^24 attempts in one batch"); return STOCS_ERR_INVALID; }
    // every trial starts from the class probabilities given at construction (instance-mode sampling decays them in place) and
    // from an empty base set: what stocs_reset_trial does -- needed only when an earlier call left the prior decayed
    if (c->h_sprob != c->h_sprob0) { const int rc0 = stocs_reset_trial(c); if (rc0) return rc0; }
    clear_trial_batch(c);
    c->bases.clear(); c->quad_off.clear(); clear_candidates(c);
    c->best_lcp = 0; c->best_index = -1; c->last_segment.clear();
    if (!c->trials) c->trials = new TrialBatch();
    TrialBatch* B = (TrialBatch*)c->trials;
    const int nT = n_trials, nA = n_attempts;
    B->mode = mode; B->nT = nT; B->nA = nA; B->max_per_base = max_per_base; B->keep = keep_details != 0; B->pieces = 0; B->robust_groups = 0;
    B->seeds.assign(seeds, seeds + nT);
    B->res.assign((size_t)nT * (size_t)nA, BaseOut());
    B->out.assign((size_t)nT, stocs_trial_result());
    B->quads.assign((size_t)nT, std::vector<long long>());
    B->T.assign((size_t)nT, std::vector<float>()); B->P = B->T; B->lcp = B->T;
    B->cbase.assign((size_t)nT, std::vector<int32_t>());
    B->post = post != NULL;
    B->hyps.assign(post ? (size_t)nT : 0, std::vector<stocs_trial_hypothesis>());
    for (int t = 0; t < nT; ++t) { memset(&B->out[(size_t)t], 0, sizeof(stocs_trial_result)); B->out[(size_t)t].best_index = -1; }
    CallTiming& TM = c->timing[TIMING_TRIALS];
    TM.begin();
    double ms_cong = 0, ms_xf = 0, ms_ver = 0, ms_asm = 0, ms_res = 0;
    const double ms_setup = now_ms() - t_entry;
    if (nT == 0) return STOCS_OK;
    if (nA > 0 && c->nS > 0) {
        const int rc = sample_trials(c, mode, nT, seeds, nA, dispersion, B->res.data(), &c->snrmw_trial0, &c->snrmw_stride);
        if (rc) { clear_trial_batch(c); B->nT = 0; B->out.clear(); return rc; }
    }
    const float4* trial_weights = mode == 1 ? c->snrmw_trial0 : NULL;
    TM.lap("sampling: every attempt of every trial in one launch + read-back");
    const long long max_bases = max_bases_per_piece(c, nA);
    size_t max_bytes = (size_t)48 << 30;      // of 288 GB: a Cm trial is ~0.9 GB of pair lists, and at Cm a piece is then what the 64-bit quads can key (40 trials)
    if (const char* e = getenv("STOCS_TRIALS_MAX_MB")) max_bytes = (size_t)std::max(1, atoi(e)) << 20;
    int piece_cap = nT;
    if (const char* e = getenv("STOCS_TRIALS_PER_PIECE")) piece_cap = std::max(1, atoi(e));   // (tests: forces several pieces)
    std::vector<int32_t> n_valid((size_t)nT, 0);
    for (int t = 0; t < nT; ++t) for (int a = 0; a < nA; ++a) n_valid[(size_t)t] += B->res[(size_t)t * nA + a].valid ? 1 : 0;
    // An error inside a piece leaves through the common epilogue below (batch state cleared, context reset, the batch record marked
    // invalid) instead of returning from the middle of the loop with a half-filled record that the getters would serve.
    int rc = STOCS_OK;
    for (int t0 = 0; t0 < nT && !rc;) {
        int t1 = t0;
        long long nb = 0;
        while (t1 < nT && t1 - t0 < piece_cap && (t1 == t0 || nb + n_valid[(size_t)t1] <= max_bases)) { nb += n_valid[(size_t)t1]; ++t1; }
        int64_t total_quads = 0;
        for (;;) {   // the piece t0 .. t1: halved until its pair lists fit the ceiling
            const double t_asm = now_ms();
            assemble_piece(c, B, t0, t1);
            const double ta = now_ms();
            ms_asm += ta - t_asm;
            int too_big = 0;
            rc = stocs_internal_find_congruent(c, &total_quads, t1 - t0 > 1 ? max_bytes : 0, &too_big);   // (one trial alone always goes, as it does through the single calls)
            ms_cong += now_ms() - ta;
            if (rc || !too_big) break;
            if (t1 - t0 <= 1) { set_error("stocs_run_trials: the pair lists of one trial exceed 2^32 entries"); rc = STOCS_ERR_CAPACITY; break; }
            t1 = t0 + (t1 - t0) / 2;
            piece_cap = t1 - t0;          // the later pieces of this batch will be about as big
        }
        if (rc) break;
        B->pieces++;
        Piece pc;
        pc.first = t0; pc.n_trials = t1 - t0; pc.post = post; pc.who = who; pc.refine_s = rs; pc.trial_weights = trial_weights;
        pc.best18.assign((size_t)pc.n_trials * 18, 0.0f);
        double ta = now_ms();
        if ((rc = stocs_make_transforms(c, max_per_base, 0, &pc.n_cand))) break;
        ms_xf += now_ms() - ta;
        ta = now_ms();
        if ((int)c->trial_cand_off.size() != pc.n_trials + 1) c->trial_cand_off.assign((size_t)pc.n_trials + 1, 0);   // (a piece without any base)
        // ---- verification: every candidate of the piece scored, the arg-max of each trial [, clustered and refined], one synchronisation ----
        if (pc.n_cand > 0 && ((rc = plan_piece(c, pc)) || (rc = score_piece(c, pc)) || (post && (rc = post_piece(c, pc))) || (rc = fetch_piece(c, B, pc)))) break;
        ms_ver += now_ms() - ta;
        B->robust_groups += pc.groups;
        ta = now_ms();
        if ((rc = collect_piece(c, B, pc))) break;
        ms_res += now_ms() - ta;
        t0 = t1;
    }
    // the context is left as stocs_reset_trial leaves it: no bases, no candidates (the batch's results live in the batch record)
    clear_trial_batch(c);
    c->bases.clear(); c->quad_off.clear(); clear_candidates(c);
    c->best_lcp = 0; c->best_index = -1;
    if (rc) { B->nT = 0; B->out.clear(); return rc; }     // no results: stocs_trials_get_* answer STOCS_ERR_STATE ("trial out of range") for a failed batch
    {
        const double t_end = CallTiming::now_s();
        auto put = [&](const char* what, double ms) { if (TM.n < CallTiming::MAX_STEPS) { TM.label[TM.n] = what; TM.ms[TM.n] = ms; ++TM.n; } };
        put("congruent sets of all trials (stocs_find_congruent_all over the concatenated base sets, all pieces)", ms_cong);
        put("transforms of all trials (stocs_make_transforms, all pieces)", ms_xf);
        put("verification: scoring launch(es) + per-trial arg-max + read-back, all pieces", ms_ver);
        put("host: batch record set-up", ms_setup);
        put("host: base sets of the pieces assembled", ms_asm);
        put("host: per-trial results (+ candidate read-back with keep_details)", ms_res);
        put("whole call by the host clock", now_ms() - t_entry);
        if (robust) put("robust refinement: groups of slots that shared the workspace, all pieces", (double)B->robust_groups);
        put("pieces (sets of launches) the batch was cut into", (double)B->pieces);
        TM.t_last = t_end;
    }
    if (out) memcpy(out, B->out.data(), sizeof(stocs_trial_result) * (size_t)nT);
    return STOCS_OK;
}

int stocs_run_trials_post(stocs_ctx* c, int mode, int n_trials, const uint64_t* seeds, int n_attempts, float dispersion, int max_per_base, int keep_details,
                          const stocs_trial_post* post, stocs_trial_result* out) {
    return run_trials_post(c, "stocs_run_trials_post", mode, n_trials, seeds, n_attempts, dispersion, max_per_base, keep_details, post, refine_plain(0, 0.0f), false, out);
}

int stocs_run_trials_post_robust(stocs_ctx* c, int mode, int n_trials, const uint64_t* seeds, int n_attempts, float dispersion, int max_per_base, int keep_details,
                                 const stocs_trial_post* post, float keep_ratio, float min_normal_cos, stocs_trial_result* out) {
    const char* who = "stocs_run_trials_post_robust";
    if (!post) { set_error("%s: NULL post", who); return STOCS_ERR_INVALID; }
    if (const char* why = robust_setting_error(keep_ratio, min_normal_cos)) { set_error("%s: %s", who, why); return STOCS_ERR_INVALID; }
    return run_trials_post(c, who, mode, n_trials, seeds, n_attempts, dispersion, max_per_base, keep_details, post, RefineSettings{0, 0.0f, keep_ratio, min_normal_cos}, true, out);
}

static TrialBatch* batch_of(stocs_ctx* c, int trial) {
    if (!c || !c->trials) { set_error("no trial batch (call stocs_run_trials first)"); return NULL; }
    TrialBatch* B = (TrialBatch*)c->trials;
    if (trial < 0 || trial >= B->nT) { set_error("trial %d out of range (%d trials in the last batch)", trial, B->nT); return NULL; }
    return B;
}

int stocs_trials_get_bases(stocs_ctx* c, int trial, int32_t* base_ids4, float* inv2, int32_t* valid, int cap_attempts, int* n_attempts) {
    TrialBatch* B = batch_of(c, trial);
    if (!B) return STOCS_ERR_STATE;
    if (n_attempts) *n_attempts = B->nA;
    for (int a = 0; a < B->nA && a < cap_attempts; ++a) {
        const BaseOut& r = B->res[(size_t)trial * B->nA + a];
        if (base_ids4) for (int k = 0; k < 4; ++k) base_ids4[4 * a + k] = r.ids[k];
        if (inv2) { inv2[2 * a] = r.inv[0]; inv2[2 * a + 1] = r.inv[1]; }
        if (valid) valid[a] = r.valid;
    }
    return B->nA > cap_attempts && (base_ids4 || inv2 || valid) ? STOCS_ERR_CAPACITY : STOCS_OK;
}

int stocs_trials_get_quad_counts(stocs_ctx* c, int trial, int64_t* counts, int cap, int* n) {
    TrialBatch* B = batch_of(c, trial);
    if (!B || !n) return B ? STOCS_ERR_INVALID : STOCS_ERR_STATE;
    const std::vector<long long>& q = B->quads[(size_t)trial];
    *n = (int)q.size();
    if (counts) for (int b = 0; b < *n && b < cap; ++b) counts[b] = (int64_t)q[(size_t)b];
    return counts && *n > cap ? STOCS_ERR_CAPACITY : STOCS_OK;
}

int stocs_trials_get_hypotheses(stocs_ctx* c, int trial, stocs_trial_hypothesis* out, int cap, int* n) {
    TrialBatch* B = batch_of(c, trial);
    if (!B) return STOCS_ERR_STATE;
    if (!n || cap < 0) return STOCS_ERR_INVALID;
    if (!B->post) { set_error("stocs_trials_get_hypotheses: the batch was run without post-processing"); return STOCS_ERR_STATE; }
    const std::vector<stocs_trial_hypothesis>& h = B->hyps[(size_t)trial];
    *n = (int)h.size();
    if (!out) return STOCS_OK;
    const int m = std::min(*n, cap);
    if (m > 0) memcpy(out, h.data(), (size_t)m * sizeof(stocs_trial_hypothesis));
    return *n > cap ? STOCS_ERR_CAPACITY : STOCS_OK;
}

int stocs_trials_get_candidates(stocs_ctx* c, int trial, float* T16_centred, float* pose16_camera, float* lcp, int32_t* base_index, int cap, int* n) {
    TrialBatch* B = batch_of(c, trial);
    if (!B || !n) return B ? STOCS_ERR_INVALID : STOCS_ERR_STATE;
    *n = B->out[(size_t)trial].n_candidates;
    if (!(T16_centred || pose16_camera || lcp || base_index)) return STOCS_OK;
    if (!B->keep) { set_error("stocs_trials_get_candidates: the batch was run without keep_details"); return STOCS_ERR_STATE; }
    const int m = std::min(*n, cap);
    if (m > 0) {
        if (T16_centred) memcpy(T16_centred, B->T[(size_t)trial].data(), (size_t)m * 64);
        if (pose16_camera) memcpy(pose16_camera, B->P[(size_t)trial].data(), (size_t)m * 64);
        if (lcp) memcpy(lcp, B->lcp[(size_t)trial].data(), (size_t)m * 4);
        if (base_index) memcpy(base_index, B->cbase[(size_t)trial].data(), (size_t)m * 4);
    }
    return *n > cap ? STOCS_ERR_CAPACITY : STOCS_OK;
}

}  // extern "C"
