// track.hip -- pose tracking across frames (stocs_track_poses): a local search around n prior poses on the context's current scene,
// scored by the context's LCP path and optionally refined by refine.hip.  No reference counterpart: the reference detects from
// scratch on every frame.  The contract (draws, float order, tie rule) is written down at the declaration in include/stocs_hip.h.
//
// Per call, everything on the context's stream with no host wait in between:
//   the priors (centred on the host) go up into the incumbents through the pinned block;
//   rounds x (track_perturb_kernel: one thread per (prior, slot) writes the round's candidates,
//             launch_lcp: the scoring path of stocs_score_transforms,
//             track_best_kernel: one workgroup per prior takes the first maximum and writes the next incumbent);
//   with refinement, the incumbents are copied into refine.hip's workspace and refine_enqueue runs on them (stocs_track_poses_robust:
//   the trimmed, normal-gated settings, in groups of priors that share the rows of the workspace);
//   track_result_kernel forms the camera poses (as refine_final_kernel does) and the result records;
//   one copy back into the pinned block (the results, then every round's candidates and scores when details are kept), ONE
//   synchronisation.
// The kernels are small (a few hundred threads for a handful of priors): what a call costs is mostly launch gaps, so nothing is
// recorded or waited on between the rounds.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "stocs_ctx.h"

namespace stocs {

struct TrackState {
    static const StateOwner OWNER = OWN_TRACK;
    DevBlock mem;   // incumbents | incumbent lcp | prior lcp | results | candidates | scores (grow-only)
    bool kept = false;           // the last call kept its details (hT / hL below)
    int n = 0, samples = 0, rounds = 0;
    std::vector<float> hT, hL;   // round-major: round r, prior p, slot j at (r * n + p) * samples + j
    ~TrackState() { mem.free(); }
};

// round r's candidates: thread i = p * S + j.  Slot 0 copies the incumbent; slot j >= 1 perturbs it about the model origin with the
// draws and the float order of the header (every operation a single IEEE add / sub / mul / div / sqrt, -ffp-contract=off)
__global__ __launch_bounds__(256) void track_perturb_kernel(const float* __restrict__ inc, int n, int S, int rounds, int r, uint64_t seed, float tau, float h,
                                                            float* __restrict__ cand) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * S) return;
    const int p = (int)(i / S), j = (int)(i - (int64_t)p * S);
    const float* T = inc + (size_t)p * 16;
    float* o = cand + (size_t)i * 16;
    if (j == 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] = T[k];
        return;
    }
    const uint64_t attempt = (uint64_t)p * (uint64_t)rounds + (uint64_t)r;
    float e[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float u = (float)(rng64(seed, attempt, 8ull * (uint64_t)j + (uint64_t)k) >> 40) * 5.9604644775390625e-8f;   // * 2^-24: exact
        e[k] = 2.0f * u - 1.0f;   // exact
    }
    const float dtx = tau * e[0], dty = tau * e[1], dtz = tau * e[2];
    const float v0 = h * e[3], v1 = h * e[4], v2 = h * e[5];
    const float d = 1.0f + (v0 * v0 + (v1 * v1 + v2 * v2));
    const float s = 1.0f / sqrtf(d);
    const float w = s, x = v0 * s, y = v1 * s, z = v2 * s;
    float D[3][3];
    D[0][0] = 1.0f - 2.0f * (y * y + z * z); D[0][1] = 2.0f * (x * y - w * z); D[0][2] = 2.0f * (x * z + w * y);
    D[1][0] = 2.0f * (x * y + w * z); D[1][1] = 1.0f - 2.0f * (x * x + z * z); D[1][2] = 2.0f * (y * z - w * x);
    D[2][0] = 2.0f * (x * z - w * y); D[2][1] = 2.0f * (y * z + w * x); D[2][2] = 1.0f - 2.0f * (x * x + y * y);
    // R' = R dR (column-major in and out: R_ab = T[b * 4 + a])
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) o[b * 4 + a] = T[0 * 4 + a] * D[0][b] + (T[1 * 4 + a] * D[1][b] + T[2 * 4 + a] * D[2][b]);
    o[3] = 0.0f; o[7] = 0.0f; o[11] = 0.0f;
    o[12] = T[12] + dtx; o[13] = T[13] + dty; o[14] = T[14] + dtz; o[15] = 1.0f;
}

// one workgroup per prior: the first maximum of its S scores by best_key (stocs_math.h), a key for EVERY slot whatever its score:
// slot 0 wins every tie, also when all scores are 0.  Writes the next incumbent and its score; round 0 also
// records the prior's own score (slot 0)
__global__ __launch_bounds__(256) void track_best_kernel(const float* __restrict__ cand, const float* __restrict__ lcp, int S, int r, float* __restrict__ inc,
                                                         float* __restrict__ inc_lcp, float* __restrict__ prior_lcp) {
    __shared__ unsigned long long sh[4];
    const int p = blockIdx.x;
    const size_t base = (size_t)p * S;
    unsigned long long k = 0;
    for (int j = (int)threadIdx.x; j < S; j += 256) {
        const unsigned long long key = best_key(lcp[base + j], (uint32_t)j);
        k = key > k ? key : k;
    }
    k = wg_max_key<4>(k, sh);
    const uint32_t j = best_key_index(k);   // < S: every key above 0 came from a slot of this prior
    if (threadIdx.x < 16) inc[(size_t)p * 16 + threadIdx.x] = cand[(base + j) * 16 + threadIdx.x];
    if (threadIdx.x == 0) {
        inc_lcp[p] = best_key_score(k);
        if (r == 0) prior_lcp[p] = lcp[base];
    }
}

// the result records: the incumbent's camera form (camera_from_centred, as refine_final_kernel) and, with
// refinement (Pr != NULL), refine.hip's outputs
__global__ __launch_bounds__(64) void track_result_kernel(const float* __restrict__ inc, const float* __restrict__ inc_lcp, const float* __restrict__ prior_lcp, int n,
                                                          V3 cscene, V3 cmodel, const float* __restrict__ Pr, const float* __restrict__ lr,
                                                          const int32_t* __restrict__ nc, const int32_t* __restrict__ it, stocs_track_result* __restrict__ res) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float* To = inc + (size_t)k * 16;
    stocs_track_result* R = res + k;
    float P[16];
    camera_from_centred(To, cscene, cmodel, P);
    R->prior_lcp = prior_lcp[k];
    R->lcp = inc_lcp[k];
    for (int i = 0; i < 16; ++i) R->pose16[i] = P[i];
    if (Pr) {
        R->refined_lcp = lr[k];
        for (int i = 0; i < 16; ++i) R->refined_pose16[i] = Pr[(size_t)k * 16 + i];
        R->n_correspondences = nc[k];
        R->iterations = it[k];
    } else {
        R->refined_lcp = inc_lcp[k];
        for (int i = 0; i < 16; ++i) R->refined_pose16[i] = P[i];
        R->n_correspondences = 0;
        R->iterations = 0;
    }
}

static int check_params(const stocs_track_params* p) {
    if (p->rounds < 1 || p->rounds > STOCS_TRACK_MAX_ROUNDS) { set_error("stocs_track_poses: rounds %d outside [1, %d]", p->rounds, STOCS_TRACK_MAX_ROUNDS); return STOCS_ERR_INVALID; }
    if (p->samples < 1) { set_error("stocs_track_poses: samples %d < 1", p->samples); return STOCS_ERR_INVALID; }
    if (!(p->max_translation > 0.0f) || !isfinite(p->max_translation)) { set_error("stocs_track_poses: max_translation %g must be positive and finite", (double)p->max_translation); return STOCS_ERR_INVALID; }
    if (!(p->max_rotation_deg > 0.0f && p->max_rotation_deg < 180.0f)) { set_error("stocs_track_poses: max_rotation_deg %g outside (0, 180)", (double)p->max_rotation_deg); return STOCS_ERR_INVALID; }
    if (!(p->shrink > 0.0f && p->shrink <= 1.0f)) { set_error("stocs_track_poses: shrink %g outside (0, 1]", (double)p->shrink); return STOCS_ERR_INVALID; }
    if (p->refine_iterations < 0) { set_error("stocs_track_poses: refine_iterations %d < 0", p->refine_iterations); return STOCS_ERR_INVALID; }
    if (!(p->max_correspondence_distance > 0.0f) || !isfinite(p->max_correspondence_distance)) {
        set_error("stocs_track_poses: correspondence distance %g must be positive and finite", (double)p->max_correspondence_distance);
        return STOCS_ERR_INVALID;
    }
    return STOCS_OK;
}

// a camera-frame prior: every entry finite, the linear part a rotation within 1e-3 (max |R^T R - I|)
static bool prior_ok(const float* P) {
    for (int i = 0; i < 16; ++i) if (!isfinite(P[i])) return false;
    double e = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double d = (double)P[a * 4] * P[b * 4] + (double)P[a * 4 + 1] * P[b * 4 + 1] + (double)P[a * 4 + 2] * P[b * 4 + 2];   // columns a, b
            e = std::max(e, fabs(d - (a == b ? 1.0 : 0.0)));
        }
    return e <= 1e-3;
}

}  // namespace stocs

using namespace stocs;

// stocs_track_poses and stocs_track_poses_robust (who); rs: keep_ratio and min_normal_cos of the refinement, its iterations and distance are prm's
static int track_poses(stocs_ctx* c, const char* who, const float* priors, int n, const stocs_track_params* prm, RefineSettings rs, stocs_track_result* out) {
    if (!c) { set_error("stocs_track_poses: NULL context"); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("stocs_track_poses: n_priors %d < 0", n); return STOCS_ERR_INVALID; }
    if (n == 0) return STOCS_OK;
    if (!priors || !prm || !out) { set_error("stocs_track_poses: NULL priors, parameters or results"); return STOCS_ERR_INVALID; }
    {
        const int rc = check_params(prm);
        if (rc) return rc;
    }
    const int S = prm->samples, R = prm->rounds;
    if ((int64_t)n * S > (int64_t)STOCS_TRACK_MAX_CANDIDATES) {
        set_error("stocs_track_poses: %d priors x %d samples above the %d candidates of a round", n, S, STOCS_TRACK_MAX_CANDIDATES);
        return STOCS_ERR_INVALID;
    }
    for (int k = 0; k < n; ++k)
        if (!prior_ok(priors + (size_t)k * 16)) { set_error("stocs_track_poses: prior %d is not finite or its rotation is not orthonormal within 1e-3", k); return STOCS_ERR_INVALID; }
    if (c->nS <= 0) { set_error("stocs_track_poses: the context has no scene"); return STOCS_ERR_STATE; }
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    TrackState* st = ctx_state<TrackState>(c);
    st->kept = false;
    const bool keep = prm->keep_details != 0;
    const int64_t nc = (int64_t)n * S;   // candidates per round
    const int kr = keep ? R : 1;         // rounds whose candidates stay on the device
    // refine.hip's grid and workspace first: growing them synchronises, and nothing of this call may be in flight then
    RefineWork w;
    const bool refine = prm->refine_iterations > 0;
    rs.iterations = prm->refine_iterations; rs.distance = prm->max_correspondence_distance;
    if (refine) {
        const int rc = refine_prepare(c, who, n, c->nS, rs, 0, &w);
        if (rc) return rc;
    }
    Carve cv;
    const size_t o_inc = cv.take((size_t)n * 64), o_inc_lcp = cv.take((size_t)n * 4), o_prior_lcp = cv.take((size_t)n * 4),
                 o_res = cv.take((size_t)n * sizeof(stocs_track_result)), o_cand = cv.take((size_t)kr * nc * 64), o_lcp = cv.take((size_t)kr * nc * 4);
    { const int rc = st->mem.grow(c->stream, cv.total); if (rc) return rc; }
    float* d_inc = Carve::at<float>(st->mem.p, o_inc); float* d_inc_lcp = Carve::at<float>(st->mem.p, o_inc_lcp); float* d_prior_lcp = Carve::at<float>(st->mem.p, o_prior_lcp);
    stocs_track_result* d_res = Carve::at<stocs_track_result>(st->mem.p, o_res); float* d_cand = Carve::at<float>(st->mem.p, o_cand); float* d_lcp = Carve::at<float>(st->mem.p, o_lcp);
    // the read-back: the results, then (details) every round's candidates and scores -- one contiguous block, laid out as on the device
    const size_t back_cand = o_cand - o_res, back_lcp = o_lcp - o_res;
    const size_t back = keep ? back_lcp + (size_t)kr * nc * 4 : (size_t)n * sizeof(stocs_track_result);
    const size_t ib = o_inc_lcp - o_inc;   // the priors go up through the front of the pinned part
    char* h_in; char* hout;
    { const int rc = pinned_for(c, ib, al256(back), &h_in, &hout); if (rc) return rc; }   // ib is a multiple of 256: hout = h_in + ib
    // camera -> centred on the host, in float (centred_from_camera: the arithmetic the device would do)
    float* hin = (float*)h_in;
    const V3 cs = c->centroid_scene, cm = c->centroid_model;
    for (int k = 0; k < n; ++k) centred_from_camera(priors + (size_t)k * 16, cs, cm, hin + (size_t)k * 16);
    STOCS_HIP_CHECK(hipMemcpyAsync(d_inc, hin, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
    const unsigned pblocks = (unsigned)((nc + 255) / 256);
    double b = 1.0;   // shrink^r
    for (int r = 0; r < R; ++r) {
        const float tau = (float)((double)prm->max_translation * b);
        const float h = (float)tan((double)prm->max_rotation_deg * b * M_PI / 360.0);
        float* cr = d_cand + (keep ? (size_t)r * nc * 16 : 0);
        float* lr = d_lcp + (keep ? (size_t)r * nc : 0);
        hipLaunchKernelGGL(track_perturb_kernel, dim3(pblocks), dim3(256), 0, c->stream, (const float*)d_inc, n, S, R, r, prm->seed, tau, h, cr);
        STOCS_HIP_CHECK(hipGetLastError());
        {
            const int rc = launch_lcp(c, cr, (int)nc, lr, NULL, NULL, NULL, 0);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(track_best_kernel, dim3((unsigned)n), dim3(256), 0, c->stream, (const float*)cr, (const float*)lr, S, r, d_inc, d_inc_lcp, d_prior_lcp);
        STOCS_HIP_CHECK(hipGetLastError());
        b *= (double)prm->shrink;
    }
    if (refine) {
        STOCS_HIP_CHECK(hipMemcpyAsync(w.d_Tin, d_inc, (size_t)n * 64, hipMemcpyDeviceToDevice, c->stream));
        const int rc = refine_enqueue(c, w, false, NULL, NULL);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(track_result_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, (const float*)d_inc, (const float*)d_inc_lcp,
                       (const float*)d_prior_lcp, n, cs, cm, refine ? (const float*)w.d_Pout : (const float*)NULL, refine ? (const float*)w.d_lcp : (const float*)NULL,
                       refine ? (const int32_t*)w.d_nc : (const int32_t*)NULL, refine ? (const int32_t*)w.d_it : (const int32_t*)NULL, d_res);
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(hipMemcpyAsync(hout, d_res, back, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    memcpy(out, hout, (size_t)n * sizeof(stocs_track_result));
    st->n = n; st->samples = S; st->rounds = R;
    if (keep) {
        st->hT.assign((const float*)(hout + back_cand), (const float*)(hout + back_cand) + (size_t)R * nc * 16);
        st->hL.assign((const float*)(hout + back_lcp), (const float*)(hout + back_lcp) + (size_t)R * nc);
        st->kept = true;
    } else {
        st->hT.clear(); st->hL.clear();
    }
    return STOCS_OK;
}

extern "C" int stocs_track_poses(stocs_ctx* c, const float* priors, int n, const stocs_track_params* prm, stocs_track_result* out) {
    return track_poses(c, "stocs_track_poses", priors, n, prm, refine_plain(0, 0.0f), out);
}

extern "C" int stocs_track_poses_robust(stocs_ctx* c, const float* priors, int n, const stocs_track_params* prm, float keep_ratio, float min_normal_cos,
                                        stocs_track_result* out) {
    if (const char* why = robust_setting_error(keep_ratio, min_normal_cos)) { set_error("stocs_track_poses_robust: %s", why); return STOCS_ERR_INVALID; }
    return track_poses(c, "stocs_track_poses_robust", priors, n, prm, RefineSettings{0, 0.0f, keep_ratio, min_normal_cos}, out);
}

extern "C" int stocs_track_get_round(stocs_ctx* c, int prior, int round, float* T16, float* lcp, int cap, int* n) {
    if (!c || !n) { set_error("stocs_track_get_round: NULL context or count"); return STOCS_ERR_INVALID; }
    const TrackState* st = ctx_state_if<TrackState>(c);
    if (!st || !st->kept) { set_error("stocs_track_get_round: the last stocs_track_poses did not keep details"); return STOCS_ERR_STATE; }
    if (prior < 0 || prior >= st->n || round < 0 || round >= st->rounds) {
        set_error("stocs_track_get_round: prior %d / round %d outside [0, %d) x [0, %d)", prior, round, st->n, st->rounds);
        return STOCS_ERR_INVALID;
    }
    const int S = st->samples;
    *n = S;
    if (!T16 && !lcp) return STOCS_OK;
    if (cap < S) { set_error("stocs_track_get_round: capacity %d < %d", cap, S); return STOCS_ERR_CAPACITY; }
    const size_t off = ((size_t)round * st->n + prior) * S;
    if (T16) memcpy(T16, st->hT.data() + off * 16, (size_t)S * 64);
    if (lcp) memcpy(lcp, st->hL.data() + off, (size_t)S * 4);
    return STOCS_OK;
}
