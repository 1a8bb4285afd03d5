// cluster.hip -- pose clustering.  Replaces clustering::greedy_clustering with get_pose_diff and quaternion_to_euler
// (reference src/pose_clustering.cpp:79-121, 27-71, 5-25; pose_diff.h).
// Host (stocs_cluster_poses): O(K log K + K*C) on at most 20 000 scored candidates of one trial, as in the reference (where it has
// no caller at all).  std::sort in the reference is unstable; a stable sort by descending score is used so that results are
// reproducible.
// Device (trial batches, stocs_run_trials_post): the candidates of a batch already sit on the device, so every trial of a piece is
// clustered there, one workgroup per trial.  The host loop is greedy non-maximum suppression, so no sort is needed: the arg-max of
// the survivors by best_key (stocs_math.h) -- highest score first, lowest index on ties, std::stable_sort's order -- is the next
// kept cluster, and every survivor within the thresholds of it (get_pose_diff(survivor, cluster), the host's argument order) drops
// out.  Same decisions as the host function, rounds = kept clusters.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "pose_diff.h"
#include "stocs_ctx.h"

namespace stocs {

static void pose_diff(const float* test, const float* base, const float* sym, float& rot_err, float& tr_err) {
    rot_err = pose_rot_err(pose_inverse_rotation(test), base, sym);
    tr_err = pose_trans_err(test, base);
}

// One workgroup per trial t of a piece.  Survivors: lcp > fraction * best_t (best_t = key hi of trial_best_kernel, the trial's best_lcp;
// the float product as the host forms it).  Per round, one pass over the survivors drops those the last kept cluster suppresses and
// takes the arg-max of the rest; the pass is also the suppression test of the round before.  Rounds stop after count + 1 clusters
// (the host's `size() > count` break) or when no survivor is left.  The translation test comes first: it is cheap, and a survivor it
// clears needs no rotation (both must hold to suppress).  The first pass reads every candidate; the survivors -- a few dozen per trial
// at the driver's fraction 0.8 -- go to LDS with their key and translation, and the later rounds walk that list only.  When more than
// CLUSTER_LDS survive (small fractions), the rounds walk the trial's candidates with a survivor flag per candidate in `alive`.
// hyp_idx[hyp_off[t] ..] gets the kept local indices in cluster order, hyp_cnt[t] their number (hyp_off[t + 1] - hyp_off[t] =
// min(count + 1, candidates of t) bounds it).
static const int CLUSTER_LDS = 2048;
__global__ __launch_bounds__(256) void trial_cluster_kernel(const float* __restrict__ P, const float* __restrict__ lcp, const int32_t* __restrict__ cand_off,
                                                            const float* __restrict__ best18, TrialClusterArgs a, uint8_t* __restrict__ alive,
                                                            const int32_t* __restrict__ hyp_off, int32_t* __restrict__ hyp_cnt, int32_t* __restrict__ hyp_idx) {
    __shared__ unsigned long long sh[4];
    __shared__ float acc[16];                       // the last kept cluster's pose
    __shared__ unsigned long long skey[CLUSTER_LDS];   // survivors: key (0: dropped) ...
    __shared__ float strans[CLUSTER_LDS][3];           // ... and translation
    __shared__ int n_surv;
    const int t = blockIdx.x;
    const int i0 = cand_off[t], n = cand_off[t + 1] - i0;
    const int h0 = hyp_off[t], cap = hyp_off[t + 1] - h0;
    const float thr = a.fraction * best18[(size_t)t * 18 + 1];
    if (threadIdx.x == 0) n_surv = 0;
    __syncthreads();
    int kept = 0, last = -1;
    bool in_lds = false;
    while (kept < cap) {
        unsigned long long k = 0;
        if (last < 0) {
            // the survivors (four loads in flight per lane)
            for (int b = (int)threadIdx.x; b < n; b += 1024) {
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = b + 256 * u < n ? lcp[(size_t)i0 + (size_t)(b + 256 * u)] : 0.0f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = b + 256 * u;
                    if (i >= n) break;
                    const size_t g = (size_t)i0 + (size_t)i;
                    const bool live = v[u] > thr;
                    alive[g] = live ? 1 : 0;
                    if (!live) continue;
                    const unsigned long long key = best_key(v[u], (uint32_t)i);
                    k = key > k ? key : k;
                    const int slot = atomicAdd(&n_surv, 1);
                    if (slot < CLUSTER_LDS) {
                        skey[slot] = key;
                        for (int d = 0; d < 3; ++d) strans[slot][d] = P[g * 16 + 12 + d];
                    }
                }
            }
        } else if (in_lds) {
            for (int j = (int)threadIdx.x; j < n_surv; j += 256) {
                const unsigned long long key = skey[j];
                if (!key) continue;
                const int i = (int)best_key_index(key);
                bool live = i != last;
                if (live && pose_trans_err3(strans[j], acc + 12) < a.min_distance &&
                    pose_rot_err(pose_inverse_rotation(P + ((size_t)i0 + (size_t)i) * 16), acc, a.sym) < a.min_angle)
                    live = false;
                if (!live) skey[j] = 0;
                else k = key > k ? key : k;
            }
        } else {
            for (int i = (int)threadIdx.x; i < n; i += 256) {
                const size_t g = (size_t)i0 + (size_t)i;
                if (!alive[g]) continue;
                bool live = i != last;
                if (live) {
                    const float* p = P + g * 16;
                    if (pose_trans_err(p, acc) < a.min_distance && pose_rot_err(pose_inverse_rotation(p), acc, a.sym) < a.min_angle) live = false;
                }
                if (!live) alive[g] = 0;
                else {
                    const unsigned long long key = best_key(lcp[g], (uint32_t)i);
                    k = key > k ? key : k;
                }
            }
        }
        k = wg_max_key<4>(k, sh);   // (its barrier also completes the survivor list of the first pass)
        if (!k) break;   // (uniform: every thread took the same maximum)
        if (last < 0) in_lds = n_surv <= CLUSTER_LDS;
        last = (int)best_key_index(k);
        if (threadIdx.x == 0) hyp_idx[h0 + kept] = last;
        if (threadIdx.x < 16) acc[threadIdx.x] = P[((size_t)i0 + (size_t)last) * 16 + threadIdx.x];
        ++kept;
        __syncthreads();   // acc written, sh read by all
        if (kept > a.count) break;   // sic: size > count
    }
    if (threadIdx.x == 0) hyp_cnt[t] = kept;
}

int enqueue_trial_cluster(stocs_ctx* c, int n_trials, const float* d_P, const float* d_lcp, const int32_t* d_cand_off, const float* d_best18,
                          const TrialClusterArgs& a, uint8_t* d_alive, const int32_t* d_hyp_off, int32_t* d_hyp_cnt, int32_t* d_hyp_idx) {
    if (n_trials <= 0) return STOCS_OK;
    hipLaunchKernelGGL(trial_cluster_kernel, dim3((unsigned)n_trials), dim3(256), 0, c->stream, d_P, d_lcp, d_cand_off, d_best18, a, d_alive, d_hyp_off,
                       d_hyp_cnt, d_hyp_idx);
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

}  // namespace stocs

using namespace stocs;

extern "C" int stocs_cluster_poses(const float* poses16, const float* lcp, int n, float acceptable_fraction, float best_score,
                                   int maximum_pose_count, float min_distance, float min_angle, const float* sym3,
                                   int32_t* out_idx, int cap, int* n_out) {
    if (n < 0 || (n && (!poses16 || !lcp)) || !sym3 || !n_out) return STOCS_ERR_INVALID;
    std::vector<int> pruned;
    for (int i = 0; i < n; ++i)
        if (lcp[i] > acceptable_fraction * best_score) pruned.push_back(i);
    std::stable_sort(pruned.begin(), pruned.end(), [&](int a, int b) { return lcp[a] > lcp[b]; });
    std::vector<int> kept;
    for (size_t ci = 0; ci < pruned.size(); ++ci) {
        const int cand = pruned[ci];
        bool inValid = false;
        for (size_t k = 0; k < kept.size(); ++k) {
            float re, te;
            pose_diff(poses16 + (size_t)cand * 16, poses16 + (size_t)kept[k] * 16, sym3, re, te);
            if (re < min_angle && te < min_distance) { inValid = true; break; }
        }
        if (!inValid) kept.push_back(cand);
        if ((int)kept.size() > maximum_pose_count) break;  // sic: size > count
    }
    *n_out = (int)kept.size();
    for (size_t i = 0; i < kept.size() && (int)i < cap; ++i) out_idx[i] = kept[i];
    return ((int)kept.size() > cap && out_idx) ? STOCS_ERR_CAPACITY : STOCS_OK;
}

// The device clustering on its own (a test and diagnosis facility: pageable copies, one synchronisation).  The kernel and its launcher
// are the pipeline's; this only puts the caller's arrays where post_piece finds the batch's.
static bool score_in_domain(float v) { return v != v || !signbit(v); }   // +0 and above, or NaN

extern "C" int stocs_cluster_trials_device(stocs_ctx* c, const float* poses16, const float* lcp, const int32_t* cand_off, const float* best_score, int n_trials,
                                           float acceptable_fraction, int maximum_pose_count, float min_distance, float min_angle, const float* sym3,
                                           int32_t* out_off, int32_t* out_cnt, int32_t* out_idx, int out_cap, int32_t* round0_survivors) {
    const char* me = "stocs_cluster_trials_device";
    if (!c) { set_error("%s: NULL context", me); return STOCS_ERR_INVALID; }
    if (n_trials < 0) { set_error("%s: negative size (n_trials %d)", me, n_trials); return STOCS_ERR_INVALID; }
    if (!cand_off || !sym3 || !out_off || (n_trials && (!best_score || !out_cnt))) { set_error("%s: NULL argument", me); return STOCS_ERR_INVALID; }
    if (maximum_pose_count < 0) { set_error("%s: maximum_pose_count %d < 0", me, maximum_pose_count); return STOCS_ERR_INVALID; }
    if (acceptable_fraction != acceptable_fraction) { set_error("%s: acceptable_fraction is NaN", me); return STOCS_ERR_INVALID; }
    if (!(min_distance > 0.0f) || !isfinite(min_distance)) { set_error("%s: min_distance %g must be positive and finite", me, (double)min_distance); return STOCS_ERR_INVALID; }
    if (!(min_angle > 0.0f) || !isfinite(min_angle)) { set_error("%s: min_angle %g must be positive and finite", me, (double)min_angle); return STOCS_ERR_INVALID; }
    if (out_cap < 0) { set_error("%s: negative capacity (out_cap %d)", me, out_cap); return STOCS_ERR_INVALID; }
    if (cand_off[0] != 0) { set_error("%s: cand_off[0] = %d, not 0", me, cand_off[0]); return STOCS_ERR_INVALID; }
    for (int t = 0; t < n_trials; ++t)
        if (cand_off[t + 1] < cand_off[t]) { set_error("%s: cand_off decreases at trial %d (%d -> %d)", me, t, cand_off[t], cand_off[t + 1]); return STOCS_ERR_INVALID; }
    const size_t N = (size_t)cand_off[n_trials], nT = (size_t)n_trials;
    if (N && (!poses16 || !lcp)) { set_error("%s: NULL candidates", me); return STOCS_ERR_INVALID; }
    for (size_t i = 0; i < N; ++i)
        if (!score_in_domain(lcp[i])) { set_error("%s: lcp[%zu] = %g is negative (scores are +0 and above, or NaN)", me, i, (double)lcp[i]); return STOCS_ERR_INVALID; }
    for (size_t t = 0; t < nT; ++t)
        if (!score_in_domain(best_score[t])) { set_error("%s: best_score[%zu] = %g is negative", me, t, (double)best_score[t]); return STOCS_ERR_INVALID; }
    out_off[0] = 0;
    for (size_t t = 0; t < nT; ++t) {
        const long long next = (long long)out_off[t] + trial_hyp_slots(maximum_pose_count, (long long)(cand_off[t + 1] - cand_off[t]));
        if (next > 0x7FFFFFFFll) { set_error("%s: more than 2^31 - 1 hypothesis slots", me); return STOCS_ERR_INVALID; }
        out_off[t + 1] = (int32_t)next;
    }
    const size_t H = (size_t)out_off[nT];
    if (H > (size_t)out_cap || (H && !out_idx)) { set_error("%s: out_idx holds %d entries, %zu are needed", me, out_idx ? out_cap : 0, H); return out_idx ? STOCS_ERR_CAPACITY : STOCS_ERR_INVALID; }
    if (n_trials == 0) return STOCS_OK;
    DeviceGuard dev_guard(c->device);
    Carve cv;
    const size_t o_P = cv.take(N * 64), o_lcp = cv.take(N * 4), o_coff = cv.take((nT + 1) * 4), o_b18 = cv.take(nT * 18 * 4), o_hoff = cv.take((nT + 1) * 4),
                 o_cnt = cv.take(nT * 4), o_idx = cv.take(H * 4), o_alive = cv.take(N);
    if (int rc = ensure_scratch(c, cv.total + 256)) return rc;
    void* d = c->d_scratch;
    float* d_P = Carve::at<float>(d, o_P); float* d_lcp = Carve::at<float>(d, o_lcp); int32_t* d_coff = Carve::at<int32_t>(d, o_coff);
    float* d_b18 = Carve::at<float>(d, o_b18); int32_t* d_hoff = Carve::at<int32_t>(d, o_hoff); int32_t* d_cnt = Carve::at<int32_t>(d, o_cnt);
    int32_t* d_idx = Carve::at<int32_t>(d, o_idx); uint8_t* d_alive = Carve::at<uint8_t>(d, o_alive);
    std::vector<float> b18(nT * 18, 0.0f);   // (key lo, key hi, pose[16]) per trial; the kernel reads the score in slot 1 alone
    for (size_t t = 0; t < nT; ++t) b18[t * 18 + 1] = best_score[t];
    if (N) {
        STOCS_HIP_CHECK(hipMemcpyAsync(d_P, poses16, N * 64, hipMemcpyHostToDevice, c->stream));
        STOCS_HIP_CHECK(hipMemcpyAsync(d_lcp, lcp, N * 4, hipMemcpyHostToDevice, c->stream));
    }
    STOCS_HIP_CHECK(hipMemcpyAsync(d_coff, cand_off, (nT + 1) * 4, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemcpyAsync(d_b18, b18.data(), nT * 18 * 4, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemcpyAsync(d_hoff, out_off, (nT + 1) * 4, hipMemcpyHostToDevice, c->stream));
    TrialClusterArgs a;
    a.fraction = acceptable_fraction; a.count = maximum_pose_count; a.min_distance = min_distance; a.min_angle = min_angle;
    for (int k = 0; k < 3; ++k) a.sym[k] = sym3[k];
    // The survivors of round 0, as the kernel itself decides them: with count 0 it stops after its first pass, and `alive` then holds
    // exactly that pass's flags (the full run below overwrites them on the path that walks them).
    std::vector<uint8_t> alive0(round0_survivors ? N : 0);
    if (round0_survivors) {
        TrialClusterArgs probe = a; probe.count = 0;
        if (int rc = enqueue_trial_cluster(c, n_trials, d_P, d_lcp, d_coff, d_b18, probe, d_alive, d_hoff, d_cnt, d_idx)) return rc;
        if (N) STOCS_HIP_CHECK(hipMemcpyAsync(alive0.data(), d_alive, N, hipMemcpyDeviceToHost, c->stream));
    }
    STOCS_HIP_CHECK(hipMemsetAsync(d_cnt, 0xFF, nT * 4, c->stream));
    if (H) STOCS_HIP_CHECK(hipMemsetAsync(d_idx, 0xFF, H * 4, c->stream));
    if (int rc = enqueue_trial_cluster(c, n_trials, d_P, d_lcp, d_coff, d_b18, a, d_alive, d_hoff, d_cnt, d_idx)) return rc;
    STOCS_HIP_CHECK(hipMemcpyAsync(out_cnt, d_cnt, nT * 4, hipMemcpyDeviceToHost, c->stream));
    if (H) STOCS_HIP_CHECK(hipMemcpyAsync(out_idx, d_idx, H * 4, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (size_t t = 0; round0_survivors && t < nT; ++t) {
        int32_t s = 0;
        for (int32_t i = cand_off[t]; i < cand_off[t + 1]; ++i) s += alive0[(size_t)i] ? 1 : 0;
        round0_survivors[t] = s;
    }
    return STOCS_OK;
}
