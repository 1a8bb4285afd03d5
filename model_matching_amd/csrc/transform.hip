// transform.hip -- candidate rigid transforms from (base, congruent quad) pairs, and the
// verification driver.  Replaces
//   ComputeRigidTransformation                         reference src/stocs.cpp:270-361
//   stocs_estimator::get_rigid_transform_from_congruent_pair      stocs.cpp:871-941
//   the <=200-per-base loop of run_stocs_estimation     src/stocs_match_one_object.cpp:120-147
//   stocs_estimator::compute_best_transform             stocs.cpp:982-1004
// One thread per (base, quad): three-point frame alignment (no SVD, no MFMA: a 3x3*3x3 product per
// candidate is not a dense contraction).  Pure IEEE float arithmetic in the order fixed by
// stocs_math.h, so the result is bit-identical to the CPU restatement.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "prims.h"
#include "stocs_ctx.h"

namespace stocs {

struct M3 { float m[3][3]; };
STOCS_HD M3 mul33(const M3& A, const M3& B) {
    M3 C;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            C.m[i][j] = A.m[i][0] * B.m[0][j] + (A.m[i][1] * B.m[1][j] + A.m[i][2] * B.m[2][j]);
    return C;
}
STOCS_HD V3 mul3v(const M3& A, V3 v) {
    return mk3(A.m[0][0] * v.x + (A.m[0][1] * v.y + A.m[0][2] * v.z),
               A.m[1][0] * v.x + (A.m[1][1] * v.y + A.m[1][2] * v.z),
               A.m[2][0] * v.x + (A.m[2][1] * v.y + A.m[2][2] * v.z));
}
__device__ __forceinline__ V3 ld3(const float4* a, int i) { float4 v = a[i]; return mk3(v.x, v.y, v.z); }

// One candidate: the arithmetic of ComputeRigidTransformation + get_rigid_transform_from_congruent_pair on three point
// pairs.  Host and device run this same function (IEEE float operations in a fixed order, sqrt the only non-trivial one),
// so a candidate computed by the per-call entry point on the host equals the batched kernel's bit for bit.
STOCS_HD int rigid_transform_one(V3 p0, V3 p1, V3 p2, V3 q0, V3 q1, V3 q2, V3 cscene, V3 cmodel, float* T, float* P) {
    const V3 centroid1 = ((p0 + p1) + p2) / 3.0f;  // stocs.cpp:885
    const V3 centroid2 = ((q0 + q1) + q2) / 3.0f;  // stocs.cpp:907-909
    int ok = 1;
    // degenerate frames: the reference returns kLargeNumber from a bool function (true with an
    // uninitialised matrix, Q2) -- deliberate divergence: reject.
    V3 vp1 = p1 - p0;
    if (sqn3(vp1) == 0) ok = 0;
    vp1 = normalized3(vp1);
    V3 vp2 = (p2 - p0) - (dot3(p2 - p0, vp1) * vp1);
    if (sqn3(vp2) == 0) ok = 0;
    vp2 = normalized3(vp2);
    const V3 vp3 = cross3(vp1, vp2);
    V3 vq1 = q1 - q0;
    if (sqn3(vq1) == 0) ok = 0;
    vq1 = normalized3(vq1);
    V3 vq2 = (q2 - q0) - (dot3(q2 - q0, vq1) * vq1);
    if (sqn3(vq2) == 0) ok = 0;
    vq2 = normalized3(vq2);
    const V3 vq3 = cross3(vq1, vq2);
    // rotation = rotate_p.transpose() * rotate_q with the frames as rows (stocs.cpp:316-326)
    M3 Pt, Q;
    Pt.m[0][0] = vp1.x; Pt.m[1][0] = vp1.y; Pt.m[2][0] = vp1.z;
    Pt.m[0][1] = vp2.x; Pt.m[1][1] = vp2.y; Pt.m[2][1] = vp2.z;
    Pt.m[0][2] = vp3.x; Pt.m[1][2] = vp3.y; Pt.m[2][2] = vp3.z;
    Q.m[0][0] = vq1.x; Q.m[0][1] = vq1.y; Q.m[0][2] = vq1.z;
    Q.m[1][0] = vq2.x; Q.m[1][1] = vq2.y; Q.m[1][2] = vq2.z;
    Q.m[2][0] = vq3.x; Q.m[2][1] = vq3.y; Q.m[2][2] = vq3.z;
    const M3 R = mul33(Pt, Q);
    // (rotation*rotation).diagonal() - 1 > 1e-6 (sic: R*R not R*R^T, Q3; stocs.cpp:329)
    const M3 RR = mul33(R, R);
    const float kSmall = 1e-6f;
    if ((RR.m[0][0] - 1.0f > kSmall) || (RR.m[1][1] - 1.0f > kSmall) || (RR.m[2][2] - 1.0f > kSmall)) ok = 0;
    // rms (stocs.cpp:334-346) only gates through "rms >= 0" (:922): false iff NaN
    {
        float rms = 0.0f;
        rms += norm3((mul3v(R, 1.0f * q0 - centroid2) - p0) + centroid1);
        rms += norm3((mul3v(R, 1.0f * q1 - centroid2) - p1) + centroid1);
        rms += norm3((mul3v(R, 1.0f * q2 - centroid2) - p2) + centroid1);
        rms /= 4.0f;
        if (!(rms >= 0.0f)) ok = 0;
    }
    // etrans = I; scale(1); translate(c1); rotate(R); translate(-c2)  (stocs.cpp:348-357)
    const V3 t = centroid1 + mul3v(R, -centroid2);
    // camera-frame translation (stocs.cpp:925-933); rot*scale of computeRotationScaling == linear part
    const V3 tc = (centroid1 + cscene) - mul3v(R, centroid2 + cmodel);
#pragma unroll
    for (int col = 0; col < 3; ++col) {
#pragma unroll
        for (int r = 0; r < 3; ++r) { T[col * 4 + r] = R.m[r][col]; P[col * 4 + r] = R.m[r][col]; }
        T[col * 4 + 3] = 0.0f; P[col * 4 + 3] = 0.0f;
    }
    T[12] = t.x; T[13] = t.y; T[14] = t.z; T[15] = 1.0f;
    P[12] = tc.x; P[13] = tc.y; P[14] = tc.z; P[15] = 1.0f;
    return ok;
}

__global__ __launch_bounds__(256) void rigid_transform_kernel(const float4* __restrict__ spos, const float4* __restrict__ mpos,
                                                              const XformJob* __restrict__ jobs, int n, V3 cscene, V3 cmodel,
                                                              float* __restrict__ T_out, float* __restrict__ P_out,
                                                              int32_t* __restrict__ ok_out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) ok_out[n] = 0;   // the flag array is scanned over n + 1 entries so that the last output is the accepted count
    if (j >= n) return;
    const XformJob job = jobs[j];
    const V3 p0 = ld3(spos, job.s[0]), p1 = ld3(spos, job.s[1]), p2 = ld3(spos, job.s[2]);
    const V3 q0 = ld3(mpos, job.q[0]), q1 = ld3(mpos, job.q[1]), q2 = ld3(mpos, job.q[2]);
    float T[16], P[16];
    const int ok = rigid_transform_one(p0, p1, p2, q0, q1, q2, cscene, cmodel, T, P);
    float4* To = (float4*)(T_out + (size_t)j * 16);
    float4* Po = (float4*)(P_out + (size_t)j * 16);
#pragma unroll
    for (int col = 0; col < 4; ++col) {
        To[col] = make_float4(T[col * 4], T[col * 4 + 1], T[col * 4 + 2], T[col * 4 + 3]);
        Po[col] = make_float4(P[col * 4], P[col * 4 + 1], P[col * 4 + 2], P[col * 4 + 3]);
    }
    ok_out[j] = ok;
}

// the winner's camera-frame pose next to its key: one copy and one synchronisation tell the host everything
__global__ __launch_bounds__(64) void winner_pose_kernel(const unsigned long long* __restrict__ key, const float* __restrict__ P, int n, float* __restrict__ out18) {
    const unsigned long long k = *key;
    if (threadIdx.x == 0) { out18[0] = __uint_as_float((uint32_t)(k & 0xFFFFFFFFull)); out18[1] = __uint_as_float((uint32_t)(k >> 32)); }
    if (threadIdx.x < 16) {
        const uint32_t id = 0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull);   // best_key_index(k), written out: the helper changes this kernel's code
        out18[2 + threadIdx.x] = (k && id < (uint32_t)n) ? P[(size_t)id * 16 + threadIdx.x] : 0.0f;
    }
}

// ---- the pick draw of stocs_make_transforms: one text for the kernel below and for the host form (draw_picks_host) ----
// A base used whole (base_used_whole) contributes ranks 0 .. nq-1 of its sorted run.  A larger one gets a seeded sample without
// replacement (divergence Q5 from the biased 2N-vector shuffle of stocs_match_one_object.cpp:134-142, whose result depends on the C
// library's unseeded generator): a partial Fisher-Yates over the base's quads in EMISSION order (the order the loop of stocs.cpp:827-858
// finds them; any fixed enumeration serves a uniform draw, and this one needs no sort), kept sparse: only the touched entries of the
// identity permutation are stored, in an open-addressing table of hmask + 1 >= 4 * max_per_base slots (hkeys[h] = -1: free), reset
// per base.  The random words are independent of the swaps: word j of a base is rng(seed of its trial, its slot there, j).
STOCS_HD uint64_t pick_word(uint64_t seed, int slot, int j) { return rng64(seed, 0x5E1EC7ull + (uint64_t)slot, (uint64_t)j); }
inline uint32_t pick_table_mask(int max_per_base) {
    uint32_t hsize = 64;
    while (hsize < 4u * (uint32_t)max_per_base) hsize <<= 1;
    return hsize - 1;
}
// step j (upward from 0) with its word r_j: swap position j with position k = j + floor(r_j (nq - j) / 2^64) and return what is now at
// position j, the j-th pick.  Only position k is stored: steps go upward and k >= j, so position j is never read again.
STOCS_HD int draw_pick_step(int* hkeys, int* hvals, uint32_t hmask, long long nq, int j, uint64_t r_j) {
    auto slot_of = [&](int i) {
        uint32_t h = ((uint32_t)i * 2654435761u) & hmask;
        while (hkeys[h] != -1 && hkeys[h] != i) h = (h + 1) & hmask;
        return h;
    };
    const int k = j + (int)mulhi64(r_j, (uint64_t)(nq - j));
    const uint32_t hj = slot_of(j);
    const int vj = hkeys[hj] == j ? hvals[hj] : j;
    int vk = vj;
    if (k != j) {
        const uint32_t hk = slot_of(k);
        vk = hkeys[hk] == k ? hvals[hk] : k;
        hkeys[hk] = k; hvals[hk] = vj;
    }
    return vk;
}
// Row b of the pick table: table[b] = (first job, quad count lo, hi, unused); trial[b] (a batch of trials, stocs_run_trials; else NULL)
// = (seed lo, seed hi, slot of the base in ITS trial, 0): the base draws with the seed of its trial and under its slot there, and its
// candidates carry that slot, exactly as when the trial runs alone.
struct BaseDraw { int first; long long nq; uint64_t seed; int slot; };
STOCS_HD BaseDraw base_draw(const uint4* table, const uint4* trial, int b, uint64_t seed) {
    const uint4 t = table[b];
    BaseDraw d = {(int)t.x, (long long)(((unsigned long long)t.z << 32) | (unsigned long long)t.y), seed, b};
    if (trial) { const uint4 tr = trial[b]; d.seed = ((uint64_t)tr.y << 32) | (uint64_t)tr.x; d.slot = (int)tr.z; }
    return d;
}

// The draw on the device, one workgroup per base, table in LDS: the words r_j are computed by all threads, the swaps are sequential
// and done by one.  Runs on the auxiliary stream next to the materialisation of the small bases.
__global__ __launch_bounds__(256) void draw_picks_kernel(const uint4* __restrict__ table, const uint4* __restrict__ trial, uint64_t seed, int max_per_base, uint32_t hmask,
                                                         Pick* __restrict__ picks, int32_t* __restrict__ job_base) {
    extern __shared__ uint32_t lds_dyn[];
    int* hkeys = (int*)lds_dyn;                          // hmask + 1
    int* hvals = hkeys + (hmask + 1);                    // hmask + 1
    int* out = hvals + (hmask + 1);                      // max_per_base
    uint64_t* r = (uint64_t*)(out + ((max_per_base + 1) & ~1));   // max_per_base (8-byte aligned: everything before is an even number of words)
    const int b = blockIdx.x;
    const BaseDraw d = base_draw(table, trial, b, seed);
    if (d.nq <= 0) return;
    if (base_used_whole(d.nq, max_per_base)) {
        for (int i = threadIdx.x; i < (int)d.nq; i += blockDim.x) { picks[d.first + i] = Pick{b, i, d.first + i, 1}; job_base[d.first + i] = d.slot; }
        return;
    }
    for (uint32_t h = threadIdx.x; h <= hmask; h += blockDim.x) hkeys[h] = -1;
    for (int j = threadIdx.x; j < max_per_base; j += blockDim.x) r[j] = pick_word(d.seed, d.slot, j);
    __syncthreads();
    if (threadIdx.x == 0)
        for (int j = 0; j < max_per_base; ++j) out[j] = draw_pick_step(hkeys, hvals, hmask, d.nq, j, r[j]);
    __syncthreads();
    for (int j = threadIdx.x; j < max_per_base; j += blockDim.x) { picks[d.first + j] = Pick{b, out[j], d.first + j, 0}; job_base[d.first + j] = d.slot; }
}

// out[k] = a[idx[k]]: the accepted-candidate counts in front of every trial's first job (= where its candidates start)
__global__ __launch_bounds__(256) void gather_i32_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ idx, int n, int32_t* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = a[idx[k]];
}

// accepted candidates (ok != 0) keep their pick order: destination = exclusive scan of the flags
__global__ __launch_bounds__(256) void compact_candidates_kernel(const float4* __restrict__ T, const float4* __restrict__ P, const int32_t* __restrict__ ok,
                                                                 const int32_t* __restrict__ pos, const int32_t* __restrict__ job_base, int n,
                                                                 float4* __restrict__ To, float4* __restrict__ Po, float* __restrict__ lcp,
                                                                 int32_t* __restrict__ base_out, unsigned long long* __restrict__ best) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0 && best) *best = 0ull;   // the arg-max word of the verification that follows (stocs_verify_all): no fill of its own there
    if (j >= n || !ok[j]) return;
    const int d = pos[j];
#pragma unroll
    for (int k = 0; k < 4; ++k) { To[(size_t)d * 4 + k] = T[(size_t)j * 4 + k]; Po[(size_t)d * 4 + k] = P[(size_t)j * 4 + k]; }
    lcp[d] = 0.0f;   // "score is not computed at this time" (stocs.cpp:935-936)
    base_out[d] = job_base[j];
}

// Where the buffers of one stocs_make_transforms call lie.  `var` is the part the host fills in the pinned block (behind PIN_VAR) and
// the device reads at the same offsets inside the scratch block (from var_at on): the two tables of base_draw and, for a batch, the
// trial words (first job of every trial in; first candidate of every trial out, behind them).
struct CandLayout {
    Carve var, dev;
    size_t table, trial, words;                                          // in var
    size_t jobs, T, P, ok, pos, job_base, scan, picks, var_at;           // in the scratch block
    CandLayout(size_t nbases, size_t n_tr) { table = var.take(16 * nbases); trial = var.take(16 * nbases); words = var.take(8 * n_tr); }
    // n jobs; flags and their exclusive scan have n + 1 entries (the last flag is 0, the last scan entry the accepted count)
    void carve_scratch(size_t n, size_t scan_bytes, size_t n_device_picks) {
        jobs = dev.take(n * sizeof(XformJob)); T = dev.take(n * 64); P = dev.take(n * 64);
        ok = dev.take((n + 1) * 4); pos = dev.take((n + 1) * 4); job_base = dev.take((n + 1) * 4);
        scan = dev.take(scan_bytes); picks = dev.take(n_device_picks * sizeof(Pick)); var_at = dev.take(var.total);
    }
};

// The pick table of the context's base set (rows as base_draw reads them), written once for both forms of the draw; *n_jobs: the picks
// of all bases together.  A base's ranks are 32-bit: this is the one place that refuses more quads.
static int build_pick_table(stocs_ctx* c, int max_per_base, uint4* table, uint4* trial, size_t* n_jobs) {
    size_t n = 0;
    for (size_t b = 0; b < c->bases.size(); ++b) {
        const unsigned long long nq64 = c->quad_off[b + 1] - c->quad_off[b];
        if (nq64 > 0x7FFFFFFFull) { set_error("base %zu has %llu congruent quads (more than 2^31 - 1)", b, nq64); return STOCS_ERR_CAPACITY; }
        table[b] = make_uint4((uint32_t)n, (uint32_t)nq64, (uint32_t)(nq64 >> 32), 0u);
        if (trial) trial[b] = make_uint4((uint32_t)c->base_seed[b], (uint32_t)(c->base_seed[b] >> 32), (uint32_t)c->base_local[b], 0u);
        n += (size_t)base_pick_count((long long)nq64, max_per_base);
    }
    *n_jobs = n;
    return STOCS_OK;
}

// The draw on the host (per-base maxima whose table does not fit LDS, contexts without an auxiliary stream): what draw_picks_kernel
// writes to the device, into two vectors
static void draw_picks_host(const uint4* table, const uint4* trial, size_t nbases, uint64_t seed, int max_per_base, std::vector<Pick>* picks, std::vector<int>* job_base) {
    const uint32_t hmask = pick_table_mask(max_per_base);
    std::vector<int> hkeys(hmask + 1), hvals(hmask + 1);
    for (size_t b = 0; b < nbases; ++b) {
        const BaseDraw d = base_draw(table, trial, (int)b, seed);
        const bool whole = base_used_whole(d.nq, max_per_base);
        if (!whole) std::fill(hkeys.begin(), hkeys.end(), -1);
        const int count = (int)base_pick_count(d.nq, max_per_base);
        for (int j = 0; j < count; ++j)
            picks->push_back(Pick{(int32_t)b, whole ? j : draw_pick_step(hkeys.data(), hvals.data(), hmask, d.nq, j, pick_word(d.seed, d.slot, j)), d.first + j, whole});
        job_base->insert(job_base->end(), (size_t)count, d.slot);
    }
}

// The draw on the device, enqueued: table upload, fork, the small bases on the main stream next to draw_picks_kernel on the auxiliary
// one, join.  The table goes up on the MAIN stream: a host-to-device copy of a few hundred kilobytes enqueued on the otherwise idle
// auxiliary stream blocked the calling thread for 5.6 ms (64 trials of the ycb frame: 195 KB; measured, profiles/r04_trials_steps.json),
// the same copy on the stream that carries the rest of the call's work returns at once.
static int enqueue_device_picks(stocs_ctx* c, const CandLayout& L, bool batch, uint64_t seed, int max_per_base) {
    const size_t nbases = c->bases.size();
    char* d_var = Carve::at<char>(c->d_scratch, L.var_at);
    uint4* d_table = Carve::at<uint4>(d_var, L.table);
    Pick* d_picks = Carve::at<Pick>(c->d_scratch, L.picks);
    int32_t* dB = Carve::at<int32_t>(c->d_scratch, L.job_base);
    const uint32_t hmask = pick_table_mask(max_per_base);
    const size_t lds = (size_t)(2 * (hmask + 1) + ((max_per_base + 1) & ~1)) * 4 + (size_t)max_per_base * 8;
    STOCS_HIP_CHECK(hipMemcpyAsync(d_var, (char*)c->h_pin + PIN_VAR, (batch ? L.trial : L.table) + 16 * nbases, hipMemcpyHostToDevice, c->stream));
    c->audit.step(0, "table upload", {}, {{d_table, "pick table"}});
    int rc = stream_edge(c, c->ev_fork, 0, 1);
    if (rc) return rc;
    rc = stocs_internal_prepare_small(c, max_per_base);
    if (rc) return rc;
    hipLaunchKernelGGL(draw_picks_kernel, dim3((unsigned)nbases), dim3(256), lds, c->aux_stream, (const uint4*)d_table,
                       batch ? Carve::at<const uint4>(d_var, L.trial) : (const uint4*)NULL, seed, max_per_base, hmask, d_picks, dB);
    STOCS_HIP_CHECK(hipGetLastError());
    c->audit.step(1, "draw picks", {{d_table, "pick table"}}, {{d_picks, "picks"}, {dB, "job bases"}});
    return stream_edge(c, c->ev_join, 1, 0);
}

}  // namespace stocs

using namespace stocs;

extern "C" {

int stocs_rigid_transform(stocs_ctx* c, const int32_t* ids4, const int32_t* quad4, float* T16, float* pose16, int* ok) {
    if (!c || !ids4 || !quad4 || !ok) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    for (int k = 0; k < 4; ++k)
        if (ids4[k] < 0 || ids4[k] >= c->nS || quad4[k] < 0 || quad4[k] >= c->nM) { set_error("index out of range"); return STOCS_ERR_INVALID; }
    // on the host, from the context's own copies of the centred clouds: the reference's caller asks for one candidate per
    // call, up to 200 per base (stocs_match_one_object.cpp:120-147) -- a device round trip each would cost 35 us
    float T[16], P[16];
    *ok = rigid_transform_one(c->h_spos[ids4[0]], c->h_spos[ids4[1]], c->h_spos[ids4[2]], c->h_mpos[quad4[0]], c->h_mpos[quad4[1]], c->h_mpos[quad4[2]],
                              c->centroid_scene, c->centroid_model, T, P);
    if (T16) memcpy(T16, T, 64);
    if (pose16) memcpy(pose16, P, 64);
    return STOCS_OK;
}

int stocs_make_transforms(stocs_ctx* c, int max_per_base, uint64_t seed, int* n_candidates) {
    if (!c || max_per_base <= 0) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    if (c->quad_off.size() != c->bases.size() + 1) { set_error("stocs_make_transforms: call stocs_find_congruent_all first"); return STOCS_ERR_STATE; }
    c->timing[TIMING_TRANSFORMS].begin();   // (the steps of this call: stocs_last_call_timing(ctx, 1, ...))
    // 1. A trial without a single congruent set -- no bases, empty pair lists, or no (base, cell) that both lists occupy -- is a valid,
    // empty result (the reference's loop simply appends nothing, stocs_match_one_object.cpp:111-147): no candidates, "no pose".
    if (c->quad_off.back() == 0) {
        clear_candidates(c);
        c->best_lcp = 0; c->best_index = -1;
        if (n_candidates) *n_candidates = 0;
        c->trial_cand_off.assign(c->trial_first_base.size(), 0);
        c->timing[TIMING_TRANSFORMS].lap("no congruent sets");
        return STOCS_OK;
    }
    if (max_per_base > (1 << 24)) { set_error("stocs_make_transforms: max_per_base %d exceeds 2^24", max_per_base); return STOCS_ERR_INVALID; }
    // the picks are drawn on the device while the table of touched entries fits LDS; the host form, the same draw, serves larger maxima
    const bool device_picks = max_per_base <= 1024 && c->aux_stream && !getenv("STOCS_TRANSFORMS_HOST_PICKS");
    int rc;
    // host-drawn picks: the device starts on the small bases while the host draws the subsets of the large ones
    if (!device_picks && (rc = stocs_internal_prepare_small(c, max_per_base))) return rc;
    // a batch of trials (stocs_run_trials): every base draws with the seed of its trial and under its slot there
    const bool batch = !c->base_seed.empty();
    if (batch && (c->base_seed.size() != c->bases.size() || c->base_local.size() != c->bases.size())) { set_error("internal: trial tables do not match the base set"); return STOCS_ERR_STATE; }
    const size_t nbases = c->bases.size(), n_tr = batch ? c->trial_first_base.size() : 0;     // n_tr: trials + 1
    // 2. the pick table, 3. the picks when the host draws them (the quads themselves are produced on the device).  n > 0: some base has quads
    CandLayout L(nbases, n_tr);
    if ((rc = ensure_pinned(c, (size_t)PIN_VAR + L.var.total))) return rc;
    char* pin_var = (char*)c->h_pin + PIN_VAR;
    uint4* table = Carve::at<uint4>(pin_var, L.table);
    uint4* trial = batch ? Carve::at<uint4>(pin_var, L.trial) : NULL;
    size_t n = 0;
    if ((rc = build_pick_table(c, max_per_base, table, trial, &n))) return rc;
    std::vector<Pick> picks;
    std::vector<int> job_base;   // per job: the slot of its base in its own trial (what its candidates carry)
    if (!device_picks) draw_picks_host(table, trial, nbases, seed, max_per_base, &picks, &job_base);
    c->timing[TIMING_TRANSFORMS].lap(device_picks ? "pick table (host)" : "small bases enqueued + host picks");
    clear_candidates(c);
    c->best_lcp = 0; c->best_index = -1;
    // 4. buffers.  Candidates stay on the device: jobs -> transforms -> order-preserving compaction of the accepted ones
    size_t scan_tmp = 0;
    STOCS_HIP_CHECK(exclusive_scan(NULL, scan_tmp, (const uint32_t*)NULL, (uint32_t*)NULL, n + 1, c->stream));
    scan_tmp = al256(scan_tmp);
    L.carve_scratch(n, scan_tmp, device_picks ? n : 0);
    if ((rc = ensure_scratch(c, L.dev.total))) return rc;
    if ((size_t)c->cand_cap < n) {
        if (c->d_cand) { STOCS_HIP_CHECK(hipStreamSynchronize(c->stream)); (void)hipFree(c->d_cand); c->d_cand = NULL; }
        c->cand_cap = (int)(n + n / 4 + 1024);
        c->cand_bytes = (size_t)c->cand_cap * (16 + 16 + 1 + 1) * 4;
        STOCS_HIP_CHECK(dev_malloc((void**)&c->d_cand, c->cand_bytes));
    }
    c->timing[TIMING_TRANSFORMS].lap("buffers (scratch, pinned, candidate block)");
    if (!c->d_best) STOCS_HIP_CHECK(dev_malloc((void**)&c->d_best, 8));
    XformJob* dJ = Carve::at<XformJob>(c->d_scratch, L.jobs);
    float *dT = Carve::at<float>(c->d_scratch, L.T), *dP = Carve::at<float>(c->d_scratch, L.P);
    int32_t* dO = Carve::at<int32_t>(c->d_scratch, L.ok);        // n + 1 flags (the last one is 0)
    int32_t* dPos = Carve::at<int32_t>(c->d_scratch, L.pos);     // their exclusive scan; dPos[n] = accepted count
    int32_t* dB = Carve::at<int32_t>(c->d_scratch, L.job_base);
    const Pick* d_picks = NULL;
    // 3. the picks when the device draws them: behind the upload of the pick table
    if (device_picks) {
        if ((rc = enqueue_device_picks(c, L, batch, seed, max_per_base))) return rc;
        d_picks = Carve::at<Pick>(c->d_scratch, L.picks);
    }
    c->timing[TIMING_TRANSFORMS].lap("enqueue pick table upload + small bases + draws (auxiliary stream)");
    // 5. resolve: picks -> jobs
    const unsigned int* d_unresolved = NULL;
    if ((rc = stocs_internal_make_jobs(c, picks.data(), d_picks, (int)n, dJ, &d_unresolved))) return rc;
    c->timing[TIMING_TRANSFORMS].lap("enqueue resolve");
    // 6. transform, scan, compact
    if (!device_picks) STOCS_HIP_CHECK(hipMemcpyAsync(dB, job_base.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(rigid_transform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_spos, c->d_mpos, dJ, (int)n,
                       c->centroid_scene, c->centroid_model, dT, dP, dO);
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(exclusive_scan(Carve::at<void>(c->d_scratch, L.scan), scan_tmp, (const uint32_t*)dO, (uint32_t*)dPos, n + 1, c->stream));
    hipLaunchKernelGGL(compact_candidates_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const float4*)dT, (const float4*)dP, dO, dPos, dB,
                       (int)n, (float4*)cand_T(c), (float4*)cand_P(c), cand_lcp(c), cand_base(c), c->d_best);
    c->best_is_zero = true;
    STOCS_HIP_CHECK(hipGetLastError());
    // 7. read-backs: accepted count and unresolved picks into their pinned slot; batch: first job of every trial in, first candidate out
    int32_t* rb = (int32_t*)((char*)c->h_pin + PIN_TRANSFORMS);
    rb[0] = 0; rb[1] = 0;
    int32_t* tr_pin = Carve::at<int32_t>(pin_var, L.words);
    if (batch) {
        int32_t* d_tr = Carve::at<int32_t>(c->d_scratch, L.var_at + L.words);
        for (size_t t = 0; t < n_tr; ++t) { const size_t b = (size_t)c->trial_first_base[t]; tr_pin[t] = (int32_t)(b < nbases ? table[b].x : n); }
        STOCS_HIP_CHECK(hipMemcpyAsync(d_tr, tr_pin, 4 * n_tr, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(gather_i32_kernel, dim3((unsigned)((n_tr + 255) / 256)), dim3(256), 0, c->stream, (const int32_t*)dPos, (const int32_t*)d_tr, (int)n_tr, d_tr + n_tr);
        STOCS_HIP_CHECK(hipGetLastError());
        STOCS_HIP_CHECK(hipMemcpyAsync(tr_pin + n_tr, d_tr + n_tr, 4 * n_tr, hipMemcpyDeviceToHost, c->stream));
    }
    STOCS_HIP_CHECK(hipMemcpyAsync(&rb[0], dPos + n, 4, hipMemcpyDeviceToHost, c->stream));
    if (d_unresolved) STOCS_HIP_CHECK(hipMemcpyAsync(&rb[1], d_unresolved, 4, hipMemcpyDeviceToHost, c->stream));
    c->audit.use(0, d_picks, false, "picks", "resolve picks"); c->audit.use(0, dB, false, "job bases", "compact candidates");
    c->timing[TIMING_TRANSFORMS].lap("enqueue transform/scan/compact + read-backs");
    // 8. the one synchronisation point of this call
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->audit.host_sync(0);
    if (!c->audit.violations.empty()) {
        set_error("stocs_make_transforms: %zu stream-ordering violation(s); first: %s", c->audit.violations.size(), c->audit.violations[0].c_str());
        c->audit.violations.clear();
        return STOCS_ERR_STATE;
    }
    c->timing[TIMING_TRANSFORMS].lap("wait for the device");
    // 9. bookkeeping
    const unsigned int n_unresolved = (unsigned int)rb[1];
    if (n_unresolved) { set_error("stocs_make_transforms: %u picks could not be resolved (internal inconsistency)", n_unresolved); return STOCS_ERR_STATE; }
    c->n_cands = rb[0];
    c->cands_stale = c->n_cands > 0;
    if (batch) c->trial_cand_off.assign(tr_pin + n_tr, tr_pin + 2 * n_tr);
    if (n_candidates) *n_candidates = c->n_cands;
    return STOCS_OK;
}

// host mirror of the device-resident candidates (T, pose, lcp, base index), downloaded when somebody asks
static int ensure_host_candidates(stocs_ctx* c) {
    if (!c->cands_stale) return STOCS_OK;
    const size_t n = (size_t)c->n_cands;
    std::vector<float> T(n * 16), P(n * 16), l(n);
    std::vector<int32_t> b(n);
    STOCS_HIP_CHECK(hipMemcpyAsync(T.data(), cand_T(c), n * 64, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipMemcpyAsync(P.data(), cand_P(c), n * 64, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipMemcpyAsync(l.data(), cand_lcp(c), n * 4, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipMemcpyAsync(b.data(), cand_base(c), n * 4, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->cands.resize(n);
    for (size_t j = 0; j < n; ++j) {
        memcpy(c->cands[j].T, &T[j * 16], 64);
        memcpy(c->cands[j].pose, &P[j * 16], 64);
        c->cands[j].lcp = l[j];   // 0 until stocs_verify_all ("score is not computed at this time", stocs.cpp:935-936)
        c->cands[j].base_index = b[j];
    }
    c->cands_stale = false;
    return STOCS_OK;
}

int stocs_get_candidates(stocs_ctx* c, float* T16, float* pose16, float* lcp, int32_t* base_index, int cap, int* n) {
    if (!c || !n) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    *n = c->n_cands;
    if (!(T16 || pose16 || lcp || base_index)) return STOCS_OK;
    int rc = ensure_host_candidates(c);
    if (rc) return rc;
    for (int i = 0; i < *n && i < cap; ++i) {
        if (T16) memcpy(T16 + (size_t)i * 16, c->cands[i].T, 64);
        if (pose16) memcpy(pose16 + (size_t)i * 16, c->cands[i].pose, 64);
        if (lcp) lcp[i] = c->cands[i].lcp;
        if (base_index) base_index[i] = c->cands[i].base_index;
    }
    return (*n > cap) ? STOCS_ERR_CAPACITY : STOCS_OK;
}

int stocs_verify_all(stocs_ctx* c, float* best_lcp, int* best_idx, float* best_pose16) {
    if (!c) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    const int n = c->n_cands;
    c->best_lcp = 0; c->best_index = -1;
    float pose[16];
    memset(pose, 0, sizeof(pose));
    c->timing[TIMING_VERIFY].begin();
    if (n > 0) {
        // scores and the arg-max stay on the device: one LCP launch over the resident transforms, then
        // compute_best_transform (stocs.cpp:987-998: strict > from 0 => first maximum wins, Q18) as an integer max
        if (!c->d_best) STOCS_HIP_CHECK(dev_malloc((void**)&c->d_best, 8));
        int rc = launch_lcp(c, cand_T(c), n, cand_lcp(c), NULL, NULL, c->d_best, 0);   // scores + the arg-max key in one launch
        if (rc) return rc;
        rc = ensure_scratch(c, 256);
        if (rc) return rc;
        float* d_out = (float*)c->d_scratch;   // the transform jobs of this trial are done with the scratch area
        hipLaunchKernelGGL(winner_pose_kernel, dim3(1), dim3(64), 0, c->stream, (const unsigned long long*)c->d_best, (const float*)cand_P(c), n, d_out);
        STOCS_HIP_CHECK(hipGetLastError());
        if ((rc = ensure_pinned(c, PIN_VAR))) return rc;
        float* out18 = (float*)((char*)c->h_pin + PIN_VERIFY);   // pinned read-back slot (18 floats)
        STOCS_HIP_CHECK(hipMemcpyAsync(out18, d_out, 18 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        c->timing[TIMING_VERIFY].lap("enqueue score + arg-max + winner");
        STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
        c->timing[TIMING_VERIFY].lap("wait for the device");
        uint32_t lo, hi;
        memcpy(&lo, &out18[0], 4); memcpy(&hi, &out18[1], 4);
        const uint64_t key = ((uint64_t)hi << 32) | lo;
        c->cands_stale = true;   // the host mirror (if any) lacks the new scores
        if (key) {
            uint32_t id = 0;
            stocs_unpack_best(key, &c->best_lcp, &id);
            c->best_index = (int)id;
            memcpy(pose, &out18[2], 64);
        }
    }
    if (best_lcp) *best_lcp = c->best_lcp;
    if (best_idx) *best_idx = c->best_index;
    if (best_pose16) memcpy(best_pose16, pose, 64);
    return STOCS_OK;
}

}  // extern "C"
