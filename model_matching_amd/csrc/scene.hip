// scene.hip -- scene-level selection of pose hypotheses across objects on the pixels of the depth image (stocs_scene_row_words,
// stocs_scene_footprints, stocs_scene_select): which hypotheses of several contexts form one consistent explanation of the frame.  The
// image-space, cross-object sibling of instances.hip, built on the splat and classification rules of render.hip.  No reference
// counterpart.  The contract is written down at the declarations in include/stocs_hip.h; tests/scene_ref.py restates it in float32
// numpy and integer set logic, and the results are equal bit for bit: depths are float bits under a minimum, counts are integer sums.
//
// stocs_scene_footprints, per chunk of hypotheses (256 MB of z-buffers; STOCS_SCENE_CHUNK=<hypotheses> forces a size):
//   clear     hipMemsetAsync with 0xFF: every hypothesis of the chunk has its own z-buffer of npix uint32 float bits, empty = all ones.
//   splat     scene_splat_kernel, render_splat_kernel's work split: one workgroup of 256 threads per (hypothesis, chunk of SCENE_CHUNK_POINTS
//             model points), the pose in scalar registers, one 32-bit atomicMin per pixel of splat_square (render_rules.h; p_2 > 1e-6: the
//             bits keep the order).
//   classify  scene_classify_kernel: a wavefront takes runs of 64 consecutive pixels of one hypothesis, classifies the touched ones with
//             z = its own minimum, turns the claim predicate into two row words with one __ballot (lane 0 stores them: no atomic on a row,
//             no bitset in LDS, padding words included) and counts with __popcll in wave-uniform registers; one integer atomicAdd per
//             counter and workgroup into the record.
// stocs_scene_select, one pinned read-back, ONE synchronisation:
//   own       scene_own_kernel, a wavefront per slot: popcount of the row, the sort key (cover_walk.h), the eligibility.
//   order     one 64-bit radix sort (prims.h) of the complemented keys with the slots as values, as instances.hip orders its hypotheses.
//   select    scene_select_kernel, ONE workgroup of 16 wavefronts with `covered` (up to 64 KB) and the group counts in LDS: the walk of
//             cover_walk.h, which instances.hip shares, behind this file's gate (eligible, and the slot's group not full; a selection
//             counts towards its group).  Cover and counts only grow.
//   finish    scene_finish_kernel, a wavefront per slot: |A_h \ covered_final| of the unselected ones and the reason, from the final state.
// The body of stocs_scene_footprints behind its checks is scene_footprints_with (render_shared.h): the chunk loop, the clears, the classify
// launch and the read-back around a z-buffer filler; the splats are one filler, the mesh of render_mesh.hip (stocs_scene_footprints_mesh)
// another.
// The ordering sort and the read-back region (results | selected | count) are cover_walk.h's; the pinned staging is pinned_for (stocs_ctx.h).
// Known limits: npix <= 2^19, n <= 16 384 slots, 1024 groups; classify walks the whole frame of every hypothesis; the walk is one workgroup.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "cover_walk.h"
#include "render_shared.h"

namespace stocs {

enum { SCENE_CHUNK_POINTS = 1024, SCENE_MAX_PIXELS = 1 << 19, SCENE_MAX_N = 16384, SCENE_MAX_GROUPS = 1024, SCENE_RUNS_PER_WAVE = 8 };
enum { SC_FOOTPRINT = 0, SC_NO_DEPTH, SC_AGREE, SC_IN_FRONT, SC_BEHIND, SC_ON_MASK, SC_CLAIMED, SC_COUNTS };
// the most dynamic LDS scene_select_kernel takes: the cover of 2^19 pixels, 1024 group counts, the round's results (of the CU's 160 KB)
#define SCENE_SELECT_MAX_LDS ((SCENE_MAX_PIXELS / 8) + SCENE_MAX_GROUPS * 4 + 4 * COVER_WAVES * 4)

struct SceneState {
    static const StateOwner OWNER = OWN_SCENE;
    ~SceneState() { work.free(); sel.free(); }
    DevBlock work;   // footprints: poses (n x 16 float) | records | one chunk of z-buffers, grow-only
    DevBlock sel;    // select: score | group | in_front | footprint | caps | own | eligible | keys (2) | slots (2) | rank | excl | cover | counts | results + selected + count | sort scratch
};

struct SceneArgs { int32_t max_selected, min_pixels; float min_fraction, max_violation; };

static int row_words(size_t npix) { return (int)((((npix + 31) / 32) + 3) & ~(size_t)3); }

// zbuf: the z-buffer of hypothesis blockIdx.y of the chunk at zbuf + blockIdx.y * npix
__global__ __launch_bounds__(256) void scene_splat_kernel(const float* __restrict__ poses, const float4* __restrict__ mpos, const float4* __restrict__ mnrm, int nM,
                                                          DepthArgs a, RenderArgs ra, uint32_t* __restrict__ zbuf) {
    const int h = (int)blockIdx.y;
    float P[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = poses[(size_t)h * 16 + i];   // the same address in every lane: uniform loads
    if (!pose_finite(P)) return;
    uint32_t* z = zbuf + (size_t)h * ((size_t)a.W * (size_t)a.H);
    const int first = (int)blockIdx.x * SCENE_CHUNK_POINTS;
    const int last = first + SCENE_CHUNK_POINTS < nM ? first + SCENE_CHUNK_POINTS : nM;
    for (int i = first + (int)threadIdx.x; i < last; i += 256) {
        const Projected p = project_point(P, mpos[i], mnrm[i], a);
        if (!p.in_image) continue;
        const uint32_t bits = __float_as_uint(p.z);
        splat_square(p, a, ra, [&](int r, int c) { atomicMin(&z[(size_t)r * (size_t)a.W + (size_t)c], bits); });
    }
}

// hypothesis blockIdx.y of the chunk: its row at rows + blockIdx.y * Wr (Wr / 2 runs of 64 pixels, the padding's included), its record at
// rec + blockIdx.y.  Run r of the hypothesis goes to wavefront r % (4 * gridDim.x); the loop bounds are wave-uniform, so every __ballot sees
// the whole wavefront.
__global__ __launch_bounds__(256) void scene_classify_kernel(const uint32_t* __restrict__ zbuf, const uint16_t* __restrict__ depth, const uint16_t* __restrict__ prob,
                                                             DepthArgs a, int npix, int Wr, int claim, uint32_t* __restrict__ rows, stocs_scene_record* __restrict__ rec) {
    __shared__ int cnt[SC_COUNTS];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int h = (int)blockIdx.y;
    const uint32_t* z = zbuf + (size_t)h * (size_t)npix;
    uint32_t* row = rows + (size_t)h * (size_t)Wr;
    if (tid < SC_COUNTS) cnt[tid] = 0;
    __syncthreads();
    const int n_runs = Wr >> 1;
    int n_foot = 0, n_nod = 0, n_agree = 0, n_front = 0, n_behind = 0, n_mask = 0, n_claim = 0;
    for (int run = (int)blockIdx.x * 4 + (tid >> 6); run < n_runs; run += (int)gridDim.x * 4) {
        const int px = run * 64 + lane;
        int cls = 0;
        if (px < npix) {
            const uint32_t bits = z[px];
            if (bits != 0xFFFFFFFFu) cls = classify_pixel(__uint_as_float(bits), (size_t)px, depth, prob, a);
        }
        const bool mine = claim ? (cls & 16) != 0 : (cls & 15) == 2;
        const unsigned long long m = __ballot(mine);
        if (lane == 0) { row[2 * run] = (uint32_t)m; row[2 * run + 1] = (uint32_t)(m >> 32); }
        n_foot += __popcll(__ballot(cls != 0)); n_nod += __popcll(__ballot((cls & 15) == 1)); n_agree += __popcll(__ballot((cls & 15) == 2));
        n_front += __popcll(__ballot((cls & 15) == 3)); n_behind += __popcll(__ballot((cls & 15) == 4)); n_mask += __popcll(__ballot((cls & 16) != 0));
        n_claim += __popcll(m);
    }
    if (lane == 0 && n_foot) {   // every other count is at most the footprint
        atomicAdd(&cnt[SC_FOOTPRINT], n_foot); atomicAdd(&cnt[SC_NO_DEPTH], n_nod); atomicAdd(&cnt[SC_AGREE], n_agree); atomicAdd(&cnt[SC_IN_FRONT], n_front);
        atomicAdd(&cnt[SC_BEHIND], n_behind); atomicAdd(&cnt[SC_ON_MASK], n_mask); atomicAdd(&cnt[SC_CLAIMED], n_claim);
    }
    __syncthreads();
    if (tid < SC_COUNTS && cnt[tid]) atomicAdd((int32_t*)(rec + h) + tid, cnt[tid]);   // the record's fields in the order of the SC_ enum
}

// a wavefront per slot, four to a workgroup: own = popcount of the row, the key of the order, the eligibility
__global__ __launch_bounds__(256) void scene_own_kernel(const uint32_t* __restrict__ rows, int Wr, int n, const float* __restrict__ score, const int32_t* __restrict__ in_front,
                                                        const int32_t* __restrict__ footprint, SceneArgs a, int32_t* __restrict__ own, uint8_t* __restrict__ eligible,
                                                        uint64_t* __restrict__ key, uint32_t* __restrict__ idx) {
    const int lane = (int)threadIdx.x & 63;
    const int h = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (h >= n) return;   // wave-uniform
    const uint4* row = (const uint4*)(rows + (size_t)h * (size_t)Wr);
    int o = 0;
    for (int i = lane; i < (Wr >> 2); i += 64) { const uint4 e = row[i]; o += __popc(e.x) + __popc(e.y) + __popc(e.z) + __popc(e.w); }
    o = wave_sum_i(o);
    if (lane == 0) {
        const float s = score[h];
        const float limit = a.max_violation * (float)footprint[h];
        own[h] = o;
        eligible[h] = (s > 0.0f && o >= a.min_pixels && (float)in_front[h] <= limit) ? 1 : 0;
        key[h] = cover_order_key(s, h);
        idx[h] = (uint32_t)h;
    }
}

// the gate of this walk: neither an ineligible slot nor one of a full group comes back, so its row need not be read.  cnt and r_g are in
// LDS: r_g[k] is the group of the slot wavefront k tests this round, kept for thread 0, which counts a selection towards it
struct SceneGate {
    const uint8_t* __restrict__ eligible; const int32_t* __restrict__ group; const int32_t* __restrict__ cap;
    int* cnt; int* r_g;
    __device__ __forceinline__ bool open(int h) const {
        const int g = group[h];
        if ((threadIdx.x & 63) == 0) r_g[threadIdx.x >> 6] = g;
        return eligible[h] != 0 && cnt[g] < cap[g];
    }
    __device__ __forceinline__ void took(int, int k) const { cnt[r_g[k]] += 1; }
};

// the walk: cover_walk (cover_walk.h) by one workgroup.  LDS: Wr words of cover, n_groups counts, then 4 x 16 words of the round's
// results (the walk's three, then the groups).
__global__ __launch_bounds__(64 * COVER_WAVES) void scene_select_kernel(const uint32_t* __restrict__ rows, int Wr, const uint32_t* __restrict__ order,
                                                                        const int32_t* __restrict__ own, const uint8_t* __restrict__ eligible,
                                                                        const int32_t* __restrict__ group, const int32_t* __restrict__ cap, int n, int n_groups,
                                                                        SceneArgs a, int32_t* __restrict__ rank, int32_t* __restrict__ excl,
                                                                        int32_t* __restrict__ selected, int32_t* __restrict__ n_selected,
                                                                        uint32_t* __restrict__ cover_out, int32_t* __restrict__ cnt_out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sel_lds[];
    int* cnt = (int*)(sel_lds + Wr);
    int* r = cnt + n_groups;
    const SceneGate gate = {eligible, group, cap, cnt, r + 3 * COVER_WAVES};
    const CoverArgs wa = {a.max_selected, a.min_pixels, a.min_fraction};
    const int tid = (int)threadIdx.x, threads = 64 * COVER_WAVES;
    for (int i = tid; i < n_groups; i += threads) cnt[i] = 0;   // in front of the walk's first barrier
    cover_walk(rows, Wr, order, own, n, wa, gate, (uint4*)sel_lds, r, rank, excl, selected, n_selected, cover_out);
    for (int i = tid; i < n_groups; i += threads) cnt_out[i] = cnt[i];
}

// a wavefront per slot, four to a workgroup: the record, decided from the final cover and counts
__global__ __launch_bounds__(256) void scene_finish_kernel(const uint32_t* __restrict__ rows, int Wr, const uint32_t* __restrict__ cover, const int32_t* __restrict__ own,
                                                           const uint8_t* __restrict__ eligible, const int32_t* __restrict__ group, const int32_t* __restrict__ cap,
                                                           const int32_t* __restrict__ cnt, const int32_t* __restrict__ rank, const int32_t* __restrict__ excl, int n,
                                                           SceneArgs a, stocs_scene_result* __restrict__ out) {
    const int lane = (int)threadIdx.x & 63;
    const int h = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (h >= n) return;   // wave-uniform
    const int r = rank[h];
    const int ex = cover_final_exclusive(rows, Wr, cover, excl, h, r, lane);
    if (lane == 0) {
        const int o = own[h], g = group[h];
        int reason = 0;
        if (r < 0) {
            if (eligible[h] == 0) reason = 1;
            else if (!(ex >= a.min_pixels && (float)ex >= a.min_fraction * (float)o)) reason = 2;
            else if (cnt[g] >= cap[g]) reason = 3;
            else reason = 4;
        }
        stocs_scene_result res;
        res.rank = r; res.own = o; res.exclusive = ex; res.reason = reason;
        out[h] = res;
    }
}


static int check_params(const char* who, const stocs_scene_params* p) {
    if (p->max_selected < 1) { set_error("%s: max_selected %d < 1", who, p->max_selected); return STOCS_ERR_INVALID; }
    if (p->min_pixels < 1) { set_error("%s: min_pixels %d < 1", who, p->min_pixels); return STOCS_ERR_INVALID; }
    if (!(p->min_exclusive_fraction > 0.0f) || !(p->min_exclusive_fraction <= 1.0f)) {
        set_error("%s: min_exclusive_fraction %g is not in (0, 1]", who, (double)p->min_exclusive_fraction);
        return STOCS_ERR_INVALID;
    }
    if (!(p->max_violation_fraction >= 0.0f) || !(p->max_violation_fraction <= 1.0f)) {
        set_error("%s: max_violation_fraction %g is not in [0, 1]", who, (double)p->max_violation_fraction);
        return STOCS_ERR_INVALID;
    }
    return STOCS_OK;
}

int scene_check_pixels(const char* who, size_t npix) {
    if (npix > (size_t)SCENE_MAX_PIXELS) {
        set_error("%s: a frame of %zu pixels, at most %d (the cover of the walk is a 64 KB bitset in LDS)", who, npix, (int)SCENE_MAX_PIXELS);
        return STOCS_ERR_CAPACITY;
    }
    return STOCS_OK;
}

}  // namespace stocs

using namespace stocs;

extern "C" void stocs_default_scene_params(stocs_scene_params* p) {
    if (!p) return;
    p->max_selected = 64; p->min_pixels = 50; p->min_exclusive_fraction = 0.5f; p->max_violation_fraction = 0.2f;
}

extern "C" int stocs_scene_row_words(int width, int height) {
    if (width < 1 || height < 1) return 0;
    return row_words((size_t)width * (size_t)height);
}

static int fill_splats(stocs_ctx* c, const void* self, const float* d_pose, int m, const DepthArgs& a, uint32_t* d_z, void*);

extern "C" int stocs_scene_footprints(stocs_ctx* c, const float* poses, int n, int slot_base, int n_slots, const stocs_render_params* prm, int claim, void* d_rows,
                                      stocs_scene_record* out) {
    static const char* who = "stocs_scene_footprints";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n == 0) return STOCS_OK;
    if (!poses || !prm || !d_rows || !out) { set_error("%s: NULL poses, parameters, rows or records", who); return STOCS_ERR_INVALID; }
    if (claim != 0 && claim != 1) { set_error("%s: claim %d is neither 0 (agree) nor 1 (on_mask)", who, claim); return STOCS_ERR_INVALID; }
    if (slot_base < 0 || (long long)slot_base + (long long)n > (long long)n_slots) {
        set_error("%s: slots %d .. %lld outside a pool of %d", who, slot_base, (long long)slot_base + (long long)n - 1, n_slots);
        return STOCS_ERR_INVALID;
    }
    { const int rc = check_params(who, prm); if (rc) return rc; }
    DepthState* F = NULL;
    { const int rc = check_frame(who, c, &F); if (rc) return rc; }
    { const int rc = scene_check_pixels(who, F->npix); if (rc) return rc; }
    const RenderArgs ra = render_args(prm, 0);
    const SceneFill fill = {fill_splats, &ra, 0};
    return scene_footprints_with(c, F, &ctx_state<SceneState>(c)->work, fill, poses, n, slot_base, prm->tolerance, prm->class_threshold, claim, d_rows, out);
}

// the splats as a SceneFill: self is the call's RenderArgs
static int fill_splats(stocs_ctx* c, const void* self, const float* d_pose, int m, const DepthArgs& a, uint32_t* d_z, void*) {
    const unsigned point_chunks = (unsigned)((c->nM + SCENE_CHUNK_POINTS - 1) / SCENE_CHUNK_POINTS);
    if (!point_chunks) return STOCS_OK;
    hipLaunchKernelGGL(scene_splat_kernel, dim3(point_chunks, (unsigned)m), dim3(256), 0, c->stream, d_pose, (const float4*)c->d_mpos_raw, (const float4*)c->d_mnrm, c->nM, a,
                       *(const RenderArgs*)self, d_z);
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

int stocs::scene_footprints_with(stocs_ctx* c, DepthState* F, DevBlock* work, const SceneFill& fill, const float* poses, int n, int slot_base, float tolerance,
                                 float class_threshold, int claim, void* d_rows, stocs_scene_record* out) {
    DeviceGuard dev_guard(c->device);
    const size_t npix = F->npix;
    const int Wr = row_words(npix);
    // one z-buffer per hypothesis of a chunk; the hypothesis is blockIdx.y (at most 65 535 per launch)
    size_t chunk = std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)n, 65535), ((size_t)256 << 20) / (4 * npix)));
    if (const char* e = getenv("STOCS_SCENE_CHUNK")) { const long v = atol(e); if (v >= 1) chunk = std::min<size_t>(std::min<size_t>((size_t)v, (size_t)n), 65535); }
    Carve cv;
    const size_t o_pose = cv.take((size_t)n * 64), o_rec = cv.take((size_t)n * sizeof(stocs_scene_record)), o_z = cv.take(chunk * npix * 4);
    const size_t o_side = fill.side_bytes ? cv.take(chunk * fill.side_bytes) : 0;
    { const int rc = work->grow(c->stream, cv.total); if (rc) return rc; }
    char* h_in; char* h_back;
    { const int rc = pinned_for(c, (size_t)n * 64, al256((size_t)n * sizeof(stocs_scene_record)), &h_in, &h_back); if (rc) return rc; }
    float* d_pose = Carve::at<float>(work->p, o_pose);
    stocs_scene_record* d_rec = Carve::at<stocs_scene_record>(work->p, o_rec);
    uint32_t* d_z = Carve::at<uint32_t>(work->p, o_z);
    memcpy(h_in, poses, (size_t)n * 64);
    STOCS_HIP_CHECK(hipMemcpyAsync(d_pose, h_in, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(d_rec, 0, (size_t)n * sizeof(stocs_scene_record), c->stream));
    const DepthArgs a = frame_args(F, tolerance, class_threshold);
    const unsigned run_blocks = (unsigned)(((size_t)(Wr / 2) + 4 * SCENE_RUNS_PER_WAVE - 1) / (4 * SCENE_RUNS_PER_WAVE));
    uint32_t* rows = (uint32_t*)d_rows + (size_t)slot_base * (size_t)Wr;
    for (int h0 = 0; h0 < n; h0 += (int)chunk) {
        const int m = std::min((int)chunk, n - h0);
        STOCS_HIP_CHECK(hipMemsetAsync(d_z, 0xFF, (size_t)m * npix * 4, c->stream));
        { const int rc = fill.fill(c, fill.self, (const float*)d_pose + (size_t)h0 * 16, m, a, d_z, work->p + o_side); if (rc) return rc; }
        hipLaunchKernelGGL(scene_classify_kernel, dim3(run_blocks, (unsigned)m), dim3(256), 0, c->stream, (const uint32_t*)d_z, frame_depth(F), frame_prob(F), a, (int)npix,
                           Wr, claim, rows + (size_t)h0 * (size_t)Wr, d_rec + h0);
        STOCS_HIP_CHECK(hipGetLastError());
    }
    STOCS_HIP_CHECK(hipMemcpyAsync(h_back, d_rec, (size_t)n * sizeof(stocs_scene_record), hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));   // another context may continue on the pool
    memcpy(out, h_back, (size_t)n * sizeof(stocs_scene_record));
    return STOCS_OK;
}

extern "C" int stocs_scene_select(stocs_ctx* c, const void* d_rows, int n, int width, int height, const float* score, const int32_t* group, const stocs_scene_record* rec,
                                  int n_groups, const int32_t* group_cap, const stocs_scene_params* prm, stocs_scene_result* out, int32_t* selected, int* n_selected) {
    static const char* who = "stocs_scene_select";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n > SCENE_MAX_N) { set_error("%s: %d slots, at most %d", who, n, (int)SCENE_MAX_N); return STOCS_ERR_INVALID; }
    if (!prm || !n_selected || (n > 0 && (!d_rows || !score || !group || !rec || !out || !selected))) {
        set_error("%s: NULL rows, scores, groups, records, parameters, results, selection or count", who);
        return STOCS_ERR_INVALID;
    }
    if (width < 1 || height < 1) { set_error("%s: a frame of %d x %d pixels", who, width, height); return STOCS_ERR_INVALID; }
    if (n_groups < 1 || n_groups > SCENE_MAX_GROUPS) { set_error("%s: %d groups, 1 .. %d", who, n_groups, (int)SCENE_MAX_GROUPS); return STOCS_ERR_INVALID; }
    { const int rc = check_params(who, prm); if (rc) return rc; }
    if (group_cap)
        for (int g = 0; g < n_groups; ++g)
            if (group_cap[g] < 1) { set_error("%s: group_cap[%d] = %d < 1", who, g, group_cap[g]); return STOCS_ERR_INVALID; }
    for (int h = 0; h < n; ++h) {   // never left to the kernels
        if (group[h] < 0 || group[h] >= n_groups) { set_error("%s: group[%d] = %d is outside [0, %d)", who, h, group[h], n_groups); return STOCS_ERR_INVALID; }
        const stocs_scene_record& r = rec[h];
        if (r.footprint < 0 || r.no_depth < 0 || r.agree < 0 || r.in_front < 0 || r.behind < 0 || r.on_mask < 0 || r.claimed < 0) {
            set_error("%s: rec[%d] has a negative count", who, h);
            return STOCS_ERR_INVALID;
        }
    }
    const size_t npix = (size_t)width * (size_t)height;
    { const int rc = scene_check_pixels(who, npix); if (rc) return rc; }
    *n_selected = 0;
    if (n == 0) return STOCS_OK;
    DeviceGuard dev_guard(c->device);
    SceneState* S = ctx_state<SceneState>(c);
    const int Wr = row_words(npix);
    SceneArgs a;
    a.max_selected = prm->max_selected < n ? prm->max_selected : n;   // no more can be selected than there are
    a.min_pixels = prm->min_pixels; a.min_fraction = prm->min_exclusive_fraction; a.max_violation = prm->max_violation_fraction;
    // what goes up is one region (score | group | in_front | footprint | caps), what comes back another (results | selected | count)
    Carve in;
    const size_t i_score = in.take((size_t)n * 4), i_group = in.take((size_t)n * 4), i_front = in.take((size_t)n * 4), i_foot = in.take((size_t)n * 4),
                 i_cap = in.take((size_t)n_groups * 4);
    CoverBack bk;
    { const int rc = bk.plan(c, n, sizeof(stocs_scene_result), a.max_selected); if (rc) return rc; }
    Carve cv;
    const size_t o_in = cv.take(in.total), o_own = cv.take((size_t)n * 4), o_elig = cv.take((size_t)n), o_key = cv.take((size_t)n * 8), o_key_s = cv.take((size_t)n * 8),
                 o_idx = cv.take((size_t)n * 4), o_idx_s = cv.take((size_t)n * 4), o_rank = cv.take((size_t)n * 4), o_excl = cv.take((size_t)n * 4),
                 o_cover = cv.take((size_t)Wr * 4), o_cnt = cv.take((size_t)n_groups * 4), o_back = cv.take(bk.total), o_sort = cv.take(bk.sort_bytes);
    { const int rc = S->sel.grow(c->stream, cv.total); if (rc) return rc; }
    char* h_in; char* h_back;
    { const int rc = pinned_for(c, in.total, bk.total, &h_in, &h_back); if (rc) return rc; }
    memcpy(h_in + i_score, score, (size_t)n * 4);
    memcpy(h_in + i_group, group, (size_t)n * 4);
    for (int h = 0; h < n; ++h) { ((int32_t*)(h_in + i_front))[h] = rec[h].in_front; ((int32_t*)(h_in + i_foot))[h] = rec[h].footprint; }
    for (int g = 0; g < n_groups; ++g) ((int32_t*)(h_in + i_cap))[g] = group_cap ? group_cap[g] : 0x7FFFFFFF;   // no cap: never full
    char* b = S->sel.p;
    char* d_in = b + o_in;
    STOCS_HIP_CHECK(hipMemcpyAsync(d_in, h_in, in.total, hipMemcpyHostToDevice, c->stream));
    const uint32_t* rows = (const uint32_t*)d_rows;
    const int32_t* d_group = Carve::at<int32_t>(d_in, i_group);
    const int32_t* d_cap = Carve::at<int32_t>(d_in, i_cap);
    int32_t* d_own = Carve::at<int32_t>(b, o_own);
    uint8_t* d_elig = Carve::at<uint8_t>(b, o_elig);
    uint32_t* d_idx_s = Carve::at<uint32_t>(b, o_idx_s);
    int32_t* d_rank = Carve::at<int32_t>(b, o_rank);
    int32_t* d_excl = Carve::at<int32_t>(b, o_excl);
    uint32_t* d_cover = Carve::at<uint32_t>(b, o_cover);
    int32_t* d_cnt = Carve::at<int32_t>(b, o_cnt);
    char* d_back = b + o_back;
    hipLaunchKernelGGL(scene_own_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, rows, Wr, n, Carve::at<float>(d_in, i_score), Carve::at<int32_t>(d_in, i_front),
                       Carve::at<int32_t>(d_in, i_foot), a, d_own, d_elig, Carve::at<uint64_t>(b, o_key), Carve::at<uint32_t>(b, o_idx));
    STOCS_HIP_CHECK(hipGetLastError());
    { const int rc = bk.order(c, b + o_sort, Carve::at<uint64_t>(b, o_key), Carve::at<uint64_t>(b, o_key_s), Carve::at<uint32_t>(b, o_idx), d_idx_s, n); if (rc) return rc; }
    const size_t lds = (size_t)Wr * 4 + (size_t)n_groups * 4 + 4 * COVER_WAVES * 4;
    // beyond 64 KB a kernel has to be told; the kernel's ceiling, not this launch's size: contexts on other threads launch the same kernel
    if (lds > 64 * 1024) STOCS_HIP_CHECK(hipFuncSetAttribute((const void*)scene_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SCENE_SELECT_MAX_LDS));
    hipLaunchKernelGGL(scene_select_kernel, dim3(1), dim3(64 * COVER_WAVES), lds, c->stream, rows, Wr, (const uint32_t*)d_idx_s, (const int32_t*)d_own,
                       (const uint8_t*)d_elig, d_group, d_cap, n, n_groups, a, d_rank, d_excl, Carve::at<int32_t>(d_back, bk.o_sel), Carve::at<int32_t>(d_back, bk.o_cnt), d_cover,
                       d_cnt);
    STOCS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(scene_finish_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, rows, Wr, (const uint32_t*)d_cover, (const int32_t*)d_own,
                       (const uint8_t*)d_elig, d_group, d_cap, (const int32_t*)d_cnt, (const int32_t*)d_rank, (const int32_t*)d_excl, n, a,
                       Carve::at<stocs_scene_result>(d_back, bk.o_rec));
    STOCS_HIP_CHECK(hipGetLastError());
    return bk.read_back(c, d_back, h_back, out, selected, n_selected);
}
