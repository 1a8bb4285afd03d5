// instances.hip -- multi-instance selection of pose hypotheses (stocs_select_instances, stocs_select_instances_rows): walk the
// hypotheses best first and keep one only if enough of the scene points it explains are not explained by one kept before it.  No
// reference counterpart (the reference returns one pose per object); the contract is written down at the declaration in
// include/stocs_hip.h and restated in numpy in tests/instances_ref.py.  Integer set logic over the match records of the scoring
// kernel's detail form: every result is held bit for bit.
//
// Per call, everything on the context's stream, one pinned read-back, ONE synchronisation:
//   rows      launch_lcp's detail form (hit, counted, lcp) for chunks of hypotheses, as stocs_lcp_hit_count chunks them (256 MB of rows;
//             STOCS_INSTANCES_CHUNK=<candidates> forces a size).  The rows form uploads the caller's rows instead.
//   mark      instance_mark_kernel, a workgroup of 256 threads per hypothesis of the chunk: the explained set E_h as a bitset of W =
//             ceil(nS / 32) words in LDS (atomicOr per counted model point), stored as a row of Wp = W rounded up to four words
//             (zero padded, so that the later kernels read rows as 16-byte words); own_h = its popcount; the sort key of step 3.
//   order     one 64-bit radix sort (prims.h) of the complemented keys with the indices as values: ascending and stable, hence
//             descending stocs_pack_best and, among the hypotheses that share the key 0, ascending index.
//   select    instance_select_kernel, ONE workgroup of 16 wavefronts with `covered` in LDS: the walk of cover_walk.h, which scene.hip
//             shares, behind this file's gate (own_h >= min_points).
//   finish    instance_finish_kernel, a wavefront per hypothesis: |E_h \ covered_final| for the unselected ones, and the records.
// The order key, the exclusive count, the ordering sort and the read-back region (records | selected | count) are cover_walk.h's too; the
// pinned staging is pinned_for (stocs_ctx.h).
// Known limits: nS <= 2^18 (a 32 KB bitset), n <= 16 384; the walk is one workgroup, so its time grows with rounds x W.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "cover_walk.h"

namespace stocs {

enum { INST_MAX_SCENE = 1 << 18, INST_MAX_N = 16384 };

struct InstancesState {
    static const StateOwner OWNER = OWN_INSTANCES;
    ~InstancesState() { rows.free(); work.free(); }
    DevBlock rows;   // one chunk of detail rows: lcp | hit | counted
    DevBlock work;   // poses | valid | lcp | own | keys (2) | indices (2) | rank | excl | cover | records + selected + count | sort scratch | E
};

// hypothesis h0 + blockIdx.x from row blockIdx.x of the chunk.  valid == NULL: every hypothesis is valid.  LDS: Wp words + 4.
__global__ __launch_bounds__(256) void instance_mark_kernel(const int32_t* __restrict__ hit, const uint8_t* __restrict__ counted, const float* __restrict__ lcp_chunk,
                                                            const uint8_t* __restrict__ valid, int nM, int nS, int Wp, int h0, uint32_t* __restrict__ E,
                                                            int32_t* __restrict__ own, float* __restrict__ lcp_out, uint64_t* __restrict__ key, uint32_t* __restrict__ idx) {
    extern __shared__ __attribute__((aligned(16))) uint32_t mark_lds[];
    uint32_t* bits = mark_lds;
    int* total = (int*)(mark_lds + Wp);
    const int tid = (int)threadIdx.x;
    const int h = h0 + (int)blockIdx.x;
    const bool ok = valid ? valid[h] != 0 : true;   // the same in every thread of the workgroup
    for (int w = tid; w < Wp; w += 256) bits[w] = 0u;
    if (tid == 0) *total = 0;
    __syncthreads();
    if (ok) {
        const int32_t* hr = hit + (size_t)blockIdx.x * (size_t)nM;
        const uint8_t* cr = counted + (size_t)blockIdx.x * (size_t)nM;
        for (int i = tid; i < nM; i += 256) {
            const int32_t s = hr[i];
            if (cr[i] != 0 && (uint32_t)s < (uint32_t)nS) atomicOr(&bits[s >> 5], 1u << (s & 31));
        }
    }
    __syncthreads();
    uint32_t* row = E + (size_t)h * (size_t)Wp;
    int cnt = 0;
    for (int w = tid; w < Wp; w += 256) { const uint32_t v = bits[w]; row[w] = v; cnt += __popc(v); }
    cnt = wave_sum_i(cnt);
    if ((tid & 63) == 0 && cnt) atomicAdd(total, cnt);
    __syncthreads();
    if (tid == 0) {
        const float l = ok ? lcp_chunk[blockIdx.x] : 0.0f;
        own[h] = *total;
        lcp_out[h] = l;
        key[h] = cover_order_key(l, h);   // step 3 of the contract
        idx[h] = (uint32_t)h;
    }
}

// the gate of this walk: excl <= own, so below min_points the row need not be read.  A selection has no side effect
struct InstanceGate {
    const int32_t* __restrict__ own; int min_points;
    __device__ __forceinline__ bool open(int h) const { return own[h] >= min_points; }
    __device__ __forceinline__ void took(int, int) const {}
};

// the walk (step 4): cover_walk (cover_walk.h) by one workgroup.  LDS: Wp words of cover, then 3 x 16 words of the round's results.
__global__ __launch_bounds__(64 * COVER_WAVES) void instance_select_kernel(const uint32_t* __restrict__ E, int Wp, const uint32_t* __restrict__ order,
                                                                           const int32_t* __restrict__ own, int n, CoverArgs a, int32_t* __restrict__ rank,
                                                                           int32_t* __restrict__ excl, int32_t* __restrict__ selected, int32_t* __restrict__ n_selected,
                                                                           uint32_t* __restrict__ cover_out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sel_lds[];
    const InstanceGate gate = {own, a.min_count};
    cover_walk(E, Wp, order, own, n, a, gate, (uint4*)sel_lds, (int*)(sel_lds + Wp), rank, excl, selected, n_selected, cover_out);
}

// step 5: a wavefront per hypothesis, four to a workgroup
__global__ __launch_bounds__(256) void instance_finish_kernel(const uint32_t* __restrict__ E, int Wp, const uint32_t* __restrict__ cover, const int32_t* __restrict__ own,
                                                              const float* __restrict__ lcp, const int32_t* __restrict__ rank, const int32_t* __restrict__ excl, int n,
                                                              stocs_instance_result* __restrict__ out) {
    const int lane = (int)threadIdx.x & 63;
    const int h = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (h >= n) return;   // wave-uniform
    const int r = rank[h];
    const int ex = cover_final_exclusive(E, Wp, cover, excl, h, r, lane);
    if (lane == 0) {
        stocs_instance_result o;
        o.rank = r; o.own = own[h]; o.exclusive = ex; o.lcp = lcp[h];
        out[h] = o;
    }
}


static int check_params(const char* who, const stocs_instance_params* p) {
    if (p->max_instances < 1) { set_error("%s: max_instances %d < 1", who, p->max_instances); return STOCS_ERR_INVALID; }
    if (p->min_points < 1) { set_error("%s: min_points %d < 1", who, p->min_points); return STOCS_ERR_INVALID; }
    if (!(p->min_exclusive_fraction > 0.0f) || !(p->min_exclusive_fraction <= 1.0f)) {
        set_error("%s: min_exclusive_fraction %g is not in (0, 1]", who, (double)p->min_exclusive_fraction);
        return STOCS_ERR_INVALID;
    }
    return STOCS_OK;
}

static int check_count(const char* who, int n) {
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n > INST_MAX_N) { set_error("%s: %d hypotheses, at most %d", who, n, (int)INST_MAX_N); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}

static int check_scene_size(const char* who, int nS) {
    if (nS > INST_MAX_SCENE) { set_error("%s: a scene of %d points, at most %d (the explained sets are 32 KB bitsets in LDS)", who, nS, (int)INST_MAX_SCENE); return STOCS_ERR_CAPACITY; }
    return STOCS_OK;
}

// the device arrays of one call, carved from InstancesState::work; the read-back is one region, laid out by `bk`
struct InstancesWork {
    float* pose; uint8_t* valid; float* lcp; int32_t* own; uint64_t* key; uint64_t* key_s; uint32_t* idx; uint32_t* idx_s; int32_t* rank; int32_t* excl;
    uint32_t* cover; char* back; void* sort_tmp; uint32_t* E;
    size_t o_pose, o_valid;
    CoverBack bk;
    int Wp, max_sel;
};

static int carve_work(stocs_ctx* c, InstancesState* S, int n, int nS, const stocs_instance_params* prm, InstancesWork* w) {
    const int W = (nS + 31) / 32;
    w->Wp = (W + 3) & ~3;
    w->max_sel = prm->max_instances < n ? prm->max_instances : n;   // no more can be selected than there are
    { const int rc = w->bk.plan(c, n, sizeof(stocs_instance_result), w->max_sel); if (rc) return rc; }
    Carve cv;
    w->o_pose = cv.take((size_t)n * 64);
    w->o_valid = cv.take((size_t)n);
    const size_t o_lcp = cv.take((size_t)n * 4), o_own = cv.take((size_t)n * 4), o_key = cv.take((size_t)n * 8), o_key_s = cv.take((size_t)n * 8);
    const size_t o_idx = cv.take((size_t)n * 4), o_idx_s = cv.take((size_t)n * 4), o_rank = cv.take((size_t)n * 4), o_excl = cv.take((size_t)n * 4);
    const size_t o_cover = cv.take((size_t)w->Wp * 4);
    const size_t o_back = cv.take(w->bk.total), o_sort = cv.take(w->bk.sort_bytes);
    const size_t o_E = cv.take((size_t)n * (size_t)w->Wp * 4);
    { const int rc = S->work.grow(c->stream, cv.total); if (rc) return rc; }
    char* b = S->work.p;
    w->pose = Carve::at<float>(b, w->o_pose); w->valid = Carve::at<uint8_t>(b, w->o_valid); w->lcp = Carve::at<float>(b, o_lcp); w->own = Carve::at<int32_t>(b, o_own);
    w->key = Carve::at<uint64_t>(b, o_key); w->key_s = Carve::at<uint64_t>(b, o_key_s); w->idx = Carve::at<uint32_t>(b, o_idx); w->idx_s = Carve::at<uint32_t>(b, o_idx_s);
    w->rank = Carve::at<int32_t>(b, o_rank); w->excl = Carve::at<int32_t>(b, o_excl); w->cover = Carve::at<uint32_t>(b, o_cover);
    w->back = b + o_back; w->sort_tmp = b + o_sort; w->E = Carve::at<uint32_t>(b, o_E);
    return STOCS_OK;
}

// marks rows [h0, h0 + m) from the chunk's detail rows
static int enqueue_mark(stocs_ctx* c, const InstancesWork& w, const int32_t* d_hit, const uint8_t* d_counted, const float* d_lcp, const uint8_t* d_valid, int nM, int nS, int h0, int m) {
    hipLaunchKernelGGL(instance_mark_kernel, dim3((unsigned)m), dim3(256), (size_t)(w.Wp + 4) * 4, c->stream, d_hit, d_counted, d_lcp, d_valid, nM, nS, w.Wp, h0, w.E, w.own,
                       w.lcp, w.key, w.idx);
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

// order, walk, records, then CoverBack::read_back: the pinned mirror of `back`, the call's one synchronisation, results to the caller
static int order_select_finish(stocs_ctx* c, const InstancesWork& w, int n, const stocs_instance_params* prm, char* h_back, stocs_instance_result* out, int32_t* selected,
                               int* n_selected) {
    { const int rc = w.bk.order(c, w.sort_tmp, w.key, w.key_s, w.idx, w.idx_s, n); if (rc) return rc; }
    const CoverArgs a = {w.max_sel, prm->min_points, prm->min_exclusive_fraction};
    hipLaunchKernelGGL(instance_select_kernel, dim3(1), dim3(64 * COVER_WAVES), (size_t)(w.Wp + 3 * COVER_WAVES) * 4, c->stream, (const uint32_t*)w.E, w.Wp,
                       (const uint32_t*)w.idx_s, (const int32_t*)w.own, n, a, w.rank, w.excl, Carve::at<int32_t>(w.back, w.bk.o_sel), Carve::at<int32_t>(w.back, w.bk.o_cnt),
                       w.cover);
    STOCS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(instance_finish_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, (const uint32_t*)w.E, w.Wp, (const uint32_t*)w.cover,
                       (const int32_t*)w.own, (const float*)w.lcp, (const int32_t*)w.rank, (const int32_t*)w.excl, n, Carve::at<stocs_instance_result>(w.back, w.bk.o_rec));
    STOCS_HIP_CHECK(hipGetLastError());
    return w.bk.read_back(c, w.back, h_back, out, selected, n_selected);
}

}  // namespace stocs

using namespace stocs;

extern "C" void stocs_default_instance_params(stocs_instance_params* p) {
    if (!p) return;
    p->max_instances = 16; p->min_points = 20; p->min_exclusive_fraction = 0.5f;
}

extern "C" int stocs_select_instances(stocs_ctx* c, const float* T16, int n, const stocs_instance_params* prm, stocs_instance_result* out, int32_t* selected,
                                      int* n_selected) {
    static const char* who = "stocs_select_instances";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    { const int rc = check_count(who, n); if (rc) return rc; }
    if (!prm || !n_selected || (n > 0 && (!T16 || !out || !selected))) { set_error("%s: NULL hypotheses, parameters, records, selection or count", who); return STOCS_ERR_INVALID; }
    { const int rc = check_params(who, prm); if (rc) return rc; }
    if (c->nS <= 0 || c->nM <= 0) { set_error("%s: the context has no scene or no model", who); return STOCS_ERR_STATE; }
    { const int rc = check_scene_size(who, c->nS); if (rc) return rc; }
    *n_selected = 0;
    if (n == 0) return STOCS_OK;
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    InstancesState* S = ctx_state<InstancesState>(c);
    const size_t M = (size_t)c->nM;
    size_t chunk = std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)256 << 20) / (5 * M)));
    if (const char* e = getenv("STOCS_INSTANCES_CHUNK")) { const long v = atol(e); if (v >= 1) chunk = std::min<size_t>((size_t)v, (size_t)n); }
    Carve rv;
    const size_t o_l = rv.take(chunk * 4), o_h = rv.take(chunk * M * 4), o_c = rv.take(chunk * M);
    { const int rc = S->rows.grow(c->stream, rv.total); if (rc) return rc; }
    InstancesWork w;
    { const int rc = carve_work(c, S, n, c->nS, prm, &w); if (rc) return rc; }
    char* h_in; char* h_back;
    const size_t in_bytes = al256((size_t)n * 64) + al256((size_t)n);
    { const int rc = pinned_for(c, in_bytes, w.bk.total, &h_in, &h_back); if (rc) return rc; }
    // step 2: a hypothesis with a non-finite entry, or all zeros, is not scored as a transform -- the launch gets the identity in its
    // place (a pose like any other to the kernel) and the marking kernel zeroes its record
    float* h_pose = (float*)h_in;
    uint8_t* h_valid = (uint8_t*)(h_in + al256((size_t)n * 64));
    memcpy(h_pose, T16, (size_t)n * 64);
    for (int h = 0; h < n; ++h) {
        float* T = h_pose + (size_t)h * 16;
        bool finite = true, zero = true;
        for (int k = 0; k < 16; ++k) { finite = finite && isfinite(T[k]); zero = zero && T[k] == 0.0f; }
        h_valid[h] = (finite && !zero) ? 1 : 0;
        if (!h_valid[h]) for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0f : 0.0f;
    }
    STOCS_HIP_CHECK(hipMemcpyAsync(w.pose, h_pose, in_bytes, hipMemcpyHostToDevice, c->stream));   // poses and flags: neighbours in both blocks
    float* dL = Carve::at<float>(S->rows.p, o_l);
    int32_t* dH = Carve::at<int32_t>(S->rows.p, o_h);
    uint8_t* dC = Carve::at<uint8_t>(S->rows.p, o_c);
    for (int h0 = 0; h0 < n; h0 += (int)chunk) {
        const int m = std::min((int)chunk, n - h0);
        int rc = launch_lcp(c, w.pose + (size_t)h0 * 16, m, dL, dH, dC, NULL, 0);
        if (rc) return rc;
        if ((rc = enqueue_mark(c, w, dH, dC, dL, w.valid, c->nM, c->nS, h0, m))) return rc;
    }
    return order_select_finish(c, w, n, prm, h_back, out, selected, n_selected);
}

extern "C" int stocs_select_instances_rows(stocs_ctx* c, const int32_t* hit, const uint8_t* counted, const float* lcp, int n, int nM, int nS,
                                           const stocs_instance_params* prm, stocs_instance_result* out, int32_t* selected, int* n_selected) {
    static const char* who = "stocs_select_instances_rows";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    { const int rc = check_count(who, n); if (rc) return rc; }
    if (nM < 1 || nS < 1) { set_error("%s: nM %d < 1 or nS %d < 1", who, nM, nS); return STOCS_ERR_INVALID; }
    if (!prm || !n_selected || (n > 0 && (!hit || !counted || !lcp || !out || !selected))) { set_error("%s: NULL rows, parameters, records, selection or count", who); return STOCS_ERR_INVALID; }
    { const int rc = check_params(who, prm); if (rc) return rc; }
    { const int rc = check_scene_size(who, nS); if (rc) return rc; }
    const size_t cells = (size_t)n * (size_t)nM;
    for (size_t i = 0; i < cells; ++i)   // never left to the kernel
        if (counted[i] && (hit[i] < 0 || hit[i] >= nS)) {
            set_error("%s: hit[%zu] = %d on a counted row is outside [0, %d)", who, i, hit[i], nS);
            return STOCS_ERR_INVALID;
        }
    *n_selected = 0;
    if (n == 0) return STOCS_OK;
    DeviceGuard dev_guard(c->device);
    InstancesState* S = ctx_state<InstancesState>(c);
    Carve rv;
    const size_t o_l = rv.take((size_t)n * 4), o_h = rv.take(cells * 4), o_c = rv.take(cells);
    { const int rc = S->rows.grow(c->stream, rv.total); if (rc) return rc; }
    InstancesWork w;
    { const int rc = carve_work(c, S, n, nS, prm, &w); if (rc) return rc; }
    char* h_in; char* h_back;
    { const int rc = pinned_for(c, 0, w.bk.total, &h_in, &h_back); if (rc) return rc; }
    float* dL = Carve::at<float>(S->rows.p, o_l);
    int32_t* dH = Carve::at<int32_t>(S->rows.p, o_h);
    uint8_t* dC = Carve::at<uint8_t>(S->rows.p, o_c);
    // a test and diagnosis facility: pageable copies, as stocs_cluster_trials_device
    STOCS_HIP_CHECK(hipMemcpyAsync(dL, lcp, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemcpyAsync(dH, hit, cells * 4, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemcpyAsync(dC, counted, cells, hipMemcpyHostToDevice, c->stream));
    { const int rc = enqueue_mark(c, w, dH, dC, dL, NULL, nM, nS, 0, n); if (rc) return rc; }
    return order_select_finish(c, w, n, prm, h_back, out, selected, n_selected);
}
