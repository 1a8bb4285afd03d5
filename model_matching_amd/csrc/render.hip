// render.hip -- joint rendering of pose hypotheses into one frame-sized key buffer (stocs_render_poses, stocs_render_resolve,
// stocs_render_labels, stocs_explain_poses): which pixels each instance owns, how much of it the others hide, and whether the depth
// image agrees with the poses taken together.  No reference counterpart.  The contract (splat rule, keys, classes, errors) is written
// down at the declarations in include/stocs_hip.h; tests/render_ref.py restates it in float32 numpy and the results are equal bit
// for bit: keys are packed integers under a minimum, counts are integer sums.
//
//   render_splat_kernel    one workgroup of 256 threads per (hypothesis, chunk of RENDER_CHUNK model points): every point goes through
//                          project_point (depth_frame.h, the depth check's steps 1-3); a point in the image walks its splat square
//                          (splat_square, render_rules.h: (2s+1)^2 pixels clamped to the image) with one 64-bit atomicMin on the key
//                          buffer per pixel.
//   render_resolve_kernel  one workgroup per hypothesis: its footprint as a bitset of ceil(W*H/32) words in dynamic LDS (the model is
//                          projected again, the same splat_square setting bits with atomicOr), then the pixels of the rows it touched
//                          are walked one thread per pixel: a set bit costs one key load and the classification of the depth check's
//                          steps 5-6 with the key's z.
//                          Every count is a __ballot + __popcll per wavefront in wave-uniform registers; thread 0 stores the record.
//   render_labels_kernel   one thread per pixel: label and state of the key.
// The clear is a hipMemsetAsync with 0xFF.  The call layout, the pose upload, the clear, the labels launch and the read-back are declared in
// render_shared.h: render_mesh.hip, the same entry points on a triangle mesh, runs through them too.  Known limits: a point's splat is walked by the one lane that projected it (up to 33 x 33
// pixels); resolve is one workgroup per hypothesis, latency-bound for a few hypotheses, and holds the whole frame's bitset (2^19 pixels).
#include <math.h>
#include <string.h>

#include "render_shared.h"
#include "wave_bits.h"

namespace stocs {

enum { RENDER_CHUNK = 1024, RENDER_MAX_PIXELS = 1 << 19 };
enum { RC_FOOTPRINT = 0, RC_HIDDEN, RC_NO_DEPTH, RC_AGREE, RC_IN_FRONT, RC_BEHIND, RC_ON_MASK, RC_COUNTS };

struct RenderState {
    static const StateOwner OWNER = OWN_RENDER;
    ~RenderState() { work.free(); }
    DevBlock work;   // own key buffer (npix uint64, stocs_explain_poses) | poses (n x 16 float) | records | labels | state, grow-only
};

__global__ __launch_bounds__(256) void render_splat_kernel(const float* __restrict__ poses, const float4* __restrict__ mpos, const float4* __restrict__ mnrm, int nM,
                                                           DepthArgs a, RenderArgs ra, unsigned long long* __restrict__ zkey) {
    const int h = (int)blockIdx.y;
    float P[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = poses[(size_t)h * 16 + i];   // the same address in every lane: uniform loads
    if (!pose_finite(P)) return;
    const unsigned long long id = (unsigned long long)(unsigned)(ra.id_base + h);
    const int first = (int)blockIdx.x * RENDER_CHUNK;
    const int last = first + RENDER_CHUNK < nM ? first + RENDER_CHUNK : nM;
    for (int i = first + (int)threadIdx.x; i < last; i += 256) {
        const Projected p = project_point(P, mpos[i], mnrm[i], a);
        if (!p.in_image) continue;
        const unsigned long long key = ((unsigned long long)__float_as_uint(p.z) << 32) | id;
        splat_square(p, a, ra, [&](int r, int c) { atomicMin(&zkey[(size_t)r * (size_t)a.W + (size_t)c], key); });
    }
}

// dynamic LDS: ceil(W*H/32) words, the footprint bitset (bit px & 31 of word px >> 5, px = row * W + col)
__global__ __launch_bounds__(256) void render_resolve_kernel(const float* __restrict__ poses, const float4* __restrict__ mpos, const float4* __restrict__ mnrm, int nM,
                                                             const uint16_t* __restrict__ depth, const uint16_t* __restrict__ prob, DepthArgs a, RenderArgs ra,
                                                             const unsigned long long* __restrict__ zkey, stocs_render_result* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t foot[];
    __shared__ int rows[2];             // first and last row touched
    __shared__ int cnt[RC_COUNTS];
    const int tid = (int)threadIdx.x;
    const int h = (int)blockIdx.x;
    float P[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = poses[(size_t)h * 16 + i];   // the same address in every lane: uniform loads
    if (!pose_finite(P)) {   // a zero record (wave-uniform exit: P is the same in every lane)
        if (tid == 0) {
            stocs_render_result r;
            r.footprint = r.visible = r.hidden = r.no_depth = r.agree = r.in_front = r.behind = r.on_mask = 0;
            out[h] = r;
        }
        return;
    }
    const int npix = a.W * a.H;
    const int nwords = (npix + 31) >> 5;
    for (int i = tid; i < nwords; i += 256) foot[i] = 0u;
    if (tid < RC_COUNTS) cnt[tid] = 0;
    if (tid == 0) { rows[0] = 0x7FFFFFFF; rows[1] = -1; }
    __syncthreads();
    // the footprint: the splat kernel's walk, setting bits
    int mnr = 0x7FFFFFFF, mxr = -1;
    for (int i = tid; i < nM; i += 256) {
        const Projected p = project_point(P, mpos[i], mnrm[i], a);
        if (!p.in_image) continue;
        const int2 rr = splat_square(p, a, ra, [&](int r, int c) {
            const int px = r * a.W + c;
            atomicOr(&foot[px >> 5], 1u << (px & 31));
        });
        mnr = rr.x < mnr ? rr.x : mnr; mxr = rr.y > mxr ? rr.y : mxr;
    }
    mnr = wave_min_i(mnr); mxr = wave_max_i(mxr);
    if ((tid & 63) == 0) { atomicMin(&rows[0], mnr); atomicMax(&rows[1], mxr); }
    __syncthreads();
    // the walk: the pixels of the touched rows, one thread per pixel; the loop bounds are wave-uniform, so every __ballot sees the whole wavefront
    const int px0 = rows[1] >= rows[0] ? rows[0] * a.W : 0;
    const int px1 = rows[1] >= rows[0] ? (rows[1] + 1) * a.W : 0;
    const uint32_t id = (uint32_t)(ra.id_base + h);
    int n_foot = 0, n_hidden = 0, n_nod = 0, n_agree = 0, n_front = 0, n_behind = 0, n_mask = 0;
    for (int base = px0; base < px1; base += 256) {
        const int px = base + tid;
        bool set = false, hidden = false;
        int cls = 0;
        if (px < px1) {
            set = (foot[px >> 5] >> (px & 31)) & 1u;
            if (set) {
                const unsigned long long key = zkey[px];
                hidden = (uint32_t)key != id;   // an empty key's low word is all ones, which no id is
                if (!hidden) cls = classify_pixel(__uint_as_float((uint32_t)(key >> 32)), (size_t)px, depth, prob, a);
            }
        }
        n_foot += __popcll(__ballot(set)); n_hidden += __popcll(__ballot(hidden));
        n_nod += __popcll(__ballot((cls & 15) == 1)); n_agree += __popcll(__ballot((cls & 15) == 2)); n_front += __popcll(__ballot((cls & 15) == 3));
        n_behind += __popcll(__ballot((cls & 15) == 4)); n_mask += __popcll(__ballot((cls & 16) != 0));
    }
    if ((tid & 63) == 0) {
        atomicAdd(&cnt[RC_FOOTPRINT], n_foot); atomicAdd(&cnt[RC_HIDDEN], n_hidden); atomicAdd(&cnt[RC_NO_DEPTH], n_nod); atomicAdd(&cnt[RC_AGREE], n_agree);
        atomicAdd(&cnt[RC_IN_FRONT], n_front); atomicAdd(&cnt[RC_BEHIND], n_behind); atomicAdd(&cnt[RC_ON_MASK], n_mask);
    }
    __syncthreads();
    if (tid == 0) {
        stocs_render_result r;
        r.footprint = cnt[RC_FOOTPRINT]; r.hidden = cnt[RC_HIDDEN]; r.visible = r.footprint - r.hidden;
        r.no_depth = cnt[RC_NO_DEPTH]; r.agree = cnt[RC_AGREE]; r.in_front = cnt[RC_IN_FRONT]; r.behind = cnt[RC_BEHIND]; r.on_mask = cnt[RC_ON_MASK];
        out[h] = r;
    }
}

__global__ __launch_bounds__(256) void render_labels_kernel(const unsigned long long* __restrict__ zkey, const uint16_t* __restrict__ depth,
                                                            const uint16_t* __restrict__ prob, DepthArgs a, size_t npix, int32_t* __restrict__ labels,
                                                            uint8_t* __restrict__ state) {
    const size_t px = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (px >= npix) return;
    const unsigned long long key = zkey[px];
    const bool empty = key == ~0ull;
    labels[px] = empty ? -1 : (int32_t)(uint32_t)key;
    state[px] = empty ? (uint8_t)0 : (uint8_t)classify_pixel(__uint_as_float((uint32_t)(key >> 32)), px, depth, prob, a);
}


int render_check_ids(const char* who, int n, int id_base) {
    if (id_base < 0 || (long long)id_base + (long long)n > 2147483647ll) {
        set_error("%s: ids %d .. %lld outside 0 .. 2^31 - 2", who, id_base, (long long)id_base + (long long)n - 1);
        return STOCS_ERR_INVALID;
    }
    return STOCS_OK;
}

static int check_capacity(const char* who, const DepthState* S) {
    if (S->npix > (size_t)RENDER_MAX_PIXELS) {
        set_error("%s: a frame of %zu pixels, at most %d (the footprint is a 64 KB bitset in LDS)", who, S->npix, (int)RENDER_MAX_PIXELS);
        return STOCS_ERR_CAPACITY;
    }
    return STOCS_OK;
}

// One call's layout (RenderLayout, render_shared.h) in the block `work` of the entry point
int render_layout(stocs_ctx* c, DevBlock* work, size_t own_key, int n, size_t label_px, size_t tail, RenderLayout* L) {
    Carve cv;
    L->key_bytes = al256(own_key * 8);
    L->o_pose = cv.take((size_t)n * 64); L->o_res = cv.take((size_t)n * sizeof(stocs_render_result));
    L->o_lab = cv.take(label_px * 4); L->o_state = cv.take(label_px);
    L->o_tail = cv.total;
    L->total = cv.total;
    { const int rc = work->grow(c->stream, L->key_bytes + cv.total + tail); if (rc) return rc; }
    { const int rc = pinned_var(c, cv.total, &L->h); if (rc) return rc; }
    L->d = work->p + L->key_bytes;
    return STOCS_OK;
}
static int render_layout(stocs_ctx* c, size_t own_key, int n, size_t label_px, RenderLayout* L) { return render_layout(c, &ctx_state<RenderState>(c)->work, own_key, n, label_px, 0, L); }

int render_upload_poses(stocs_ctx* c, const RenderLayout& L, const float* poses, int n) {
    memcpy(L.h + L.o_pose, poses, (size_t)n * 64);
    STOCS_HIP_CHECK(hipMemcpyAsync(L.d + L.o_pose, L.h + L.o_pose, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
    return STOCS_OK;
}

int render_enqueue_clear(stocs_ctx* c, const DepthState* S, void* d_zkey) {
    STOCS_HIP_CHECK(hipMemsetAsync(d_zkey, 0xFF, S->npix * 8, c->stream));
    return STOCS_OK;
}

static int enqueue_splat(stocs_ctx* c, const DepthState* S, const RenderLayout& L, int n, const stocs_render_params* prm, int id_base, void* d_zkey) {
    const unsigned chunks = (unsigned)((c->nM + RENDER_CHUNK - 1) / RENDER_CHUNK);
    if (chunks == 0) return STOCS_OK;
    // the hypothesis is blockIdx.y (at most 65 535 per launch)
    for (int h0 = 0; h0 < n; h0 += 65535) {
        const int nh = n - h0 < 65535 ? n - h0 : 65535;
        hipLaunchKernelGGL(render_splat_kernel, dim3(chunks, (unsigned)nh), dim3(256), 0, c->stream, (const float*)(L.d + L.o_pose) + (size_t)h0 * 16,
                           (const float4*)c->d_mpos_raw, (const float4*)c->d_mnrm, c->nM, frame_args(S, prm), render_args(prm, id_base + h0), (unsigned long long*)d_zkey);
        STOCS_HIP_CHECK(hipGetLastError());
    }
    return STOCS_OK;
}

static int enqueue_resolve(stocs_ctx* c, const DepthState* S, const RenderLayout& L, int n, const stocs_render_params* prm, int id_base, const void* d_zkey) {
    const size_t lds = ((S->npix + 31) / 32) * 4;
    hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)n), dim3(256), lds, c->stream, (const float*)(L.d + L.o_pose), (const float4*)c->d_mpos_raw,
                       (const float4*)c->d_mnrm, c->nM, frame_depth(S), frame_prob(S), frame_args(S, prm), render_args(prm, id_base),
                       (const unsigned long long*)d_zkey, (stocs_render_result*)(L.d + L.o_res));
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

int render_enqueue_labels(stocs_ctx* c, const DepthState* S, const RenderLayout& L, float tolerance, float class_threshold, const void* d_zkey) {
    hipLaunchKernelGGL(render_labels_kernel, dim3((unsigned)((S->npix + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long*)d_zkey, frame_depth(S),
                       frame_prob(S), frame_args(S, tolerance, class_threshold), S->npix, (int32_t*)(L.d + L.o_lab), (uint8_t*)(L.d + L.o_state));
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}
static int enqueue_labels(stocs_ctx* c, const DepthState* S, const RenderLayout& L, const stocs_render_params* prm, const void* d_zkey) {
    return render_enqueue_labels(c, S, L, prm->tolerance, prm->class_threshold, d_zkey);
}

int render_read_back(stocs_ctx* c, const RenderLayout& L, size_t from, size_t to) {
    STOCS_HIP_CHECK(hipMemcpyAsync(L.h + from, L.d + from, to - from, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return STOCS_OK;
}

}  // namespace stocs

using namespace stocs;

extern "C" void stocs_default_render_params(stocs_render_params* p) {
    if (!p) return;
    p->point_radius = 0.005f; p->max_splat_px = 8; p->tolerance = 0.01f; p->class_threshold = 0.10f;
}

extern "C" int stocs_render_poses(stocs_ctx* c, const float* poses, int n, int id_base, const stocs_render_params* prm, void* d_zkey, int clear) {
    static const char* who = "stocs_render_poses";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n == 0) return STOCS_OK;
    if (!poses || !prm || !d_zkey) { set_error("%s: NULL poses, parameters or key buffer", who); return STOCS_ERR_INVALID; }
    { const int rc = check_params(who, prm); if (rc) return rc; }
    { const int rc = render_check_ids(who, n, id_base); if (rc) return rc; }
    DepthState* S = NULL;
    { const int rc = check_frame(who, c, &S); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    RenderLayout L;
    { const int rc = render_layout(c, 0, n, 0, &L); if (rc) return rc; }
    { const int rc = render_upload_poses(c, L, poses, n); if (rc) return rc; }
    if (clear) { const int rc = render_enqueue_clear(c, S, d_zkey); if (rc) return rc; }
    { const int rc = enqueue_splat(c, S, L, n, prm, id_base, d_zkey); if (rc) return rc; }
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));   // another context may continue on the buffer
    return STOCS_OK;
}

extern "C" int stocs_render_resolve(stocs_ctx* c, const float* poses, int n, int id_base, const stocs_render_params* prm, const void* d_zkey,
                                    stocs_render_result* out) {
    static const char* who = "stocs_render_resolve";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n == 0) return STOCS_OK;
    if (!poses || !prm || !d_zkey || !out) { set_error("%s: NULL poses, parameters, key buffer or results", who); return STOCS_ERR_INVALID; }
    { const int rc = check_params(who, prm); if (rc) return rc; }
    { const int rc = render_check_ids(who, n, id_base); if (rc) return rc; }
    DepthState* S = NULL;
    { const int rc = check_frame(who, c, &S); if (rc) return rc; }
    { const int rc = check_capacity(who, S); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    RenderLayout L;
    { const int rc = render_layout(c, 0, n, 0, &L); if (rc) return rc; }
    { const int rc = render_upload_poses(c, L, poses, n); if (rc) return rc; }
    { const int rc = enqueue_resolve(c, S, L, n, prm, id_base, d_zkey); if (rc) return rc; }
    { const int rc = render_read_back(c, L, L.o_res, L.o_res + (size_t)n * sizeof(stocs_render_result)); if (rc) return rc; }
    memcpy(out, L.h + L.o_res, (size_t)n * sizeof(stocs_render_result));
    return STOCS_OK;
}

extern "C" int stocs_render_labels(stocs_ctx* c, const void* d_zkey, const stocs_render_params* prm, int32_t* labels, uint8_t* state) {
    static const char* who = "stocs_render_labels";
    if (!c || !d_zkey || !prm || !labels) { set_error("%s: NULL context, key buffer, parameters or labels", who); return STOCS_ERR_INVALID; }
    { const int rc = check_params(who, prm); if (rc) return rc; }
    DepthState* S = NULL;
    { const int rc = check_frame(who, c, &S); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    RenderLayout L;
    { const int rc = render_layout(c, 0, 0, S->npix, &L); if (rc) return rc; }
    { const int rc = enqueue_labels(c, S, L, prm, d_zkey); if (rc) return rc; }
    { const int rc = render_read_back(c, L, L.o_lab, L.o_state + S->npix); if (rc) return rc; }
    memcpy(labels, L.h + L.o_lab, S->npix * 4);
    if (state) memcpy(state, L.h + L.o_state, S->npix);
    return STOCS_OK;
}

extern "C" int stocs_explain_poses(stocs_ctx* c, const float* poses, int n, const stocs_render_params* prm, stocs_render_result* out, int32_t* labels,
                                   uint8_t* state) {
    static const char* who = "stocs_explain_poses";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n == 0 && !labels) return STOCS_OK;
    if (n > 0) {
        if (!poses || !prm || !out) { set_error("%s: NULL poses, parameters or results", who); return STOCS_ERR_INVALID; }
        { const int rc = check_params(who, prm); if (rc) return rc; }
        { const int rc = render_check_ids(who, n, 0); if (rc) return rc; }
    }
    DepthState* S = NULL;
    { const int rc = check_frame(who, c, &S); if (rc) return rc; }
    if (n == 0) {   // nothing rendered: the all-empty label image, no device work
        for (size_t i = 0; i < S->npix; ++i) labels[i] = -1;
        if (state) memset(state, 0, S->npix);
        return STOCS_OK;
    }
    { const int rc = check_capacity(who, S); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    RenderLayout L;
    { const int rc = render_layout(c, S->npix, n, labels ? S->npix : 0, &L); if (rc) return rc; }
    void* d_zkey = ctx_state_if<RenderState>(c)->work.p;
    { const int rc = render_upload_poses(c, L, poses, n); if (rc) return rc; }
    { const int rc = render_enqueue_clear(c, S, d_zkey); if (rc) return rc; }
    { const int rc = enqueue_splat(c, S, L, n, prm, 0, d_zkey); if (rc) return rc; }
    { const int rc = enqueue_resolve(c, S, L, n, prm, 0, d_zkey); if (rc) return rc; }
    if (labels) { const int rc = enqueue_labels(c, S, L, prm, d_zkey); if (rc) return rc; }
    { const int rc = render_read_back(c, L, L.o_res, labels ? L.o_state + S->npix : L.o_res + (size_t)n * sizeof(stocs_render_result)); if (rc) return rc; }
    memcpy(out, L.h + L.o_res, (size_t)n * sizeof(stocs_render_result));
    if (labels) memcpy(labels, L.h + L.o_lab, S->npix * 4);
    if (labels && state) memcpy(state, L.h + L.o_state, S->npix);
    return STOCS_OK;
}
