// render_mesh.hip -- the joint renderer and the scene footprints on the triangle mesh of stocs_ctx_set_mesh (stocs_render_poses_mesh,
// stocs_render_resolve_mesh, stocs_explain_poses_mesh, stocs_scene_footprints_mesh): instance masks, what hides what, the agreement with
// the depth image and the pixel rows of scene selection from the exact surface instead of point splats.  No reference counterpart.  The
// contract is written down at the declarations in include/stocs_hip.h as a composition of Z_h, the image stocs_render_depth_mesh defines
// for pose h alone; tests/render_mesh_ref.py restates it on tests/mesh_ref.py and the results are equal bit for bit: keys are packed
// integers under a minimum, counts are integer sums.
//
//   render    mesh.hip's mesh_render_kernel with its key sink (mesh_enqueue_keys): every pose of the launch writes the one key buffer, one
//             64-bit atomicMin per hit pixel, the id in a scalar register.
//   resolve   per chunk of poses (256 MB of z-buffers; STOCS_RENDER_MESH_CHUNK=<poses> forces a size) every pose is rendered ALONE into a
//             z-buffer of its own with the depth sink (mesh_enqueue_depth), which also leaves its rectangle.  render_resolve_mesh_kernel
//             then walks the rows of that rectangle: a wavefront takes runs of 64 consecutive pixels of one pose, each lane loads the
//             pose's own depth (4 bytes, coalesced) and, where one is present, the key (8 bytes): hidden if the key's id is another's, else
//             classified with the key's z (classify_pixel, render_rules.h).  Every count is a __ballot + __popcll in wave-uniform registers
//             (the loop bounds are wave-uniform); one integer atomicAdd per counter and workgroup into the record.  Several workgroups per
//             pose, no footprint bitset, no cap on the frame.
//   scene     scene.hip's chunk loop and classify kernel as they stand (scene_footprints_with), the z-buffers filled by the depth sink.
// Clear, pose upload, labels and read-back are render.hip's (render_shared.h).
// Known limits: the resolve renders every pose a second time (the key buffer holds only the winners' depths); a pose whose rectangle is
// a few rows leaves most workgroups of its column of the grid without a run.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "render_shared.h"

namespace stocs {

enum { RM_RUNS_PER_WAVE = 8 };
enum { RM_FOOTPRINT = 0, RM_VISIBLE, RM_HIDDEN, RM_NO_DEPTH, RM_AGREE, RM_IN_FRONT, RM_BEHIND, RM_ON_MASK, RM_COUNTS };   // the fields of stocs_render_result in order

struct RenderMeshState {
    static const StateOwner OWNER = OWN_RENDER_MESH;
    ~RenderMeshState() { render.free(); resolve.free(); explain.free(); scene.free(); }
    DevBlock render;    // stocs_render_poses_mesh: poses | rectangles, grow-only
    DevBlock resolve;   // stocs_render_resolve_mesh: poses | records | one chunk of rectangles and z-buffers, grow-only
    DevBlock explain;   // stocs_explain_poses_mesh: own key buffer | poses | records | labels | state | rectangles | one chunk of rectangles and z-buffers, grow-only
    DevBlock scene;     // stocs_scene_footprints_mesh: poses | records | one chunk of z-buffers and rectangles, grow-only
    float last_ms[2] = {-1.0f, -1.0f};   // "device_clock": HIP-event time of the last call's key render and of its last chunk's resolve kernel (-1: not taken)
};

// pose blockIdx.y of the chunk: its z-buffer at zbuf + blockIdx.y * npix, its rectangle at box + blockIdx.y * VSD_BOX_WORDS, its id
// id_base + blockIdx.y, its record at rec + blockIdx.y (zeroed in front).  Run r of the rectangle's rows goes to wavefront
// r % (4 * gridDim.x); the loop bounds are wave-uniform, so every __ballot sees the whole wavefront.
__global__ __launch_bounds__(256) void render_resolve_mesh_kernel(const uint32_t* __restrict__ zbuf, const int32_t* __restrict__ box, const unsigned long long* __restrict__ zkey,
                                                                  const uint16_t* __restrict__ depth, const uint16_t* __restrict__ prob, DepthArgs a, int id_base,
                                                                  stocs_render_result* __restrict__ rec) {
    __shared__ int cnt[RM_COUNTS];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int h = (int)blockIdx.y;
    const int32_t* bx = box + (size_t)h * VSD_BOX_WORDS;
    const int r0 = -bx[VB_NEG_R0], r1 = bx[VB_R1];   // the same address in every lane: uniform loads
    if (bx[VB_C1] < 0 || r1 < r0) return;            // nothing rendered (the whole workgroup: no barrier is left behind)
    const size_t npix = (size_t)a.W * (size_t)a.H;
    const uint32_t* z = zbuf + (size_t)h * npix;
    const uint32_t id = (uint32_t)(id_base + h);
    if (tid < RM_COUNTS) cnt[tid] = 0;
    __syncthreads();
    // 0 <= r0 <= r1 <= H - 1: the rows of clamped boxes
    const size_t px0 = (size_t)r0 * (size_t)a.W, px1 = (size_t)(r1 + 1) * (size_t)a.W;
    const size_t n_runs = (px1 - px0 + 63) >> 6;
    int n_foot = 0, n_vis = 0, n_hidden = 0, n_nod = 0, n_agree = 0, n_front = 0, n_behind = 0, n_mask = 0;
    for (size_t run = (size_t)blockIdx.x * 4 + (size_t)(tid >> 6); run < n_runs; run += (size_t)gridDim.x * 4) {
        const size_t px = px0 + run * 64 + (size_t)lane;
        bool set = false, hidden = false;
        int cls = 0;
        if (px < px1) {
            set = z[px] != 0xFFFFFFFFu;
            if (set) {
                const unsigned long long key = zkey[px];
                hidden = (uint32_t)key != id;   // an empty key's low word is all ones, which no id is
                if (!hidden) cls = classify_pixel(__uint_as_float((uint32_t)(key >> 32)), px, depth, prob, a);
            }
        }
        n_foot += __popcll(__ballot(set)); n_hidden += __popcll(__ballot(hidden)); n_vis += __popcll(__ballot(set && !hidden));
        n_nod += __popcll(__ballot((cls & 15) == 1)); n_agree += __popcll(__ballot((cls & 15) == 2)); n_front += __popcll(__ballot((cls & 15) == 3));
        n_behind += __popcll(__ballot((cls & 15) == 4)); n_mask += __popcll(__ballot((cls & 16) != 0));
    }
    if (lane == 0 && n_foot) {   // every other count is at most the footprint
        atomicAdd(&cnt[RM_FOOTPRINT], n_foot); atomicAdd(&cnt[RM_VISIBLE], n_vis); atomicAdd(&cnt[RM_HIDDEN], n_hidden); atomicAdd(&cnt[RM_NO_DEPTH], n_nod);
        atomicAdd(&cnt[RM_AGREE], n_agree); atomicAdd(&cnt[RM_IN_FRONT], n_front); atomicAdd(&cnt[RM_BEHIND], n_behind); atomicAdd(&cnt[RM_ON_MASK], n_mask);
    }
    __syncthreads();
    if (tid < RM_COUNTS && cnt[tid]) atomicAdd((int32_t*)(rec + h) + tid, cnt[tid]);   // the record's fields in the order of the RM_ enum
}

// how many poses a chunk of z-buffers holds: 256 MB of them, or what STOCS_RENDER_MESH_CHUNK says; the pose is blockIdx.y
static size_t resolve_chunk(int n, size_t npix) {
    size_t chunk = std::max<size_t>(1, ((size_t)256 << 20) / (4 * npix));
    if (const char* e = getenv("STOCS_RENDER_MESH_CHUNK")) { const long v = atol(e); if (v >= 1) chunk = (size_t)v; }
    return std::min<size_t>(std::min<size_t>(chunk, (size_t)n), 65535);
}
static size_t resolve_tail(size_t chunk, size_t npix) { return al256(chunk * VSD_BOX_WORDS * 4) + al256(chunk * npix * 4); }

// the resolve of the n poses of the layout against d_zkey, chunk by chunk in the layout's tail at `tail`: records into the layout's region
static int enqueue_resolve_mesh(stocs_ctx* c, const DepthState* S, const RenderLayout& L, size_t tail, size_t chunk, int n, const DepthArgs& a, int id_base,
                                const void* d_zkey, bool dev_clock) {
    const size_t npix = S->npix;
    int32_t* d_box = (int32_t*)(L.d + tail);
    uint32_t* d_z = (uint32_t*)(L.d + tail + al256(chunk * VSD_BOX_WORDS * 4));
    const float* d_pose = (const float*)(L.d + L.o_pose);
    stocs_render_result* d_rec = (stocs_render_result*)(L.d + L.o_res);
    STOCS_HIP_CHECK(hipMemsetAsync(d_rec, 0, (size_t)n * sizeof(stocs_render_result), c->stream));
    const unsigned run_blocks = (unsigned)std::max<size_t>(1, ((npix + 63) / 64 + 4 * RM_RUNS_PER_WAVE - 1) / (4 * RM_RUNS_PER_WAVE));
    for (int h0 = 0; h0 < n; h0 += (int)chunk) {
        const int m = std::min((int)chunk, n - h0);
        const bool timed = dev_clock && h0 + m == n;
        STOCS_HIP_CHECK(hipMemsetAsync(d_z, 0xFF, (size_t)m * npix * 4, c->stream));
        STOCS_HIP_CHECK(hipMemsetAsync(d_box, 0x80, (size_t)m * VSD_BOX_WORDS * 4, c->stream));
        { const int rc = mesh_enqueue_depth(c, d_pose + (size_t)h0 * 16, m, a, d_z, d_box); if (rc) return rc; }
        if (timed) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[2], c->stream));
        hipLaunchKernelGGL(render_resolve_mesh_kernel, dim3(std::min(run_blocks, 65535u), (unsigned)m), dim3(256), 0, c->stream, (const uint32_t*)d_z, (const int32_t*)d_box,
                           (const unsigned long long*)d_zkey, frame_depth(S), frame_prob(S), a, id_base + h0, d_rec + h0);
        STOCS_HIP_CHECK(hipGetLastError());
        if (timed) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[3], c->stream));
    }
    return STOCS_OK;
}

// the rectangles of a key render: n of them, cleared, at d_box
static int enqueue_keys(stocs_ctx* c, const float* d_pose, int n, const DepthArgs& a, int id_base, void* d_zkey, int32_t* d_box, bool dev_clock) {
    STOCS_HIP_CHECK(hipMemsetAsync(d_box, 0x80, (size_t)n * VSD_BOX_WORDS * 4, c->stream));
    if (dev_clock) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[0], c->stream));
    { const int rc = mesh_enqueue_keys(c, d_pose, n, a, id_base, (unsigned long long*)d_zkey, d_box); if (rc) return rc; }
    if (dev_clock) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[1], c->stream));
    return STOCS_OK;
}

// after the call's synchronisation: the events of a "device_clock" call into last_ms
static void read_clock(stocs_ctx* c, bool keys, bool resolve) {
    RenderMeshState* R = ctx_state<RenderMeshState>(c);
    R->last_ms[0] = R->last_ms[1] = -1.0f;
    if (!c->device_clock) return;
    float ms = 0.0f;
    if (keys && hipEventElapsedTime(&ms, c->ev_t[0], c->ev_t[1]) == hipSuccess) R->last_ms[0] = ms;
    if (resolve && hipEventElapsedTime(&ms, c->ev_t[2], c->ev_t[3]) == hipSuccess) R->last_ms[1] = ms;
}

// the mesh as a SceneFill: d_side holds the chunk's rectangles
static int fill_mesh(stocs_ctx* c, const void*, const float* d_pose, int m, const DepthArgs& a, uint32_t* d_z, void* d_side) {
    STOCS_HIP_CHECK(hipMemsetAsync(d_side, 0x80, (size_t)m * VSD_BOX_WORDS * 4, c->stream));
    return mesh_enqueue_depth(c, d_pose, m, a, d_z, (int32_t*)d_side);
}

}  // namespace stocs

using namespace stocs;

extern "C" int stocs_render_mesh_last_device_ms(const stocs_ctx* c, float* key_ms, float* resolve_ms) {
    if (!c) { set_error("stocs_render_mesh_last_device_ms: NULL context"); return STOCS_ERR_INVALID; }
    const RenderMeshState* R = ctx_state_if<RenderMeshState>(c);
    if (key_ms) *key_ms = R ? R->last_ms[0] : -1.0f;
    if (resolve_ms) *resolve_ms = R ? R->last_ms[1] : -1.0f;
    return STOCS_OK;
}

extern "C" int stocs_render_poses_mesh(stocs_ctx* c, const float* poses, int n, int id_base, void* d_zkey, int clear) {
    static const char* who = "stocs_render_poses_mesh";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n == 0) return STOCS_OK;
    if (!poses || !d_zkey) { set_error("%s: NULL poses or key buffer", who); return STOCS_ERR_INVALID; }
    { const int rc = render_check_ids(who, n, id_base); if (rc) return rc; }
    { const int rc = mesh_check_present(who, c); if (rc) return rc; }
    DepthState* S = NULL;
    { const int rc = check_frame(who, c, &S); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    const bool dev_clock = c->device_clock != 0;
    RenderLayout L;
    { const int rc = render_layout(c, &ctx_state<RenderMeshState>(c)->render, 0, n, 0, al256((size_t)n * VSD_BOX_WORDS * 4), &L); if (rc) return rc; }
    { const int rc = render_upload_poses(c, L, poses, n); if (rc) return rc; }
    if (clear) { const int rc = render_enqueue_clear(c, S, d_zkey); if (rc) return rc; }
    { const int rc = enqueue_keys(c, (const float*)(L.d + L.o_pose), n, frame_args(S, 1.0f, 0.0f), id_base, d_zkey, (int32_t*)(L.d + L.o_tail), dev_clock); if (rc) return rc; }
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));   // another context may continue on the buffer
    read_clock(c, true, false);
    return STOCS_OK;
}

extern "C" int stocs_render_resolve_mesh(stocs_ctx* c, const float* poses, int n, int id_base, const stocs_render_params* prm, const void* d_zkey,
                                         stocs_render_result* out) {
    static const char* who = "stocs_render_resolve_mesh";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n == 0) return STOCS_OK;
    if (!poses || !prm || !d_zkey || !out) { set_error("%s: NULL poses, parameters, key buffer or results", who); return STOCS_ERR_INVALID; }
    { const int rc = check_classify_params(who, prm); if (rc) return rc; }
    { const int rc = render_check_ids(who, n, id_base); if (rc) return rc; }
    { const int rc = mesh_check_present(who, c); if (rc) return rc; }
    DepthState* S = NULL;
    { const int rc = check_frame(who, c, &S); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    const bool dev_clock = c->device_clock != 0;
    const size_t chunk = resolve_chunk(n, S->npix);
    RenderLayout L;
    { const int rc = render_layout(c, &ctx_state<RenderMeshState>(c)->resolve, 0, n, 0, resolve_tail(chunk, S->npix), &L); if (rc) return rc; }
    { const int rc = render_upload_poses(c, L, poses, n); if (rc) return rc; }
    { const int rc = enqueue_resolve_mesh(c, S, L, L.o_tail, chunk, n, frame_args(S, prm), id_base, d_zkey, dev_clock); if (rc) return rc; }
    { const int rc = render_read_back(c, L, L.o_res, L.o_res + (size_t)n * sizeof(stocs_render_result)); if (rc) return rc; }
    read_clock(c, false, true);
    memcpy(out, L.h + L.o_res, (size_t)n * sizeof(stocs_render_result));
    return STOCS_OK;
}

extern "C" int stocs_explain_poses_mesh(stocs_ctx* c, const float* poses, int n, const stocs_render_params* prm, stocs_render_result* out, int32_t* labels,
                                        uint8_t* state) {
    static const char* who = "stocs_explain_poses_mesh";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n == 0 && !labels) return STOCS_OK;
    if (n > 0) {
        if (!poses || !prm || !out) { set_error("%s: NULL poses, parameters or results", who); return STOCS_ERR_INVALID; }
        { const int rc = check_classify_params(who, prm); if (rc) return rc; }
        { const int rc = render_check_ids(who, n, 0); if (rc) return rc; }
        { const int rc = mesh_check_present(who, c); if (rc) return rc; }
    }
    DepthState* S = NULL;
    { const int rc = check_frame(who, c, &S); if (rc) return rc; }
    if (n == 0) {   // nothing rendered: the all-empty label image, no device work
        for (size_t i = 0; i < S->npix; ++i) labels[i] = -1;
        if (state) memset(state, 0, S->npix);
        return STOCS_OK;
    }
    DeviceGuard dev_guard(c->device);
    const bool dev_clock = c->device_clock != 0;
    RenderMeshState* R = ctx_state<RenderMeshState>(c);
    const size_t chunk = resolve_chunk(n, S->npix);
    const size_t key_boxes = al256((size_t)n * VSD_BOX_WORDS * 4);
    RenderLayout L;
    { const int rc = render_layout(c, &R->explain, S->npix, n, labels ? S->npix : 0, key_boxes + resolve_tail(chunk, S->npix), &L); if (rc) return rc; }
    void* d_zkey = R->explain.p;
    const DepthArgs a = frame_args(S, prm);
    { const int rc = render_upload_poses(c, L, poses, n); if (rc) return rc; }
    { const int rc = render_enqueue_clear(c, S, d_zkey); if (rc) return rc; }
    { const int rc = enqueue_keys(c, (const float*)(L.d + L.o_pose), n, a, 0, d_zkey, (int32_t*)(L.d + L.o_tail), dev_clock); if (rc) return rc; }
    { const int rc = enqueue_resolve_mesh(c, S, L, L.o_tail + key_boxes, chunk, n, a, 0, d_zkey, dev_clock); if (rc) return rc; }
    if (labels) { const int rc = render_enqueue_labels(c, S, L, prm->tolerance, prm->class_threshold, d_zkey); if (rc) return rc; }
    { const int rc = render_read_back(c, L, L.o_res, labels ? L.o_state + S->npix : L.o_res + (size_t)n * sizeof(stocs_render_result)); if (rc) return rc; }
    read_clock(c, true, true);
    memcpy(out, L.h + L.o_res, (size_t)n * sizeof(stocs_render_result));
    if (labels) memcpy(labels, L.h + L.o_lab, S->npix * 4);
    if (labels && state) memcpy(state, L.h + L.o_state, S->npix);
    return STOCS_OK;
}

extern "C" int stocs_scene_footprints_mesh(stocs_ctx* c, const float* poses, int n, int slot_base, int n_slots, const stocs_render_params* prm, int claim, void* d_rows,
                                           stocs_scene_record* out) {
    static const char* who = "stocs_scene_footprints_mesh";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n == 0) return STOCS_OK;
    if (!poses || !prm || !d_rows || !out) { set_error("%s: NULL poses, parameters, rows or records", who); return STOCS_ERR_INVALID; }
    if (claim != 0 && claim != 1) { set_error("%s: claim %d is neither 0 (agree) nor 1 (on_mask)", who, claim); return STOCS_ERR_INVALID; }
    if (slot_base < 0 || (long long)slot_base + (long long)n > (long long)n_slots) {
        set_error("%s: slots %d .. %lld outside a pool of %d", who, slot_base, (long long)slot_base + (long long)n - 1, n_slots);
        return STOCS_ERR_INVALID;
    }
    { const int rc = check_classify_params(who, prm); if (rc) return rc; }
    { const int rc = mesh_check_present(who, c); if (rc) return rc; }
    DepthState* F = NULL;
    { const int rc = check_frame(who, c, &F); if (rc) return rc; }
    { const int rc = scene_check_pixels(who, F->npix); if (rc) return rc; }
    const SceneFill fill = {fill_mesh, NULL, (size_t)VSD_BOX_WORDS * 4};
    return scene_footprints_with(c, F, &ctx_state<RenderMeshState>(c)->scene, fill, poses, n, slot_base, prm->tolerance, prm->class_threshold, claim, d_rows, out);
}
