// vsd.hip -- the surfel depth renderer and the visible-surface discrepancy on top of it (stocs_render_depth, stocs_pose_errors_vsd): the
// third measure of the BOP benchmark next to pose_error_sym.hip's MSSD and MSPD, and the only one that looks at what the camera saw.  No
// reference counterpart.  The contract (float order, comparisons, the z-buffer) is written down at the declarations in
// include/stocs_hip.h; tests/vsd_ref.py restates it in float32 numpy, and the results are equal bit for bit: depths are float bits under
// a minimum, counts are integer sums.
//
// scene.hip's layout: a z-buffer of npix uint32 float bits per rendered pose in a chunk of workspace (256 MB; STOCS_VSD_CHUNK=<poses>
// forces a size), empty = all ones, cleared by hipMemsetAsync.  A chunk holds whole pairs (ground truth, estimate); with n_gt == 1 the one
// ground truth is rendered once, in the first chunk's launch, into a buffer of its own that stays beside the chunks.
//   render    vsd_render_kernel: a workgroup of four wavefronts per (pose, VSD_POINTS = 256 model points: one batch of 64 per wavefront; a
//             wavefront that walks more surfels one after the other makes small calls a latency chain), the pose in scalar registers.  A
//             wavefront projects 64 points, one per lane, and then takes the in_image ones in turn (__ballot, lowest lane first): the surfel's
//             ten values go into scalar registers by readlane, and all 64 lanes sweep its clipped square, pixel idx = lane + 64 pass, with one
//             ray-disc test (three IEEE divisions) each and a 32-bit atomicMin per hit pixel.  In large calls on dense models (surfel_args) a
//             hit pixel first reads its stored depth and only issues the atomic when its own is nearer: the stored value only falls, so a
//             stale read costs an atomic and never a result.  Unlike the splat kernels (one lane writes a point's whole square, their listed
//             limit) a surfel of 33 x 33 pixels is 17 passes of the wavefront.  Each wavefront adds its surfels' clipped squares to the pose's
//             bounding rectangle: four atomicMax.
//   compare   vsd_compare_kernel: one pass per pair over the union of the two rectangles in both z-buffers and the frame, 64 consecutive
//             pixels of it per wavefront and round; the
//             22 counts by __ballot and popcount in scalar registers, added to LDS words once per wavefront, one integer atomicAdd per
//             non-zero counter and workgroup into the pair's counts.  A round whose 64 pixels are empty in both buffers reads nothing else.
// The e[t] of a record are formed on the host from the counts that come back (one division each).  stocs_render_depth runs the render
// kernel alone and turns bits into floats while it copies the pinned block out.
// The two call bodies take a renderer (vsd_shared.h): mesh.hip fills the same z-buffers from triangles and shares the chunks, the rectangle
// slots, the clears, the compare and the records with the surfels.
// STOCS_VSD_FORM=<bits> forces a form of the kernels (vsd_form below); every form gives the same bits.
// Known limits: whole frames are cleared (a pose's rectangle is known only after projection); a pixel's ray (two divisions) is recomputed
// for every surfel that tests it.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "eval_call.h"
#include "pose_error_math.h"
#include "render_rules.h"
#include "vsd_shared.h"
#include "wave_bits.h"

namespace stocs {

enum { VSD_POINTS = STOCS_VSD_POINTS, VSD_COUNTS = 6 + STOCS_VSD_MAX_TAU, VSD_REC_WORDS = 24, VSD_ROUNDS_PER_BLOCK = 8 };
enum { VC_PX_EST = 0, VC_PX_GT, VC_VIS_EST, VC_VIS_GT, VC_INTER, VC_UNI, VC_FAR };

struct VsdState {
    static const StateOwner OWNER = OWN_VSD;
    ~VsdState() { work.free(); }
    DevBlock work;   // poses in render order (16 floats each) | counts (VSD_REC_WORDS int32 per pair) | the rectangles and the z-buffers of one chunk, grow-only
};

struct VsdSurfelArgs { float radius, r2; int max_px, read_first; };
struct VsdCompareArgs { float delta; int n_tau; float tau[STOCS_VSD_MAX_TAU]; };

// zbuf: the z-buffer of pose blockIdx.y of the launch at zbuf + blockIdx.y * npix, its rectangle at box + blockIdx.y * VSD_BOX_WORDS
__global__ __launch_bounds__(256) void vsd_render_kernel(const float* __restrict__ poses, const float4* __restrict__ mpos, const float4* __restrict__ mnrm, int nM, DepthArgs a,
                                                         VsdSurfelArgs sa, uint32_t* zbuf, int32_t* __restrict__ box) {
    const int h = (int)blockIdx.y;
    float P[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = poses[(size_t)h * 16 + i];   // the same address in every lane: uniform loads
    if (!pose_finite(P)) return;
    uint32_t* z = zbuf + (size_t)h * ((size_t)a.W * (size_t)a.H);
    int b_nc0 = (int)0x80808080, b_c1 = (int)0x80808080, b_nr0 = (int)0x80808080, b_r1 = (int)0x80808080;   // this lane's share of the rectangle
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int first = (int)blockIdx.x * VSD_POINTS;
    const int last = first + VSD_POINTS < nM ? first + VSD_POINTS : nM;
    for (int base = first + wave * 64; base < last; base += 256) {   // wave-uniform bounds: every __ballot sees the whole wavefront
        const int i = base + lane;
        float p0 = 0.0f, p1 = 0.0f, p2 = 1.0f, q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, f = 0.0f;
        int col = 0, row = 0, s = 0;
        bool in_image = false;
        if (i < last) {
            // steps 1-3 of the depth-check contract: project_point's expressions (depth_frame.h), with p, q and f kept
            const float4 m = mpos[i], k = mnrm[i];
            p0 = (P[0] * m.x + (P[4] * m.y + P[8] * m.z)) + P[12];
            p1 = (P[1] * m.x + (P[5] * m.y + P[9] * m.z)) + P[13];
            p2 = (P[2] * m.x + (P[6] * m.y + P[10] * m.z)) + P[14];
            q0 = P[0] * k.x + (P[4] * k.y + P[8] * k.z);
            q1 = P[1] * k.x + (P[5] * k.y + P[9] * k.z);
            q2 = P[2] * k.x + (P[6] * k.y + P[10] * k.z);
            f = q0 * p0 + (q1 * p1 + q2 * p2);
            const bool facing = f < 0.0f && p2 > 1e-6f;
            const float u = floorf(((a.fx * p0) / p2 + a.cx) + 0.5f);
            const float v = floorf(((a.fy * p1) / p2 + a.cy) + 0.5f);
            in_image = facing && u >= 0.0f && u < (float)a.W && v >= 0.0f && v < (float)a.H;
            if (in_image) {
                col = (int)u; row = (int)v;
                s = (int)fminf(floorf((a.fx * sa.radius) / p2 + 0.5f), (float)sa.max_px);
                const int nc0 = col - s > 0 ? s - col : 0, c1 = col + s < a.W - 1 ? col + s : a.W - 1;
                const int nr0 = row - s > 0 ? s - row : 0, r1 = row + s < a.H - 1 ? row + s : a.H - 1;
                b_nc0 = nc0 > b_nc0 ? nc0 : b_nc0; b_c1 = c1 > b_c1 ? c1 : b_c1; b_nr0 = nr0 > b_nr0 ? nr0 : b_nr0; b_r1 = r1 > b_r1 ? r1 : b_r1;
            }
        }
        unsigned long long todo = __ballot(in_image);
        while (todo) {   // wave-uniform: one surfel at a time, in scalar registers
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const float sp0 = lane_f(p0, src), sp1 = lane_f(p1, src), sp2 = lane_f(p2, src);
            const float sq0 = lane_f(q0, src), sq1 = lane_f(q1, src), sq2 = lane_f(q2, src), sf = lane_f(f, src);
            const int scol = lane_i(col, src), srow = lane_i(row, src), ss = lane_i(s, src);
            const int r0 = srow - ss > 0 ? srow - ss : 0, r1 = srow + ss < a.H - 1 ? srow + ss : a.H - 1;
            const int c0 = scol - ss > 0 ? scol - ss : 0, c1 = scol + ss < a.W - 1 ? scol + ss : a.W - 1;
            const int w = c1 - c0 + 1, npx = w * (r1 - r0 + 1);   // 1 <= w <= 33, npx <= 1089
            // idx / w for idx < 1089 by one multiply: mul = floor(65536 / w) + 1 overshoots 65536 / w by at most 1, so the quotient's error
            // idx / 65536 < 1 / 33 never reaches the next integer.  65536.0f / w is off an integer by at least 1 / 33 when w does not divide it.
            const int mul = (int)(65536.0f / (float)w) + 1;
            for (int idx = lane; idx < npx; idx += 64) {
                const int rr = (idx * mul) >> 16;
                const int r = r0 + rr, c = c0 + (idx - rr * w);
                const float xn = ((float)c - a.cx) / a.fx, yn = ((float)r - a.cy) / a.fy;
                const float dn = sq0 * xn + (sq1 * yn + sq2);
                if (!(dn < 0.0f)) continue;
                const float zz = sf / dn;
                if (!(zz > 1e-6f)) continue;
                const float ex = xn * zz - sp0, ey = yn * zz - sp1, ez = zz - sp2;
                if (!((ex * ex) + ((ey * ey) + (ez * ez)) <= sa.r2)) continue;
                uint32_t* cell = &z[(size_t)r * (size_t)a.W + (size_t)c];   // 0 <= r < H, 0 <= c < W by the clip above
                const uint32_t bits = __float_as_uint(zz);
                if (!sa.read_first || bits < *cell) atomicMin(cell, bits);
            }
        }
    }
    b_nc0 = wave_max_i(b_nc0); b_c1 = wave_max_i(b_c1); b_nr0 = wave_max_i(b_nr0); b_r1 = wave_max_i(b_r1);
    if (lane == 0 && b_c1 >= 0) {   // some surfel of this wavefront was in the image
        int32_t* bx = box + (size_t)h * VSD_BOX_WORDS;
        atomicMax(&bx[VB_NEG_C0], b_nc0); atomicMax(&bx[VB_C1], b_c1); atomicMax(&bx[VB_NEG_R0], b_nr0); atomicMax(&bx[VB_R1], b_r1);
    }
}

// pair blockIdx.y of the launch: the estimate's z-buffer at zE + pair * strideE, the ground truth's at zG + pair * strideG (0: one for all),
// its counts at cnt_out + pair * VSD_REC_WORDS.  With boxE the walk covers the union of the two rendered rectangles (boxE + pair * box_strideE
// and boxG + pair * box_strideG words: a rectangle per z-buffer, in the same order), else the whole frame.  The loop bounds are wave-uniform, so every
// __ballot sees the whole wavefront.
__global__ __launch_bounds__(256) void vsd_compare_kernel(const uint32_t* __restrict__ zE, size_t strideE, const uint32_t* __restrict__ zG, size_t strideG,
                                                          const int32_t* __restrict__ boxE, int box_strideE, const int32_t* __restrict__ boxG, int box_strideG, const uint16_t* __restrict__ depth,
                                                          DepthArgs a, VsdCompareArgs v, int32_t* __restrict__ cnt_out) {
    __shared__ int cnt[VSD_COUNTS];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int pair = (int)blockIdx.y;
    const uint32_t* ze = zE + (size_t)pair * strideE;
    const uint32_t* zg = zG + (size_t)pair * strideG;
    int c0 = 0, r0 = 0, bw = a.W, bh = a.H;
    if (boxE) {   // a kernel argument: wave-uniform, and so are the eight loads
        const int32_t* be = boxE + (size_t)pair * (size_t)box_strideE;
        const int32_t* bg = boxG + (size_t)pair * (size_t)box_strideG;
        const int nc0 = be[VB_NEG_C0] > bg[VB_NEG_C0] ? be[VB_NEG_C0] : bg[VB_NEG_C0], c1 = be[VB_C1] > bg[VB_C1] ? be[VB_C1] : bg[VB_C1];
        const int nr0 = be[VB_NEG_R0] > bg[VB_NEG_R0] ? be[VB_NEG_R0] : bg[VB_NEG_R0], r1 = be[VB_R1] > bg[VB_R1] ? be[VB_R1] : bg[VB_R1];
        if (c1 < 0) return;   // neither pose rendered anything: the counts stay zero
        c0 = -nc0; r0 = -nr0; bw = c1 - c0 + 1; bh = r1 - r0 + 1;
    }
    const int npix = bw * bh;
    if (tid < VSD_COUNTS) cnt[tid] = 0;
    __syncthreads();
    int n_pe = 0, n_pg = 0, n_ve = 0, n_vg = 0, n_in = 0, n_un = 0;
    int n_far[STOCS_VSD_MAX_TAU];
#pragma unroll
    for (int t = 0; t < STOCS_VSD_MAX_TAU; ++t) n_far[t] = 0;
    const int wave_base = __builtin_amdgcn_readfirstlane(tid >> 6) * 64;
    for (int base = (int)blockIdx.x * 256 + wave_base; base < npix; base += (int)gridDim.x * 256) {
        const int idx = base + lane;
        const int rr = idx / bw;
        const int r = r0 + rr, c = c0 + (idx - rr * bw);
        const int px = r * a.W + c;   // inside the frame when idx < npix
        uint32_t be = 0xFFFFFFFFu, bg = 0xFFFFFFFFu;
        if (idx < npix) { be = ze[px]; bg = zg[px]; }
        const bool pe = be != 0xFFFFFFFFu, pg = bg != 0xFFFFFFFFu;
        if (__ballot(pe || pg) == 0ull) continue;   // wave-uniform
        bool visE = false, visG = false, inter = false;
        float dd = 0.0f;
        if (pe || pg) {
            const float xn = ((float)c - a.cx) / a.fx, yn = ((float)r - a.cy) / a.fy;
            const float k = stocs_sqrtf((xn * xn + yn * yn) + 1.0f);
            const uint16_t raw = depth[px];
            const float dS = ((float)raw * a.depth_scale) * k;
            const float dE = __uint_as_float(be) * k, dG = __uint_as_float(bg) * k;   // of an absent surface: NaN, never used
            visG = pg && (raw == 0 || dG - dS <= v.delta);
            visE = pe && (raw == 0 || dE - dS <= v.delta || visG);
            inter = visG && visE;
            dd = fabsf(dG - dE);
        }
        n_pe += __popcll(__ballot(pe)); n_pg += __popcll(__ballot(pg)); n_ve += __popcll(__ballot(visE)); n_vg += __popcll(__ballot(visG));
        n_in += __popcll(__ballot(inter)); n_un += __popcll(__ballot(visG || visE));
#pragma unroll
        for (int t = 0; t < STOCS_VSD_MAX_TAU; ++t)
            if (t < v.n_tau) n_far[t] += __popcll(__ballot(inter && dd >= v.tau[t]));   // wave-uniform: n_tau is a kernel argument
    }
    if (lane == 0 && (n_pe | n_pg)) {   // every other count is at most these two
        atomicAdd(&cnt[VC_PX_EST], n_pe); atomicAdd(&cnt[VC_PX_GT], n_pg); atomicAdd(&cnt[VC_VIS_EST], n_ve); atomicAdd(&cnt[VC_VIS_GT], n_vg);
        atomicAdd(&cnt[VC_INTER], n_in); atomicAdd(&cnt[VC_UNI], n_un);
#pragma unroll
        for (int t = 0; t < STOCS_VSD_MAX_TAU; ++t) atomicAdd(&cnt[VC_FAR + t], n_far[t]);
    }
    __syncthreads();
    if (tid < VSD_COUNTS && cnt[tid]) atomicAdd(cnt_out + (size_t)pair * VSD_REC_WORDS + tid, cnt[tid]);   // the counts in the order of the VC_ enum
}

// surfel_radius and max_splat_px, which both entry points read
static int check_surfel(const char* who, const stocs_vsd_params* p) {
    if (!(p->surfel_radius > 0.0f) || !isfinite(p->surfel_radius)) { set_error("%s: surfel_radius %g must be positive and finite", who, (double)p->surfel_radius); return STOCS_ERR_INVALID; }
    if (p->max_splat_px < 0 || p->max_splat_px > RENDER_MAX_SPLAT) { set_error("%s: max_splat_px %d outside 0..%d", who, p->max_splat_px, (int)RENDER_MAX_SPLAT); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}

// delta and the taus, which the compare reads
static int check_compare(const char* who, const stocs_vsd_params* p) {
    if (!(p->delta > 0.0f) || !isfinite(p->delta)) { set_error("%s: delta %g must be positive and finite", who, (double)p->delta); return STOCS_ERR_INVALID; }
    if (p->n_tau < 1 || p->n_tau > STOCS_VSD_MAX_TAU) { set_error("%s: n_tau %d outside 1..%d", who, p->n_tau, (int)STOCS_VSD_MAX_TAU); return STOCS_ERR_INVALID; }
    for (int t = 0; t < p->n_tau; ++t)
        if (!(p->tau[t] > 0.0f) || !isfinite(p->tau[t])) { set_error("%s: tau[%d] = %g must be positive and finite", who, t, (double)p->tau[t]); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}

static int check_vsd(const char* who, const stocs_vsd_params* p) {
    { const int rc = check_surfel(who, p); if (rc) return rc; }
    return check_compare(who, p);
}

// STOCS_VSD_FORM=<bits> in the environment chooses the kernels' forms, for measurements and for the tests; no bit changes a result.
// 1: compare whole frames, not the pair's bounding rectangle; 2: every hit pixel issues its atomicMin without reading the stored depth
// first, 4: every hit pixel reads first (neither: the call's size decides, surfel_args)
enum { VSD_FORM_WHOLE_FRAMES = 1, VSD_FORM_BLIND_ATOMICS = 2, VSD_FORM_READ_FIRST = 4 };
// Reading the stored depth saves the atomics of the surfels that lose a pixel and costs every pass of a wavefront a memory round trip.
// It pays on a model dense enough that several surfels meet in a pixel, in a call with enough wavefronts to hide the round trip
// (measured: DESIGN 7.15); elsewhere the atomics go out blind.
enum { VSD_DENSE_POINTS = 2048, VSD_BUSY_POINTS = 200000 };
static int vsd_form() {
    const char* e = getenv("STOCS_VSD_FORM");
    return e ? atoi(e) : 0;
}

static VsdSurfelArgs surfel_args(const stocs_vsd_params* p, int nM, size_t n_render) {
    VsdSurfelArgs s;
    s.radius = p->surfel_radius; s.r2 = p->surfel_radius * p->surfel_radius; s.max_px = p->max_splat_px;
    const int form = vsd_form();
    s.read_first = (form & VSD_FORM_BLIND_ATOMICS) ? 0 : (form & VSD_FORM_READ_FIRST) ? 1 : (nM >= VSD_DENSE_POINTS && (size_t)nM * n_render >= (size_t)VSD_BUSY_POINTS);
    return s;
}

// m poses at d_pose into the m z-buffers at d_z and their rectangles at d_box, both cleared first
static int render_into(stocs_ctx* c, const VsdRenderer& rd, const float* d_pose, int m, const DepthArgs& a, size_t npix, uint32_t* d_z, int32_t* d_box) {
    STOCS_HIP_CHECK(hipMemsetAsync(d_z, 0xFF, (size_t)m * npix * 4, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(d_box, 0x80, (size_t)m * VSD_BOX_WORDS * 4, c->stream));
    return rd.render(c, rd.self, d_pose, m, a, d_z, d_box);
}

// how many rendered poses a chunk of z-buffers holds: 256 MB of them, or what STOCS_VSD_CHUNK says
static size_t chunk_poses(size_t npix) {
    size_t chunk = std::max<size_t>(2, ((size_t)256 << 20) / (4 * npix));
    if (const char* e = getenv("STOCS_VSD_CHUNK")) { const long v = atol(e); if (v >= 1) chunk = (size_t)v; }
    return std::min<size_t>(chunk, 65534);   // a rendered pose is blockIdx.y
}

// the surfel renderer as a VsdRenderer: self is the call's VsdSurfelArgs
static int render_surfels(stocs_ctx* c, const void* self, const float* d_pose, int m, const DepthArgs& a, uint32_t* d_z, int32_t* d_box) {
    const VsdSurfelArgs& sa = *(const VsdSurfelArgs*)self;
    const unsigned point_chunks = (unsigned)((c->nM + VSD_POINTS - 1) / VSD_POINTS);
    hipLaunchKernelGGL(vsd_render_kernel, dim3(point_chunks, (unsigned)m), dim3(256), 0, c->stream, d_pose, (const float4*)c->d_mpos_raw, (const float4*)c->d_mnrm, c->nM, a, sa,
                       d_z, d_box);
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

}  // namespace stocs

using namespace stocs;

extern "C" void stocs_default_vsd_params(stocs_vsd_params* p) {
    if (!p) return;
    p->surfel_radius = 0.006f; p->max_splat_px = 16; p->delta = 0.015f; p->n_tau = 0;
    for (int t = 0; t < STOCS_VSD_MAX_TAU; ++t) p->tau[t] = 0.0f;
}

extern "C" int stocs_check_vsd_params(const stocs_vsd_params* p) {
    if (!p) { set_error("stocs_check_vsd_params: NULL parameters"); return STOCS_ERR_INVALID; }
    return check_vsd("stocs_check_vsd_params", p);
}

int stocs::vsd_check_compare_params(const char* who, const stocs_vsd_params* p) { return check_compare(who, p); }

extern "C" int stocs_render_depth(stocs_ctx* c, const float* poses, int n, const stocs_vsd_params* prm, float* depth) {
    static const char* who = "stocs_render_depth";
    { int rc; if (check_batch(who, c, n, &rc)) return rc; }
    if (!poses || !prm || !depth) { set_error("%s: NULL poses, parameters or images", who); return STOCS_ERR_INVALID; }
    { const int rc = check_surfel(who, prm); if (rc) return rc; }
    { const int rc = check_model(who, c); if (rc) return rc; }
    DepthState* F = NULL;
    { const int rc = check_frame(who, c, &F); if (rc) return rc; }
    const VsdSurfelArgs sa = surfel_args(prm, c->nM, (size_t)n);
    const VsdRenderer rd = {render_surfels, &sa};
    return vsd_render_depth_with(c, F, rd, poses, n, depth);
}

int stocs::vsd_render_depth_with(stocs_ctx* c, DepthState* F, const VsdRenderer& rd, const float* poses, int n, float* depth) {
    DeviceGuard dev_guard(c->device);
    VsdState* S = ctx_state<VsdState>(c);
    const size_t npix = F->npix;
    // pieces of at most 32 MB of images (one at least): what the pinned block has to hold
    const size_t piece = std::min<size_t>(std::min<size_t>((size_t)n, chunk_poses(npix)), std::max<size_t>(1, ((size_t)32 << 20) / (4 * npix)));
    Carve cv;
    const size_t o_pose = cv.take(piece * 64), o_box = cv.take(piece * VSD_BOX_WORDS * 4), o_z = cv.take(piece * npix * 4);
    { const int rc = S->work.grow(c->stream, cv.total); if (rc) return rc; }
    char* hp;   // the pinned mirror of the regions, at the same offsets
    { const int rc = pinned_var(c, cv.total, &hp); if (rc) return rc; }
    float* d_pose = Carve::at<float>(S->work.p, o_pose);
    uint32_t* d_z = Carve::at<uint32_t>(S->work.p, o_z);
    int32_t* d_box = Carve::at<int32_t>(S->work.p, o_box);
    const DepthArgs a = frame_args(F, 1.0f, 0.0f);
    for (int h0 = 0; h0 < n; h0 += (int)piece) {
        const int m = std::min((int)piece, n - h0);
        memcpy(hp + o_pose, poses + (size_t)h0 * 16, (size_t)m * 64);
        STOCS_HIP_CHECK(hipMemcpyAsync(d_pose, hp + o_pose, (size_t)m * 64, hipMemcpyHostToDevice, c->stream));
        { const int rc = render_into(c, rd, d_pose, m, a, npix, d_z, d_box); if (rc) return rc; }
        STOCS_HIP_CHECK(hipMemcpyAsync(hp + o_z, d_z, (size_t)m * npix * 4, hipMemcpyDeviceToHost, c->stream));
        STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
        const uint32_t* bits = Carve::at<const uint32_t>(hp, o_z);
        float* out = depth + (size_t)h0 * npix;
        for (size_t i = 0; i < (size_t)m * npix; ++i) {   // bits to floats, empty to 0
            const uint32_t b = bits[i];
            float zf = 0.0f;
            if (b != 0xFFFFFFFFu) memcpy(&zf, &b, 4);
            out[i] = zf;
        }
    }
    return STOCS_OK;
}

extern "C" int stocs_pose_errors_vsd(stocs_ctx* c, const float* est, int n, const float* gt, int n_gt, const stocs_vsd_params* prm, stocs_vsd_record* out) {
    static const char* who = "stocs_pose_errors_vsd";
    { int rc; if (check_batch(who, c, n, &rc)) return rc; }
    { const int rc = check_pairs(who, est, n, gt, n_gt, out); if (rc) return rc; }
    if (!prm) { set_error("%s: NULL parameters", who); return STOCS_ERR_INVALID; }
    { const int rc = check_vsd(who, prm); if (rc) return rc; }
    { const int rc = check_model(who, c); if (rc) return rc; }
    DepthState* F = NULL;
    { const int rc = check_frame(who, c, &F); if (rc) return rc; }
    const VsdSurfelArgs sa = surfel_args(prm, c->nM, n_gt == 1 ? (size_t)n + 1 : 2 * (size_t)n);
    const VsdRenderer rd = {render_surfels, &sa};
    return vsd_pose_errors_with(c, F, TIMING_VSD, rd, est, n, gt, n_gt, prm, out);
}

int stocs::vsd_pose_errors_with(stocs_ctx* c, DepthState* F, TimingSlot timing_slot, const VsdRenderer& rd, const float* est, int n, const float* gt, int n_gt,
                                const stocs_vsd_params* prm, stocs_vsd_record* out) {
    DeviceGuard dev_guard(c->device);
    VsdState* S = ctx_state<VsdState>(c);
    TimedCall tc(c, timing_slot);
    const size_t npix = F->npix;
    const bool one_gt = n_gt == 1;
    // render order: one ground truth first and the estimates behind it, or (ground truth k, estimate k) pair by pair
    const size_t n_render = one_gt ? (size_t)n + 1 : 2 * (size_t)n;
    const size_t chunk = chunk_poses(npix);
    const int per = (int)std::min<size_t>((size_t)n, one_gt ? chunk : std::max<size_t>(1, chunk / 2));   // pairs per chunk
    const size_t slots = one_gt ? 1 + (size_t)per : 2 * (size_t)per;
    Carve cv;
    const size_t o_pose = cv.take(n_render * 64), o_cnt = cv.take((size_t)n * VSD_REC_WORDS * 4), o_box = cv.take(slots * VSD_BOX_WORDS * 4), o_z = cv.take(slots * npix * 4);
    { const int rc = S->work.grow(c->stream, cv.total); if (rc) return rc; }
    char* h_in; char* h_back;
    { const int rc = pinned_for(c, n_render * 64, (size_t)n * VSD_REC_WORDS * 4, &h_in, &h_back); if (rc) return rc; }
    float* d_pose = Carve::at<float>(S->work.p, o_pose);
    int32_t* d_cnt = Carve::at<int32_t>(S->work.p, o_cnt);
    uint32_t* d_z = Carve::at<uint32_t>(S->work.p, o_z);
    int32_t* d_box = Carve::at<int32_t>(S->work.p, o_box);   // a rectangle per z-buffer, in the same order
    const bool rects = !(vsd_form() & VSD_FORM_WHOLE_FRAMES);
    tc.start();   // (the first step counts the growing of the two blocks)
    if (one_gt) {
        memcpy(h_in, gt, 64);
        memcpy(h_in + 64, est, (size_t)n * 64);
    } else {
        for (int k = 0; k < n; ++k) {
            memcpy(h_in + (size_t)k * 128, gt + (size_t)k * 16, 64);
            memcpy(h_in + (size_t)k * 128 + 64, est + (size_t)k * 16, 64);
        }
    }
    STOCS_HIP_CHECK(hipMemcpyAsync(d_pose, h_in, n_render * 64, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(d_cnt, 0, (size_t)n * VSD_REC_WORDS * 4, c->stream));
    const DepthArgs a = frame_args(F, 1.0f, 0.0f);
    VsdCompareArgs va;
    va.delta = prm->delta; va.n_tau = prm->n_tau;
    for (int t = 0; t < STOCS_VSD_MAX_TAU; ++t) va.tau[t] = t < prm->n_tau ? prm->tau[t] : 0.0f;
    const unsigned cmp_blocks = (unsigned)((npix + 256 * VSD_ROUNDS_PER_BLOCK - 1) / (256 * VSD_ROUNDS_PER_BLOCK));
    { const int rc = tc.device_begin(); if (rc) return rc; }
    for (int k0 = 0; k0 < n; k0 += per) {
        const int m = std::min(per, n - k0);
        if (one_gt) {
            // the ground truth's buffer is slot 0 and its pose the first: the first chunk's launch renders it with its estimates
            const int lead = k0 == 0 ? 1 : 0;
            { const int rc = render_into(c, rd, d_pose + (size_t)(1 - lead + k0) * 16, m + lead, a, npix, d_z + (1 - lead) * npix, d_box + (1 - lead) * VSD_BOX_WORDS); if (rc) return rc; }
            hipLaunchKernelGGL(vsd_compare_kernel, dim3(cmp_blocks, (unsigned)m), dim3(256), 0, c->stream, (const uint32_t*)(d_z + npix), npix, (const uint32_t*)d_z, (size_t)0,
                               rects ? (const int32_t*)(d_box + VSD_BOX_WORDS) : (const int32_t*)NULL, (int)VSD_BOX_WORDS, (const int32_t*)d_box, 0, frame_depth(F), a, va,
                               d_cnt + (size_t)k0 * VSD_REC_WORDS);
        } else {
            { const int rc = render_into(c, rd, d_pose + (size_t)k0 * 32, 2 * m, a, npix, d_z, d_box); if (rc) return rc; }
            hipLaunchKernelGGL(vsd_compare_kernel, dim3(cmp_blocks, (unsigned)m), dim3(256), 0, c->stream, (const uint32_t*)(d_z + npix), 2 * npix, (const uint32_t*)d_z, 2 * npix,
                               rects ? (const int32_t*)(d_box + VSD_BOX_WORDS) : (const int32_t*)NULL, 2 * (int)VSD_BOX_WORDS, (const int32_t*)d_box, 2 * (int)VSD_BOX_WORDS,
                               frame_depth(F), a, va, d_cnt + (size_t)k0 * VSD_REC_WORDS);
        }
        STOCS_HIP_CHECK(hipGetLastError());
    }
    { const int rc = tc.device_end(); if (rc) return rc; }
    STOCS_HIP_CHECK(hipMemcpyAsync(h_back, d_cnt, (size_t)n * VSD_REC_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    { const int rc = tc.enqueued_wait(); if (rc) return rc; }
    for (int k = 0; k < n; ++k) {
        const int32_t* w = (const int32_t*)h_back + (size_t)k * VSD_REC_WORDS;
        stocs_vsd_record r;
        r.px_est = w[VC_PX_EST]; r.px_gt = w[VC_PX_GT]; r.vis_est = w[VC_VIS_EST]; r.vis_gt = w[VC_VIS_GT]; r.inter = w[VC_INTER]; r.uni = w[VC_UNI];
        for (int t = 0; t < STOCS_VSD_MAX_TAU; ++t) {
            r.far[t] = w[VC_FAR + t];
            r.e[t] = t < prm->n_tau ? (r.uni > 0 ? (float)(r.far[t] + (r.uni - r.inter)) / (float)r.uni : 1.0f) : 0.0f;
        }
        r.valid = pair_valid(est, gt, n_gt, k) ? 1 : 0;   // step 5 of stocs_pose_errors; the counts stand
        r.reserved = 0;
        out[k] = r;
    }
    return tc.finish();
}
