// mesh.hip -- the triangle mesh as a second model representation on the context (stocs_ctx_set_mesh), its exact, watertight depth
// rasteriser (stocs_render_depth_mesh) and VSD on it (stocs_pose_errors_vsd_mesh).  No reference counterpart.  The contract (float order,
// the edge rule, the z-buffer) is written down at the declarations in include/stocs_hip.h; tests/mesh_ref.py restates it in float32 numpy,
// and the results are equal bit for bit: a depth is a minimum of float bits, so a render depends on neither triangle order nor winding,
// batch, chunk or kernel form (which corner a triangle starts with may change the last bits of its depths, never its pixels: the contract).
//
// Everything around the render is vsd.hip's (vsd_shared.h): the chunks of z-buffers, the per-pose rectangles, the clears, the compare
// kernel and the record read-back.  This file only fills z-buffers -- and, for render_mesh.hip (render_shared.h), key buffers: the kernel
// and its helpers are templates on the pixel sink, DepthSink (a z-buffer of float bits per pose, 32-bit atomicMin) or KeySink (one buffer
// of (float bits << 32 | id) for all poses of the launch, 64-bit atomicMin, the id in a scalar register).  The set-up, the tiers and the
// forms below are the same text for both.  TriKeySink (refine_visible.hip) is the third: pose h has its own buffer of
// (float bits << 32 | triangle index), so the winner of a pixel names its facet.  It alone asks for the index (Sink::wants_tri): the
// extra readlane and the extra LDS array are behind `if constexpr`, and the other two instantiations are the instructions they were.
//   render    mesh_render_kernel: a workgroup of four wavefronts per (pose, 256 triangles), the pose in scalar registers.  A wavefront sets up
//             64 triangles, one per lane: three vertex gathers, the transform, the clamped box, the three edge normals.  Then per triangle:
//               small   a box of at most STOCS_MESH_SMALL_PX pixels: its lane walks it (a dense mesh: a handful of pixels per triangle, and
//                       64 of them at once)
//               wave    larger boxes, taken in turn (__ballot, lowest lane first): the sixteen values of the triangle go into scalar
//                       registers by readlane and all 64 lanes sweep the box in tiles of tw x 64 / tw pixels, tw the power of two that
//                       covers the box's width (at most 64): no division, no cap on the box
//               group   boxes above MESH_GROUP_PX pixels are put into LDS and, behind a barrier, swept by the four wavefronts together in
//                       tiles of tw x 256 / tw (a CAD model's face is thousands of passes of one wavefront)
//             One atomicMin per hit pixel (32-bit depths or 64-bit keys: the sink), blind or behind a read of the stored value (the stored value only falls, so a stale read
//             costs an atomic and never a result).  Each wavefront adds its triangles' boxes to the pose's rectangle: four atomicMax.
// STOCS_MESH_FORM=<bits> forces forms (mesh_form below); every form gives the same bits.
// Known limits: no near-plane clipping (a triangle with a vertex at or behind z = 1e-6 renders nothing); a group box is swept by one
// workgroup, so a call of one pose of a 12-triangle model runs on one compute unit; every vertex is transformed once per triangle that
// uses it (about six times on a closed mesh).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mesh_sample.h"
#include "eval_call.h"
#include "render_shared.h"
#include "wave_bits.h"

namespace stocs {

enum { MESH_SMALL_PX = STOCS_MESH_SMALL_PX, MESH_GROUP_PX = 8192, MESH_TRIS = 256, MESH_MAX_V = 1 << 24, MESH_MAX_T = 1 << 22 };

struct MeshState {
    static const StateOwner OWNER = OWN_MESH;
    ~MeshState() { verts.free(); tris.free(); }
    DevBlock verts;   // nv float4 (x, y, z, 0), grow-only
    DevBlock tris;    // nt int4 (i0, i1, i2, 0), grow-only
    int nv = 0, nt = 0;
};

struct MeshArgs { int nt, small_px, group_px, read_first; };

// the sixteen values of a set-up triangle
struct MeshTri {
    float a0, a1, a2, b0, b1, b2, c0, c1, c2;   // the edge normals nA = B x C, nB = C x A, nC = A x B
    float za, zb, zc;                           // A_2, B_2, C_2
    int c_lo, c_hi, r_lo, r_hi;
};

// Where a hit pixel goes.  The kernel and its helpers are templates on the sink; it is made per workgroup from the launch's Target and the
// pose blockIdx.y, so what it holds is uniform (scalar registers).
// DepthSink: pose h of the launch has its own z-buffer at zbuf + h * npix, a minimum of float bits (stocs_render_depth_mesh)
struct DepthSink {
    typedef uint32_t* Target;
    static constexpr bool wants_tri = false;
    uint32_t* z;
    __device__ __forceinline__ DepthSink(Target zbuf, int h, size_t npix) : z(zbuf + (size_t)h * npix) {}
    __device__ __forceinline__ void hit(size_t px, uint32_t bits, int read_first, int) const {
        uint32_t* cell = &z[px];
        if (!read_first || bits < *cell) atomicMin(cell, bits);
    }
};
// KeySink: every pose of the launch writes the one key buffer of stocs_render_poses_mesh, a minimum of (float bits << 32 | id)
struct KeyTarget { unsigned long long* zkey; int id_base; };
struct KeySink {
    typedef KeyTarget Target;
    static constexpr bool wants_tri = false;
    unsigned long long* z;
    unsigned long long id;
    __device__ __forceinline__ KeySink(Target t, int h, size_t) : z(t.zkey), id((unsigned long long)(unsigned)(t.id_base + h)) {}
    __device__ __forceinline__ void hit(size_t px, uint32_t bits, int read_first, int) const {
        unsigned long long* cell = &z[px];
        const unsigned long long key = ((unsigned long long)bits << 32) | id;
        if (!read_first || key < *cell) atomicMin(cell, key);
    }
};
// TriKeySink: pose h of the launch has its own key buffer at zkey + h * npix, a minimum of (float bits << 32 | triangle index): the
// nearest surface, on equal depth bits the lowest triangle (stocs_refine_poses_visible)
struct TriKeySink {
    typedef unsigned long long* Target;
    static constexpr bool wants_tri = true;
    unsigned long long* z;
    __device__ __forceinline__ TriKeySink(Target zkey, int h, size_t npix) : z(zkey + (size_t)h * npix) {}
    __device__ __forceinline__ void hit(size_t px, uint32_t bits, int read_first, int tri) const {
        unsigned long long* cell = &z[px];
        const unsigned long long key = ((unsigned long long)bits << 32) | (unsigned long long)(unsigned)tri;
        if (!read_first || key < *cell) atomicMin(cell, key);
    }
};

// step 4 of the contract for pixel (r, c), 0 <= r < H, 0 <= c < W
template <class Sink>
__device__ __forceinline__ void mesh_pixel(const Sink& z, const DepthArgs& a, int read_first, int r, int c, const MeshTri& t, int tri) {
    const float xn = ((float)c - a.cx) / a.fx, yn = ((float)r - a.cy) / a.fy;
    const float u = xn * t.a0 + (yn * t.a1 + t.a2);
    const float v = xn * t.b0 + (yn * t.b1 + t.b2);
    const float w = xn * t.c0 + (yn * t.c1 + t.c2);
    const float det = u + (v + w);
    const bool inside = (u >= 0.0f && v >= 0.0f && w >= 0.0f) || (u <= 0.0f && v <= 0.0f && w <= 0.0f);
    if (!inside || !(det != 0.0f)) return;
    const float zz = (u * t.za + (v * t.zb + w * t.zc)) / det;
    if (!(zz > 1e-6f)) return;
    z.hit((size_t)r * (size_t)a.W + (size_t)c, __float_as_uint(zz), read_first, tri);
}

// T = 1 << log_t threads (tid among them) sweep the box of t, whose values are uniform over them: tiles of tw x T / tw pixels
template <class Sink>
__device__ __forceinline__ void mesh_sweep(const Sink& z, const DepthArgs& a, int read_first, int tid, int log_t, const MeshTri& t, int tri) {
    const int w = t.c_hi - t.c_lo + 1;
    int log_w = 0;
    while (log_w < 6 && (1 << log_w) < w) ++log_w;   // uniform: at most six rounds
    const int tw = 1 << log_w, th = 1 << (log_t - log_w);
    const int dc = tid & (tw - 1), dr = tid >> log_w;
    for (int r0 = t.r_lo; r0 <= t.r_hi; r0 += th) {
        const int r = r0 + dr;
        for (int c0 = t.c_lo; c0 <= t.c_hi; c0 += tw) {
            const int c = c0 + dc;
            if (r <= t.r_hi && c <= t.c_hi) mesh_pixel(z, a, read_first, r, c, t, tri);   // inside the clamped box: inside the frame
        }
    }
}

__device__ __forceinline__ float uniform_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// target: where pose blockIdx.y of the launch writes (DepthSink, KeySink); its rectangle at box + blockIdx.y * VSD_BOX_WORDS
template <class Sink>
__global__ __launch_bounds__(256) void mesh_render_kernel(const float* __restrict__ poses, const float4* __restrict__ verts, const int4* __restrict__ tris, DepthArgs a, MeshArgs ma,
                                                          typename Sink::Target target, int32_t* __restrict__ box) {
    __shared__ float g_val[12][MESH_TRIS];
    __shared__ int g_box[4][MESH_TRIS];
    __shared__ int g_n;
    __shared__ int g_tri[Sink::wants_tri ? MESH_TRIS : 1];   // the triangle of a slot, for the sink that keeps it
    const int h = (int)blockIdx.y;
    float P[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = poses[(size_t)h * 16 + i];   // the same address in every lane: uniform loads
    if (!pose_finite(P)) return;                                      // the whole workgroup: no barrier is left behind
    const Sink z(target, h, (size_t)a.W * (size_t)a.H);
    const int tid = (int)threadIdx.x, lane = tid & 63;
    if (tid == 0) g_n = 0;
    __syncthreads();
    const int i = (int)blockIdx.x * MESH_TRIS + tid;
    MeshTri t;
    t.a0 = t.a1 = t.a2 = t.b0 = t.b1 = t.b2 = t.c0 = t.c1 = t.c2 = 0.0f; t.za = t.zb = t.zc = 1.0f;
    t.c_lo = t.r_lo = 0; t.c_hi = t.r_hi = -1;
    bool live = false;
    if (i < ma.nt) {
        const int4 id = tris[i];   // 0 <= id.x, id.y, id.z < nv: stocs_ctx_set_mesh refuses anything else
        const float4 va = verts[id.x], vb = verts[id.y], vc = verts[id.z];
        const float A0 = (P[0] * va.x + (P[4] * va.y + P[8] * va.z)) + P[12], A1 = (P[1] * va.x + (P[5] * va.y + P[9] * va.z)) + P[13], A2 = (P[2] * va.x + (P[6] * va.y + P[10] * va.z)) + P[14];
        const float B0 = (P[0] * vb.x + (P[4] * vb.y + P[8] * vb.z)) + P[12], B1 = (P[1] * vb.x + (P[5] * vb.y + P[9] * vb.z)) + P[13], B2 = (P[2] * vb.x + (P[6] * vb.y + P[10] * vb.z)) + P[14];
        const float C0 = (P[0] * vc.x + (P[4] * vc.y + P[8] * vc.z)) + P[12], C1 = (P[1] * vc.x + (P[5] * vc.y + P[9] * vc.z)) + P[13], C2 = (P[2] * vc.x + (P[6] * vc.y + P[10] * vc.z)) + P[14];
        const bool finite = isfinite(A0) && isfinite(A1) && isfinite(A2) && isfinite(B0) && isfinite(B1) && isfinite(B2) && isfinite(C0) && isfinite(C1) && isfinite(C2);
        if (finite && A2 > 1e-6f && B2 > 1e-6f && C2 > 1e-6f) {
            const float xa = (a.fx * A0) / A2 + a.cx, xb = (a.fx * B0) / B2 + a.cx, xc = (a.fx * C0) / C2 + a.cx;
            const float ya = (a.fy * A1) / A2 + a.cy, yb = (a.fy * B1) / B2 + a.cy, yc = (a.fy * C1) / C2 + a.cy;
            const float c_lo = fmaxf(floorf(fminf(xa, fminf(xb, xc))) - 1.0f, 0.0f), c_hi = fminf(floorf(fmaxf(xa, fmaxf(xb, xc))) + 2.0f, (float)(a.W - 1));
            const float r_lo = fmaxf(floorf(fminf(ya, fminf(yb, yc))) - 1.0f, 0.0f), r_hi = fminf(floorf(fmaxf(ya, fmaxf(yb, yc))) + 2.0f, (float)(a.H - 1));
            if (c_lo <= c_hi && r_lo <= r_hi) {   // in float: 0 <= lo <= hi <= W - 1 (H - 1), so the conversions are exact
                live = true;
                t.c_lo = (int)c_lo; t.c_hi = (int)c_hi; t.r_lo = (int)r_lo; t.r_hi = (int)r_hi;
                t.a0 = B1 * C2 - B2 * C1; t.a1 = B2 * C0 - B0 * C2; t.a2 = B0 * C1 - B1 * C0;
                t.b0 = C1 * A2 - C2 * A1; t.b1 = C2 * A0 - C0 * A2; t.b2 = C0 * A1 - C1 * A0;
                t.c0 = A1 * B2 - A2 * B1; t.c1 = A2 * B0 - A0 * B2; t.c2 = A0 * B1 - A1 * B0;
                t.za = A2; t.zb = B2; t.zc = C2;
            }
        }
    }
    // npx as a 64-bit product: W and H are ints, their product need not be
    const long long npx = live ? (long long)(t.c_hi - t.c_lo + 1) * (long long)(t.r_hi - t.r_lo + 1) : 0;
    const bool small = live && npx <= (long long)ma.small_px;
    const bool group = live && !small && npx > (long long)ma.group_px;
    if (small) {   // this lane's own box
        for (int r = t.r_lo; r <= t.r_hi; ++r)
            for (int c = t.c_lo; c <= t.c_hi; ++c) mesh_pixel(z, a, ma.read_first, r, c, t, i);
    }
    unsigned long long todo = __ballot(live && !small && !group);
    while (todo) {   // wave-uniform: one triangle at a time, in scalar registers
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        MeshTri s;
        s.a0 = lane_f(t.a0, src); s.a1 = lane_f(t.a1, src); s.a2 = lane_f(t.a2, src);
        s.b0 = lane_f(t.b0, src); s.b1 = lane_f(t.b1, src); s.b2 = lane_f(t.b2, src);
        s.c0 = lane_f(t.c0, src); s.c1 = lane_f(t.c1, src); s.c2 = lane_f(t.c2, src);
        s.za = lane_f(t.za, src); s.zb = lane_f(t.zb, src); s.zc = lane_f(t.zc, src);
        s.c_lo = lane_i(t.c_lo, src); s.c_hi = lane_i(t.c_hi, src); s.r_lo = lane_i(t.r_lo, src); s.r_hi = lane_i(t.r_hi, src);
        int s_tri = 0;
        if constexpr (Sink::wants_tri) s_tri = lane_i(i, src);
        mesh_sweep(z, a, ma.read_first, lane, 6, s, s_tri);
    }
    if (group) {   // at most one per thread: slot < MESH_TRIS
        const int slot = atomicAdd(&g_n, 1);
        g_val[0][slot] = t.a0; g_val[1][slot] = t.a1; g_val[2][slot] = t.a2; g_val[3][slot] = t.b0; g_val[4][slot] = t.b1; g_val[5][slot] = t.b2;
        g_val[6][slot] = t.c0; g_val[7][slot] = t.c1; g_val[8][slot] = t.c2; g_val[9][slot] = t.za; g_val[10][slot] = t.zb; g_val[11][slot] = t.zc;
        g_box[0][slot] = t.c_lo; g_box[1][slot] = t.c_hi; g_box[2][slot] = t.r_lo; g_box[3][slot] = t.r_hi;
        if constexpr (Sink::wants_tri) g_tri[slot] = i;
    }
    __syncthreads();   // every thread of the workgroup arrives: nothing above returns after the first barrier
    const int n_group = g_n;
    for (int e = 0; e < n_group; ++e) {   // workgroup-uniform
        MeshTri s;
        s.a0 = uniform_f(g_val[0][e]); s.a1 = uniform_f(g_val[1][e]); s.a2 = uniform_f(g_val[2][e]);
        s.b0 = uniform_f(g_val[3][e]); s.b1 = uniform_f(g_val[4][e]); s.b2 = uniform_f(g_val[5][e]);
        s.c0 = uniform_f(g_val[6][e]); s.c1 = uniform_f(g_val[7][e]); s.c2 = uniform_f(g_val[8][e]);
        s.za = uniform_f(g_val[9][e]); s.zb = uniform_f(g_val[10][e]); s.zc = uniform_f(g_val[11][e]);
        s.c_lo = __builtin_amdgcn_readfirstlane(g_box[0][e]); s.c_hi = __builtin_amdgcn_readfirstlane(g_box[1][e]);
        s.r_lo = __builtin_amdgcn_readfirstlane(g_box[2][e]); s.r_hi = __builtin_amdgcn_readfirstlane(g_box[3][e]);
        int s_tri = 0;
        if constexpr (Sink::wants_tri) s_tri = __builtin_amdgcn_readfirstlane(g_tri[e]);
        mesh_sweep(z, a, ma.read_first, tid, 8, s, s_tri);
    }
    // the pose's rectangle: the union of the live triangles' boxes
    int b_nc0 = live ? -t.c_lo : (int)0x80808080, b_c1 = live ? t.c_hi : (int)0x80808080, b_nr0 = live ? -t.r_lo : (int)0x80808080, b_r1 = live ? t.r_hi : (int)0x80808080;
    b_nc0 = wave_max_i(b_nc0); b_c1 = wave_max_i(b_c1); b_nr0 = wave_max_i(b_nr0); b_r1 = wave_max_i(b_r1);
    if (lane == 0 && b_c1 >= 0) {
        int32_t* bx = box + (size_t)h * VSD_BOX_WORDS;
        atomicMax(&bx[VB_NEG_C0], b_nc0); atomicMax(&bx[VB_C1], b_c1); atomicMax(&bx[VB_NEG_R0], b_nr0); atomicMax(&bx[VB_R1], b_r1);
    }
}

// STOCS_MESH_FORM=<bits> in the environment chooses the kernel's forms, for measurements and for the tests; no bit changes a result.
// 1: every box up to MESH_GROUP_PX pixels is walked by its own lane; 2: every box is swept by a wavefront or the workgroup, none by its
// lane; 4: every hit pixel reads the stored depth before its atomicMin, 8: none does (neither: none does);
// 16: no box goes to the workgroup (a wavefront sweeps the largest too)
enum { MESH_FORM_LANES_OWN = 1, MESH_FORM_COOPERATIVE = 2, MESH_FORM_READ_FIRST = 4, MESH_FORM_BLIND = 8, MESH_FORM_NO_GROUP = 16 };
// Reading first lost or tied in every measured row (profiles/mesh_forms.json): a closed mesh puts two or three triangles on a
// pixel where 6 mm surfels put a dozen, so the read saves few atomics.  The atomics go out blind unless the form says otherwise.
static int mesh_form() {
    const char* e = getenv("STOCS_MESH_FORM");
    return e ? atoi(e) : 0;
}

static MeshArgs mesh_args(int nt) {
    MeshArgs m;
    const int form = mesh_form();
    m.nt = nt;
    int small_px = (int)MESH_SMALL_PX;
    if (const char* e = getenv("STOCS_MESH_SMALL_PX")) { const int v = atoi(e); if (v >= 0 && v <= (int)MESH_GROUP_PX) small_px = v; }   // measurements only (tools/mesh_time.py)
    m.small_px = (form & MESH_FORM_COOPERATIVE) ? 0 : (form & MESH_FORM_LANES_OWN) ? (int)MESH_GROUP_PX : small_px;
    m.group_px = (form & MESH_FORM_NO_GROUP) ? 0x7FFFFFFF : (int)MESH_GROUP_PX;
    m.read_first = (form & MESH_FORM_BLIND) ? 0 : (form & MESH_FORM_READ_FIRST) ? 1 : 0;
    return m;
}

// the mesh renderer as a VsdRenderer: self is the call's MeshArgs
static int render_mesh(stocs_ctx* c, const void* self, const float* d_pose, int m, const DepthArgs& a, uint32_t* d_z, int32_t* d_box) {
    const MeshArgs& ma = *(const MeshArgs*)self;
    const MeshState* S = ctx_state_if<MeshState>(c);
    const unsigned tri_chunks = (unsigned)((ma.nt + MESH_TRIS - 1) / MESH_TRIS);
    hipLaunchKernelGGL(mesh_render_kernel<DepthSink>, dim3(tri_chunks, (unsigned)m), dim3(256), 0, c->stream, d_pose, (const float4*)S->verts.p, (const int4*)S->tris.p, a, ma, d_z,
                       d_box);
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

int mesh_enqueue_depth(stocs_ctx* c, const float* d_pose, int m, const DepthArgs& a, uint32_t* d_z, int32_t* d_box) {
    const MeshArgs ma = mesh_args(ctx_state_if<MeshState>(c)->nt);
    return render_mesh(c, &ma, d_pose, m, a, d_z, d_box);
}

int mesh_enqueue_keys(stocs_ctx* c, const float* d_pose, int m, const DepthArgs& a, int id_base, unsigned long long* d_zkey, int32_t* d_box) {
    const MeshState* S = ctx_state_if<MeshState>(c);
    const MeshArgs ma = mesh_args(S->nt);
    const unsigned tri_chunks = (unsigned)((ma.nt + MESH_TRIS - 1) / MESH_TRIS);
    // the pose is blockIdx.y (at most 65 535 per launch)
    for (int h0 = 0; h0 < m; h0 += 65535) {
        const int mh = m - h0 < 65535 ? m - h0 : 65535;
        const KeyTarget target = {d_zkey, id_base + h0};
        hipLaunchKernelGGL(mesh_render_kernel<KeySink>, dim3(tri_chunks, (unsigned)mh), dim3(256), 0, c->stream, d_pose + (size_t)h0 * 16, (const float4*)S->verts.p,
                           (const int4*)S->tris.p, a, ma, target, d_box + (size_t)h0 * VSD_BOX_WORDS);
        STOCS_HIP_CHECK(hipGetLastError());
    }
    return STOCS_OK;
}

int mesh_enqueue_tri_keys(stocs_ctx* c, const float* d_pose, int m, const DepthArgs& a, unsigned long long* d_zkey, int32_t* d_box) {
    const MeshState* S = ctx_state_if<MeshState>(c);
    const MeshArgs ma = mesh_args(S->nt);
    const unsigned tri_chunks = (unsigned)((ma.nt + MESH_TRIS - 1) / MESH_TRIS);
    // the pose is blockIdx.y: m <= 65 535, the caller's chunks see to that
    hipLaunchKernelGGL(mesh_render_kernel<TriKeySink>, dim3(tri_chunks, (unsigned)m), dim3(256), 0, c->stream, d_pose, (const float4*)S->verts.p, (const int4*)S->tris.p, a, ma,
                       d_zkey, d_box);
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

// the mesh on the device for a kernel that reads facets by index (refine_visible.hip): nt int4 triangles, float4 vertices
void mesh_device_arrays(const stocs_ctx* c, const float4** verts, const int4** tris) {
    const MeshState* S = ctx_state_if<MeshState>(c);
    *verts = (const float4*)S->verts.p; *tris = (const int4*)S->tris.p;
}

int mesh_triangles(const stocs_ctx* c) { const MeshState* S = ctx_state_if<MeshState>(c); return S ? S->nt : 0; }

int mesh_check_present(const char* who, stocs_ctx* c) {
    const MeshState* S = ctx_state_if<MeshState>(c);
    if (!S || S->nt < 1) { set_error("%s: the context has no mesh (stocs_ctx_set_mesh)", who); return STOCS_ERR_STATE; }
    return STOCS_OK;
}

}  // namespace stocs

using namespace stocs;

extern "C" int stocs_mesh_small_px(void) { return (int)MESH_SMALL_PX; }

int stocs::mesh_check_as(const char* who, const float* pos3, int nv, const int32_t* tris3, int nt, bool finite_vertices) {
    if (nv < 0 || nt < 0) { set_error("%s: nv %d or nt %d < 0", who, nv, nt); return STOCS_ERR_INVALID; }
    if ((nv && !pos3) || (nt && !tris3)) { set_error("%s: NULL vertices or triangles", who); return STOCS_ERR_INVALID; }
    if (nv > MESH_MAX_V || nt > MESH_MAX_T) { set_error("%s: %d vertices, %d triangles above %d, %d", who, nv, nt, (int)MESH_MAX_V, (int)MESH_MAX_T); return STOCS_ERR_CAPACITY; }
    for (size_t k = 0; finite_vertices && k < (size_t)nv * 3; ++k)
        if (!isfinite(pos3[k])) { set_error("%s: vertex %zu is not finite", who, k / 3); return STOCS_ERR_INVALID; }
    for (size_t k = 0; k < (size_t)nt * 3; ++k)
        if (tris3[k] < 0 || tris3[k] >= nv) { set_error("%s: triangle %zu has index %d outside 0..%d", who, k / 3, (int)tris3[k], nv - 1); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}

extern "C" int stocs_mesh_check(const float* pos3, int nv, const int32_t* tris3, int nt) { return mesh_check_as("stocs_mesh_check", pos3, nv, tris3, nt, true); }

extern "C" int stocs_ctx_set_mesh(stocs_ctx* c, const float* pos3, int nv, const int32_t* tris3, int nt) {
    static const char* who = "stocs_ctx_set_mesh";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (nv < 0 || nt < 0) { set_error("%s: nv %d or nt %d < 0", who, nv, nt); return STOCS_ERR_INVALID; }
    if (nt == 0) {   // drops the mesh; the blocks stay for the next one
        if (MeshState* S = ctx_state_if<MeshState>(c)) { S->nv = 0; S->nt = 0; }
        return STOCS_OK;
    }
    if (!pos3 || !tris3) { set_error("%s: NULL vertices or triangles", who); return STOCS_ERR_INVALID; }
    { const int rc = stocs_mesh_check(pos3, nv, tris3, nt); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    MeshState* S = ctx_state<MeshState>(c);
    S->nv = 0; S->nt = 0;   // a failure below leaves no mesh
    { const int rc = S->verts.grow(c->stream, (size_t)nv * 16); if (rc) return rc; }
    { const int rc = S->tris.grow(c->stream, (size_t)nt * 16); if (rc) return rc; }
    char* hp;
    const size_t o_t = al256((size_t)nv * 16);
    { const int rc = pinned_var(c, o_t + (size_t)nt * 16, &hp); if (rc) return rc; }
    float* hv = (float*)hp;
    int32_t* ht = (int32_t*)(hp + o_t);
    for (int i = 0; i < nv; ++i) { hv[4 * i] = pos3[3 * i]; hv[4 * i + 1] = pos3[3 * i + 1]; hv[4 * i + 2] = pos3[3 * i + 2]; hv[4 * i + 3] = 0.0f; }
    for (int i = 0; i < nt; ++i) { ht[4 * i] = tris3[3 * i]; ht[4 * i + 1] = tris3[3 * i + 1]; ht[4 * i + 2] = tris3[3 * i + 2]; ht[4 * i + 3] = 0; }
    STOCS_HIP_CHECK(hipMemcpyAsync(S->verts.p, hv, (size_t)nv * 16, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemcpyAsync(S->tris.p, ht, (size_t)nt * 16, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));   // the pinned block is the next call's to overwrite
    S->nv = nv; S->nt = nt;
    return STOCS_OK;
}

extern "C" int stocs_ctx_mesh_info(const stocs_ctx* c, int* nv, int* nt) {
    if (!c) { set_error("stocs_ctx_mesh_info: NULL context"); return STOCS_ERR_INVALID; }
    const MeshState* S = ctx_state_if<MeshState>(c);
    if (nv) *nv = S ? S->nv : 0;
    if (nt) *nt = S ? S->nt : 0;
    return STOCS_OK;
}

extern "C" int stocs_render_depth_mesh(stocs_ctx* c, const float* poses, int n, float* depth) {
    static const char* who = "stocs_render_depth_mesh";
    { int rc; if (check_batch(who, c, n, &rc)) return rc; }
    if (!poses || !depth) { set_error("%s: NULL poses or images", who); return STOCS_ERR_INVALID; }
    { const int rc = mesh_check_present(who, c); if (rc) return rc; }
    DepthState* F = NULL;
    { const int rc = check_frame(who, c, &F); if (rc) return rc; }
    const MeshArgs ma = mesh_args(ctx_state_if<MeshState>(c)->nt);
    const VsdRenderer rd = {render_mesh, &ma};
    return vsd_render_depth_with(c, F, rd, poses, n, depth);
}

extern "C" int stocs_pose_errors_vsd_mesh(stocs_ctx* c, const float* est, int n, const float* gt, int n_gt, const stocs_vsd_params* prm, stocs_vsd_record* out) {
    static const char* who = "stocs_pose_errors_vsd_mesh";
    { int rc; if (check_batch(who, c, n, &rc)) return rc; }
    { const int rc = check_pairs(who, est, n, gt, n_gt, out); if (rc) return rc; }
    if (!prm) { set_error("%s: NULL parameters", who); return STOCS_ERR_INVALID; }
    { const int rc = vsd_check_compare_params(who, prm); if (rc) return rc; }   // surfel_radius and max_splat_px are not read
    { const int rc = mesh_check_present(who, c); if (rc) return rc; }
    DepthState* F = NULL;
    { const int rc = check_frame(who, c, &F); if (rc) return rc; }
    const MeshArgs ma = mesh_args(ctx_state_if<MeshState>(c)->nt);
    const VsdRenderer rd = {render_mesh, &ma};
    return vsd_pose_errors_with(c, F, TIMING_VSD_MESH, rd, est, n, gt, n_gt, prm, out);
}
