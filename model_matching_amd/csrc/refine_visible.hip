// refine_visible.hip -- projective, point-to-plane refinement of camera-frame poses of the context's mesh against the frame of
// stocs_ctx_set_frame (stocs_refine_poses_visible, stocs_refine_visible_detail).  No reference counterpart.  Association is by pixel: the
// model point of a pixel is the surface the rasteriser sees there at the current hypothesis, its normal the exact normal of the facet that
// won the pixel, its partner the depth pixel on the same ray.  The contract (float order, the gates, the row, the 29 sums, the update) is
// written down at the declarations in include/stocs_hip.h; tests/refine_visible_ref.py restates it in numpy: keys and states are equal
// bit for bit, sums and poses within the rounding bounds of the double sums.
//
// Per chunk of poses (256 MB of key buffers; STOCS_REFINE_VISIBLE_CHUNK=<poses> forces a size) and per iteration, chained on the stream:
//   render      mesh.hip's rasteriser with its triangle-key sink (mesh_enqueue_tri_keys): pose h fills its own buffer of
//               (float bits << 32 | triangle index) and leaves its rectangle.
//   accumulate  a grid of (G workgroups, pose), G a function of the frame's size alone (refine_visible_groups), the pose in scalar
//               registers.  Workgroup g takes rows r0 + g, r0 + g + G, ... of the pose's rectangle, read from the box words on the device;
//               its four wavefronts take the rows' runs of 64 pixels in turn.  Per pixel: one 8-byte key load; where a key is present the
//               depth (and class) load, the int4 of the triangle, its three vertex gathers, the gates in float, the row in double.  Each
//               lane keeps the 29 sums in double; counts are __ballot + __popcll in wave-uniform registers.  A butterfly over the wavefront,
//               the four waves in order: one partial per workgroup, no float atomics.  The shipping form puts the empty key back into every
//               pixel it found set, so the buffer is clear again for the next iteration's render: only what a render wrote is cleared,
//               the whole chunk once per call.
//   solve       one wavefront per hypothesis: lane l sums partials l, l + 64, ..., a butterfly, solve6, the float pose in place (the next
//               render reads it), the record.
// A hypothesis's walk depends on its rectangle and on G alone, so its result is bitwise independent of the batch, of its position in it
// and of the chunk.  The detail form (a compile-time argument, as in refine.hip) stops after the sums, writes the per-pixel state and
// leaves the keys in place for the read-back.
// The damped form (stocs_refine_poses_visible_damped; tests/refine_visible_damped_ref.py) runs the same render and the same
// accumulation K + 1 times and puts another kernel in the solve's place; the contour form (stocs_refine_poses_visible_contour, DESIGN
// 7.22; tests/refine_visible_contour_ref.py) is the damped form with one more kernel per evaluation.  One solve kernel serves both:
//   damped solve  one wavefront per hypothesis: the solve's reduction, then lane 0 in double: the cost, accept or reject against the pose's
//               accepted state (pose, 29 sums, cost, lambda, kept in the workspace), and from it the sums moved to a pivot on the object, the
//               damped 6x6 solve, the bound and the next trial pose in the slot the next render reads (rv_damped_decide); a trace row when
//               asked for.  As the contour form (a compile-time argument) it reduces both sets of partials, decides on M = S + w Sc with the
//               cost over the object pixels, and fills the record's contour fields from that decision.
//   object count  once per call: N_O, the frame's pixels with a measurement and a class probability at the threshold, by __ballot.
//   contour     between the render and the accumulation (which clears the keys), on the accumulation's grid: the pose's rectangle grown
//               by the pull radius in tiles of 16 rows x 64 columns; per tile with an uncovered object pixel, "key present" of the tile and
//               its halo as bit rows in LDS (one __ballot per 64 keys), per pixel the nearest set bit of each row of the window by
//               count-leading/trailing-zeros under the minimum of (d2, linear index), one key load for the winner's depth, the 3-D gate,
//               three point-to-point rows in double; 29 sums and three counts per workgroup in the accumulation's fixed order.
// Host: the batch entry points are their checks and one frame (VisibleCall): workspace, staging, per chunk and evaluation
// render, contour pass, accumulation, the form's solve; one read-back, one event read-out.  Blocks: workspace, DampedWork, DetailWork.
// Known limits: the plain step is an undamped Gauss-Newton step whose rotation is about the camera's origin: on a solid whose visible surface
// constrains a motion weakly it can be large and leave the pose worse (measured on the Cm solid; the restatement does the
// same, bit for bit; the damped form is the remedy); a frozen hypothesis is still rendered and walked in the remaining iterations of its chunk (nothing reads the result);
// the rasteriser's limits (no near-plane clipping; one pose of a 12-triangle model renders on one compute unit) are this file's too.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "render_shared.h"
#include "solve6.h"

namespace stocs {

enum { RV_SUMS = 29, RV_COUNTS = 5, RV_MAX_GROUPS = 64 };
enum { RV_PRESENT = 0, RV_NO_DEPTH, RV_OFF_CLASS, RV_TOO_FAR, RV_GRAZING };   // the integer counts of a partial; counted is sum 27
static const unsigned long long RV_EMPTY = 0xFFFFFFFFFFFFFFFFull;

struct RefineVisibleState {
    static const StateOwner OWNER = OWN_REFINE_VISIBLE;
    ~RefineVisibleState() { work.free(); detail.free(); damped.free(); }
    DevBlock work;     // poses | records | frozen flags | rectangles | partial sums | partial counts | one chunk of key buffers, grow-only
    DevBlock detail;   // both detail entry points (DetailWork): nearest | state | sums | contour partials, grow-only
    DevBlock damped;   // the damped and the contour form (DampedWork): accepted poses | records | trace | accepted sums, cost, lambda | done flags | contour partials | N_O, grow-only
    float last_ms[3] = {-1.0f, -1.0f, -1.0f};  // "device_clock": HIP-event time of the last call's last render, accumulation and solve (-1: not taken)
    float last_contour_ms = -1.0f;             // the same of the last call's last contour pass
};

struct RvArgs {
    float max_d2;      // max_distance * max_distance, in float
    float min_cos2;    // min_view_cos * min_view_cos, in float
    int groups;        // G
};

struct RvNoDetail { static constexpr bool on = false; };
struct RvDetailOut {
    static constexpr bool on = true;
    uint8_t* state;    // H * W, preset 0
    double* sums29;
};

// G: workgroups per pose of the accumulation, from the frame's size alone (one per 2048 pixels, at most 64)
static int refine_visible_groups(size_t npix) { return (int)std::min<size_t>(std::max<size_t>(npix >> 11, 1), (size_t)RV_MAX_GROUPS); }

// steps 1-4 of the contract for the pixel at (r, c) whose key is set: its state, and for a counted pixel its 29 products added to v
__device__ __forceinline__ int rv_pixel(const float* P, const float4* __restrict__ verts, const int4* __restrict__ tris, const uint16_t* __restrict__ depth,
                                        const uint16_t* __restrict__ prob, const DepthArgs& a, const RvArgs& ra, int r, int c, size_t px, unsigned long long key,
                                        double* v) {
    const uint16_t raw = depth[px];
    if (raw == 0) return 1;
    if (prob) {
        const float cp = (float)((double)prob[px] * (1.0 / 10000));
        if (cp < a.class_threshold) return 2;
    }
    const float xn = ((float)c - a.cx) / a.fx, yn = ((float)r - a.cy) / a.fy;
    const float z = __uint_as_float((uint32_t)(key >> 32));
    const float d = (float)raw * a.depth_scale;
    const float p0 = xn * z, p1 = yn * z, q0 = xn * d, q1 = yn * d;
    const float e0 = p0 - q0, e1 = p1 - q1, e2 = z - d;
    const float D = e0 * e0 + (e1 * e1 + e2 * e2);
    if (D > ra.max_d2) return 3;
    const int4 id = tris[(uint32_t)key];   // a key's low word is the index of a triangle of the mesh: only the rasteriser writes keys
    const float4 va = verts[id.x], vb = verts[id.y], vc = verts[id.z];
    const float A0 = (P[0] * va.x + (P[4] * va.y + P[8] * va.z)) + P[12], A1 = (P[1] * va.x + (P[5] * va.y + P[9] * va.z)) + P[13], A2 = (P[2] * va.x + (P[6] * va.y + P[10] * va.z)) + P[14];
    const float B0 = (P[0] * vb.x + (P[4] * vb.y + P[8] * vb.z)) + P[12], B1 = (P[1] * vb.x + (P[5] * vb.y + P[9] * vb.z)) + P[13], B2 = (P[2] * vb.x + (P[6] * vb.y + P[10] * vb.z)) + P[14];
    const float C0 = (P[0] * vc.x + (P[4] * vc.y + P[8] * vc.z)) + P[12], C1 = (P[1] * vc.x + (P[5] * vc.y + P[9] * vc.z)) + P[13], C2 = (P[2] * vc.x + (P[6] * vc.y + P[10] * vc.z)) + P[14];
    const float u0 = B0 - A0, u1 = B1 - A1, u2 = B2 - A2, w0 = C0 - A0, w1 = C1 - A1, w2 = C2 - A2;
    const float m0 = u1 * w2 - u2 * w1, m1 = u2 * w0 - u0 * w2, m2 = u0 * w1 - u1 * w0;
    const float s = m0 * p0 + (m1 * p1 + m2 * z);
    const float mm = m0 * m0 + (m1 * m1 + m2 * m2);
    const float pp = p0 * p0 + (p1 * p1 + z * z);
    if (!(mm != 0.0f) || s * s < ra.min_cos2 * (mm * pp)) return 4;
    // counted: the row in double from the floats above
    const double dm0 = m0, dm1 = m1, dm2 = m2;
    const double len = sqrt(dm0 * dm0 + (dm1 * dm1 + dm2 * dm2));
    const double sg = s > 0.0f ? -1.0 : 1.0;
    const double n0 = (sg * dm0) / len, n1 = (sg * dm1) / len, n2 = (sg * dm2) / len;
    const double qx = q0, qy = q1, qz = d;
    const double ar[6] = {qy * n2 - qz * n1, qz * n0 - qx * n2, qx * n1 - qy * n0, n0, n1, n2};   // [q x n, n]
    const double b = (n0 * (qx - (double)p0) + n1 * (qy - (double)p1)) + n2 * (qz - (double)z);
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { v[k] += ar[i] * ar[j]; ++k; }
#pragma unroll
    for (int i = 0; i < 6; ++i) v[21 + i] += ar[i] * b;
    v[27] += 1.0;
    v[28] += b * b;
    return 5;
}

// Pose blockIdx.y of the chunk: its keys at zkey + blockIdx.y * npix, its rectangle at box + blockIdx.y * VSD_BOX_WORDS, its partials at
// partial + (blockIdx.y * G + blockIdx.x) * RV_SUMS and pcount + (blockIdx.y * G + blockIdx.x) * RV_COUNTS.  The loop bounds are
// wave-uniform, so every __ballot sees the whole wavefront.  Every workgroup writes its partial: a pose that rendered nothing has zeros.
template <class Detail>
__global__ __launch_bounds__(256) void refine_visible_accumulate_kernel(const float* __restrict__ poses, const float4* __restrict__ verts, const int4* __restrict__ tris,
                                                                        unsigned long long* __restrict__ zkey, const int32_t* __restrict__ box,
                                                                        const uint16_t* __restrict__ depth, const uint16_t* __restrict__ prob, DepthArgs a, RvArgs ra,
                                                                        double* __restrict__ partial, int32_t* __restrict__ pcount, Detail det) {
    __shared__ double red[4][RV_SUMS];
    __shared__ int cnt[4][RV_COUNTS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = (int)blockIdx.y, g = (int)blockIdx.x;
    float P[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = poses[(size_t)h * 16 + i];   // the same address in every lane: uniform loads
    const int32_t* bx = box + (size_t)h * VSD_BOX_WORDS;
    const int c0 = -bx[VB_NEG_C0], c1 = bx[VB_C1], r0 = -bx[VB_NEG_R0], r1 = bx[VB_R1];
    // a rendered pose: 0 <= c0 <= c1 <= W - 1 and 0 <= r0 <= r1 <= H - 1, the union of clamped boxes; nothing rendered: c1 < 0
    const bool any = c1 >= 0 && c1 >= c0 && r1 >= r0 && r0 + g <= r1;
    const int n_runs = any ? (c1 - c0 + 64) >> 6 : 0;
    const int n_rows = any ? (r1 - (r0 + g)) / ra.groups + 1 : 0;
    const int n_items = n_rows * n_runs;   // at most H * (W / 64 + 1)
    unsigned long long* zk = zkey + (size_t)h * ((size_t)a.W * (size_t)a.H);
    double v[RV_SUMS];
#pragma unroll
    for (int k = 0; k < RV_SUMS; ++k) v[k] = 0.0;
    int n_present = 0, n_nod = 0, n_off = 0, n_far = 0, n_graze = 0;
    for (int item = wave; item < n_items; item += 4) {
        const int row = item / n_runs, run = item - row * n_runs;
        const int r = r0 + g + row * ra.groups, c = c0 + run * 64 + lane;
        int st = 0;
        if (c <= c1) {
            const size_t px = (size_t)r * (size_t)a.W + (size_t)c;
            const unsigned long long key = zk[px];
            if (key != RV_EMPTY) {
                st = rv_pixel(P, verts, tris, depth, prob, a, ra, r, c, px, key, v);
                if constexpr (Detail::on) det.state[px] = (uint8_t)st;
                else zk[px] = RV_EMPTY;   // what the render wrote is cleared for the next one
            }
        }
        n_present += __popcll(__ballot(st != 0)); n_nod += __popcll(__ballot(st == 1)); n_off += __popcll(__ballot(st == 2));
        n_far += __popcll(__ballot(st == 3)); n_graze += __popcll(__ballot(st == 4));
    }
    // the reduction in a fixed order: a butterfly over the wavefront, then the four waves in order
    if (__any(v[27] != 0.0)) {
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int k = 0; k < RV_SUMS; ++k) v[k] += __shfl_xor(v[k], o, 64);
    }   // else: no counted pixel in the wavefront, every sum is 0
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < RV_SUMS; ++k) red[wave][k] = v[k];
        cnt[wave][RV_PRESENT] = n_present; cnt[wave][RV_NO_DEPTH] = n_nod; cnt[wave][RV_OFF_CLASS] = n_off; cnt[wave][RV_TOO_FAR] = n_far; cnt[wave][RV_GRAZING] = n_graze;
    }
    __syncthreads();
    const size_t slot = (size_t)h * (size_t)ra.groups + (size_t)g;
    if (tid < RV_SUMS) partial[slot * RV_SUMS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    if (tid < RV_COUNTS) pcount[slot * RV_COUNTS + tid] = ((cnt[0][tid] + cnt[1][tid]) + cnt[2][tid]) + cnt[3][tid];
}

// The fixed-order reduction of a pose's G partials S (sums) and N (counts) by one wavefront: lane l sums partials l, l + 64, ... in order,
// then a butterfly over the wavefront; every lane ends with the totals.  The order depends on G alone, whatever the batch.
__device__ __forceinline__ void rv_reduce_partials(const double* __restrict__ partial, const int32_t* __restrict__ pcount, int h, int groups, int lane, double (&acc)[RV_SUMS],
                                                   int (&n)[RV_COUNTS]) {
    const double* S = partial + (size_t)h * (size_t)groups * RV_SUMS;
    const int32_t* N = pcount + (size_t)h * (size_t)groups * RV_COUNTS;
#pragma unroll
    for (int k = 0; k < RV_SUMS; ++k) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < RV_COUNTS; ++k) n[k] = 0;
    for (int g = lane; g < groups; g += 64) {
#pragma unroll
        for (int k = 0; k < RV_SUMS; ++k) acc[k] += S[(size_t)g * RV_SUMS + k];
#pragma unroll
        for (int k = 0; k < RV_COUNTS; ++k) n[k] += N[(size_t)g * RV_COUNTS + k];
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < RV_SUMS; ++k) acc[k] += __shfl_xor(acc[k], o, 64);
#pragma unroll
        for (int k = 0; k < RV_COUNTS; ++k) n[k] += __shfl_xor(n[k], o, 64);
    }
}

// One wavefront per hypothesis of the chunk.  update == 0 (max_iterations == 0): the record alone.  Detail::on: the sums go to
// det.sums29 and nothing else happens.
template <class Detail>
__global__ __launch_bounds__(64) void refine_visible_solve_kernel(float* __restrict__ poses, const double* __restrict__ partial, const int32_t* __restrict__ pcount, int groups,
                                                                  int update, int32_t* __restrict__ frozen, stocs_refine_visible_result* __restrict__ rec, Detail det) {
    const int h = (int)blockIdx.x, lane = (int)threadIdx.x;
    if constexpr (!Detail::on) { if (frozen[h]) return; }   // the same address in every lane: the whole wavefront
    double acc[RV_SUMS];
    int n[RV_COUNTS];
    rv_reduce_partials(partial, pcount, h, groups, lane, acc, n);
    if (lane) return;
    if constexpr (Detail::on) {
#pragma unroll
        for (int k = 0; k < RV_SUMS; ++k) det.sums29[k] = acc[k];
        return;
    }
    float* Ph = poses + (size_t)h * 16;
    float P[16];
    bool nonzero = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) { P[i] = Ph[i]; nonzero = nonzero || P[i] != 0.0f; }
    stocs_refine_visible_result* R = rec + h;   // zeroed in front of the first iteration
    if (!pose_finite(P) || !nonzero) { frozen[h] = 1; return; }   // renders nothing: the zero record, the pose as it came
    const int count = (int)acc[27];
    R->present = n[RV_PRESENT]; R->no_depth = n[RV_NO_DEPTH]; R->off_class = n[RV_OFF_CLASS]; R->too_far = n[RV_TOO_FAR]; R->grazing = n[RV_GRAZING];
    R->counted = count;
    R->rms = count > 0 ? sqrtf((float)(acc[28] / (double)count)) : 0.0f;
    if (!update) return;
    if (count < 6) { frozen[h] = 1; R->frozen = 1; return; }   // not enough pixels: keep the current pose
    double A[6][6], b[6], x[6];
    int k = 0;
    for (int r = 0; r < 6; ++r) for (int c = r; c < 6; ++c) { A[r][c] = acc[k]; A[c][r] = acc[k]; k++; }
    for (int r = 0; r < 6; ++r) b[r] = acc[21 + r];
    if (!solve6(A, b, x)) { frozen[h] = 1; R->frozen = 1; return; }
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    const double Rm[3][3] = {{cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa},
                             {sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa},
                             {-sb, cb * sa, cb * ca}};
    // P <- Delta P on the left, column-major: entry (r, c) at P[4 c + r]; the last row stays
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            double e = (Rm[r][0] * (double)P[4 * c] + Rm[r][1] * (double)P[4 * c + 1]) + Rm[r][2] * (double)P[4 * c + 2];
            if (c == 3) e += x[3 + r];
            Ph[4 * c + r] = (float)e;
        }
    R->iterations += 1;
}

// ---- the damped form (stocs_refine_poses_visible_damped): the same render and accumulation, another solve step
struct RvDampedArgs {
    double max_d2;                 // (double) of the float product the accumulation compares with
    double lambda0, down, up;
    double max_rot, max_trans;     // +inf: no bound
    double pm[3];                  // pivot_model
    int pivot, K;
};
// what a pose keeps between evaluations beside its accepted pose and its record: the accepted sums, the accepted cost, lambda
struct RvDampedState { double S[RV_SUMS]; double cost, lambda; };

// What follows the cost C of evaluation e in the damped contract, lane 0's, in double: the decision against the pose's accepted state, and
// for e < K the next trial from the accepted state (steps 1-7), written into the slot Ph the next render reads.  sys: the sums the system
// is made from ([0..26]; [28] is the record's b^T b; kept whole as the accepted sums); n, count: the evaluation's counts; enough: whether
// the evaluation at e = 0 carries a system at all.  P holds the evaluated pose and, behind a rejection, the accepted one.
__device__ __forceinline__ bool rv_damped_decide(float* Ph, float* Pah, float (&P)[16], stocs_refine_visible_damped_result* R,
                                                 RvDampedState* St, int32_t* done_h, stocs_refine_visible_trace* trace_h, int e,
                                                 RvDampedArgs da, const double (&sys)[RV_SUMS], const int (&n)[RV_COUNTS], int count, double C, bool enough) {
    double lambda = e == 0 ? da.lambda0 : St->lambda;
    const bool ok = e == 0 || C < St->cost;
    double Sa[27];   // what the next trial is made from: the 21 + 6 accepted sums
    if (ok) {
        R->base.present = n[RV_PRESENT]; R->base.no_depth = n[RV_NO_DEPTH]; R->base.off_class = n[RV_OFF_CLASS]; R->base.too_far = n[RV_TOO_FAR];
        R->base.grazing = n[RV_GRAZING]; R->base.counted = count;
        R->base.rms = count > 0 ? sqrtf((float)(sys[28] / (double)count)) : 0.0f;
        R->cost = (float)C;
#pragma unroll
        for (int k = 0; k < RV_SUMS; ++k) St->S[k] = sys[k];
#pragma unroll
        for (int k = 0; k < 27; ++k) Sa[k] = sys[k];
        St->cost = C;
        if (e > 0) {
            lambda = fmax(lambda / da.down, 1e-9);
            R->base.iterations += 1;
#pragma unroll
            for (int i = 0; i < 16; ++i) Pah[i] = P[i];
        }
    } else {
        lambda = fmin(lambda * da.up, 1e9);
        R->rejected += 1;
#pragma unroll
        for (int k = 0; k < 27; ++k) Sa[k] = St->S[k];
#pragma unroll
        for (int i = 0; i < 16; ++i) P[i] = Pah[i];   // from here on P is the accepted pose
    }
    St->lambda = lambda;
    R->lambda = (float)lambda;
    R->evaluations += 1;
    stocs_refine_visible_trace* Tr = trace_h ? trace_h + (size_t)e : NULL;   // row e of the pose's K + 1
    if (Tr) {
#pragma unroll
        for (int i = 0; i < 16; ++i) Tr->pose[i] = Ph[i];
        Tr->cost = C; Tr->lambda = lambda; Tr->accepted = ok ? 1 : 0; Tr->state = 1;
    }
    if (e == da.K) return ok;
    bool freeze = e == 0 && !enough;   // not enough pixels at the start: the pose as it came
    double x[6];
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    if (!freeze) {
        // 1. the pivot in the camera frame
        if (da.pivot) {
            c0 = (((double)P[0] * da.pm[0] + (double)P[4] * da.pm[1]) + (double)P[8] * da.pm[2]) + (double)P[12];
            c1 = (((double)P[1] * da.pm[0] + (double)P[5] * da.pm[1]) + (double)P[9] * da.pm[2]) + (double)P[13];
            c2 = (((double)P[2] * da.pm[0] + (double)P[6] * da.pm[1]) + (double)P[10] * da.pm[2]) + (double)P[14];
        }
        // 2. M' = T M T^T, v' = T v with T = [[I, -[c]x], [0, I]]: rows 0..2 of T M, then columns 0..2 of (T M) T^T
        const double Cx[3][3] = {{0.0, -c2, c1}, {c2, 0.0, -c0}, {-c1, c0, 0.0}};
        double M[6][6], A[6][6], b[6];
        int k = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int q = r; q < 6; ++q) { M[r][q] = Sa[k]; M[q][r] = Sa[k]; k++; }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int q = 0; q < 6; ++q) M[r][q] = M[r][q] - ((Cx[r][0] * M[3][q] + Cx[r][1] * M[4][q]) + Cx[r][2] * M[5][q]);
            b[r] = Sa[21 + r] - ((Cx[r][0] * Sa[24] + Cx[r][1] * Sa[25]) + Cx[r][2] * Sa[26]);
            b[3 + r] = Sa[24 + r];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int q = 0; q < 6; ++q)
                A[r][q] = q < 3 ? M[r][q] - ((M[r][3] * Cx[q][0] + M[r][4] * Cx[q][1]) + M[r][5] * Cx[q][2]) : M[r][q];
        // 3. damping, 4. the solve
#pragma unroll
        for (int r = 0; r < 6; ++r) A[r][r] = A[r][r] * (1.0 + lambda);
        freeze = !solve6(A, b, x);
    }
    if (freeze) {
        *done_h = 1; R->base.frozen = 1;
        if (Tr) Tr->state = 3;
        return ok;
    }
    // 5. the bound
    double s = 1.0;
    const double nr = sqrt(x[0] * x[0] + (x[1] * x[1] + x[2] * x[2])), nt = sqrt(x[3] * x[3] + (x[4] * x[4] + x[5] * x[5]));
    if (nr > 0.0 && da.max_rot / nr < s) s = da.max_rot / nr;
    if (nt > 0.0 && da.max_trans / nt < s) s = da.max_trans / nt;
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = s * x[i];
    // 6. the motion about c, 7. the next trial (float)(Delta Pa)
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    const double Rm[3][3] = {{cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa},
                             {sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa},
                             {-sb, cb * sa, cb * ca}};
    const double cc[3] = {c0, c1, c2};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double t = (x[3 + r] + cc[r]) - ((Rm[r][0] * c0 + Rm[r][1] * c1) + Rm[r][2] * c2);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double v = (Rm[r][0] * (double)P[4 * q] + Rm[r][1] * (double)P[4 * q + 1]) + Rm[r][2] * (double)P[4 * q + 2];
            if (q == 3) v += t;
            Ph[4 * q + r] = (float)v;   // the slot's last row is the start's, as every accepted pose's is
        }
    }
    return ok;
}

// ---- the contour form (stocs_refine_poses_visible_contour): the damped form's evaluation plus a pass over the frame's object
// pixels that the render left uncovered, each pulled towards the nearest silhouette pixel
enum { RC_TILE_ROWS = 16, RC_MAX_RADIUS = 64, RC_BIT_ROWS = RC_TILE_ROWS + 2 * RC_MAX_RADIUS };
enum { RC_UNREACHED = 0, RC_BEYOND, RC_PULLED };   // the integer counts of a contour partial (RV_COUNTS wide: the rest is 0)
enum { RC_FAR = 999 };                             // "no set bit on this side": above every radius

struct RcArgs {
    float pull_d2;     // pull_distance * pull_distance, in float
    int R;             // pull_radius_px
    int groups;        // G
};
struct RcNoDetail { static constexpr bool on = false; };
struct RcDetailOut {
    static constexpr bool on = true;
    uint8_t* state;    // H * W, preset 0
    int32_t* nearest;  // H * W, preset -1
};

// N_O of the frame: pixels with a measurement whose class probability reaches the threshold.  Integer counts: any order gives the same.
__global__ __launch_bounds__(256) void refine_visible_object_count_kernel(const uint16_t* __restrict__ depth, const uint16_t* __restrict__ prob, size_t npix,
                                                                          float class_threshold, int32_t* __restrict__ n_object) {
    int mine = 0;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t base = (size_t)blockIdx.x * 256; base < npix; base += stride) {   // wave-uniform bounds: every __ballot sees the whole wavefront
        const size_t px = base + threadIdx.x;
        bool in = false;
        if (px < npix && depth[px] != 0) in = (float)((double)prob[px] * (1.0 / 10000)) >= class_threshold;
        mine += __popcll(__ballot(in));
    }
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_object, mine);
}

// the nearest set bit of a 192-bit row (words lo, mid, hi; mid's bit `lane` is the pixel's own column) on either side of the pixel: the
// distances to the left (dl) and to the right (dr) in columns, 0 .. 64, RC_FAR where there is none within 64
__device__ __forceinline__ void rc_nearest_in_row(unsigned long long lo, unsigned long long mid, unsigned long long hi, int lane, int& dl, int& dr) {
    const unsigned long long right = lane ? (mid >> lane) | (hi << (64 - lane)) : mid;           // bit k: column c + k
    const unsigned long long left = lane == 63 ? mid : (mid << (63 - lane)) | (lo >> (lane + 1));   // bit 63 - k: column c - k
    dr = right ? (int)__builtin_ctzll(right) : (((hi >> lane) & 1ull) ? 64 : RC_FAR);
    dl = left ? (int)__builtin_clzll(left) : (((lo >> lane) & 1ull) ? 64 : RC_FAR);
}

// Pose blockIdx.y of the chunk, the grid of the accumulation.  The pose's rectangle grown by R and clamped to the frame is cut into tiles of
// RC_TILE_ROWS rows x 64 columns from its upper left corner; workgroup g takes tiles g, g + G, ... in row-major order, its four wavefronts
// rows w, w + 4, w + 8, w + 12 of a tile, a lane one column.  Per tile: (A) which of its pixels are object pixels with an empty key; a
// tile without one is done.  (B) "key present" of the tile plus its halo of R rows and 64 columns as bit rows in LDS, one __ballot per 64
// keys; only the pose's own rectangle is read (nothing is set outside it).  (C) per pixel the exact minimum of (d2, index) over the rows
// of the window, nearest rows first, until a row's dr dr alone is above the best d2; the winner's key is the only one loaded for its depth.
// Keys are read and never written.  Sums and counts are reduced as the accumulation's: one partial per workgroup.
template <class Detail>
__global__ __launch_bounds__(256) void refine_visible_contour_kernel(const unsigned long long* __restrict__ zkey, const int32_t* __restrict__ box,
                                                                     const uint16_t* __restrict__ depth, const uint16_t* __restrict__ prob, DepthArgs a, RcArgs ca,
                                                                     double* __restrict__ partial, int32_t* __restrict__ pcount, Detail det) {
    __shared__ unsigned long long bits[RC_BIT_ROWS][3];
    __shared__ double red[4][RV_SUMS];
    __shared__ int cnt[4][3];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = (int)blockIdx.y, g = (int)blockIdx.x;
    const int32_t* bx = box + (size_t)h * VSD_BOX_WORDS;
    const int c0 = -bx[VB_NEG_C0], c1 = bx[VB_C1], r0 = -bx[VB_NEG_R0], r1 = bx[VB_R1];
    const bool any = c1 >= 0 && c1 >= c0 && r1 >= r0;   // as in the accumulation: a rendered pose has 0 <= c0 <= c1 <= W - 1, 0 <= r0 <= r1 <= H - 1
    const int R = ca.R;
    const int ec0 = max(c0 - R, 0), ec1 = min(c1 + R, a.W - 1), er0 = max(r0 - R, 0), er1 = min(r1 + R, a.H - 1);
    const int n_tcols = any ? (ec1 - ec0 + 64) >> 6 : 0;
    const int n_trows = any ? (er1 - er0 + RC_TILE_ROWS) / RC_TILE_ROWS : 0;
    const int n_tiles = n_trows * n_tcols;
    const unsigned long long* zk = zkey + (size_t)h * ((size_t)a.W * (size_t)a.H);
    double v[RV_SUMS];
#pragma unroll
    for (int k = 0; k < RV_SUMS; ++k) v[k] = 0.0;
    int n_unreached = 0, n_beyond = 0, n_pulled = 0;
    for (int tile = g; tile < n_tiles; tile += ca.groups) {
        const int trow = tile / n_tcols, tcol = tile - trow * n_tcols;
        const int tr0 = er0 + trow * RC_TILE_ROWS, tr1 = min(tr0 + RC_TILE_ROWS - 1, er1);
        const int cs = ec0 + tcol * 64, c = cs + lane;
        // (A) the uncovered object pixels of the tile
        uint16_t raw[4];
        bool need[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = tr0 + wave + 4 * i;
            raw[i] = 0; need[i] = false;
            if (r <= tr1 && c <= ec1) {
                const size_t px = (size_t)r * (size_t)a.W + (size_t)c;
                raw[i] = depth[px];
                if (raw[i] != 0 && (float)((double)prob[px] * (1.0 / 10000)) >= a.class_threshold) need[i] = zk[px] == RV_EMPTY;
            }
        }
        if (!__syncthreads_or((need[0] || need[1]) || (need[2] || need[3]))) continue;   // the barrier also ends the previous tile's reads of bits
        // (B) the bit rows of rows wr0 .. wr1: at most RC_TILE_ROWS + 2 R of them
        const int wr0 = max(tr0 - R, r0), wr1 = min(tr1 + R, r1);
        const int n_words = wr1 >= wr0 ? (wr1 - wr0 + 1) * 3 : 0;
        for (int it = wave; it < n_words; it += 4) {
            const int row = it / 3, j = it - row * 3;
            const int col = cs - 64 + 64 * j + lane;
            bool set = false;
            if (col >= c0 && col <= c1) set = zk[(size_t)(wr0 + row) * (size_t)a.W + (size_t)col] != RV_EMPTY;
            const unsigned long long word = __ballot(set);
            if (lane == 0) bits[row][j] = word;
        }
        __syncthreads();
        // (C) the search, the gate and the rows
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = tr0 + wave + 4 * i;
            int st = 0;
            if (need[i]) {
                unsigned long long best = RV_EMPTY;   // d2 << 32 | linear index: the minimum is the contract's nearest pixel
                const int lo = max(r - R, wr0), hi = min(r + R, wr1);
                for (int k = 0; k <= R; ++k) {
                    if ((unsigned long long)(k * k) > (best >> 32)) break;   // no row further away can hold a nearer or an equal pixel
                    for (int s = 0; s < (k ? 2 : 1); ++s) {
                        const int rs = s ? r + k : r - k;
                        if (rs < lo || rs > hi) continue;
                        int dl, dr;
                        rc_nearest_in_row(bits[rs - wr0][0], bits[rs - wr0][1], bits[rs - wr0][2], lane, dl, dr);
                        if (dl <= R) best = min(best, ((unsigned long long)(k * k + dl * dl) << 32) | (unsigned long long)(uint32_t)(rs * a.W + (c - dl)));
                        if (dr <= R) best = min(best, ((unsigned long long)(k * k + dr * dr) << 32) | (unsigned long long)(uint32_t)(rs * a.W + (c + dr)));
                    }
                }
                st = 1;
                if (best != RV_EMPTY) {
                    const int idx = (int)(uint32_t)best, rs = idx / a.W, cs_ = idx - rs * a.W;
                    const float z = __uint_as_float((uint32_t)(zk[idx] >> 32));
                    const float xs = ((float)cs_ - a.cx) / a.fx, ys = ((float)rs - a.cy) / a.fy;
                    const float xu = ((float)c - a.cx) / a.fx, yu = ((float)r - a.cy) / a.fy;
                    const float d = (float)raw[i] * a.depth_scale;
                    const float p0 = xs * z, p1 = ys * z, q0 = xu * d, q1 = yu * d;
                    const float e0 = q0 - p0, e1 = q1 - p1, e2 = d - z;
                    const float D = e0 * e0 + (e1 * e1 + e2 * e2);
                    st = 2;
                    if (!(D > ca.pull_d2)) {
                        st = 3;
                        const double px_ = p0, py_ = p1, pz_ = z;
                        const double rows[3][6] = {{0.0, pz_, -py_, 1.0, 0.0, 0.0}, {-pz_, 0.0, px_, 0.0, 1.0, 0.0}, {py_, -px_, 0.0, 0.0, 0.0, 1.0}};   // [p x e_k, e_k]
                        const double bk[3] = {(double)e0, (double)e1, (double)e2};
#pragma unroll
                        for (int m = 0; m < 3; ++m) {
                            int q = 0;
#pragma unroll
                            for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                                for (int jj = ii; jj < 6; ++jj) { v[q] += rows[m][ii] * rows[m][jj]; ++q; }
#pragma unroll
                            for (int ii = 0; ii < 6; ++ii) v[21 + ii] += rows[m][ii] * bk[m];
                            v[28] += bk[m] * bk[m];
                        }
                        v[27] += 1.0;
                    }
                    if constexpr (Detail::on) det.nearest[(size_t)r * (size_t)a.W + (size_t)c] = idx;
                }
                if constexpr (Detail::on) det.state[(size_t)r * (size_t)a.W + (size_t)c] = (uint8_t)st;
            }
            n_unreached += __popcll(__ballot(st == 1)); n_beyond += __popcll(__ballot(st == 2)); n_pulled += __popcll(__ballot(st == 3));
        }
    }
    if (__any(v[27] != 0.0)) {
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int k = 0; k < RV_SUMS; ++k) v[k] += __shfl_xor(v[k], o, 64);
    }   // else: no pulled pixel in the wavefront, every sum is 0
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < RV_SUMS; ++k) red[wave][k] = v[k];
        cnt[wave][RC_UNREACHED] = n_unreached; cnt[wave][RC_BEYOND] = n_beyond; cnt[wave][RC_PULLED] = n_pulled;
    }
    __syncthreads();
    const size_t slot = (size_t)h * (size_t)ca.groups + (size_t)g;
    if (tid < RV_SUMS) partial[slot * RV_SUMS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    if (tid < RV_COUNTS) pcount[slot * RV_COUNTS + tid] = tid < 3 ? ((cnt[0][tid] + cnt[1][tid]) + cnt[2][tid]) + cnt[3][tid] : 0;
}

// ---- the damped solve of both forms.  A form names its record and says whether contour partials exist
struct RvDampedForm {
    typedef stocs_refine_visible_damped_result Record;
    static constexpr bool contour = false;
};
struct RvContourForm {
    typedef stocs_refine_visible_contour_result Record;
    static constexpr bool contour = true;
    const double* part; const int32_t* cnt;   // the chunk's contour partials
    const int32_t* n_object;                  // N_O
    double w;                                 // (double) contour_weight; 0: no contour partials are read
    double pull_d2;                           // (double) of the float product the contour kernel compares with
};

// One wavefront per hypothesis of the chunk, after evaluation e of K + 1: the reduction of refine_visible_solve_kernel, the cost, the
// decision against the accepted state, and for e < K the next trial from the accepted state (rv_damped_decide), written into the pose
// slot the next render reads.  Everything behind the reduction is lane 0's, in double.  The contour form reduces both sets of partials in
// the same fixed order, decides on the totals M = S + w Sc, v likewise, with the cost over the frame's object pixels, and fills its own
// fields of the record from the decision.
template <class Form>
__global__ __launch_bounds__(64) void refine_visible_damped_solve_kernel(float* __restrict__ poses, const double* __restrict__ partial, const int32_t* __restrict__ pcount,
                                                                         int groups, int e, RvDampedArgs da, float* __restrict__ accepted, RvDampedState* __restrict__ state,
                                                                         int32_t* __restrict__ done, typename Form::Record* __restrict__ rec,
                                                                         stocs_refine_visible_trace* __restrict__ trace, Form f) {
    const int h = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (done[h]) return;   // the same address in every lane: the whole wavefront
    double acc[RV_SUMS], con[Form::contour ? RV_SUMS : 1];
    int n[RV_COUNTS], nc[Form::contour ? RV_COUNTS : 1];
    rv_reduce_partials(partial, pcount, h, groups, lane, acc, n);
    if constexpr (Form::contour) {
        if (f.w != 0.0) rv_reduce_partials(f.part, f.cnt, h, groups, lane, con, nc);
        else {
#pragma unroll
            for (int k = 0; k < RV_SUMS; ++k) con[k] = 0.0;
#pragma unroll
            for (int k = 0; k < RV_COUNTS; ++k) nc[k] = 0;
        }
    }
    if (lane) return;
    float* Ph = poses + (size_t)h * 16;
    float* Pah = accepted + (size_t)h * 16;
    float P[16];
    bool nonzero = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) { P[i] = Ph[i]; nonzero = nonzero || P[i] != 0.0f; }
    if (e == 0 && (!pose_finite(P) || !nonzero)) { done[h] = 1; return; }   // renders nothing: the zero record, the pose as it came
    typename Form::Record* R = rec + h;   // zeroed in front of the first evaluation
    stocs_refine_visible_trace* trace_h = trace ? trace + (size_t)h * (size_t)(da.K + 1) : (stocs_refine_visible_trace*)NULL;
    const int count = (int)acc[27];
    if constexpr (!Form::contour) {
        const double C = count < 6 ? (double)INFINITY : (acc[28] + da.max_d2 * (double)n[RV_TOO_FAR]) / (double)(count + n[RV_TOO_FAR]);
        rv_damped_decide(Ph, Pah, P, R, state + h, done + h, trace_h, e, da, acc, n, count, C, count >= 6);
    } else {
        const int pulled = nc[RC_PULLED], n_obj = *f.n_object;
        const int uncovered = n_obj - ((n[RV_TOO_FAR] + n[RV_GRAZING]) + count);
        double sys[RV_SUMS];
#pragma unroll
        for (int k = 0; k < 27; ++k) sys[k] = acc[k] + f.w * con[k];
        sys[27] = acc[27]; sys[28] = acc[28];
        const bool enough = count + 3 * pulled >= 6;
        const double C = !enough ? (double)INFINITY
                                 : ((acc[28] + da.max_d2 * (double)n[RV_TOO_FAR]) + f.w * (con[28] + f.pull_d2 * (double)(uncovered - pulled))) /
                                       ((double)(count + n[RV_TOO_FAR]) + f.w * (double)uncovered);
        if (rv_damped_decide(Ph, Pah, P, &R->damped, state + h, done + h, trace_h, e, da, sys, n, count, C, enough)) {   // accepted: its contour fields
            R->object_px = n_obj; R->uncovered = uncovered; R->unreached = nc[RC_UNREACHED]; R->beyond = nc[RC_BEYOND]; R->pulled = pulled;
            R->pull_rms = pulled > 0 ? sqrtf((float)(con[28] / (double)pulled)) : 0.0f;
        }
    }
}

static const char* params_error(const stocs_refine_visible_params* p) {
    if (p->max_iterations < 0) return "max_iterations must be >= 0";
    if (!(p->max_distance > 0.0f) || !isfinite(p->max_distance)) return "max_distance must be positive and finite";
    if (!(p->min_view_cos >= 0.0f && p->min_view_cos < 1.0f)) return "min_view_cos must be in [0, 1)";
    if (!isfinite(p->class_threshold)) return "class_threshold is not finite";
    return NULL;
}

static const char* damped_params_error(const stocs_refine_visible_damped_params* p) {
    if (const char* why = params_error(&p->base)) return why;
    if (!(p->lambda0 >= 0.0f) || !isfinite(p->lambda0)) return "lambda0 must be >= 0 and finite";
    if (!(p->lambda_down >= 1.0f) || !isfinite(p->lambda_down)) return "lambda_down must be >= 1 and finite";
    if (!(p->lambda_up >= 1.0f) || !isfinite(p->lambda_up)) return "lambda_up must be >= 1 and finite";
    if (!(p->max_step_rotation > 0.0f)) return "max_step_rotation must be positive (+inf: no bound)";
    if (!(p->max_step_translation > 0.0f)) return "max_step_translation must be positive (+inf: no bound)";
    if (p->pivot != 0 && p->pivot != 1) return "pivot must be 0 (the camera's origin) or 1 (pivot_model)";
    if (!isfinite(p->pivot_model[0]) || !isfinite(p->pivot_model[1]) || !isfinite(p->pivot_model[2])) return "pivot_model is not finite";
    return NULL;
}

static const char* contour_params_error(const stocs_refine_visible_contour_params* p) {
    if (const char* why = damped_params_error(&p->damped)) return why;
    if (!(p->contour_weight >= 0.0f) || !isfinite(p->contour_weight)) return "contour_weight must be >= 0 and finite";
    if (p->pull_radius_px < 1 || p->pull_radius_px > RC_MAX_RADIUS) return "pull_radius_px must be in 1 .. 64";
    if (!(p->pull_distance > 0.0f) || !isfinite(p->pull_distance)) return "pull_distance must be positive and finite";
    return NULL;
}

// how many poses a chunk of key buffers holds: 256 MB of them, or what STOCS_REFINE_VISIBLE_CHUNK says; the pose is blockIdx.y
static size_t visible_chunk(int n, size_t npix) {
    size_t chunk = std::max<size_t>(1, ((size_t)256 << 20) / (8 * npix));
    if (const char* e = getenv("STOCS_REFINE_VISIBLE_CHUNK")) { const long v = atol(e); if (v >= 1) chunk = (size_t)v; }
    return std::min<size_t>(std::min<size_t>(chunk, (size_t)n), 65535);
}

// the workspace of n poses in chunks of `chunk`
struct VisibleWork {
    size_t o_pose, o_rec, o_frozen, o_box, o_part, o_cnt, o_key, total;
    char* d;
    float* pose() const { return (float*)(d + o_pose); }
    stocs_refine_visible_result* rec() const { return (stocs_refine_visible_result*)(d + o_rec); }
    int32_t* frozen() const { return (int32_t*)(d + o_frozen); }
    int32_t* box() const { return (int32_t*)(d + o_box); }
    double* part() const { return (double*)(d + o_part); }
    int32_t* cnt() const { return (int32_t*)(d + o_cnt); }
    unsigned long long* key() const { return (unsigned long long*)(d + o_key); }
};
static int visible_work(stocs_ctx* c, int n, size_t chunk, size_t npix, int groups, VisibleWork* w) {
    Carve cv;
    w->o_pose = cv.take((size_t)n * 64);   // the records lie behind the poses: one copy reads both back
    w->o_rec = cv.take((size_t)n * sizeof(stocs_refine_visible_result));
    w->o_frozen = cv.take((size_t)n * 4);
    w->o_box = cv.take(chunk * VSD_BOX_WORDS * 4);
    w->o_part = cv.take(chunk * (size_t)groups * RV_SUMS * 8);
    w->o_cnt = cv.take(chunk * (size_t)groups * RV_COUNTS * 4);
    w->o_key = cv.take(chunk * npix * 8);
    w->total = cv.total;
    RefineVisibleState* S = ctx_state<RefineVisibleState>(c);
    { const int rc = S->work.grow(c->stream, cv.total); if (rc) return rc; }
    w->d = S->work.p;
    return STOCS_OK;
}

// The workspace of n poses of the damped and the contour form, in RefineVisibleState::damped.  What comes back lies in front, so one copy
// reads it: accepted poses | records (rec_size each) | trace (K + 1 rows per pose, when asked for).  contour_slots: the chunk's contour
// partials (chunk * G), 0 for the damped form, which has no N_O either.
struct DampedWork {
    size_t o_acc, o_rec, o_trace, o_state, o_done, o_cpart, o_ccnt, o_nobj, trace_bytes, back_all, back_bytes;
    char* d;
    float* acc() const { return (float*)(d + o_acc); }
    stocs_refine_visible_trace* trace() const { return trace_bytes ? (stocs_refine_visible_trace*)(d + o_trace) : NULL; }
    RvDampedState* state() const { return (RvDampedState*)(d + o_state); }
    int32_t* done() const { return (int32_t*)(d + o_done); }
    double* cpart() const { return (double*)(d + o_cpart); }
    int32_t* ccnt() const { return (int32_t*)(d + o_ccnt); }
    int32_t* nobj() const { return (int32_t*)(d + o_nobj); }
};
static int damped_work(stocs_ctx* c, int n, int K, size_t rec_size, bool traced, size_t contour_slots, DampedWork* w) {
    Carve cv;
    w->trace_bytes = traced ? (size_t)n * (size_t)(K + 1) * sizeof(stocs_refine_visible_trace) : 0;
    w->o_acc = cv.take((size_t)n * 64);
    w->o_rec = cv.take((size_t)n * rec_size);
    w->o_trace = cv.take(w->trace_bytes);
    w->back_all = cv.total;
    w->back_bytes = traced ? w->o_trace + w->trace_bytes : w->o_rec + (size_t)n * rec_size;
    w->o_state = cv.take((size_t)n * sizeof(RvDampedState));
    w->o_done = cv.take((size_t)n * 4);
    w->o_cpart = cv.take(contour_slots * RV_SUMS * 8);
    w->o_ccnt = cv.take(contour_slots * RV_COUNTS * 4);
    w->o_nobj = cv.take(contour_slots ? 4 : 0);
    RefineVisibleState* S = ctx_state<RefineVisibleState>(c);
    { const int rc = S->damped.grow(c->stream, cv.total); if (rc) return rc; }
    w->d = S->damped.p;
    return STOCS_OK;
}

static RvDampedArgs damped_args(const stocs_refine_visible_damped_params* p, const RvArgs& ra) {
    RvDampedArgs da;
    da.max_d2 = (double)ra.max_d2; da.lambda0 = (double)p->lambda0; da.down = (double)p->lambda_down; da.up = (double)p->lambda_up;
    da.max_rot = (double)p->max_step_rotation; da.max_trans = (double)p->max_step_translation;
    for (int k = 0; k < 3; ++k) da.pm[k] = (double)p->pivot_model[k];
    da.pivot = p->pivot; da.K = p->base.max_iterations;
    return da;
}

// ---- one evaluation of poses h0 .. h0 + m of the workspace, in three parts (their key buffers are clear in front and, behind the shipping
// accumulation, clear again)
// rectangles cleared, render
static int enqueue_render(stocs_ctx* c, const VisibleWork& w, int h0, int m, const DepthArgs& a, bool timed) {
    STOCS_HIP_CHECK(hipMemsetAsync(w.box(), 0x80, (size_t)m * VSD_BOX_WORDS * 4, c->stream));
    if (timed) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[0], c->stream));
    return mesh_enqueue_tri_keys(c, w.pose() + (size_t)h0 * 16, m, a, w.key(), w.box());
}
// the contour pass on the keys: its arguments and where the chunk's contour partials go; run: whether the form's weight asks for it
struct RcPass { RcArgs ca; double* part; int32_t* cnt; bool run; };
template <class Detail>
static int enqueue_contour(stocs_ctx* c, const DepthState* F, const VisibleWork& w, int m, const DepthArgs& a, const RcPass& cp, Detail det, bool timed) {
    if (timed) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[4], c->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(refine_visible_contour_kernel<Detail>), dim3((unsigned)cp.ca.groups, (unsigned)m), dim3(256), 0, c->stream,
                       (const unsigned long long*)w.key(), (const int32_t*)w.box(), frame_depth(F), frame_prob(F), a, cp.ca, cp.part, cp.cnt, det);
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}
template <class Detail>
static int enqueue_accumulate(stocs_ctx* c, const DepthState* F, const VisibleWork& w, int h0, int m, const DepthArgs& a, const RvArgs& ra, Detail det, bool timed) {
    const float4* verts; const int4* tris;
    mesh_device_arrays(c, &verts, &tris);
    if (timed) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[1], c->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(refine_visible_accumulate_kernel<Detail>), dim3((unsigned)ra.groups, (unsigned)m), dim3(256), 0, c->stream,
                       (const float*)(w.pose() + (size_t)h0 * 16), verts, tris, w.key(), (const int32_t*)w.box(), frame_depth(F), frame_prob(F), a, ra, w.part(), w.cnt(), det);
    STOCS_HIP_CHECK(hipGetLastError());
    if (timed) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[2], c->stream));
    return STOCS_OK;
}

// ---- the checks, in the documented orders
// the refusals every batch entry point starts with.  True: the call ends here with *rc (n == 0: STOCS_OK)
static bool visible_refuse(const char* who, const stocs_ctx* c, const void* poses, int n, const void* prm, const void* pose16_out, const void* out, int* rc) {
    *rc = STOCS_ERR_INVALID;
    if (!c) { set_error("%s: NULL context", who); return true; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return true; }
    if (n == 0) { *rc = STOCS_OK; return true; }
    if (!poses || !prm || !pose16_out || !out) { set_error("%s: NULL poses, parameters or results", who); return true; }
    return false;
}
// a stocs_check_*_params entry point
template <class P>
static int params_check(const char* who, const P* p, const char* (*error)(const P*)) {
    if (!p) { set_error("%s: NULL parameters", who); return STOCS_ERR_INVALID; }
    if (const char* why = error(p)) { set_error("%s: %s", who, why); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}
// behind an entry point's own NULL tests: the plain parameters, the mesh, the frame
static int visible_check(const char* who, stocs_ctx* c, const stocs_refine_visible_params* p, DepthState** F) {
    if (const char* why = params_error(p)) { set_error("%s: %s", who, why); return STOCS_ERR_INVALID; }
    { const int rc = mesh_check_present(who, c); if (rc) return rc; }
    return check_frame(who, c, F);
}
// ... of both contour entry points: the contour parameters, the damped order, then the class image
static int contour_check(const char* who, stocs_ctx* c, const stocs_refine_visible_contour_params* p, DepthState** F) {
    if (const char* why = contour_params_error(p)) { set_error("%s: %s", who, why); return STOCS_ERR_INVALID; }
    { const int rc = visible_check(who, c, &p->damped.base, F); if (rc) return rc; }
    if (!frame_prob(*F)) { set_error("%s: the frame has no class image: the object pixels are not defined (stocs_ctx_set_frame)", who); return STOCS_ERR_STATE; }
    return STOCS_OK;
}

static RvArgs visible_args(const stocs_refine_visible_params* p, int groups) {
    RvArgs ra;
    ra.max_d2 = p->max_distance * p->max_distance; ra.min_cos2 = p->min_view_cos * p->min_view_cos; ra.groups = groups;
    return ra;
}
static RcArgs contour_args(const stocs_refine_visible_contour_params* p, int groups) {
    RcArgs ca;
    ca.pull_d2 = p->pull_distance * p->pull_distance; ca.R = p->pull_radius_px; ca.groups = groups;
    return ca;
}

// ---- The call frame of the three batch entry points.  Made behind the last refusal, it holds the device, the chunk size, G, the
// arguments of render and accumulation and the workspace of n poses (rc: whether that could be had).  run() stages the poses through the
// pinned block, runs all evaluations of a chunk before the next chunk starts -- render, the contour pass if there is one to run,
// accumulation, the form's solve step -- and reads back_bytes at d_back back in one copy behind the call's one synchronisation.
struct VisibleCall {
    DeviceGuard guard;
    stocs_ctx* c; const DepthState* F;
    int n, groups, rc;
    size_t npix, chunk;
    DepthArgs a; RvArgs ra; VisibleWork w;
    VisibleCall(stocs_ctx* c_, const DepthState* F_, int n_, const stocs_refine_visible_params* p)
        : guard(c_->device), c(c_), F(F_), n(n_), groups(refine_visible_groups(F_->npix)), npix(F_->npix), chunk(visible_chunk(n_, F_->npix)),
          a(frame_args(F_, 0.0f, p->class_threshold)), ra(visible_args(p, groups)) {
        rc = visible_work(c, n, chunk, npix, groups, &w);
    }
    // evaluations: per chunk; cp: the contour form's pass (NULL: another form); d_accepted: where the start goes beside the slot the render
    // reads (NULL: nowhere); step(h0, m, e) launches the form's solve behind evaluation e of poses h0 .. h0 + m; *hback: what came back
    template <class Step>
    int run(const float* poses, int evaluations, const RcPass* cp, float* d_accepted, Step step, const void* d_back, size_t back_bytes, char** hback) {
        const bool dev_clock = c->device_clock != 0, pass = cp && cp->run;
        char* hin;
        { const int r = pinned_for(c, (size_t)n * 64, back_bytes, &hin, hback); if (r) return r; }
        memcpy(hin, poses, (size_t)n * 64);
        STOCS_HIP_CHECK(hipMemcpyAsync(w.pose(), hin, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));   // the slot the render reads
        if (d_accepted) STOCS_HIP_CHECK(hipMemcpyAsync(d_accepted, hin, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
        for (int h0 = 0; h0 < n; h0 += (int)chunk) {
            const int m = std::min((int)chunk, n - h0);
            STOCS_HIP_CHECK(hipMemsetAsync(w.key(), 0xFF, (size_t)m * npix * 8, c->stream));
            for (int e = 0; e < evaluations; ++e) {
                const bool timed = dev_clock && h0 + m == n && e + 1 == evaluations;   // the call's last evaluation
                { const int r = enqueue_render(c, w, h0, m, a, timed); if (r) return r; }
                if (pass) { const int r = enqueue_contour(c, F, w, m, a, *cp, RcNoDetail(), timed); if (r) return r; }
                { const int r = enqueue_accumulate(c, F, w, h0, m, a, ra, RvNoDetail(), timed); if (r) return r; }
                { const int r = step(h0, m, e); if (r) return r; }
                if (timed) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[3], c->stream));
            }
        }
        STOCS_HIP_CHECK(hipMemcpyAsync(*hback, d_back, back_bytes, hipMemcpyDeviceToHost, c->stream));
        STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
        // the event read-out: render, the contour pass if run (with it the render ends where the contour kernel starts), accumulation, solve
        RefineVisibleState* S = ctx_state<RefineVisibleState>(c);
        S->last_ms[0] = S->last_ms[1] = S->last_ms[2] = -1.0f;
        if (cp) S->last_contour_ms = -1.0f;
        const int mark[5] = {0, pass ? 4 : 1, 1, 2, 3};
        float* const slot[4] = {&S->last_ms[0], pass ? &S->last_contour_ms : (float*)NULL, &S->last_ms[1], &S->last_ms[2]};
        float ms = 0.0f;
        for (int k = 0; dev_clock && k < 4; ++k)
            if (slot[k] && hipEventElapsedTime(&ms, c->ev_t[mark[k]], c->ev_t[mark[k + 1]]) == hipSuccess) *slot[k] = ms;
        return STOCS_OK;
    }
};

// The damped and the contour entry point behind their checks (cprm: the contour form's parameters): K + 1 evaluations per chunk with the
// damped solve of the form, the accepted pose and the record in the damped block, read back with the trace behind them.  The contour form
// counts N_O in front and has the contour pass inside every evaluation.
template <class Form>
static int damped_call(stocs_ctx* c, const DepthState* F, const float* poses, int n, const stocs_refine_visible_damped_params* dp,
                       const stocs_refine_visible_contour_params* cprm, float* pose16_out, typename Form::Record* out, stocs_refine_visible_trace* trace) {
    typedef typename Form::Record Record;
    VisibleCall vc(c, F, n, &dp->base);
    if (vc.rc) return vc.rc;
    const int K = dp->base.max_iterations;
    DampedWork dw;
    { const int rc = damped_work(c, n, K, sizeof(Record), trace != NULL, Form::contour ? vc.chunk * (size_t)vc.groups : 0, &dw); if (rc) return rc; }
    STOCS_HIP_CHECK(hipMemsetAsync(dw.d + dw.o_rec, 0, dw.back_all - dw.o_rec, c->stream));   // records and trace
    STOCS_HIP_CHECK(hipMemsetAsync(dw.done(), 0, (size_t)n * 4, c->stream));
    const RvDampedArgs da = damped_args(dp, vc.ra);
    Form f;
    RcPass cp;
    if constexpr (Form::contour) {
        STOCS_HIP_CHECK(hipMemsetAsync(dw.nobj(), 0, 4, c->stream));
        hipLaunchKernelGGL(refine_visible_object_count_kernel, dim3((unsigned)std::min<size_t>((vc.npix + 255) / 256, 1024)), dim3(256), 0, c->stream, frame_depth(F),
                           frame_prob(F), vc.npix, vc.a.class_threshold, dw.nobj());
        STOCS_HIP_CHECK(hipGetLastError());
        cp.ca = contour_args(cprm, vc.groups); cp.part = dw.cpart(); cp.cnt = dw.ccnt(); cp.run = cprm->contour_weight != 0.0f;
        f.part = cp.part; f.cnt = cp.cnt; f.n_object = dw.nobj(); f.w = (double)cprm->contour_weight; f.pull_d2 = (double)cp.ca.pull_d2;
    }
    Record* d_rec = (Record*)(dw.d + dw.o_rec);
    char* hback;
    const int rc = vc.run(poses, K + 1, Form::contour ? &cp : (const RcPass*)NULL, dw.acc(), [&](int h0, int m, int e) -> int {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(refine_visible_damped_solve_kernel<Form>), dim3((unsigned)m), dim3(64), 0, c->stream, vc.w.pose() + (size_t)h0 * 16,
                           (const double*)vc.w.part(), (const int32_t*)vc.w.cnt(), vc.groups, e, da, dw.acc() + (size_t)h0 * 16, dw.state() + h0, dw.done() + h0, d_rec + h0,
                           dw.trace() ? dw.trace() + (size_t)h0 * (size_t)(K + 1) : (stocs_refine_visible_trace*)NULL, f);
        STOCS_HIP_CHECK(hipGetLastError());
        return STOCS_OK;
    }, dw.d, dw.back_bytes, &hback);
    if (rc) return rc;
    memcpy(pose16_out, hback + dw.o_acc, (size_t)n * 64);
    memcpy(out, hback + dw.o_rec, (size_t)n * sizeof(Record));
    if (trace) memcpy(trace, hback + dw.o_trace, dw.trace_bytes);
    return STOCS_OK;
}

// The front of both detail entry points, synchronous paths for tests and diagnosis: ONE pose, pageable copies, ONE evaluation.  The
// workspace of one pose and the planes in RefineVisibleState::detail (nearest and the contour partials only for the contour detail), the
// pose up, the keys and the planes cleared.
struct DetailWork { VisibleWork w; int groups; DepthArgs a; uint8_t* state; int32_t* nearest; double* sums29; double* cpart; int32_t* ccnt; };
static int detail_begin(stocs_ctx* c, const DepthState* F, const float* pose, float class_threshold, bool contour, DetailWork* d) {
    const size_t npix = F->npix;
    d->groups = refine_visible_groups(npix);
    d->a = frame_args(F, 0.0f, class_threshold);
    { const int rc = visible_work(c, 1, 1, npix, d->groups, &d->w); if (rc) return rc; }
    RefineVisibleState* S = ctx_state<RefineVisibleState>(c);
    Carve cv;
    const size_t o_near = cv.take(contour ? npix * 4 : 0), o_state = cv.take(npix), o_sums = cv.take(RV_SUMS * 8);
    const size_t o_cpart = cv.take(contour ? (size_t)d->groups * RV_SUMS * 8 : 0), o_ccnt = cv.take(contour ? (size_t)d->groups * RV_COUNTS * 4 : 0);
    { const int rc = S->detail.grow(c->stream, cv.total); if (rc) return rc; }
    char* base = S->detail.p;
    d->nearest = Carve::at<int32_t>(base, o_near); d->state = Carve::at<uint8_t>(base, o_state); d->sums29 = Carve::at<double>(base, o_sums);
    d->cpart = Carve::at<double>(base, o_cpart); d->ccnt = Carve::at<int32_t>(base, o_ccnt);
    STOCS_HIP_CHECK(hipMemcpyAsync(d->w.pose(), pose, 64, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(d->w.key(), 0xFF, npix * 8, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(d->state, 0, npix, c->stream));
    if (contour) STOCS_HIP_CHECK(hipMemsetAsync(d->nearest, 0xFF, npix * 4, c->stream));
    return STOCS_OK;
}
// ... and their end: the 29 sums of the partials (part, cnt) as the solve step forms them, the one synchronisation
static int detail_sums(stocs_ctx* c, const DetailWork& d, const double* part, const int32_t* cnt) {
    RvDetailOut det;
    det.state = NULL; det.sums29 = d.sums29;
    hipLaunchKernelGGL(refine_visible_solve_kernel<RvDetailOut>, dim3(1), dim3(64), 0, c->stream, d.w.pose(), part, cnt, d.groups, 0, d.w.frozen(), d.w.rec(), det);
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return STOCS_OK;
}

}  // namespace stocs

using namespace stocs;

extern "C" void stocs_default_refine_visible_params(stocs_refine_visible_params* p) {
    if (!p) return;
    p->max_iterations = 5; p->max_distance = 0.02f; p->min_view_cos = 0.0f; p->class_threshold = 0.10f;
}

extern "C" void stocs_default_refine_visible_damped_params(stocs_refine_visible_damped_params* p) {
    if (!p) return;
    stocs_default_refine_visible_params(&p->base);
    p->lambda0 = 1.0f; p->lambda_down = 4.0f; p->lambda_up = 16.0f;
    p->max_step_rotation = 0.0872664626f;   // 5 degrees
    p->max_step_translation = 0.01f;
    p->pivot = 1;
    p->pivot_model[0] = p->pivot_model[1] = p->pivot_model[2] = 0.0f;
}

extern "C" void stocs_default_refine_visible_contour_params(stocs_refine_visible_contour_params* p) {
    if (!p) return;
    stocs_default_refine_visible_damped_params(&p->damped);
    p->contour_weight = 1.0f; p->pull_radius_px = 16; p->pull_distance = 0.03f;
}

extern "C" int stocs_check_refine_visible_params(const stocs_refine_visible_params* p) { return params_check("stocs_check_refine_visible_params", p, params_error); }
extern "C" int stocs_check_refine_visible_damped_params(const stocs_refine_visible_damped_params* p) {
    return params_check("stocs_check_refine_visible_damped_params", p, damped_params_error);
}
extern "C" int stocs_check_refine_visible_contour_params(const stocs_refine_visible_contour_params* p) {
    return params_check("stocs_check_refine_visible_contour_params", p, contour_params_error);
}

extern "C" int stocs_refine_visible_groups(int width, int height) {
    if (width < 1 || height < 1) return 0;
    return refine_visible_groups((size_t)width * (size_t)height);
}

extern "C" int stocs_refine_visible_last_device_ms(const stocs_ctx* c, float* render_ms, float* accumulate_ms, float* solve_ms) {
    if (!c) { set_error("stocs_refine_visible_last_device_ms: NULL context"); return STOCS_ERR_INVALID; }
    const RefineVisibleState* S = ctx_state_if<RefineVisibleState>(c);
    if (render_ms) *render_ms = S ? S->last_ms[0] : -1.0f;
    if (accumulate_ms) *accumulate_ms = S ? S->last_ms[1] : -1.0f;
    if (solve_ms) *solve_ms = S ? S->last_ms[2] : -1.0f;
    return STOCS_OK;
}

extern "C" int stocs_refine_visible_contour_last_device_ms(const stocs_ctx* c, float* contour_ms) {
    if (!c) { set_error("stocs_refine_visible_contour_last_device_ms: NULL context"); return STOCS_ERR_INVALID; }
    const RefineVisibleState* S = ctx_state_if<RefineVisibleState>(c);
    if (contour_ms) *contour_ms = S ? S->last_contour_ms : -1.0f;
    return STOCS_OK;
}

// The plain form: max(max_iterations, 1) evaluations per chunk, each followed by the plain solve; poses and records come back from the
// workspace, where the records lie behind the poses.
extern "C" int stocs_refine_poses_visible(stocs_ctx* c, const float* poses, int n, const stocs_refine_visible_params* prm, float* pose16_out,
                                          stocs_refine_visible_result* out) {
    static const char* who = "stocs_refine_poses_visible";
    int rc;
    if (visible_refuse(who, c, poses, n, prm, pose16_out, out, &rc)) return rc;
    DepthState* F = NULL;
    if ((rc = visible_check(who, c, prm, &F))) return rc;
    VisibleCall vc(c, F, n, prm);
    if (vc.rc) return vc.rc;
    const VisibleWork& w = vc.w;
    STOCS_HIP_CHECK(hipMemsetAsync(w.rec(), 0, (size_t)n * sizeof(stocs_refine_visible_result), c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(w.frozen(), 0, (size_t)n * 4, c->stream));
    const int update = prm->max_iterations > 0 ? 1 : 0;
    char* hback;
    rc = vc.run(poses, std::max(prm->max_iterations, 1), NULL, NULL, [&](int h0, int m, int) -> int {
        hipLaunchKernelGGL(refine_visible_solve_kernel<RvNoDetail>, dim3((unsigned)m), dim3(64), 0, c->stream, w.pose() + (size_t)h0 * 16, (const double*)w.part(),
                           (const int32_t*)w.cnt(), vc.groups, update, w.frozen() + h0, w.rec() + h0, RvNoDetail());
        STOCS_HIP_CHECK(hipGetLastError());
        return STOCS_OK;
    }, w.pose(), w.o_rec - w.o_pose + (size_t)n * sizeof(stocs_refine_visible_result), &hback);
    if (rc) return rc;
    memcpy(pose16_out, hback, (size_t)n * 64);
    memcpy(out, hback + (w.o_rec - w.o_pose), (size_t)n * sizeof(stocs_refine_visible_result));
    return STOCS_OK;
}

extern "C" int stocs_refine_poses_visible_damped(stocs_ctx* c, const float* poses, int n, const stocs_refine_visible_damped_params* prm, float* pose16_out,
                                                 stocs_refine_visible_damped_result* out, stocs_refine_visible_trace* trace) {
    static const char* who = "stocs_refine_poses_visible_damped";
    int rc;
    if (visible_refuse(who, c, poses, n, prm, pose16_out, out, &rc)) return rc;
    DepthState* F = NULL;
    if (const char* why = damped_params_error(prm)) { set_error("%s: %s", who, why); return STOCS_ERR_INVALID; }   // its own parameters in front
    if ((rc = visible_check(who, c, &prm->base, &F))) return rc;
    return damped_call<RvDampedForm>(c, F, poses, n, prm, NULL, pose16_out, out, trace);
}

extern "C" int stocs_refine_poses_visible_contour(stocs_ctx* c, const float* poses, int n, const stocs_refine_visible_contour_params* prm, float* pose16_out,
                                                  stocs_refine_visible_contour_result* out, stocs_refine_visible_trace* trace) {
    static const char* who = "stocs_refine_poses_visible_contour";
    int rc;
    if (visible_refuse(who, c, poses, n, prm, pose16_out, out, &rc)) return rc;
    DepthState* F = NULL;
    if ((rc = contour_check(who, c, prm, &F))) return rc;
    return damped_call<RvContourForm>(c, F, poses, n, &prm->damped, prm, pose16_out, out, trace);
}

// The keys as the render left them, the state per pixel, the 29 sums of one evaluation of one pose.
extern "C" int stocs_refine_visible_detail(stocs_ctx* c, const float* pose, const stocs_refine_visible_params* prm, uint64_t* keys, uint8_t* state, double* sums29) {
    static const char* who = "stocs_refine_visible_detail";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (!pose || !prm || !sums29) { set_error("%s: NULL pose, parameters or sums", who); return STOCS_ERR_INVALID; }
    DepthState* F = NULL;
    { const int rc = visible_check(who, c, prm, &F); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    DetailWork d;
    { const int rc = detail_begin(c, F, pose, prm->class_threshold, false, &d); if (rc) return rc; }
    RvDetailOut det;
    det.state = d.state; det.sums29 = d.sums29;
    { const int rc = enqueue_render(c, d.w, 0, 1, d.a, false); if (rc) return rc; }
    { const int rc = enqueue_accumulate(c, F, d.w, 0, 1, d.a, visible_args(prm, d.groups), det, false); if (rc) return rc; }
    { const int rc = detail_sums(c, d, d.w.part(), d.w.cnt()); if (rc) return rc; }
    if (keys) STOCS_HIP_CHECK(hipMemcpy(keys, d.w.key(), F->npix * 8, hipMemcpyDeviceToHost));
    if (state) STOCS_HIP_CHECK(hipMemcpy(state, d.state, F->npix, hipMemcpyDeviceToHost));
    STOCS_HIP_CHECK(hipMemcpy(sums29, d.sums29, RV_SUMS * 8, hipMemcpyDeviceToHost));
    return STOCS_OK;
}

// The render and the contour pass of one evaluation of one pose: the state and the nearest silhouette pixel per pixel, the 29 contour sums.
extern "C" int stocs_refine_visible_contour_detail(stocs_ctx* c, const float* pose, const stocs_refine_visible_contour_params* prm, uint8_t* state, int32_t* nearest,
                                                   double* sums29) {
    static const char* who = "stocs_refine_visible_contour_detail";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (!pose || !prm || !sums29) { set_error("%s: NULL pose, parameters or sums", who); return STOCS_ERR_INVALID; }
    DepthState* F = NULL;
    { const int rc = contour_check(who, c, prm, &F); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    DetailWork d;
    { const int rc = detail_begin(c, F, pose, prm->damped.base.class_threshold, true, &d); if (rc) return rc; }
    RcDetailOut det;
    det.state = d.state; det.nearest = d.nearest;
    const RcPass cp = {contour_args(prm, d.groups), d.cpart, d.ccnt, true};
    { const int rc = enqueue_render(c, d.w, 0, 1, d.a, false); if (rc) return rc; }
    { const int rc = enqueue_contour(c, F, d.w, 1, d.a, cp, det, false); if (rc) return rc; }
    { const int rc = detail_sums(c, d, cp.part, cp.cnt); if (rc) return rc; }
    if (state) STOCS_HIP_CHECK(hipMemcpy(state, d.state, F->npix, hipMemcpyDeviceToHost));
    if (nearest) STOCS_HIP_CHECK(hipMemcpy(nearest, d.nearest, F->npix * 4, hipMemcpyDeviceToHost));
    STOCS_HIP_CHECK(hipMemcpy(sums29, d.sums29, RV_SUMS * 8, hipMemcpyDeviceToHost));
    return STOCS_OK;
}
