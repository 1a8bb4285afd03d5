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
// accumulation K + 1 times and puts another kernel in the solve's place:
//   damped solve  one wavefront per hypothesis: the solve's reduction (rv_reduce_partials), then lane 0 in double: the cost of the
//               evaluation, accept or reject against the pose's accepted state (pose, 29 sums, cost, lambda, kept in the workspace between
//               evaluations), and from the accepted state the sums moved to a pivot on the object, the damped 6x6 solve, the bound and the
//               next trial pose, written into the slot the next render reads; one trace row per evaluation when asked for.
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
    DevBlock detail;   // stocs_refine_visible_detail: state | sums, grow-only
    DevBlock damped;   // stocs_refine_poses_visible_damped: accepted poses | records | trace | accepted sums, cost, lambda | done flags, grow-only
    float last_ms[3] = {-1.0f, -1.0f, -1.0f};  // "device_clock": HIP-event time of the last call's last render, accumulation and solve (-1: not taken)
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

// One wavefront per hypothesis of the chunk, after evaluation e of K + 1: the reduction of refine_visible_solve_kernel, the cost, the
// decision against the accepted state, and for e < K the next trial from the accepted state (steps 1-7 of the contract), written into the
// pose slot the next render reads.  Everything behind the reduction is lane 0's, in double.
__global__ __launch_bounds__(64) void refine_visible_damped_solve_kernel(float* __restrict__ poses, const double* __restrict__ partial, const int32_t* __restrict__ pcount,
                                                                         int groups, int e, RvDampedArgs da, float* __restrict__ accepted, RvDampedState* __restrict__ state,
                                                                         int32_t* __restrict__ done, stocs_refine_visible_damped_result* __restrict__ rec,
                                                                         stocs_refine_visible_trace* __restrict__ trace) {
    const int h = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (done[h]) return;   // the same address in every lane: the whole wavefront
    double acc[RV_SUMS];
    int n[RV_COUNTS];
    rv_reduce_partials(partial, pcount, h, groups, lane, acc, n);
    if (lane) return;
    float* Ph = poses + (size_t)h * 16;
    float* Pah = accepted + (size_t)h * 16;
    float P[16];
    bool nonzero = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) { P[i] = Ph[i]; nonzero = nonzero || P[i] != 0.0f; }
    stocs_refine_visible_damped_result* R = rec + h;   // zeroed in front of the first evaluation
    RvDampedState* St = state + h;
    if (e == 0 && (!pose_finite(P) || !nonzero)) { done[h] = 1; return; }   // renders nothing: the zero record, the pose as it came
    const int count = (int)acc[27];
    const double C = count < 6 ? (double)INFINITY : (acc[28] + da.max_d2 * (double)n[RV_TOO_FAR]) / (double)(count + n[RV_TOO_FAR]);
    double lambda = e == 0 ? da.lambda0 : St->lambda;
    const bool ok = e == 0 || C < St->cost;
    double Sa[27];   // what the next trial is made from: the 21 + 6 accepted sums
    if (ok) {
        R->base.present = n[RV_PRESENT]; R->base.no_depth = n[RV_NO_DEPTH]; R->base.off_class = n[RV_OFF_CLASS]; R->base.too_far = n[RV_TOO_FAR];
        R->base.grazing = n[RV_GRAZING]; R->base.counted = count;
        R->base.rms = count > 0 ? sqrtf((float)(acc[28] / (double)count)) : 0.0f;
        R->cost = (float)C;
#pragma unroll
        for (int k = 0; k < RV_SUMS; ++k) St->S[k] = acc[k];
#pragma unroll
        for (int k = 0; k < 27; ++k) Sa[k] = acc[k];
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
    stocs_refine_visible_trace* Tr = trace ? trace + (size_t)h * (size_t)(da.K + 1) + (size_t)e : NULL;
    if (Tr) {
#pragma unroll
        for (int i = 0; i < 16; ++i) Tr->pose[i] = Ph[i];
        Tr->cost = C; Tr->lambda = lambda; Tr->accepted = ok ? 1 : 0; Tr->state = 1;
    }
    if (e == da.K) return;
    bool freeze = e == 0 && count < 6;   // not enough pixels at the start: the pose as it came
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
        done[h] = 1; R->base.frozen = 1;
        if (Tr) Tr->state = 3;
        return;
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

// one evaluation of poses h0 .. h0 + m of the workspace: rectangles cleared, render, accumulate (their key buffers are clear in front
// and, in the shipping form, behind)
template <class Detail>
static int enqueue_evaluate(stocs_ctx* c, const DepthState* F, const VisibleWork& w, int h0, int m, const DepthArgs& a, const RvArgs& ra, Detail det, bool timed) {
    const float4* verts; const int4* tris;
    mesh_device_arrays(c, &verts, &tris);
    STOCS_HIP_CHECK(hipMemsetAsync(w.box(), 0x80, (size_t)m * VSD_BOX_WORDS * 4, c->stream));
    if (timed) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[0], c->stream));
    { const int rc = mesh_enqueue_tri_keys(c, w.pose() + (size_t)h0 * 16, m, a, w.key(), w.box()); if (rc) return rc; }
    if (timed) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[1], c->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(refine_visible_accumulate_kernel<Detail>), dim3((unsigned)ra.groups, (unsigned)m), dim3(256), 0, c->stream,
                       (const float*)(w.pose() + (size_t)h0 * 16), verts, tris, w.key(), (const int32_t*)w.box(), frame_depth(F), frame_prob(F), a, ra, w.part(), w.cnt(), det);
    STOCS_HIP_CHECK(hipGetLastError());
    if (timed) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[2], c->stream));
    return STOCS_OK;
}

// the checks both entry points make behind their own NULL tests, in the documented order
static int visible_check(const char* who, stocs_ctx* c, const stocs_refine_visible_params* p, DepthState** F) {
    if (const char* why = params_error(p)) { set_error("%s: %s", who, why); return STOCS_ERR_INVALID; }
    { const int rc = mesh_check_present(who, c); if (rc) return rc; }
    return check_frame(who, c, F);
}

static RvArgs visible_args(const stocs_refine_visible_params* p, int groups) {
    RvArgs ra;
    ra.max_d2 = p->max_distance * p->max_distance; ra.min_cos2 = p->min_view_cos * p->min_view_cos; ra.groups = groups;
    return ra;
}

}  // namespace stocs

using namespace stocs;

extern "C" void stocs_default_refine_visible_params(stocs_refine_visible_params* p) {
    if (!p) return;
    p->max_iterations = 5; p->max_distance = 0.02f; p->min_view_cos = 0.0f; p->class_threshold = 0.10f;
}

extern "C" int stocs_check_refine_visible_params(const stocs_refine_visible_params* p) {
    if (!p) { set_error("stocs_check_refine_visible_params: NULL parameters"); return STOCS_ERR_INVALID; }
    if (const char* why = params_error(p)) { set_error("stocs_check_refine_visible_params: %s", why); return STOCS_ERR_INVALID; }
    return STOCS_OK;
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

extern "C" int stocs_refine_poses_visible(stocs_ctx* c, const float* poses, int n, const stocs_refine_visible_params* prm, float* pose16_out,
                                          stocs_refine_visible_result* out) {
    static const char* who = "stocs_refine_poses_visible";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n == 0) return STOCS_OK;
    if (!poses || !prm || !pose16_out || !out) { set_error("%s: NULL poses, parameters or results", who); return STOCS_ERR_INVALID; }
    DepthState* F = NULL;
    { const int rc = visible_check(who, c, prm, &F); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    const bool dev_clock = c->device_clock != 0;
    const size_t npix = F->npix, chunk = visible_chunk(n, npix);
    const int groups = refine_visible_groups(npix);
    VisibleWork w;
    { const int rc = visible_work(c, n, chunk, npix, groups, &w); if (rc) return rc; }
    const size_t back_bytes = w.o_rec - w.o_pose + (size_t)n * sizeof(stocs_refine_visible_result);
    char* hin; char* hback;
    { const int rc = pinned_for(c, (size_t)n * 64, back_bytes, &hin, &hback); if (rc) return rc; }
    memcpy(hin, poses, (size_t)n * 64);
    STOCS_HIP_CHECK(hipMemcpyAsync(w.pose(), hin, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(w.rec(), 0, (size_t)n * sizeof(stocs_refine_visible_result), c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(w.frozen(), 0, (size_t)n * 4, c->stream));
    const DepthArgs a = frame_args(F, 0.0f, prm->class_threshold);
    const RvArgs ra = visible_args(prm, groups);
    const int evaluations = std::max(prm->max_iterations, 1), update = prm->max_iterations > 0 ? 1 : 0;
    for (int h0 = 0; h0 < n; h0 += (int)chunk) {   // all iterations of a chunk before the next one starts
        const int m = std::min((int)chunk, n - h0);
        STOCS_HIP_CHECK(hipMemsetAsync(w.key(), 0xFF, (size_t)m * npix * 8, c->stream));
        for (int it = 0; it < evaluations; ++it) {
            const bool timed = dev_clock && h0 + m == n && it + 1 == evaluations;
            { const int rc = enqueue_evaluate(c, F, w, h0, m, a, ra, RvNoDetail(), timed); if (rc) return rc; }
            hipLaunchKernelGGL(refine_visible_solve_kernel<RvNoDetail>, dim3((unsigned)m), dim3(64), 0, c->stream, w.pose() + (size_t)h0 * 16, (const double*)w.part(),
                               (const int32_t*)w.cnt(), groups, update, w.frozen() + h0, w.rec() + h0, RvNoDetail());
            STOCS_HIP_CHECK(hipGetLastError());
            if (timed) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[3], c->stream));
        }
    }
    STOCS_HIP_CHECK(hipMemcpyAsync(hback, w.pose(), back_bytes, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    RefineVisibleState* S = ctx_state<RefineVisibleState>(c);
    S->last_ms[0] = S->last_ms[1] = S->last_ms[2] = -1.0f;
    if (dev_clock) {
        float ms = 0.0f;
        for (int k = 0; k < 3; ++k)
            if (hipEventElapsedTime(&ms, c->ev_t[k], c->ev_t[k + 1]) == hipSuccess) S->last_ms[k] = ms;
    }
    memcpy(pose16_out, hback, (size_t)n * 64);
    memcpy(out, hback + (w.o_rec - w.o_pose), (size_t)n * sizeof(stocs_refine_visible_result));
    return STOCS_OK;
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

extern "C" int stocs_check_refine_visible_damped_params(const stocs_refine_visible_damped_params* p) {
    if (!p) { set_error("stocs_check_refine_visible_damped_params: NULL parameters"); return STOCS_ERR_INVALID; }
    if (const char* why = damped_params_error(p)) { set_error("stocs_check_refine_visible_damped_params: %s", why); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}

// The plain call's frame with another solve step: K + 1 evaluations per chunk, the accepted pose and the record in the damped block,
// read back with the trace behind them in one copy.
extern "C" int stocs_refine_poses_visible_damped(stocs_ctx* c, const float* poses, int n, const stocs_refine_visible_damped_params* prm, float* pose16_out,
                                                 stocs_refine_visible_damped_result* out, stocs_refine_visible_trace* trace) {
    static const char* who = "stocs_refine_poses_visible_damped";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n == 0) return STOCS_OK;
    if (!poses || !prm || !pose16_out || !out) { set_error("%s: NULL poses, parameters or results", who); return STOCS_ERR_INVALID; }
    if (const char* why = damped_params_error(prm)) { set_error("%s: %s", who, why); return STOCS_ERR_INVALID; }
    DepthState* F = NULL;
    { const int rc = visible_check(who, c, &prm->base, &F); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    const bool dev_clock = c->device_clock != 0;
    const size_t npix = F->npix, chunk = visible_chunk(n, npix);
    const int groups = refine_visible_groups(npix), K = prm->base.max_iterations;
    VisibleWork w;
    { const int rc = visible_work(c, n, chunk, npix, groups, &w); if (rc) return rc; }
    RefineVisibleState* S = ctx_state<RefineVisibleState>(c);
    const size_t rows = (size_t)n * (size_t)(K + 1);
    Carve cv;   // what comes back lies in front: accepted poses | records | trace
    const size_t o_acc = cv.take((size_t)n * 64), o_rec = cv.take((size_t)n * sizeof(stocs_refine_visible_damped_result));
    const size_t o_trace = cv.take(trace ? rows * sizeof(stocs_refine_visible_trace) : 0), back_all = cv.total;
    const size_t o_state = cv.take((size_t)n * sizeof(RvDampedState)), o_done = cv.take((size_t)n * 4);
    { const int rc = S->damped.grow(c->stream, cv.total); if (rc) return rc; }
    float* d_acc = Carve::at<float>(S->damped.p, o_acc);
    stocs_refine_visible_damped_result* d_rec = Carve::at<stocs_refine_visible_damped_result>(S->damped.p, o_rec);
    stocs_refine_visible_trace* d_trace = trace ? Carve::at<stocs_refine_visible_trace>(S->damped.p, o_trace) : NULL;
    RvDampedState* d_state = Carve::at<RvDampedState>(S->damped.p, o_state);
    int32_t* d_done = Carve::at<int32_t>(S->damped.p, o_done);
    const size_t back_bytes = trace ? o_trace + rows * sizeof(stocs_refine_visible_trace) : o_rec + (size_t)n * sizeof(stocs_refine_visible_damped_result);
    char* hin; char* hback;
    { const int rc = pinned_for(c, (size_t)n * 64, back_bytes, &hin, &hback); if (rc) return rc; }
    memcpy(hin, poses, (size_t)n * 64);
    STOCS_HIP_CHECK(hipMemcpyAsync(w.pose(), hin, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));   // the slot the render reads
    STOCS_HIP_CHECK(hipMemcpyAsync(d_acc, hin, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));      // the accepted pose: the start
    STOCS_HIP_CHECK(hipMemsetAsync(S->damped.p + o_rec, 0, back_all - o_rec, c->stream));               // records and trace
    STOCS_HIP_CHECK(hipMemsetAsync(d_done, 0, (size_t)n * 4, c->stream));
    const DepthArgs a = frame_args(F, 0.0f, prm->base.class_threshold);
    const RvArgs ra = visible_args(&prm->base, groups);
    RvDampedArgs da;
    da.max_d2 = (double)ra.max_d2; da.lambda0 = (double)prm->lambda0; da.down = (double)prm->lambda_down; da.up = (double)prm->lambda_up;
    da.max_rot = (double)prm->max_step_rotation; da.max_trans = (double)prm->max_step_translation;
    for (int k = 0; k < 3; ++k) da.pm[k] = (double)prm->pivot_model[k];
    da.pivot = prm->pivot; da.K = K;
    for (int h0 = 0; h0 < n; h0 += (int)chunk) {   // all evaluations of a chunk before the next one starts
        const int m = std::min((int)chunk, n - h0);
        STOCS_HIP_CHECK(hipMemsetAsync(w.key(), 0xFF, (size_t)m * npix * 8, c->stream));
        for (int e = 0; e <= K; ++e) {
            const bool timed = dev_clock && h0 + m == n && e == K;
            { const int rc = enqueue_evaluate(c, F, w, h0, m, a, ra, RvNoDetail(), timed); if (rc) return rc; }
            hipLaunchKernelGGL(refine_visible_damped_solve_kernel, dim3((unsigned)m), dim3(64), 0, c->stream, w.pose() + (size_t)h0 * 16, (const double*)w.part(),
                               (const int32_t*)w.cnt(), groups, e, da, d_acc + (size_t)h0 * 16, d_state + h0, d_done + h0, d_rec + h0,
                               d_trace ? d_trace + (size_t)h0 * (size_t)(K + 1) : (stocs_refine_visible_trace*)NULL);
            STOCS_HIP_CHECK(hipGetLastError());
            if (timed) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[3], c->stream));
        }
    }
    STOCS_HIP_CHECK(hipMemcpyAsync(hback, S->damped.p, back_bytes, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    S->last_ms[0] = S->last_ms[1] = S->last_ms[2] = -1.0f;
    if (dev_clock) {
        float ms = 0.0f;
        for (int k = 0; k < 3; ++k)
            if (hipEventElapsedTime(&ms, c->ev_t[k], c->ev_t[k + 1]) == hipSuccess) S->last_ms[k] = ms;
    }
    memcpy(pose16_out, hback + o_acc, (size_t)n * 64);
    memcpy(out, hback + o_rec, (size_t)n * sizeof(stocs_refine_visible_damped_result));
    if (trace) memcpy(trace, hback + o_trace, rows * sizeof(stocs_refine_visible_trace));
    return STOCS_OK;
}

// A plain, synchronous path (a test and diagnosis facility): ONE pose, pageable copies, ONE evaluation; the keys as the render left
// them, the state per pixel, the 29 sums as the solve step forms them.
extern "C" int stocs_refine_visible_detail(stocs_ctx* c, const float* pose, const stocs_refine_visible_params* prm, uint64_t* keys, uint8_t* state, double* sums29) {
    static const char* who = "stocs_refine_visible_detail";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (!pose || !prm || !sums29) { set_error("%s: NULL pose, parameters or sums", who); return STOCS_ERR_INVALID; }
    DepthState* F = NULL;
    { const int rc = visible_check(who, c, prm, &F); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    const size_t npix = F->npix;
    const int groups = refine_visible_groups(npix);
    VisibleWork w;
    { const int rc = visible_work(c, 1, 1, npix, groups, &w); if (rc) return rc; }
    RefineVisibleState* S = ctx_state<RefineVisibleState>(c);
    Carve cv;
    const size_t o_state = cv.take(npix), o_sums = cv.take(RV_SUMS * 8);
    { const int rc = S->detail.grow(c->stream, cv.total); if (rc) return rc; }
    RvDetailOut det;
    det.state = Carve::at<uint8_t>(S->detail.p, o_state); det.sums29 = Carve::at<double>(S->detail.p, o_sums);
    STOCS_HIP_CHECK(hipMemcpyAsync(w.pose(), pose, 64, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(w.key(), 0xFF, npix * 8, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(det.state, 0, npix, c->stream));
    const DepthArgs a = frame_args(F, 0.0f, prm->class_threshold);
    { const int rc = enqueue_evaluate(c, F, w, 0, 1, a, visible_args(prm, groups), det, false); if (rc) return rc; }
    hipLaunchKernelGGL(refine_visible_solve_kernel<RvDetailOut>, dim3(1), dim3(64), 0, c->stream, w.pose(), (const double*)w.part(), (const int32_t*)w.cnt(), groups, 0,
                       w.frozen(), w.rec(), det);
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (keys) STOCS_HIP_CHECK(hipMemcpy(keys, w.key(), npix * 8, hipMemcpyDeviceToHost));
    if (state) STOCS_HIP_CHECK(hipMemcpy(state, det.state, npix, hipMemcpyDeviceToHost));
    STOCS_HIP_CHECK(hipMemcpy(sums29, det.sums29, RV_SUMS * 8, hipMemcpyDeviceToHost));
    return STOCS_OK;
}
