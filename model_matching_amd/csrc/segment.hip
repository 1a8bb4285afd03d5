// segment.hip -- depth-only frames: support-plane removal and depth-connected segments (stocs_segment_frame, no reference counterpart).
// A frame without a class-probability image gets one from its geometry: the dominant plane is found by scored three-pixel hypotheses and
// refitted on exact integer moments, what stands on it is split into 4-connected components under a depth-jump rule, and the components
// that are large enough become the segments.  The contract is at the declaration in include/stocs_hip.h; tests/segment_ref.py restates
// it in float32 numpy, equal bit for bit.
//
// Kernels, in launch order (one stream, no host round trip between them; everything integer or order-free, no float atomic on a sum):
//   seg_points        pixel -> point (float4, w = valid), the flags of the strided lattice, n_valid
//   (library scan)    positions of the valid lattice pixels; seg_compact packs their points: the score kernel's lanes are all busy
//   seg_hypotheses    one lane per hypothesis: three draws -> A, m = e1 x e2, tol^2 |m|^2, alive
//   seg_score         grid (tiles of 1024 scored points x blocks of 64 hypotheses): four points per lane in registers, a hypothesis is
//                     eight wave-uniform floats (scalar loads), __ballot + __popcll, LDS counters, one atomic per (workgroup, hypothesis)
//   seg_winner        the maximum of (count << 32) | ~h, the share test
//   seg_refit         int64 moments of the winner's inliers over every valid pixel: lane accumulators, butterfly, one atomic per workgroup
//                     and moment; seg_plane: one lane forms the plane from them in double (Jacobi, SEG_SWEEPS sweeps)
//   seg_heights       pixel classes against the float plane, the foreground depth image (NaN elsewhere), labels = own index
//   bend (stocs_segment_frame_convex only; steps 4a and 4b)  form 1 seg_smooth (a lane per pixel, the window from device memory) +
//                     seg_bend (the four far smoothed points from device memory); form 2 seg_bend_tiles (a workgroup per tile: raw depths of
//                     the foreground with a halo of r + s in LDS, the smoothed points of the tile and a halo of r in LDS, both tests from
//                     LDS).  Either writes the second depth image (NaN at cut pixels) that the kernels below then read, L = -1 at cut
//                     pixels, the cut image and five counts (ballots, one atomic per workgroup and counter).
//   label             form 1 seg_union_global + seg_flatten; form 2 seg_tiles (runs by ballot, union-find on run heads in LDS) +
//                     seg_borders (tile borders only, device memory) + seg_flatten.  Every link points from a larger index to a smaller
//                     one, so both forms end at the component's lowest index whatever the order.
//   seg_sizes, seg_keep, (library scan), seg_records_init, seg_relabel, seg_edges
//
// Host: both entry points refuse their NULL pointers and hand a SegCall to segment_run, the one launch sequence; the thread's arena per device
// and pinned block are a ThreadCache (thread_cache.h) of this file's own, beside ingest.hip's; SegLast is the clock and what the three
// stocs_segment_last_* entry points return.  What a third cut rule or label form adds: DESIGN 7.26.
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>

#include "prims.h"
#include "segment.h"
#include "segment_rules.h"
#include "stocs_ctx.h"
#include "thread_cache.h"
#include "wave_bits.h"

namespace stocs {

// what the kernels leave for the host: the result, the refit's count and nine moments, the winner's hypothesis
struct SegHeader {
    stocs_segment_result r;
    long long mom[10];     // n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz of q = llrint(v * 65536)
    float win[8];          // A, m, tol^2 |m|^2, alive
    stocs_segment_convex_result c;   // the bend step's counts (behind everything the older kernels address)
};

__device__ __forceinline__ bool seg_join(float za, float zb, float jump_abs, float jump_rel) {
    return fabsf(za - zb) <= jump_abs + jump_rel * fminf(za, zb);   // false when either is NaN (not foreground)
}
__device__ __forceinline__ bool seg_inlier(float4 p, const float* __restrict__ q) {
    const float dx = p.x - q[0], dy = p.y - q[1], dz = p.z - q[2];
    const float s = q[3] * dx + (q[4] * dy + q[5] * dz);
    return s * s <= q[6];
}

// the counting tails (wg_add_counts) address these counters as arrays: n_on_plane, n_above, n_below and n_tested_h .. n_cut are adjacent
static_assert(offsetof(stocs_segment_result, n_above) == offsetof(stocs_segment_result, n_on_plane) + 4 && offsetof(stocs_segment_result, n_below) == offsetof(stocs_segment_result, n_on_plane) + 8, "seg_heights");
static_assert(offsetof(stocs_segment_convex_result, n_tested_h) == 0 && offsetof(stocs_segment_convex_result, n_cut) == 16, "seg_bend_store");

__device__ __forceinline__ float seg_nan() { return __int_as_float(0x7fc00000); }   // the quiet NaN of "not foreground", "cut" and "outside the image"
// seg_unproject, pixel -> point, is in segment_rules.h: the shapes of labelled regions (segment_shapes.hip) form their points by it too

__global__ __launch_bounds__(256) void seg_points_kernel(const uint16_t* __restrict__ depth, int W, int H, float fx, float cx, float fy, float cy, float depth_scale,
                                                         float max_depth, int stride, int LW, float4* __restrict__ P, uint32_t* __restrict__ lat_flag,
                                                         SegHeader* __restrict__ hdr) {
    __shared__ int s_n[4][1];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false;
    if (idx < W * H) {
        const int i = idx / W, j = idx % W;
        const uint16_t raw = depth[idx];
        const float z = (float)raw * depth_scale;
        valid = raw != 0 && z <= max_depth;
        const V3 q = seg_unproject(i, j, z, fx, cx, fy, cy);
        P[idx] = make_float4(q.x, q.y, q.z, valid ? 1.0f : 0.0f);
        if (i % stride == 0 && j % stride == 0) lat_flag[(i / stride) * LW + j / stride] = valid ? 1u : 0u;
    }
    const int c = __popcll(__ballot(valid));
    wg_add_counts<1>(&c, s_n, &hdr->r.n_valid);
}

__global__ __launch_bounds__(256) void seg_compact_kernel(const float4* __restrict__ P, int W, int stride, int LW, int nl, const uint32_t* __restrict__ lat_flag,
                                                          const uint32_t* __restrict__ lat_pos, float4* __restrict__ SP) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nl || !lat_flag[e]) return;
    SP[lat_pos[e]] = P[(size_t)(e / LW) * stride * W + (size_t)(e % LW) * stride];
}

__global__ __launch_bounds__(256) void seg_hypotheses_kernel(const float4* __restrict__ P, uint32_t npix, int Hn, uint64_t seed, float tol, float* __restrict__ hyp) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= Hn) return;
    uint32_t ix[3];
    for (int k = 0; k < 3; ++k) ix[k] = (uint32_t)(((rng64(seed, (uint64_t)h, (uint64_t)k) >> 32) * (uint64_t)npix) >> 32);
    const float4 a = P[ix[0]], b = P[ix[1]], c = P[ix[2]];
    const V3 A = mk3(a.x, a.y, a.z);
    const V3 m = cross3(mk3(b.x, b.y, b.z) - A, mk3(c.x, c.y, c.z) - A);
    const float mm = m.x * m.x + (m.y * m.y + m.z * m.z);
    const bool alive = a.w != 0.0f && b.w != 0.0f && c.w != 0.0f && ix[0] != ix[1] && ix[0] != ix[2] && ix[1] != ix[2] && mm > 0.0f && mm < INFINITY;
    float* q = hyp + 8 * (size_t)h;
    q[0] = A.x; q[1] = A.y; q[2] = A.z; q[3] = m.x; q[4] = m.y; q[5] = m.z; q[6] = (tol * tol) * mm; q[7] = alive ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(256) void seg_score_kernel(const float4* __restrict__ SP, const uint32_t* __restrict__ n_scored_p, const float* __restrict__ hyp, int Hn,
                                                        uint32_t* __restrict__ cnt) {
    __shared__ uint32_t s_c[SEG_SCORE_HYP];
    const uint32_t ns = *n_scored_p;
    const uint32_t base = blockIdx.x * (uint32_t)SEG_SCORE_PTS;
    if (base >= ns) return;                                   // the grid is sized on the lattice; the valid part of it is known on the device only
    float4 p[4]; bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = base + k * 256 + threadIdx.x;
        ok[k] = i < ns;
        p[k] = ok[k] ? SP[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (threadIdx.x < SEG_SCORE_HYP) s_c[threadIdx.x] = 0;
    __syncthreads();
    const int h0 = blockIdx.y * SEG_SCORE_HYP;
    const int hn = min((int)SEG_SCORE_HYP, Hn - h0);
    for (int hh = 0; hh < hn; ++hh) {
        const float* __restrict__ q = hyp + 8 * (size_t)(h0 + hh);   // wave-uniform address: scalar loads
        if (q[7] == 0.0f) continue;                                   // a dead hypothesis costs one load
        int c = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) c += __popcll(__ballot(ok[k] && seg_inlier(p[k], q)));
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_c[hh], (uint32_t)c);
    }
    __syncthreads();
    if ((int)threadIdx.x < hn && s_c[threadIdx.x]) atomicAdd(&cnt[h0 + threadIdx.x], s_c[threadIdx.x]);
}

__global__ __launch_bounds__(256) void seg_winner_kernel(const float* __restrict__ hyp, const uint32_t* __restrict__ cnt, int Hn, const uint32_t* __restrict__ n_scored_p,
                                                         float min_share, SegHeader* __restrict__ hdr) {
    __shared__ unsigned long long s_k[4];
    unsigned long long key = 0;
    for (int h = threadIdx.x; h < Hn; h += 256) {
        const uint32_t c = cnt[h];
        if (c && hyp[8 * (size_t)h + 7] != 0.0f) { const unsigned long long k = ((unsigned long long)c << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)h); key = k > key ? k : key; }
    }
    key = wg_max_key<4>(key, s_k);
    if (threadIdx.x == 0) {
        const uint32_t ns = *n_scored_p;
        hdr->r.n_scored = (int)ns;
        hdr->r.winner = -1;
        if (key) {
            const uint32_t h = best_key_index(key), c = (uint32_t)(key >> 32);
            hdr->r.winner = (int)h; hdr->r.winner_count = (int)c;
            for (int k = 0; k < 8; ++k) hdr->win[k] = hyp[8 * (size_t)h + k];
            hdr->r.plane_found = ((double)c < (double)min_share * (double)ns) ? 0 : 1;
        }
    }
}

__global__ __launch_bounds__(256) void seg_refit_kernel(const float4* __restrict__ P, int npix, SegHeader* __restrict__ hdr) {
    __shared__ long long s_m[4][10];
    if (!hdr->r.plane_found) return;
    float q[8];
    for (int k = 0; k < 8; ++k) q[k] = hdr->win[k];
    long long m[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const float4 p = P[i];
        // |v| < 16 m keeps |q| below 2^20 and a squared term below 2^40: 2^22 pixels sum below 2^62
        if (p.w != 0.0f && seg_inlier(p, q) && fabsf(p.x) < 16.0f && fabsf(p.y) < 16.0f && fabsf(p.z) < 16.0f) {
            const long long x = __double2ll_rn((double)p.x * 65536.0), y = __double2ll_rn((double)p.y * 65536.0), z = __double2ll_rn((double)p.z * 65536.0);
            m[0] += 1; m[1] += x; m[2] += y; m[3] += z;
            m[4] += x * x; m[5] += x * y; m[6] += x * z; m[7] += y * y; m[8] += y * z; m[9] += z * z;
        }
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) m[k] = wave_sum_ll(m[k]);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 10; ++k) s_m[threadIdx.x >> 6][k] = m[k];
    __syncthreads();
    if (threadIdx.x < 10) {
        const long long t = (s_m[0][threadIdx.x] + s_m[1][threadIdx.x]) + (s_m[2][threadIdx.x] + s_m[3][threadIdx.x]);
        if (t) atomicAdd((unsigned long long*)&hdr->mom[threadIdx.x], (unsigned long long)t);
    }
}

// the eigenvector of the smallest eigenvalue of a symmetric 3x3: cyclic Jacobi in double, SEG_SWEEPS sweeps
__device__ void seg_smallest_eigvec(double a00, double a01, double a02, double a11, double a12, double a22, double v[3]) {
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < SEG_SWEEPS; ++sweep) {
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            if (A[p][q] == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
            const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < 3; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
            for (int k = 0; k < 3; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
            for (int k = 0; k < 3; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
        }
    }
    int m = 0;
    if (A[1][1] < A[m][m]) m = 1;
    if (A[2][2] < A[m][m]) m = 2;
    v[0] = V[0][m]; v[1] = V[1][m]; v[2] = V[2][m];
}

// one lane: centroid and covariance in double from the integer moments, the normal, the orientation d > 0, one cast to float
__global__ void seg_plane_kernel(SegHeader* __restrict__ hdr) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || !hdr->r.plane_found) return;
    const long long* M = hdr->mom;
    const double n = (double)M[0], u = 1.0 / 65536.0;
    hdr->r.n_refit = (int)M[0];
    double nv[3] = {0, 0, 0}, d = 0;
    bool good = false;
    if (M[0] >= 3) {
        const double cx = (double)M[1] / n * u, cy = (double)M[2] / n * u, cz = (double)M[3] / n * u, uu = u * u;
        double v[3];
        seg_smallest_eigvec((double)M[4] / n * uu - cx * cx, (double)M[5] / n * uu - cx * cy, (double)M[6] / n * uu - cx * cz, (double)M[7] / n * uu - cy * cy,
                            (double)M[8] / n * uu - cy * cz, (double)M[9] / n * uu - cz * cz, v);
        const double l = sqrt(v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]));
        for (int k = 0; k < 3; ++k) nv[k] = v[k] / l;
        d = -(nv[0] * cx + (nv[1] * cy + nv[2] * cz));
        good = isfinite(nv[0]) && isfinite(nv[1]) && isfinite(nv[2]) && isfinite(d);
    }
    if (!good) {   // the winner's own plane
        const double m0 = hdr->win[3], m1 = hdr->win[4], m2 = hdr->win[5];
        const double l = sqrt(m0 * m0 + (m1 * m1 + m2 * m2));
        nv[0] = m0 / l; nv[1] = m1 / l; nv[2] = m2 / l;
        d = -(nv[0] * (double)hdr->win[0] + (nv[1] * (double)hdr->win[1] + nv[2] * (double)hdr->win[2]));
    }
    if (d < 0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; d = -d; }
    hdr->r.plane[0] = (float)nv[0]; hdr->r.plane[1] = (float)nv[1]; hdr->r.plane[2] = (float)nv[2]; hdr->r.plane[3] = (float)d;
}

__global__ __launch_bounds__(256) void seg_heights_kernel(const float4* __restrict__ P, int npix, float tol, float max_height, SegHeader* __restrict__ hdr,
                                                          float* __restrict__ fz, int* __restrict__ L, uint32_t* __restrict__ size) {
    __shared__ int s_n[4][3];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool found = hdr->r.plane_found != 0;
    const float n0 = hdr->r.plane[0], n1 = hdr->r.plane[1], n2 = hdr->r.plane[2], d = hdr->r.plane[3];
    bool on = false, above = false, below = false;
    if (idx < npix) {
        const float4 p = P[idx];
        const bool valid = p.w != 0.0f;
        bool fg = valid;
        if (found) {
            const float h = (n0 * p.x + (n1 * p.y + n2 * p.z)) + d;
            on = valid && fabsf(h) <= tol; above = valid && h > tol; below = valid && h < -tol;
            fg = above && h <= max_height;
        }
        fz[idx] = fg ? p.z : seg_nan();
        L[idx] = fg ? idx : -1;
        size[idx] = 0;
    }
    const int c[3] = {(int)__popcll(__ballot(on)), (int)__popcll(__ballot(above)), (int)__popcll(__ballot(below))};
    wg_add_counts<3>(c, s_n, &hdr->r.n_on_plane);
}

// ---- steps 4a and 4b: the concavity cut in front of the labelling (stocs_segment_frame_convex).  A smoothed point is (xs, ys, zs); off the
// foreground and outside the image all three are NaN, so every test on it is false.
__device__ __forceinline__ V3 seg_nan3() { const float n = seg_nan(); return mk3(n, n, n); }
// zs of the integer window sum, and x, y from it as seg_points forms them from z
__device__ __forceinline__ V3 seg_smoothed_point(uint32_t S, uint32_t N, int i, int j, float fx, float cx, float fy, float cy, float depth_scale) {
    return seg_unproject(i, j, ((float)S / (float)N) * depth_scale, fx, cx, fy, cy);
}
// one triple: bit 0 tested, bit 1 cut
__device__ __forceinline__ int seg_bend_triple(V3 l, V3 c, V3 r, float rf, float jump_abs, float jump_rel, float cos2) {
    if (!(fabsf(l.z - c.z) <= rf * (jump_abs + jump_rel * fminf(c.z, l.z)) && fabsf(r.z - c.z) <= rf * (jump_abs + jump_rel * fminf(c.z, r.z)))) return 0;
    const V3 a = c - l, b = r - c;
    const V3 m = mk3((l.x + r.x) - (c.x + c.x), (l.y + r.y) - (c.y + c.y), (l.z + r.z) - (c.z + c.z));
    const float ab = a.x * b.x + (a.y * b.y + a.z * b.z), aa = a.x * a.x + (a.y * a.y + a.z * a.z), bb = b.x * b.x + (b.y * b.y + b.z * b.z);
    const bool toward = m.x * c.x + (m.y * c.y + m.z * c.z) < 0.0f;
    const bool bend = ab <= 0.0f || ab * ab < cos2 * (aa * bb);
    return (toward && bend) ? 3 : 1;
}
// what a lane leaves of its pixel (th, tv: the two triples' bits); its wavefront's five counts are added to acc, in the order of
// stocs_segment_convex_result's counters (wg_add_counts<5> on &hdr->c.n_tested_h ends either kernel)
__device__ __forceinline__ void seg_bend_store(bool inside, int idx, float z, int th, int tv, float* __restrict__ fz2, int* __restrict__ L, uint8_t* __restrict__ cut, int* acc) {
    const int bits = ((th >> 1) & 1) | (tv & 2);
    if (inside) {
        cut[idx] = (uint8_t)bits;
        fz2[idx] = bits ? seg_nan() : z;
        if (bits) L[idx] = -1;
    }
    acc[0] += __popcll(__ballot(th & 1)); acc[1] += __popcll(__ballot(tv & 1)); acc[2] += __popcll(__ballot(th & 2)); acc[3] += __popcll(__ballot(tv & 2));
    acc[4] += __popcll(__ballot(bits != 0));
}

// form 1, step 4a: a lane per pixel, the window read from device memory
__global__ __launch_bounds__(256) void seg_smooth_kernel(const uint16_t* __restrict__ depth, const float* __restrict__ fz, int W, int H, float fx, float cx, float fy, float cy,
                                                         float depth_scale, float jump_abs, float jump_rel, int s, float4* __restrict__ PS, float* __restrict__ zs_out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= W * H) return;
    const int i = idx / W, j = idx % W;
    const float zc = fz[idx];
    V3 q = seg_nan3();
    if (zc == zc) {
        uint32_t S = 0, N = 0;
        for (int y = max(i - s, 0); y <= min(i + s, H - 1); ++y)
            for (int x = max(j - s, 0); x <= min(j + s, W - 1); ++x)
                if (seg_join(zc, fz[y * W + x], jump_abs, jump_rel)) { S += depth[y * W + x]; ++N; }
        q = seg_smoothed_point(S, N, i, j, fx, cx, fy, cy, depth_scale);
    }
    PS[idx] = make_float4(q.x, q.y, q.z, 0.0f);
    if (zs_out) zs_out[idx] = q.z;
}
// form 1, step 4b: the centre's and the four far smoothed points from device memory
__global__ __launch_bounds__(256) void seg_bend_kernel(const float4* __restrict__ PS, const float* __restrict__ fz, int W, int H, int r, float jump_abs, float jump_rel, float cos2,
                                                       float* __restrict__ fz2, int* __restrict__ L, uint8_t* __restrict__ cut, SegHeader* __restrict__ hdr) {
    __shared__ int s_n[4][5];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool inside = idx < W * H;
    int th = 0, tv = 0;
    if (inside && r > 0) {
        const int i = idx / W, j = idx % W;
        const float4 c4 = PS[idx];
        const V3 c = mk3(c4.x, c4.y, c4.z);
        if (c.z == c.z) {
            const float rf = (float)r;
            if (j - r >= 0 && j + r < W) { const float4 a = PS[idx - r], b = PS[idx + r]; th = seg_bend_triple(mk3(a.x, a.y, a.z), c, mk3(b.x, b.y, b.z), rf, jump_abs, jump_rel, cos2); }
            if (i - r >= 0 && i + r < H) { const float4 a = PS[idx - r * W], b = PS[idx + r * W]; tv = seg_bend_triple(mk3(a.x, a.y, a.z), c, mk3(b.x, b.y, b.z), rf, jump_abs, jump_rel, cos2); }
        }
    }
    int acc[5] = {0, 0, 0, 0, 0};
    seg_bend_store(inside, idx, inside ? fz[idx] : 0.0f, th, tv, fz2, L, cut, acc);
    wg_add_counts<5>(acc, s_n, &hdr->c.n_tested_h);
}

// form 2: a workgroup per tile of SEG_TILE_W x SEG_TILE_H pixels.  Stage: the raw depth of every foreground pixel of the tile and a halo of
// r + s (0: not foreground or outside the image; a foreground pixel's raw depth is never 0); a tile that holds no foreground ends there.  Then the smoothed point of every pixel of the
// tile and a halo of r, once, the window read from the staged depths (the window is gated on the centre's depth, so it is not a separable
// sum; it is an integer sum, so its order is free).  Then both tests from LDS: a wavefront holds a tile row, so its lanes read consecutive words.
enum { SEG_BEND_SW = SEG_TILE_W + 2 * (SEG_MAX_BEND + SEG_MAX_SMOOTH), SEG_BEND_SH = SEG_TILE_H + 2 * (SEG_MAX_BEND + SEG_MAX_SMOOTH),
       SEG_BEND_ZW = SEG_TILE_W + 2 * SEG_MAX_BEND, SEG_BEND_ZH = SEG_TILE_H + 2 * SEG_MAX_BEND };
__global__ __launch_bounds__(256) void seg_bend_tiles_kernel(const uint16_t* __restrict__ depth, const float* __restrict__ fz, int W, int H, float fx, float cx, float fy, float cy,
                                                             float depth_scale, float jump_abs, float jump_rel, int s, int r, float cos2, float* __restrict__ fz2,
                                                             int* __restrict__ L, uint8_t* __restrict__ cut, float* __restrict__ zs_out, SegHeader* __restrict__ hdr) {
    __shared__ uint16_t s_raw[SEG_BEND_SW * SEG_BEND_SH];
    __shared__ float s_x[SEG_BEND_ZW * SEG_BEND_ZH], s_y[SEG_BEND_ZW * SEG_BEND_ZH], s_z[SEG_BEND_ZW * SEG_BEND_ZH];
    __shared__ int s_n[4][5];
    const int x0 = blockIdx.x * SEG_TILE_W, y0 = blockIdx.y * SEG_TILE_H;
    const int hs = r + s, SW = SEG_TILE_W + 2 * hs, SH = SEG_TILE_H + 2 * hs, ZW = SEG_TILE_W + 2 * r, ZH = SEG_TILE_H + 2 * r;
    int own = 0;                                                          // foreground in the tile itself (not its halo)
    for (int t = threadIdx.x; t < SW * SH; t += 256) {
        const int x = x0 - hs + t % SW, y = y0 - hs + t / SW;
        uint16_t v = 0;
        if (x >= 0 && x < W && y >= 0 && y < H) { const float z = fz[y * W + x]; if (z == z) v = depth[y * W + x]; }
        s_raw[t] = v;
        own |= (v != 0 && x >= x0 && x < x0 + SEG_TILE_W && y >= y0 && y < y0 + SEG_TILE_H) ? 1 : 0;
    }
    if (!__syncthreads_or(own)) {                                         // a tile without foreground (the support plane, the background): nothing to smooth, test or count
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + (threadIdx.x & 63), y = y0 + (threadIdx.x >> 6) * 4 + k;
            if (x < W && y < H) { cut[y * W + x] = 0; fz2[y * W + x] = seg_nan(); if (zs_out) zs_out[y * W + x] = seg_nan(); }
        }
        return;
    }
    for (int t = threadIdx.x; t < ZW * ZH; t += 256) {
        const int lx = t % ZW, ly = t / ZW, x = x0 - r + lx, y = y0 - r + ly;
        const uint16_t* row = s_raw + (ly + s) * SW + (lx + s);          // the centre in the staged block; the window around it lies inside the block
        const uint32_t rc = row[0];
        V3 q = seg_nan3();
        if (rc) {
            const float zc = (float)rc * depth_scale;
            uint32_t S = 0, N = 0;
            for (int dy = -s; dy <= s; ++dy)
                for (int dx = -s; dx <= s; ++dx) {
                    const uint32_t rw = row[dy * SW + dx];
                    if (rw && seg_join(zc, (float)rw * depth_scale, jump_abs, jump_rel)) { S += rw; ++N; }
                }
            q = seg_smoothed_point(S, N, y, x, fx, cx, fy, cy, depth_scale);
            if (zs_out && lx >= r && lx < r + SEG_TILE_W && ly >= r && ly < r + SEG_TILE_H) zs_out[y * W + x] = q.z;     // rc != 0: inside the image
        } else if (zs_out && lx >= r && lx < r + SEG_TILE_W && ly >= r && ly < r + SEG_TILE_H && x < W && y < H) {
            zs_out[y * W + x] = q.z;
        }
        s_x[t] = q.x; s_y[t] = q.y; s_z[t] = q.z;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float rf = (float)r;
    int acc[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ty = wave * 4 + k, x = x0 + lane, y = y0 + ty;
        const bool inside = x < W && y < H;
        const int at = (ty + r) * ZW + (lane + r);
        const uint32_t rc = s_raw[(ty + hs) * SW + (lane + hs)];
        int th = 0, tv = 0;
        if (r > 0 && rc) {
            const V3 c = mk3(s_x[at], s_y[at], s_z[at]);
            th = seg_bend_triple(mk3(s_x[at - r], s_y[at - r], s_z[at - r]), c, mk3(s_x[at + r], s_y[at + r], s_z[at + r]), rf, jump_abs, jump_rel, cos2);
            tv = seg_bend_triple(mk3(s_x[at - r * ZW], s_y[at - r * ZW], s_z[at - r * ZW]), c, mk3(s_x[at + r * ZW], s_y[at + r * ZW], s_z[at + r * ZW]), rf, jump_abs, jump_rel, cos2);
        }
        seg_bend_store(inside, y * W + x, rc ? (float)rc * depth_scale : seg_nan(), th, tv, fz2, L, cut, acc);
    }
    wg_add_counts<5>(acc, s_n, &hdr->c.n_tested_h);
}

// ---- union-find.  L[x] <= x always, L[x] is in x's component, and only a root (L[x] == x) is ever given a new parent by the link below, or
// a node a smaller one: values only fall.  A read may be stale (another compute unit's L1 is not refreshed): it then names an earlier parent,
// still an ancestor, so a find only walks further; the link itself is an atomic at the L2.  No lane ever waits for another.
// SCOPE: the memory scope of the plain reads, __HIP_MEMORY_SCOPE_AGENT for labels in device memory, __HIP_MEMORY_SCOPE_WORKGROUP for a tile's in LDS.
template <int SCOPE>
__device__ __forceinline__ int seg_find(int* L, int x) {
    for (;;) { const int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, SCOPE); if (p == x) return x; x = p; }
}
template <int SCOPE>
__device__ __forceinline__ void seg_union(int* L, int a, int b) {
    for (;;) {
        a = seg_find<SCOPE>(L, a); b = seg_find<SCOPE>(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b);       // a > b: a's parent becomes b unless somebody gave it a smaller one
        if (old == a) return;
        a = old;                                   // a had a parent `old` < a by now: its tree still has to meet b's
    }
}

// form 1: every foreground pixel joins its left and its upper neighbour in device memory
__global__ __launch_bounds__(256) void seg_union_global_kernel(const float* __restrict__ fz, int W, int H, float jump_abs, float jump_rel, int* L) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= W * H) return;
    const float z = fz[idx];
    if (!(z == z)) return;
    const int i = idx / W, j = idx % W;
    if (j > 0 && seg_join(z, fz[idx - 1], jump_abs, jump_rel)) seg_union<__HIP_MEMORY_SCOPE_AGENT>(L, idx, idx - 1);
    if (i > 0 && seg_join(z, fz[idx - W], jump_abs, jump_rel)) seg_union<__HIP_MEMORY_SCOPE_AGENT>(L, idx, idx - W);
}

// form 2: a workgroup labels one tile of SEG_TILE_W x SEG_TILE_H pixels in LDS.  A wavefront holds a tile row: one ballot of "joins its left
// neighbour" gives every lane the head of its run (the highest lane at or below it that does not join).  Union-find runs on the heads only: a
// pixel links its run to the run above when it joins upward and the pixel to its left does not already make the same link.  The tile's local
// order is the frame's linear order restricted to the tile, so a local root is the lowest frame index of its part of the component.
__global__ __launch_bounds__(256) void seg_tiles_kernel(const float* __restrict__ fz, int W, int H, float jump_abs, float jump_rel, int* __restrict__ L) {
    __shared__ int s_lab[SEG_TILE_W * SEG_TILE_H];
    __shared__ unsigned long long s_jl[SEG_TILE_H];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * SEG_TILE_W + lane, y0 = blockIdx.y * SEG_TILE_H;
    const float nanf_ = seg_nan();
    float z[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = wave * 4 + k, y = y0 + r;
        z[k] = (x < W && y < H) ? fz[(size_t)y * W + x] : nanf_;
        float zl = __shfl_up(z[k], 1, 64);
        if (lane == 0) zl = nanf_;
        const unsigned long long jl = __ballot(seg_join(z[k], zl, jump_abs, jump_rel));
        if (lane == 0) s_jl[r] = jl;
        const unsigned long long heads = ~jl & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));   // bit 0 is always set
        s_lab[r * SEG_TILE_W + lane] = (z[k] == z[k]) ? r * SEG_TILE_W + (63 - __clzll((long long)heads)) : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = wave * 4 + k, y = y0 + r;
        if (r == 0) continue;
        const float zu = (x < W && y < H) ? fz[(size_t)(y - 1) * W + x] : nanf_;
        const bool ju = seg_join(z[k], zu, jump_abs, jump_rel);
        const unsigned long long ub = __ballot(ju);
        const unsigned long long same = s_jl[r] & (ub << 1) & s_jl[r - 1];     // my left neighbour is in my run, joins upward, and its upper one is in my upper one's run
        if (ju && !((same >> lane) & 1ull)) seg_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, r * SEG_TILE_W + lane, (r - 1) * SEG_TILE_W + lane);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = wave * 4 + k, y = y0 + r;
        if (!(z[k] == z[k])) continue;
        const int root = seg_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, r * SEG_TILE_W + lane);
        L[(size_t)y * W + x] = (y0 + root / SEG_TILE_W) * W + blockIdx.x * SEG_TILE_W + root % SEG_TILE_W;
    }
}
// the joins that cross a tile border, one lane per border pixel: first the (ntx - 1) * H pixels of the left columns, then the (nty - 1) * W of the top rows
__global__ __launch_bounds__(256) void seg_borders_kernel(const float* __restrict__ fz, int W, int H, int n_col, int n_all, float jump_abs, float jump_rel, int* L) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_all) return;
    int idx, nb;
    if (t < n_col) { const int y = t % H, x = (t / H + 1) * SEG_TILE_W; idx = y * W + x; nb = idx - 1; }
    else { const int u = t - n_col, x = u % W, y = (u / W + 1) * SEG_TILE_H; idx = y * W + x; nb = idx - W; }
    if (seg_join(fz[idx], fz[nb], jump_abs, jump_rel)) seg_union<__HIP_MEMORY_SCOPE_AGENT>(L, idx, nb);
}
__global__ __launch_bounds__(256) void seg_flatten_kernel(int npix, int* L) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix) return;
    const int p = __hip_atomic_load(&L[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p < 0 || p == idx) return;
    const int r = seg_find<__HIP_MEMORY_SCOPE_AGENT>(L, p);
    if (r != p) __hip_atomic_store(&L[idx], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // a root's own entry is never written here
}

// pixels per root: the lanes of a wavefront that share the first lane's root add once
__global__ __launch_bounds__(256) void seg_sizes_kernel(const int* __restrict__ L, int npix, uint32_t* __restrict__ size) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = idx < npix ? L[idx] : -1;
    const unsigned long long act = __ballot(r >= 0);
    if (!act) return;
    const int r0 = __shfl(r, (int)__ffsll((long long)act) - 1, 64);
    const unsigned long long same = __ballot(r == r0);
    if (r == r0) { if ((int)(threadIdx.x & 63) == (int)__ffsll((long long)same) - 1) atomicAdd(&size[r0], (uint32_t)__popcll(same)); }
    else if (r >= 0) atomicAdd(&size[r], 1u);
}
__global__ __launch_bounds__(256) void seg_keep_kernel(const int* __restrict__ L, const uint32_t* __restrict__ size, int npix, uint32_t min_pixels, uint32_t* __restrict__ keep,
                                                       SegHeader* __restrict__ hdr) {
    __shared__ int s_n[4][1];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = idx < npix && L[idx] == idx;
    if (idx <= npix) keep[idx] = (root && size[idx] >= min_pixels) ? 1u : 0u;     // entry npix: the scan's total
    const int c = __popcll(__ballot(root));
    wg_add_counts<1>(&c, s_n, &hdr->r.n_components);
}
__global__ __launch_bounds__(256) void seg_records_init_kernel(const uint32_t* __restrict__ keep, const uint32_t* __restrict__ kpos, const uint32_t* __restrict__ size, int npix,
                                                               stocs_segment_record* __restrict__ rec, SegHeader* __restrict__ hdr) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0) hdr->r.n_segments = (int)kpos[npix];
    if (idx >= npix || !keep[idx]) return;
    stocs_segment_record r;
    r.root = idx; r.pixels = (int)size[idx]; r.c0 = 0x7FFFFFFF; r.r0 = 0x7FFFFFFF; r.c1 = -1; r.r1 = -1;
    r.zmin = INFINITY; r.zmax = 0.0f;
    rec[kpos[idx]] = r;
}
// labels, the class image, and the records' boxes and depth extremes: integer minima and maxima (a foreground depth is positive, so its
// bits order as the floats do).  The lanes of a wavefront that share the first labelled lane's segment reduce by shuffles first.
__global__ __launch_bounds__(256) void seg_relabel_kernel(const int* __restrict__ L, const float* __restrict__ fz, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ kpos,
                                                          int W, int npix, int32_t* __restrict__ labels, uint16_t* __restrict__ cls, stocs_segment_record* rec) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    int lab = 0;
    if (idx < npix) {
        const int r = L[idx];
        if (r >= 0 && keep[r]) lab = (int)kpos[r] + 1;
        labels[idx] = lab;
        cls[idx] = lab ? (uint16_t)10000 : (uint16_t)0;
    }
    const unsigned long long act = __ballot(lab != 0);
    if (!act) return;
    const int lab0 = __shfl(lab, (int)__ffsll((long long)act) - 1, 64);
    const bool mine = lab == lab0;
    const int row = idx < npix ? idx / W : 0, col = idx < npix ? idx % W : 0;
    const int zb = lab ? __float_as_int(fz[idx]) : 0;
    const int big = 0x7FFFFFFF;
    const int c0 = wave_min_i(mine ? col : big), r0 = wave_min_i(mine ? row : big), c1 = wave_max_i(mine ? col : -1), r1 = wave_max_i(mine ? row : -1);
    const int z0 = wave_min_i(mine ? zb : big), z1 = wave_max_i(mine ? zb : 0);
    if (mine) {
        if ((int)(threadIdx.x & 63) == (int)__ffsll((long long)act) - 1) {
            stocs_segment_record* q = rec + (lab0 - 1);
            atomicMin(&q->c0, c0); atomicMin(&q->r0, r0); atomicMax(&q->c1, c1); atomicMax(&q->r1, r1);
            atomicMin((int*)&q->zmin, z0); atomicMax((int*)&q->zmax, z1);
        }
    } else if (lab) {
        stocs_segment_record* q = rec + (lab - 1);
        atomicMin(&q->c0, col); atomicMin(&q->r0, row); atomicMax(&q->c1, col); atomicMax(&q->r1, row);
        atomicMin((int*)&q->zmin, zb); atomicMax((int*)&q->zmax, zb);
    }
}
__global__ __launch_bounds__(256) void seg_edges_kernel(const int32_t* __restrict__ labels, int W, int H, uint8_t* __restrict__ edge) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= W * H) return;
    const int i = idx / W, j = idx % W, lab = labels[idx];
    bool in = lab != 0;
    if (in && j > 0) in = labels[idx - 1] == lab;
    if (in && j + 1 < W) in = labels[idx + 1] == lab;
    if (in && i > 0) in = labels[idx - W] == lab;
    if (in && i + 1 < H) in = labels[idx + W] == lab;
    edge[idx] = in ? 255 : 0;
}

// ---- the calling thread's cached memory (stocs_trim gives it back through segment_trim): the arena per device and the pinned block
// (an instance of its own: a thread that also ingests keeps both), and what its last call left
static thread_local ThreadCache tl_seg_cache;

// What the thread's last call left for the three stocs_segment_last_* entry points, one validity state each, and the clock behind two of
// them (STOCS_SEGMENT_CLOCK=1): HIP events at named marks of the launch sequence, owned with the device they were made on.  Plain data,
// all zero at first, so that it can be thread_local.
struct SegLast {
    enum Mark { SCORE_BEGIN, SCORE_END, BEND_BEGIN, BEND_END, LABEL_BEGIN, LABEL_END, N_MARKS };
    hipEvent_t ev[N_MARKS];
    bool ev_made; int ev_dev;
    float score_ms, label_ms, bend_ms;
    long long mom[10];
    bool ms_valid, bend_valid, mom_valid;     // stocs_segment_last_device_ms, _bend_ms, _moments

    void invalidate() { ms_valid = bend_valid = mom_valid = false; }
    // the events, on `dev`: made by the thread's first clocked call, and anew when it has moved to another device
    int arm(int dev) {
        if (ev_made && ev_dev != dev) drop_events();
        if (!ev_made) { for (int k = 0; k < N_MARKS; ++k) STOCS_HIP_CHECK(hipEventCreate(&ev[k])); ev_made = true; ev_dev = dev; }
        return STOCS_OK;
    }
    // behind the call's synchronisation: the moments always, the times of a clocked call, the bend step's of a clocked convex call
    int read(const long long* moments, bool clocked, bool bend) {
        for (int k = 0; k < 10; ++k) mom[k] = moments[k];
        mom_valid = true;
        if (!clocked) return STOCS_OK;
        STOCS_HIP_CHECK(hipEventElapsedTime(&score_ms, ev[SCORE_BEGIN], ev[SCORE_END]));
        STOCS_HIP_CHECK(hipEventElapsedTime(&label_ms, ev[LABEL_BEGIN], ev[LABEL_END]));
        ms_valid = true;
        if (bend) { STOCS_HIP_CHECK(hipEventElapsedTime(&bend_ms, ev[BEND_BEGIN], ev[BEND_END])); bend_valid = true; }
        return STOCS_OK;
    }
    void drop_events() { if (ev_made) { for (int k = 0; k < N_MARKS; ++k) (void)hipEventDestroy(ev[k]); ev_made = false; } }
};
static thread_local SegLast tl_seg_last;

void segment_trim() {
    tl_seg_cache.trim();
    tl_seg_last.drop_events();
    segment_shapes_trim();
}

// STOCS_SEGMENT_FORM, STOCS_SEGMENT_BEND_FORM: unset, empty or 0 (the default), 1 or 2; what_1, what_2 name the two forms in the refusal
static int env_form(const char* name, const char* what_1, const char* what_2, int* form) {
    const char* e = getenv(name);
    *form = 0;
    if (!e || !*e) return STOCS_OK;
    if ((e[0] == '0' || e[0] == '1' || e[0] == '2') && e[1] == 0) { *form = e[0] - '0'; return STOCS_OK; }
    set_error("%s=%s: 0 (default), 1 (%s) or 2 (%s)", name, e, what_1, what_2);
    return STOCS_ERR_INVALID;
}
// the default label form: the one that was faster in every row of profiles/segment_time.json
enum { SEG_DEFAULT_FORM = 2 };
// the default bend form: the one that was faster on the camera frames of profiles/segment_convex_time.json: 20 - 29 us
// against 30 - 35 us at 640 x 480; the tiled form is ahead only where the whole frame is foreground
enum { SEG_DEFAULT_BEND_FORM = 1 };

}  // namespace stocs

using namespace stocs;

extern "C" {

void stocs_default_segment_params(stocs_segment_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_depth = 2.0f; p->plane_hypotheses = 1024; p->score_stride = 4; p->plane_tolerance = 0.01f; p->plane_min_share = 0.15f;
    p->max_height = 0.5f; p->jump_abs = 0.005f; p->jump_rel = 0.01f; p->min_pixels = 200; p->seed = 1;
}

int stocs_check_segment_params(const stocs_segment_params* p) {
    if (!p) { set_error("stocs_check_segment_params: NULL params"); return STOCS_ERR_INVALID; }
    if (!(p->max_depth > 0) || !std::isfinite(p->max_depth)) { set_error("segment params: max_depth %g is not finite or not above 0", (double)p->max_depth); return STOCS_ERR_INVALID; }
    if (p->plane_hypotheses < 0 || p->plane_hypotheses > SEG_MAX_HYP) { set_error("segment params: plane_hypotheses %d outside 0..%d", p->plane_hypotheses, (int)SEG_MAX_HYP); return STOCS_ERR_INVALID; }
    if (p->score_stride < 1) { set_error("segment params: score_stride %d < 1", p->score_stride); return STOCS_ERR_INVALID; }
    if (!(p->plane_tolerance > 0) || !std::isfinite(p->plane_tolerance)) { set_error("segment params: plane_tolerance %g is not finite or not above 0", (double)p->plane_tolerance); return STOCS_ERR_INVALID; }
    if (!(p->plane_min_share >= 0 && p->plane_min_share <= 1)) { set_error("segment params: plane_min_share %g outside [0, 1]", (double)p->plane_min_share); return STOCS_ERR_INVALID; }
    if (!(p->max_height > 0) || !std::isfinite(p->max_height)) { set_error("segment params: max_height %g is not finite or not above 0", (double)p->max_height); return STOCS_ERR_INVALID; }
    if (!(p->jump_abs >= 0) || !std::isfinite(p->jump_abs)) { set_error("segment params: jump_abs %g is not finite or below 0", (double)p->jump_abs); return STOCS_ERR_INVALID; }
    if (!(p->jump_rel >= 0) || !std::isfinite(p->jump_rel)) { set_error("segment params: jump_rel %g is not finite or below 0", (double)p->jump_rel); return STOCS_ERR_INVALID; }
    if (p->min_pixels < 1) { set_error("segment params: min_pixels %d < 1", p->min_pixels); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}

void stocs_default_segment_convex_params(stocs_segment_convex_params* cp) {
    if (!cp) return;
    memset(cp, 0, sizeof(*cp));
    cp->bend_radius = 4; cp->smooth_radius = 2; cp->bend_cos = 0.90630779f;
}

int stocs_check_segment_convex_params(const stocs_segment_convex_params* cp) {
    if (!cp) { set_error("stocs_check_segment_convex_params: NULL params"); return STOCS_ERR_INVALID; }
    if (cp->bend_radius < 0 || cp->bend_radius > SEG_MAX_BEND) { set_error("segment convex params: bend_radius %d outside 0..%d", cp->bend_radius, (int)SEG_MAX_BEND); return STOCS_ERR_INVALID; }
    if (cp->smooth_radius < 0 || cp->smooth_radius > SEG_MAX_SMOOTH) { set_error("segment convex params: smooth_radius %d outside 0..%d", cp->smooth_radius, (int)SEG_MAX_SMOOTH); return STOCS_ERR_INVALID; }
    if (!(cp->bend_cos >= 0 && cp->bend_cos <= 1)) { set_error("segment convex params: bend_cos %g outside [0, 1]", (double)cp->bend_cos); return STOCS_ERR_INVALID; }
    if (cp->reserved != 0) { set_error("segment convex params: reserved %d is not 0", cp->reserved); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}

int stocs_segment_last_bend_ms(float* bend_ms) {
    if (!tl_seg_last.bend_valid) { set_error("stocs_segment_last_bend_ms: no stocs_segment_frame_convex of this thread ran with STOCS_SEGMENT_CLOCK=1"); return STOCS_ERR_STATE; }
    if (bend_ms) *bend_ms = tl_seg_last.bend_ms;
    return STOCS_OK;
}

int stocs_segment_tile(int* width, int* height) {
    if (width) *width = SEG_TILE_W;
    if (height) *height = SEG_TILE_H;
    return STOCS_OK;
}

int stocs_segment_last_device_ms(float* score_ms, float* label_ms) {
    if (!tl_seg_last.ms_valid) { set_error("stocs_segment_last_device_ms: no stocs_segment_frame of this thread ran with STOCS_SEGMENT_CLOCK=1"); return STOCS_ERR_STATE; }
    if (score_ms) *score_ms = tl_seg_last.score_ms;
    if (label_ms) *label_ms = tl_seg_last.label_ms;
    return STOCS_OK;
}

int stocs_segment_last_moments(int64_t* moments10) {
    if (!moments10) { set_error("stocs_segment_last_moments: NULL output"); return STOCS_ERR_INVALID; }
    if (!tl_seg_last.mom_valid) { set_error("stocs_segment_last_moments: no stocs_segment_frame of this thread has run"); return STOCS_ERR_STATE; }
    for (int k = 0; k < 10; ++k) moments10[k] = (int64_t)tl_seg_last.mom[k];
    return STOCS_OK;
}

}  // extern "C"

namespace stocs {
// what an entry point hands to the one launch sequence: its name for messages, and where the results go (each image may be NULL)
struct SegCall {
    const char* who;
    uint16_t* class_prob; int32_t* labels; uint8_t* edge; uint8_t* cut; float* smoothed;
    stocs_segment_record* records; int cap_records;
    stocs_segment_result* out; stocs_segment_convex_result* cout;
};
static int seg_refuse_null(const char* who) { set_error("%s: NULL camera, depth image, params or result", who); return STOCS_ERR_INVALID; }

// Both entry points: one launch sequence.  cp == NULL is stocs_segment_frame: no bend step, the label kernels read the foreground depth image
// itself.  The entry point has refused its NULL pointers.
static int segment_run(const stocs_camera* cam, const uint16_t* depth, const stocs_segment_params* p, const stocs_segment_convex_params* cp, int device, const SegCall& o) {
    const char* who = o.who;
    if (cam->width < 1 || cam->height < 1) { set_error("%s: frame of %d x %d pixels", who, cam->width, cam->height); return STOCS_ERR_INVALID; }
    int rc = stocs_check_segment_params(p);
    if (rc) return rc;
    if (cp && (rc = stocs_check_segment_convex_params(cp))) return rc;
    if (o.cap_records < 0 || (!o.records && o.cap_records > 0)) { set_error("%s: cap_records %d with %s records", who, o.cap_records, o.records ? "given" : "NULL"); return STOCS_ERR_INVALID; }
    if ((long long)cam->width * cam->height > (long long)SEG_MAX_PIX) { set_error("%s: %d x %d pixels, above 2^22 (the refit's moments are 64-bit sums)", who, cam->width, cam->height); return STOCS_ERR_CAPACITY; }
    int form = 0, bform = 0;
    if ((rc = env_form("STOCS_SEGMENT_FORM", "device-memory union-find", "tiles in LDS", &form))) return rc;
    if (cp && (rc = env_form("STOCS_SEGMENT_BEND_FORM", "a lane per pixel, device memory", "tiles in LDS", &bform))) return rc;
    if (form == 0) form = SEG_DEFAULT_FORM;
    if (bform == 0) bform = SEG_DEFAULT_BEND_FORM;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available: this library has no CPU fallback"); return STOCS_ERR_NO_DEVICE; }
    if (device >= 0) STOCS_HIP_CHECK(hipSetDevice(device));
    SegLast& last = tl_seg_last;
    last.invalidate();                                                                  // a call refused above leaves the last call's record as it was

    const int W = cam->width, H = cam->height, npix = W * H, s = p->score_stride, Hn = p->plane_hypotheses;
    const int LW = (W + s - 1) / s, LH = (H + s - 1) / s, nl = LW * LH;
    const int ntx = (W + SEG_TILE_W - 1) / SEG_TILE_W, nty = (H + SEG_TILE_H - 1) / SEG_TILE_H;   // the tiles of seg_bend_tiles and seg_tiles
    const size_t nrec_dev = (size_t)npix / (size_t)p->min_pixels;                       // no more segments than this fit the frame
    const size_t nrec_copy = std::min<size_t>(nrec_dev, (size_t)o.cap_records);
    hipStream_t st = NULL;

    Arena* ws = NULL;
    if ((rc = tl_seg_cache.begin(device, &ws))) return rc;

    // the block that comes back in one copy: header | labels | class image | edge image | records
    Carve oc;
    const size_t o_hdr = oc.take(sizeof(SegHeader)), o_lab = oc.take(4 * (size_t)npix), o_cls = oc.take(2 * (size_t)npix), o_edge = oc.take((size_t)npix);
    const size_t o_cut = cp ? oc.take((size_t)npix) : 0, o_zs = (cp && o.smoothed) ? oc.take(4 * (size_t)npix) : 0;       // in front of the records: they come back too
    const size_t o_rec = oc.take(32 * std::max<size_t>(nrec_dev, 1));
    const size_t back_bytes = o_rec + 32 * nrec_copy;
    char* pin = NULL;
    if ((rc = tl_seg_cache.staging(al256(back_bytes) + 2 * (size_t)npix, &pin))) return rc;
    char* pin_depth = pin + al256(back_bytes);

    char* d_out = NULL; uint16_t* dD = NULL; float4 *P = NULL, *SP = NULL; uint32_t *lat_flag = NULL, *lat_pos = NULL, *cnt = NULL, *size = NULL, *keep = NULL, *kpos = NULL;
    float *hyp = NULL, *fz = NULL, *fz2 = NULL; float4* PS = NULL; int* L = NULL; char* tmp = NULL;
    size_t tb_lat = 0, tb_keep = 0;
    STOCS_HIP_CHECK(exclusive_scan(NULL, tb_lat, lat_flag, lat_pos, (size_t)nl + 1, st));
    STOCS_HIP_CHECK(exclusive_scan(NULL, tb_keep, keep, kpos, (size_t)npix + 1, st));
    if ((rc = ws->take(oc.total, (void**)&d_out)) || (rc = ws->take(2 * (size_t)npix, (void**)&dD)) || (rc = ws->take(16 * (size_t)npix, (void**)&P)) ||
        (rc = ws->take(16 * (size_t)nl, (void**)&SP)) || (rc = ws->take(4 * ((size_t)nl + 1), (void**)&lat_flag)) || (rc = ws->take(4 * ((size_t)nl + 1), (void**)&lat_pos)) ||
        (rc = ws->take(4 * (size_t)std::max(Hn, 1), (void**)&cnt)) || (rc = ws->take(32 * (size_t)std::max(Hn, 1), (void**)&hyp)) || (rc = ws->take(4 * (size_t)npix, (void**)&fz)) ||
        (rc = ws->take(4 * (size_t)npix, (void**)&L)) || (rc = ws->take(4 * (size_t)npix, (void**)&size)) || (rc = ws->take(4 * ((size_t)npix + 1), (void**)&keep)) ||
        (rc = ws->take(4 * ((size_t)npix + 1), (void**)&kpos)) || (rc = ws->take(std::max(tb_lat, tb_keep), (void**)&tmp)))
        return rc;
    if (cp && ((rc = ws->take(4 * (size_t)npix, (void**)&fz2)) || (bform == 1 && (rc = ws->take(16 * (size_t)npix, (void**)&PS))))) return rc;
    SegHeader* hdr = Carve::at<SegHeader>(d_out, o_hdr);
    int32_t* d_lab = Carve::at<int32_t>(d_out, o_lab); uint16_t* d_cls = Carve::at<uint16_t>(d_out, o_cls); uint8_t* d_edge = Carve::at<uint8_t>(d_out, o_edge);
    uint8_t* d_cut = cp ? Carve::at<uint8_t>(d_out, o_cut) : NULL; float* d_zs = (cp && o.smoothed) ? Carve::at<float>(d_out, o_zs) : NULL;
    stocs_segment_record* d_rec = Carve::at<stocs_segment_record>(d_out, o_rec);

    const char* ce = getenv("STOCS_SEGMENT_CLOCK");
    const bool clock = ce != NULL && atoi(ce) == 1;
    if (clock && (rc = last.arm(tl_seg_cache.dev))) return rc;
    const auto mark = [&](SegLast::Mark m) { return clock ? hipEventRecord(last.ev[m], st) : hipSuccess; };

    memcpy(pin_depth, depth, 2 * (size_t)npix);
    STOCS_HIP_CHECK(hipMemcpyAsync(dD, pin_depth, 2 * (size_t)npix, hipMemcpyHostToDevice, st));
    STOCS_HIP_CHECK(hipMemsetAsync(hdr, 0, sizeof(SegHeader), st));
    STOCS_HIP_CHECK(hipMemsetAsync(lat_flag, 0, 4 * ((size_t)nl + 1), st));
    STOCS_HIP_CHECK(hipMemsetAsync(cnt, 0, 4 * (size_t)std::max(Hn, 1), st));
    const dim3 B(256), gp((unsigned)((npix + 255) / 256)), gp1((unsigned)((npix + 256) / 256)), gl((unsigned)((nl + 255) / 256)), gt((unsigned)ntx, (unsigned)nty);
    hipLaunchKernelGGL(seg_points_kernel, gp, B, 0, st, dD, W, H, cam->fx, cam->cx, cam->fy, cam->cy, cam->depth_scale, p->max_depth, s, LW, P, lat_flag, hdr);
    STOCS_HIP_CHECK(exclusive_scan(tmp, tb_lat, lat_flag, lat_pos, (size_t)nl + 1, st));
    hipLaunchKernelGGL(seg_compact_kernel, gl, B, 0, st, P, W, s, LW, nl, lat_flag, lat_pos, SP);
    STOCS_HIP_CHECK(mark(SegLast::SCORE_BEGIN));
    if (Hn > 0) {
        hipLaunchKernelGGL(seg_hypotheses_kernel, dim3((unsigned)((Hn + 255) / 256)), B, 0, st, P, (uint32_t)npix, Hn, p->seed, p->plane_tolerance, hyp);
        hipLaunchKernelGGL(seg_score_kernel, dim3((unsigned)((nl + SEG_SCORE_PTS - 1) / SEG_SCORE_PTS), (unsigned)((Hn + SEG_SCORE_HYP - 1) / SEG_SCORE_HYP)), B, 0, st, SP, lat_pos + nl, hyp, Hn, cnt);
    }
    hipLaunchKernelGGL(seg_winner_kernel, dim3(1), B, 0, st, hyp, cnt, Hn, lat_pos + nl, p->plane_min_share, hdr);
    STOCS_HIP_CHECK(mark(SegLast::SCORE_END));
    if (Hn > 0) {
        hipLaunchKernelGGL(seg_refit_kernel, dim3(std::min(gp.x, 256u)), B, 0, st, P, npix, hdr);
        hipLaunchKernelGGL(seg_plane_kernel, dim3(1), dim3(64), 0, st, hdr);
    }
    hipLaunchKernelGGL(seg_heights_kernel, gp, B, 0, st, P, npix, p->plane_tolerance, p->max_height, hdr, fz, L, size);
    const float* lz = fz;                                                               // the depth image the label kernels and the relabelling read
    if (cp) {
        const float cos2 = cp->bend_cos * cp->bend_cos;
        STOCS_HIP_CHECK(mark(SegLast::BEND_BEGIN));
        if (bform == 1) {
            hipLaunchKernelGGL(seg_smooth_kernel, gp, B, 0, st, dD, fz, W, H, cam->fx, cam->cx, cam->fy, cam->cy, cam->depth_scale, p->jump_abs, p->jump_rel, cp->smooth_radius, PS, d_zs);
            hipLaunchKernelGGL(seg_bend_kernel, gp, B, 0, st, PS, fz, W, H, cp->bend_radius, p->jump_abs, p->jump_rel, cos2, fz2, L, d_cut, hdr);
        } else {
            hipLaunchKernelGGL(seg_bend_tiles_kernel, gt, B, 0, st, dD, fz, W, H, cam->fx, cam->cx, cam->fy, cam->cy, cam->depth_scale, p->jump_abs, p->jump_rel, cp->smooth_radius,
                               cp->bend_radius, cos2, fz2, L, d_cut, d_zs, hdr);
        }
        STOCS_HIP_CHECK(mark(SegLast::BEND_END));
        lz = fz2;
    }
    STOCS_HIP_CHECK(mark(SegLast::LABEL_BEGIN));
    if (form == 1) {
        hipLaunchKernelGGL(seg_union_global_kernel, gp, B, 0, st, lz, W, H, p->jump_abs, p->jump_rel, L);
    } else {
        hipLaunchKernelGGL(seg_tiles_kernel, gt, B, 0, st, lz, W, H, p->jump_abs, p->jump_rel, L);
        const int n_col = (ntx - 1) * H, n_all = n_col + (nty - 1) * W;
        if (n_all > 0) hipLaunchKernelGGL(seg_borders_kernel, dim3((unsigned)((n_all + 255) / 256)), B, 0, st, lz, W, H, n_col, n_all, p->jump_abs, p->jump_rel, L);
    }
    hipLaunchKernelGGL(seg_flatten_kernel, gp, B, 0, st, npix, L);
    STOCS_HIP_CHECK(mark(SegLast::LABEL_END));
    hipLaunchKernelGGL(seg_sizes_kernel, gp, B, 0, st, L, npix, size);
    hipLaunchKernelGGL(seg_keep_kernel, gp1, B, 0, st, L, size, npix, (uint32_t)p->min_pixels, keep, hdr);
    STOCS_HIP_CHECK(exclusive_scan(tmp, tb_keep, keep, kpos, (size_t)npix + 1, st));
    hipLaunchKernelGGL(seg_records_init_kernel, gp, B, 0, st, keep, kpos, size, npix, d_rec, hdr);
    hipLaunchKernelGGL(seg_relabel_kernel, gp, B, 0, st, L, lz, keep, kpos, W, npix, d_lab, d_cls, d_rec);
    hipLaunchKernelGGL(seg_edges_kernel, gp, B, 0, st, d_lab, W, H, d_edge);
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(hipMemcpyAsync(pin, d_out, back_bytes, hipMemcpyDeviceToHost, st));
    STOCS_HIP_CHECK(hipStreamSynchronize(st));

    const SegHeader* h = Carve::at<const SegHeader>(pin, o_hdr);
    stocs_segment_result* out = o.out;
    *out = h->r;
    if (o.cout) *o.cout = h->c;
    if (!out->plane_found) { out->plane[0] = out->plane[1] = out->plane[2] = out->plane[3] = 0.0f; out->n_refit = 0; }
    if ((rc = last.read(h->mom, clock, cp != NULL))) return rc;
    if (out->n_segments > o.cap_records) { set_error("%s: %d segments, cap_records %d", who, out->n_segments, o.cap_records); return STOCS_ERR_CAPACITY; }
    if (o.labels) memcpy(o.labels, pin + o_lab, 4 * (size_t)npix);
    if (o.class_prob) memcpy(o.class_prob, pin + o_cls, 2 * (size_t)npix);
    if (o.edge) memcpy(o.edge, pin + o_edge, (size_t)npix);
    if (o.cut) memcpy(o.cut, pin + o_cut, (size_t)npix);
    if (o.smoothed) memcpy(o.smoothed, pin + o_zs, 4 * (size_t)npix);
    if (out->n_segments > 0) memcpy(o.records, pin + o_rec, 32 * (size_t)out->n_segments);
    return STOCS_OK;
}
}  // namespace stocs

extern "C" {

int stocs_segment_frame(const stocs_camera* cam, const uint16_t* depth, const stocs_segment_params* p, int device, uint16_t* class_prob, int32_t* labels,
                        uint8_t* edge, stocs_segment_record* records, int cap_records, stocs_segment_result* out) {
    const SegCall o = {"stocs_segment_frame", class_prob, labels, edge, NULL, NULL, records, cap_records, out, NULL};
    if (!(cam && depth && p && out)) return seg_refuse_null(o.who);
    return segment_run(cam, depth, p, NULL, device, o);
}

int stocs_segment_frame_convex(const stocs_camera* cam, const uint16_t* depth, const stocs_segment_params* p, const stocs_segment_convex_params* cp, int device,
                               uint16_t* class_prob, int32_t* labels, uint8_t* edge, uint8_t* cut, float* smoothed, stocs_segment_record* records, int cap_records,
                               stocs_segment_result* out, stocs_segment_convex_result* cout) {
    const SegCall o = {"stocs_segment_frame_convex", class_prob, labels, edge, cut, smoothed, records, cap_records, out, cout};
    if (!(cam && depth && p && cp && out && cout)) return seg_refuse_null(o.who);
    return segment_run(cam, depth, p, cp, device, o);
}

}  // extern "C"
