// refine.hip -- batched point-to-plane refinement of pose hypotheses on the context (stocs_refine_poses): the reference's one
// refinement step, clustering::point_to_plane_icp (src/pose_clustering.cpp:123-140: PCL ICP with normals, 5 iterations,
// 3.5 cm), applied to n centred-frame hypotheses at once and rescored by the context's LCP path.  The arithmetic is that of
// icp.hip and oracle/ingest_oracle.py::icp (nearest model point within the distance, lowest model index on equal distance,
// linearised point-to-plane least squares in double, 6x6 solve, U <- [Rz Ry Rx | t] U); PARITY WITH PCL IS UNPINNED.
//
// Direction as in the reference: the scene segment is aligned onto the model, so one correspondence structure over the model
// serves every hypothesis and every frame.  Per hypothesis k the source is s_i = U_k T_k^-1 x_i.
//   1. Model grid: uniform cells of edge h >= distance over the centred model's box (a 27-cell walk is exact), model points
//      sorted by cell (prims.h radix sort), positions in cell order as float4 with the model index in w: one load per candidate
//      feeds the distance and the tie-break.  Built at the first call, cached with its distance, rebuilt when it changes.
//   2. Accumulate: one workgroup per (hypothesis, 256-point chunk of the source); each lane one source point: own cell, then the
//      neighbours whose box is nearer than the best candidate so far (the model staged in LDS when it is small); the chosen
//      point's normal is read once, by index.  The 27 entries of A^T A | A^T b and the count in double, reduced in a fixed
//      order to one partial per workgroup (no atomics).
//   3. Solve: one wavefront per hypothesis sums its partials in chunk order and solves; U and the frozen flag live on the device,
//      so the iterations chain on the stream.  Then T' = T U^-1, its camera form, the LCP launch, one copy and ONE synchronisation.
// A hypothesis's result depends on its own T and the source alone: the chunking is fixed by the source size, so it is bitwise
// independent of the batch it shares a call with and of its position there.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "prims.h"
#include "stocs_ctx.h"

namespace stocs {

// Cap on the cells of the model grid (eight octant offsets of 4 bytes each): a distance small against the model's extent grows the cell edge
// until the box holds at most this many cells (the walk stays exact: cells only get bigger than the distance).
static const int64_t REFINE_GRID_MAX_CELLS = (int64_t)1 << 18;
static const int REFINE_CHUNK = 256;   // source points per workgroup of the accumulation
static const size_t REFINE_LDS_BYTES = 48 << 10;   // models whose positions and offsets fit are walked from LDS
static const int REFINE_OCTANT_DENSITY = 32;        // from this many model points per cell on, octants are tested one by one

struct RefHyp {
    double Tinv[12];   // row-major 3x4: centred scene -> centred model under the input hypothesis
    double U[12];      // row-major 3x4: the refinement so far (model frame)
    int32_t ncorr;     // correspondences of the last evaluated iteration
    int32_t iters;     // updates applied
    int32_t frozen;    // < 6 correspondences, a singular system or a degenerate input: no further iteration
    int32_t pad;
};

struct RefineGrid {
    float dist;   // correspondence distance it was built for (0: not built)
    float ox, oy, oz, h, inv_h;
    int nx, ny, nz;
    float lo[3], hi[3];   // model box widened by the distance: a source point outside it has no correspondence
    uint32_t* d_off;      // 8 ncells + 1 offsets into the cell-ordered positions: cell c, octant o starts at d_off[8 c + o]
    float4* d_pos;        // xyz + bits(model index)
    DevBlock mem;
};

struct RefineState {
    RefineGrid g;
    DevBlock work;   // hypotheses | T in | source indices | partials | outputs (grow-only)
    DevBlock detail; // stocs_refine_detail: match | counted | sums (grow-only)
    DevBlock robust; // refine_robust.h: rank words | model indices | select results of stocs_refine_poses_robust (grow-only)
};

__global__ __launch_bounds__(256) void refine_keys_kernel(const float4* __restrict__ mpos, int nM, float ox, float oy, float oz, float inv_h, int nx, int ny,
                                                          int nz, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nM) return;
    const float4 p = mpos[i];
    const float ux = (p.x - ox) * inv_h, uy = (p.y - oy) * inv_h, uz = (p.z - oz) * inv_h;
    const int cx = min(max((int)floorf(ux), 0), nx - 1);
    const int cy = min(max((int)floorf(uy), 0), ny - 1);
    const int cz = min(max((int)floorf(uz), 0), nz - 1);
    // octant of the cell: the half of each axis the point lies in (the walk tests the octants' boxes, refine_accumulate_kernel)
    const int oct = (ux - (float)cx >= 0.5f ? 1 : 0) | (uy - (float)cy >= 0.5f ? 2 : 0) | (uz - (float)cz >= 0.5f ? 4 : 0);
    keys[i] = (uint32_t)(((cz * ny + cy) * nx + cx) * 8 + oct);
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void refine_scatter_kernel(const float4* __restrict__ mpos, int nM, const uint32_t* __restrict__ perm, float4* __restrict__ gpos) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nM) return;
    const uint32_t i = perm[j];
    const float4 p = mpos[i];
    gpos[j] = make_float4(p.x, p.y, p.z, __int_as_float((int)i));
}

// off[c] = first slot whose key is >= c (c = 0 .. number of octants)
__global__ __launch_bounds__(256) void refine_offsets_kernel(const uint32_t* __restrict__ keys_sorted, int nM, int ncells, uint32_t* __restrict__ off) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > ncells) return;
    int lo = 0, hi = nM;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys_sorted[mid] < (uint32_t)c) lo = mid + 1; else hi = mid;
    }
    off[c] = (uint32_t)lo;
}

// general 3x4 inverse (row-major [R | t]) by the adjugate, in double; false when the linear part is singular or not finite
STOCS_HD bool inv34(const double* M, double* I) {
    const double a = M[0], b = M[1], c = M[2], d = M[4], e = M[5], f = M[6], g = M[8], h = M[9], k = M[10];
    const double A = e * k - f * h, B = f * g - d * k, C = d * h - e * g;
    const double det = a * A + b * B + c * C;
    if (!(det != 0.0) || !isfinite(det)) return false;
    const double r = 1.0 / det;
    I[0] = A * r; I[1] = (c * h - b * k) * r; I[2] = (b * f - c * e) * r;
    I[4] = B * r; I[5] = (a * k - c * g) * r; I[6] = (c * d - a * f) * r;
    I[8] = C * r; I[9] = (b * g - a * h) * r; I[10] = (a * e - b * d) * r;
    for (int i = 0; i < 3; ++i) I[i * 4 + 3] = -(I[i * 4] * M[3] + I[i * 4 + 1] * M[7] + I[i * 4 + 2] * M[11]);
    return true;
}

// Gaussian elimination with partial pivoting (first largest pivot, as icp.hip's host solve), unrolled so that the system stays in
// registers: the row swap is a select on every candidate row instead of an indexed access
STOCS_HD bool solve6(double A[6][6], double b[6], double x[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        int p = c;
        double pv = fabs(A[c][c]);
#pragma unroll
        for (int r = c + 1; r < 6; ++r) { const double v = fabs(A[r][c]); if (v > pv) { pv = v; p = r; } }
        if (pv < 1e-300) return false;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            const bool sw = r == p;
#pragma unroll
            for (int k = 0; k < 6; ++k) { const double t = A[r][k]; A[r][k] = sw ? A[c][k] : t; A[c][k] = sw ? t : A[c][k]; }
            const double t = b[r]; b[r] = sw ? b[c] : t; b[c] = sw ? t : b[c];
        }
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            const double f = A[r][c] / A[c][c];
#pragma unroll
            for (int k = c; k < 6; ++k) A[r][k] -= f * A[c][k];
            b[r] -= f * b[c];
        }
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double s = b[r];
#pragma unroll
        for (int k = r + 1; k < 6; ++k) s -= A[r][k] * x[k];
        x[r] = s / A[r][r];
    }
    return true;
}

// live != NULL: hypothesis k takes part only when live[k] (the unused slots of a trial batch's hypotheses start frozen)
__global__ __launch_bounds__(64) void refine_init_kernel(const float* __restrict__ Tin, int n, const int32_t* __restrict__ live, RefHyp* __restrict__ hyp) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float* T = Tin + (size_t)k * 16;
    double M[12];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) M[r * 4 + c] = (double)T[c * 4 + r];
    RefHyp h;
    const bool ok = inv34(M, h.Tinv);
    if (!ok) for (int i = 0; i < 12; ++i) h.Tinv[i] = 0.0;
    for (int i = 0; i < 12; ++i) h.U[i] = (i % 5 == 0) ? 1.0 : 0.0;
    h.ncorr = 0; h.iters = 0; h.frozen = ok && (!live || live[k]) ? 0 : 1; h.pad = 0;
    hyp[k] = h;
}

struct RefArgs {
    const float4* spos;   // centred scene (xyz, class probability)
    const int32_t* idx;   // source subset (NULL: every scene point)
    int nsrc, nchunks, nM, nsub;
    int octants;          // 1: test the octants of a cell before walking them (dense cells), 0: walk whole cells
    const uint32_t* off;
    const float4* gpos;   // cell order, model index in w
    const float4* mpos;   // original order: the chosen point and its normal
    const float4* mnrm;
    float ox, oy, oz, inv_h;
    int nx, ny, nz;
    float h2, margin_u;   // cell edge squared; slack of the box distances in cell units
    float lox, loy, loz, hix, hiy, hiz;
    float max_d2_f;       // the squared distance, rounded up a little: where the float search starts
    double max_d2;
};

// What stocs_refine_detail reads out of the accumulation and the summation of ONE hypothesis (arrays preset to -1 / 0 / 0: a lane
// that never reaches a store leaves them).  The shipping kernels are the RefNoDetail instantiations: an empty trailing argument, every
// `if constexpr (Detail::on)` discarded, the same instructions as without it.
struct RefNoDetail { static constexpr bool on = false; };
struct RefDetailOut {
    static constexpr bool on = true;
    int32_t* match;     // nsrc: the model index the walk chose, -1 none
    uint8_t* counted;   // nsrc: passed the double threshold test
    double* sums28;     // the 28 sums as the solve step forms them
};

// kLds: the cell-ordered model positions and the offsets are staged in LDS first (small models, REFINE_LDS_BYTES): the walk's loads
// then cost a fraction of a cache hit
template <bool kLds, class Detail>
__global__ __launch_bounds__(256) void refine_accumulate_kernel(RefArgs a, const RefHyp* __restrict__ hyp, double* __restrict__ partial, Detail det) {
    extern __shared__ float4 lds_pos[];   // kLds: nM positions, then the nsub + 1 octant offsets
    uint32_t* lds_off = (uint32_t*)(lds_pos + a.nM);
    const int hk = blockIdx.x / a.nchunks, ch = blockIdx.x - hk * a.nchunks;
    const RefHyp* H = hyp + hk;
    if (H->frozen) return;   // uniform over the workgroup; the solve never reads this hypothesis's partials again
    if (kLds) {
        for (int j = threadIdx.x; j < a.nM; j += REFINE_CHUNK) lds_pos[j] = a.gpos[j];
        for (int j = threadIdx.x; j <= a.nsub; j += REFINE_CHUNK) lds_off[j] = a.off[j];
        __syncthreads();
    }
    const int i = ch * REFINE_CHUNK + (int)threadIdx.x;
    double v[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) v[k] = 0.0;
    if (i < a.nsrc) {
        const float4 x = a.spos[a.idx ? a.idx[i] : i];
        const double* Ti = H->Tinv;
        const double* U = H->U;
        // the source cloud in the model frame, as a caller would hand it over (float), then the running estimate in double
        const float s0x = (float)(Ti[0] * x.x + Ti[1] * x.y + Ti[2] * x.z + Ti[3]);
        const float s0y = (float)(Ti[4] * x.x + Ti[5] * x.y + Ti[6] * x.z + Ti[7]);
        const float s0z = (float)(Ti[8] * x.x + Ti[9] * x.y + Ti[10] * x.z + Ti[11]);
        const double sx = U[0] * s0x + U[1] * s0y + U[2] * s0z + U[3];
        const double sy = U[4] * s0x + U[5] * s0y + U[6] * s0z + U[7];
        const double sz = U[8] * s0x + U[9] * s0y + U[10] * s0z + U[11];
        const float fx = (float)sx, fy = (float)sy, fz = (float)sz;
        if (fx >= a.lox && fx <= a.hix && fy >= a.loy && fy <= a.hiy && fz >= a.loz && fz <= a.hiz) {
            // position in cell units; a box (cell or octant) whose distance from the point, less a margin for the float rounding
            // of the assignment, exceeds the best candidate so far cannot hold a nearer (or equally near) point
            const float ux = (fx - a.ox) * a.inv_h, uy = (fy - a.oy) * a.inv_h, uz = (fz - a.oz) * a.inv_h;
            const int cx = min(max((int)floorf(ux), -1), a.nx);
            const int cy = min(max((int)floorf(uy), -1), a.ny);
            const int cz = min(max((int)floorf(uz), -1), a.nz);
            auto gap = [&](float u, float lo, float hi) { return fmaxf(fmaxf(lo - u, u - hi) - a.margin_u, 0.0f); };
            // candidates beyond the distance cannot correspond: the search starts at the threshold (the double test below decides).
            // (squared distance bits, model index) as one 64-bit key: its minimum is the nearest point, the lowest index on a tie
            // (squared distances are never negative, so their bits order as the floats do)
            uint64_t key = ((uint64_t)__float_as_uint(a.max_d2_f) << 32) | 0xFFFFFFFFull;
            // own cell first, then the 26 neighbours (the result does not depend on the visiting order); in each, the octants
            for (int tt = 0; tt < 27; ++tt) {
                const int t = tt < 14 ? 13 - tt : tt;   // 13 = (0, 0, 0)
                const int x = cx + t % 3 - 1, y = cy + (t / 3) % 3 - 1, z = cz + t / 9 - 1;
                if (x < 0 || x >= a.nx || y < 0 || y >= a.ny || z < 0 || z >= a.nz) continue;
                const float fxl = (float)x, fyl = (float)y, fzl = (float)z;
                {
                    const float gx = gap(ux, fxl, fxl + 1.0f), gy = gap(uy, fyl, fyl + 1.0f), gz = gap(uz, fzl, fzl + 1.0f);
                    if (a.h2 * ((gx * gx + gy * gy) + gz * gz) > __uint_as_float((uint32_t)(key >> 32))) continue;
                }
                const int base = ((z * a.ny + y) * a.nx + x) * 8;
                for (int o = 0; o < 8; o += a.octants ? 1 : 8) {   // sparse cells: the whole cell as one range
                    if (a.octants) {
                        const float bx = fxl + 0.5f * (float)(o & 1), by = fyl + 0.5f * (float)((o >> 1) & 1), bz = fzl + 0.5f * (float)(o >> 2);
                        const float gx = gap(ux, bx, bx + 0.5f), gy = gap(uy, by, by + 0.5f), gz = gap(uz, bz, bz + 0.5f);
                        if (a.h2 * ((gx * gx + gy * gy) + gz * gz) > __uint_as_float((uint32_t)(key >> 32))) continue;
                    }
                    const int e = base + o + (a.octants ? 1 : 8);
                    const int beg = (int)(kLds ? lds_off[base + o] : a.off[base + o]), end = (int)(kLds ? lds_off[e] : a.off[e]);
#pragma unroll 4
                    for (int j = beg; j < end; ++j) {
                        const float4 p = kLds ? lds_pos[j] : a.gpos[j];
                        const float dx = fx - p.x, dy = fy - p.y, dz = fz - p.z;
                        const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                        const uint64_t k = ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)__float_as_uint(p.w);
                        key = k < key ? k : key;
                    }
                }
            }
            if constexpr (Detail::on) det.match[i] = (int32_t)(uint32_t)key;   // the key's start value carries index -1
            if ((uint32_t)key != 0xFFFFFFFFu) {
                const uint32_t id = (uint32_t)key;
                const float4 t = a.mpos[id], nn = a.mnrm[id];
                const double ddx = sx - t.x, ddy = sy - t.y, ddz = sz - t.z;
                if (ddx * ddx + ddy * ddy + ddz * ddz <= a.max_d2) {
                    const double ar[6] = {sy * nn.z - sz * nn.y, sz * nn.x - sx * nn.z, sx * nn.y - sy * nn.x, (double)nn.x, (double)nn.y, (double)nn.z};   // [s x n, n]
                    const double b = (t.x - sx) * nn.x + (t.y - sy) * nn.y + (t.z - sz) * nn.z;
                    int k = 0;
#pragma unroll
                    for (int r = 0; r < 6; ++r)
#pragma unroll
                        for (int c = r; c < 6; ++c) v[k++] = ar[r] * ar[c];
#pragma unroll
                    for (int r = 0; r < 6; ++r) v[21 + r] = ar[r] * b;
                    v[27] = 1.0;
                    if constexpr (Detail::on) det.counted[i] = 1;
                }
            }
        }
    }
    __shared__ double red[REFINE_CHUNK / 64][28];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (__any(v[27] != 0.0)) {
        // butterfly, stage by stage over all 28 sums (28 independent exchanges in flight per stage)
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int k = 0; k < 28; ++k) v[k] += __shfl_xor(v[k], o, 64);
    }   // else: no correspondence in the wavefront, every sum is 0
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 28; ++k) red[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 28) partial[(size_t)blockIdx.x * 28 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// Detail::on: the sums go to det.sums28 and nothing else happens (no solve, the hypothesis stays as it is)
template <class Detail>
__global__ __launch_bounds__(64) void refine_solve_kernel(RefHyp* __restrict__ hyp, const double* __restrict__ partial, int nchunks, Detail det) {
    RefHyp* H = hyp + blockIdx.x;
    if (H->frozen) return;
    // lane l sums chunks l, l + 64, ... in order, then a butterfly over the wavefront: a fixed order, whatever the batch
    const double* P = partial + (size_t)blockIdx.x * nchunks * 28;
    double acc[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0.0;
    for (int ch = threadIdx.x; ch < nchunks; ch += 64)
#pragma unroll
        for (int k = 0; k < 28; ++k) acc[k] += P[(size_t)ch * 28 + k];
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int k = 0; k < 28; ++k) acc[k] += __shfl_xor(acc[k], o, 64);
    if (threadIdx.x) return;
    if constexpr (Detail::on) {
#pragma unroll
        for (int k = 0; k < 28; ++k) det.sums28[k] = acc[k];
        return;
    }
    const int ncorr = (int)acc[27];
    H->ncorr = ncorr;
    if (ncorr < 6) { H->frozen = 1; return; }   // not enough correspondences: keep the current estimate
    double A[6][6], b[6], x[6];
    int k = 0;
    for (int r = 0; r < 6; ++r) for (int c = r; c < 6; ++c) { A[r][c] = acc[k]; A[c][r] = acc[k]; k++; }
    for (int r = 0; r < 6; ++r) b[r] = acc[21 + r];
    if (!solve6(A, b, x)) { H->frozen = 1; return; }
    // update = [Rz(gamma) Ry(beta) Rx(alpha) | t], composed on the left of the running estimate
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    const double R[3][3] = {{cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa},
                            {sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa},
                            {-sb, cb * sa, cb * ca}};
    double N[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 4; ++c) N[r * 4 + c] = R[r][0] * H->U[0 * 4 + c] + R[r][1] * H->U[1 * 4 + c] + R[r][2] * H->U[2 * 4 + c];
        N[r * 4 + 3] += x[3 + r];
    }
    for (int i = 0; i < 12; ++i) H->U[i] = N[i];
    H->iters += 1;
}

// T' = T U^-1 (centred frames), its camera form (camera_from_centred: rigid_transform_kernel's tc = (c1 + cscene) - R (c2 + cmodel)
// with c1 = t', c2 = 0), the counts.  A hypothesis that was never updated comes back bit for bit.
__global__ __launch_bounds__(64) void refine_final_kernel(const float* __restrict__ Tin, const RefHyp* __restrict__ hyp, int n, V3 cscene, V3 cmodel,
                                                          float* __restrict__ Tout, float* __restrict__ Pout, int32_t* __restrict__ ncorr, int32_t* __restrict__ iters) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float* T = Tin + (size_t)k * 16;
    float* To = Tout + (size_t)k * 16;
    float* Po = Pout + (size_t)k * 16;
    const RefHyp& H = hyp[k];
    if (H.iters == 0) {
        for (int i = 0; i < 16; ++i) To[i] = T[i];
    } else {
        double Ui[12];
        inv34(H.U, Ui);   // a product of rotations: never singular
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c)
                To[c * 4 + r] = (float)((double)T[0 * 4 + r] * Ui[0 * 4 + c] + (double)T[1 * 4 + r] * Ui[1 * 4 + c] + (double)T[2 * 4 + r] * Ui[2 * 4 + c]);
            To[12 + r] = (float)((double)T[0 * 4 + r] * Ui[3] + (double)T[1 * 4 + r] * Ui[7] + (double)T[2 * 4 + r] * Ui[11] + (double)T[12 + r]);
        }
        To[3] = To[7] = To[11] = 0.0f; To[15] = 1.0f;
    }
    camera_from_centred(To, cscene, cmodel, Po);
    ncorr[k] = H.ncorr;
    iters[k] = H.iters;
}

// the model grid for correspondence distance d (stream-ordered; no synchronisation unless its memory has to grow)
static int build_refine_grid(stocs_ctx* c, RefineState* S, float d) {
    RefineGrid& g = S->g;
    const int nM = c->nM;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < nM; ++i)
        for (int k = 0; k < 3; ++k) { const float v = comp3(c->h_mpos[(size_t)i], k); mn[k] = std::min(mn[k], v); mx[k] = std::max(mx[k], v); }
    // 0.1 % over the distance: a point within d of a model point lies in a neighbouring cell despite float rounding of the cell index
    float h = d * 1.001f;
    int n3[3];
    int64_t cells = 0;
    for (;;) {
        const float inv_h = 1.0f / h;
        cells = 1;
        for (int k = 0; k < 3; ++k) { n3[k] = (int)floorf((mx[k] - mn[k]) * inv_h) + 1; cells *= n3[k]; }
        if (cells <= REFINE_GRID_MAX_CELLS) break;
        h *= 1.25f;
    }
    g.ox = mn[0]; g.oy = mn[1]; g.oz = mn[2]; g.h = h; g.inv_h = 1.0f / h;
    g.nx = n3[0]; g.ny = n3[1]; g.nz = n3[2];
    for (int k = 0; k < 3; ++k) { g.lo[k] = mn[k] - d; g.hi[k] = mx[k] + d; }
    const int64_t nsub = cells * 8;   // octants
    int bits = 1;
    while (((int64_t)1 << bits) < nsub) ++bits;
    size_t tmp_bytes = 0;
    STOCS_HIP_CHECK(sort_pairs(NULL, tmp_bytes, (const uint32_t*)NULL, (uint32_t*)NULL, (const uint32_t*)NULL, (uint32_t*)NULL, (size_t)nM, 0, (unsigned)bits, c->stream));
    // offsets | cell-ordered positions | keys, sorted keys, values, sorted values | sort scratch
    Carve cv;
    const size_t o_off = cv.take((size_t)(nsub + 1) * 4), o_pos = cv.take((size_t)nM * 16), o_keys = cv.take((size_t)nM * 4), o_keys_s = cv.take((size_t)nM * 4),
                 o_vals = cv.take((size_t)nM * 4), o_vals_s = cv.take((size_t)nM * 4), o_tmp = cv.take(tmp_bytes);
    { const int rc = g.mem.grow(c->stream, cv.total); if (rc) return rc; }
    g.d_off = Carve::at<uint32_t>(g.mem.p, o_off); g.d_pos = Carve::at<float4>(g.mem.p, o_pos);
    uint32_t* keys = Carve::at<uint32_t>(g.mem.p, o_keys); uint32_t* keys_s = Carve::at<uint32_t>(g.mem.p, o_keys_s);
    uint32_t* vals = Carve::at<uint32_t>(g.mem.p, o_vals); uint32_t* vals_s = Carve::at<uint32_t>(g.mem.p, o_vals_s);
    const unsigned mb = (unsigned)((nM + 255) / 256);
    hipLaunchKernelGGL(refine_keys_kernel, dim3(mb), dim3(256), 0, c->stream, c->d_mpos, nM, g.ox, g.oy, g.oz, g.inv_h, g.nx, g.ny, g.nz, keys, vals);
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(sort_pairs(g.mem.p + o_tmp, tmp_bytes, keys, keys_s, vals, vals_s, (size_t)nM, 0, (unsigned)bits, c->stream));
    hipLaunchKernelGGL(refine_scatter_kernel, dim3(mb), dim3(256), 0, c->stream, c->d_mpos, nM, vals_s, g.d_pos);
    STOCS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(refine_offsets_kernel, dim3((unsigned)((nsub + 1 + 255) / 256)), dim3(256), 0, c->stream, keys_s, nM, (int)nsub, g.d_off);
    STOCS_HIP_CHECK(hipGetLastError());
    g.dist = d;
    return STOCS_OK;
}

// the model grid for the distance and the grow-only workspace of n hypotheses over nsrc source points (may synchronise when either
// has to be (re)built or grown; nothing of the workspace may be in flight then)
int refine_prepare(stocs_ctx* c, int n, int nsrc, float max_correspondence_distance, RefineWork* w) {
    const int nchunks = (nsrc + REFINE_CHUNK - 1) / REFINE_CHUNK;
    if ((int64_t)n * std::max(nchunks, 1) >= ((int64_t)1 << 31)) { set_error("refinement: %d hypotheses x %d chunks: too many workgroups", n, nchunks); return STOCS_ERR_INVALID; }
    if (!c->refine) {
        c->refine = new RefineState();   // (value-initialised: no grid, no workspace)
    }
    RefineState* S = (RefineState*)c->refine;
    if (S->g.dist != max_correspondence_distance) {
        const int rc = build_refine_grid(c, S, max_correspondence_distance);
        if (rc) { S->g.dist = 0.0f; return rc; }
    }
    // device block: hypotheses | T in | source indices | partials | T out | P out | lcp | n_corr | iterations
    const size_t out_bytes = (size_t)n * (64 + 64 + 4 + 4 + 4);
    Carve cv;
    const size_t o_hyp = cv.take((size_t)n * sizeof(RefHyp)), o_Tin = cv.take((size_t)n * 64), o_idx = cv.take((size_t)std::max(nsrc, 1) * 4),
                 o_part = cv.take((size_t)n * std::max(nchunks, 1) * 28 * 8), o_out = cv.take(out_bytes);
    { const int rc = S->work.grow(c->stream, cv.total); if (rc) return rc; }
    w->d_hyp = S->work.p + o_hyp; w->d_Tin = Carve::at<float>(S->work.p, o_Tin); w->d_idx = Carve::at<int32_t>(S->work.p, o_idx);
    w->d_part = Carve::at<double>(S->work.p, o_part); w->d_Tout = Carve::at<float>(S->work.p, o_out);
    w->d_Pout = w->d_Tout + (size_t)n * 16;
    w->d_lcp = w->d_Pout + (size_t)n * 16;
    w->d_nc = (int32_t*)(w->d_lcp + n);
    w->d_it = w->d_nc + n;
    w->out_bytes = out_bytes;
    w->n = n; w->nsrc = nsrc; w->nchunks = nchunks;
    return STOCS_OK;
}

// the accumulation's arguments for the context's grid and this distance; *lds_bytes: what staging the model in LDS takes
static RefArgs refine_args(stocs_ctx* c, const RefineWork& w, bool use_idx, float max_correspondence_distance, size_t* lds_bytes) {
    RefineState* S = (RefineState*)c->refine;
    const int nchunks = w.nchunks;
    RefArgs a;
    a.spos = c->d_spos; a.idx = use_idx ? w.d_idx : NULL; a.nsrc = w.nsrc; a.nchunks = nchunks; a.nM = c->nM; a.nsub = 8 * S->g.nx * S->g.ny * S->g.nz;
    a.octants = c->nM >= REFINE_OCTANT_DENSITY * S->g.nx * S->g.ny * S->g.nz ? 1 : 0;
    a.off = S->g.d_off; a.gpos = S->g.d_pos; a.mpos = c->d_mpos; a.mnrm = c->d_mnrm;
    a.ox = S->g.ox; a.oy = S->g.oy; a.oz = S->g.oz; a.inv_h = S->g.inv_h;
    a.nx = S->g.nx; a.ny = S->g.ny; a.nz = S->g.nz;
    a.lox = S->g.lo[0]; a.loy = S->g.lo[1]; a.loz = S->g.lo[2]; a.hix = S->g.hi[0]; a.hiy = S->g.hi[1]; a.hiz = S->g.hi[2];
    a.max_d2 = (double)max_correspondence_distance * (double)max_correspondence_distance;
    a.max_d2_f = (float)(a.max_d2 * (1.0 + 1e-5));
    a.h2 = S->g.h * S->g.h;
    a.margin_u = 1e-3f + 1e-6f * (float)std::max(S->g.nx, std::max(S->g.ny, S->g.nz));
    *lds_bytes = (size_t)c->nM * 16 + ((size_t)a.nsub + 1) * 4;
    return a;
}

// init, max_iterations x (accumulate, solve), final, the LCP launch -- on the stream, no copy, no synchronisation.  Input: w.d_Tin
// (n centred T16); the source is w.d_idx[0 .. nsrc) when use_idx, else every scene point; live: see refine_init_kernel.  The LCP
// launch follows the context's scoring state (c->snrmw_override / c->lcp_cand_trial of an instance-mode batch included)
int refine_enqueue(stocs_ctx* c, const RefineWork& w, bool use_idx, const int32_t* d_live, int max_iterations, float max_correspondence_distance) {
    const int n = w.n, nchunks = w.nchunks;
    RefHyp* d_hyp = (RefHyp*)w.d_hyp;
    const unsigned hblocks = (unsigned)((n + 63) / 64);
    hipLaunchKernelGGL(refine_init_kernel, dim3(hblocks), dim3(64), 0, c->stream, (const float*)w.d_Tin, n, d_live, d_hyp);
    STOCS_HIP_CHECK(hipGetLastError());
    size_t lds_bytes = 0;
    const RefArgs a = refine_args(c, w, use_idx, max_correspondence_distance, &lds_bytes);
    for (int it = 0; it < max_iterations; ++it) {
        if (nchunks > 0) {
            if (lds_bytes <= REFINE_LDS_BYTES)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(refine_accumulate_kernel<true, RefNoDetail>), dim3((unsigned)(n * nchunks)), dim3(REFINE_CHUNK), lds_bytes, c->stream, a,
                                   (const RefHyp*)d_hyp, w.d_part, RefNoDetail());
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(refine_accumulate_kernel<false, RefNoDetail>), dim3((unsigned)(n * nchunks)), dim3(REFINE_CHUNK), 0, c->stream, a,
                                   (const RefHyp*)d_hyp, w.d_part, RefNoDetail());
            STOCS_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(refine_solve_kernel<RefNoDetail>, dim3((unsigned)n), dim3(64), 0, c->stream, d_hyp, (const double*)w.d_part, nchunks, RefNoDetail());
        STOCS_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(refine_final_kernel, dim3(hblocks), dim3(64), 0, c->stream, (const float*)w.d_Tin, (const RefHyp*)d_hyp, n, c->centroid_scene,
                       c->centroid_model, w.d_Tout, w.d_Pout, w.d_nc, w.d_it);
    STOCS_HIP_CHECK(hipGetLastError());
    return launch_lcp(c, w.d_Tout, n, w.d_lcp, NULL, NULL, NULL, 0);
}

}  // namespace stocs

using namespace stocs;

extern "C" void stocs_internal_free_refine(stocs_ctx* c) {
    if (!c || !c->refine) return;
    RefineState* S = (RefineState*)c->refine;
    S->g.mem.free(); S->work.free(); S->detail.free(); S->robust.free();
    delete S;
    c->refine = NULL;
}

extern "C" int stocs_refine_poses(stocs_ctx* c, const float* T16_in, int n, const int32_t* src_idx, int n_src, int max_iterations,
                                  float max_correspondence_distance, float* T16_out, float* pose16_out, float* lcp_out, int32_t* n_corr_out,
                                  int32_t* iterations_out) {
    if (!c) { set_error("stocs_refine_poses: NULL context"); return STOCS_ERR_INVALID; }
    if (n < 0 || n_src < 0) { set_error("stocs_refine_poses: negative size (n %d, n_src %d)", n, n_src); return STOCS_ERR_INVALID; }
    if (n > 0 && !T16_in) { set_error("stocs_refine_poses: NULL hypotheses"); return STOCS_ERR_INVALID; }
    if (max_iterations < 0) { set_error("stocs_refine_poses: max_iterations %d < 0", max_iterations); return STOCS_ERR_INVALID; }
    if (!(max_correspondence_distance > 0.0f) || !isfinite(max_correspondence_distance)) {
        set_error("stocs_refine_poses: correspondence distance %g must be positive and finite", (double)max_correspondence_distance);
        return STOCS_ERR_INVALID;
    }
    if (c->nS <= 0) { set_error("stocs_refine_poses: the context has no scene"); return STOCS_ERR_STATE; }
    if (src_idx)
        for (int i = 0; i < n_src; ++i)
            if (src_idx[i] < 0 || src_idx[i] >= c->nS) { set_error("stocs_refine_poses: src_idx[%d] = %d outside [0, %d)", i, src_idx[i], c->nS); return STOCS_ERR_INVALID; }
    if (n == 0) return STOCS_OK;
    const int nsrc = src_idx ? n_src : c->nS;
    {
        const int nchunks = (nsrc + REFINE_CHUNK - 1) / REFINE_CHUNK;
        if ((int64_t)n * std::max(nchunks, 1) >= ((int64_t)1 << 31)) { set_error("stocs_refine_poses: %d hypotheses x %d chunks: too many workgroups", n, nchunks); return STOCS_ERR_INVALID; }
    }
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    RefineWork w;
    {
        const int rc = refine_prepare(c, n, nsrc, max_correspondence_distance, &w);
        if (rc) return rc;
    }
    // inputs and outputs go through the context's pinned block (grown only when this call needs more than it has)
    const size_t out_bytes = w.out_bytes;
    const size_t in_bytes = al256((size_t)n * 64) + al256((size_t)(src_idx ? nsrc : 0) * 4);
    char* hin; char* hout;
    { const int rc = pinned_for(c, in_bytes, al256(out_bytes), &hin, &hout); if (rc) return rc; }   // in_bytes is a multiple of 256: hout = hin + in_bytes
    memcpy(hin, T16_in, (size_t)n * 64);
    if (src_idx && nsrc) memcpy(hin + al256((size_t)n * 64), src_idx, (size_t)nsrc * 4);
    STOCS_HIP_CHECK(hipMemcpyAsync(w.d_Tin, hin, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
    if (src_idx && nsrc) STOCS_HIP_CHECK(hipMemcpyAsync(w.d_idx, hin + al256((size_t)n * 64), (size_t)nsrc * 4, hipMemcpyHostToDevice, c->stream));
    {
        const int rc = refine_enqueue(c, w, src_idx != NULL, NULL, max_iterations, max_correspondence_distance);
        if (rc) return rc;
    }
    STOCS_HIP_CHECK(hipMemcpyAsync(hout, w.d_Tout, out_bytes, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    const char* o = hout;
    if (T16_out) memcpy(T16_out, o, (size_t)n * 64);
    if (pose16_out) memcpy(pose16_out, o + (size_t)n * 64, (size_t)n * 64);
    if (lcp_out) memcpy(lcp_out, o + (size_t)n * 128, (size_t)n * 4);
    if (n_corr_out) memcpy(n_corr_out, o + (size_t)n * 132, (size_t)n * 4);
    if (iterations_out) memcpy(iterations_out, o + (size_t)n * 136, (size_t)n * 4);
    return STOCS_OK;
}

extern "C" int stocs_refine_detail(stocs_ctx* c, const float* T16_in, const int32_t* src_idx, int n_src, float max_correspondence_distance, int32_t* match,
                                   uint8_t* counted, double* sums28) {
    if (!c) { set_error("stocs_refine_detail: NULL context"); return STOCS_ERR_INVALID; }
    if (n_src < 0) { set_error("stocs_refine_detail: negative size (n_src %d)", n_src); return STOCS_ERR_INVALID; }
    if (!T16_in) { set_error("stocs_refine_detail: NULL hypothesis"); return STOCS_ERR_INVALID; }
    if (!(max_correspondence_distance > 0.0f) || !isfinite(max_correspondence_distance)) {
        set_error("stocs_refine_detail: correspondence distance %g must be positive and finite", (double)max_correspondence_distance);
        return STOCS_ERR_INVALID;
    }
    if (c->nS <= 0) { set_error("stocs_refine_detail: the context has no scene"); return STOCS_ERR_STATE; }
    if (src_idx)
        for (int i = 0; i < n_src; ++i)
            if (src_idx[i] < 0 || src_idx[i] >= c->nS) { set_error("stocs_refine_detail: src_idx[%d] = %d outside [0, %d)", i, src_idx[i], c->nS); return STOCS_ERR_INVALID; }
    const int nsrc = src_idx ? n_src : c->nS;
    if (nsrc > 0 && (!match || !counted)) { set_error("stocs_refine_detail: NULL output"); return STOCS_ERR_INVALID; }
    DeviceGuard dev_guard(c->device);
    RefineWork w;
    {
        const int rc = refine_prepare(c, 1, nsrc, max_correspondence_distance, &w);
        if (rc) return rc;
    }
    RefineState* S = (RefineState*)c->refine;
    Carve cv;
    const size_t o_match = cv.take((size_t)std::max(nsrc, 1) * 4), o_cnt = cv.take((size_t)std::max(nsrc, 1)), o_sums = cv.take(28 * 8);
    { const int rc = S->detail.grow(c->stream, cv.total); if (rc) return rc; }
    int32_t* d_match = Carve::at<int32_t>(S->detail.p, o_match);
    uint8_t* d_cnt = Carve::at<uint8_t>(S->detail.p, o_cnt);
    double* d_sums = Carve::at<double>(S->detail.p, o_sums);
    // a plain, synchronous path (a test and diagnosis facility): pageable copies, one hypothesis
    STOCS_HIP_CHECK(hipMemcpyAsync(w.d_Tin, T16_in, 64, hipMemcpyHostToDevice, c->stream));
    if (src_idx && nsrc) STOCS_HIP_CHECK(hipMemcpyAsync(w.d_idx, src_idx, (size_t)nsrc * 4, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(d_match, 0xFF, (size_t)std::max(nsrc, 1) * 4, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(d_cnt, 0, (size_t)std::max(nsrc, 1), c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(d_sums, 0, 28 * 8, c->stream));   // (a frozen hypothesis is summed by nobody)
    RefDetailOut det;
    det.match = d_match; det.counted = d_cnt; det.sums28 = d_sums;
    RefHyp* d_hyp = (RefHyp*)w.d_hyp;
    hipLaunchKernelGGL(refine_init_kernel, dim3(1), dim3(64), 0, c->stream, (const float*)w.d_Tin, 1, (const int32_t*)NULL, d_hyp);
    STOCS_HIP_CHECK(hipGetLastError());
    size_t lds_bytes = 0;
    const RefArgs a = refine_args(c, w, src_idx != NULL, max_correspondence_distance, &lds_bytes);
    if (w.nchunks > 0) {
        if (lds_bytes <= REFINE_LDS_BYTES)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(refine_accumulate_kernel<true, RefDetailOut>), dim3((unsigned)w.nchunks), dim3(REFINE_CHUNK), lds_bytes, c->stream, a,
                               (const RefHyp*)d_hyp, w.d_part, det);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(refine_accumulate_kernel<false, RefDetailOut>), dim3((unsigned)w.nchunks), dim3(REFINE_CHUNK), 0, c->stream, a,
                               (const RefHyp*)d_hyp, w.d_part, det);
        STOCS_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(refine_solve_kernel<RefDetailOut>, dim3(1), dim3(64), 0, c->stream, d_hyp, (const double*)w.d_part, w.nchunks, det);
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (nsrc) {
        STOCS_HIP_CHECK(hipMemcpy(match, d_match, (size_t)nsrc * 4, hipMemcpyDeviceToHost));
        STOCS_HIP_CHECK(hipMemcpy(counted, d_cnt, (size_t)nsrc, hipMemcpyDeviceToHost));
    }
    if (sums28) STOCS_HIP_CHECK(hipMemcpy(sums28, d_sums, 28 * 8, hipMemcpyDeviceToHost));
    return STOCS_OK;
}

// the trimmed, normal-gated form (stocs_refine_poses_robust, stocs_refine_robust_detail): its own kernels on this file's state
#include "refine_robust.h"
