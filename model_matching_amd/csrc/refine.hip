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
//
// The trimmed, normal-gated form (stocs_refine_poses_robust; include/stocs_hip.h states its contract) is the same layer under other
// settings (RefineSettings, stocs_ctx.h): one device core, one iteration driver (refine_prepare, refine_enqueue) and one call frame
// serve both.  keep_ratio == 1 is step 2 as it stands, with the gate's test compiled in when the gate is on; keep_ratio < 1 replaces
// step 2 by match, select and kept (refine_robust.h), in groups of hypotheses that share the rank rows.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "solve6.h"
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

struct RefineState {   // (value-initialised: no grid, no workspace)
    static const StateOwner OWNER = OWN_REFINE;
    RefineGrid g;
    DevBlock work;   // hypotheses | T in | source indices | partials | outputs (grow-only)
    DevBlock detail; // stocs_refine_detail: match | counted | sums (grow-only)
    DevBlock robust; // refine_robust.h: rank words | model indices | select results of stocs_refine_poses_robust (grow-only)
    ~RefineState() { g.mem.free(); work.free(); detail.free(); robust.free(); }
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

// The normal gate of the accumulation, a compile-time argument like Detail: RefNoGate is empty and every `if constexpr (Gate::on)` is
// discarded (the plain form); RefGate carries what the test reads.
struct RefNoGate { static constexpr bool on = false; };
struct RefGate {
    static constexpr bool on = true;
    const float4* snrm;   // the base scene's unit normals (xyz), never an instance-mode override
    double min_cos;
};

// ---- the device core: every piece once; refine_accumulate_kernel below and the match / kept kernels of refine_robust.h are composed from them ----

// kLds: the cell-ordered model positions and the offsets are staged in LDS first (small models, REFINE_LDS_BYTES): the walk's loads
// then cost a fraction of a cache hit
template <bool kLds>
__device__ __forceinline__ void ref_stage(const RefArgs& a, float4* lds_pos, uint32_t* lds_off) {
    if (kLds) {
        for (int j = threadIdx.x; j < a.nM; j += REFINE_CHUNK) lds_pos[j] = a.gpos[j];
        for (int j = threadIdx.x; j <= a.nsub; j += REFINE_CHUNK) lds_off[j] = a.off[j];
        __syncthreads();
    }
}

// the source point in the model frame: as a caller would hand it over (float), then the running estimate in double
struct RefSource { double sx, sy, sz; float fx, fy, fz; };
__device__ __forceinline__ RefSource ref_source(const RefArgs& a, const RefHyp* H, int sidx) {
    const float4 x = a.spos[sidx];
    const double* Ti = H->Tinv;
    const double* U = H->U;
    const float s0x = (float)(Ti[0] * x.x + Ti[1] * x.y + Ti[2] * x.z + Ti[3]);
    const float s0y = (float)(Ti[4] * x.x + Ti[5] * x.y + Ti[6] * x.z + Ti[7]);
    const float s0z = (float)(Ti[8] * x.x + Ti[9] * x.y + Ti[10] * x.z + Ti[11]);
    RefSource s;
    s.sx = U[0] * s0x + U[1] * s0y + U[2] * s0z + U[3];
    s.sy = U[4] * s0x + U[5] * s0y + U[6] * s0z + U[7];
    s.sz = U[8] * s0x + U[9] * s0y + U[10] * s0z + U[11];
    s.fx = (float)s.sx; s.fy = (float)s.sy; s.fz = (float)s.sz;
    return s;
}

// The walk: (squared distance bits, model index) of the nearest model point below the search bound as one 64-bit key -- its minimum is
// the nearest point, the lowest index on a tie (squared distances are never negative, so their bits order as the floats do).  The
// start value (bound, index -1) when there is none or the point lies outside the widened box.  Candidates beyond the distance cannot
// correspond: the search starts at the threshold (ref_within's double test decides).
template <bool kLds>
__device__ __forceinline__ uint64_t ref_walk(const RefArgs& a, float fx, float fy, float fz, const float4* lds_pos, const uint32_t* lds_off) {
    uint64_t key = ((uint64_t)__float_as_uint(a.max_d2_f) << 32) | 0xFFFFFFFFull;
    if (!(fx >= a.lox && fx <= a.hix && fy >= a.loy && fy <= a.hiy && fz >= a.loz && fz <= a.hiz)) return key;
    // position in cell units; a box (cell or octant) whose distance from the point, less a margin for the float rounding of the
    // assignment, exceeds the best candidate so far cannot hold a nearer (or equally near) point
    const float ux = (fx - a.ox) * a.inv_h, uy = (fy - a.oy) * a.inv_h, uz = (fz - a.oz) * a.inv_h;
    const int cx = min(max((int)floorf(ux), -1), a.nx);
    const int cy = min(max((int)floorf(uy), -1), a.ny);
    const int cz = min(max((int)floorf(uz), -1), a.nz);
    auto gap = [&](float u, float lo, float hi) { return fmaxf(fmaxf(lo - u, u - hi) - a.margin_u, 0.0f); };
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
    return key;
}

// the candidate test of a matched pair, first part: the distance in double
__device__ __forceinline__ bool ref_within(const RefArgs& a, uint32_t id, const RefSource& s) {
    const float4 t = a.mpos[id];
    const double ddx = s.sx - t.x, ddy = s.sy - t.y, ddz = s.sz - t.z;
    return ddx * ddx + ddy * ddy + ddz * ddz <= a.max_d2;
}

// ... second part, with the gate on: c = (g.x n.x + g.y n.y) + g.z n.z >= min_cos with g = U_R (Tinv_R ns) in double, one operation at
// a time, left to right (g is not normalised)
__device__ __forceinline__ bool ref_normals_agree(const RefArgs& a, const float4* snrm, double min_cos, const RefHyp* H, uint32_t id, int sidx) {
    const float4 ns = snrm[sidx], nn = a.mnrm[id];
    const double* Ti = H->Tinv;
    const double* U = H->U;
    const double qx = Ti[0] * ns.x + Ti[1] * ns.y + Ti[2] * ns.z;
    const double qy = Ti[4] * ns.x + Ti[5] * ns.y + Ti[6] * ns.z;
    const double qz = Ti[8] * ns.x + Ti[9] * ns.y + Ti[10] * ns.z;
    const double gx = U[0] * qx + U[1] * qy + U[2] * qz;
    const double gy = U[4] * qx + U[5] * qy + U[6] * qz;
    const double gz = U[8] * qx + U[9] * qy + U[10] * qz;
    const double c = (gx * nn.x + gy * nn.y) + gz * nn.z;
    return c >= min_cos;
}

// the 28 products of one pair that counts: the 21 upper entries of a a^T row by row, a b, 1 with a = [s x n, n]; the chosen point and
// its normal are read by index
__device__ __forceinline__ void ref_products(const RefArgs& a, uint32_t id, const RefSource& s, double* v) {
    const float4 t = a.mpos[id], nn = a.mnrm[id];
    const double sx = s.sx, sy = s.sy, sz = s.sz;
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
}

// the reduction in a fixed order, no atomics: a butterfly over the wavefront, then the four waves in order -> one partial per workgroup
__device__ __forceinline__ void ref_reduce(double* v, double* __restrict__ partial) {
    __shared__ double red[REFINE_CHUNK / 64][28];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (__any(v[27] != 0.0)) {
        // stage by stage over all 28 sums (28 independent exchanges in flight per stage)
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

// One workgroup per (hypothesis, 256-point chunk of the source), each lane one source point: walk, candidate test, products, reduction.
// Every candidate counts: the plain form, and the robust one with keep_ratio == 1 (Gate: with its normal test).
template <bool kLds, class Detail, class Gate>
__global__ __launch_bounds__(256) void refine_accumulate_kernel(RefArgs a, const RefHyp* __restrict__ hyp, double* __restrict__ partial, Detail det, Gate gate) {
    extern __shared__ float4 lds_pos[];   // kLds: nM positions, then the nsub + 1 octant offsets
    uint32_t* lds_off = (uint32_t*)(lds_pos + a.nM);
    const int hk = blockIdx.x / a.nchunks, ch = blockIdx.x - hk * a.nchunks;
    const RefHyp* H = hyp + hk;
    if (H->frozen) return;   // uniform over the workgroup; the solve never reads this hypothesis's partials again
    ref_stage<kLds>(a, lds_pos, lds_off);
    const int i = ch * REFINE_CHUNK + (int)threadIdx.x;
    double v[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) v[k] = 0.0;
    if (i < a.nsrc) {
        const int sidx = a.idx ? a.idx[i] : i;
        const RefSource s = ref_source(a, H, sidx);
        const uint64_t key = ref_walk<kLds>(a, s.fx, s.fy, s.fz, lds_pos, lds_off);
        const uint32_t id = (uint32_t)key;
        if constexpr (Detail::on) det.match[i] = (int32_t)id;   // the key's start value carries index -1
        bool counts = id != 0xFFFFFFFFu && ref_within(a, id, s);
        if constexpr (Gate::on) counts = counts && ref_normals_agree(a, gate.snrm, gate.min_cos, H, id, sidx);
        if (counts) {
            ref_products(a, id, s, v);
            if constexpr (Detail::on) det.counted[i] = 1;
        }
    }
    ref_reduce(v, partial);
}

#include "refine_robust.h"   // match, select, kept: the trimmed form's kernels (inside this namespace)

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

// The group rule.  The rows take 8 bytes per (hypothesis, source point), and a batch piece's slots are an upper bound taken before the
// counts are known: n hypotheses are refined in groups of consecutive hypotheses, the largest run whose demand group x nsrc x 8 stays
// within STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES and at least one; only a source too large for ONE hypothesis is refused.
// STOCS_REFINE_ROBUST_GROUP_BYTES (read per call) lowers the limit (tests: forces several groups).  No rows: one group.
int refine_prepare(stocs_ctx* c, const char* who, int n, int nsrc, const RefineSettings& s, int flags, RefineWork* w) {
    *w = RefineWork();
    const int nchunks = (nsrc + REFINE_CHUNK - 1) / REFINE_CHUNK;
    if ((int64_t)n * std::max(nchunks, 1) >= ((int64_t)1 << 31)) { set_error("%s: %d hypotheses x %d chunks: too many workgroups", who, n, nchunks); return STOCS_ERR_INVALID; }
    if (const char* why = robust_setting_error(s.keep_ratio, s.min_normal_cos)) { set_error("%s: %s", who, why); return STOCS_ERR_INVALID; }
    const bool rows = s.keep_ratio != 1.0f || (flags & REFINE_ROWS);
    int group = std::max(n, 1);
    if (rows) {
        const uint64_t per = (uint64_t)std::max(nsrc, 1) * 8u;
        uint64_t limit = (uint64_t)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES;
        if (per > limit) {
            set_error("%s: %d source points need %llu workspace bytes for one hypothesis, the limit is %llu", who, nsrc, (unsigned long long)per, (unsigned long long)limit);
            return STOCS_ERR_INVALID;
        }
        if (const char* e = getenv("STOCS_REFINE_ROBUST_GROUP_BYTES")) { const long long v = atoll(e); if (v > 0 && (uint64_t)v < limit) limit = (uint64_t)v; }
        if (!(flags & REFINE_ONE_GROUP)) group = (int)std::min<uint64_t>(std::max<uint64_t>(limit / per, 1), (uint64_t)group);
    }
    RefineState* S = ctx_state<RefineState>(c);
    if (S->g.dist != s.distance) {
        const int rc = build_refine_grid(c, S, s.distance);
        if (rc) { S->g.dist = 0.0f; return rc; }
    }
    // device block: hypotheses | T in | source indices | partials | T out | P out | lcp | n_corr | iterations
    const size_t out_bytes = (size_t)n * (64 + 64 + 4 + 4 + 4);
    Carve cv;
    const size_t o_hyp = cv.take((size_t)n * sizeof(RefHyp)), o_Tin = cv.take((size_t)n * 64), o_idx = cv.take((size_t)std::max(nsrc, 1) * 4),
                 o_part = cv.take((size_t)n * std::max(nchunks, 1) * 28 * 8), o_out = cv.take(out_bytes);
    { const int rc = S->work.grow(c->stream, cv.total); if (rc) return rc; }
    RefineWork p;
    if (rows) {   // rank words | model indices | select results
        const size_t cells = (size_t)group * (size_t)std::max(nsrc, 1);
        Carve rv;
        const size_t o_word = rv.take(cells * 4), o_match = rv.take(cells * 4), o_sel = rv.take((size_t)group * sizeof(RobustSel));
        { const int rc = S->robust.grow(c->stream, rv.total); if (rc) return rc; }
        p.d_word = Carve::at<uint32_t>(S->robust.p, o_word); p.d_match = Carve::at<int32_t>(S->robust.p, o_match); p.d_sel = S->robust.p + o_sel;
    }
    p.d_hyp = S->work.p + o_hyp; p.d_Tin = Carve::at<float>(S->work.p, o_Tin); p.d_idx = Carve::at<int32_t>(S->work.p, o_idx);
    p.d_part = Carve::at<double>(S->work.p, o_part); p.d_Tout = Carve::at<float>(S->work.p, o_out);
    p.d_Pout = p.d_Tout + (size_t)n * 16;
    p.d_lcp = p.d_Pout + (size_t)n * 16;
    p.d_nc = (int32_t*)(p.d_lcp + n);
    p.d_it = p.d_nc + n;
    p.out_bytes = out_bytes;
    p.n = n; p.nsrc = nsrc; p.nchunks = nchunks;
    p.s = s; p.rows = rows; p.group = group;
    *w = p;
    return STOCS_OK;
}

// what the evaluation's kernels take: the walk's arguments for the context's grid and the distance, the robust ones, and what staging
// the model in LDS takes
struct RefEval { RefArgs a; RobustArgs r; size_t lds_bytes; };
static RefEval refine_eval_args(stocs_ctx* c, const RefineWork& w, bool use_idx) {
    RefineState* S = ctx_state_if<RefineState>(c);
    RefEval e;
    RefArgs& a = e.a;
    a.spos = c->d_spos; a.idx = use_idx ? w.d_idx : NULL; a.nsrc = w.nsrc; a.nchunks = w.nchunks; a.nM = c->nM; a.nsub = 8 * S->g.nx * S->g.ny * S->g.nz;
    a.octants = c->nM >= REFINE_OCTANT_DENSITY * S->g.nx * S->g.ny * S->g.nz ? 1 : 0;
    a.off = S->g.d_off; a.gpos = S->g.d_pos; a.mpos = c->d_mpos; a.mnrm = c->d_mnrm;
    a.ox = S->g.ox; a.oy = S->g.oy; a.oz = S->g.oz; a.inv_h = S->g.inv_h;
    a.nx = S->g.nx; a.ny = S->g.ny; a.nz = S->g.nz;
    a.lox = S->g.lo[0]; a.loy = S->g.lo[1]; a.loz = S->g.lo[2]; a.hix = S->g.hi[0]; a.hiy = S->g.hi[1]; a.hiz = S->g.hi[2];
    a.max_d2 = (double)w.s.distance * (double)w.s.distance;
    a.max_d2_f = (float)(a.max_d2 * (1.0 + 1e-5));
    a.h2 = S->g.h * S->g.h;
    a.margin_u = 1e-3f + 1e-6f * (float)std::max(S->g.nx, std::max(S->g.ny, S->g.nz));
    e.lds_bytes = (size_t)c->nM * 16 + ((size_t)a.nsub + 1) * 4;
    RobustArgs& r = e.r;
    r.snrm = c->d_snrmw; r.gate = w.s.min_normal_cos >= -1.0f ? 1 : 0; r.min_cos = (double)w.s.min_normal_cos;
    r.word = w.d_word; r.match = w.d_match; r.sel = (RobustSel*)w.d_sel;
    return e;
}

template <class Detail, class Gate>
static void launch_accumulate(stocs_ctx* c, const RefEval& e, dim3 grid, const RefHyp* hyp, double* part, Detail det, Gate gate) {
    if (e.lds_bytes <= REFINE_LDS_BYTES)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(refine_accumulate_kernel<true, Detail, Gate>), grid, dim3(REFINE_CHUNK), e.lds_bytes, c->stream, e.a, hyp, part, det, gate);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(refine_accumulate_kernel<false, Detail, Gate>), grid, dim3(REFINE_CHUNK), 0, c->stream, e.a, hyp, part, det, gate);
}

// One evaluation of hypotheses g0 .. g0 + gn into their partials, the launches in front of the solve.  No rows: everything that
// passes counts, ONE launch (the gate-off instantiation for the plain form and the robust one alike); rows: match, select, kept on
// rows 0 .. gn.  The detail entry points pass what they read out (acc: no rows and no gate; kept: rows), everybody else NULL.
static int refine_evaluate(stocs_ctx* c, const RefineWork& w, const RefEval& e, int g0, int gn, const RefDetailOut* acc, const RobustDetailOut* kept) {
    const RefHyp* hyp = (const RefHyp*)w.d_hyp + g0;
    double* part = w.d_part + (size_t)g0 * (size_t)w.nchunks * 28;
    const dim3 grid((unsigned)(gn * w.nchunks)), block(REFINE_CHUNK);
    if (!w.rows) {
        if (e.r.gate) launch_accumulate(c, e, grid, hyp, part, RefNoDetail(), RefGate{e.r.snrm, e.r.min_cos});
        else if (acc) launch_accumulate(c, e, grid, hyp, part, *acc, RefNoGate());
        else launch_accumulate(c, e, grid, hyp, part, RefNoDetail(), RefNoGate());
        STOCS_HIP_CHECK(hipGetLastError());
        return STOCS_OK;
    }
    if (e.lds_bytes <= REFINE_LDS_BYTES) hipLaunchKernelGGL(HIP_KERNEL_NAME(robust_match_kernel<true>), grid, block, e.lds_bytes, c->stream, e.a, e.r, hyp);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(robust_match_kernel<false>), grid, block, 0, c->stream, e.a, e.r, hyp);
    STOCS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(robust_select_kernel, dim3((unsigned)gn), dim3(256), 0, c->stream, hyp, w.nsrc, w.s.keep_ratio, (const uint32_t*)e.r.word, e.r.sel);
    STOCS_HIP_CHECK(hipGetLastError());
    if (kept) hipLaunchKernelGGL(HIP_KERNEL_NAME(robust_kept_kernel<RobustDetailOut>), grid, block, 0, c->stream, e.a, e.r, hyp, part, *kept);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(robust_kept_kernel<RobustNoDetail>), grid, block, 0, c->stream, e.a, e.r, hyp, part, RobustNoDetail());
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

static int launch_refine_init(stocs_ctx* c, const RefineWork& w, const int32_t* d_live) {
    if (!w.d_hyp || (w.rows && !w.d_word)) { set_error("refinement: the workspace was not planned (refine_prepare)"); return STOCS_ERR_STATE; }
    hipLaunchKernelGGL(refine_init_kernel, dim3((unsigned)((w.n + 63) / 64)), dim3(64), 0, c->stream, (const float*)w.d_Tin, w.n, d_live, (RefHyp*)w.d_hyp);
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

// The iteration driver (stocs_ctx.h states the contract).  A dead hypothesis starts frozen and every kernel, the select included, leaves
// at its first test.  A hypothesis's launches see its own RefHyp, partials and rows alone: the results do not depend on the grouping.
// The LCP launch follows the context's scoring state (c->snrmw_override / c->lcp_cand_trial of an instance-mode batch included).
int refine_enqueue(stocs_ctx* c, const RefineWork& w, bool use_idx, const int32_t* d_live, int* n_groups) {
    { const int rc = launch_refine_init(c, w, d_live); if (rc) return rc; }
    const int n = w.n;
    RefHyp* d_hyp = (RefHyp*)w.d_hyp;
    const RefEval e = refine_eval_args(c, w, use_idx);
    int groups = 0;
    for (int g0 = 0; g0 < n && w.s.iterations > 0; g0 += w.group, ++groups) {
        const int gn = std::min(w.group, n - g0);
        for (int it = 0; it < w.s.iterations; ++it) {
            if (w.nchunks > 0) {
                const int rc = refine_evaluate(c, w, e, g0, gn, NULL, NULL);
                if (rc) return rc;
            }
            hipLaunchKernelGGL(refine_solve_kernel<RefNoDetail>, dim3((unsigned)gn), dim3(64), 0, c->stream, d_hyp + g0,
                               (const double*)w.d_part + (size_t)g0 * (size_t)w.nchunks * 28, w.nchunks, RefNoDetail());
            STOCS_HIP_CHECK(hipGetLastError());
        }
    }
    if (n_groups) *n_groups = groups;
    hipLaunchKernelGGL(refine_final_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, (const float*)w.d_Tin, (const RefHyp*)d_hyp, n, c->centroid_scene,
                       c->centroid_model, w.d_Tout, w.d_Pout, w.d_nc, w.d_it);
    STOCS_HIP_CHECK(hipGetLastError());
    return launch_lcp(c, w.d_Tout, n, w.d_lcp, NULL, NULL, NULL, 0);
}

// the checks every entry point of this file makes, one wording each; n hypotheses at T16_in
static int refine_check_call(stocs_ctx* c, const char* who, const float* T16_in, int n, const int32_t* src_idx, int n_src, const RefineSettings& s) {
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0 || n_src < 0) { set_error("%s: negative size (n %d, n_src %d)", who, n, n_src); return STOCS_ERR_INVALID; }
    if (n > 0 && !T16_in) { set_error("%s: NULL hypotheses", who); return STOCS_ERR_INVALID; }
    if (s.iterations < 0) { set_error("%s: max_iterations %d < 0", who, s.iterations); return STOCS_ERR_INVALID; }
    if (!(s.distance > 0.0f) || !isfinite(s.distance)) { set_error("%s: correspondence distance %g must be positive and finite", who, (double)s.distance); return STOCS_ERR_INVALID; }
    if (const char* why = robust_setting_error(s.keep_ratio, s.min_normal_cos)) { set_error("%s: %s", who, why); return STOCS_ERR_INVALID; }
    if (c->nS <= 0) { set_error("%s: the context has no scene", who); return STOCS_ERR_STATE; }
    if (src_idx)
        for (int i = 0; i < n_src; ++i)
            if (src_idx[i] < 0 || src_idx[i] >= c->nS) { set_error("%s: src_idx[%d] = %d outside [0, %d)", who, i, src_idx[i], c->nS); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}

static RefineSettings refine_settings_of(const stocs_refine_robust_params* p) {
    return RefineSettings{p->max_iterations, p->max_correspondence_distance, p->keep_ratio, p->min_normal_cos};
}

// The frame of stocs_refine_poses and stocs_refine_poses_robust: checks, T16_in / src_idx through the context's pinned block (grown only
// when this call needs more than it has), the enqueue, ONE read-back and ONE synchronisation, the outputs unpacked.  robust: the demand
// n x nsrc x 8 is bounded instead of grouped, and n_cand is preset (a hypothesis that is never evaluated: 0) and read back.
static int refine_poses_call(stocs_ctx* c, const char* who, const float* T16_in, int n, const int32_t* src_idx, int n_src, const RefineSettings& s, bool robust,
                             float* T16_out, float* pose16_out, float* lcp_out, int32_t* n_corr_out, int32_t* n_cand_out, int32_t* iterations_out) {
    { const int rc = refine_check_call(c, who, T16_in, n, src_idx, n_src, s); if (rc) return rc; }
    if (n == 0) return STOCS_OK;
    const int nsrc = src_idx ? n_src : c->nS;
    if (robust && (uint64_t)n * (uint64_t)nsrc * 8u > (uint64_t)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES) {
        set_error("%s: %d hypotheses x %d source points need %llu workspace bytes, the limit is %llu", who, n, nsrc, (unsigned long long)n * (unsigned long long)nsrc * 8ull,
                  (unsigned long long)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES);
        return STOCS_ERR_INVALID;
    }
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    RefineWork w;
    { const int rc = refine_prepare(c, who, n, nsrc, s, REFINE_ONE_GROUP, &w); if (rc) return rc; }
    const size_t out_bytes = w.out_bytes, sel_bytes = w.rows ? (size_t)n * sizeof(RobustSel) : 0;
    const size_t in_bytes = al256((size_t)n * 64) + al256((size_t)(src_idx ? nsrc : 0) * 4);
    char* hin; char* hout;
    { const int rc = pinned_for(c, in_bytes, al256(out_bytes) + al256(sel_bytes), &hin, &hout); if (rc) return rc; }   // in_bytes is a multiple of 256: hout = hin + in_bytes
    memcpy(hin, T16_in, (size_t)n * 64);
    if (src_idx && nsrc) memcpy(hin + al256((size_t)n * 64), src_idx, (size_t)nsrc * 4);
    STOCS_HIP_CHECK(hipMemcpyAsync(w.d_Tin, hin, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
    if (src_idx && nsrc) STOCS_HIP_CHECK(hipMemcpyAsync(w.d_idx, hin + al256((size_t)n * 64), (size_t)nsrc * 4, hipMemcpyHostToDevice, c->stream));
    if (sel_bytes) STOCS_HIP_CHECK(hipMemsetAsync(w.d_sel, 0, sel_bytes, c->stream));
    { const int rc = refine_enqueue(c, w, src_idx != NULL, NULL, NULL); if (rc) return rc; }
    STOCS_HIP_CHECK(hipMemcpyAsync(hout, w.d_Tout, out_bytes, hipMemcpyDeviceToHost, c->stream));
    const RobustSel* hsel = (const RobustSel*)(hout + al256(out_bytes));
    if (sel_bytes) STOCS_HIP_CHECK(hipMemcpyAsync((void*)hsel, w.d_sel, sel_bytes, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    const char* o = hout;
    if (T16_out) memcpy(T16_out, o, (size_t)n * 64);
    if (pose16_out) memcpy(pose16_out, o + (size_t)n * 64, (size_t)n * 64);
    if (lcp_out) memcpy(lcp_out, o + (size_t)n * 128, (size_t)n * 4);
    if (n_corr_out) memcpy(n_corr_out, o + (size_t)n * 132, (size_t)n * 4);
    if (iterations_out) memcpy(iterations_out, o + (size_t)n * 136, (size_t)n * 4);
    if (n_cand_out) {
        if (!w.rows) memcpy(n_cand_out, o + (size_t)n * 132, (size_t)n * 4);   // everything kept: the candidates are the correspondences
        else for (int k = 0; k < n; ++k) n_cand_out[k] = hsel[k].ncand;
    }
    return STOCS_OK;
}

// The frame of stocs_refine_detail and stocs_refine_robust_detail, a plain, synchronous path (a test and diagnosis facility): ONE
// hypothesis, pageable copies, presets (what a hypothesis that is never evaluated -- a singular linear part -- reports: match -1, flag 0,
// rank all ones, sums 0), ONE evaluation, the 28 sums as the solve step forms them.  flag: counted (plain) or kept (robust: always
// match, select, kept; rank and sel are read back too).
static int refine_detail_call(stocs_ctx* c, const char* who, const float* T16_in, const int32_t* src_idx, int n_src, const RefineSettings& s, bool robust, bool have_outputs,
                              int32_t* match, uint8_t* flag, uint32_t* rank, RobustSel* sel, double* sums28) {
    { const int rc = refine_check_call(c, who, T16_in, 1, src_idx, n_src, s); if (rc) return rc; }
    const int nsrc = src_idx ? n_src : c->nS;
    if (nsrc > 0 && !have_outputs) { set_error("%s: NULL output", who); return STOCS_ERR_INVALID; }
    DeviceGuard dev_guard(c->device);
    RefineWork w;
    { const int rc = refine_prepare(c, who, 1, nsrc, s, robust ? REFINE_ONE_GROUP | REFINE_ROWS : REFINE_ONE_GROUP, &w); if (rc) return rc; }
    RefineState* S = ctx_state_if<RefineState>(c);
    const size_t cells = (size_t)std::max(nsrc, 1);
    Carve cv;
    const size_t o_match = cv.take(cells * 4), o_flag = cv.take(cells), o_sums = cv.take(28 * 8);
    { const int rc = S->detail.grow(c->stream, cv.total); if (rc) return rc; }
    RefDetailOut det;
    det.match = Carve::at<int32_t>(S->detail.p, o_match); det.counted = Carve::at<uint8_t>(S->detail.p, o_flag); det.sums28 = Carve::at<double>(S->detail.p, o_sums);
    RobustDetailOut kept;
    kept.kept = det.counted;
    STOCS_HIP_CHECK(hipMemcpyAsync(w.d_Tin, T16_in, 64, hipMemcpyHostToDevice, c->stream));
    if (src_idx && nsrc) STOCS_HIP_CHECK(hipMemcpyAsync(w.d_idx, src_idx, (size_t)nsrc * 4, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(det.match, 0xFF, cells * 4, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(det.counted, 0, cells, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(det.sums28, 0, 28 * 8, c->stream));   // (a frozen hypothesis is summed by nobody)
    if (w.rows) {
        STOCS_HIP_CHECK(hipMemsetAsync(w.d_word, 0xFF, cells * 4, c->stream));
        STOCS_HIP_CHECK(hipMemsetAsync(w.d_sel, 0, sizeof(RobustSel), c->stream));
    }
    { const int rc = launch_refine_init(c, w, NULL); if (rc) return rc; }
    RefEval e = refine_eval_args(c, w, src_idx != NULL);
    e.r.match = det.match;   // the match kernel's model indices go where the accumulation's would
    if (w.nchunks > 0) {
        const int rc = refine_evaluate(c, w, e, 0, 1, &det, &kept);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(refine_solve_kernel<RefDetailOut>, dim3(1), dim3(64), 0, c->stream, (RefHyp*)w.d_hyp, (const double*)w.d_part, w.nchunks, det);
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (nsrc) {
        STOCS_HIP_CHECK(hipMemcpy(match, det.match, (size_t)nsrc * 4, hipMemcpyDeviceToHost));
        STOCS_HIP_CHECK(hipMemcpy(flag, det.counted, (size_t)nsrc, hipMemcpyDeviceToHost));
        if (w.rows) STOCS_HIP_CHECK(hipMemcpy(rank, w.d_word, (size_t)nsrc * 4, hipMemcpyDeviceToHost));
    }
    if (w.rows) STOCS_HIP_CHECK(hipMemcpy(sel, w.d_sel, sizeof(RobustSel), hipMemcpyDeviceToHost));
    if (sums28) STOCS_HIP_CHECK(hipMemcpy(sums28, det.sums28, 28 * 8, hipMemcpyDeviceToHost));
    return STOCS_OK;
}

}  // namespace stocs

using namespace stocs;

extern "C" int stocs_refine_poses(stocs_ctx* c, const float* T16_in, int n, const int32_t* src_idx, int n_src, int max_iterations,
                                  float max_correspondence_distance, float* T16_out, float* pose16_out, float* lcp_out, int32_t* n_corr_out,
                                  int32_t* iterations_out) {
    return refine_poses_call(c, "stocs_refine_poses", T16_in, n, src_idx, n_src, refine_plain(max_iterations, max_correspondence_distance), false, T16_out, pose16_out,
                             lcp_out, n_corr_out, NULL, iterations_out);
}

extern "C" int stocs_refine_poses_robust(stocs_ctx* c, const float* T16_in, int n, const int32_t* src_idx, int n_src, const stocs_refine_robust_params* p,
                                         float* T16_out, float* pose16_out, float* lcp_out, int32_t* n_corr_out, int32_t* n_cand_out, int32_t* iterations_out) {
    const char* who = "stocs_refine_poses_robust";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (!p) { set_error("%s: NULL params", who); return STOCS_ERR_INVALID; }
    return refine_poses_call(c, who, T16_in, n, src_idx, n_src, refine_settings_of(p), true, T16_out, pose16_out, lcp_out, n_corr_out, n_cand_out, iterations_out);
}

extern "C" int stocs_refine_detail(stocs_ctx* c, const float* T16_in, const int32_t* src_idx, int n_src, float max_correspondence_distance, int32_t* match,
                                   uint8_t* counted, double* sums28) {
    return refine_detail_call(c, "stocs_refine_detail", T16_in, src_idx, n_src, refine_plain(0, max_correspondence_distance), false, match && counted, match, counted, NULL,
                              NULL, sums28);
}

extern "C" int stocs_refine_robust_detail(stocs_ctx* c, const float* T16_in, const int32_t* src_idx, int n_src, const stocs_refine_robust_params* p, int32_t* match,
                                          uint8_t* candidate, uint8_t* kept, uint32_t* rank, int32_t* k_out, int32_t* n_cand_out, double* sums28) {
    const char* who = "stocs_refine_robust_detail";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (!p) { set_error("%s: NULL params", who); return STOCS_ERR_INVALID; }
    RobustSel sel;
    const int rc = refine_detail_call(c, who, T16_in, src_idx, n_src, refine_settings_of(p), true, match && candidate && kept && rank, match, kept, rank, &sel, sums28);
    if (rc) return rc;
    const int nsrc = src_idx ? n_src : c->nS;
    for (int i = 0; i < nsrc; ++i) candidate[i] = rank[i] != 0xFFFFFFFFu ? 1 : 0;   // by definition of the rank word
    if (k_out) *k_out = sel.k;
    if (n_cand_out) *n_cand_out = sel.ncand;
    return STOCS_OK;
}

extern "C" int stocs_refine_robust_workspace(stocs_ctx* c, void** address, uint64_t* bytes) {
    if (!c) { set_error("stocs_refine_robust_workspace: NULL context"); return STOCS_ERR_INVALID; }
    RefineState* S = ctx_state_if<RefineState>(c);
    if (address) *address = S ? (void*)S->robust.p : NULL;
    if (bytes) *bytes = S ? (uint64_t)S->robust.bytes : 0;
    return STOCS_OK;
}
