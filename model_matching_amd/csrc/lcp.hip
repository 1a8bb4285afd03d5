// lcp.hip -- batched weighted-LCP verification, THE METRIC KERNEL ("candidate poses verified / s").
// Replaces stocs_estimator::compute_alignment_score_for_rigid_transform (reference
// src/stocs.cpp:1006-1041) and the kd-tree query it calls per model point
// (reference include/super4pcs/accelerators/kdtree.h:394-459).
//
// Mapping: one candidate transform per workgroup of four wavefronts, which take the candidate's 64-point steps in turn and
// add their integer partial sums through LDS at the end (the only barrier); small models run one wavefront per candidate.
// Several candidates per workgroup, and a model tile shared through LDS, were measured and lost.
// The 3x4 transform is wave-uniform (scalar loads -> SGPRs).  A lane takes one patch-ordered model
// point per step: coalesced 16-byte loads, and the 64 queries of one step fall into a handful
// of neighbouring grid cells, so the cell/list gathers of a wave share cache lines.
// Per query: transform the point, locate its cell (one word of the flat cell table, or top -> brick -> cell word), scan that cell's
// candidate list (every scene point within epsilon of the cell box) for the nearest point with
// d^2 <= epsilon^2, then the 30-degree normal test as an exact threshold on the dot product, and an
// integer (2^32 fixed-point) sum of the class-probability weights.  No atomics on the sums: results are run-to-run
// deterministic and do not depend on the batch or on how the points are split over wavefronts.  (The one atomic of the walk, an
// LDS add per window of the split forms' shared list of live sub-patches, decides the ORDER in which a candidate's sub-patches
// are walked and by which wavefront -- not deterministic -- and nothing else: integer sums do not depend on that order.)
// The queue-fed kernel (lcp_coopq_kernel, the automatic choice) first rules out the 16-point sub-patches whose bounding
// sphere is out of reach of the scene (patch test, one look-up in a distance field of the scene) and walks the live ones
// four to a step -- the four wavefronts of a candidate from one list in LDS, step s to wavefront s & 3 --, collects the
// queries that survive the sub-cell mask in a per-wave LDS ring and verifies them 16 at a time, four lanes per query
// with two entries of a 128-byte list line each.
//
// Kernels: lcp_coopq_kernel (eight named switches, the table of its legal forms above it), lcp_coop_kernel (the per-step scan of dense
// scenes, a cross-check), lcp_kernel (a lane per query, a cross-check) and lcp_exact_kernel (exact_ties).  choose_lcp_form picks one,
// launch_lcp_form is the only place that names their instantiations.  The forms that lost their A/B runs are listed in
// DESIGN_HISTORY.md with the last commit that holds their code; a measurement build (make tools) adds the ablation bits only.
//
// Roofline: HBM-read model, algorithmic bytes 68 + 52*|M| per pose.
#include <stdlib.h>
#include <string.h>

#include <cstring>


#include <algorithm>
#include <utility>

#include "kdtree.h"
#include "normal_cone.h"
#include "octant_lists.h"
#include "patch_normals.h"
#include "prims.h"
#include "stocs_ctx.h"

namespace stocs {

struct LcpArgs {
    const float4* mpos;   // centred model positions in patch order (ctx.hip), NaN-padded to whole 64-point steps + one; w: the bits of the
                          // packed model normal (normal_cone.h), read by the gated queue forms and the gate count only
    const float4* mnrm;
    const int32_t* mperm; // sorted slot -> original model index (detail output only)
    int M;
    const int32_t* top;
    const uint4* cells;
    const uint4* flat;    // cell words addressed by (cz*ny + cy)*nx + cx, or NULL (brick look-up through top / cells)
    const float4* list;
    const float4* snrmw;  // scene unit normal + class-probability weight
    // instance-mode trial batches (stocs_run_trials): candidate i belongs to trial cand_trial[i] of the batch and adds the class
    // probabilities as ITS trial's sampling decayed them (Q8): that trial's copy lies cand_trial[i] * snrmw_stride bytes behind snrmw
    const int32_t* cand_trial;   // NULL: every candidate scores against snrmw itself
    size_t snrmw_stride;
    const float* chunk_r; // per 8-entry chunk: lower bound of |entry - cell centre| (dense scenes), else NULL
    float ox, oy, oz, inv_h, inv_h4, h;
    int nx, ny, nz, nbx, nby;
    float sq_eps, dot_lo, eps;
    float bound_margin;     // slack of the early-exit / nearest-point bound tests of the centre-sorted lists: relative to epsilon and to the
                            // scene's coordinate magnitude (the float rounding of |query - cell centre| scales with the coordinates)
    int has_nearest;        // the z word of a dense grid's cell is a lower bound of |cell centre - nearest listed point| (SceneGrid::has_nearest)
    const int32_t* order;   // processing slot -> candidate (NULL: identity): candidates that land in the same part of the scene run together
    int xcd_blocks;         // != 0: workgroups of one XCD take a contiguous run of slots (each XCD has its own L2)
    unsigned long long* best;   // != NULL: compute_best_transform in the kernel's epilogue -- every candidate's packed (score, ~id) key joins an
    uint32_t id_offset;         // atomic max on this word (integer max: order independent), id = id_offset + candidate
    // > 0: the shared-list forms also test the sub-patches' normal cones (patch_normals.h) against the cone field, whose reach this is;
    // 0: off (the option, no field, not yet filled).  The records need no pointers of their own: the sub-patch cones lie behind the
    // spheres (sub + 4 * steps), the field's cones behind the distances (dist + cells).  The word fills the gap in front of the next
    // pointer, so the record keeps its size and every other member its place: no other kernel's argument loads move
    float nreach;
    // patch test (lcp_coopq_kernel): bounding sphere per 64-point step + the scene's distance field (SceneGrid::d_dist); patch == NULL: off
    const float4* patch;
    const float4* sub;    // bounding sphere per 16-point sub-patch (ctx.hip), the unit of that test in the CU = 16 kernels
    const float* dist;
    float gox, goy, goz, g, inv_g, cap;
    int gnx, gny, gnz;
#ifdef STOCS_TOOLS_BUILD
    int ablate;             // measurement build only (STOCS_LCP_ABLATE): parts of the kernel switched off to price them; scores are then wrong
#endif
};
#ifdef STOCS_TOOLS_BUILD
#define STOCS_ABLATE(a, bit) (((a).ablate & (bit)) != 0)
#else
#define STOCS_ABLATE(a, bit) false
#endif

// workgroup -> first processing slot.  The hardware hands consecutive workgroups to the 8 XCDs round-robin; with
// xcd_blocks the workgroups that land on one XCD take consecutive slot blocks, so an XCD's L2 sees one
// contiguous part of the (spatially ordered) candidate list.  Then slot -> candidate through the order array.
__device__ __forceinline__ int lcp_candidate(const LcpArgs& a, int n, int w, int wpb = 4) {
    int blk = blockIdx.x;
    if (a.xcd_blocks == 1) {
        const int nb = gridDim.x, per = nb >> 3, rem = nb & 7, xcd = blk & 7;
        blk = xcd * per + (xcd < rem ? xcd : rem) + (blk >> 3);
    } else if (a.xcd_blocks > 1) {   // chunks of xcd_blocks consecutive blocks per XCD, chunks dealt round-robin (balanced)
        const int C = a.xcd_blocks, nb = gridDim.x, full = (nb / (8 * C)) * (8 * C);
        if (blk < full) {
            const int xcd = blk & 7, j = blk >> 3;
            blk = ((j / C) * 8 + xcd) * C + (j % C);
        }
    }
    const int slot = __builtin_amdgcn_readfirstlane(blk * wpb + w);
    if (slot >= n) return -1;
    return a.order ? __builtin_amdgcn_readfirstlane(a.order[slot]) : slot;
}


// the scene normals + weights candidate `cand` scores against (wave-uniform: scalar loads)
__device__ __forceinline__ const float4* lcp_weights_of(const LcpArgs& a, int cand) {
    if (!a.cand_trial) return a.snrmw;
    const int t = __builtin_amdgcn_readfirstlane(a.cand_trial[cand < 0 ? 0 : cand]);
    return (const float4*)((const char*)a.snrmw + (size_t)t * a.snrmw_stride);
}

#define DPP_QUAD_XOR1 0xB1   /* quad_perm [1,0,3,2] */
#define DPP_QUAD_XOR2 0x4E   /* quad_perm [2,3,0,1] */
#define DPP_HALF_MIRROR 0x141 /* lane k <-> 7-k inside each group of 8 */

// Score accumulation.  The reference adds class probabilities in a sequential float loop (stocs.cpp:1033); a parallel
// kernel cannot keep that order, so the weights are added as 2^32 fixed-point integers instead: exact for every weight
// >= 2^-9 (class probabilities are >= the 0.10 threshold), hence independent of the order -- of the lane a point lands on,
// of how a candidate's model points are split over wavefronts, of the batch it is scored in.  The score is the correctly
// rounded float of the exact mean; the reference's running float sum differs from it by ~1e-7 (tests: <= 1e-5).
__device__ __forceinline__ unsigned long long lcp_addend(float w) {
    return w > 0.0f ? (unsigned long long)(w * 4294967296.0f) : 0ull;   // exact product (power of two), truncating conversion
}
__device__ __forceinline__ void lcp_add(unsigned long long& acc, float w) {
    if (w > 0.0f) acc += (unsigned long long)(w * 4294967296.0f);   // exact product (power of two), truncating conversion
}
__device__ __forceinline__ unsigned long long lcp_wave_sum(unsigned long long acc) {
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    return acc;
}
__device__ __forceinline__ float lcp_finish(unsigned long long total, int M) {
    return (float)((double)total * (1.0 / 4294967296.0) / (double)M);
}
// the candidate's score, and -- when the caller wants the arg-max with it -- its key of compute_best_transform (stocs.cpp:987-998:
// larger score wins, lower id wins ties, scores that are not positive never win): one atomic per candidate, no second kernel
__device__ __forceinline__ void lcp_store(const LcpArgs& a, float* __restrict__ out, int cand, unsigned long long total) {
    const float s = lcp_finish(total, a.M);
    out[cand] = s;
    if (a.best && s > 0.0f)
        atomicMax(a.best, best_key(s, a.id_offset + (uint32_t)cand));
}

// candidate update: inclusive radius (kdtree.h:424), ties -> larger scene index.  When a list is stored in
// ascending index order (IDX: every grid except the dense, centre-sorted one) `<=` implements the tie rule.
template <bool IDX>
__device__ __forceinline__ void take_if_better(float d, int ei, float& gd, int& gi) {
    if (IDX) { if (d <= gd) { gd = d; gi = ei; } }
    else { if (d < gd || (d == gd && ei > gi)) { gd = d; gi = ei; } }
}

template <bool DETAIL, bool IDX = true>
__global__ __launch_bounds__(256) void lcp_kernel(LcpArgs a, const float* __restrict__ T16, float* __restrict__ out,
                                                  int n, int32_t* __restrict__ hit_out, uint8_t* __restrict__ cnt_out) {
    const int lane = threadIdx.x & 63;
    const int cand = lcp_candidate(a, n, threadIdx.x >> 6);
    if (cand < 0) return;
    const float* T = T16 + (size_t)cand * 16;
    const float4* __restrict__ snrmw = lcp_weights_of(a, cand);
    const float t0 = T[0], t1 = T[1], t2 = T[2], t4 = T[4], t5 = T[5], t6 = T[6], t8 = T[8], t9 = T[9], t10 = T[10],
                t12 = T[12], t13 = T[13], t14 = T[14];
    unsigned long long acc = 0ull;
    for (int i = lane; i < a.M; i += 64) {
        const float4 p = a.mpos[i];
        // (mat * p.homogeneous()).head<3>()
        const float qx = ((t0 * p.x + t4 * p.y) + t8 * p.z) + t12;
        const float qy = ((t1 * p.x + t5 * p.y) + t9 * p.z) + t13;
        const float qz = ((t2 * p.x + t6 * p.y) + t10 * p.z) + t14;
        const float fx = floorf((qx - a.ox) * a.inv_h);
        const float fy = floorf((qy - a.oy) * a.inv_h);
        const float fz = floorf((qz - a.oz) * a.inv_h);
        int best = -1;
        if (fx >= 0.0f && fy >= 0.0f && fz >= 0.0f && fx < (float)a.nx && fy < (float)a.ny && fz < (float)a.nz) {
            const int cx = (int)fx, cy = (int)fy, cz = (int)fz;
            const int brick = a.top[((cz >> 3) * a.nby + (cy >> 3)) * a.nbx + (cx >> 3)];
            if (brick >= 0) {
                const uint4 cw = a.cells[(size_t)brick * 512 + (((cz & 7) << 6) | ((cy & 7) << 3) | (cx & 7))];
                float bd = a.sq_eps;
                const uint32_t cn = cw.y & STOCS_CONE_COUNT_MASK;   // (the bits above hold the cell's normal cone: normal_cone.h)
                for (uint32_t k = 0; k < cn; ++k) {
                    const float4 s = a.list[cw.x + k];
                    const float dx = qx - s.x, dy = qy - s.y, dz = qz - s.z;
                    const float d = dx * dx + (dy * dy + dz * dz);
                    take_if_better<IDX>(d, __float_as_int(s.w), bd, best);
                }
            }
        }
        bool counted = false;
        if (best >= 0) {
            const float4 nm = a.mnrm[i];
            // mat.block<3,3>(0,0) * normal
            const float nx = t0 * nm.x + (t4 * nm.y + t8 * nm.z);
            const float ny = t1 * nm.x + (t5 * nm.y + t9 * nm.z);
            const float nz = t2 * nm.x + (t6 * nm.y + t10 * nm.z);
            const float4 sn = snrmw[best];
            const float d = sn.x * nx + (sn.y * ny + sn.z * nz);
            // acos(d)*180/pi < 30 as an exact threshold; d > 1 -> NaN angle -> not counted (Q7)
            counted = (d >= a.dot_lo) && (d <= 1.0f);
            if (counted) lcp_add(acc, sn.w);
        }
        if (DETAIL) {
            const int orig = a.mperm[i];
            hit_out[(size_t)cand * a.M + orig] = best;
            cnt_out[(size_t)cand * a.M + orig] = counted ? 1 : 0;
        }
    }
    // fixed-shape butterfly: deterministic
    acc = lcp_wave_sum(acc);
    if (lane == 0) lcp_store(a, out, cand, acc);
}

// ---------------------------------------------------------------------------------------------
// Per-step cooperative scan of dense scenes (lcp_variant 31): the independent cross-check of the queue kernel's dense form.
// What the ISA of lcp_kernel shows (profiles/r01_lcp_analysis.md): its list loop issues ~18 instructions per trip for the ~18 of
// 64 lanes that own a list, i.e. about one issued wave-instruction per list entry, and every entry is its own 16-byte gather.
// Here the hit queries of a step are compacted through LDS and each 8-lane group takes ONE query: the group streams the query's
// 8-padded list two 128-byte lines per trip (all 64 lanes useful), keeps its running best in registers across lines, and reduces
// once per query with DPP (pure VALU; __shfl/ds_bpermute would go through the LDS pipeline).  The lists are sorted by distance
// from the cell centre, with a lower bound of that distance per line: a query stops at the first line that the triangle
// inequality rules out.  Tie rule identical to lcp_kernel: smallest d^2, then largest scene index; same lane -> point assignment
// and reduction tree, so scores are bitwise equal to it.
// SPLIT: four wavefronts share one candidate (see lcp_coopq_kernel); else one wavefront per candidate -- one per workgroup when
// scoring, four candidates per 256-thread workgroup in the detail form.
// ---------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

// minimum of a squared distance over the GL lanes of a query group.  Squared distances are non-negative and never NaN here
// (a NaN distance fails `d <= best` and is never kept), so their bit patterns order like unsigned integers: an integer
// minimum needs no NaN canonicalisation and takes its DPP operand directly -- 3 instructions instead of 10.
template <int GL>
__device__ __forceinline__ float group_min_nonneg(float v) {
    uint32_t u = __float_as_uint(v);
    if (GL >= 2) u = min(u, (uint32_t)__builtin_amdgcn_update_dpp((int)u, (int)u, DPP_QUAD_XOR1, 0xF, 0xF, false));
    if (GL >= 4) u = min(u, (uint32_t)__builtin_amdgcn_update_dpp((int)u, (int)u, DPP_QUAD_XOR2, 0xF, 0xF, false));
    if (GL == 8) u = min(u, (uint32_t)__builtin_amdgcn_update_dpp((int)u, (int)u, DPP_HALF_MIRROR, 0xF, 0xF, false));
    return __uint_as_float(u);
}

// wavefronts per workgroup of the cooperative kernels: the four that share a candidate (SPLIT); four candidates side by side in
// the detail form; else a workgroup is one wavefront
constexpr int lcp_waves_per_block(bool detail, bool split) { return (split || detail) ? 4 : 1; }

template <bool DETAIL, bool SPLIT>
__global__ __launch_bounds__(64 * lcp_waves_per_block(DETAIL, SPLIT)) void lcp_coop_kernel(LcpArgs a, const float* __restrict__ T16, float* __restrict__ out,
                                                       int n, int32_t* __restrict__ hit_out, uint8_t* __restrict__ cnt_out) {
    static_assert(!(DETAIL && SPLIT), "the detail form is not split");
    constexpr int WPB = lcp_waves_per_block(DETAIL, SPLIT);
    constexpr int UNR = 2;             // list lines per trip
    __shared__ float4 qt[WPB][64];     // per lane: qx, qy, qz, bits(list offset)
    __shared__ uint32_t qn[WPB][64];   // per lane: list length
    __shared__ uint32_t hl[WPB][64];   // compacted hit list: r-th hit lane
    __shared__ float rd[WPB][64];      // per lane: best d^2
    __shared__ int ri[WPB][64];        // per lane: best scene index
    __shared__ float qd[WPB][64];      // per lane: |query - cell centre|
    __shared__ unsigned long long part[WPB];
    const int lane = threadIdx.x & 63;
    const int sub = lane & 7, grp = lane >> 3;
    const int w = threadIdx.x >> 6;
    // SPLIT: the WPB wavefronts of the workgroup share one candidate and take its 64-point steps round-robin (see lcp_coopq_kernel)
    const int cand = SPLIT ? lcp_candidate(a, n, 0, 1) : lcp_candidate(a, n, w, WPB);
    if (cand < 0) return;
    const int first = SPLIT ? 64 * w : 0, stride = SPLIT ? 64 * WPB : 64;
    const float4* __restrict__ snrmw = lcp_weights_of(a, cand);
    const float* T = T16 + (size_t)cand * 16;
    const float t0 = T[0], t1 = T[1], t2 = T[2], t4 = T[4], t5 = T[5], t6 = T[6], t8 = T[8], t9 = T[9], t10 = T[10],
                t12 = T[12], t13 = T[13], t14 = T[14];
    unsigned long long acc = 0ull;
    for (int base = first; base < a.M; base += stride) {
        const int i = base + lane;
        float qx = 0.f, qy = 0.f, qz = 0.f, qcd = 0.f;
        uint32_t off = 0, cnt = 0;
        if (i < a.M) {
            const float4 p = a.mpos[i];
            qx = ((t0 * p.x + t4 * p.y) + t8 * p.z) + t12;
            qy = ((t1 * p.x + t5 * p.y) + t9 * p.z) + t13;
            qz = ((t2 * p.x + t6 * p.y) + t10 * p.z) + t14;
            const float ux = (qx - a.ox) * a.inv_h, uy = (qy - a.oy) * a.inv_h, uz = (qz - a.oz) * a.inv_h;
            const float fx = floorf(ux), fy = floorf(uy), fz = floorf(uz);
            if (fx >= 0.0f && fy >= 0.0f && fz >= 0.0f && fx < (float)a.nx && fy < (float)a.ny && fz < (float)a.nz) {
                const int cx = (int)fx, cy = (int)fy, cz = (int)fz;
                const int brick = STOCS_ABLATE(a, 1) ? -1 : a.top[((cz >> 3) * a.nby + (cy >> 3)) * a.nbx + (cx >> 3)];   // 1: no look-ups at all
                if (brick >= 0) {
                    uint4 cw = make_uint4(0u, 0u, 0u, 0u);
                    if (!STOCS_ABLATE(a, 128)) cw = a.cells[(size_t)brick * 512 + (((cz & 7) << 6) | ((cy & 7) << 3) | (cx & 7))];   // 128: top table only
                    // sub-cell filter: no scene point within epsilon of this 1/4-cell => no neighbour possible
                    const int sb = ((int)((uz - fz) * 4.0f) << 4) | ((int)((uy - fy) * 4.0f) << 2) | (int)((ux - fx) * 4.0f);
                    const uint32_t mw = a.has_nearest ? 0xFFFFFFFFu : (sb < 32 ? cw.z : cw.w);   // (has_nearest: no mask on this grid, z holds a distance)
                    off = cw.x; cnt = ((mw >> (sb & 31)) & 1u) ? (cw.y & STOCS_CONE_COUNT_MASK) : 0u;
                    if (STOCS_ABLATE(a, 2)) cnt = cw.x == 0xFFFFFFF1u ? 1u : 0u;   // 2: look-ups done, nobody survives
                    const float ex = qx - (a.ox + ((float)cx + 0.5f) * a.h), ey = qy - (a.oy + ((float)cy + 0.5f) * a.h),
                                ez = qz - (a.oz + ((float)cz + 0.5f) * a.h);
                    qcd = sqrtf(ex * ex + (ey * ey + ez * ez));
                }
            }
        }
        const bool hit = cnt != 0;
        const unsigned long long mask = __ballot(hit);
        int best = -1;
        if (mask) {
            const int nh = __popcll(mask);
            if (hit) {
                const int rank = __popcll(mask & ((1ull << lane) - 1ull));
                hl[w][rank] = (uint32_t)lane;
                qt[w][lane] = make_float4(qx, qy, qz, __int_as_float((int)off));
                qn[w][lane] = cnt;
                qd[w][lane] = qcd;
            }
            __builtin_amdgcn_wave_barrier();
            for (int s = 0; s < nh; s += 8) {
                const int slot = s + grp;
                const bool gact = slot < nh;
                const uint32_t L = gact ? hl[w][slot] : 0u;
                const float4 qq = qt[w][L];
                const uint32_t c = gact ? qn[w][L] : 0u;
                const float4* lp = a.list + (uint32_t)__float_as_int(qq.w) + sub;
                float gd = a.sq_eps;
                int gi = -1;
                // lists are sorted by distance from the cell centre: stop at the first chunk that the
                // triangle inequality rules out (|q - p| >= |p - c| - |q - c| > sqrt(best) for all later p)
                const float qcg = qd[w][L];
                const uint32_t chunk0 = (uint32_t)__float_as_int(qq.w) >> 3;
                uint32_t nchunks = (c + 7u) >> 3;
                float gb = a.sq_eps;   // best d^2 of the whole group so far
                if (STOCS_ABLATE(a, 4)) nchunks = min(nchunks, (uint32_t)UNR);   // 4: the first trip of every list only
                for (uint32_t j = 0; __any(j < nchunks); j += UNR) {
                    if (j < nchunks && j > 0 && (STOCS_ABLATE(a, 256) ? 0.0f : a.chunk_r[chunk0 + j]) - qcg > sqrtf(gb) + a.bound_margin) nchunks = 0;   // 256: no chunk bounds (scan everything)
                    float4 e[UNR];
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        e[u] = make_float4(1e30f, 1e30f, 1e30f, __int_as_float(-1));
                        if (j + u < nchunks) e[u] = lp[(j + u) << 3];   // whole 128-byte line per group; tail entries are sentinels
                    }
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const float dx = qq.x - e[u].x, dy = qq.y - e[u].y, dz = qq.z - e[u].z;
                        const float d = dx * dx + (dy * dy + dz * dz);
                        const int ei = __float_as_int(e[u].w);
                        if (d < gd || (d == gd && ei > gi)) { gd = d; gi = ei; }   // the lists are not in index order
                    }
                    gb = fminf(gd, dpp_f32<DPP_QUAD_XOR1>(gd));
                    gb = fminf(gb, dpp_f32<DPP_QUAD_XOR2>(gb));
                    gb = fminf(gb, dpp_f32<DPP_HALF_MIRROR>(gb));
                }
                // group minimum of d^2 (DPP), then the largest index among the lanes that hold it
                float dm = fminf(gd, dpp_f32<DPP_QUAD_XOR1>(gd));
                dm = fminf(dm, dpp_f32<DPP_QUAD_XOR2>(dm));
                dm = fminf(dm, dpp_f32<DPP_HALF_MIRROR>(dm));
                int im = (gd == dm) ? gi : -1;
                im = max(im, dpp_i32<DPP_QUAD_XOR1>(im));
                im = max(im, dpp_i32<DPP_QUAD_XOR2>(im));
                im = max(im, dpp_i32<DPP_HALF_MIRROR>(im));
                if (gact && sub == 0) { rd[w][L] = dm; ri[w][L] = im; }
            }
            __builtin_amdgcn_wave_barrier();
            if (hit) best = ri[w][lane];
            __builtin_amdgcn_wave_barrier();
        }
        bool counted = false;
        if (best >= 0 && STOCS_ABLATE(a, 8)) lcp_add(acc, 0.5f);   // 8: no normal test
        else if (best >= 0) {
            const float4 nm = a.mnrm[i];
            const float nx = t0 * nm.x + (t4 * nm.y + t8 * nm.z);
            const float ny = t1 * nm.x + (t5 * nm.y + t9 * nm.z);
            const float nz = t2 * nm.x + (t6 * nm.y + t10 * nm.z);
            const float4 sn = snrmw[best];
            const float d = sn.x * nx + (sn.y * ny + sn.z * nz);
            counted = (d >= a.dot_lo) && (d <= 1.0f);
            if (counted) lcp_add(acc, sn.w);
        }
        if (DETAIL && i < a.M) {
            const int orig = a.mperm[i];
            hit_out[(size_t)cand * a.M + orig] = best;
            cnt_out[(size_t)cand * a.M + orig] = counted ? 1 : 0;
        }
    }
    acc = lcp_wave_sum(acc);
    if (SPLIT) {
        if (lane == 0) part[w] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long total = 0;
#pragma unroll
            for (int k = 0; k < WPB; ++k) total += part[k];
            lcp_store(a, out, cand, total);
        }
    } else if (lane == 0) lcp_store(a, out, cand, acc);
}

// ---------------------------------------------------------------------------------------------
// Patch test.  The 64 model points of a step lie in a sphere (centre c, radius r; ctx.hip).  Under the candidate transform
// x -> A x + t every one of them lands within s * r of A c + t, s >= the largest singular value of A (1 for a rigid
// transform; bounded by linear_norm_bound, stocs_math.h: the square root of the largest absolute row sum of A^T A, so that a caller's non-rigid matrix
// is handled too).  The scene's distance field gives a lower bound of the distance from A c + t to the nearest scene point;
// when that exceeds s * r + epsilon no point of the step has a scene point within epsilon, the step adds nothing to the
// score (stocs.cpp:1019-1024) and is skipped: one look-up per step instead of 64.  Margins cover the float rounding of the
// transform, of the field and of the cell centre; positions that are not finite are never ruled out here.
// ---------------------------------------------------------------------------------------------
//
// The test comes in two halves with the field look-up between them, and neither half branches around a load: the whole 16-byte record
// is used whatever the centre is (a record whose radius word is wanted only behind the magnitude test arrives as a 12-byte load and
// a dependent 4-byte one), and a centre that is not finite or lies outside the table looks up cell 0, whose value it does not use.  A
// caller with two records can so have both record loads, then both look-ups, in flight together.
struct LcpPatchProbe {
    float cx, cy, cz, fx, fy, fz;
    uint32_t cell;   // of a.dist; 0 when !inside
    bool inside;     // finite, and one cell inside the border: the float cell of a position next to the box never names a cell outside the table
};
__device__ __forceinline__ LcpPatchProbe lcp_patch_probe(const LcpArgs& a, const float4 sp, float t0, float t1, float t2, float t4, float t5, float t6,
                                                         float t8, float t9, float t10, float t12, float t13, float t14) {
    LcpPatchProbe p;
    p.cx = ((t0 * sp.x + t4 * sp.y) + t8 * sp.z) + t12;
    p.cy = ((t1 * sp.x + t5 * sp.y) + t9 * sp.z) + t13;
    p.cz = ((t2 * sp.x + t6 * sp.y) + t10 * sp.z) + t14;
    const float mag = fabsf(p.cx) + (fabsf(p.cy) + fabsf(p.cz));
    const float ux = (p.cx - a.gox) * a.inv_g, uy = (p.cy - a.goy) * a.inv_g, uz = (p.cz - a.goz) * a.inv_g;
    p.fx = floorf(ux); p.fy = floorf(uy); p.fz = floorf(uz);
    p.inside = (mag < 1.0e18f) && p.fx >= 1.0f && p.fy >= 1.0f && p.fz >= 1.0f && p.fx < (float)(a.gnx - 1) && p.fy < (float)(a.gny - 1) && p.fz < (float)(a.gnz - 1);
    p.cell = p.inside ? ((uint32_t)(int)p.fz * (uint32_t)a.gny + (uint32_t)(int)p.fy) * (uint32_t)a.gnx + (uint32_t)(int)p.fx : 0u;   // <= 16 M cells
    return p;
}
// v = a.dist[p.cell]
__device__ __forceinline__ bool lcp_patch_verdict(const LcpArgs& a, const LcpPatchProbe& p, float radius, float sn, float v) {
    const float mag = fabsf(p.cx) + (fabsf(p.cy) + fabsf(p.cz));
    const float need = (sn * radius + a.eps * 1.002f) + (4.0e-6f + 4.0e-6f * mag);
    const float ex = p.cx - (a.gox + (p.fx + 0.5f) * a.g), ey = p.cy - (a.goy + (p.fy + 0.5f) * a.g), ez = p.cz - (a.goz + (p.fz + 0.5f) * a.g);
    // outside (or in the border cells of) the table: at least cap from every scene point
    const float room = p.inside ? v - sqrtf(ex * ex + (ey * ey + ez * ez)) : a.cap;
    return (mag < 1.0e18f) && room > need;
}
// The normal-cone half of the test for a sub-patch the sphere test leaves alive (patch_normals.h): rec = the sub-patch's cone, cw = the
// cone of the probe's cell.  The cell's reach must hold every scene point the sub-patch can be counted with: the sphere test's `need`
// plus the distance of the centre from the cell's centre, against a.nreach.  Outside the table, in its border, for a centre that is not
// finite: no test (cell 0 was read, its word is not used)
__device__ __forceinline__ bool lcp_patch_normals_dead(const LcpArgs& a, const LcpPatchProbe& p, float radius, float sn, const float4 rec, uint32_t cw,
                                                       float t0, float t1, float t2, float t4, float t5, float t6, float t8, float t9, float t10) {
    const float mag = fabsf(p.cx) + (fabsf(p.cy) + fabsf(p.cz));
    const float need = (sn * radius + a.eps * 1.002f) + (4.0e-6f + 4.0e-6f * mag);
    const float ex = p.cx - (a.gox + (p.fx + 0.5f) * a.g), ey = p.cy - (a.goy + (p.fy + 0.5f) * a.g), ez = p.cz - (a.goz + (p.fz + 0.5f) * a.g);
    const bool within = p.inside && need + sqrtf(ex * ex + (ey * ey + ez * ez)) < a.nreach;
    return within && pn_rules_out(cw, rec.x, rec.y, rec.z, rec.w, sn, t0, t1, t2, t4, t5, t6, t8, t9, t10, a.dot_lo);
}
static_assert(STOCS_PN_MAX_MODEL == 16 * 512, "the cone field is built for the models the shared-list forms score (LCP_SHARED_LIVE)");

// the test in one piece, branching: for the forms that have no registers to spare for the halves (the ring and whole-step forms of the
// queue kernel: up to 28 bytes of scratch with them)
__device__ __forceinline__ bool lcp_patch_dead(const LcpArgs& a, const float4 sp, float sn, float t0, float t1, float t2, float t4, float t5, float t6,
                                               float t8, float t9, float t10, float t12, float t13, float t14) {
    const float cx = ((t0 * sp.x + t4 * sp.y) + t8 * sp.z) + t12;
    const float cy = ((t1 * sp.x + t5 * sp.y) + t9 * sp.z) + t13;
    const float cz = ((t2 * sp.x + t6 * sp.y) + t10 * sp.z) + t14;
    const float mag = fabsf(cx) + (fabsf(cy) + fabsf(cz));
    if (!(mag < 1.0e18f)) return false;
    const float need = (sn * sp.w + a.eps * 1.002f) + (4.0e-6f + 4.0e-6f * mag);
    const float ux = (cx - a.gox) * a.inv_g, uy = (cy - a.goy) * a.inv_g, uz = (cz - a.goz) * a.inv_g;
    const float fx = floorf(ux), fy = floorf(uy), fz = floorf(uz);
    // one cell inside the border: the float cell of a position next to the box never names a cell outside the table
    if (fx >= 1.0f && fy >= 1.0f && fz >= 1.0f && fx < (float)(a.gnx - 1) && fy < (float)(a.gny - 1) && fz < (float)(a.gnz - 1)) {
        const float v = a.dist[((uint32_t)(int)fz * (uint32_t)a.gny + (uint32_t)(int)fy) * (uint32_t)a.gnx + (uint32_t)(int)fx];   // <= 16 M cells
        const float ex = cx - (a.gox + (fx + 0.5f) * a.g), ey = cy - (a.goy + (fy + 0.5f) * a.g), ez = cz - (a.goz + (fz + 0.5f) * a.g);
        return v - sqrtf(ex * ex + (ey * ey + ez * ez)) > need;
    }
    // outside (or in the border cells of) the table: at least cap from every scene point
    return a.cap > need;
}

// ---------------------------------------------------------------------------------------------
// Queue-fed cooperative scan (lcp_variant 24 on sparse scenes, 39 on dense ones; the automatic choice): the cooperative scan of
// lcp_coop_kernel fed from a per-wave LDS ring that collects the hit queries of successive steps (ballot + mbcnt compaction), so
// that every lane group always owns a query (with ~11 hits per 64-point step the groups of the per-step scan are ~69 % busy) and
// the normal test runs on full wavefronts.  Lane <-> point assignment of the accumulation differs from lcp_kernel, the sums are
// integers: the scores are the same bit for bit, and run-to-run deterministic.
//
// The switches:
//   DETAIL  write hit_out / cnt_out (per-point results for the parity tests).  Changes what is written, not how it is computed --
//           but for the workgroup shape: four candidates per 256-thread workgroup, not split, brick look-ups.
//   DENSE   dense scenes: lists sorted by distance from the cell centre (not by index), a lower bound of that distance per
//           8-entry line; a query stops at the first line the triangle inequality rules out, as in lcp_coop_kernel -- but fed from
//           the queue, so that the first lines of 16 queries are in flight together.  Else index-ordered lists, walked to the end.
//   SPLIT   the four wavefronts of a workgroup share ONE candidate and take its 64-point steps round-robin (a trial's ~8 000
//           candidates are a single round of wavefronts on the chip, and four times as many, four times shorter wavefronts finish
//           it sooner; big batches lose nothing); the partial sums are integers, so the score is the same bit for bit.
//           Else one wavefront per candidate.
//   FLAT    the cell word comes from the flat cell table (one look-up) instead of top -> brick -> cell.
//   NEAR    pruned lists on grids finer than epsilon (has_nearest): the cell word's z is a lower bound of |cell centre - nearest
//           listed point| (no sub-cell mask there); a query farther from the centre than that bound + epsilon never touches the
//           list -- DENSE's first test without its line-by-line exit, which lists of ~5 entries have no use for.
//   CU      (lcp_cull_unit) points per bounding sphere of the patch test: 64, whole steps; 16, sub-patches, the live ones packed
//           four to a step.
//   SHARED  (with SPLIT and CU = 16, models of up to 8 192 points) the four wavefronts of a candidate fill and walk ONE list of live
//           sub-patches (LCP_SHARED_LIVE entries, the memory of the four rings), step s of it to wavefront s & 3.  Else a ring per
//           wavefront: larger models, whose sub-patches the list does not hold, and every form that is not split.  Chosen on the
//           host by the model size alone, so that a larger model runs exactly the code it ran before the list existed.
//
//   GATE    (scoring forms on sparse lists: DETAIL = 0, DENSE = 0; a grid with normal cones, lcp_normal_gate) a query whose cell's cone of
//           scene normals cannot pass the normal test against the rotated model normal never joins the queue (normal_cone.h).  The
//           detail forms keep every query: hit_out names the neighbour also when it is not counted.  Not for the split ring forms of
//           CU = 16 (models beyond 8 192 points): they have 62-63 VGPRs without the gate and spill 12 to 20 bytes with it, wherever
//           the model normal is requested -- three of the four still spill with the packed normal of the position's fourth word.
//
// The legal forms (45 instantiations; SHARED = 0 and GATE = 0 unless stated; the static_assert rejects every other):
//   scoring, sparse   DENSE = 0, SPLIT in {0, 1}, FLAT in {0, 1}, NEAR in {0, 1}, CU in {16, 64}         16 forms
//   scoring, dense    DENSE = 1, SPLIT = 1, FLAT = 0, NEAR = 0, CU in {16, 64}                            2 forms
//   shared list       every scoring form with SPLIT = 1 and CU = 16 once more with SHARED = 1            5 forms
//                     (the dense queue form is always split, whatever lcp_split and the model size say)
//   gated             every sparse scoring form but the split ring forms of CU = 16, once more with GATE = 1   16 forms
//   detail, sparse    DENSE = 0, SPLIT = 0, FLAT = 0, NEAR in {0, 1}, CU in {16, 64}                      4 forms
//   detail, dense     DENSE = 1, SPLIT = 0, FLAT = 0, NEAR = 0, CU in {16, 64}                            2 forms
// ---------------------------------------------------------------------------------------------
// entries of the workgroup-wide list of live sub-patches (SPLIT, CU = 16): the sub-patches of a model of up to 8 192 points
constexpr int LCP_SHARED_LIVE = 512;

constexpr bool lcp_queue_form_legal(bool detail, bool dense, bool split, bool flat, bool near, int cu, bool shared, bool gate) {
    return !(gate && (detail || dense || (split && cu == 16 && !shared))) && (cu == 16 || cu == 64) && (!shared || (split && cu == 16)) && (detail ? (!split && !flat && !(dense && near)) : (!dense || (split && !flat && !near)));
}

template <bool DETAIL, bool DENSE, bool SPLIT, bool FLAT, bool NEAR, int CU, bool SHARED, bool GATE>
__global__ __launch_bounds__(64 * lcp_waves_per_block(DETAIL, SPLIT), 8) void lcp_coopq_kernel(LcpArgs a, const float* __restrict__ T16, float* __restrict__ out,
                                                        int n, int32_t* __restrict__ hit_out, uint8_t* __restrict__ cnt_out) {
    static_assert(lcp_queue_form_legal(DETAIL, DENSE, SPLIT, FLAT, NEAR, CU, SHARED, GATE), "not one of the forms in the table above");
    constexpr int WPB = lcp_waves_per_block(DETAIL, SPLIT);
    constexpr bool IDX = !DENSE;     // index-ordered lists: `<=` implements the tie rule (take_if_better)
    constexpr bool EARLY = DENSE;    // centre-sorted lists: line-by-line exit
    // GL lanes verify one query together: each reads EPL entries of a 128-byte list line, NG queries per trip.  Four lanes with two
    // entries each and one trip in flight: Cm 1.34 -> 1.18 ms against eight lanes with one entry each and four trips in flight
    // (profiles/r03_lcp_patch_and_group_ab.json); two lanes 1.45 ms, a lane per query 3.16 ms
    constexpr int GL = 4, EPL = 8 / GL, NG = 64 / GL;
    // FIRST: list lines requested in a query's first trip (the second line of a list that has one arrives with the first: half of
    // the survivors' lists at Cm are longer than a line; one line: +2 % at 65 536 candidates, +7 % at 8 192; three: +3 %); not with
    // EARLY, whose later lines wait for the bound test -- early exit decides line by line
    constexpr int FIRST = DENSE ? 1 : 2, E0 = EPL * FIRST;
    // NOSENT: no sentinel entries, no predicated list loads -- a group without a query reads list line 0 (its result is never
    // stored), a list shorter than the trip reads its last line again: the same entries, the same winner (predicated loads and
    // sentinels: +1.2 %, +2.4 % at 8 192 candidates).  Not with EARLY, which skips the lines it rules out instead of reading them
    constexpr bool NOSENT = !DENSE;
    constexpr int UNR = 1;           // list lines per trip after the first (two: +3 %)
    constexpr int PIPE = 1;          // trips in flight (two: 1.18 -> 1.185 ms at Cm; three and four spill)
    // CHAIN: fewer dependent memory round trips per wavefront -- whole-record loads, both windows of the patch test in flight together,
    // a sorted record per query in place of three dependent LDS reads in front of every verify trip (Cm 0.805 -> 0.785 ms, 8 192
    // candidates 0.1328 -> 0.1269; profiles/lcp_chain_ab.json, _isa.md).  For the shared-list forms, which have 5 to 13 VGPRs to spare;
    // the others sit at 55 to 64, two of the gated ones spill 8 bytes with the whole-record normal test alone, and every one keeps
    // exactly the code it had
    constexpr bool CHAIN = SHARED;
    static_assert(!EARLY || (FIRST == 1 && !NOSENT), "early exit decides line by line");
    __shared__ float4 qt[WPB][128];     // qx, qy, qz, bits(list offset)
    __shared__ float qcd[EARLY ? WPB : 1][EARLY ? 128 : 1];   // |query - cell centre| (EARLY)
    __shared__ uint32_t qn[WPB][128];   // list length
    __shared__ uint32_t qs[WPB][128];   // model slot (patch order)
    __shared__ int ri[WPB][128];        // best scene index
    __shared__ uint8_t ord[WPB][64];    // batch order sorted by list length (!CHAIN)
    __shared__ uint2 srec[CHAIN ? WPB : 1][CHAIN ? 64 : 1];   // CHAIN: the batch sorted by list length: (list offset, list length | ring slot << 16)
    __shared__ unsigned long long part[WPB];
    const int lane = threadIdx.x & 63;
    // (the wavefront index stays in a VGPR: forced into an SGPR the kernel is 12 % slower, profiles/r04_lcp_w_uniform_isa.md)
    const int w = threadIdx.x >> 6;
    const int cand = SPLIT ? lcp_candidate(a, n, 0, 1) : lcp_candidate(a, n, w, WPB);
    if (cand < 0) return;   // SPLIT: the whole workgroup leaves together
    const float4* __restrict__ snrmw = lcp_weights_of(a, cand);
    // SHARED: the sphere records of this wavefront's two windows of the patch test (below) do not depend on the candidate: both are
    // requested here, back to back and ahead of the wait for the transform.  The lanes of a window that reach beyond the model read the
    // last record (a clamped index, no branch around the load); their result is discarded.  (A shared-list form runs only with the test on -- CU = 16 is chosen by a.patch,
    // choose_lcp_form -- so a.sub is there)
    const bool patch_on = SHARED && !STOCS_ABLATE(a, 64);
    // The second window of a wavefront lies wholly beyond the model for models of up to 64 * (4 + w) sub-patches (three of the eight
    // windows at 313 sub-patches): its loads and its tests are skipped, on a wave-uniform branch.  With a.nreach > 0 (wave-uniform) the
    // sub-patches' normal cones are requested with the spheres: they lie behind them (patch_normals.h)
    const bool two = SHARED && __builtin_amdgcn_readfirstlane((int)(((threadIdx.x >> 6) + 4) << 6)) < ((a.M + 15) >> 4);
    const bool pn_on = SHARED && a.nreach > 0.0f;
    float4 wsp[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    float4 wsn[2] = {make_float4(0.f, 0.f, 0.f, STOCS_PN_NO_TEST), make_float4(0.f, 0.f, 0.f, STOCS_PN_NO_TEST)};
    if (SHARED) {
        const int last_sub = max(((a.M + 15) >> 4) - 1, 0);
        const float4* const subn = a.sub + (((a.M + 63) >> 6) << 2);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j == 0 || two) {
                const int q = min((int)(((threadIdx.x >> 6) + 4 * j) << 6) + lane, last_sub);
                wsp[j] = a.sub[q];
                if (pn_on) wsn[j] = subn[q];
            }
        }
    }
    const float* T = T16 + (size_t)cand * 16;
    const float t0 = T[0], t1 = T[1], t2 = T[2], t4 = T[4], t5 = T[5], t6 = T[6], t8 = T[8], t9 = T[9], t10 = T[10],
                t12 = T[12], t13 = T[13], t14 = T[14];
    unsigned long long acc = 0ull;
    int head = 0, tail = 0;
    // GATE: the norm bound of the linear part (the patch test's too) and, from it, the ONE wave-uniform threshold of the gate on the
    // packed model normals (normal_cone.h: 511 (dot_lo - s K), rounded downwards; NaN or -inf for a matrix that is not finite)
    const float gnorm = GATE ? linear_norm_bound(t0, t1, t2, t4, t5, t6, t8, t9, t10) : 0.0f;
    const float gthr = GATE ? model_normal_gate_threshold(a.dot_lo, gnorm) : 0.0f;

    auto process = [&](int nq) {
        // order the pending queries by list length (number of 128-byte lines) so that the groups of a trip stream lists of
        // similar length: a counting sort with ballots (without it, two trips in flight: Cm 1.185 -> 1.24 ms).  Most lists are one or two lines:
        // three classes -- one trip, two, more -- do it at a third of the instructions of a sort over all lengths
        {
            uint32_t cls = 4;   // no query
            uint2 rec = make_uint2(0u, 0u);
            if (lane < nq) {
                const int idx = (head + lane) & 127;
                const uint32_t len = qn[w][idx];
                const uint32_t nch = (len + 7u) >> 3;
                cls = nch <= (uint32_t)FIRST ? 1u : (nch <= (uint32_t)(FIRST + UNR) ? 2u : 3u);
                if (CHAIN) rec = make_uint2((uint32_t)__float_as_int(qt[w][idx].w), len | ((uint32_t)idx << 16));   // (len <= STOCS_CONE_COUNT_MASK: 16 bits)
            }
            const unsigned long long below = (1ull << lane) - 1ull;
            const unsigned long long m1 = __ballot(cls == 1u), m2 = __ballot(cls == 2u), m3 = __ballot(cls == 3u);
            const int n1 = __popcll(m1), n2 = __popcll(m2);
            const int pos = cls == 1u ? __popcll(m1 & below) : (cls == 2u ? n1 + __popcll(m2 & below) : n1 + n2 + __popcll(m3 & below));
            if (CHAIN) { if (lane < nq) srec[w][pos] = rec; }
            else if (lane < nq) ord[w][pos] = (uint8_t)lane;
            __builtin_amdgcn_wave_barrier();
        }
        // a trip: NG queries, GL lanes each.  The first FIRST lines of the lists of PIPE trips are requested back to back, then
        // compared: one memory round trip serves most of the queries
        // CHAIN: a trip finds offset, length and ring slot of its query in ONE record at a static address, not behind the chain
        // order -> length -> offset of three dependent LDS reads; and the record of the next trip is requested behind this trip's list
        // loads, so that it arrives under them (the last trip reads its own again; records behind the call's queries are stale and
        // replaced below).  Two VGPRs: all four records ahead of the first trip cost eight, and the gated forms then reach 64 and one spills
        static_assert(!CHAIN || PIPE == 1, "one record per trip");
        uint2 rec_next = make_uint2(0u, 0u);
        if (CHAIN) rec_next = srec[w][lane / GL];
        for (int s0 = 0; s0 < nq; s0 += NG * PIPE) {
            const int sub = lane & (GL - 1), grp = lane / GL;
            // a group without a query takes the ring slot of the call's first one, with no entries: the later lines of a trip are read by
            // every group through the offset that sits in that slot (a stale record may name a slot that was never written)
            const uint2 rec = s0 + grp < nq ? rec_next : make_uint2(0u, (uint32_t)(head & 127) << 16);
            float4 e0[PIPE][E0];
            bool wide[PIPE];
            int idxs[PIPE];
            uint32_t cs[PIPE];
#pragma unroll
            for (int u = 0; u < PIPE; ++u) {
                const int slot = s0 + NG * u + grp;
                const bool gact = slot < nq;
                idxs[u] = CHAIN ? (int)((rec.y >> 16) & 127u) : (head + (int)ord[w][gact ? slot : 0]) & 127;
                cs[u] = gact ? (CHAIN ? (rec.y & 0xFFFFu) : qn[w][idxs[u]]) : 0u;
                wide[u] = true;
                if (!NOSENT) {
#pragma unroll
                    for (int e = 0; e < E0; ++e) e0[u][e] = make_float4(1e30f, 1e30f, 1e30f, __int_as_float(-1));
                }
                if (STOCS_ABLATE(a, 4)) {   // 4: no list loads (every survivor "hits" scene point 0 at distance 0)
                    if (cs[u]) { const float4 qq0 = qt[w][idxs[u]]; e0[u][0] = make_float4(qq0.x, qq0.y, qq0.z, __int_as_float(0)); }
                    cs[u] = cs[u] ? 1u : 0u;
                }
                else if (NOSENT) {
                    // no sentinels, no predication: a group without a query reads list line 0 (its result is never stored), a list
                    // shorter than the trip reads its last line again -- the same entries, the same winner
                    const float4* l0 = a.list + (cs[u] ? (CHAIN ? rec.x : (uint32_t)__float_as_int(qt[w][idxs[u]].w)) : 0u) + sub;
                    const uint32_t last = cs[u] ? ((cs[u] - 1u) & ~7u) : 0u;
#pragma unroll
                    for (int e = 0; e < EPL; ++e) e0[u][e] = l0[GL * e];
                    // the later lines of the first trip only when some list of this trip has them (the queries are ordered by list
                    // length, so a third of the trips are single-line lists throughout: no addresses spent on re-reading those)
                    wide[u] = FIRST > 1 && __any(cs[u] > 8u);
                    if (wide[u]) {
#pragma unroll
                        for (int e = EPL; e < E0; ++e) e0[u][e] = l0[min((uint32_t)(8 * (e / EPL)), last) + GL * (e % EPL)];
                    }
                }
                else if (cs[u]) {
                    const float4* l0 = a.list + (CHAIN ? rec.x : (uint32_t)__float_as_int(qt[w][idxs[u]].w)) + sub;
#pragma unroll
                    for (int e = 0; e < E0; ++e) e0[u][e] = l0[GL * e];   // (E0 = EPL: one line)
                }
            }
            if (CHAIN) rec_next = srec[w][min(s0 + NG * PIPE, 64 - NG * PIPE) + grp];
#pragma unroll
            for (int u = 0; u < PIPE; ++u) {
                const float4 qq = qt[w][idxs[u]];
                const uint32_t c = cs[u];
                const float4* lp = a.list + (uint32_t)__float_as_int(qq.w) + sub;
                const uint32_t last_line = c ? ((c - 1u) & ~7u) : 0u;
                float gd = a.sq_eps;
                int gi = -1;
#pragma unroll
                for (int e = 0; e < EPL; ++e) {   // ascending entries: `<=` keeps the larger index on ties (IDX lists)
                    const float dx = qq.x - e0[u][e].x, dy = qq.y - e0[u][e].y, dz = qq.z - e0[u][e].z;
                    const float d = dx * dx + (dy * dy + dz * dz);
                    take_if_better<IDX>(d, __float_as_int(e0[u][e].w), gd, gi);
                }
                if (FIRST > 1 && wide[u]) {
#pragma unroll
                    for (int e = EPL; e < E0; ++e) {
                        const float dx = qq.x - e0[u][e].x, dy = qq.y - e0[u][e].y, dz = qq.z - e0[u][e].z;
                        const float d = dx * dx + (dy * dy + dz * dz);
                        take_if_better<IDX>(d, __float_as_int(e0[u][e].w), gd, gi);
                    }
                }
                if (EARLY) {
                    const float qcg = qcd[w][idxs[u]];
                    const uint32_t chunk0 = (uint32_t)__float_as_int(qq.w) >> 3;
                    uint32_t cc = c;   // entries still to be looked at (0 once the rest of the list is ruled out)
                    for (uint32_t k = 8; __any(k < cc); k += 8 * UNR) {
                        // |q - p| >= |p - centre| - |q - centre| > sqrt(best of the group) for every later p: stop
                        if (k < cc && a.chunk_r[chunk0 + (k >> 3)] - qcg > sqrtf(group_min_nonneg<GL>(gd)) + a.bound_margin) cc = 0;
                        float4 e[EPL];
                        if (k < cc) {   // a line's entries under ONE condition: its loads leave together
#pragma unroll
                            for (int x = 0; x < EPL; ++x) e[x] = lp[k + GL * x];
                        } else {
#pragma unroll
                            for (int x = 0; x < EPL; ++x) e[x] = make_float4(1e30f, 1e30f, 1e30f, __int_as_float(-1));
                        }
#pragma unroll
                        for (int x = 0; x < EPL; ++x) {
                            const float dx = qq.x - e[x].x, dy = qq.y - e[x].y, dz = qq.z - e[x].z;
                            const float d = dx * dx + (dy * dy + dz * dz);
                            take_if_better<IDX>(d, __float_as_int(e[x].w), gd, gi);
                        }
                    }
                } else {
                    for (uint32_t k = 8 * FIRST; __any(k < c); k += 8 * UNR) {
                        const uint32_t kk = min(k, last_line);   // a list shorter than this trip reads its last line again (the same entries: harmless)
                        float4 e[EPL];
#pragma unroll
                        for (int x = 0; x < EPL; ++x) e[x] = lp[kk + GL * x];
#pragma unroll
                        for (int x = 0; x < EPL; ++x) {
                            const float dx = qq.x - e[x].x, dy = qq.y - e[x].y, dz = qq.z - e[x].z;
                            const float d = dx * dx + (dy * dy + dz * dz);
                            take_if_better<IDX>(d, __float_as_int(e[x].w), gd, gi);
                        }
                    }
                }
                const float dm = group_min_nonneg<GL>(gd);
                int im = (gd == dm) ? gi : -1;
                im = max(im, dpp_i32<DPP_QUAD_XOR1>(im));
                im = max(im, dpp_i32<DPP_QUAD_XOR2>(im));
                if (c && sub == 0) ri[w][idxs[u]] = im;
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < nq) {
            const int idx = (head + lane) & 127;
            const int best = ri[w][idx];
            const uint32_t slot_i = qs[w][idx];
            bool counted = false;
            if (best >= 0 && STOCS_ABLATE(a, 8)) { lcp_add(acc, 0.5f); }   // 8: no normal test
            else if (best >= 0) {
                const float4 nm = STOCS_ABLATE(a, 16) ? make_float4(0.f, 0.f, 1.f, 0.f) : a.mnrm[slot_i];   // 16: no model-normal gather
                const float nx = t0 * nm.x + (t4 * nm.y + t8 * nm.z);
                const float ny = t1 * nm.x + (t5 * nm.y + t9 * nm.z);
                const float nz = t2 * nm.x + (t6 * nm.y + t10 * nm.z);
                const float4 sn = STOCS_ABLATE(a, 32) ? make_float4(nx, ny, nz, 0.5f) : snrmw[best];         // 32: no scene-normal gather
                // the addend is formed from the record's fourth word ahead of the test and selected behind it: all four words are used
                // whatever the test says, so the record arrives as ONE 16-byte load (a weight wanted only by the counted lanes arrives as a
                // dependent 4-byte load behind a 12-byte one)
                const unsigned long long add = CHAIN ? lcp_addend(sn.w) : 0ull;
                const float d = sn.x * nx + (sn.y * ny + sn.z * nz);
                counted = (d >= a.dot_lo) && (d <= 1.0f);
                if (CHAIN) acc += counted ? add : 0ull;
                else if (counted) lcp_add(acc, sn.w);
            }
            if (DETAIL) {
                const int orig = a.mperm[slot_i];
                hit_out[(size_t)cand * a.M + orig] = best;
                cnt_out[(size_t)cand * a.M + orig] = counted ? 1 : 0;
            }
        }
        __builtin_amdgcn_wave_barrier();
    };

    // one 64-point step of this wavefront's candidate: model point p of slot i
    auto step = [&](const int i, const float4 p) {
        float qx = 0.f, qy = 0.f, qz = 0.f, qcentre = 0.f, nearest = 0.f;
        uint32_t off = 0, cnt = 0, yw = 0;
        constexpr uint32_t cmask = STOCS_CONE_COUNT_MASK;   // the list length in the count word; the cell's normal cone sits above it
        // slots beyond the model hold NaN positions (ctx.hip): they run through the look-up like any other query and match nothing;
        // only the per-point outputs of the detail form need the bound
        if (!DETAIL || i < a.M) {
            qx = ((t0 * p.x + t4 * p.y) + t8 * p.z) + t12;
            qy = ((t1 * p.x + t5 * p.y) + t9 * p.z) + t13;
            qz = ((t2 * p.x + t6 * p.y) + t10 * p.z) + t14;
            // one floor per axis at quarter-cell resolution gives both the cell (>> 2) and the sub-cell
            // (& 3); unsigned compares do the bounds test (a NaN query floors to 0, scans cell 0 and
            // matches nothing because every NaN distance fails d <= best)
            const int c4x = __float2int_rd((qx - a.ox) * a.inv_h4), c4y = __float2int_rd((qy - a.oy) * a.inv_h4),
                      c4z = __float2int_rd((qz - a.oz) * a.inv_h4);
            const int cx = c4x >> 2, cy = c4y >> 2, cz = c4z >> 2;
            if ((unsigned)cx < (unsigned)a.nx && (unsigned)cy < (unsigned)a.ny && (unsigned)cz < (unsigned)a.nz) {
                const int sb = ((c4z & 3) << 4) | ((c4y & 3) << 2) | (c4x & 3);
                if (FLAT) {   // one look-up: an empty cell is an all-zero word (count 0, mask 0)
                    uint4 cw = make_uint4(0u, 0u, 0u, 0u);
                    if (!STOCS_ABLATE(a, 1))   // 1: no cell-word look-up at all
                        cw = a.flat[(uint32_t)((cz * a.ny + cy) * a.nx + cx)];
                    const uint32_t mw = sb < 32 ? cw.z : cw.w;
                    // a flagged word (only the flat table has them) names the cell's block of octant lines: the query reads the ONE line of
                    // its octant as a list of 8 entries -- the count such a word carries -- a subset of the cell's list that holds the same
                    // winner (octant_lists.h)
                    off = octant_word_flagged(cw.x) ? octant_line_offset(cw.x, (uint32_t)sb) : cw.x;
                    yw = cw.y; cnt = ((mw >> (sb & 31)) & 1u) ? (cw.y & cmask) : 0u;
                    if (STOCS_ABLATE(a, 2)) cnt = cw.x == 0xFFFFFFF1u ? 1u : 0u;   // 2: look-up done, nobody survives
                } else {
                    const int brick = a.top[((cz >> 3) * a.nby + (cy >> 3)) * a.nbx + (cx >> 3)];
                    if (brick >= 0) {
                        const uint4 cw = a.cells[(uint32_t)brick * 512u + (uint32_t)(((cz & 7) << 6) | ((cy & 7) << 3) | (cx & 7))];
                        yw = cw.y;
                        if ((EARLY || NEAR) && a.has_nearest) { off = cw.x; cnt = cw.y & cmask; nearest = __uint_as_float(cw.z); }   // no mask on these grids: z = distance bound
                        else { const uint32_t mw = a.has_nearest ? 0xFFFFFFFFu : (sb < 32 ? cw.z : cw.w); off = cw.x; cnt = ((mw >> (sb & 31)) & 1u) ? (cw.y & cmask) : 0u; }
                    }
                }
            }
            if ((EARLY || (NEAR && a.has_nearest)) && cnt) {
                const float ex = qx - (a.ox + ((float)cx + 0.5f) * a.h), ey = qy - (a.oy + ((float)cy + 0.5f) * a.h), ez = qz - (a.oz + ((float)cz + 0.5f) * a.h);
                qcentre = sqrtf(ex * ex + (ey * ey + ez * ez));
                // every listed point is at least `nearest` from the cell centre, hence at least nearest - |q - centre| from the query:
                // beyond epsilon the list is not worth a look
                if (a.has_nearest && nearest - qcentre > a.eps + a.bound_margin) cnt = 0;
            }
            // GATE: a query whose cell's normal cone cannot reach dot_lo against the rotated model normal would find its neighbour and
            // then fail the normal test (cone_rules_out_packed, normal_cone.h): it never joins the queue.  The model normal is the packed
            // one in the fourth word of the position (ctx.hip): it arrived with p, one step ahead; the exact one is read by the normal test
            if (GATE && cnt && cone_rules_out_packed(yw, __float_as_uint(p.w), t0, t1, t2, t4, t5, t6, t8, t9, t10, gthr)) cnt = 0;
            if (DETAIL && cnt == 0) {
                const int orig = a.mperm[i];
                hit_out[(size_t)cand * a.M + orig] = -1;
                cnt_out[(size_t)cand * a.M + orig] = 0;
            }
        }
        const bool hit = cnt != 0;
        const unsigned long long mask = __ballot(hit);
        if (mask) {
            if (hit) {
                const int rank = __popcll(mask & ((1ull << lane) - 1ull));
                const int sl = (tail + rank) & 127;
                qt[w][sl] = make_float4(qx, qy, qz, __int_as_float((int)off));
                qn[w][sl] = cnt;
                qs[w][sl] = (uint32_t)i;
                if (EARLY) qcd[w][sl] = qcentre;
            }
            tail += __popcll(mask);
            __builtin_amdgcn_wave_barrier();
            if (tail - head >= 64) {
                process(64);
                head += 64;
            }
        }
    };
    if (CU == 16) {
    // The wavefront's steps as 16-point sub-patches, four per step, 64 at a time: every lane tests the sphere of one sub-patch
    // (a.sub), and the live ones join a per-wave ring in LDS (ballot + mbcnt compaction, as the query queue).  Each 64-lane step
    // takes the next four entries of the ring -- lane l walks point l & 15 of the (l >> 4)-th -- and a window is tested only when
    // fewer than four are left, so only the wavefront's last step can be partial; its empty lanes read the NaN padding behind
    // the model.  (The selection costs a few vector instructions and one LDS read per step: picking the four with scalar
    // find-first-set costs more scalar issue slots than the skipped steps save.)  The model point of the next step is requested
    // one step ahead, as below.
    __shared__ uint16_t live_q[WPB][128];   // global sub-patch indices, a ring (at most 3 + 64 entries pending)
    const int nsteps = (a.M + 63) >> 6;
    if (SHARED) {   // (a.M <= 16 * LCP_SHARED_LIVE: choose_lcp_form)
    // The four wavefronts of a candidate share ONE list of live sub-patches (the memory of the four rings, taken as one array).
    // Window k (sub-patches 64 k .. 64 k + 63) is tested by wavefront k & 3; the live ones of a window are appended behind a base
    // taken with one LDS atomic add per window, so the order of the list differs from run to run -- the scores do not, their sums
    // are integers.  After one barrier the 64-lane steps are dealt round-robin: step s = entries 4 s .. 4 s + 3 goes to wavefront
    // s & 3.  Every wavefront then runs ceil or floor of a quarter of the candidate's steps whatever part of the model the pose
    // leaves alive, the candidate has one partial step instead of up to four (its empty lanes read the NaN padding behind the
    // model), and its sub-patches take ceil(n / 64) windows instead of two per wavefront.  The step loop is a counted loop; the
    // model point of the next step is requested one step ahead, as below.
    __shared__ int live_n;
    uint16_t* const live_all = &live_q[0][0];
    static_assert(!SHARED || WPB * 128 == LCP_SHARED_LIVE, "the shared list is the memory of the per-wave rings");
    if (threadIdx.x == 0) live_n = 0;
    const int nsubs = (a.M + 15) >> 4;   // <= LCP_SHARED_LIVE: at most two windows per wavefront
    const float snorm = GATE ? gnorm : (a.patch ? linear_norm_bound(t0, t1, t2, t4, t5, t6, t8, t9, t10) : 0.0f);
    // windows w and w + 4: both centres, then both look-ups of the distance field back to back, then the two verdicts -- two memory
    // round trips in front of the barrier, not four
    unsigned long long lm[2];
    {
        bool live[2];
        LcpPatchProbe pp[2];
        float fv[2] = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 2; ++j) live[j] = ((w + 4 * j) << 6) + lane < nsubs;
        if (patch_on) {
            // (the cone of a cell is requested with its distance: one round trip for both)
            const uint32_t* const ncone = (const uint32_t*)a.dist + (size_t)a.gnx * (size_t)a.gny * (size_t)a.gnz;
            uint32_t cw[2] = {0u, 0u};
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (j == 0 || two) pp[j] = lcp_patch_probe(a, wsp[j], t0, t1, t2, t4, t5, t6, t8, t9, t10, t12, t13, t14);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (j == 0 || two) {
                    fv[j] = a.dist[pp[j].cell];
                    if (pn_on) cw[j] = ncone[pp[j].cell];
                }
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (j == 0 || two) {
                    live[j] = live[j] && !lcp_patch_verdict(a, pp[j], wsp[j].w, snorm, fv[j]);
                    if (pn_on) live[j] = live[j] && !lcp_patch_normals_dead(a, pp[j], wsp[j].w, snorm, wsn[j], cw[j], t0, t1, t2, t4, t5, t6, t8, t9, t10);
                }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) lm[j] = __ballot(live[j]);
    }
    __syncthreads();   // live_n is zero for everyone (the tests above needed no LDS: nobody waits here for long)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (lm[j]) {   // (wave-uniform)
            int base = 0;
            if (lane == 0) base = atomicAdd(&live_n, __popcll(lm[j]));
            base = __builtin_amdgcn_readfirstlane(base);
            if ((lm[j] >> lane) & 1ull)   // base + rank < the candidate's live sub-patches <= nsubs <= LCP_SHARED_LIVE
                live_all[base + __popcll(lm[j] & ((1ull << lane) - 1ull))] = (uint16_t)(((w + 4 * j) << 6) + lane);
        }
    }
    __syncthreads();
    const int nlive = __builtin_amdgcn_readfirstlane(live_n);
    const int nst = (nlive + 3) >> 2;                                          // steps of the candidate
    const int mine = __builtin_amdgcn_readfirstlane((nst + 3 - w) >> 2);       // steps w, w + 4, ... of them
    // lane l of this wavefront's k-th step walks point l & 15 of entry 16 k + 4 w + (l >> 4); entries beyond the list: the NaN padding
    const int e0 = 4 * w + (lane >> 4);
    auto slot = [&](int k) { const int e = e0 + 16 * k; return e < nlive ? ((int)live_all[e] << 4) + (lane & 15) : (nsteps << 6) + lane; };
    if (mine > 0) {
        // (the sorted positions are padded to whole steps and one step beyond: no bounds checks on these loads)
        int i = slot(0);
        float4 p_next = a.mpos[i];
        for (int k = 0; k < mine; ++k) {
            const int ic = i;
            const float4 p = p_next;
            i = k + 1 < mine ? slot(k + 1) : ic;   // behind the last step its own point is requested once more: no branch around the load
            p_next = a.mpos[i];
            step(ic, p);
        }
    }
    } else {
    const int wfirst = SPLIT ? w : 0, nw = SPLIT ? WPB : 1;
    // this wavefront's sub-patches: k -> step wfirst + (k >> 2) * nw, quarter k & 3 (wave-uniform: the walk's loops branch on scalars)
    const int nsub = __builtin_amdgcn_readfirstlane(4 * ((nsteps - wfirst + nw - 1) / nw));
    const float snorm = GATE ? gnorm : (a.patch ? linear_norm_bound(t0, t1, t2, t4, t5, t6, t8, t9, t10) : 0.0f);
    int qh = 0, qtl = 0;   // ring head and tail
    for (int s0 = 0;; s0 += 64) {
        {   // the window s0 .. s0 + 63 (wave-uniform)
            const int kl = s0 + lane, q = 4 * (wfirst + (kl >> 2) * nw) + (kl & 3);
            const bool in = kl < nsub && (q << 4) < a.M;   // (the quarters of the last step that lie wholly beyond the model: none)
            bool live = in;
            if (a.patch && live && !STOCS_ABLATE(a, 64))
                live = !lcp_patch_dead(a, a.sub[q], snorm, t0, t1, t2, t4, t5, t6, t8, t9, t10, t12, t13, t14);
            const unsigned long long mask = __ballot(live);
            if (live) live_q[w][(qtl + __popcll(mask & ((1ull << lane) - 1ull))) & 127] = (uint16_t)q;
            qtl += __popcll(mask);
            if (DETAIL && a.patch) {   // the skipped sub-patches' points: no neighbour, not counted
                unsigned long long dead = __ballot(in && !live);
                while (dead) {
                    const int j = __builtin_ctzll(dead);
                    dead &= dead - 1ull;
                    const int id = ((4 * (wfirst + ((s0 + j) >> 2) * nw) + ((s0 + j) & 3)) << 4) + lane;
                    if (lane < 16 && id < a.M) {
                        const int orig = a.mperm[id];
                        hit_out[(size_t)cand * a.M + orig] = -1;
                        cnt_out[(size_t)cand * a.M + orig] = 0;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        const bool last = s0 + 64 >= nsub;
        // the steps: four queued sub-patches each, fewer only in the last step of the last window (its other lanes: the NaN padding)
        const int g = lane >> 4;
        auto slot = [&](int t) { return g < t ? ((int)live_q[w][(qh + g) & 127] << 4) + (lane & 15) : (nsteps << 6) + lane; };
        int t = min(qtl - qh, 4);
        if (t == 4 || (last && t > 0)) {
            // (the sorted positions are padded to whole steps and one step beyond: no bounds checks on these loads)
            int i = slot(t);
            float4 p_next = a.mpos[i];
            for (;;) {
                const int ic = i;
                const float4 p = p_next;
                qh += t;
                t = min(qtl - qh, 4);
                const bool more = t == 4 || (last && t > 0);
                i = more ? slot(t) : ic;   // behind the last step its own point is requested once more: no branch around the load
                p_next = a.mpos[i];
                step(ic, p);
                if (!more) break;
            }
        }
        if (last) break;
    }
    }
    } else {
    // The wavefront's steps, 64 at a time: every lane tests the patch of one step (a.patch), the ballot is the list of the
    // steps that have to be walked; the model point of the NEXT such step is requested one step ahead (takes one of the
    // three dependent loads of the look-up chain off the critical path).
    const int nsteps = (a.M + 63) >> 6;
    const int wfirst = SPLIT ? w : 0, nw = SPLIT ? WPB : 1;
    const int nk = (nsteps - wfirst + nw - 1) / nw;
    const float snorm = GATE ? gnorm : (a.patch ? linear_norm_bound(t0, t1, t2, t4, t5, t6, t8, t9, t10) : 0.0f);
    for (int k0 = 0; k0 < nk; k0 += 64) {
        const int kk = k0 + lane;
        bool live = kk < nk;
        if (a.patch && live && !STOCS_ABLATE(a, 64))
            live = !lcp_patch_dead(a, a.patch[wfirst + kk * nw], snorm, t0, t1, t2, t4, t5, t6, t8, t9, t10, t12, t13, t14);
        unsigned long long todo = __ballot(live);
        if (DETAIL && a.patch) {   // the skipped steps' points: no neighbour, not counted
            unsigned long long dead = __ballot(kk < nk && !live);
            while (dead) {
                const int j = __builtin_ctzll(dead);
                dead &= dead - 1ull;
                const int i = ((wfirst + (k0 + j) * nw) << 6) + lane;
                if (i < a.M) {
                    const int orig = a.mperm[i];
                    hit_out[(size_t)cand * a.M + orig] = -1;
                    cnt_out[(size_t)cand * a.M + orig] = 0;
                }
            }
        }
        if (!todo) continue;
        // (the sorted positions are padded to whole steps and one step beyond: no bounds checks on these loads)
        int j = __builtin_ctzll(todo);
        float4 p_next = a.mpos[((wfirst + (k0 + j) * nw) << 6) + lane];
        for (;;) {
            const int i = ((wfirst + (k0 + j) * nw) << 6) + lane;
            const float4 p = p_next;
            todo &= todo - 1ull;
            j = todo ? __builtin_ctzll(todo) : j;   // behind the last step its own point is requested once more: no branch around the load
            p_next = a.mpos[((wfirst + (k0 + j) * nw) << 6) + lane];
            step(i, p);
            if (!todo) break;
        }
    }
    }
    if (tail - head > 0) process(tail - head);
    acc = lcp_wave_sum(acc);
    if (SPLIT) {
        if (lane == 0) part[w] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long total = 0;
#pragma unroll
            for (int k = 0; k < WPB; ++k) total += part[k];
            lcp_store(a, out, cand, total);
        }
    } else if (lane == 0) lcp_store(a, out, cand, acc);
}

// ---------------------------------------------------------------------------------------------
// Exact-ties scoring (stocs_set_option "exact_ties" = 1; divergence Q11).  The form of lcp_kernel (a lane per query,
// one wavefront per candidate, the whole cell list scanned: no sub-cell mask, no early exit, no patch test), which also records
// whether the query's minimum distance within epsilon^2 is held by two or more listed points.  Such a query -- and one whose only
// answer lies exactly at epsilon^2, where the reference's strict split-plane pruning (kdtree.h:409) can skip the point -- is answered
// again by the reference-order kd-tree (kdtree.h), whose answer is the reference's: the point its visiting order reaches last.
// Every other query has one nearest point, which both structures find.  The lists hold every scene point within epsilon of the cell
// box except the dominated ones of grid.hip's pruning, which are strictly farther than another listed point from every position of
// the cell and so can neither win nor tie.  Scores, detail rows, per-trial weights and the arg-max key go through the same helpers as
// the scan kernels.  ties[0] counts the queries sent to the tree, ties[1] those whose tree answer differs from the largest-index rule.
// ---------------------------------------------------------------------------------------------
template <bool DETAIL>
__global__ __launch_bounds__(256) void lcp_exact_kernel(LcpArgs a, const float* __restrict__ T16, float* __restrict__ out, int n,
                                                        int32_t* __restrict__ hit_out, uint8_t* __restrict__ cnt_out,
                                                        const KdNodeP* __restrict__ kd_nodes, const float4* __restrict__ kd_pts,
                                                        unsigned long long* __restrict__ ties) {
    const int lane = threadIdx.x & 63;
    const int cand = lcp_candidate(a, n, threadIdx.x >> 6);
    if (cand < 0) return;
    const float* T = T16 + (size_t)cand * 16;
    const float4* __restrict__ snrmw = lcp_weights_of(a, cand);
    const float t0 = T[0], t1 = T[1], t2 = T[2], t4 = T[4], t5 = T[5], t6 = T[6], t8 = T[8], t9 = T[9], t10 = T[10],
                t12 = T[12], t13 = T[13], t14 = T[14];
    unsigned long long acc = 0ull, n_flag = 0ull, n_changed = 0ull;
    for (int i = lane; i < a.M; i += 64) {
        const float4 p = a.mpos[i];
        const float qx = ((t0 * p.x + t4 * p.y) + t8 * p.z) + t12;
        const float qy = ((t1 * p.x + t5 * p.y) + t9 * p.z) + t13;
        const float qz = ((t2 * p.x + t6 * p.y) + t10 * p.z) + t14;
        const float fx = floorf((qx - a.ox) * a.inv_h);
        const float fy = floorf((qy - a.oy) * a.inv_h);
        const float fz = floorf((qz - a.oz) * a.inv_h);
        int best = -1;
        bool tie = false;
        float bd = a.sq_eps;
        if (fx >= 0.0f && fy >= 0.0f && fz >= 0.0f && fx < (float)a.nx && fy < (float)a.ny && fz < (float)a.nz) {
            const int cx = (int)fx, cy = (int)fy, cz = (int)fz;
            const int brick = a.top[((cz >> 3) * a.nby + (cy >> 3)) * a.nbx + (cx >> 3)];
            if (brick >= 0) {
                const uint4 cw = a.cells[(size_t)brick * 512 + (((cz & 7) << 6) | ((cy & 7) << 3) | (cx & 7))];
                const uint32_t cn = cw.y & STOCS_CONE_COUNT_MASK;   // (the bits above hold the cell's normal cone: normal_cone.h)
                for (uint32_t k = 0; k < cn; ++k) {
                    const float4 s = a.list[cw.x + k];
                    const float dx = qx - s.x, dy = qy - s.y, dz = qz - s.z;
                    const float d = dx * dx + (dy * dy + dz * dz);
                    const int ei = __float_as_int(s.w);
                    // any list order (the dense grid's lists are sorted by distance from the cell centre): the largest index among the
                    // points at the minimum; a tie only against a point already held, not against the initial bound epsilon^2
                    if (d < bd) { bd = d; best = ei; tie = false; }
                    else if (d == bd) { if (best >= 0) { tie = true; best = max(best, ei); } else best = ei; }
                }
            }
        }
        if (tie || (best >= 0 && bd == a.sq_eps)) {
            const int kb = kd_query_closest(kd_nodes, kd_pts, qx, qy, qz, a.sq_eps);
            n_flag++;
            if (kb != best) n_changed++;
            best = kb;
        }
        bool counted = false;
        if (best >= 0) {
            const float4 nm = a.mnrm[i];
            const float nx = t0 * nm.x + (t4 * nm.y + t8 * nm.z);
            const float ny = t1 * nm.x + (t5 * nm.y + t9 * nm.z);
            const float nz = t2 * nm.x + (t6 * nm.y + t10 * nm.z);
            const float4 sn = snrmw[best];
            const float d = sn.x * nx + (sn.y * ny + sn.z * nz);
            counted = (d >= a.dot_lo) && (d <= 1.0f);
            if (counted) lcp_add(acc, sn.w);
        }
        if (DETAIL) {
            const int orig = a.mperm[i];
            hit_out[(size_t)cand * a.M + orig] = best;
            cnt_out[(size_t)cand * a.M + orig] = counted ? 1 : 0;
        }
    }
    acc = lcp_wave_sum(acc);
    n_flag = lcp_wave_sum(n_flag);
    n_changed = lcp_wave_sum(n_changed);
    if (lane == 0) {
        lcp_store(a, out, cand, acc);
        if (n_flag) atomicAdd(&ties[0], n_flag);
        if (n_changed) atomicAdd(&ties[1], n_changed);
    }
}

// compute_best_transform (stocs.cpp:982-1004) on the device: the maximum of the positive scores' keys (best_key, stocs_math.h)
__global__ __launch_bounds__(256) void best_kernel(const float* __restrict__ lcp, int n, uint32_t id_offset, unsigned long long* __restrict__ best) {
    unsigned long long k = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float s = lcp[i];
        if (s > 0.0f) { const unsigned long long key = best_key(s, id_offset + (uint32_t)i); k = key > k ? key : k; }
    }
    k = wave_max_key(k);
    if ((threadIdx.x & 63) == 0 && k) atomicMax(best, k);
}

// the same for one batch of moderate size in ONE workgroup: no zero fill in front, no atomics, the key is simply written.  best_key and wave_max_key
// stay written out here: with either the compiler orders this kernel's instructions differently (profiles/post_layer_refactor.md)
__global__ __launch_bounds__(1024) void best_single_kernel(const float* __restrict__ lcp, int n, uint32_t id_offset, unsigned long long* __restrict__ best) {
    __shared__ unsigned long long sh[16];
    unsigned long long k = 0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const float s = lcp[i];
        if (s > 0.0f) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(0xFFFFFFFFu - (id_offset + (uint32_t)i));
            k = key > k ? key : k;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off, 64);
        k = o > k ? o : k;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) k = sh[w] > k ? sh[w] : k;
        *best = k;
    }
}

// processing order of a batch: Morton code of the candidate's translation (= where the model centroid lands) in the
// scene grid's bounding box, 8 bits per axis (2 mm at a 0.5 m scene: candidate batches are concentrated around a few
// hypotheses, coarse buckets of 1.5 cm lost a third of the gain).  Candidates that put the model in the same place read the same
// bricks, cell words and lists; running them back to back raises the L1 / L2 hit rates (Cm: 1.67 -> 1.44 ms).
__device__ __forceinline__ uint32_t spread10(uint32_t x) {
    x &= 0x3ff; x = (x | (x << 16)) & 0x30000ff; x = (x | (x << 8)) & 0x300f00f; x = (x | (x << 4)) & 0x30c30c3; x = (x | (x << 2)) & 0x9249249;
    return x;
}
__global__ __launch_bounds__(256) void order_keys_kernel(const float* __restrict__ T16, int n, float ox, float oy, float oz, float sx, float sy, float sz,
                                                         uint32_t* __restrict__ keys, int32_t* __restrict__ vals, unsigned long long* __restrict__ best) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && best) *best = 0ull;   // the arg-max word of the launch that follows (saves a fill kernel of its own)
    if (i >= n) return;
    const float* T = T16 + (size_t)i * 16;
    const float qx = fminf(fmaxf((T[12] - ox) * sx, 0.0f), 255.0f), qy = fminf(fmaxf((T[13] - oy) * sy, 0.0f), 255.0f),
                qz = fminf(fmaxf((T[14] - oz) * sz, 0.0f), 255.0f);   // NaN -> 0 (fmaxf ignores it)
    keys[i] = (spread10((uint32_t)qz) << 2) | (spread10((uint32_t)qy) << 1) | spread10((uint32_t)qx);
    vals[i] = i;
}

// ---------------------------------------------------------------------------------------------
// Kernel selection.  The library ships the kernels the automatic choice uses -- the queue-fed scan over index-ordered lists on
// sparse scenes (lcp_variant 24), over centre-sorted lists with early exit on dense ones (39) -- plus two independent
// cross-checks: the per-step cooperative scan over the centre-sorted lists (31) and the plain lane-per-query kernel (0); every
// one of them returns the reference's scores.  What lost an A/B run is gone from the code (DESIGN_HISTORY.md lists the forms and
// the last commit that holds them; profiles/r01_lcp_analysis.md, profiles/r03_lcp_patch_and_group_ab.json hold their figures).
// ---------------------------------------------------------------------------------------------
enum LcpKernel { LCP_PLAIN, LCP_STEP, LCP_QUEUE, LCP_EXACT };   // lcp_kernel, lcp_coop_kernel, lcp_coopq_kernel, lcp_exact_kernel
struct LcpForm {
    LcpKernel kernel;
    bool detail;   // every kernel: per-point output
    bool dense;    // plain and queue kernels: centre-sorted lists (the per-step kernel knows no other)
    bool split;    // per-step and queue kernels: four wavefronts share a candidate
    bool flat, near;   // queue kernel (see the table above it); false elsewhere
    int cu;            // queue kernel: 16 or 64; 64 elsewhere
    bool shared;       // queue kernel, split and cu == 16: one list of live sub-patches per candidate (models of up to 8 192 points)
    bool gate;         // queue kernel, scoring forms on sparse lists: the normal-cone gate (a grid with cones, lcp_normal_gate = 1)
};

static bool lcp_variant_selectable(int v) { return v == 99 || v == 0 || v == 24 || v == 31 || v == 39; }

// The form a call runs.  Must not depend on the batch size (a candidate's score is batch-invariant).
static LcpForm choose_lcp_form(const stocs_ctx* c, const LcpArgs& a, bool detail) {
    LcpForm f = {LCP_QUEUE, detail, false, false, false, false, 64, false, false};
    if (c->exact_ties) { f.kernel = LCP_EXACT; return f; }
    // dense grids keep their lists sorted by distance from the cell centre (not by index): only kernels instantiated with the
    // order-independent tie rule may scan them
    f.dense = c->grid.d_chunk_r != NULL;
    const int variant = c->lcp_variant >= 0 ? c->lcp_variant : 99;
    // automatic: the queue kernel on every grid.  (Sparse grids with more than 10 entries per list once went to a per-step scan; since
    // the queue kernel verifies with four lanes per query it wins there too: 50 000 / 12 500 points 3.54 -> 2.35 ms.)  On dense grids
    // it runs with early exit, lanes per query as on sparse scenes (C5: 6.33 -> 5.81 ms).  A variant the grid cannot run maps to the
    // queue form of that grid: 24 on a dense grid -> 39, 31 and 39 on a sparse one -> 24
    if (variant == 0) f.kernel = (detail && f.dense) ? LCP_STEP : LCP_PLAIN;   // (no plain detail kernel for centre-sorted lists)
    else if (variant == 31 && f.dense) f.kernel = LCP_STEP;
    // four wavefronts per candidate pay from 512 model points on.  Queue kernel: a trial's ~8 000 candidates finish 40 % sooner (one
    // round of long wavefronts becomes four rounds of short ones), 32 768 candidates 9 % sooner, 65 536 the same.  Per-step kernel:
    // C5 (16 384 candidates x 50 000 points) 11.6 -> 8.3 ms; eight: 8.1 ms, but 20 % slower at Cm.  The detail forms are never
    // split, the dense queue form always is
    const bool split = c->lcp_split && a.M >= 512;
    if (f.kernel == LCP_STEP) f.split = !detail && split;
    if (f.kernel == LCP_QUEUE) {
        f.split = !detail && (f.dense || split);
        f.flat = !detail && !f.dense && c->lcp_flat && a.flat;
        f.near = !f.dense && a.has_nearest;   // pruned lists on a grid finer than epsilon: the distance bound in place of the sub-cell mask
        // the unit of the patch test (lcp_cull_unit); without the test the walk of whole steps (CU = 64) is the one to run
        f.cu = (a.patch && c->lcp_cull_unit == 16) ? 16 : 64;
        f.shared = f.split && f.cu == 16 && a.M <= 16 * LCP_SHARED_LIVE;   // (the model size, never the batch)
        // the cones hold the normals of c->d_snrmw; a trial batch's own arrays (snrmw_override, cand_trial) are copies of it whose
        // weights alone differ (sample.hip: init_trial_state_kernel copies, the sampling writes .w), so those launches stay gated
        f.gate = !detail && !f.dense && c->grid.has_cones && c->lcp_normal_gate != 0 && !(f.split && f.cu == 16 && !f.shared);   // (no gated split ring form at CU = 16: the table)
    }
    return f;
}

typedef void (*LcpScanFn)(LcpArgs, const float*, float*, int, int32_t*, uint8_t*);

// the queue kernel of a form: bits 0..7 of I are DETAIL, DENSE, SPLIT, FLAT, NEAR, CU == 16, SHARED and GATE; NULL where the form is not legal
template <int I>
static LcpScanFn lcp_queue_fn() {
    constexpr bool DETAIL = (I & 1) != 0, DENSE = (I & 2) != 0, SPLIT = (I & 4) != 0, FLAT = (I & 8) != 0, NEAR = (I & 16) != 0;
    constexpr int CU = (I & 32) ? 16 : 64;
    constexpr bool SHARED = (I & 64) != 0, GATE = (I & 128) != 0;
    if constexpr (lcp_queue_form_legal(DETAIL, DENSE, SPLIT, FLAT, NEAR, CU, SHARED, GATE)) return lcp_coopq_kernel<DETAIL, DENSE, SPLIT, FLAT, NEAR, CU, SHARED, GATE>;
    else return NULL;
}
template <int... I>
static LcpScanFn lcp_queue_fn(const LcpForm& f, std::integer_sequence<int, I...>) {
    static const LcpScanFn table[] = {lcp_queue_fn<I>()...};
    return table[(f.detail ? 1 : 0) | (f.dense ? 2 : 0) | (f.split ? 4 : 0) | (f.flat ? 8 : 0) | (f.near ? 16 : 0) | (f.cu == 16 ? 32 : 0) | (f.shared ? 64 : 0) | (f.gate ? 128 : 0)];
}

// Run-time form -> template instantiation, grid and block: the one place that names the kernels.
static int launch_lcp_form(stocs_ctx* c, const LcpForm& f, const LcpArgs& a, const float* d_T16, int n, float* d_lcp, int32_t* d_hit, uint8_t* d_counted) {
    // split: a workgroup of four wavefronts per candidate.  Else the cooperative scoring kernels run one wavefront per workgroup and
    // candidate; the plain and exact kernels and every detail form put four candidates into a workgroup
    const bool cooperative = f.kernel == LCP_STEP || f.kernel == LCP_QUEUE;
    const bool one_wave = cooperative && !f.detail && !f.split;
    const dim3 grid((unsigned)(f.split || one_wave ? n : (n + 3) / 4)), block(one_wave ? 64 : 256);
    if (f.kernel == LCP_EXACT) {
        if (f.detail) hipLaunchKernelGGL(lcp_exact_kernel<true>, grid, block, 0, c->stream, a, d_T16, d_lcp, n, d_hit, d_counted, c->d_kd_nodes, c->d_kd_pts, c->d_ties);
        else hipLaunchKernelGGL(lcp_exact_kernel<false>, grid, block, 0, c->stream, a, d_T16, d_lcp, n, d_hit, d_counted, c->d_kd_nodes, c->d_kd_pts, c->d_ties);
    } else {
        LcpScanFn fn = NULL;
        if (f.kernel == LCP_QUEUE) fn = lcp_queue_fn(f, std::make_integer_sequence<int, 256>());
        else if (f.kernel == LCP_STEP) fn = f.detail ? lcp_coop_kernel<true, false> : (f.split ? lcp_coop_kernel<false, true> : lcp_coop_kernel<false, false>);
        else if (!f.detail) fn = f.dense ? lcp_kernel<false, false> : lcp_kernel<false, true>;
        else if (!f.dense) fn = lcp_kernel<true, true>;
        if (!fn) { set_error("launch_lcp: no kernel for this form (kernel %d, detail %d, dense %d, split %d, flat %d, near %d, cu %d, shared %d, gate %d)", (int)f.kernel, (int)f.detail, (int)f.dense, (int)f.split, (int)f.flat, (int)f.near, f.cu, (int)f.shared, (int)f.gate); return STOCS_ERR_STATE; }
        hipLaunchKernelGGL(fn, grid, block, 0, c->stream, a, d_T16, d_lcp, n, d_hit, d_counted);
    }
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

// The form of this launch, and with it whether the launch tests the sub-patches' normal cones: only a shared-list form reads the cone
// field, so only a launch that runs one fills it (once per scene, behind the distances) and is given its reach.  A model that is never
// split, lcp_split = 0, lcp_cull_unit = 64 and the detail forms never pay for the field.
static int launch_chosen_form(stocs_ctx* c, LcpArgs& a, const float* d_T16, int n, float* d_lcp, int32_t* d_hit, uint8_t* d_counted) {
    const LcpForm f = choose_lcp_form(c, a, d_hit != NULL);
    a.nreach = 0.0f;
    if (f.kernel == LCP_QUEUE && f.shared && c->lcp_patch_normals && c->grid.d_ncone && c->grid.dist_ready) {
        int rc = fill_cull_field(c);
        if (rc) return rc;
        a.nreach = c->grid.pn_reach;
        c->pn_launches++;
    }
    return launch_lcp_form(c, f, a, d_T16, n, d_lcp, d_hit, d_counted);
}

int launch_lcp(stocs_ctx* c, const float* d_T16, int n, float* d_lcp, int32_t* d_hit, uint8_t* d_counted, unsigned long long* d_best8, uint32_t id_offset) {
    if (n <= 0) { if (d_best8) STOCS_HIP_CHECK(hipMemsetAsync(d_best8, 0, 8, c->stream)); return STOCS_OK; }
    bool best_zeroed = false;
    LcpArgs a;
    a.best = d_best8; a.id_offset = id_offset;
#ifdef STOCS_TOOLS_BUILD
    a.ablate = getenv("STOCS_LCP_ABLATE") ? atoi(getenv("STOCS_LCP_ABLATE")) : 0;
#endif
    a.mpos = c->d_mpos_s; a.mnrm = c->d_mnrm_s; a.mperm = c->d_mperm; a.M = c->nM;
    a.top = c->grid.d_top; a.cells = c->grid.d_cells; a.flat = c->grid.d_flat; a.list = c->grid.d_list; a.snrmw = c->snrmw_override ? c->snrmw_override : c->d_snrmw;
    a.cand_trial = c->lcp_cand_trial; a.snrmw_stride = c->lcp_cand_trial ? c->snrmw_stride : 0;
    a.ox = c->grid.ox; a.oy = c->grid.oy; a.oz = c->grid.oz; a.inv_h = c->grid.inv_h; a.inv_h4 = c->grid.inv_h * 4.0f; a.h = c->grid.h; a.chunk_r = c->grid.d_chunk_r;
    a.nx = c->grid.nx; a.ny = c->grid.ny; a.nz = c->grid.nz; a.nbx = c->grid.nbx; a.nby = c->grid.nby;
    a.sq_eps = c->prm.distance_threshold * c->prm.distance_threshold;  // sq_eps = epsilon*epsilon, stocs.cpp:1014
    a.dot_lo = c->thr.lcp_dot_lo;
    a.eps = c->prm.distance_threshold;
    a.has_nearest = c->grid.has_nearest ? 1 : 0;
    {   // 4e-6 at metre scale (epsilon 5 mm, coordinates below half a metre); clouds in millimetres get a thousand times that
        double mag = 0.0;
        for (int k = 0; k < 3; ++k) mag = std::max(mag, std::max(fabs(c->grid.bb_mn[k]), fabs(c->grid.bb_mx[k])));
        a.bound_margin = (float)(4.0e-4 * (double)c->prm.distance_threshold + 4.0e-6 * mag);
    }
    // patch test: its distance field costs one pass over the scene points (0.24 ms at Cm) and takes ~6 % off a launch, so it is filled
    // once the scene has seen 1e9 point queries (three steps of the metric batch; ~25 trials of one frame) -- a caller that scores one
    // trial per frame never pays for it.  The scores do not depend on it
    a.patch = NULL; a.sub = NULL; a.dist = NULL; a.nreach = 0.0f;
    a.gox = a.goy = a.goz = 0.f; a.g = a.inv_g = a.cap = 0.f; a.gnx = a.gny = a.gnz = 0;
    c->scene_scored++;
    c->scene_work += (double)n * (double)c->nM;
    if (c->exact_ties) {
        // the reference-order tie rule (lcp_exact_kernel): every candidate in batch order, the arg-max in the same epilogue
        int rc = ensure_kdtree(c);
        if (rc) return rc;
        if (!c->ties_started) { STOCS_HIP_CHECK(hipMemsetAsync(c->d_ties, 0, 16, c->stream)); c->ties_started = true; }
        a.order = NULL; a.xcd_blocks = 0;
        if (d_best8 && !(d_best8 == c->d_best && c->best_is_zero)) STOCS_HIP_CHECK(hipMemsetAsync(d_best8, 0, 8, c->stream));
        if (d_best8 == c->d_best) c->best_is_zero = false;
        return launch_chosen_form(c, a, d_T16, n, d_lcp, d_hit, d_counted);
    }
    if (c->lcp_cull && c->grid.d_dist && c->d_mpatch && (c->grid.dist_ready || c->lcp_cull >= 2 || c->scene_work >= c->lcp_cull_after)) {
        int rc = fill_cull_field(c, NULL, false);   // the distances; the cones when the form of this launch reads them (launch_chosen_form)
        if (rc) return rc;
        if (c->cull_pending) { STOCS_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_cull, 0)); c->cull_pending = false; }   // filled at stocs_ctx_set_scene, on the auxiliary stream
        a.patch = c->d_mpatch; a.sub = c->d_msub; a.dist = c->grid.d_dist;
        a.gox = c->grid.cg_ox; a.goy = c->grid.cg_oy; a.goz = c->grid.cg_oz; a.g = c->grid.cg_g; a.inv_g = c->grid.cg_inv_g; a.cap = c->grid.cg_cap;
        a.gnx = c->grid.cg_nx; a.gny = c->grid.cg_ny; a.gnz = c->grid.cg_nz;
    }
    // octant lines of the long cells (octant_lists.h): like the distance field they cost about what one launch of 8 000 candidates takes
    // and pay on big batches (-2 to -2.9 % at Cm; STOCS_GRID_OCTANTS=0 builds a grid without them), so they are written once the scene has seen the same amount of work, whatever lcp_cull says.
    // The scores do not depend on them
    if (c->grid.oct_pending && c->scene_work >= c->lcp_cull_after) { int rc = build_octant_lines(c); if (rc) return rc; }
    a.order = NULL; a.xcd_blocks = 0;
    // big batches against scenes whose lists do not stay in the caches: spatially ordered processing (the ordering costs ~50 us; scores
    // do not depend on it).  Until the first half of round 3 it paid at Cm too (1.67 -> 1.44 ms in round 1); with the four-lane verify
    // trips it is a wash there (9 MB of lists: 1.115 ms either way at 65 536 candidates, +3 % at 32 768, +8 % for a 1 000-point model)
    // and still worth 7-12 % from 20 MB of lists on (50 000-point scene 2.55 -> 2.38 ms, C5 6.53 -> 5.73): the threshold is 12 MB;
    // lcp_order >= 2 orders whatever the size
    const bool lists_spill = (double)c->grid.n_entries * 16.0 >= 12.0e6;
    if (!d_hit && n >= 1024 && (double)n * (double)c->nM >= 1.5e8 && c->lcp_order && (lists_spill || c->lcp_order >= 2)) {
        const size_t kb = al256((size_t)n * 4);
        size_t tb = 0;
        STOCS_HIP_CHECK(sort_pairs(NULL, tb, (const uint32_t*)NULL, (uint32_t*)NULL, (const uint32_t*)NULL, (uint32_t*)NULL, (size_t)n, 0, 24, c->stream));
        const size_t need = 4 * kb + tb;
        { const int rc = c->order.grow(c->stream, need); if (rc) return rc; }
        char* p = c->order.p;
        uint32_t* keys = (uint32_t*)p; uint32_t* keys_s = (uint32_t*)(p + kb);
        int32_t* vals = (int32_t*)(p + 2 * kb); int32_t* order = (int32_t*)(p + 3 * kb);
        void* tmp = p + 4 * kb;
        const float sx = 256.0f / ((float)c->grid.nx * c->grid.h), sy = 256.0f / ((float)c->grid.ny * c->grid.h), sz = 256.0f / ((float)c->grid.nz * c->grid.h);
        hipLaunchKernelGGL(order_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_T16, n, c->grid.ox, c->grid.oy, c->grid.oz, sx, sy, sz,
                           keys, vals, d_best8);
        best_zeroed = true;
        STOCS_HIP_CHECK(sort_pairs(tmp, tb, keys, keys_s, (const uint32_t*)vals, (uint32_t*)order, (size_t)n, 0, 24, c->stream));
        a.order = order;
        // XCD placement of the ordered list (lcp_candidate): 0 = workgroup i takes slot i, and the hardware deals consecutive workgroups to
        // the eight XCDs in turn; k > 2 = an XCD takes runs of k consecutive slots, so that what is resident on it at one time (~250
        // workgroups) comes from one or two stretches of the ordered list and shares list lines in ITS L2.  Pays only when the lists are
        // far beyond the Infinity Cache: C5 (1.6 GB) 5.73 -> 5.38 ms with runs of 128 (96: 5.60, 160: 5.95, 256: 5.49, 512 and more: 6.3
        // -- whole XCDs finish late), 65 536 candidates 20.6 -> 19.4; a 100 000-point scene (158 MB) 2.74 -> 2.98, 50 000 points 2.38 -> 2.50
        const bool lists_huge = (double)c->grid.n_entries * 16.0 >= 512.0e6;
        a.xcd_blocks = c->lcp_order >= 2 ? (c->lcp_order == 2 ? 1 : c->lcp_order) : (lists_huge ? 128 : 0);
    }
    if (d_best8 && d_best8 == c->d_best && c->best_is_zero) best_zeroed = true;   // stocs_make_transforms left the word zeroed for this launch
    if (d_best8 == c->d_best) c->best_is_zero = false;
    if (d_best8 && !best_zeroed) STOCS_HIP_CHECK(hipMemsetAsync(d_best8, 0, 8, c->stream));
    return launch_chosen_form(c, a, d_T16, n, d_lcp, d_hit, d_counted);
}

// the arg-max key of n scores (n > 0) into *d_key8, on the context's stream: one workgroup up to 2^18 scores, else zero fill + atomic max
static int enqueue_best(stocs_ctx* c, const float* d_lcp, int n, uint32_t id_offset, unsigned long long* d_key8) {
    if (n <= (1 << 18)) {
        hipLaunchKernelGGL(best_single_kernel, dim3(1), dim3(1024), 0, c->stream, d_lcp, n, id_offset, d_key8);
    } else {
        STOCS_HIP_CHECK(hipMemsetAsync(d_key8, 0, 8, c->stream));
        const int blocks = std::min((n + 255) / 256, 1024);
        hipLaunchKernelGGL(best_kernel, dim3(blocks), dim3(256), 0, c->stream, d_lcp, n, id_offset, d_key8);
    }
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

// the context's own key word (c->d_best) -> host, through pinned memory; waits for the stream
static int read_best_key(stocs_ctx* c, uint64_t* key) {
    int rc = ensure_pinned(c, PIN_VAR);
    if (rc) return rc;
    uint64_t* key_pin = (uint64_t*)((char*)c->h_pin + PIN_BEST);
    STOCS_HIP_CHECK(hipMemcpyAsync(key_pin, c->d_best, 8, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    *key = *key_pin;
    return STOCS_OK;
}

}  // namespace stocs

using namespace stocs;

extern "C" {

int stocs_score_transforms_device(stocs_ctx* c, const void* d_T16, int n, void* d_lcp) {
    if (!c || n < 0 || (n && (!d_T16 || !d_lcp))) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    return launch_lcp(c, (const float*)d_T16, n, (float*)d_lcp, NULL, NULL, NULL, 0);
}

int stocs_score_transforms(stocs_ctx* c, const float* T_host, int n, float* lcp_host) {
    if (!c || n < 0 || (n && (!T_host || !lcp_host))) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    if (n == 0) return STOCS_OK;
    const size_t tb = (size_t)n * 64, lb = (size_t)n * 4;
    int rc = ensure_scratch(c, tb + lb + 256);
    if (rc) return rc;
    float* dT = (float*)c->d_scratch;
    float* dL = (float*)((char*)c->d_scratch + al256(tb));
    STOCS_HIP_CHECK(hipMemcpyAsync(dT, T_host, tb, hipMemcpyHostToDevice, c->stream));
    rc = launch_lcp(c, dT, n, dL, NULL, NULL, NULL, 0);
    if (rc) return rc;
    STOCS_HIP_CHECK(hipMemcpyAsync(lcp_host, dL, lb, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return STOCS_OK;
}

int stocs_lcp_detail(stocs_ctx* c, const float* T_host, int32_t* hit, uint8_t* counted) {
    if (!c || !T_host || !hit || !counted) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    const size_t M = (size_t)c->nM;
    int rc = ensure_scratch(c, 256 + 256 + M * 4 + 256 + M);
    if (rc) return rc;
    char* base = (char*)c->d_scratch;
    float* dT = (float*)base;
    float* dL = (float*)(base + 256);
    int32_t* dH = (int32_t*)(base + 512);
    uint8_t* dC = (uint8_t*)(base + 512 + al256(M * 4));
    STOCS_HIP_CHECK(hipMemcpyAsync(dT, T_host, 64, hipMemcpyHostToDevice, c->stream));
    rc = launch_lcp(c, dT, 1, dL, dH, dC, NULL, 0);
    if (rc) return rc;
    STOCS_HIP_CHECK(hipMemcpyAsync(hit, dH, M * 4, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipMemcpyAsync(counted, dC, M, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return STOCS_OK;
}

// hits / counted flags of a chunk of candidates -> two totals
__global__ __launch_bounds__(256) void hit_count_kernel(const int32_t* __restrict__ hit, const uint8_t* __restrict__ counted, size_t n, unsigned long long* __restrict__ out2) {
    unsigned long long h = 0, k = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { h += hit[i] >= 0 ? 1u : 0u; k += counted[i] ? 1u : 0u; }
    for (int off = 32; off > 0; off >>= 1) { h += __shfl_xor(h, off, 64); k += __shfl_xor(k, off, 64); }
    if ((threadIdx.x & 63) == 0) { if (h) atomicAdd(&out2[0], h); if (k) atomicAdd(&out2[1], k); }
}

int stocs_lcp_hit_count(stocs_ctx* c, const void* d_T16, int n, int64_t* hits, int64_t* counted) {
    if (!c || n < 0 || (n && !d_T16) || !hits) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    *hits = 0;
    if (counted) *counted = 0;
    if (n == 0 || c->nM == 0) return STOCS_OK;
    const size_t M = (size_t)c->nM;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)256 << 20) / (5 * M)));
    const size_t hb = al256((size_t)chunk * M * 4), cb = al256((size_t)chunk * M), lb = al256((size_t)chunk * 4);
    int rc = ensure_scratch(c, 256 + lb + hb + cb);
    if (rc) return rc;
    char* base = (char*)c->d_scratch;
    unsigned long long* d_out = (unsigned long long*)base;
    float* dL = (float*)(base + 256);
    int32_t* dH = (int32_t*)(base + 256 + lb);
    uint8_t* dC = (uint8_t*)(base + 256 + lb + hb);
    STOCS_HIP_CHECK(hipMemsetAsync(d_out, 0, 16, c->stream));
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        rc = launch_lcp(c, (const float*)d_T16 + (size_t)i0 * 16, m, dL, dH, dC, NULL, 0);
        if (rc) return rc;
        hipLaunchKernelGGL(hit_count_kernel, dim3(1024), dim3(256), 0, c->stream, (const int32_t*)dH, (const uint8_t*)dC, (size_t)m * M, d_out);
        STOCS_HIP_CHECK(hipGetLastError());
    }
    if ((rc = ensure_pinned(c, PIN_VAR))) return rc;
    unsigned long long* pin = (unsigned long long*)((char*)c->h_pin + PIN_BEST);
    STOCS_HIP_CHECK(hipMemcpyAsync(pin, d_out, 16, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    *hits = (int64_t)pin[0];
    if (counted) *counted = (int64_t)pin[1];
    return STOCS_OK;
}

// stocs_lcp_gate_count: one lane per (candidate, model slot).  The query, its cell and the sub-cell mask as the queue kernel's step
// computes them (brick look-up; no mask on has_nearest grids), then the kernel's own gate function on the packed model normal that
// the kernel reads (the fourth word of the position) with the kernel's own threshold
__global__ __launch_bounds__(256) void gate_count_kernel(LcpArgs a, const float* __restrict__ T16, size_t total, const uint8_t* __restrict__ counted,
                                                         unsigned long long* __restrict__ out3, int has_cones) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long nq = 0, nr = 0, nb = 0;
    if (g < total) {
        const size_t cand = g / (size_t)a.M;
        const int i = (int)(g % (size_t)a.M);
        const float* T = T16 + cand * 16;
        const float t0 = T[0], t1 = T[1], t2 = T[2], t4 = T[4], t5 = T[5], t6 = T[6], t8 = T[8], t9 = T[9], t10 = T[10], t12 = T[12], t13 = T[13], t14 = T[14];
        const float4 p = a.mpos[i];
        const float qx = ((t0 * p.x + t4 * p.y) + t8 * p.z) + t12;
        const float qy = ((t1 * p.x + t5 * p.y) + t9 * p.z) + t13;
        const float qz = ((t2 * p.x + t6 * p.y) + t10 * p.z) + t14;
        const int c4x = __float2int_rd((qx - a.ox) * a.inv_h4), c4y = __float2int_rd((qy - a.oy) * a.inv_h4), c4z = __float2int_rd((qz - a.oz) * a.inv_h4);
        const int cx = c4x >> 2, cy = c4y >> 2, cz = c4z >> 2;
        uint32_t cnt = 0, yw = 0;
        if ((unsigned)cx < (unsigned)a.nx && (unsigned)cy < (unsigned)a.ny && (unsigned)cz < (unsigned)a.nz) {
            const int sb = ((c4z & 3) << 4) | ((c4y & 3) << 2) | (c4x & 3);
            const int brick = a.top[((cz >> 3) * a.nby + (cy >> 3)) * a.nbx + (cx >> 3)];
            if (brick >= 0) {
                const uint4 cw = a.cells[(uint32_t)brick * 512u + (uint32_t)(((cz & 7) << 6) | ((cy & 7) << 3) | (cx & 7))];
                const uint32_t mw = a.has_nearest ? 0xFFFFFFFFu : (sb < 32 ? cw.z : cw.w);
                yw = cw.y; cnt = ((mw >> (sb & 31)) & 1u) ? (cw.y & STOCS_CONE_COUNT_MASK) : 0u;
            }
        }
        if (cnt) {
            nq = 1;
            const float gthr = model_normal_gate_threshold(a.dot_lo, linear_norm_bound(t0, t1, t2, t4, t5, t6, t8, t9, t10));
            if (has_cones && cone_rules_out_packed(yw, __float_as_uint(p.w), t0, t1, t2, t4, t5, t6, t8, t9, t10, gthr)) {
                nr = 1;
                nb = counted[cand * (size_t)a.M + (size_t)a.mperm[i]] ? 1 : 0;
            }
        }
    }
    nq = lcp_wave_sum(nq); nr = lcp_wave_sum(nr); nb = lcp_wave_sum(nb);
    if ((threadIdx.x & 63) == 0) { if (nq) atomicAdd(&out3[0], nq); if (nr) atomicAdd(&out3[1], nr); if (nb) atomicAdd(&out3[2], nb); }
}

int stocs_lcp_gate_count(stocs_ctx* c, const void* d_T16, int n, int64_t out[3]) {
    if (!c || n < 0 || (n && !d_T16) || !out) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    out[0] = out[1] = out[2] = 0;
    if (n == 0 || c->nM == 0 || c->nS == 0) return STOCS_OK;
    const size_t M = (size_t)c->nM;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)256 << 20) / (5 * M)));
    const size_t hb = al256((size_t)chunk * M * 4), cb = al256((size_t)chunk * M), lb = al256((size_t)chunk * 4);
    int rc = ensure_scratch(c, 256 + lb + hb + cb);
    if (rc) return rc;
    char* base = (char*)c->d_scratch;
    unsigned long long* d_out = (unsigned long long*)base;
    float* dL = (float*)(base + 256);
    int32_t* dH = (int32_t*)(base + 256 + lb);
    uint8_t* dC = (uint8_t*)(base + 256 + lb + hb);
    LcpArgs a;
    memset(&a, 0, sizeof(a));
    a.mpos = c->d_mpos_s; a.mnrm = c->d_mnrm_s; a.mperm = c->d_mperm; a.M = c->nM;
    a.top = c->grid.d_top; a.cells = c->grid.d_cells;
    a.ox = c->grid.ox; a.oy = c->grid.oy; a.oz = c->grid.oz; a.inv_h4 = c->grid.inv_h * 4.0f;
    a.nx = c->grid.nx; a.ny = c->grid.ny; a.nz = c->grid.nz; a.nbx = c->grid.nbx; a.nby = c->grid.nby;
    a.dot_lo = c->thr.lcp_dot_lo;
    a.has_nearest = c->grid.has_nearest ? 1 : 0;
    STOCS_HIP_CHECK(hipMemsetAsync(d_out, 0, 24, c->stream));
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        const float* dT = (const float*)d_T16 + (size_t)i0 * 16;
        rc = launch_lcp(c, dT, m, dL, dH, dC, NULL, 0);
        if (rc) return rc;
        const size_t total = (size_t)m * M;
        hipLaunchKernelGGL(gate_count_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, a, dT, total, (const uint8_t*)dC, d_out, c->grid.has_cones ? 1 : 0);
        STOCS_HIP_CHECK(hipGetLastError());
    }
    if ((rc = ensure_pinned(c, PIN_VAR))) return rc;
    unsigned long long* pin = (unsigned long long*)((char*)c->h_pin + PIN_BEST);
    STOCS_HIP_CHECK(hipMemcpyAsync(pin, d_out, 24, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; ++k) out[k] = (int64_t)pin[k];
    return STOCS_OK;
}

// stocs_lcp_patch_normal_count: one lane per (candidate, sub-patch), the two halves of the patch test as the shared-list forms' prologue
// runs them (the same device functions, the same records), and the detail form's counted flags of the sub-patch's 16 points
__global__ __launch_bounds__(256) void patch_normal_count_kernel(LcpArgs a, const float* __restrict__ T16, size_t total, const uint8_t* __restrict__ counted,
                                                                 unsigned long long* __restrict__ out3) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nsubs = (a.M + 15) >> 4;
    unsigned long long nl = 0, nr = 0, nb = 0;
    if (g < total) {
        const size_t cand = g / (size_t)nsubs;
        const int q = (int)(g % (size_t)nsubs);
        const float* T = T16 + cand * 16;
        const float t0 = T[0], t1 = T[1], t2 = T[2], t4 = T[4], t5 = T[5], t6 = T[6], t8 = T[8], t9 = T[9], t10 = T[10], t12 = T[12], t13 = T[13], t14 = T[14];
        const float sn = linear_norm_bound(t0, t1, t2, t4, t5, t6, t8, t9, t10);
        const float4 sp = a.sub[q], rec = a.sub[(((a.M + 63) >> 6) << 2) + q];
        const LcpPatchProbe pp = lcp_patch_probe(a, sp, t0, t1, t2, t4, t5, t6, t8, t9, t10, t12, t13, t14);
        const uint32_t* const ncone = (const uint32_t*)a.dist + (size_t)a.gnx * (size_t)a.gny * (size_t)a.gnz;
        if (!lcp_patch_verdict(a, pp, sp.w, sn, a.dist[pp.cell])) {
            nl = 1;
            if (lcp_patch_normals_dead(a, pp, sp.w, sn, rec, ncone[pp.cell], t0, t1, t2, t4, t5, t6, t8, t9, t10)) {
                nr = 1;
                for (int i = 16 * q; i < min(16 * q + 16, a.M); ++i) nb |= counted[cand * (size_t)a.M + (size_t)a.mperm[i]] ? 1ull : 0ull;
            }
        }
    }
    nl = lcp_wave_sum(nl); nr = lcp_wave_sum(nr); nb = lcp_wave_sum(nb);
    if ((threadIdx.x & 63) == 0) { if (nl) atomicAdd(&out3[0], nl); if (nr) atomicAdd(&out3[1], nr); if (nb) atomicAdd(&out3[2], nb); }
}

int stocs_lcp_patch_normal_count(stocs_ctx* c, const void* d_T16, int n, int64_t out[3]) {
    if (!c || n < 0 || (n && !d_T16) || !out) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    out[0] = out[1] = out[2] = 0;
    if (n == 0 || c->nM == 0 || c->nS == 0 || !c->grid.d_dist || !c->grid.d_ncone || !c->d_msub) return STOCS_OK;
    const size_t M = (size_t)c->nM, nsubs = (M + 15) / 16;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)256 << 20) / (5 * M)));
    const size_t hb = al256((size_t)chunk * M * 4), cb = al256((size_t)chunk * M), lb = al256((size_t)chunk * 4);
    int rc = ensure_scratch(c, 256 + lb + hb + cb);
    if (rc) return rc;
    char* base = (char*)c->d_scratch;
    unsigned long long* d_out = (unsigned long long*)base;
    float* dL = (float*)(base + 256);
    int32_t* dH = (int32_t*)(base + 256 + lb);
    uint8_t* dC = (uint8_t*)(base + 256 + lb + hb);
    // both fields, whatever the options and the scene's scoring work say
    const int keep = c->lcp_patch_normals;
    c->lcp_patch_normals = 1;
    rc = fill_cull_field(c);
    c->lcp_patch_normals = keep;
    if (rc) return rc;
    if (c->cull_pending) { STOCS_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_cull, 0)); c->cull_pending = false; }
    LcpArgs a;
    memset(&a, 0, sizeof(a));
    a.M = c->nM; a.mperm = c->d_mperm; a.sub = c->d_msub; a.dist = c->grid.d_dist;
    a.eps = c->prm.distance_threshold; a.dot_lo = c->thr.lcp_dot_lo; a.nreach = c->grid.pn_reach;
    a.gox = c->grid.cg_ox; a.goy = c->grid.cg_oy; a.goz = c->grid.cg_oz; a.g = c->grid.cg_g; a.inv_g = c->grid.cg_inv_g; a.cap = c->grid.cg_cap;
    a.gnx = c->grid.cg_nx; a.gny = c->grid.cg_ny; a.gnz = c->grid.cg_nz;
    STOCS_HIP_CHECK(hipMemsetAsync(d_out, 0, 24, c->stream));
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        const float* dT = (const float*)d_T16 + (size_t)i0 * 16;
        rc = launch_lcp(c, dT, m, dL, dH, dC, NULL, 0);   // the detail form: counted flags per (candidate, model point)
        if (rc) return rc;
        const size_t total = (size_t)m * nsubs;
        hipLaunchKernelGGL(patch_normal_count_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, a, dT, total, (const uint8_t*)dC, d_out);
        STOCS_HIP_CHECK(hipGetLastError());
    }
    if ((rc = ensure_pinned(c, PIN_VAR))) return rc;
    unsigned long long* pin = (unsigned long long*)((char*)c->h_pin + PIN_BEST);
    STOCS_HIP_CHECK(hipMemcpyAsync(pin, d_out, 24, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; ++k) out[k] = (int64_t)pin[k];
    return STOCS_OK;
}

int stocs_patch_normal_info(stocs_ctx* c, double out[4]) {
    if (!c || !out) return STOCS_ERR_INVALID;
    const SceneGrid& g = c->grid;
    out[0] = g.d_ncone ? (double)g.pn_reach : 0.0;
    out[1] = g.d_ncone ? (double)g.pn_w : 0.0;
    out[2] = g.d_ncone && g.ncone_ready ? 1.0 : 0.0;
    out[3] = (double)c->pn_launches;
    return STOCS_OK;
}

float stocs_patch_normal_bound_host(uint32_t cone_word, const float* v3, float sb, float s, int* outside, float* axis3) {
    bool o = false;
    const float b = pn_bound(cone_word, v3[0], v3[1], v3[2], sb, s, &o);
    if (outside) *outside = o ? 1 : 0;
    if (axis3) pn_axis(cone_word, axis3[0], axis3[1], axis3[2]);
    return b;
}

int stocs_best_device(stocs_ctx* c, const void* d_lcp, int n, uint32_t id_offset, uint64_t* key) {
    if (!c || !key || n < 0 || (n && !d_lcp)) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    *key = 0;
    if (n == 0) return STOCS_OK;
    if (!c->d_best) STOCS_HIP_CHECK(dev_malloc((void**)&c->d_best, 8));
    c->best_is_zero = false;
    int rc = enqueue_best(c, (const float*)d_lcp, n, id_offset, c->d_best);
    if (rc) return rc;
    return read_best_key(c, key);
}

int stocs_best_device_async(stocs_ctx* c, const void* d_lcp, int n, uint32_t id_offset, void* d_key8) {
    if (!c || !d_key8 || n < 0 || (n && !d_lcp)) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    if (n == 0) { STOCS_HIP_CHECK(hipMemsetAsync(d_key8, 0, 8, c->stream)); return STOCS_OK; }
    return enqueue_best(c, (const float*)d_lcp, n, id_offset, (unsigned long long*)d_key8);
}

int stocs_score_best_device_async(stocs_ctx* c, const void* d_T16, int n, void* d_lcp, uint32_t id_offset, void* d_key8) {
    if (!c || !d_key8 || n < 0 || (n && (!d_T16 || !d_lcp))) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    return launch_lcp(c, (const float*)d_T16, n, (float*)d_lcp, NULL, NULL, (unsigned long long*)d_key8, id_offset);
}

int stocs_score_best_device(stocs_ctx* c, const void* d_T16, int n, void* d_lcp, uint32_t id_offset, uint64_t* key) {
    if (!c || !key) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    if (!c->d_best) STOCS_HIP_CHECK(dev_malloc((void**)&c->d_best, 8));
    int rc = stocs_score_best_device_async(c, d_T16, n, d_lcp, id_offset, c->d_best);
    if (rc) return rc;
    return read_best_key(c, key);
}

int stocs_set_option(stocs_ctx* c, const char* key, int value) {
    if (!c || !key) return STOCS_ERR_INVALID;
    if (!strcmp(key, "lcp_variant")) {
        if (!lcp_variant_selectable(value)) { set_error("stocs_set_option: lcp_variant %d is not part of this build (99 automatic, 0, 24, 31, 39)", value); return STOCS_ERR_INVALID; }
        c->lcp_variant = value;
        return STOCS_OK;
    }
    // 0 off, 1 spatial order, 2 + XCD-contiguous halves of the list, k > 2 + chunks of k consecutive slots per XCD
    if (!strcmp(key, "lcp_order") && value >= 0 && value <= 4096) { c->lcp_order = value; return STOCS_OK; }
    // 1: stocs_find_congruent_all times its kernel groups with HIP events ("device: ..." steps of stocs_last_call_timing); 0 (default): host steps only
    if (!strcmp(key, "device_clock") && (value == 0 || value == 1)) { c->device_clock = value; return STOCS_OK; }
    // 0: brick look-ups only, 1: the flat cell table when the grid has one (takes effect for kernels launched afterwards;
    // the table itself is built with the scene grid)
    if (!strcmp(key, "lcp_flat") && (value == 0 || value == 1)) { c->lcp_flat = value; return STOCS_OK; }
    // 1 (default): the queue kernel's scoring forms on sparse lists drop the queries that their cell's normal cone rules out before they
    // reach the queue (same scores); 0: the forms without the gate
    if (!strcmp(key, "lcp_normal_gate")) {
        if (value != 0 && value != 1) { set_error("stocs_set_option: lcp_normal_gate takes 0 or 1, not %d", value); return STOCS_ERR_INVALID; }
        c->lcp_normal_gate = value;
        return STOCS_OK;
    }
    // 1: tied nearest-neighbour queries take the reference kd-tree's answer (lcp_exact_kernel, kdtree.h); 0 (default): largest index
    if (!strcmp(key, "exact_ties")) {
        if (value != 0 && value != 1) { set_error("stocs_set_option: exact_ties takes 0 or 1, not %d", value); return STOCS_ERR_INVALID; }
        c->exact_ties = value;
        return STOCS_OK;
    }
    // 1 (default): the shared-list forms' patch test also rules sub-patches out by their normal cones (patch_normals.h; same scores); 0: spheres alone
    if (!strcmp(key, "lcp_patch_normals")) {
        if (value != 0 && value != 1) { set_error("stocs_set_option: lcp_patch_normals takes 0 or 1, not %d", value); return STOCS_ERR_INVALID; }
        c->lcp_patch_normals = value;
        return STOCS_OK;
    }
    // 0: one wavefront per candidate, 1 (default): four wavefronts share a candidate's model points (same scores)
    if (!strcmp(key, "lcp_split") && (value == 0 || value == 1)) { c->lcp_split = value; return STOCS_OK; }
    // 0: every 64-point step is walked; 1 (default): steps whose bounding sphere is out of reach of the scene are skipped once the scene's
    // distance field pays (1e9 point queries against the scene so far); 2: from the first call (same scores in every case)
    if (!strcmp(key, "lcp_cull") && value >= 0 && value <= 2) { c->lcp_cull = value; return STOCS_OK; }
    // points per bounding sphere of that test: 16 (default: sub-patches, the live ones packed four to a step) or 64 (whole steps)
    if (!strcmp(key, "lcp_cull_unit") && (value == 16 || value == 64)) { c->lcp_cull_unit = value; return STOCS_OK; }
    // the threshold of lcp_cull = 1, in MILLIONS of point queries (candidates x model points) scored against the current scene:
    // default 1000 (= 1e9: the field costs ~0.25 ms at 20 000 scene points and takes ~6 % off a launch); 0 = from the first call
    if (!strcmp(key, "lcp_cull_after") && value >= 0) { c->lcp_cull_after = (double)value * 1.0e6; return STOCS_OK; }
    // lanes that verify one queued query together: 4 (two list entries per lane) is the only form; the key is kept for callers that set it
    if (!strcmp(key, "lcp_group") && value == 4) return STOCS_OK;
    set_error("stocs_set_option: unknown option or value");
    return STOCS_ERR_INVALID;
}

int stocs_get_cull_state(stocs_ctx* c, float* patches4, int32_t* perm, int* n_patches, float* geom8, float* dist, int64_t dist_cap, int64_t* n_dist) {
    if (!c || !n_patches || !n_dist) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    const int np = c->d_mpatch ? (c->nM + 63) / 64 : 0;
    *n_patches = np;
    const SceneGrid& g = c->grid;
    const int64_t nd = g.d_dist ? (int64_t)g.cg_nx * g.cg_ny * g.cg_nz : 0;
    *n_dist = nd;
    // (everything that can fail comes before the first copy into the caller's pageable buffers: no copy is left in flight on an error return)
    if (dist && nd) {
        if (dist_cap < nd) return STOCS_ERR_CAPACITY;
        int rc = fill_cull_field(c);
        if (rc) return rc;
        if (c->cull_pending) { STOCS_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_cull, 0)); c->cull_pending = false; }
    }
    if (patches4 && np) STOCS_HIP_CHECK(hipMemcpyAsync(patches4, c->d_mpatch, (size_t)np * 16, hipMemcpyDeviceToHost, c->stream));
    if (perm) for (int i = 0; i < c->nM; ++i) perm[i] = c->h_mperm[i];
    if (geom8) {
        geom8[0] = g.cg_ox; geom8[1] = g.cg_oy; geom8[2] = g.cg_oz; geom8[3] = g.cg_g; geom8[4] = g.cg_cap;
        geom8[5] = (float)g.cg_nx; geom8[6] = (float)g.cg_ny; geom8[7] = (float)g.cg_nz;
    }
    hipError_t e = hipSuccess;
    if (dist && nd) e = hipMemcpyAsync(dist, g.d_dist, (size_t)nd * 4, hipMemcpyDeviceToHost, c->stream);
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));   // also behind a failed enqueue: the earlier copies have landed before the caller's buffers go away
    STOCS_HIP_CHECK(e);
    return STOCS_OK;
}

int stocs_get_grid_info(stocs_ctx* c, stocs_grid_info* info) {
    if (!c || !info) { set_error("stocs_get_grid_info: NULL %s", !c ? "context" : "info"); return STOCS_ERR_INVALID; }
    memset(info, 0, sizeof(*info));
    const SceneGrid& g = c->grid;
    if (c->nS <= 0 || !g.d_top) { set_error("stocs_get_grid_info: no scene"); return STOCS_ERR_STATE; }
    info->origin[0] = g.ox; info->origin[1] = g.oy; info->origin[2] = g.oz;
    info->h = g.h; info->inv_h = g.inv_h; info->div = g.div;
    info->cells[0] = g.nx; info->cells[1] = g.ny; info->cells[2] = g.nz;
    info->bricks[0] = g.nbx; info->bricks[1] = g.nby; info->bricks[2] = g.nbz;
    info->centre_sorted = g.d_chunk_r != NULL; info->pruned = g.pruned; info->has_nearest = g.has_nearest; info->has_cones = g.has_cones;
    info->has_flat = g.d_flat != NULL;
    info->sort = g.sort_kind; info->prune_group = g.prune_group; info->prune_k = g.prune_k; info->longest_list = g.longest_list;
    info->n_incidences = g.n_inc; info->n_cells = g.n_cells; info->n_bricks = g.n_bricks; info->n_entries = g.n_entries;
    return STOCS_OK;
}

int stocs_get_grid_octants(stocs_ctx* c, int64_t* counts3) {
    if (!c || !counts3) { set_error("stocs_get_grid_octants: NULL %s", !c ? "context" : "counts"); return STOCS_ERR_INVALID; }
    counts3[0] = 0; counts3[1] = 0; counts3[2] = 0;
    const SceneGrid& g = c->grid;
    if (c->nS <= 0 || !g.d_top) { set_error("stocs_get_grid_octants: no scene"); return STOCS_ERR_STATE; }
    counts3[0] = g.n_long_cells; counts3[1] = g.n_octant_cells; counts3[2] = g.n_octant_entries;
    return STOCS_OK;
}

int stocs_time_score_kernel(stocs_ctx* c, const void* d_T16, int n, void* d_lcp, int reps, float* avg_ms) {
    if (!c || !avg_ms || reps <= 0 || n <= 0) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    STOCS_HIP_CHECK(hipEventRecord(c->ev0, c->stream));
    for (int r = 0; r < reps; ++r) {
        int rc = launch_lcp(c, (const float*)d_T16, n, (float*)d_lcp, NULL, NULL, NULL, 0);
        if (rc) return rc;
    }
    STOCS_HIP_CHECK(hipEventRecord(c->ev1, c->stream));
    STOCS_HIP_CHECK(hipEventSynchronize(c->ev1));
    float ms = 0;
    STOCS_HIP_CHECK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *avg_ms = ms / (float)reps;
    return STOCS_OK;
}

}  // extern "C"
