// grid.hip -- the scene brick grid (SceneGrid, stocs_ctx.h) built on the GPU.
// Replaces the kd-tree construction of the reference (Super4PCS::KdTree, include/super4pcs/accelerators/
// kdtree.h:191-330, built by stocs_estimator::kdtree_initialize, stocs.cpp:966-980) as the spatial index of the
// verification pass; the restricted-radius query it has to answer is kdtree.h:387-442.
//
// A new scene arrives with every camera frame, so the build is part of the per-frame latency: every stage is
// kernels and rocPRIM primitives on the context's stream (the host computes the geometry, grid_geometry.h, and sizes buffers).
// build_grid_gpu runs them in this order (the stages of its Build), for the GridForm it is given:
//   1. count: per point the cells whose box is within r of it -- r = 1.001 eps, more on scenes wider than ~2 100 eps, see
//      grid_geometry.h (double arithmetic, the same predicate for count and fill) -- and the prefix sums of those counts;
//   2. sort: the (cell key, point) incidences, one stable radix sort by cell key (brick << 9 | local cell) -- incidences are
//      generated in ascending point order, so a cell's list comes out in ascending scene index (the tie rule of the scan kernels
//      relies on it); centre-sorted lists append a 16-bit quantised distance to the cell centre to the key;
//   3. cells: run boundaries -> non-empty cells -> bricks (prefix sums);
//   4. layout: per cell its first incidence, key and brick; pruned lists: the entries that can win somewhere in the cell;
//      padded list offsets (multiples of 8 entries = whole 128-byte lines, sentinel-filled);
//   5. lists: cell words (offset, count, 64-bit sub-cell mask), the top-level brick table, the flat table, the lists;
//   6. chunk_bounds (centre-sorted lists): per 8-entry chunk a lower bound of the distance to the cell centre (suffix minimum
//      of the exact distances, so the quantised order only affects how early the scan stops, never the result).
// HBM-bound integer/byte work; no MFMA.
#include <math.h>

#include <algorithm>

#include "normal_cone.h"
#include "patch_normals.h"
#include "octant_lists.h"
#include "prims.h"
#include "stocs_ctx.h"

namespace stocs {

struct GridGeom {
    double of[3];     // origin (the float origin the scan kernels use, widened)
    double h, r;      // cell edge, inclusion radius
    int n[3];         // cells per axis
    int nbx, nby;
    int dense;        // 1: key carries the quantised centre distance
    double qscale;    // quantisation of the centre distance to 16 bits
};

__device__ __forceinline__ void cell_range(const GridGeom& G, const double p[3], int lo[3], int hi[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = max(0, (int)floor((p[k] - G.r - G.of[k]) / G.h));
        hi[k] = min(G.n[k] - 1, (int)floor((p[k] + G.r - G.of[k]) / G.h));
    }
}

__device__ __forceinline__ double box_dist2(const GridGeom& G, const double p[3], int cx, int cy, int cz) {
    const int cc[3] = {cx, cy, cz};
    double d2 = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double b0 = G.of[k] + cc[k] * G.h, b1 = b0 + G.h;
        const double d = p[k] < b0 ? b0 - p[k] : (p[k] > b1 ? p[k] - b1 : 0.0);
        d2 += d * d;
    }
    return d2;
}

// FILL = false: number of cells within r of every point; FILL = true: their (key, point) records
// keys32 != NULL (FILL; keys of at most 32 bits): the records' keys go there as 32-bit words (the library's own sort takes those)
template <bool FILL>
__global__ __launch_bounds__(256) void incidence_kernel(GridGeom G, const float4* __restrict__ spos, int nS, uint32_t* __restrict__ cnt,
                                                        const unsigned long long* __restrict__ off, uint64_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals, uint32_t* __restrict__ keys32 = NULL) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nS) return;
    const float4 pf = spos[i];
    const double p[3] = {pf.x, pf.y, pf.z};
    int lo[3], hi[3];
    cell_range(G, p, lo, hi);
    uint32_t c = 0;
    unsigned long long o = FILL ? off[i] : 0ull;
    for (int cz = lo[2]; cz <= hi[2]; ++cz)
        for (int cy = lo[1]; cy <= hi[1]; ++cy)
            for (int cx = lo[0]; cx <= hi[0]; ++cx) {
                if (box_dist2(G, p, cx, cy, cz) > G.r * G.r) continue;
                if (FILL) {
                    const uint64_t brick = ((uint64_t)(cz >> 3) * G.nby + (uint64_t)(cy >> 3)) * G.nbx + (uint64_t)(cx >> 3);
                    uint64_t key = (brick << 9) | (uint64_t)(((cz & 7) << 6) | ((cy & 7) << 3) | (cx & 7));
                    if (G.dense) {
                        const double dx = p[0] - (G.of[0] + (cx + 0.5) * G.h), dy = p[1] - (G.of[1] + (cy + 0.5) * G.h),
                                     dz = p[2] - (G.of[2] + (cz + 0.5) * G.h);
                        const double q = sqrt(dx * dx + dy * dy + dz * dz) * G.qscale;
                        key = (key << 16) | (uint64_t)(q < 65535.0 ? (unsigned)q : 65535u);
                    }
                    if (keys32) keys32[o + c] = (uint32_t)key; else keys[o + c] = key;
                    vals[o + c] = (uint32_t)i;
                }
                c++;
            }
    if (!FILL) cnt[i] = c;
}

__global__ __launch_bounds__(256) void widen_keys_kernel(const uint32_t* __restrict__ k32, size_t n, uint64_t* __restrict__ k64) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) k64[e] = (uint64_t)k32[e];
}

// first incidence of every cell (keys sorted; the low `qbits` bits are not part of the cell)
__global__ __launch_bounds__(256) void cell_flags_kernel(const uint64_t* __restrict__ keys, size_t n, int qbits, uint32_t* __restrict__ cflag,
                                                         uint32_t* __restrict__ bflag) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const uint64_t ck = keys[e] >> qbits;
    const uint64_t pk = e ? (keys[e - 1] >> qbits) : ~0ull;
    cflag[e] = (e == 0 || ck != pk) ? 1u : 0u;
    bflag[e] = (e == 0 || (ck >> 9) != (pk >> 9)) ? 1u : 0u;   // first incidence of a brick
}

// per non-empty cell: first incidence, cell key, brick ordinal
__global__ __launch_bounds__(256) void cell_records_kernel(const uint64_t* __restrict__ keys, size_t n, int qbits, const uint32_t* __restrict__ cflag,
                                                           const uint32_t* __restrict__ cidx, const uint32_t* __restrict__ bflag,
                                                           const uint32_t* __restrict__ bidx, uint32_t* __restrict__ cell_first, uint64_t* __restrict__ cell_key,
                                                           uint32_t* __restrict__ cell_brick) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || !cflag[e]) return;
    const uint32_t c = cidx[e];        // exclusive scan of cflag = ordinal of this cell
    cell_first[c] = (uint32_t)e;
    cell_key[c] = keys[e] >> qbits;
    // bidx = exclusive scan of the brick-start flags: the bricks that start strictly before e.  The cell's own brick
    // is that many if e opens it, one less otherwise
    cell_brick[c] = bidx[e] + bflag[e] - 1u;
}

// padded length of every cell's list
__global__ __launch_bounds__(256) void cell_padded_kernel(const uint32_t* __restrict__ cell_first, uint32_t n_cells, uint32_t n_inc, uint32_t pad,
                                                          uint32_t* __restrict__ padded, uint32_t* __restrict__ max_count) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cells) return;
    const uint32_t cnt = (c + 1 < n_cells ? cell_first[c + 1] : n_inc) - cell_first[c];
    padded[c] = (cnt + pad - 1u) & ~(pad - 1u);   // whole 128-byte lines: 8 entries of 16 bytes, or 16 of 8 bytes (dense scenes)
    atomicMax(max_count, cnt);
}

__global__ __launch_bounds__(256) void fill_i32_kernel(int32_t* __restrict__ a, size_t n, int32_t v) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = v;
}
__global__ __launch_bounds__(256) void fill_list_kernel(float4* __restrict__ a, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = make_float4(1.0e30f, 1.0e30f, 1.0e30f, __int_as_float(-1));   // sentinel: far away, index -1
}
__global__ __launch_bounds__(256) void zero_cells_kernel(uint4* __restrict__ a, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = make_uint4(0u, 0u, 0u, 0u);
}

// cell word + top table; one wavefront per non-empty cell, lane = sub-cell.  Sub-cell masks (cell edge = eps
// only): bit s is set when some point of the cell's list lies within r of sub-cell s (any point that close to a
// sub-cell is that close to the cell, hence in its list); the 64 lanes ballot the mask.
__global__ __launch_bounds__(256) void cell_words_kernel(GridGeom G, int div, const uint32_t* __restrict__ cell_first, const uint64_t* __restrict__ cell_key,
                                                         const uint32_t* __restrict__ cell_brick, const uint32_t* __restrict__ list_off,
                                                         uint32_t n_cells, uint32_t n_inc, const uint32_t* __restrict__ vals,
                                                         const float4* __restrict__ spos, int32_t* __restrict__ top, uint4* __restrict__ cells,
                                                         uint4* __restrict__ flat, const uint32_t* __restrict__ kept,
                                                         const uint32_t* __restrict__ rank, const float4* __restrict__ snrmw, int cones) {
    const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int s = threadIdx.x & 63;
    if (c >= n_cells) return;   // whole wavefront
    const uint32_t first = cell_first[c];
    const uint32_t cnt = (c + 1 < n_cells ? cell_first[c + 1] : n_inc) - first;
    const uint64_t key = cell_key[c];
    const uint64_t brick = key >> 9;
    const uint32_t local = (uint32_t)(key & 511);
    const uint32_t b = cell_brick[c];
    uint32_t mlo = 0xFFFFFFFFu, mhi = 0xFFFFFFFFu;
    if (div == 1) {
        const int bx = (int)(brick % (uint64_t)G.nbx), by = (int)((brick / (uint64_t)G.nbx) % (uint64_t)G.nby),
                  bz = (int)(brick / ((uint64_t)G.nbx * (uint64_t)G.nby));
        const int cx = bx * 8 + (int)(local & 7), cy = by * 8 + (int)((local >> 3) & 7), cz = bz * 8 + (int)(local >> 6);
        const double hs = G.h / 4.0;
        const int sc[3] = {4 * cx + (s & 3), 4 * cy + ((s >> 2) & 3), 4 * cz + (s >> 4)};
        bool any = false;
        for (uint32_t k = 0; k < cnt && !any; ++k) {
            const float4 pf = spos[vals[first + k]];   // same address in every lane: one broadcast load
            const double p[3] = {pf.x, pf.y, pf.z};
            double d2 = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double b0 = G.of[a] + sc[a] * hs, b1 = b0 + hs;
                const double d = p[a] < b0 ? b0 - p[a] : (p[a] > b1 ? p[a] - b1 : 0.0);
                d2 += d * d;
            }
            any = d2 <= G.r * G.r;
        }
        const unsigned long long m = __ballot(any);
        mlo = (uint32_t)(m & 0xFFFFFFFFull); mhi = (uint32_t)(m >> 32);
    }
    // normal cone of the cell's stored list (normal_cone.h): the lanes take the list's entries in turn.  Axis = the mean direction,
    // quantised; the half-angle is then measured against the axis as the kernels decode it, in double, and rounded outwards
    uint32_t cone = 0u;
    if (cones) {
        // a lane's first entry stays in registers for the second pass (lists beyond 64 entries are read again); the axis needs no rigour
        // (float sums: any axis is a valid one), the angle against it does
        float4 n0 = make_float4(0.f, 0.f, 0.f, 0.f);
        bool have0 = false, bad = false;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (uint32_t k = (uint32_t)s; k < cnt; k += 64) {
            if (rank && rank[first + k] == 0xFFFFFFFFu) continue;   // pruned away: not in the stored list
            const float4 nf = snrmw[vals[first + k]];
            if (k < 64) { n0 = nf; have0 = true; }
            const double n2 = (double)nf.x * nf.x + (double)nf.y * nf.y + (double)nf.z * nf.z;
            if (!(n2 >= 0.99980001 && n2 <= 1.00020001)) { bad = true; continue; }   // off unit length by more than 1e-4 (NaN included)
            sx += nf.x; sy += nf.y; sz += nf.z;
        }
        for (int off = 32; off > 0; off >>= 1) { sx += __shfl_xor(sx, off, 64); sy += __shfl_xor(sy, off, 64); sz += __shfl_xor(sz, off, 64); }
        const double l1 = fabs((double)sx) + fabs((double)sy) + fabs((double)sz);
        if (!__any(bad) && l1 > 1.0e-9) {
            double px = sx / l1, py = sy / l1;
            if (sz < 0) { const double qx = (1.0 - fabs(py)) * (px >= 0 ? 1.0 : -1.0), qy = (1.0 - fabs(px)) * (py >= 0 ? 1.0 : -1.0); px = qx; py = qy; }
            const double amax = (double)STOCS_CONE_AXIS_MAX;
            const uint32_t u8 = (uint32_t)fmin(fmax(floor((px * 0.5 + 0.5) * amax + 0.5), 0.0), amax);
            const uint32_t v8 = (uint32_t)fmin(fmax(floor((py * 0.5 + 0.5) * amax + 0.5), 0.0), amax);
            float fx, fy, fz;
            cone_axis(cone_pack(u8, v8, 0u), fx, fy, fz);
            const double o2 = (double)fx * fx + (double)fy * fy + (double)fz * fz;
            // cos of the angle to the decoded axis, in double, as a float rounded DOWN (a wider cone); minimum over the list
            auto cos_down = [&](const float4 nf) {
                const double n2 = (double)nf.x * nf.x + (double)nf.y * nf.y + (double)nf.z * nf.z;
                return __double2float_rd(((double)nf.x * fx + (double)nf.y * fy + (double)nf.z * fz) / sqrt(n2 * o2));
            };
            float cmin = 1.0f;
            if (have0) cmin = fminf(cmin, cos_down(n0));
            for (uint32_t k = (uint32_t)s + 64; k < cnt; k += 64) {
                if (rank && rank[first + k] == 0xFFFFFFFFu) continue;
                cmin = fminf(cmin, cos_down(snrmw[vals[first + k]]));
            }
            for (int off = 32; off > 0; off >>= 1) cmin = fminf(cmin, __shfl_xor(cmin, off, 64));
            if (cmin > 0.0f) {   // below 90 degrees
                const double cm = (double)cmin;
                const double sd = sqrt(fmax((1.0 - cm) * (1.0 + cm), 0.0));
                const uint32_t cls = (uint32_t)floor(sd * (double)STOCS_CONE_SIN_STEPS + 1.0e-4) + 1u;   // sin(half-angle) < cls / 16, double rounding included
                if (cls <= STOCS_CONE_MAX_CLASS) cone = cone_pack(u8, v8, cls);
            }
        }
    }
    if (s == 0) {
        top[brick] = (int32_t)b;   // every cell of the brick writes the same value
        const uint4 w = make_uint4(list_off[c], (kept ? kept[c] : cnt) | cone, mlo, mhi);   // (pruned lists: the mask above still comes from every point within r)
        cells[(size_t)b * 512 + local] = w;
        if (flat) {
            const int bx = (int)(brick % (uint64_t)G.nbx), by = (int)((brick / (uint64_t)G.nbx) % (uint64_t)G.nby), bz = (int)(brick / ((uint64_t)G.nbx * (uint64_t)G.nby));
            const int cx = bx * 8 + (int)(local & 7), cy = by * 8 + (int)((local >> 3) & 7), cz = bz * 8 + (int)(local >> 6);
            if (cx < G.n[0] && cy < G.n[1] && cz < G.n[2]) flat[((size_t)cz * G.n[1] + cy) * G.n[0] + cx] = w;
        }
    }
}

// list entries: incidence e of cell c goes to list_off[c] + (e - first[c])
__global__ __launch_bounds__(256) void list_fill_kernel(const uint32_t* __restrict__ cflag, const uint32_t* __restrict__ cidx,
                                                        const uint32_t* __restrict__ cell_first, const uint32_t* __restrict__ list_off,
                                                        const uint32_t* __restrict__ vals, size_t n, const float4* __restrict__ spos,
                                                        float4* __restrict__ list, const uint32_t* __restrict__ rank) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    if (rank) {                        // pruned lists: the survivors of a cell, in order
        const uint32_t r = rank[e];
        if (r == 0xFFFFFFFFu) return;
        const uint32_t c = cidx[e] + cflag[e] - 1u;
        const uint32_t pt = vals[e];
        const float4 p = spos[pt];
        list[(size_t)list_off[c] + r] = make_float4(p.x, p.y, p.z, __int_as_float((int)pt));
        return;
    }
    // cidx = exclusive scan of the cell-start flags: the cells that start strictly before e; the own cell is that
    // many if e opens it, one less otherwise
    const uint32_t c = cidx[e] + cflag[e] - 1u;
    const uint32_t pt = vals[e];
    const float4 p = spos[pt];
    list[(size_t)list_off[c] + (e - cell_first[c])] = make_float4(p.x, p.y, p.z, __int_as_float((int)pt));
}

// dense scenes: chunk_r[j] = (minimum exact distance to the cell centre over chunks >= j), rounded down
__global__ __launch_bounds__(256) void chunk_bounds_kernel(GridGeom G, const uint32_t* __restrict__ cell_first, const uint64_t* __restrict__ cell_key,
                                                           const uint32_t* __restrict__ list_off, uint32_t n_cells, uint32_t n_inc,
                                                           const float4* __restrict__ list, float* __restrict__ chunk_r) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cells) return;
    const uint32_t cnt = (c + 1 < n_cells ? cell_first[c + 1] : n_inc) - cell_first[c];
    const uint64_t key = cell_key[c];
    const uint64_t brick = key >> 9;
    const uint32_t local = (uint32_t)(key & 511);
    const int bx = (int)(brick % (uint64_t)G.nbx), by = (int)((brick / (uint64_t)G.nbx) % (uint64_t)G.nby),
              bz = (int)(brick / ((uint64_t)G.nbx * (uint64_t)G.nby));
    const int cx = bx * 8 + (int)(local & 7), cy = by * 8 + (int)((local >> 3) & 7), cz = bz * 8 + (int)(local >> 6);
    const double ccx = G.of[0] + (cx + 0.5) * G.h, ccy = G.of[1] + (cy + 0.5) * G.h, ccz = G.of[2] + (cz + 0.5) * G.h;
    const uint32_t o = list_off[c];
    double run = 1e300;
    for (int k = (int)cnt - 1; k >= 0; --k) {
        const float4 e = list[(size_t)o + k];
        const double dx = e.x - ccx, dy = e.y - ccy, dz = e.z - ccz;
        run = fmin(run, sqrt(dx * dx + dy * dy + dz * dz));
        if ((k & 7) == 0) chunk_r[(o + (uint32_t)k) >> 3] = (float)(run - (2e-6 + 2.5e-7 * run));   // below the exact value also after the conversion to float, at any coordinate scale
    }
}

// dense scenes with cell edges below epsilon (the sub-cell masks are all ones there): the z word of a cell takes a lower bound of
// the distance from the cell centre to its nearest listed point (= the bound of the list's first chunk).  A query at distance t
// from the centre has no neighbour within epsilon when bound - t > epsilon, and the scan kernel then never touches the list.
__global__ __launch_bounds__(256) void cell_nearest_kernel(const uint64_t* __restrict__ cell_key, const uint32_t* __restrict__ cell_brick, const uint32_t* __restrict__ list_off,
                                                           uint32_t n_cells, const float* __restrict__ chunk_r, uint4* __restrict__ cells) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cells) return;
    cells[(size_t)cell_brick[c] * 512 + (uint32_t)(cell_key[c] & 511)].z = __float_as_uint(chunk_r[list_off[c] >> 3]);
}


// ---------------------------------------------------------------------------------------------
// Dominance pruning of the candidate lists (round 5).  A cell's list holds every scene point within r of the cell box, so that ONE
// list answers the radius-epsilon nearest-neighbour query of any position in the cell; but most of those points can never be the
// ANSWER for a position in this cell.  For two listed points p, p' the difference of the squared distances from a position q is
// linear in q,
//     f(q) = |q - p|^2 - |q - p'|^2 = |u|^2 - |u'|^2 - 2 s . (u - u'),      u = p - centre, u' = p' - centre, s = q - centre,
// so over the (slightly widened) cell box |s_k| <= hh its minimum is |u|^2 - |u'|^2 - 2 hh |u - u'|_1.  When that minimum exceeds a
// margin that covers the scan kernels' float evaluation of both squared distances, p' is strictly nearer than p for EVERY position
// the kernels can assign to this cell: p never wins there -- not on distance, not on a tie -- and is dropped from the list.  The
// nearest neighbour of every query, its index and the tie rule are unchanged (whoever wins a query is by definition not dominated);
// the kd-tree of the reference (kdtree.h:394-459) returns that same point.  Dominators tried per entry: the PRUNE_K listed points
// nearest to the cell centre (any listed point may serve; these prune best).  On a surface sampled every 1.5 mm with cells of
// 1.25 mm the lists shrink from ~45 entries to ~5 whatever the cell's height above the surface: one 128-byte line answers a query,
// where the centre-sorted lists with early exit of rounds 2-4 read 15-20 entries in a dependent line -> bound -> line chain.
// One wavefront per cell; double arithmetic relative to the cell centre (float positions are exact in double).
// ---------------------------------------------------------------------------------------------
// GS lanes per cell (64, or 16 on sparse scenes whose lists hold a handful of points: four cells per wavefront); a list longer than GS is
// walked GS entries at a time, its first GS entries stay in registers for the selection rounds.
template <int PRUNE_K, int GS>
__global__ __launch_bounds__(256) void prune_kernel(GridGeom G, double hh, double margin, const uint32_t* __restrict__ cell_first, const uint64_t* __restrict__ cell_key,
                                                    uint32_t n_cells, uint32_t n_inc, const uint32_t* __restrict__ vals, const float4* __restrict__ spos,
                                                    uint32_t* __restrict__ rank, uint32_t* __restrict__ kept, float* __restrict__ nearest) {
    const uint32_t c = blockIdx.x * (256u / GS) + (threadIdx.x / GS);
    const int lane = threadIdx.x & (GS - 1), wlane = threadIdx.x & 63;
    const bool cell_ok = c < n_cells;                             // (a wavefront of 16-lane groups may hold cells beyond the end: they idle through the ballots)
    const uint32_t first = cell_ok ? cell_first[c] : 0u;
    const uint32_t cnt = cell_ok ? (c + 1 < n_cells ? cell_first[c + 1] : n_inc) - first : 0u;
    const uint64_t key = cell_ok ? cell_key[c] : 0ull;
    const uint64_t brick = key >> 9;
    const uint32_t local = (uint32_t)(key & 511);
    const int bx = (int)(brick % (uint64_t)G.nbx), by = (int)((brick / (uint64_t)G.nbx) % (uint64_t)G.nby), bz = (int)(brick / ((uint64_t)G.nbx * (uint64_t)G.nby));
    const int cx = bx * 8 + (int)(local & 7), cy = by * 8 + (int)((local >> 3) & 7), cz = bz * 8 + (int)(local >> 6);
    const double ccx = G.of[0] + (cx + 0.5) * G.h, ccy = G.of[1] + (cy + 0.5) * G.h, ccz = G.of[2] + (cz + 0.5) * G.h;
    // the group's first GS entries, one per lane
    double ux0 = 0, uy0 = 0, uz0 = 0, n20 = 0;
    if ((uint32_t)lane < cnt) {
        const float4 pf = spos[vals[first + (uint32_t)lane]];
        ux0 = (double)pf.x - ccx; uy0 = (double)pf.y - ccy; uz0 = (double)pf.z - ccz;
        n20 = ux0 * ux0 + uy0 * uy0 + uz0 * uz0;
    }
    // ---- the PRUNE_K entries nearest to the centre: PRUNE_K rounds of "smallest (distance, position) key above the last one" ----
    double dux[PRUNE_K], duy[PRUNE_K], duz[PRUNE_K], dn2[PRUNE_K];
    unsigned long long last = 0ull;
    int nd = 0;
    uint32_t cnt_max = cnt;                                       // (uniform over the wavefront: the loops below run for the longest list of its groups)
    if (GS < 64) for (int off = GS; off < 64; off <<= 1) cnt_max = max(cnt_max, (uint32_t)__shfl_xor((int)cnt_max, off, 64));
#pragma unroll
    for (int j = 0; j < PRUNE_K; ++j) {
        if ((uint32_t)j >= cnt_max) break;
        unsigned long long best = ~0ull;
        if ((uint32_t)lane < cnt) {
            const unsigned long long kk = ((unsigned long long)__float_as_uint((float)n20) << 32) | (unsigned long long)(lane + 1);
            if (kk > last) best = kk;
        }
        for (uint32_t k = (uint32_t)lane + GS; k < cnt; k += GS) {
            const float4 pf = spos[vals[first + k]];
            const double ux = (double)pf.x - ccx, uy = (double)pf.y - ccy, uz = (double)pf.z - ccz;
            const float d2 = (float)(ux * ux + uy * uy + uz * uz);        // (selection only: any listed point is a valid dominator)
            const unsigned long long kk = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(k + 1u);
            if (kk > last && kk < best) best = kk;
        }
        for (int off = GS / 2; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(best, off, GS); best = o < best ? o : best; }
        if (best == ~0ull) continue;                              // this group's list is exhausted (another group's may not be)
        last = best;
        const uint32_t kb = (uint32_t)(best & 0xFFFFFFFFull) - 1u;
        double vx, vy, vz;
        if (kb < (uint32_t)GS) {                                  // held by a lane of the group
            vx = __shfl(ux0, (int)kb, GS); vy = __shfl(uy0, (int)kb, GS); vz = __shfl(uz0, (int)kb, GS);
        } else {
            const float4 pf = spos[vals[first + kb]];             // (the same address in every lane of the group)
            vx = (double)pf.x - ccx; vy = (double)pf.y - ccy; vz = (double)pf.z - ccz;
        }
        dux[j] = vx; duy[j] = vy; duz[j] = vz;
        dn2[j] = vx * vx + vy * vy + vz * vz;
        nd = j + 1;
    }
    // ---- every entry against the dominators ----
    uint32_t base = 0;
    for (uint32_t k0 = 0; k0 < cnt_max; k0 += GS) {
        const uint32_t k = k0 + (uint32_t)lane;
        bool keep = false;
        if (k < cnt) {
            double ux = ux0, uy = uy0, uz = uz0, n2 = n20;
            if (k0) {
                const float4 pf = spos[vals[first + k]];
                ux = (double)pf.x - ccx; uy = (double)pf.y - ccy; uz = (double)pf.z - ccz;
                n2 = ux * ux + uy * uy + uz * uz;
            }
            keep = true;
#pragma unroll
            for (int j = 0; j < PRUNE_K; ++j) {
                if (j < nd) {
                    const double fmin_ = (n2 - dn2[j]) - 2.0 * hh * (fabs(ux - dux[j]) + fabs(uy - duy[j]) + fabs(uz - duz[j]));
                    if (fmin_ > margin) keep = false;      // (an entry is never its own dominator: f is 0 there)
                }
            }
        }
        unsigned long long m = __ballot(keep);
        if (GS < 64) m = (m >> (wlane & ~(GS - 1))) & ((1ull << GS) - 1ull);      // the group's own lanes
        if (k < cnt) rank[first + k] = keep ? base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) : 0xFFFFFFFFu;
        base += (uint32_t)__popcll(m);
    }
    if (lane == 0 && cell_ok) {
        kept[c] = base;
        // lower bound of |centre - nearest listed point| (the nearest is never dominated), below the exact value also as a float
        const double d0 = nd ? sqrt(dn2[0]) : 0.0;
        nearest[c] = (float)fmax(d0 - (2e-6 + 2.5e-7 * d0), 0.0);
    }
}

// block != 0 (octant lines, below): a cell that keeps more than one line of entries reserves `block` entries behind its padded list;
// oct[0] counts those cells
__global__ __launch_bounds__(256) void cell_padded_kept_kernel(const uint32_t* __restrict__ kept, uint32_t n_cells, uint32_t pad, uint32_t* __restrict__ padded,
                                                               uint32_t* __restrict__ max_count, unsigned long long* __restrict__ total, uint32_t block,
                                                               uint32_t* __restrict__ oct) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cells) return;
    const uint32_t cnt = kept[c];
    const bool is_long = block && cnt > STOCS_OCTANT_LINE;
    padded[c] = ((cnt + pad - 1u) & ~(pad - 1u)) + (is_long ? block : 0u);
    if (is_long) atomicAdd(&oct[0], 1u);
    atomicMax(max_count, cnt);
    unsigned long long t = cnt;
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(total, t);
}

// ---------------------------------------------------------------------------------------------
// Octant lines (octant_lists.h; sparse pruned grids at cell edge epsilon with a flat table).  Behind the plain list of every cell that
// keeps more than 8 entries, cell_padded_kept_kernel reserved 64 entries: eight lines, one per octant of the cell.  One thread per
// (cell, octant) -- eight neighbouring lanes per cell -- prunes the cell's STORED list over its octant box and writes the line; when
// all eight octants fit their lines the cell's word in the FLAT table takes the block's offset under the flag and the count 8.  The brick table and
// the plain list are not touched: every other reader works as before.  oct[1] counts the flagged cells, oct[2] their octants' entries.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void octant_lines_kernel(GridGeom G, double hw, double margin, const uint64_t* __restrict__ cell_key,
                                                           const uint32_t* __restrict__ list_off, const uint32_t* __restrict__ kept, uint32_t n_cells,
                                                           float4* __restrict__ list, uint4* __restrict__ flat, uint32_t* __restrict__ oct) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = t >> 3, o = t & 7u;
    const uint32_t cnt = c < n_cells ? kept[c] : 0u;
    uint32_t n = 0, block_off = 0;
    size_t fidx = 0;
    bool in_flat = false;
    if (cnt > STOCS_OCTANT_LINE) {
        const uint64_t key = cell_key[c];
        const uint64_t brick = key >> 9;
        const uint32_t local = (uint32_t)(key & 511);
        const int bx = (int)(brick % (uint64_t)G.nbx), by = (int)((brick / (uint64_t)G.nbx) % (uint64_t)G.nby), bz = (int)(brick / ((uint64_t)G.nbx * (uint64_t)G.nby));
        const int cx = bx * 8 + (int)(local & 7), cy = by * 8 + (int)((local >> 3) & 7), cz = bz * 8 + (int)(local >> 6);
        in_flat = cx < G.n[0] && cy < G.n[1] && cz < G.n[2];
        fidx = ((size_t)cz * G.n[1] + cy) * G.n[0] + cx;
        const double ctr[3] = {G.of[0] + (cx + 0.25 + 0.5 * (double)(o & 1u)) * G.h, G.of[1] + (cy + 0.25 + 0.5 * (double)((o >> 1) & 1u)) * G.h,
                               G.of[2] + (cz + 0.25 + 0.5 * (double)(o >> 2)) * G.h};
        const uint32_t lo = list_off[c];
        block_off = lo + ((cnt + 7u) & ~7u);      // (the cell's padded size is this plus the block: cell_padded_kept_kernel)
        n = octant_line_build(list + lo, cnt, ctr, 0.25 * G.h, hw, G.r, margin, list + block_off + octant_line_start_of_octant(o));
    }
    // the eight lanes of a cell agree: every octant fits its line (an empty one keeps the sentinel fill; no mask bit leads there)
    const unsigned long long over = __ballot(n > STOCS_OCTANT_LINE);
    const int lane = threadIdx.x & 63;
    const bool fits = cnt > STOCS_OCTANT_LINE && in_flat && ((over >> (lane & ~7)) & 0xFFull) == 0ull;
    if (fits) {
        atomicAdd(&oct[2], n);
        if (o == 0) {   // the block under the flag, and the length of a line for the count (the cone above it stays)
            flat[fidx].x = octant_word_pack(block_off);
            flat[fidx].y = (flat[fidx].y & ~STOCS_CONE_COUNT_MASK) | STOCS_OCTANT_LINE;
            atomicAdd(&oct[1], 1u);
        }
    }
}

__global__ __launch_bounds__(256) void cell_nearest_store_kernel(const uint64_t* __restrict__ cell_key, const uint32_t* __restrict__ cell_brick, uint32_t n_cells,
                                                                 const float* __restrict__ nearest, uint4* __restrict__ cells) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cells) return;
    cells[(size_t)cell_brick[c] * 512 + (uint32_t)(cell_key[c] & 511)].z = __float_as_uint(nearest[c]);
}

// ---------------------------------------------------------------------------------------------
// The build, host side.  Which grid comes out is the GridForm (grid_form, ctx.hip) plus the four predicates here, which need a count
// of the build; build_grid_gpu runs the stages of `Build` in order, with a read-back wherever the next one sizes its buffers by a count.
// ---------------------------------------------------------------------------------------------
static inline unsigned grid_of(size_t n) { return (unsigned)((n + 255) / 256); }

// keys of at most 32 bits (every sparse scene: ~21 bits of cell) and a frame's worth of incidences: the library's own onesweep (sort32.hip,
// one launch per 8-bit pass) where rocPRIM's 64-bit radix_sort_pairs runs ~17 small launches (150 us of a frame's stocs_ctx_set_scene in
// round 5a); both stable
static bool own_sort_pays(const GridForm& f, size_t n_inc, unsigned end_bit) { return sort_own_wanted(n_inc, f.own_sort) && end_bit <= 32 && n_inc < ((size_t)1 << 30); }
// a handful of points per cell: 16 lanes per cell, four cells per wavefront; else a wavefront per cell
static int prune_group(size_t n_inc, uint32_t n_cells) { return (double)n_inc <= 12.0 * (double)n_cells ? 16 : 64; }
// the flat copy of the cell words (one look-up per query instead of two dependent ones) while the table stays within 512 MB
static bool flat_fits(const GridForm& f, const GridBox& B) { return f.flat && (size_t)B.n[0] * B.n[1] * B.n[2] * sizeof(uint4) <= ((size_t)512 << 20); }
// octant lines behind the long lists of a pruned grid with a flat table (octant_lists.h).  On by default although the step's drop at Cm
// (2 to 2.9 %, the faster build in all 30 alternations) cleared three times the run-to-run range in one visit of three only: the line
// select in the FLAT forms costs a grid WITHOUT lines 1.4 % against the parent (five alternations, slower in each), so off is the
// slower default, not the neutral one.  At most n_inc / 9 cells are long: below 2^24 incidences their blocks stay far
// below the 2^31 entries an offset can address
static bool octants_fit(const GridForm& f, bool flat, size_t n_inc) { return f.octants && flat && n_inc < ((size_t)1 << 24); }

typedef void (*PruneKernel)(GridGeom, double, double, const uint32_t*, const uint64_t*, uint32_t, uint32_t, const uint32_t*, const float4*, uint32_t*, uint32_t*, float*);
static PruneKernel prune_kernel_for(int k, int group) {
    if (group == 16) return k == 4 ? prune_kernel<4, 16> : k == 16 ? prune_kernel<16, 16> : prune_kernel<8, 16>;
    return k == 4 ? prune_kernel<4, 64> : k == 16 ? prune_kernel<16, 64> : prune_kernel<8, 64>;
}

static GridGeom device_geom(const GridBox& B, bool centre_sorted) {
    GridGeom G;
    for (int k = 0; k < 3; ++k) { G.of[k] = B.of[k]; G.n[k] = B.n[k]; }   // the FLOAT origin of the scan kernels' floor((q - o_f) * inv_h), widened
    G.h = B.h; G.r = B.r; G.nbx = B.nb[0]; G.nby = B.nb[1];
    G.dense = centre_sorted ? 1 : 0; G.qscale = B.qscale;
    return G;
}

static PinGrid* pin_grid(stocs_ctx* c) { return (PinGrid*)((char*)c->h_pin + PIN_GRID); }

struct Build {   // one build in flight
    stocs_ctx* c;
    const GridForm& form;
    SceneGrid& g;
    GridStages& S;        // = g.stages
    PinGrid* pin;         // the read-backs (a copy into a pageable stack word would take the runtime's staging path)
    GridGeom G;
    hipStream_t st;
    bool flat, octants;   // decided once the incidences are counted

    // temporaries: the context's workspace arena (no hipMalloc / hipFree in steady state)
    template <class T> int tmp(T** p, size_t n) { return c->grid_ws.take(std::max<size_t>(n, 1) * sizeof(T), (void**)p); }
    template <class K, class... A> void run(K kernel, size_t threads, A... a) { hipLaunchKernelGGL(kernel, dim3(grid_of(threads)), dim3(256), 0, st, a...); }
    template <class T> int read_back(T* pinned, const T* dev, int n = 1) { STOCS_HIP_CHECK(hipMemcpyAsync(pinned, dev, n * sizeof(T), hipMemcpyDeviceToHost, st)); return STOCS_OK; }

    // out[0 .. n] = the exclusive prefix sums of in[0 .. n): out[n] is the total.  The scan runs over n + 1 words, and in[n] -- read, but
    // part of no output -- needs no value.  *t == NULL: the temporary is sized for this call and taken; later calls of at most this size reuse it
    template <class In, class Out> int scan_total(char** t, size_t* bytes, const In* in, Out* out, size_t n) {
        if (!*t) {
            STOCS_HIP_CHECK(exclusive_scan(NULL, *bytes, in, out, n + 1, st));
            if (int rc = tmp(t, *bytes)) return rc;
        }
        STOCS_HIP_CHECK(exclusive_scan(*t, *bytes, in, out, n + 1, st));
        return STOCS_OK;
    }

    // Stable sort of the S.n_inc (key, point) pairs by the low end_bit bits into S.keys / S.vals.  own: the keys lie as 32-bit words in the
    // first half of `keys` (the unsorted 64-bit array is not needed), are sorted into its second half and widened into S.keys for the
    // kernels behind, and S.sort_err points at the sort's error word
    int sort_pairs_take(bool own, uint64_t* keys, const uint32_t* vals, unsigned end_bit) {
        const size_t n = S.n_inc;
        size_t bytes = 0;
        char* t;
        int rc;
        if (!own) {
            STOCS_HIP_CHECK(sort_pairs(NULL, bytes, keys, S.keys, vals, S.vals, n, 0, end_bit, st));
            if ((rc = tmp(&t, bytes))) return rc;
            STOCS_HIP_CHECK(sort_pairs(t, bytes, keys, S.keys, vals, S.vals, n, 0, end_bit, st));
            return STOCS_OK;
        }
        uint32_t *k32 = (uint32_t*)keys, *k32s = k32 + n;
        STOCS_HIP_CHECK(sort_pairs_own(NULL, bytes, k32, k32s, vals, S.vals, n, 0, end_bit, NULL, 1, st));
        if ((rc = tmp(&t, bytes))) return rc;
        STOCS_HIP_CHECK(sort_pairs_own(t, bytes, k32, k32s, vals, S.vals, n, 0, end_bit, NULL, 1, st));
        run(widen_keys_kernel, n, k32s, n, S.keys);
        S.sort_err = (const uint32_t*)(t + sort_own_err_offset());
        return STOCS_OK;
    }

    // 1. incidences: per scene point the number of cells within r of it and, by prefix sums, its first incidence; the total is read back
    int count() {
        const int nS = c->nS;
        uint32_t* d_cnt;
        char* t = NULL;
        size_t bytes = 0;
        int rc;
        if ((rc = tmp(&d_cnt, (size_t)nS + 1)) || (rc = tmp(&S.off, (size_t)nS + 1))) return rc;
        run(incidence_kernel<false>, nS, G, c->d_spos, nS, d_cnt, (const unsigned long long*)NULL, (uint64_t*)NULL, (uint32_t*)NULL, (uint32_t*)NULL);
        if ((rc = scan_total(&t, &bytes, d_cnt, S.off, (size_t)nS))) return rc;
        return read_back(&pin->n_inc, S.off + nS);
    }

    // 2. sort: the (key, point) records of every point, sorted stably by cell (and quantised centre distance)
    int sort() {
        const int nS = c->nS;
        uint64_t* d_keys;
        uint32_t* d_vals;
        int rc;
        if ((rc = tmp(&d_keys, S.n_inc)) || (rc = tmp(&S.keys, S.n_inc)) || (rc = tmp(&d_vals, S.n_inc)) || (rc = tmp(&S.vals, S.n_inc))) return rc;
        const unsigned end_bit = (unsigned)std::min(64, S.box.cell_bits + form.qbits);
        const bool own = own_sort_pays(form, S.n_inc, end_bit);
        g.sort_kind = own ? STOCS_GRID_SORT_OWN : STOCS_GRID_SORT_ROCPRIM;
        run(incidence_kernel<true>, nS, G, c->d_spos, nS, (uint32_t*)NULL, S.off, own ? (uint64_t*)NULL : d_keys, d_vals, own ? (uint32_t*)d_keys : (uint32_t*)NULL);
        STOCS_HIP_CHECK(hipGetLastError());
        return sort_pairs_take(own, d_keys, d_vals, end_bit);
    }

    // 3. cells and bricks: the incidences that open a cell / a brick, their ordinals by prefix sums; both totals and the sort's error
    // word are read back
    int cells() {
        const size_t n = S.n_inc;
        int rc;
        if ((rc = tmp(&S.cflag, n + 1)) || (rc = tmp(&S.bflag, n + 1)) || (rc = tmp(&S.cidx, n + 1)) || (rc = tmp(&S.bidx, n + 1))) return rc;
        run(cell_flags_kernel, n, S.keys, n, form.qbits, S.cflag, S.bflag);
        if ((rc = scan_total(&S.scan_tmp, &S.scan_bytes, S.cflag, S.cidx, n)) || (rc = scan_total(&S.scan_tmp, &S.scan_bytes, S.bflag, S.bidx, n))) return rc;
        if ((rc = read_back(&pin->n_cells, S.cidx + n)) || (rc = read_back(&pin->n_bricks, S.bidx + n))) return rc;
        return S.sort_err ? read_back(&pin->sort_err, S.sort_err) : STOCS_OK;
    }

    // 4. list layout: per non-empty cell its first incidence, key and brick; pruned lists: every entry's place among its cell's survivors;
    // then the padded list lengths (whole 128-byte lines; behind a long pruned list its octant block) and, by prefix sums, the list
    // offsets.  The list entries, the longest list and the kept entries are read back
    int layout() {
        const uint32_t n_cells = S.n_cells, n_inc = (uint32_t)S.n_inc;
        const size_t nc1 = (size_t)n_cells + 1;
        int rc;
        if ((rc = tmp(&S.cell_first, nc1)) || (rc = tmp(&S.cell_brick, nc1)) || (rc = tmp(&S.padded, nc1)) || (rc = tmp(&S.list_off, nc1)) || (rc = tmp(&S.cell_key, nc1)) ||
            (rc = tmp(&S.counters, GridStages::COUNTER_WORDS)))
            return rc;
        run(cell_records_kernel, n_inc, S.keys, S.n_inc, form.qbits, S.cflag, S.cidx, S.bflag, S.bidx, S.cell_first, S.cell_key, S.cell_brick);
        run(fill_i32_kernel, GridStages::COUNTER_WORDS, (int32_t*)S.counters, (size_t)GridStages::COUNTER_WORDS, 0);
        if (form.layout == GRID_PRUNED) {
            if ((rc = tmp(&S.rank, S.n_inc + 1)) || (rc = tmp(&S.kept, nc1)) || (rc = tmp(&S.nearest, nc1))) return rc;
            g.prune_group = prune_group(S.n_inc, n_cells);
            g.prune_k = form.prune_k;
            run(prune_kernel_for(g.prune_k, g.prune_group), (size_t)n_cells * g.prune_group, G, S.box.hh, S.box.margin, S.cell_first, S.cell_key, n_cells, n_inc, S.vals,
                c->d_spos, S.rank, S.kept, S.nearest);
            run(cell_padded_kept_kernel, n_cells, S.kept, n_cells, 8u, S.padded, S.longest(), S.total(), octants ? STOCS_OCTANT_BLOCK : 0u, S.oct());
        } else
            run(cell_padded_kernel, n_cells, S.cell_first, n_cells, n_inc, 8u, S.padded, S.longest());
        if ((rc = scan_total(&S.scan_tmp, &S.scan_bytes, S.padded, S.list_off, (size_t)n_cells))) return rc;
        if ((rc = read_back(&pin->n_list, S.list_off + n_cells)) || (rc = read_back(&pin->longest, S.longest()))) return rc;
        return form.layout == GRID_PRUNED ? read_back(&pin->n_kept, S.total()) : STOCS_OK;
    }

    // 5. cell words and lists: the grid itself, in c->grid_mem -- cell words (offset, count | cone, sub-cell mask) in their bricks and in
    // the flat table, the top-level brick table, the sentinel-filled lists
    int lists() {
        const uint32_t n_cells = S.n_cells;
        const size_t n_words = (size_t)S.n_bricks * 512, n_list = std::max<size_t>(S.n_list, 8), n_flat = (size_t)S.box.n[0] * S.box.n[1] * S.box.n[2];
        int rc;
        g.has_cones = form.cones;
        if ((rc = c->grid_mem.take(std::max<size_t>(n_words, 1) * sizeof(uint4), (void**)&g.d_cells)) || (rc = c->grid_mem.take(n_list * sizeof(float4), (void**)&g.d_list))) return rc;
        run(zero_cells_kernel, n_words, g.d_cells, n_words);
        if (flat) {
            if ((rc = c->grid_mem.take(n_flat * sizeof(uint4), (void**)&g.d_flat))) return rc;
            run(zero_cells_kernel, n_flat, g.d_flat, n_flat);
        }
        run(fill_list_kernel, n_list, g.d_list, n_list);
        run(cell_words_kernel, (size_t)n_cells * 64, G, form.div, S.cell_first, S.cell_key, S.cell_brick, S.list_off, n_cells, (uint32_t)S.n_inc, S.vals, c->d_spos, g.d_top,
            g.d_cells, g.d_flat, S.kept, S.rank, c->d_snrmw, g.has_cones ? 1 : 0);
        run(list_fill_kernel, S.n_inc, S.cflag, S.cidx, S.cell_first, S.list_off, S.vals, S.n_inc, c->d_spos, g.d_list, S.rank);
        STOCS_HIP_CHECK(hipGetLastError());
        if (octants) {
            // The lines themselves are written later, by build_octant_lines, once the scene has been scored often enough for them to pay
            // (lcp.hip; the threshold of the distance field): the build only reserved their blocks and counts the long cells.  What that
            // call needs stays in g.stages until the next build resets the workspace
            if ((rc = read_back(&pin->n_long_cells, S.oct()))) return rc;   // lands with the build's last synchronisation
            g.oct_pending = true;
        }
        if (form.layout == GRID_PRUNED && form.div > 1) {   // no sub-cell masks on grids finer than epsilon: the z word takes the distance bound (has_nearest)
            run(cell_nearest_store_kernel, n_cells, S.cell_key, S.cell_brick, n_cells, S.nearest, g.d_cells);
            g.has_nearest = true;
        }
        return STOCS_OK;
    }

    // 6. dense chunk bounds (centre-sorted lists): per 8-entry chunk a lower bound of the distance to the cell centre; on grids finer
    // than epsilon the z word of a cell takes the bound of its first chunk
    int chunk_bounds() {
        const size_t n_chunks = S.n_list / 8;
        if (int rc = c->grid_mem.take(std::max<size_t>(n_chunks, 1) * sizeof(float), (void**)&g.d_chunk_r)) return rc;
        run(fill_i32_kernel, n_chunks, (int32_t*)g.d_chunk_r, n_chunks, 0);
        run(chunk_bounds_kernel, S.n_cells, G, S.cell_first, S.cell_key, S.list_off, S.n_cells, (uint32_t)S.n_inc, g.d_list, g.d_chunk_r);
        g.has_nearest = form.div > 1;
        if (g.has_nearest) run(cell_nearest_kernel, S.n_cells, S.cell_key, S.cell_brick, S.list_off, S.n_cells, g.d_chunk_r, g.d_cells);
        STOCS_HIP_CHECK(hipGetLastError());
        return STOCS_OK;
    }
};

int build_grid_gpu(stocs_ctx* c, const GridForm& form) {
    SceneGrid& g = c->grid;
    const int nS = c->nS;
    hipStream_t st = c->stream;
    int rc;
    reset_grid(g);
    double mn[3] = {1e30, 1e30, 1e30}, mx[3] = {-1e30, -1e30, -1e30};
    for (int i = 0; i < nS; ++i) {
        const V3 p = c->h_spos[i];
        const double v[3] = {p.x, p.y, p.z};
        for (int k = 0; k < 3; ++k) { mn[k] = std::min(mn[k], v[k]); mx[k] = std::max(mx[k], v[k]); }
    }
    for (int k = 0; k < 3; ++k) { g.bb_mn[k] = nS ? mn[k] : 0.0; g.bb_mx[k] = nS ? mx[k] : 0.0; }
    GridStages& S = g.stages;
    const GridBox& B = S.box = grid_geometry(g.bb_mn, g.bb_mx, (double)c->prm.distance_threshold, form.div);
    g.ox = B.of[0]; g.oy = B.of[1]; g.oz = B.of[2];
    g.h = B.hf; g.inv_h = B.inv_h; g.div = form.div;
    g.nx = B.n[0]; g.ny = B.n[1]; g.nz = B.n[2];
    g.nbx = B.nb[0]; g.nby = B.nb[1]; g.nbz = B.nb[2];
    if (B.n_top > (int64_t)STOCS_GRID_MAX_BRICKS) { set_error("scene extent too large for the brick grid"); return STOCS_ERR_INVALID; }

    STOCS_HIP_CHECK(hipStreamSynchronize(st));   // the previous grid and the previous build's temporaries are recycled
    if ((rc = c->grid_ws.reset()) || (rc = c->grid_mem.reset()) || (rc = ensure_pinned(c, PIN_VAR))) return rc;
    Build b = {c, form, g, S, pin_grid(c), device_geom(B, form.layout == GRID_CENTRE_SORTED), st, false, false};
    PinGrid& pin = *b.pin = PinGrid();
    if ((rc = c->grid_mem.take((size_t)std::max<int64_t>(B.n_top, 1) * 4, (void**)&g.d_top))) return rc;
    b.run(fill_i32_kernel, (size_t)B.n_top, g.d_top, (size_t)B.n_top, -1);
    if (nS == 0) {
        if ((rc = c->grid_mem.take(16, (void**)&g.d_cells)) || (rc = c->grid_mem.take(8 * 16, (void**)&g.d_list))) return rc;
        STOCS_HIP_CHECK(hipStreamSynchronize(st));
        return STOCS_OK;
    }
    if ((rc = b.count())) return rc;
    STOCS_HIP_CHECK(hipStreamSynchronize(st));
    // padded lists stay below 2^31 entries (32-bit offsets in the cell words)
    if (pin.n_inc >= (1ull << 28)) { set_error("scene grid lists too large (%llu incidences)", pin.n_inc); return STOCS_ERR_INVALID; }
    S.n_inc = (size_t)pin.n_inc;
    g.n_inc = (int64_t)pin.n_inc;
    b.flat = flat_fits(form, B);
    b.octants = octants_fit(form, b.flat, S.n_inc);
    if ((rc = b.sort()) || (rc = b.cells())) return rc;
    STOCS_HIP_CHECK(hipStreamSynchronize(st));
    if (pin.sort_err) { set_error("scene grid: the incidence sort gave up waiting for a tile (sort32.hip)"); return STOCS_ERR_HIP; }
    S.n_cells = pin.n_cells; S.n_bricks = pin.n_bricks;
    g.n_cells = (int64_t)S.n_cells;
    if ((rc = b.layout())) return rc;
    STOCS_HIP_CHECK(hipStreamSynchronize(st));
    S.n_list = pin.n_list;
    g.longest_list = (int)pin.longest;
    if (pin.longest > 65535u) { set_error("more than 65535 scene points within epsilon of one grid cell"); return STOCS_ERR_INVALID; }
    if ((rc = b.lists()) || (form.layout == GRID_CENTRE_SORTED && (rc = b.chunk_bounds()))) return rc;
    STOCS_HIP_CHECK(hipStreamSynchronize(st));
    g.n_bricks = (int)S.n_bricks;
    // the plain lists only: the octant blocks are not part of what the launch layer weighs (lcp.hip: lists_spill, lists_huge)
    g.n_long_cells = (int64_t)pin.n_long_cells;
    g.n_entries = (int64_t)S.n_list - (int64_t)STOCS_OCTANT_BLOCK * g.n_long_cells;
    g.pruned = form.layout == GRID_PRUNED;
    g.avg_list_len = S.n_cells ? (double)(g.pruned ? pin.n_kept : pin.n_inc) / (double)S.n_cells : 0.0;
    g.avg_dilated_len = S.n_cells ? (double)S.n_inc / (double)S.n_cells : 0.0;
    return STOCS_OK;
}

// The octant lines of the current grid (octant_lines_kernel), on the context's stream, once per scene; no-op when the grid has none
// to build.  Called by the scoring launch that takes the scene's work past the threshold: one kernel over the long cells (0.05 ms
// at Cm or on a camera frame, as much as a launch of 8 000 candidates takes there -- a frame that is scored once never pays it) and
// one synchronisation for the two counts of stocs_get_grid_octants.
int build_octant_lines(stocs_ctx* c) {
    SceneGrid& g = c->grid;
    const GridStages& S = g.stages;
    if (!g.oct_pending) return STOCS_OK;
    g.oct_pending = false;
    if (!g.d_flat || !g.d_list || g.n_long_cells == 0) return STOCS_OK;
    if (int rc = ensure_pinned(c, PIN_VAR)) return rc;
    PinGrid* pin = pin_grid(c);
    pin->n_octant_cells = 0; pin->n_octant_entries = 0;
    // eight lanes per cell; cells with one line of entries leave at once
    hipLaunchKernelGGL(octant_lines_kernel, dim3(grid_of((size_t)S.n_cells * 8)), dim3(256), 0, c->stream, device_geom(S.box, false), S.box.oct_hw, S.box.margin, S.cell_key,
                       S.list_off, S.kept, S.n_cells, g.d_list, g.d_flat, S.oct());
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(hipMemcpyAsync(&pin->n_octant_cells, S.oct() + 1, 8, hipMemcpyDeviceToHost, c->stream));   // (and n_octant_entries behind it)
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    g.n_octant_cells = (int64_t)pin->n_octant_cells; g.n_octant_entries = (int64_t)pin->n_octant_entries;
    return STOCS_OK;
}

// ---------------------------------------------------------------------------------------------
// Distance field for the patch test of the scan kernels (SceneGrid::d_dist).  A 64-point step of the model whose bounding
// sphere, under a candidate transform, is farther than epsilon from every scene point cannot contribute to the score
// (stocs.cpp:1019-1024: a model point only counts with a scene point within epsilon), so the kernel skips it after ONE
// look-up here instead of 64 in the cell table.  Per coarse cell: the distance from the cell's centre to the nearest scene
// point (float, shortened by more than its rounding), capped; a position x in the cell is at least value - |x - centre| from the scene.
// ---------------------------------------------------------------------------------------------
struct CullGeom {
    double o[3], g, cap;
    int n[3], w;
};

__global__ __launch_bounds__(256) void dist_fill_kernel(float* __restrict__ t, size_t n, float v) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) t[i] = v;
}

// One wavefront per scene point: 16 lanes walk an x row of the point's window, the four quarter-waves take four (y, z) rows at a
// time, so that an access touches 4 table lines instead of 64 and a point's set-up is done once.  Float arithmetic with the cell
// centre computed exactly as the scan kernel computes it; the stored value is shortened by more than every rounding on the way.
// Distances are non-negative floats, whose bit patterns order like unsigned integers: an integer atomic minimum, tried only when a
// device-scope read is larger (a plain load may be served by this XCD's L2 with a value other XCDs have lowered long ago).
// 0.23 ms at Cm (20 000 points x 2 197 cells: 44 M visits, 23 M inside the cap) -- and that is the memory-side atomic minima on
// lines that ~20 points fight over at the same time, not the shape of the loop: a thread per (point, row) walking x alone took
// 0.46 ms (64 lines per access), a workgroup per 16 points and row 0.24, this form 0.23, four reads in flight per lane 0.31.
__global__ __launch_bounds__(256) void dist_splat_kernel(CullGeom G, float ox, float oy, float oz, float g, float cap, const float4* __restrict__ spos, int nS,
                                                         uint32_t* __restrict__ t) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nS) return;
    const int lane = threadIdx.x & 63, xo0 = lane & 15, rsub = lane >> 4;
    const int side = 2 * G.w + 1;
    const float4 p = spos[i];
    const float inv_g = 1.0f / g, cap2 = cap * cap;
    const int ix = (int)floorf((p.x - ox) * inv_g), iy0 = (int)floorf((p.y - oy) * inv_g) - G.w, iz0 = (int)floorf((p.z - oz) * inv_g) - G.w;
    for (int r = rsub; r < side * side; r += 4) {
        const int iz = iz0 + r / side, iy = iy0 + r % side;
        if (iy < 0 || iy >= G.n[1] || iz < 0 || iz >= G.n[2]) continue;
        const float dy = p.y - (oy + ((float)iy + 0.5f) * g), dz = p.z - (oz + ((float)iz + 0.5f) * g);
        const float dyz = dy * dy + dz * dz;
        if (dyz >= cap2) continue;
        const size_t row = ((size_t)iz * G.n[1] + iy) * G.n[0];
        for (int xo = xo0; xo < side; xo += 16) {
            const int cx = ix - G.w + xo;
            if (cx < 0 || cx >= G.n[0]) continue;
            const float dx = p.x - (ox + ((float)cx + 0.5f) * g);
            const float d2 = dx * dx + dyz;
            if (d2 >= cap2) continue;
            const float v = fmaxf(sqrtf(d2) * (1.0f - 2.0e-6f) - 1.0e-6f, 0.0f);
            const uint32_t u = __float_as_uint(v);
            if (u < __hip_atomic_load(&t[row + cx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&t[row + cx], u);
        }
    }
}

// Geometry and memory of the field for the current grid, scene box and model (the cap follows the model's patch radii: a
// patch can only be ruled out when field value - half a cell diagonal exceeds its radius + epsilon).  Called at the end of a
// grid build so that filling it later allocates nothing.
int prepare_cull_field(stocs_ctx* c) {
    SceneGrid& g = c->grid;
    g.d_dist = NULL; g.dist_ready = false;
    g.d_ncone = NULL; g.d_nsum = NULL; g.ncone_ready = false; g.pn_rb = g.pn_reach = 0.0f; g.pn_w = 0;
    if (c->nS <= 0 || c->nM < 64 || !c->d_mpatch) return STOCS_OK;
    const double eps = (double)c->prm.distance_threshold;
    if (!(eps > 0)) return STOCS_OK;
    double cg = eps;
    const double cap = std::min((double)c->patch_r_ref, 8.0 * eps) + eps + cg;
    double ext[3];
    int64_t cells = 0;
    for (;;) {   // coarser cells for boxes that would need more than 16 M of them
        cells = 1;
        for (int k = 0; k < 3; ++k) { ext[k] = (g.bb_mx[k] - g.bb_mn[k]) + 2.0 * (cap + cg); cells *= (int64_t)floor(ext[k] / cg) + 1; }
        if (cells <= ((int64_t)16 << 20)) break;
        cg *= 1.25;
    }
    g.cg_g = (float)cg; g.cg_inv_g = (float)(1.0 / (double)g.cg_g);
    g.cg_cap = (float)cap;
    g.cg_ox = (float)(g.bb_mn[0] - cap - cg); g.cg_oy = (float)(g.bb_mn[1] - cap - cg); g.cg_oz = (float)(g.bb_mn[2] - cap - cg);
    const double of[3] = {g.cg_ox, g.cg_oy, g.cg_oz};
    int n[3];
    for (int k = 0; k < 3; ++k) n[k] = (int)floor((g.bb_mx[k] + cap + cg - of[k]) / (double)g.cg_g) + 1;
    g.cg_nx = n[0]; g.cg_ny = n[1]; g.cg_nz = n[2];
    g.cg_w = (int)ceil(cap / (double)g.cg_g);
    // the cone field of the sub-patch normal test (patch_normals.h) over the same cells, for models the shared-list forms of the queue
    // kernel score: one more word per cell right behind the distances, three words per cell of sums for its build.  The reach follows the
    // model's sub-patch radii as the cap follows its patch radii: a sub-patch of radius r at e from a cell's centre needs r + epsilon + e
    const size_t n_cells = (size_t)n[0] * n[1] * n[2];
    // Only where a shared-list form can run at all: the option on as the grid is built, a model of up to 8 192 points that the queue
    // kernel splits (512 points on; dense grids split every model).  lcp_split and lcp_cull_unit can change later: whether a launch
    // runs such a form, and so whether the cones are ever filled, is decided launch by launch (lcp.hip)
    const bool shared_possible = c->lcp_patch_normals && c->nM <= STOCS_PN_MAX_MODEL && (c->nM >= 512 || g.d_chunk_r != NULL);
    if (!shared_possible) return c->grid_mem.take(n_cells * sizeof(float), (void**)&g.d_dist);
    // The radius term is clamped as the cap's is: the fill visits (2 pn_w + 1)^3 cells per scene point, twice, so its cost grows with
    // the cube of the reach, and the cones of a wide reach rule nothing out anyway.  At most STOCS_PN_MAX_REACH_EPS + 1 epsilon + half
    // a cell diagonal: 5.9 cells, four times the visits of Cm's 3.7.  A sub-patch beyond it is "not testable", as the kernel has it
    g.pn_rb = (float)(std::min((double)c->sub_r_ref, STOCS_PN_MAX_REACH_EPS * eps) + eps + 0.5 * sqrt(3.0) * (double)g.cg_g);
    g.pn_reach = pn_reach_for_kernel(g.pn_rb);
    g.pn_w = (int)ceil((double)g.pn_rb / (double)g.cg_g);
    if (int rc = c->grid_mem.take(2 * n_cells * sizeof(float), (void**)&g.d_dist)) return rc;
    g.d_ncone = (uint32_t*)(g.d_dist + n_cells);
    return c->grid_mem.take(3 * n_cells * sizeof(int32_t), (void**)&g.d_nsum);
}

// ---- the cone field (patch_normals.h) ----
// One wavefront per scene point, its window walked as dist_splat_kernel walks it (the cell centres computed as the scan kernel
// computes them); a cell takes part when the point's float distance from its centre is below rb.  Integer atomics only, so the field
// is the same from run to run:
//   PASS 0   the axis sums, fixed point: round(1024 n) per component (a point whose normal is not of unit length within 1e-4 adds nothing)
//   (cone_axis_kernel: per cell, the sums -> the octahedral axis, class 0)
//   PASS 1   the class of the point's normal against the axis AS DECODED (double, rounded outwards), atomic maximum on the word: the
//            low 24 bits of every operand of a cell are the same axis, so the maximum is the maximum of the classes
template <int PASS>
__global__ __launch_bounds__(256) void cone_splat_kernel(CullGeom G, float ox, float oy, float oz, float g, float rb, const float4* __restrict__ spos,
                                                         const float4* __restrict__ snrmw, int nS, int32_t* __restrict__ nsum, uint32_t* __restrict__ ncone) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nS) return;
    const int lane = threadIdx.x & 63, xo0 = lane & 15, rsub = lane >> 4;
    const int side = 2 * G.w + 1;
    const float4 p = spos[i];
    const float4 nf = snrmw[i];
    const double n2 = (double)nf.x * nf.x + (double)nf.y * nf.y + (double)nf.z * nf.z;
    const bool unit = n2 >= 0.99980001 && n2 <= 1.00020001;   // within 1e-4 of unit length (false for a NaN)
    if (PASS == 0 && !unit) return;
    const int kx = unit ? (int)rintf(nf.x * 1024.0f) : 0, ky = unit ? (int)rintf(nf.y * 1024.0f) : 0, kz = unit ? (int)rintf(nf.z * 1024.0f) : 0;
    const float inv_g = 1.0f / g, rb2 = rb * rb;
    if (!(fabsf(p.x) + (fabsf(p.y) + fabsf(p.z)) < 1.0e18f)) return;   // (a position that is not finite is within reach of nothing)
    const int ix = (int)floorf((p.x - ox) * inv_g), iy0 = (int)floorf((p.y - oy) * inv_g) - G.w, iz0 = (int)floorf((p.z - oz) * inv_g) - G.w;
    for (int r = rsub; r < side * side; r += 4) {
        const int iz = iz0 + r / side, iy = iy0 + r % side;
        if (iy < 0 || iy >= G.n[1] || iz < 0 || iz >= G.n[2]) continue;
        const float dy = p.y - (oy + ((float)iy + 0.5f) * g), dz = p.z - (oz + ((float)iz + 0.5f) * g);
        const float dyz = dy * dy + dz * dz;
        if (dyz >= rb2) continue;
        const size_t row = ((size_t)iz * G.n[1] + iy) * G.n[0];
        for (int xo = xo0; xo < side; xo += 16) {
            const int cx = ix - G.w + xo;
            if (cx < 0 || cx >= G.n[0]) continue;
            const float dx = p.x - (ox + ((float)cx + 0.5f) * g);
            if (dx * dx + dyz >= rb2) continue;
            const size_t cell = row + cx;
            if (PASS == 0) {
                atomicAdd(&nsum[3 * cell], kx); atomicAdd(&nsum[3 * cell + 1], ky); atomicAdd(&nsum[3 * cell + 2], kz);
            } else {
                const uint32_t w0 = __hip_atomic_load(&ncone[cell], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                uint32_t cls = STOCS_PN_BAD_CLASS;
                if (unit) {
                    float fx, fy, fz;
                    pn_axis(w0, fx, fy, fz);
                    const double o2 = (double)fx * fx + (double)fy * fy + (double)fz * fz;
                    const double cs = ((double)nf.x * fx + (double)nf.y * fy + (double)nf.z * fz) / sqrt(n2 * o2);
                    if (cs > 0.0) {   // below 90 degrees
                        const double sd = sqrt(fmax((1.0 - cs) * (1.0 + cs), 0.0));
                        cls = (uint32_t)fmin(floor(sd * (double)STOCS_PN_SIN_STEPS + 1.0e-4) + 1.0, (double)STOCS_PN_BAD_CLASS);   // sin(angle) < cls / 256, the double rounding included
                    }
                }
                const uint32_t w1 = (w0 & 0xFFFFFFu) | (cls << 24);
                if (w1 > w0) atomicMax(&ncone[cell], w1);
            }
        }
    }
}

__global__ __launch_bounds__(256) void cone_axis_kernel(const int32_t* __restrict__ nsum, uint32_t* __restrict__ ncone, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double sx = (double)nsum[3 * i], sy = (double)nsum[3 * i + 1], sz = (double)nsum[3 * i + 2];
    const double l1 = fabs(sx) + fabs(sy) + fabs(sz);
    uint32_t w = 0u;   // (no sum: the axis of word 0 is as good as any, the classes are measured against it)
    if (l1 > 0.0) {
        double px = sx / l1, py = sy / l1;
        if (sz < 0) { const double qx = (1.0 - fabs(py)) * (px >= 0 ? 1.0 : -1.0), qy = (1.0 - fabs(px)) * (py >= 0 ? 1.0 : -1.0); px = qx; py = qy; }
        const double amax = (double)STOCS_PN_AXIS_MAX;
        w = pn_pack((uint32_t)fmin(fmax(floor((px * 0.5 + 0.5) * amax + 0.5), 0.0), amax), (uint32_t)fmin(fmax(floor((py * 0.5 + 0.5) * amax + 0.5), 0.0), amax), 0u);
    }
    ncone[i] = w;
}

int fill_cull_field(stocs_ctx* c, hipStream_t st, bool cones) {
    SceneGrid& g = c->grid;
    cones = cones && g.d_ncone && !g.ncone_ready && c->lcp_patch_normals;
    if (!g.d_dist || (g.dist_ready && !cones)) return STOCS_OK;
    if (!st) st = c->stream;
    CullGeom G;
    G.o[0] = g.cg_ox; G.o[1] = g.cg_oy; G.o[2] = g.cg_oz;   // the float origin and edge the scan kernels use, widened
    G.g = g.cg_g; G.cap = g.cg_cap;
    G.n[0] = g.cg_nx; G.n[1] = g.cg_ny; G.n[2] = g.cg_nz; G.w = g.cg_w;
    const size_t n = (size_t)g.cg_nx * g.cg_ny * g.cg_nz;
    if (!g.dist_ready) {
        hipLaunchKernelGGL(dist_fill_kernel, dim3(grid_of(n)), dim3(256), 0, st, g.d_dist, n, g.cg_cap);
        hipLaunchKernelGGL(dist_splat_kernel, dim3((unsigned)((c->nS + 3) / 4)), dim3(256), 0, st, G, g.cg_ox, g.cg_oy, g.cg_oz, g.cg_g, g.cg_cap,
                           c->d_spos, c->nS, (uint32_t*)g.d_dist);
        STOCS_HIP_CHECK(hipGetLastError());
        g.dist_ready = true;
    }
    if (cones) {
        G.w = g.pn_w;
        const dim3 per_point((unsigned)((c->nS + 3) / 4));
        STOCS_HIP_CHECK(hipMemsetAsync(g.d_nsum, 0, 3 * n * sizeof(int32_t), st));
        hipLaunchKernelGGL(cone_splat_kernel<0>, per_point, dim3(256), 0, st, G, g.cg_ox, g.cg_oy, g.cg_oz, g.cg_g, g.pn_rb, c->d_spos, c->d_snrmw, c->nS, g.d_nsum, g.d_ncone);
        hipLaunchKernelGGL(cone_axis_kernel, dim3(grid_of(n)), dim3(256), 0, st, g.d_nsum, g.d_ncone, n);
        hipLaunchKernelGGL(cone_splat_kernel<1>, per_point, dim3(256), 0, st, G, g.cg_ox, g.cg_oy, g.cg_oz, g.cg_g, g.pn_rb, c->d_spos, c->d_snrmw, c->nS, g.d_nsum, g.d_ncone);
        STOCS_HIP_CHECK(hipGetLastError());
        g.ncone_ready = true;
    }
    return STOCS_OK;
}

}  // namespace stocs
