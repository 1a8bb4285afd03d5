// congruent.hip -- congruent 4-point sets on the model for every sampled base (HOT LOOP B).
// Replaces
//   stocs_estimator::find_congruent_sets_on_model         reference src/stocs.cpp:753-869
//   Super4PCS::IndexedNormalSet<Point,3,7,float>          reference include/super4pcs/accelerators/
//                                                         normalset.h:65-151, normalset.hpp:57-214
//   index helpers                                         accelerators/utils.h:139-148
//   PairCreationFunctor::getNormalizedEpsilon             include/super4pcs/pairCreationFunctor.h:141-143
//
// The reference builds, per base, a pointer grid (egSize^3 position cells, each a lazily allocated
// array of 343 std::vectors) over the "intersection" points of the P pairs and queries it once per
// Q pair along a sampled cone of directions.  Here all bases are processed together:
//   1. plan_*_kernel: the two PPF keys of the base, the source buckets of each lookup (CSR ranges of the index, in
//      ascending index position); host: the cone sample table (<= 56 unit vectors from libm's acosf/atanf/sinf/cosf --
//      per-base scalars, exactly the reference's values);
//   2. gather_key_kernel: the P and Q pair lists of all bases straight out of the device index, each entry with its
//      32-bit key (base, position cell of its intersection point);
//   3. ONE stable rocPRIM radix sort per list replaces the pointer grid: the Q entries by (base, position cell) in three
//      passes; the P entries by position cell alone in two -- the gather is base-major, so the entries of a (base, cell)
//      stay together, in index order, and the run table finds them;
//   4. p_records_kernel: per P entry a 16-byte record (world-space intersection point, direction cell), the direction
//      cell alone as 2 bytes, and the per-(base, cell) run table;
//   5. join, one lane per Q pair in (base, cell) order: cone -> direction-cell bitset in LDS (filtered exact arithmetic,
//      cone_cells.h), one pass over the P run of the query's cell, |e_Q - e_P|^2 <= epsilon (sic, Q1) -- a gate that cannot
//      fail inside one position cell while 12 epsilon^2 < epsilon, in which case the count reads the direction cells
//      alone.  Only the COUNT pass runs here (+ an exclusive scan);
//   6. quads are produced on demand: a base with fewer than the per-base maximum is materialised and
//      radix-sorted into the order of the reference's std::set<pair<P index, Q index>>; a base with
//      more is only ever sampled, and each sampled rank is resolved by re-running the join of the one Q
//      pair that owns it (resolve_picks_kernel) -- the 10^7-10^8 quads of a Cm trial are never written.
// Enumeration of a base's quads for that sampling ("walk order", a documented divergence like the seeded draw
// itself): by (position cell of the Q pair, index position of the Q pair, index position of the
// P pair), where the index position of a model pair is its place in the PPF index (ascending quantised feature,
// then ascending (id1, id2)).  The oracle enumerates the same way.
// The join is irregular integer/gather work: HBM/L2-bound, no MFMA.
#include <functional>
#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <cstring>


#include <algorithm>

#include "cone_cells.h"
#include "congruent_lists.h"
#include "prims.h"
#include "stocs_ctx.h"

namespace stocs {

__device__ __forceinline__ V3 ld3c(const float4* a, int i) { const float4 v = a[i]; return mk3(v.x, v.y, v.z); }

// ---- planning of the lookups on the device (what plan_lookup of ppf_index.hip does per key on the host) ----
// One 64-lane workgroup per (base, list): the PPF key of the base's point pair (stocs.cpp:771-772, the reference's double
// arithmetic), its 128 probes of the bucket table in ASCENDING key order -- F = K - o with o0 in {-tr, 0}, ok in
// {-2 rot, -rot, 0, rot}, rgbd.cpp:130-137 read from the query side -- two per lane, then lane 0 merges adjacent buckets
// into ranges exactly as plan_lookup does: the gathered list is in index order.
__global__ __launch_bounds__(64) void plan_ranges_kernel(const uint32_t* __restrict__ bucket_start, int tr, int rot, int NA, int nD,
                                                         const int32_t* __restrict__ bids, const float4* __restrict__ spos, const float4* __restrict__ snrm,
                                                         int nB, uint2* __restrict__ ranges, uint32_t* __restrict__ n_ranges, uint32_t* __restrict__ totals) {
    __shared__ uint32_t ss[128], se[128];
    const int b = blockIdx.x, list = blockIdx.y, lane = threadIdx.x;
    const int i0 = bids[4 * b + 2 * list], i1 = bids[4 * b + 2 * list + 1];
    int K[4];
    ppf_compute(ld3c(spos, i0), ld3c(snrm, i0), ld3c(spos, i1), ld3c(snrm, i1), tr, rot, K);
    const bool valid = !(K[0] <= 5 || K[1] < 0 || K[2] < 0 || K[3] < 0) && !(K[0] % tr || K[1] % rot || K[2] % rot || K[3] % rot);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h;                              // probe number in visiting order: a, then F1, F2, F3 ascending
        const int a = p >> 6, bi = (p >> 4) & 3, ci = (p >> 2) & 3, di = p & 3;
        const int F0 = K[0] + a * tr, F1 = K[1] + (bi - 1) * rot, F2 = K[2] + (ci - 1) * rot, F3 = K[3] + (di - 1) * rot;
        uint32_t s0 = 0, e0 = 0;
        if (valid && F1 >= 0 && F2 >= 0 && F3 >= 0) {
            const int fd = F0 / tr, f1 = F1 / rot, f2 = F2 / rot, f3 = F3 / rot;
            if (fd < nD && f1 < NA && f2 < NA && f3 < NA) {
                const uint32_t key = ppf_pack(fd, f1, f2, f3, NA);
                s0 = bucket_start[key]; e0 = bucket_start[key + 1];
                if (e0 <= s0) { s0 = 0; e0 = 0; }
            }
        }
        ss[p] = s0; se[p] = e0;
    }
    __syncthreads();
    if (lane == 0) {
        uint2* out = ranges + ((size_t)list * nB + b) * 128;
        uint32_t n = 0, total = 0, cs = 0, ce = 0;
        for (int p = 0; p < 128; ++p) {
            const uint32_t s0 = ss[p], e0 = se[p];
            if (e0 <= s0) continue;
            total += e0 - s0;
            if (n && ce == s0) ce = e0;
            else { if (n) out[n - 1] = make_uint2(cs, ce); cs = s0; ce = e0; ++n; }
        }
        if (n) out[n - 1] = make_uint2(cs, ce);
        n_ranges[(size_t)list * nB + b] = n;
        totals[(size_t)list * nB + b] = total;
    }
}

// One workgroup of 1024: offsets of every base in the gathered lists (a base without P pairs or without Q pairs gets neither,
// stocs.cpp:788), the segment arrays the gather walks, the list offsets patched into the base jobs, the totals for the host.
// Four in-place scans over arrays of nB + 1 words in device memory (any number of bases: a trial batch brings thousands), then
// everything else in parallel over the bases.
__global__ __launch_bounds__(1024) void plan_offsets_kernel(int nB, const uint2* __restrict__ ranges, const uint32_t* __restrict__ n_ranges, const uint32_t* __restrict__ totals,
                                                            BaseJob* __restrict__ jobs, Segment* __restrict__ psegs, Segment* __restrict__ qsegs,
                                                            uint32_t* __restrict__ p_off, uint32_t* __restrict__ q_off, uint32_t* __restrict__ sp_off, uint32_t* __restrict__ sq_off,
                                                            PlanOut* __restrict__ out, unsigned int* __restrict__ err) {
    __shared__ uint32_t s_part[1024];
    __shared__ unsigned long long s_tot[2];
    if (threadIdx.x < 2) s_tot[threadIdx.x] = 0ull;
    if (threadIdx.x < 64) err[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long tp = 0, tq = 0;
    for (int b = threadIdx.x; b <= nB; b += blockDim.x) {
        uint32_t np = 0, nq = 0, rp = 0, rq = 0;
        if (b < nB) { np = totals[b]; nq = totals[nB + b]; rp = n_ranges[b]; rq = n_ranges[nB + b]; }
        if (np == 0 || nq == 0) { np = 0; nq = 0; rp = 0; rq = 0; }
        p_off[b] = np; q_off[b] = nq; sp_off[b] = rp; sq_off[b] = rq;      // counts now, exclusive offsets after the scans (element nB: the totals)
        tp += np; tq += nq;
    }
    for (int off = 32; off > 0; off >>= 1) { tp += __shfl_xor(tp, off, 64); tq += __shfl_xor(tq, off, 64); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&s_tot[0], tp); atomicAdd(&s_tot[1], tq); }
    __syncthreads();
    block_scan_1024(p_off, (uint32_t)nB + 1u, s_part, [&](uint32_t b, uint32_t o, uint32_t v) { if (b < (uint32_t)nB) { jobs[b].p_off = o; jobs[b].p_len = v; } });
    __syncthreads();
    block_scan_1024(q_off, (uint32_t)nB + 1u, s_part, [&](uint32_t b, uint32_t o, uint32_t v) { if (b < (uint32_t)nB) { jobs[b].q_off = o; jobs[b].q_len = v; } });
    __syncthreads();
    block_scan_1024(sp_off, (uint32_t)nB + 1u, s_part, [](uint32_t, uint32_t, uint32_t) {});
    __syncthreads();
    block_scan_1024(sq_off, (uint32_t)nB + 1u, s_part, [](uint32_t, uint32_t, uint32_t) {});
    __syncthreads();
    if (threadIdx.x == 0) {
        out->totP = s_tot[0]; out->totQ = s_tot[1]; out->n_pseg = sp_off[nB]; out->n_qseg = sq_off[nB];
        out->overflow = (s_tot[0] >= 0xFFFF0000ull || s_tot[1] >= 0xFFFF0000ull) ? 1u : 0u; out->pad = 0;
    }
}

// The segment arrays the gathers walk, from the offsets laid out above: one wavefront per (base, list) -- the <= 128 ranges of a
// lookup, two per lane, their destinations an exclusive wavefront scan of their lengths.  (Inside plan_offsets_kernel, one thread
// per base, this loop was 170 us for the 6 000 bases of a 64-trial batch.)
__global__ __launch_bounds__(256) void plan_segments_kernel(int nB, const uint2* __restrict__ ranges, const uint32_t* __restrict__ n_ranges, const uint32_t* __restrict__ totals,
                                                            Segment* __restrict__ psegs, Segment* __restrict__ qsegs, const uint32_t* __restrict__ p_off,
                                                            const uint32_t* __restrict__ q_off, const uint32_t* __restrict__ sp_off, const uint32_t* __restrict__ sq_off) {
    const int lane = threadIdx.x & 63;
    const int job = blockIdx.x * 4 + (threadIdx.x >> 6);       // (base, list)
    if (job >= 2 * nB) return;
    const int b = job >> 1, list = job & 1;
    if (totals[b] == 0 || totals[nB + b] == 0) return;          // a base without P pairs or without Q pairs gets neither (stocs.cpp:788)
    const uint2* r = ranges + ((size_t)list * nB + b) * 128;
    Segment* sg = list ? qsegs + sq_off[b] : psegs + sp_off[b];
    const uint32_t d0 = list ? q_off[b] : p_off[b];
    const uint32_t n = n_ranges[(size_t)list * nB + b];
    uint32_t carry = 0;
    for (uint32_t k0 = 0; k0 < n; k0 += 64) {
        const uint32_t k = k0 + (uint32_t)lane;
        const uint2 v = k < n ? r[k] : make_uint2(0u, 0u);
        const uint32_t len = v.y - v.x;
        uint32_t inc = len;
        for (int dd = 1; dd < 64; dd <<= 1) { const uint32_t o = __shfl_up(inc, dd, 64); if (lane >= dd) inc += o; }
        if (k < n) { Segment o = {v.x, len, d0 + carry + (inc - len), (uint32_t)b}; sg[k] = o; }
        carry += __shfl(inc, 63, 64);
    }
}

// Zero fill as an ordinary kernel on the context's stream
__global__ __launch_bounds__(256) void zero_u32_kernel(uint32_t* __restrict__ a, size_t n, uint32_t* __restrict__ b) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { a[i] = 0; if (b) b[i] = 0; }
}

// After the sort: one record per P entry -- invPoint of stocs.cpp:845-849 (once per P entry instead of once per (Q, P)
// test) and the direction cell of normalset.hpp:114-131 (0xFFFF: never inserted) -- and for every (base, position cell)
// the run of its P entries.  Replaces the pointer grid _grid[pId] -> AngularGrid of normalset.h:87-88.
template <class KeyT>
__global__ __launch_bounds__(256) void p_records_kernel(const KeyT* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t totP, int cell_bits,
                                                        long long NC, const BaseJob* __restrict__ jobs, const float4* __restrict__ munit,
                                                        const float4* __restrict__ mpos, float nepsilon, float4* __restrict__ prec,
                                                        uint16_t* __restrict__ pdc, uint32_t* __restrict__ cfirst, uint32_t* __restrict__ cend) {
    // four entries per thread, 256 apart: the four (key, pair) loads, then the model points of all four, are in flight together (one entry per
    // thread left the kernel waiting on three dependent round trips: 1.8 TB/s over the 66 M entries of a 32-trial piece).
    // prec == NULL (the distance gate cannot fail inside a position cell, CongruentState::close_cells): the join decides on direction cells
    // alone, nobody reads the world-space point -- neither it nor the two model positions behind it are touched.
    constexpr int R = 4;
    const uint32_t e0 = blockIdx.x * (256u * R) + threadIdx.x;
    const KeyT cmask = ((KeyT)1 << cell_bits) - (KeyT)1;
    KeyT key[R], kprev[R], knext[R];
    uint32_t pr[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const uint32_t e = e0 + (uint32_t)k * 256u;
        const bool in = e < totP;
        key[k] = in ? keys[e] : (KeyT)0; pr[k] = in ? vals[e] : 0u;
        kprev[k] = (cfirst && in && e > 0u) ? keys[e - 1u] : (KeyT)0;
        knext[k] = (cfirst && in && e + 1u < totP) ? keys[e + 1u] : (KeyT)0;
    }
    float4 ua[R], ub[R];
#pragma unroll
    for (int k = 0; k < R; ++k) { ua[k] = munit[pr[k] >> 16]; ub[k] = munit[pr[k] & 0xFFFF]; }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const uint32_t e = e0 + (uint32_t)k * 256u;
        if (e >= totP) continue;
        const uint32_t b = (uint32_t)(key[k] >> cell_bits);
        const KeyT pc = key[k] & cmask;
        int dc = 0xFFFF;
        if (pc != cmask) {
            const int nc = index_normal(normalized3(mk3(ub[k].x, ub[k].y, ub[k].z) - mk3(ua[k].x, ua[k].y, ua[k].z)), nepsilon);
            if (nc >= 0 && nc < 343) dc = nc;
        }
        if (prec) {
            const int ia = pr[k] >> 16, ib = pr[k] & 0xFFFF;
            const V3 pp1 = ld3c(mpos, ia), pp2 = ld3c(mpos, ib);
            const V3 ip = pp1 + (pp2 - pp1) * jobs[b].inv1;
            prec[e] = make_float4(ip.x, ip.y, ip.z, __int_as_float(dc));
        }
        if (pdc) pdc[e] = (uint16_t)dc;
        if (!cfirst || pc == cmask) continue;
        const bool first = (e == 0) || kprev[k] != key[k];
        const bool last = (e + 1 == totP) || knext[k] != key[k];
        if (first) cfirst[(long long)b * NC + (long long)pc] = e;
        if (last) cend[(long long)b * NC + (long long)pc] = e + 1;
    }
}

// Everything the join needs, by value.
template <class KeyT>
struct JoinArgs {
    const BaseJob* jobs; const uint32_t* q_off; int nB;
    const float4* munit; const float4* mpos;
    const KeyT* qkeys; const uint32_t* qvals; uint32_t totQ;   // Q entries in (base, cell, index position) order
    const KeyT* pkeys; const uint32_t* pvals; const float4* prec;
    const uint16_t* pdc;   // direction cells alone when the distance gate of stocs.cpp:854 cannot fail inside a position cell (else NULL)
    const uint32_t* cfirst; const uint32_t* cend; long long NC;
    float nepsilon, half_inv_neps, dist_thr;
    const float2* trig;    // [STOCS_MAX_CONE + 1][STOCS_MAX_CONE]: (cos, sin) of theta_a for every sample count
    int id_bits, cell_bits;
    int base_in_key;   // the packed quad key carries the base above the four ids (it does whenever 4 id_bits + base_bits <= 64)
#ifdef STOCS_TOOLS_BUILD
    int gmin, rmin;   // STOCS_JOIN_GMIN / STOCS_JOIN_RMIN: the thresholds of join_count_kernel's group-wise counting, for sweeps
    int ablate;   // measurement build (STOCS_JOIN_ABLATE): 1 = no cone sampling (every direction cell set), 2 = no walk over the P run
#endif
};
#ifdef STOCS_TOOLS_BUILD
#define STOCS_JOIN_ABLATE(A, bit) (((A).ablate & (bit)) != 0)
#define JOIN_GMIN(A) (A).gmin
#define JOIN_RMIN(A) (uint32_t)(A).rmin
#else
#define STOCS_JOIN_ABLATE(A, bit) false
#define JOIN_GMIN(A) JOIN_GROUP_MIN
#define JOIN_RMIN(A) (uint32_t)JOIN_RUN_MIN
#endif

// the run of P entries that live in position cell `key` (only the query's own cell is inspected, Q9)
template <class KeyT>
__device__ __forceinline__ void p_run(const JoinArgs<KeyT>& A, const BaseJob& J, uint32_t b, KeyT key, KeyT pc, uint32_t* lo, uint32_t* hi) {
    if (A.cfirst) {
        *lo = A.cfirst[(long long)b * A.NC + (long long)pc];
        *hi = A.cend[(long long)b * A.NC + (long long)pc];
        return;
    }
    const KeyT* keys = A.pkeys + J.p_off;
    uint32_t l = 0, h = J.p_len;
    while (l < h) { const uint32_t mid = (l + h) >> 1; if (keys[mid] < key) l = mid + 1; else h = mid; }
    *lo = J.p_off + l;
    h = J.p_len;
    while (l < h) { const uint32_t mid = (l + h) >> 1; if (keys[mid] <= key) l = mid + 1; else h = mid; }
    *hi = J.p_off + l;
}

// Cone tables of the bases a workgroup's Q entries belong to, staged in LDS: the (x, y) components of a base's samples
// (z = cos alpha is folded into the filter).  A workgroup's 256 consecutive entries of the (base, cell)-sorted list
// belong to one base, seldom two; entries of a base beyond JOIN_LDS_BASES read the table from global memory.
#define JOIN_LDS_BASES 2
struct JoinLds {
    uint32_t seen[256][11];                          // 343-bit direction-cell set per lane (11 is odd: no bank conflicts)
    float2 dirs[JOIN_LDS_BASES][STOCS_MAX_CONE];
};

// The join of ONE Q entry against the P entries of its position cell: stocs.cpp:827-858 + normalset.hpp:166-214.
//   MODE 0: count;  MODE 1: write every match to out[0..] (walk order).
// b0 = base of the workgroup's first entry (its table is lds.dirs[0], the next base's lds.dirs[1]).
//   MODE 2: count, but only up to the direction-cell set: the P run comes back in *run_lo / *run_hi (empty: nothing can match)
//           and the caller counts (join_count_kernel does that per (base, cell) group of its workgroup).
template <int MODE, class KeyT>
__device__ __forceinline__ uint32_t join_one(const JoinArgs<KeyT>& A, uint32_t i, JoinLds& lds, uint32_t b0, uint64_t* __restrict__ out,
                                             uint32_t* run_lo = NULL, uint32_t* run_hi = NULL) {
    uint32_t* my = lds.seen[threadIdx.x];
    const KeyT key = A.qkeys[i];
    const KeyT cmask = ((KeyT)1 << A.cell_bits) - (KeyT)1;
    const KeyT pc = key & cmask;
    if (pc == cmask) return 0;
    const uint32_t b = (uint32_t)(key >> A.cell_bits);
    const BaseJob& J = A.jobs[b];
    const int nb = J.nb;
    if (J.p_len == 0 || nb == 0) return 0;
    uint32_t lo, hi;
    p_run(A, J, b, key, pc, &lo, &hi);
    if (lo >= hi) return 0;
    const uint32_t qr = A.qvals[i];
    const int qa = qr >> 16, qb = qr & 0xFFFF;
    const V3 p1 = ld3c(A.munit, qa), p2 = ld3c(A.munit, qb);
    const V3 pq1 = ld3c(A.mpos, qa), pq2 = ld3c(A.mpos, qb);
    const V3 queryQ = pq1 + J.inv2 * (pq2 - pq1);
    const V3 queryn = normalized3(p2 - p1);
    // direction cells hit by the sampled cone (std::set<unsigned> colored of normalset.hpp:188-204)
#pragma unroll
    for (int k = 0; k < 11; ++k) my[k] = 0;
    float q[4];
    quat_from_z(queryn, q);
    const float dz = J.cos_alpha;
    const ConeFilter cf = cone_filter_setup(q, dz, A.half_inv_neps);
    auto colour = [&](float dx, float dy) {
        int id = cone_cell_filtered(cf, dx, dy);
        if (id < 0) {   // within 5e-5 of a cell boundary (or not finite): the reference's own arithmetic decides
            id = cone_cell_exact(q, mk3(dx, dy, dz), A.nepsilon);
            if (id < 0) return;  // std::array::at would throw (NaN direction)
        }
        // this lane's own words; the no-return LDS atomic is one instruction and needs no wait
        __hip_atomic_fetch_or(&my[id >> 5], 1u << (id & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    };
    if (STOCS_JOIN_ABLATE(A, 1)) {
#pragma unroll
        for (int k = 0; k < 11; ++k) my[k] = 0xFFFFFFFFu;
    } else
    if (b - b0 < (uint32_t)JOIN_LDS_BASES) {   // the sample after this one is read while this one is evaluated
        const float2* tab = lds.dirs[b - b0];
        float2 d = tab[0];
        for (int a = 0; a < nb; ++a) {
            const float2 dn = tab[a + 1 < nb ? a + 1 : a];
            colour(d.x, d.y);
            d = dn;
        }
    } else {
        const float2* tr = A.trig + (size_t)nb * STOCS_MAX_CONE;
        const float sa = J.sin_alpha;
        for (int a = 0; a < nb; ++a) { const float2 t = tr[a]; colour(sa * t.x, sa * t.y); }
    }
    // one linear pass over the position cell's P entries against the direction bitset, four records in flight
    uint32_t local = 0;
    const int id_bits = A.id_bits;
    auto test = [&](const float4& r, uint32_t k) {
        const uint32_t dc = (uint32_t)__float_as_int(r.w);
        if (dc >= 343u || !((my[dc >> 5] >> (dc & 31)) & 1u)) return;
        if (sqn3(queryQ - mk3(r.x, r.y, r.z)) <= A.dist_thr) {  // squared metres vs metres (Q1), reproduced
            if (MODE == 1) {   // sort key: base, then (P.first, P.second, Q.first, Q.second) == the std::set order
                const uint32_t pr = A.pvals[k];
                const int pa = pr >> 16, pb = pr & 0xFFFF;
                out[local] = (A.base_in_key ? (uint64_t)b << (4 * id_bits) : 0ull) | ((uint64_t)pa << (3 * id_bits)) | ((uint64_t)pb << (2 * id_bits)) |
                             ((uint64_t)qa << id_bits) | (uint64_t)qb;
            }
            local++;
        }
    };
    if (MODE == 2) { *run_lo = lo; *run_hi = hi; return 0; }
    if (STOCS_JOIN_ABLATE(A, 2)) return my[0] & 1u;
    if (MODE == 0 && A.pdc) {
        // Counting with the gate out of the way: ||e_Q - e_P||^2 <= epsilon (squared metres against metres, Q1) holds for ANY
        // two points of one position cell -- the cell edge is below 2 epsilon, so the squared diagonal is below 12 epsilon^2,
        // and the host enables this path only when that is comfortably below epsilon -- so an entry matches iff its direction
        // cell is in the cone's set: 2 bytes per entry instead of 16, eight entries per load.
        const uint16_t* dcs = A.pdc;
        auto hit = [&](uint32_t dc) { return dc < 343u && ((my[dc >> 5] >> (dc & 31)) & 1u) ? 1u : 0u; };
        uint32_t k = lo;
        for (; k < hi && (k & 7u); ++k) local += hit(dcs[k]);
        for (; k + 8 <= hi; k += 8) {
            const uint4 v = *(const uint4*)(dcs + k);
            local += hit(v.x & 0xFFFFu) + hit(v.x >> 16) + hit(v.y & 0xFFFFu) + hit(v.y >> 16) + hit(v.z & 0xFFFFu) + hit(v.z >> 16) + hit(v.w & 0xFFFFu) + hit(v.w >> 16);
        }
        for (; k < hi; ++k) local += hit(dcs[k]);
        return local;
    }
    if (A.pdc) {   // (MODE 1 with the gate out of the way: the same decision as the count above, the pairs of the matches read on demand)
        for (uint32_t k = lo; k < hi; ++k) {
            const uint32_t dc = A.pdc[k];
            if (dc >= 343u || !((my[dc >> 5] >> (dc & 31)) & 1u)) continue;
            const uint32_t pr = A.pvals[k];
            const int pa = pr >> 16, pb = pr & 0xFFFF;
            out[local++] = (A.base_in_key ? (uint64_t)b << (4 * id_bits) : 0ull) | ((uint64_t)pa << (3 * id_bits)) | ((uint64_t)pb << (2 * id_bits)) |
                           ((uint64_t)qa << id_bits) | (uint64_t)qb;
        }
        return local;
    }
    uint32_t k = lo;
    for (; k + 4 <= hi; k += 4) {
        const float4 r0 = A.prec[k], r1 = A.prec[k + 1], r2 = A.prec[k + 2], r3 = A.prec[k + 3];
        test(r0, k); test(r1, k + 1); test(r2, k + 2); test(r3, k + 3);
    }
    for (; k < hi; ++k) test(A.prec[k], k);
    return local;
}

// workgroup prologue of the join kernels: cone tables of the first JOIN_LDS_BASES bases of the workgroup's entries
template <class KeyT>
__device__ __forceinline__ uint32_t join_stage_tables(const JoinArgs<KeyT>& A, JoinLds& lds, uint32_t i0 = 0xFFFFFFFFu) {
    if (i0 == 0xFFFFFFFFu) i0 = blockIdx.x * blockDim.x;
    const uint32_t b0 = (uint32_t)(A.qkeys[i0] >> A.cell_bits);   // i0 < totQ for every launched workgroup
    for (int t = threadIdx.x; t < JOIN_LDS_BASES * STOCS_MAX_CONE; t += blockDim.x) {
        const uint32_t b = b0 + (uint32_t)(t / STOCS_MAX_CONE);
        const int a = t % STOCS_MAX_CONE;
        float2 d = make_float2(0.f, 0.f);
        if (b < (uint32_t)A.nB && a < A.jobs[b].nb) { const float2 tr = A.trig[(size_t)A.jobs[b].nb * STOCS_MAX_CONE + a]; const float sa = A.jobs[b].sin_alpha; d = make_float2(sa * tr.x, sa * tr.y); }
        lds.dirs[t / STOCS_MAX_CONE][a] = d;
    }
    __syncthreads();
    return b0;
}

// per-base totals: the scanned count at the first Q entry of every base (one small copy instead of one per base)
__global__ __launch_bounds__(256) void base_offsets_kernel(const unsigned long long* __restrict__ qoffe, const uint32_t* __restrict__ q_off, int n,
                                                           unsigned long long* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n) out[b] = qoffe[q_off[b]];
}

// count pass, one lane per Q entry in (base, position cell) order
// The Q entries are in (base, cell) order, so the 64 of a wavefront fall into a few groups that walk the SAME P run, each
// entry against its own direction-cell set.  Three quarters of the entries have no P entry in their cell and are done at once;
// the rest sit in the big bases, where a cell holds ~300 Q entries and ~300 P entries, and their walks were 60 % of this kernel
// (device clock 0.32 ms: 0.14 without the walk, 0.25 without the cone samples; tools/join_ablate.py; a CPU census of a Cm trial:
// 18 % of the entries carry 98 % of the walk).  When the distance gate cannot fail (A.pdc: direction cells alone decide) a
// match count is the sum over the set's cells of (P entries of the run in that cell): a group of >= JOIN_GROUP_MIN lanes whose
// run has >= JOIN_RUN_MIN entries builds that histogram once per wavefront in LDS (16-bit counters, the wavefront's 64 lanes
// reading the run two bytes per entry) and every lane of the group adds up <= 56 counters instead of testing ~300 entries.
// Smaller groups and shorter runs walk the run as before.  No workgroup barrier: wavefronts without work leave at once.
// Same counts either way (integer sums).
#define JOIN_GROUP_MIN 1
#define JOIN_RUN_MIN 64
template <class KeyT>
__global__ __launch_bounds__(256) void join_count_kernel(JoinArgs<KeyT> A, unsigned long long* __restrict__ qcnt) {
    __shared__ JoinLds lds;
    __shared__ uint32_t s_hist[4][172];            // per wavefront: 344 16-bit counters, two per word
    const uint32_t b0 = join_stage_tables(A, lds);
    const uint32_t tid = threadIdx.x, i = blockIdx.x * blockDim.x + tid;
    const int lane = tid & 63, w = tid >> 6;
    const bool live = i < A.totQ;
    if (i == 0) qcnt[A.totQ] = 0;   // the scan runs over totQ + 1 entries so that its last output is the total
    if (!A.pdc || STOCS_JOIN_ABLATE(A, 3)) {   // the gate has to be evaluated per (Q, P) couple: every entry walks its run
        if (live) qcnt[i] = join_one<0>(A, i, lds, b0, (uint64_t*)NULL);
        return;
    }
    uint32_t lo = 0, hi = 0;
    if (live) (void)join_one<2>(A, i, lds, b0, (uint64_t*)NULL, &lo, &hi);   // direction-cell set in lds.seen[tid], the run in lo / hi
    const bool has = hi > lo;
    if (!__any(has)) { if (live) qcnt[i] = 0; return; }
    // groups of the wavefront = maximal stretches of lanes with the same run
    const uint32_t plo = __shfl_up(lo, 1, 64), phi = __shfl_up(hi, 1, 64);
    const bool head = lane == 0 || plo != lo || phi != hi;
    const unsigned long long heads = __ballot(head);
    const int g0 = 63 - __clzll((long long)(heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull))));
    const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
    const int g1 = above ? lane + __ffsll((long long)above) : 64;
    const bool big = has && (hi - lo) < 65536u && (g1 - g0) >= JOIN_GMIN(A) && (hi - lo) >= JOIN_RMIN(A);
    const uint32_t* my = lds.seen[tid];
    const uint16_t* dcs = A.pdc;
    uint32_t count = 0;
    if (has && !big) {   // small groups / short runs: walk the run, eight 2-byte direction cells per load
        auto hit = [&](uint32_t dc) { return dc < 343u && ((my[dc >> 5] >> (dc & 31)) & 1u) ? 1u : 0u; };
        uint32_t k = lo;
        for (; k < hi && (k & 7u); ++k) count += hit(dcs[k]);
        for (; k + 8 <= hi; k += 8) {
            const uint4 v = *(const uint4*)(dcs + k);
            count += hit(v.x & 0xFFFFu) + hit(v.x >> 16) + hit(v.y & 0xFFFFu) + hit(v.y >> 16) + hit(v.z & 0xFFFFu) + hit(v.z >> 16) + hit(v.w & 0xFFFFu) + hit(v.w >> 16);
        }
        for (; k < hi; ++k) count += hit(dcs[k]);
    }
    // the big groups of this wavefront, one after the other (at most 64 / JOIN_GROUP_MIN of them)
    unsigned long long todo = __ballot(head && big);
    uint32_t* hist = s_hist[w];
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const uint32_t glo = (uint32_t)__shfl((int)lo, leader, 64), ghi = (uint32_t)__shfl((int)hi, leader, 64);
        const int gend = __shfl(g1, leader, 64);
        for (int c = lane; c < 172; c += 64) hist[c] = 0;
        __builtin_amdgcn_wave_barrier();
        for (uint32_t k0 = glo; k0 < ghi; k0 += 256) {   // four loads in flight per lane
            uint32_t dc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const uint32_t k = k0 + 64u * u + (uint32_t)lane; dc[u] = k < ghi ? dcs[k] : 0xFFFFu; }
#pragma unroll
            for (int u = 0; u < 4; ++u) if (dc[u] < 343u) atomicAdd(&hist[dc[u] >> 1], 1u << (16u * (dc[u] & 1u)));
        }
        __builtin_amdgcn_wave_barrier();
        if (lane >= leader && lane < gend) {
#pragma unroll
            for (int ww = 0; ww < 11; ++ww) {
                uint32_t bits = my[ww];
                while (bits) {
                    const uint32_t dc = 32u * ww + (uint32_t)(__ffs((int)bits) - 1);
                    count += (hist[dc >> 1] >> (16u * (dc & 1u))) & 0xFFFFu;
                    bits &= bits - 1u;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (live) qcnt[i] = count;
}

// fill pass for the bases whose out_base is not ~0: destinations from the exclusive scan of the counts (no atomics).
// `blocks` lists, per workgroup, the (first, end) Q entries it takes: only the Q ranges of the selected bases are walked
// (a trial materialises a handful of small bases out of a hundred: the sweep over all Q entries was 50 us at Cm).
template <class KeyT>
__global__ __launch_bounds__(256) void join_fill_kernel(JoinArgs<KeyT> A, const unsigned long long* __restrict__ qoffe,
                                                        const unsigned long long* __restrict__ out_base, uint64_t* __restrict__ quads,
                                                        const uint2* __restrict__ blocks) {
    __shared__ JoinLds lds;
    const uint2 range = blocks[blockIdx.x];
    const uint32_t b0 = join_stage_tables(A, lds, range.x);
    const uint32_t i = range.x + threadIdx.x;
    if (i >= range.y) return;
    const uint32_t b = (uint32_t)(A.qkeys[i] >> A.cell_bits);
    const unsigned long long ob = out_base[b];
    if (ob == ~0ull) return;
    const unsigned long long o0 = qoffe[i];
    if (qoffe[i + 1] == o0) return;
    join_one<1>(A, i, lds, b0, quads + ob + (o0 - qoffe[A.q_off[b]]));
}

// the four model ids of a packed quad key (id_bits each, below the base when the key carries one)
STOCS_HD void unpack_quad(uint64_t key, int id_bits, int32_t out[4]) {
    const uint64_t m = (1ull << id_bits) - 1ull;
    out[0] = (int32_t)((key >> (3 * id_bits)) & m); out[1] = (int32_t)((key >> (2 * id_bits)) & m);
    out[2] = (int32_t)((key >> id_bits) & m); out[3] = (int32_t)(key & m);
}

__device__ __forceinline__ void store_job(XformJob* jobs, int dst, const int32_t* base_ids, int b, uint64_t key, int id_bits) {
    XformJob job;
#pragma unroll
    for (int k = 0; k < 4; ++k) job.s[k] = base_ids[4 * b + k];
    unpack_quad(key, id_bits, job.q);
    jobs[dst] = job;
}

// picks -> transform jobs.  A pick is either a rank in a small base's sorted run (all quads are used, in the
// reference's std::set order) or a rank in a big base's WALK order (Q entries in (cell, index) order, each one's matches
// in P-run order): the Q entry is found by binary search in the scanned counts and its join is re-run up to
// the wanted match, so the 10^7-10^8 quads of the big bases are never materialised.  One wavefront per pick:
// the cone samples are spread over the lanes (LDS bitset, the reference's exact arithmetic), the P run is tested 64
// entries at a time and the wanted match is located with ballot / popcount, in run order.
template <class KeyT>
__global__ __launch_bounds__(256) void resolve_picks_kernel(JoinArgs<KeyT> A, const unsigned long long* __restrict__ qoffe, const Pick* __restrict__ picks, int n,
                                                            const uint64_t* __restrict__ sorted_quads, const unsigned long long* __restrict__ sorted_off,
                                                            const int32_t* __restrict__ base_ids, XformJob* __restrict__ jobs,
                                                            uint64_t* __restrict__ keys_out, unsigned int* __restrict__ n_unresolved) {
    __shared__ uint32_t seen_all[4][12];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x * 4 + w;
    if (j >= n) return;   // whole wave leaves; no block-wide barrier below
    uint32_t* seen = seen_all[w];
    const Pick pk = picks[j];
    const int b = pk.base;
    uint64_t key = ~0ull;
    if (pk.sorted) {
        key = sorted_quads[sorted_off[b] + (unsigned long long)pk.rank];
    } else {
        const uint32_t q0 = A.q_off[b], q1 = A.q_off[b + 1];
        const unsigned long long target = qoffe[q0] + (unsigned long long)pk.rank;
        uint32_t elo = q0, ehi = q1 - 1;   // last i in [q0, q1) with qoffe[i] <= target
        while (elo < ehi) {
            const uint32_t mid = elo + ((ehi - elo + 1) >> 1);
            if (qoffe[mid] <= target) elo = mid; else ehi = mid - 1;
        }
        unsigned long long want = target - qoffe[elo];
        // ---- the join of Q entry elo, wave-wide (same arithmetic as join_one) ----
        const BaseJob& J = A.jobs[b];
        const KeyT qk = A.qkeys[elo];
        const KeyT cmask = ((KeyT)1 << A.cell_bits) - (KeyT)1;
        const KeyT pc = qk & cmask;
        const uint32_t qr = A.qvals[elo];
        const int qa = qr >> 16, qb = qr & 0xFFFF;
        const V3 p1 = ld3c(A.munit, qa), p2 = ld3c(A.munit, qb);
        const V3 pq1 = ld3c(A.mpos, qa), pq2 = ld3c(A.mpos, qb);
        const V3 queryQ = pq1 + J.inv2 * (pq2 - pq1);
        const V3 queryn = normalized3(p2 - p1);
        uint32_t lo = 0, hi = 0;
        // a Q entry without a position cell has no matches and is never selected; stay in bounds regardless
        if (pc != cmask) p_run(A, J, (uint32_t)b, qk, pc, &lo, &hi);
        if (lane < 12) seen[lane] = 0;
        __threadfence_block(); __builtin_amdgcn_wave_barrier();
        float q[4];
        quat_from_z(queryn, q);
        if (lane < J.nb) {
            const float2 tr = A.trig[(size_t)J.nb * STOCS_MAX_CONE + lane];
            const int id = cone_cell_exact(q, mk3(J.sin_alpha * tr.x, J.sin_alpha * tr.y, J.cos_alpha), A.nepsilon);
            if (id >= 0) atomicOr(&seen[id >> 5], 1u << (id & 31));
        }
        __threadfence_block(); __builtin_amdgcn_wave_barrier();
        const int id_bits = A.id_bits;
        for (uint32_t k0 = lo; k0 < hi; k0 += 64) {
            const uint32_t k = k0 + lane;
            bool hit = false;
            int pa = 0, pb = 0;
            if (k < hi && A.pdc) {   // the gate cannot fail inside a position cell: direction cells alone (no records were written)
                const uint32_t dc = A.pdc[k];
                if (dc < 343u && ((seen[dc >> 5] >> (dc & 31)) & 1u)) {
                    const uint32_t pr = A.pvals[k];
                    pa = pr >> 16; pb = pr & 0xFFFF;
                    hit = true;
                }
            } else if (k < hi) {
                const float4 r = A.prec[k];
                const uint32_t dc = (uint32_t)__float_as_int(r.w);
                if (dc < 343u && ((seen[dc >> 5] >> (dc & 31)) & 1u)) {
                    const uint32_t pr = A.pvals[k];
                    pa = pr >> 16; pb = pr & 0xFFFF;
                    hit = sqn3(queryQ - mk3(r.x, r.y, r.z)) <= A.dist_thr;
                }
            }
            const unsigned long long m = __ballot(hit);
            const unsigned long long cnt = (unsigned long long)__popcll(m);
            if (want < cnt) {
                const unsigned long long below = m & ((1ull << lane) - 1ull);
                if (hit && (unsigned long long)__popcll(below) == want)
                    key = (A.base_in_key ? (uint64_t)b << (4 * id_bits) : 0ull) | ((uint64_t)pa << (3 * id_bits)) | ((uint64_t)pb << (2 * id_bits)) |
                          ((uint64_t)qa << id_bits) | (uint64_t)qb;
                // hand the winner's key to every lane
                const int src = __ffsll((long long)__ballot(key != ~0ull)) - 1;
                key = ((uint64_t)(uint32_t)__shfl((int)(key >> 32), src, 64) << 32) | (uint64_t)(uint32_t)__shfl((int)(key & 0xFFFFFFFFull), src, 64);
                break;
            }
            want -= cnt;
        }
    }
    if (lane == 0) {
        if (key == ~0ull) {   // cannot happen while counts and join agree; never hand an invalid quad to the next kernel
            atomicAdd(n_unresolved, 1u);
            key = 0;          // quad (0,0,0,0): a degenerate frame, rejected by rigid_transform_kernel
        }
        if (jobs) store_job(jobs, pk.dst, base_ids, b, key, A.id_bits);
        if (keys_out) keys_out[pk.dst] = key;
    }
}

// Device memory of this file comes from two arenas (stocs_ctx.h) owned by the context, reset (not freed) at the start
// of the entry point that owns the arena: after the first trial a call does no hipMalloc / hipFree at all.
static thread_local Arena* tl_arena = NULL;   // set by every entry point of this file before it allocates

template <class T>
struct DevBuf {   // typed view of arena memory; nothing to release
    T* p;
    DevBuf() : p(NULL) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    int alloc(size_t n) { return tl_arena->take(n * sizeof(T), (void**)&p); }
};

// What stays on the device after the count pass (stocs_find_congruent_all) so that quads can be produced on
// demand: the sorted Q list, the sorted P list with its records and cell tables and the scanned per-Q match counts.
struct CongruentState {
    Arena arena_state;   // the buffers below + the temporaries of stocs_find_congruent_all; reset by that call
    Arena arena_tmp;     // temporaries of the calls that produce quads afterwards; reset by each of them
    bool valid = false;  // a count pass has completed and its buffers are intact
    // host work of the current call that only the join needs (the cone records of a batch's thousands of bases: three libm calls each,
    // 0.2 ms for 6 400 bases), done by the count pass while the device gathers instead of before anything is enqueued
    std::function<int()> deferred;
    // quads of the small bases, materialised ahead of the picks that refer to them (stocs_internal_prepare_small)
    bool small_ready = false, small_any = false;
    DevBuf<uint64_t> d_small_sorted;
    DevBuf<unsigned long long> d_small_soff;
    bool wide = false;   // 64-bit sort keys (only without the cell table: more than 32 bits of (base, cell))
    int nB = 0;
    uint32_t totP = 0, totQ = 0;
    long long NC = 0;
    bool use_table = false;
    float nepsilon = 0, half_inv_neps = 0;
    int id_bits = 16, base_bits = 1, cell_bits = 1;
    bool base_in_key = true;   // packed quad keys carry the base (4 id_bits + base_bits <= 64); else bases are told apart by their runs
    DevBuf<BaseJob> d_jobs;
    DevBuf<uint32_t> d_qoff, d_pvals, d_qvals, d_cfirst, d_cend;
    DevBuf<char> d_pkeys, d_qkeys;   // KeyT arrays (uint32_t, or uint64_t when wide)
    DevBuf<float4> d_prec;
    DevBuf<uint16_t> d_pdc;
    bool close_cells = false;     // the distance gate cannot fail inside a position cell: count on direction cells alone
    DevBuf<unsigned long long> d_qoffe;
    DevBuf<int32_t> d_bids;
    DevBuf<unsigned int> d_err;   // picks resolve_picks_kernel could not resolve (internal consistency check)
    // host sources of asynchronous uploads issued by materialise / make_jobs: kept here so that they outlive the copy
    // (those calls return without synchronising; the caller's own synchronisation point comes before the next reuse)
    std::vector<unsigned long long> h_out_base, h_off;
    std::vector<uint32_t> h_qoff;          // Q range of every base (host copy of d_qoff)
    bool reduce = false;                   // this trial's lists are reduced to the entries with a partner cell
    unsigned long long hist_P = 0, hist_Q = 0;   // planned list lengths of the last trial on this scene (capacities of the next one)
    int hist_nB = 0;
    bool no_quads = false;                 // the last count found no (base, cell) that both lists occupy
    std::vector<uint2> h_blocks;           // workgroup -> Q range of the last materialise
    void* h_stage = NULL;         // pinned staging of the per-trial tables (one upload per trial)
    size_t stage_bytes = 0;
    float2* d_trig = NULL;        // the shared (cos, sin) table of the cone samples, uploaded once per context
    char* d_plan = NULL;          // persistent planning buffer: jobs, base ids, ranges, segments, offsets (outside the arenas:
    size_t plan_bytes = 0;        // it is written before the trial's sizes -- and with them the arena's -- are known)
    template <class KeyT>
    JoinArgs<KeyT> args(const stocs_ctx* c) const {
        JoinArgs<KeyT> A;
        A.jobs = d_jobs.p; A.q_off = d_qoff.p; A.nB = nB; A.munit = c->d_munit; A.mpos = c->d_mpos;
        A.qkeys = (const KeyT*)d_qkeys.p; A.qvals = d_qvals.p; A.totQ = totQ;
        A.pkeys = (const KeyT*)d_pkeys.p; A.pvals = d_pvals.p; A.prec = d_prec.p; A.pdc = close_cells ? d_pdc.p : NULL;
        A.cfirst = use_table ? d_cfirst.p : NULL; A.cend = use_table ? d_cend.p : NULL; A.NC = NC;
        A.nepsilon = nepsilon; A.half_inv_neps = half_inv_neps; A.dist_thr = c->prm.distance_threshold; A.id_bits = id_bits; A.cell_bits = cell_bits;
        A.trig = d_trig;
        A.base_in_key = base_in_key ? 1 : 0;
#ifdef STOCS_TOOLS_BUILD
        A.gmin = JOIN_GROUP_MIN; A.rmin = JOIN_RUN_MIN;
        A.ablate = getenv("STOCS_JOIN_ABLATE") ? atoi(getenv("STOCS_JOIN_ABLATE")) : 0;
        if (getenv("STOCS_JOIN_GMIN")) A.gmin = atoi(getenv("STOCS_JOIN_GMIN"));
        if (getenv("STOCS_JOIN_RMIN")) A.rmin = atoi(getenv("STOCS_JOIN_RMIN"));
#endif
        return A;
    }
};

// Materialises the quads of the bases with sel[b] != 0 into one device buffer, sorted by (base, a, b, c, d) =
// per base the order of the reference's std::set<pair<P index, Q index>>.  off[b] .. off[b+1] is base b's run.
template <class KeyT>
static int materialise_t(stocs_ctx* c, CongruentState* S, const std::vector<char>& sel, DevBuf<uint64_t>* out, std::vector<unsigned long long>* off) {
    const int nB = S->nB;
    std::vector<unsigned long long>& out_base = S->h_out_base;
    out_base.assign(nB, ~0ull);
    off->assign(nB + 1, 0);
    unsigned long long tot = 0;
    for (int b = 0; b < nB; ++b) {
        (*off)[b] = tot;
        if (sel[b]) { out_base[b] = tot; tot += c->quad_off[b + 1] - c->quad_off[b]; }
    }
    (*off)[nB] = tot;
    if (tot == 0) return STOCS_OK;
    if (tot > (1ull << 31)) { set_error("%llu congruent quads requested at once: more than 2^31, refusing to materialise them", tot); return STOCS_ERR_CAPACITY; }
    hipStream_t st = c->stream;
    DevBuf<unsigned long long> d_ob; DevBuf<uint64_t> d_raw; DevBuf<char> d_tmp; DevBuf<uint2> d_blocks;
    std::vector<uint2>& blocks = S->h_blocks;
    blocks.clear();
    for (int b = 0; b < nB; ++b)
        if (sel[b] && c->quad_off[b + 1] > c->quad_off[b])
            for (uint32_t i0 = S->h_qoff[b]; i0 < S->h_qoff[b + 1]; i0 += 256) blocks.push_back(make_uint2(i0, std::min(i0 + 256u, S->h_qoff[b + 1])));
    int rc;
    if ((rc = d_ob.alloc(nB)) || (rc = d_raw.alloc(tot)) || (rc = out->alloc(tot)) || (rc = d_blocks.alloc(std::max<size_t>(blocks.size(), 1)))) return rc;
    STOCS_HIP_CHECK(hipMemcpyAsync(d_ob.p, out_base.data(), 8 * (size_t)nB, hipMemcpyHostToDevice, st));
    STOCS_HIP_CHECK(hipMemcpyAsync(d_blocks.p, blocks.data(), sizeof(uint2) * blocks.size(), hipMemcpyHostToDevice, st));
    if (!blocks.empty())
        hipLaunchKernelGGL(join_fill_kernel<KeyT>, dim3((unsigned)blocks.size()), dim3(256), 0, st, S->args<KeyT>(c), S->d_qoffe.p, d_ob.p, d_raw.p, d_blocks.p);
    STOCS_HIP_CHECK(hipGetLastError());
    size_t tmp = 0;
    int n_sel = 0;
    for (int b = 0; b < nB; ++b) n_sel += sel[b] ? 1 : 0;
    if (S->base_in_key || n_sel <= 1) {   // one sort over everything: the base is part of the key (or there is only one)
        const unsigned end_bit = (unsigned)(4 * S->id_bits + (S->base_in_key ? S->base_bits : 0));
        STOCS_HIP_CHECK(sort_keys(NULL, tmp, d_raw.p, out->p, (size_t)tot, 0, end_bit, st));
        if ((rc = d_tmp.alloc(tmp))) return rc;
        STOCS_HIP_CHECK(sort_keys(d_tmp.p, tmp, d_raw.p, out->p, (size_t)tot, 0, end_bit, st));
    } else {
        // models beyond 16 384 points at 100 bases: four 15- or 16-bit ids fill the 64 bits, so the key holds the ids alone and
        // every base's run (off[b] .. off[b+1], filled base by base) is sorted as a segment of its own
        DevBuf<unsigned long long> d_off;
        if ((rc = d_off.alloc((size_t)nB + 1))) return rc;
        STOCS_HIP_CHECK(hipMemcpyAsync(d_off.p, off->data(), 8 * ((size_t)nB + 1), hipMemcpyHostToDevice, st));   // *off outlives the copy (S->h_off or the caller's)
        const unsigned end_bit = (unsigned)(4 * S->id_bits);
        STOCS_HIP_CHECK(segmented_sort_keys(NULL, tmp, d_raw.p, out->p, (unsigned)tot, (unsigned)nB, d_off.p, d_off.p + 1, 0, end_bit, st));
        if ((rc = d_tmp.alloc(tmp))) return rc;
        STOCS_HIP_CHECK(segmented_sort_keys(d_tmp.p, tmp, d_raw.p, out->p, (unsigned)tot, (unsigned)nB, d_off.p, d_off.p + 1, 0, end_bit, st));
    }
    // no synchronisation: the temporaries are arena memory, recycled only by a later call's reset, and every later use is
    // ordered behind this work on the context's stream (out_base was copied from pageable memory: staged by the runtime
    // before hipMemcpyAsync returned)
    return STOCS_OK;
}
static int materialise(stocs_ctx* c, CongruentState* S, const std::vector<char>& sel, DevBuf<uint64_t>* out, std::vector<unsigned long long>* off) {
    return S->wide ? materialise_t<uint64_t>(c, S, sel, out, off) : materialise_t<uint32_t>(c, S, sel, out, off);
}

template <class KeyT>
static void launch_resolve_picks_t(stocs_ctx* c, CongruentState* S, const Pick* picks, int n, const uint64_t* sorted, const unsigned long long* soff, XformJob* jobs, uint64_t* keys_out) {
    hipLaunchKernelGGL(resolve_picks_kernel<KeyT>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, S->template args<KeyT>(c), S->d_qoffe.p, picks, n, sorted, soff,
                       S->d_bids.p, jobs, keys_out, S->d_err.p);
}
// n device-resident picks -> transform jobs and / or packed quad keys (either may be NULL), one wavefront per pick on the context's
// stream; sorted / soff: the materialised runs the picks with sorted != 0 refer to (NULL when there are none)
static int launch_resolve_picks(stocs_ctx* c, CongruentState* S, const Pick* picks, int n, const uint64_t* sorted, const unsigned long long* soff, XformJob* jobs, uint64_t* keys_out) {
    if (S->wide) launch_resolve_picks_t<uint64_t>(c, S, picks, n, sorted, soff, jobs, keys_out);
    else launch_resolve_picks_t<uint32_t>(c, S, picks, n, sorted, soff, jobs, keys_out);
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

// (cos, sin) of the sample angles theta_a = a * angleStep for every sample count nb (normalset.hpp:183-188: float libm on per-count
// scalars, exactly the reference's values); row nb of [STOCS_MAX_CONE + 1][STOCS_MAX_CONE]
static const float* cone_trig() {
    static float trig[STOCS_MAX_CONE + 1][STOCS_MAX_CONE][2];
    static bool ready = false;
    static pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
    pthread_mutex_lock(&mu);
    if (!ready) {
        memset(trig, 0, sizeof(trig));
        for (unsigned nb = 1; nb <= STOCS_MAX_CONE; ++nb) {
            const float angleStep = (float)((double)2.0f * M_PI / (double)(float)nb);
            for (unsigned a = 0; a < nb; ++a) {
                const float theta = (float)a * angleStep;
                trig[nb][a][0] = cosf(theta);
                trig[nb][a][1] = sinf(theta);
            }
        }
        ready = true;
    }
    pthread_mutex_unlock(&mu);
    return &trig[0][0][0];
}

// the cone fields of the base jobs, uploaded on their own when the host computes them while the device already plans and gathers
__global__ __launch_bounds__(256) void patch_cone_kernel(BaseJob* __restrict__ jobs, const float4* __restrict__ cone, int nB) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nB) return;
    const float4 v = cone[b];
    jobs[b].cos_alpha = v.x; jobs[b].sin_alpha = v.y; jobs[b].nb = __float_as_int(v.z);
}

// cone samples of a base: normalset.hpp:178-190 (float libm calls on per-base scalars: exactly the reference's values): their
// number and sin(alpha); sample a is (sin_alpha * cos theta_a, sin_alpha * sin theta_a, cos_alpha) with the shared table above
static void fill_cone_table(BaseJob* J) {
    const float alpha = acosf(J->cos_alpha);
    const float perimeter = (float)((double)2.0f * M_PI * (double)atanf(alpha));  // sic (Q10)
    const unsigned nb = (unsigned)(2 * ceilf(perimeter * 7.0f / 2.0f));
    J->sin_alpha = sinf(alpha);
    J->nb = (nb > STOCS_MAX_CONE || !(alpha == alpha)) ? 0 : (int)nb;  // nb <= 56 for any alpha in [0, pi]; NaN alpha -> no samples
}

// STOCS_DEBUG_TIMING: synchronised steps on stderr (tools read them)
#define STOCS_TICK(label)                                                                          \
    if (dbg) { (void)hipStreamSynchronize(c->stream); const double t_ = CallTiming::now_s(); fprintf(stderr, "[stocs congruent] %-18s %8.3f ms\n", label, (t_ - tprev) * 1e3); tprev = t_; }

// device part of stocs_find_congruent_all for one key width
// The stable sort of a pair list by (base, cell).  The lists are base-major already (the gather, and the compaction of the survivors, emit
// base after base), so 32-bit keys go through the library's own SEGMENTED onesweep (sort32.hip, round 5): every base's stretch -- seg_off,
// the per-base offsets on the device -- is sorted by its cell bits alone, two passes whatever the number of bases (rocPRIM over all
// significant bits: three for a single trial's Q list, four for a 40-trial piece).  STOCS_SORT=rocprim keeps rocPRIM's radix_sort_pairs
// selectable for A/B; 64-bit keys (position grids beyond 2^32 (base, cell) values) always take it.  `own` says which one ran: the own sort
// keeps an error word at the start of its temporary block.
static bool cong_sort_own() { static const bool own = !(getenv("STOCS_SORT") && !strcmp(getenv("STOCS_SORT"), "rocprim")); return own; }
static hipError_t cong_sort(void* tmp, size_t& bytes, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout, size_t n, unsigned cell_bits, unsigned end_bit,
                            const uint32_t* seg_off, int n_seg, hipStream_t st, bool* own) {
    *own = cong_sort_own() && n_seg > 0 && n < ((size_t)1 << 30);   // (30-bit prefixes in its look-back words)
#ifdef STOCS_TOOLS_BUILD
    // measurement build: STOCS_DUMP_SORT=<prefix> writes the unsorted list of every sort (header n, n_seg, cell_bits; keys; values; offsets) to
    // <prefix>_<k>.bin -- tools/sort_real.py replays them through stocs_debug_sort_pairs (real key skew, real base lengths)
    if (tmp && getenv("STOCS_DUMP_SORT") && n > 0) {
        static int k_dump = 0;
        (void)hipStreamSynchronize(st);
        std::vector<uint32_t> hk(n), hv(n), ho((size_t)n_seg + 1);
        (void)hipMemcpy(hk.data(), kin, n * 4, hipMemcpyDeviceToHost); (void)hipMemcpy(hv.data(), vin, n * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(ho.data(), seg_off, ((size_t)n_seg + 1) * 4, hipMemcpyDeviceToHost);
        char path[512];
        snprintf(path, sizeof path, "%s_%d.bin", getenv("STOCS_DUMP_SORT"), k_dump++);
        if (FILE* f = fopen(path, "wb")) {
            const uint32_t hdr[4] = {(uint32_t)n, (uint32_t)n_seg, cell_bits, end_bit};
            fwrite(hdr, 4, 4, f); fwrite(hk.data(), 4, n, f); fwrite(hv.data(), 4, n, f); fwrite(ho.data(), 4, (size_t)n_seg + 1, f); fclose(f);
        }
    }
#endif
    return *own ? sort_pairs_own(tmp, bytes, kin, kout, vin, vout, n, 0, cell_bits, seg_off, (uint32_t)n_seg, st) : sort_pairs(tmp, bytes, kin, kout, vin, vout, n, 0, end_bit, st);
}
static hipError_t cong_sort(void* tmp, size_t& bytes, const uint64_t* kin, uint64_t* kout, const uint32_t* vin, uint32_t* vout, size_t n, unsigned, unsigned end_bit,
                            const uint32_t*, int, hipStream_t st, bool* own) {
    *own = false;
    return sort_pairs(tmp, bytes, kin, kout, vin, vout, n, 0, end_bit, st);
}

// the per-trial tables of a planned trial, all in the context's persistent planning buffer (device)
struct PlanDev {
    BaseJob* jobs; Segment* psegs; Segment* qsegs; uint32_t* q_off; uint32_t* p_off; int32_t* bids; unsigned int* err;
    int n_pseg, n_qseg;
};

// The planning buffer of a call with nB bases: jobs | base ids | error words | ranges | range counts | totals | P segments | Q segments |
// p_off | q_off | segment offsets | result.  A lookup is at most 128 ranges, so every region has a bound that depends on nB alone.  The
// host stages the upload (jobs | base ids | error words, at the same offsets) in its pinned block, and the deferred cone records behind it.
struct PlanLayout {
    size_t jobs, bids, err, rng, nr, tot, pseg, qseg, poff, qoff, spo, sqo, out, bytes;   // device
    size_t up, cone, stage;                                                                // pinned staging
    explicit PlanLayout(int nB) {
        const size_t nb = (size_t)nB;
        jobs = 0; bids = jobs + al256(sizeof(BaseJob) * nb); err = bids + al256(16 * nb); rng = err + 256; nr = rng + al256(2 * nb * 128 * 8);
        tot = nr + al256(2 * nb * 4); pseg = tot + al256(2 * nb * 4); qseg = pseg + al256(nb * 128 * sizeof(Segment));
        poff = qseg + al256(nb * 128 * sizeof(Segment)); qoff = poff + al256((nb + 1) * 4); spo = qoff + al256((nb + 2) * 4); sqo = spo + al256((nb + 1) * 4);
        out = sqo + al256((nb + 1) * 4); bytes = out + 256;
        up = err + 256; cone = up; stage = cone + al256(sizeof(float4) * nb);
    }
};

// the layout kernel of the plan: list offsets into the base jobs, segment offsets, totals (launched again by the capacity redo)
static void launch_plan_offsets(hipStream_t st, int nB, char* dpl, const PlanLayout& L, const PlanDev& plan) {
    hipLaunchKernelGGL(plan_offsets_kernel, dim3(1), dim3(1024), 0, st, nB, (const uint2*)(dpl + L.rng), (const uint32_t*)(dpl + L.nr), (const uint32_t*)(dpl + L.tot),
                       plan.jobs, plan.psegs, plan.qsegs, plan.p_off, plan.q_off, (uint32_t*)(dpl + L.spo), (uint32_t*)(dpl + L.sqo), (PlanOut*)(dpl + L.out), plan.err);
}

// The per-call switches of this file (tests and A/B), read once at the top of each call: together with the sizes they decide the form
// the call takes.  (STOCS_SORT and STOCS_GATHER_WGS are read once per process: cong_sort_own, gather_max_wgs.)
struct CongruentSwitches {
    int min_id_bits = 0;                        // STOCS_CONGRUENT_ID_BITS: keeps the wide-id form of the quad keys testable on small models
    int force_streams = 0;                      // 2: STOCS_CONGRUENT_TWO_STREAMS, 1: STOCS_CONGRUENT_ONE_STREAM
    double capacity = 1.6, slack = 1048576.0;   // STOCS_CONGRUENT_CAPACITY: the factor, without slack (below 1 it forces the redo with exact sizes)
    bool wide_keys, keep_all, exact_sizes, distance_gate, no_lds_bits, p_fullsort;   // STOCS_CONGRUENT_<NAME>
    bool debug_streams, debug_timing;           // STOCS_DEBUG_STREAMS (the stream audit), STOCS_DEBUG_TIMING (synchronised steps on stderr)
    static CongruentSwitches read() {
        auto on = [](const char* name) { return getenv(name) != NULL; };
        CongruentSwitches w;
        if (const char* e = getenv("STOCS_CONGRUENT_ID_BITS")) w.min_id_bits = std::min(16, atoi(e));
        w.force_streams = on("STOCS_CONGRUENT_TWO_STREAMS") ? 2 : (on("STOCS_CONGRUENT_ONE_STREAM") ? 1 : 0);
        if (const char* e = getenv("STOCS_CONGRUENT_CAPACITY")) { w.capacity = atof(e); w.slack = 1.0; }
        w.wide_keys = on("STOCS_CONGRUENT_WIDE_KEYS"); w.keep_all = on("STOCS_CONGRUENT_KEEP_ALL"); w.exact_sizes = on("STOCS_CONGRUENT_EXACT_SIZES");
        w.distance_gate = on("STOCS_CONGRUENT_DISTANCE_GATE"); w.no_lds_bits = on("STOCS_CONGRUENT_NO_LDS_BITS"); w.p_fullsort = on("STOCS_CONGRUENT_P_FULLSORT");
        w.debug_streams = on("STOCS_DEBUG_STREAMS"); w.debug_timing = on("STOCS_DEBUG_TIMING");
        return w;
    }
};

// ---- the form of a pass ----
// The key layout of a call: a pure function of the number of bases, the model size, the position grid and the switches.
struct KeyLayout { long long NC; bool use_table; int base_bits, id_bits, cell_bits; bool wide, reduce; };
static KeyLayout key_layout(int nB, int nM, int egSize, const CongruentSwitches& sw) {
    KeyLayout K;
    K.NC = (long long)egSize * egSize * egSize;
    // (8 bytes of run table + 2 of occupancy per (base, cell): up to 2.7 GB -- a trial batch brings thousands of bases, and 288 GB are there for it)
    K.use_table = K.NC > 0 && K.NC * (long long)nB <= (long long)256 * 1024 * 1024;
    K.base_bits = 1; K.id_bits = 1; K.cell_bits = 1;
    while ((1 << K.base_bits) < nB) K.base_bits++;
    while ((1 << K.id_bits) < nM) K.id_bits++;
    K.id_bits = std::max(K.id_bits, sw.min_id_bits);
    {   // cells 0 .. limit-1 plus the all-ones "no cell" value
        const unsigned long long lim = K.use_table ? (unsigned long long)K.NC : ((unsigned long long)1 << 31);
        while (K.cell_bits < 40 && (((unsigned long long)1 << K.cell_bits) - 1ull) < lim) K.cell_bits++;
    }
    K.wide = K.base_bits + K.cell_bits > 32 || sw.wide_keys;
    // both pair lists are reduced to the entries with a partner cell when one byte per (base, cell) is a small table (CountPass::reduce_lists)
    K.reduce = K.use_table && ((unsigned long long)nB << K.cell_bits) <= (1ull << 29) && !sw.keep_all;
    return K;
}

// The form ONE count pass takes, decided here and nowhere else: from the key layout, the switches and the list sizes of THIS pass (nP, nQ:
// capacities when the pass is optimistic, exact sizes otherwise -- so the first pass and the redo of an outgrown plan may differ in
// one_stream).  It also owns the strings that name the form in the call's timing record.
struct PassForm {
    bool wide, use_table, reduce, one_stream;
    bool optimistic;              // sized by capacities: the kernels read the planned totals from the device (d_po)
    uint32_t lds_words;           // one base's occupancy bits in LDS (gather: collected there; count: the other list's, tested there) while they fit 32 KB
    unsigned end_bit, end_bit_p;  // bits the Q sort and the P sort look at
    hipStream_t st, sq;           // P's stream (the context's) and Q's (the auxiliary one when the pass has two streams)
    int s0, s1;                   // their indices in the stream audit
    bool two_streams() const { return sq != st; }
    int audit_stream(int side) const { return side ? s1 : s0; }
    const char* reserve_label() const { return !use_table ? "arena reserve (no run table, 64-bit keys)" : (wide ? "arena reserve (64-bit keys)" : "arena reserve"); }
    const char* enqueue_label() const { return reduce ? "enqueue compact/sort/records/join/scan" : "enqueue gather/sort/records/join/scan"; }
    const char* clock_label(const char* all, const char* red, const char* one) const { return one_stream ? one : (reduce ? red : all); }   // (NULL: not a group of this form)
};
static PassForm pass_form(const stocs_ctx* c, const KeyLayout& K, const CongruentSwitches& sw, int nB, size_t nP, size_t nQ, bool optimistic) {
    PassForm F;
    F.wide = K.wide; F.use_table = K.use_table; F.reduce = K.reduce; F.optimistic = optimistic;
    // ONE stream (round 5b) for the reduced 32-bit form: P and Q go through every step in the SAME launch (blockIdx.y), the survivors of both
    // land in one list and ONE segmented sort over 2 nB segments sorts it.  The two-stream form of rounds 3-5a (P on the context's stream, Q on
    // the auxiliary one) paid ~11 us per event edge between the streams, five of them in a trial -- a tenth of a Cm trial's congruent phase;
    // it stays for 64-bit keys, unreduced lists and rocPRIM's sort, and under STOCS_CONGRUENT_TWO_STREAMS for A/B.
    // Lists beyond 10^8 entries -- the pieces of a trial batch at the metric size -- keep the two streams: there the edges are nothing and the
    // overlap of unlike kernels (P's records next to Q's sort) is worth 2 % (64 Cm trials: 2 040 against 1 985 trials/s).
    F.one_stream = K.reduce && !K.wide && cong_sort_own() && (nP + nQ) < ((size_t)1 << 30) && nB < (1 << 22) && sw.force_streams != 2 &&
                   (sw.force_streams == 1 || nP + nQ < (size_t)100000000);
    F.st = c->stream;
    F.sq = (c->aux_stream && !F.one_stream) ? c->aux_stream : c->stream;
    F.s0 = 0; F.s1 = F.sq != F.st ? 1 : 0;
    F.lds_words = (K.cell_bits >= 5 && K.cell_bits <= 18 && !sw.no_lds_bits) ? (1u << (K.cell_bits - 5)) : 0u;
    F.end_bit = (unsigned)(K.cell_bits + K.base_bits);
    // P side with the run table: sorted by position cell ALONE.  The gather emits base after base and the sort is stable, so
    // inside a cell the entries stay grouped by base, in index order inside a base: the runs of (base, cell) are contiguous
    // all the same, the table finds them wherever they are, and 15 bits are two radix passes where 22 are three.
    F.end_bit_p = (K.use_table && !sw.p_fullsort) ? (unsigned)K.cell_bits : F.end_bit;
    return F;
}

// ---- the list kernels of a pass: one launch helper, one declaration ----
enum ListKernel { LIST_GATHER, LIST_COUNT, LIST_COMPACT };
// what the list kernels of one pass are given: the two records and the pass's constants
template <class KeyT>
struct ListPass {
    ListSide<KeyT> side[2];
    const uint32_t* pairs; const BaseJob* jobs; const float4* munit; int cell_bits; long long cell_limit; const PlanOut* d_po; uint32_t lds_words; int nB;
    const uint32_t* p_off; const uint32_t* q_off; uint32_t* comb_off;   // the combined compaction: the lists' offsets per base, the segment offsets of the one sort
};
// the buffers of a list and its steps as the stream audit names them
struct ListNames { const char *segs, *keys, *vals, *occ, *tiles, *alive, *okeys, *ovals, *gather, *count, *compact; };
static const ListNames LIST_NAMES[2] = {
    {"P segments", "gathered P keys", "gathered P pairs", "occupancy of P", "tile counts of P", "alive bits of P", "surviving P keys", "surviving P pairs",
     "gather P", "survivors count P", "compact P"},
    {"Q segments", "gathered Q keys", "gathered Q pairs", "occupancy of Q", "tile counts of Q", "alive bits of Q", "surviving Q keys", "surviving Q pairs",
     "gather Q", "survivors count Q", "compact Q"}};

// ONE launch of a list kernel for the lists side0 .. side0 + ny - 1 on the stream with audit index s, and what it reads and writes declared to
// the stream audit from the records the kernel was given.  The grid is the largest any of its lists asks for (a workgroup beyond a list's
// end leaves at once); both lists compacted in one launch go into ONE list (the third plane writes its segment offsets).
template <class KeyT>
static void launch_list_kernel(stocs_ctx* c, ListKernel k, const ListPass<KeyT>& A, int side0, int ny, int s) {
    const ListSide<KeyT>&P = A.side[0], &Q = A.side[1];
    hipStream_t stream = ctx_stream(c, s);
    unsigned gx = 1u;
    for (int y = side0; y < side0 + ny; ++y) {
        const uint32_t groups = (uint32_t)((((size_t)A.side[y].n + SURV_TILE - 1) / SURV_TILE + 3) / 4);     // four tiles of survivors per workgroup and trip
        gx = std::max(gx, k == LIST_GATHER ? gather_grid(A.side[y].n) : (k == LIST_COUNT ? std::min(groups, GATHER_MAX_WGS) : groups));
    }
    const int combined = (k == LIST_COMPACT && ny == 2) ? 1 : 0;
    switch (k) {
    case LIST_GATHER:
        hipLaunchKernelGGL(gather_key_kernel<KeyT>, dim3(gx, (unsigned)ny), dim3(256), A.lds_words * 4, stream, A.pairs, P, Q, side0, A.jobs, A.munit, A.cell_bits, A.cell_limit, A.d_po,
                           A.lds_words, (uint32_t)A.nB);
        break;
    case LIST_COUNT:
        hipLaunchKernelGGL(survivors_count_kernel<KeyT>, dim3(gx, (unsigned)ny), dim3(256), A.lds_words * 4, stream, P, Q, side0, A.d_po, A.lds_words, A.cell_bits);
        break;
    case LIST_COMPACT:
        hipLaunchKernelGGL(survivors_compact_kernel<KeyT>, dim3(gx, (unsigned)(ny + combined)), dim3(256), 0, stream, P, Q, side0, combined, A.d_po, A.p_off, A.q_off, A.nB, A.comb_off);
        break;
    }
    for (int y = side0; y < side0 + ny; ++y) {
        const ListSide<KeyT>& X = A.side[y];
        const ListNames& N = LIST_NAMES[y];
        switch (k) {
        case LIST_GATHER: c->audit.step(s, N.gather, {{X.segs, N.segs}, {A.jobs, "base jobs"}}, {{X.keys, N.keys}, {X.vals, N.vals}, {X.occ, N.occ}}); break;
        case LIST_COUNT: c->audit.step(s, N.count, {{X.keys, N.keys}, {X.other, LIST_NAMES[1 - y].occ}}, {{X.tiles, N.tiles}, {X.alive, N.alive}}); break;
        case LIST_COMPACT: c->audit.step(s, N.compact, {{X.keys, N.keys}, {X.vals, N.vals}, {X.alive, N.alive}, {X.tiles, N.tiles}}, {{X.okeys, N.okeys}, {X.ovals, N.ovals}}); break;
        }
    }
}

// One step for BOTH lists, in the form of the pass.  One stream: ONE launch with gridDim.y == 2 on the context's stream.  Otherwise one launch
// per list, `first`'s list first, P on the context's stream and Q on the pass's second one -- the order of the two enqueues is the caller's
// and matters (the side enqueued second starts later).  after(side) follows each list's launch (the one launch for both: both calls behind it,
// in the same order): the events a list's step is followed by.
template <class KeyT, class After>
static int issue_lists(stocs_ctx* c, const PassForm& F, ListKernel k, const ListPass<KeyT>& A, int first, After after) {
    int rc;
    if (F.one_stream) {
        launch_list_kernel(c, k, A, 0, 2, F.s0);
        if ((rc = after(first)) || (rc = after(1 - first))) return rc;
        return STOCS_OK;
    }
    for (int i = 0; i < 2; ++i) {
        const int side = i ? 1 - first : first;
        launch_list_kernel(c, k, A, side, 1, F.audit_stream(side));
        if ((rc = after(side))) return rc;
    }
    return STOCS_OK;
}

// One cong_sort call, described once: the size query and the run take it from here.  An inactive descriptor (the Q sort of the one-stream
// form, whose list is sorted as the second half of P's) does nothing and needs no bytes.
struct SortNames { const char *what, *kin, *vin, *seg, *kout, *vout, *tmp; };
static const SortNames SORT_NAMES[2] = {
    {"sort P", "P keys to sort", "P pairs to sort", "P offsets per base", "sorted P keys", "sorted P pairs", "sort scratch P"},
    {"sort Q", "Q keys to sort", "Q pairs to sort", "Q offsets per base", "sorted Q keys", "sorted Q pairs", "sort scratch Q"}};
template <class KeyT>
struct SortCall {
    bool active;
    const KeyT* kin; KeyT* kout; const uint32_t* vin; uint32_t* vout; size_t n; unsigned cell_bits, end_bit; const uint32_t* seg_off; int n_seg;
    int s;               // audit index of its stream
    size_t bytes;        // of temporary storage (bytes_needed)
    bool own;            // the library's own sort runs (decided per list: by its length per base): its error word is read back
    char* tmp;
    hipError_t bytes_needed(stocs_ctx* c) { bytes = 0; own = false; return active ? cong_sort(NULL, bytes, kin, kout, vin, vout, n, cell_bits, end_bit, seg_off, n_seg, ctx_stream(c, s), &own) : hipSuccess; }
    hipError_t run(stocs_ctx* c, int side, char* t) {
        tmp = t;
        if (!active) return hipSuccess;
        const hipError_t e = cong_sort(tmp, bytes, kin, kout, vin, vout, n, cell_bits, end_bit, seg_off, n_seg, ctx_stream(c, s), &own);
        const SortNames& N = SORT_NAMES[side];
        c->audit.step(s, N.what, {{kin, N.kin}, {vin, N.vin}, {seg_off, N.seg}}, {{kout, N.kout}, {vout, N.vout}, {tmp, N.tmp}});
        return e;
    }
    // the own sort keeps an error word at the start of its temporary block (a look-back wait that ran into its bound)
    hipError_t read_error(uint32_t* pinned, hipStream_t st) const { return (active && own) ? hipMemcpyAsync(pinned, tmp + sort_own_err_offset(), 4, hipMemcpyDeviceToHost, st) : hipSuccess; }
};

// ---- one count pass ----
// The count pass over the planned lists: (reduce_lists,) sorts, P records and run table, join count, scan, per-base quad offsets -- a short
// list of stages (run) over the state they share.
// F.optimistic: the host has NOT read the plan -- S->totP / S->totQ are capacities the buffers and launches are sized by, the kernels read
// the planned totals from *d_po, and the plan's totals arrive with the survivors' in ONE read-back (po_pin).  *outgrown (not an error) when
// the plan turned out larger than the capacities: the caller redoes the pass with the exact sizes it now knows.
template <class KeyT>
struct CountPass {
    stocs_ctx* const c; CongruentState* const S; const PlanDev& plan; const PassForm& F; double& tprev;
    const PlanOut* const d_po; const PlanOut* const po_pin;   // the plan's totals on the device and in the pinned block (NULL unless F.optimistic)
    const bool dbg;
    // The device's own clock of the kernel groups (HIP events between them, reported by stocs_last_call_timing as "device: ..." steps) is
    // OPT-IN since round 5b (stocs_set_option "device_clock" / STOCS_DEVICE_CLOCK=1): on this runtime every event recorded between two kernels
    // of a stream leaves the queue idle for ~5 us, and the nine of a call were 45 us of a Cm trial's 600.  The host's steps between the call's
    // own synchronisation points are always recorded.
    const bool dev_clock;
    const int nB;
    const size_t nP0, nQ0;   // the gathered lists as planned (F.optimistic: their capacities)
    size_t nP, nQ;           // the lists that are sorted and joined (the survivors, when the lists are reduced)
    hipStream_t const st;
    StreamAudit& AU;         // STOCS_DEBUG_STREAMS: every step below says what it reads and writes
    ListPass<KeyT> A;
    // the pair lists as gathered and, when they are reduced, their survivors (ONE buffer for both lists in the one-stream form: Q's behind P's)
    DevBuf<KeyT> pk_raw, qk_raw, pk_c, qk_c;
    DevBuf<uint32_t> pv_raw, qv_raw, pv_c, qv_c, comb_off;
    DevBuf<uint32_t> d_surv;                             // one zeroed block: occupancy of P | occupancy of Q | P tile counts (+ total) | Q tile counts (+ total)
    DevBuf<unsigned long long> d_bits_p, d_bits_q;       // one bit per gathered entry: survives (written by the count, read by the compaction)
    size_t n_surv_words = 0;
    uint32_t ntp = 0, ntq = 0;                           // tiles of the gathered lists
    SortCall<KeyT> sort_p, sort_q;
    DevBuf<char> d_tmp_p, d_tmp_q;
    uint32_t* sort_err_pin = NULL;

    CountPass(stocs_ctx* c_, CongruentState* S_, const PlanDev& plan_, const PassForm& F_, bool dbg_, double& tprev_, const PlanOut* d_po_, const PlanOut* po_pin_)
        : c(c_), S(S_), plan(plan_), F(F_), tprev(tprev_), d_po(d_po_), po_pin(po_pin_), dbg(dbg_), dev_clock(c_->device_clock != 0), nB(S_->nB), nP0(S_->totP), nQ0(S_->totQ),
          nP(S_->totP), nQ(S_->totQ), st(c_->stream), AU(c_->audit) {}

    int clock_stamp(CongEvent e, hipStream_t s) { if (dev_clock) STOCS_HIP_CHECK(hipEventRecord(c->ev_t[e], s)); return STOCS_OK; }
    // main -> aux: what the context's stream holds now comes before whatever the second stream is given next (nothing to do with one stream)
    int fork() { return F.two_streams() ? stream_edge(c, c->ev_fork, F.s0, F.s1) : STOCS_OK; }
    int run_deferred(const char* label) {
        if (!S->deferred) return STOCS_OK;
        const int rd = S->deferred();
        S->deferred = nullptr;
        if (rd) return rd;
        c->timing[TIMING_CONGRUENT].lap(label);
        return STOCS_OK;
    }

    // -- stage: the pass's lists and the records its kernels are given (every buffer the records name is allocated here) --
    int allocate_lists() {
        int rc;
        if ((rc = pk_raw.alloc(nP0)) || (rc = pv_raw.alloc(nP0)) || (rc = qk_raw.alloc(nQ0)) || (rc = qv_raw.alloc(nQ0))) return rc;
        S->d_jobs.p = plan.jobs; S->d_qoff.p = plan.q_off; S->d_bids.p = plan.bids; S->d_err.p = plan.err;
        memset(&A, 0, sizeof A);
        A.pairs = c->index.d_pairs; A.jobs = plan.jobs; A.munit = c->d_munit; A.cell_bits = S->cell_bits; A.cell_limit = S->use_table ? S->NC : ((long long)1 << 31);
        A.nB = nB; A.p_off = plan.p_off; A.q_off = plan.q_off;
        ListSide<KeyT>&P = A.side[0], &Q = A.side[1];
        P.segs = plan.psegs; P.nseg = plan.n_pseg; P.n = (uint32_t)nP0; P.keys = pk_raw.p; P.vals = pv_raw.p;
        Q.segs = plan.qsegs; Q.nseg = plan.n_qseg; Q.n = (uint32_t)nQ0; Q.keys = qk_raw.p; Q.vals = qv_raw.p;
        if (!F.reduce) return STOCS_OK;       // (the unreduced gather: no occupancy, no plan on the device, no LDS words)
        A.d_po = d_po; A.lds_words = F.lds_words;
        const size_t W = (size_t)((((unsigned long long)nB << S->cell_bits) + 31) >> 5) + 1;   // words of one occupancy table: one bit per (base, cell) value
        ntp = (uint32_t)((nP0 + SURV_TILE - 1) / SURV_TILE); ntq = (uint32_t)((nQ0 + SURV_TILE - 1) / SURV_TILE);
        const size_t o_tp = 2 * W, o_tq = o_tp + ntp + 1;
        n_surv_words = o_tq + ntq + 1;
        if ((rc = d_surv.alloc(n_surv_words))) return rc;
        if ((rc = d_bits_p.alloc((size_t)std::max(ntp, 1u) * (SURV_TILE / 64))) || (rc = d_bits_q.alloc((size_t)std::max(ntq, 1u) * (SURV_TILE / 64)))) return rc;
        // the compacted lists are sized by the gathered ones (the survivors' totals are what the host waits for while they are written)
        if (F.one_stream) { if ((rc = pk_c.alloc(nP0 + nQ0)) || (rc = pv_c.alloc(nP0 + nQ0)) || (rc = comb_off.alloc(2 * (size_t)nB + 1))) return rc; }
        else if ((rc = pk_c.alloc(nP0)) || (rc = pv_c.alloc(nP0)) || (rc = qk_c.alloc(nQ0)) || (rc = qv_c.alloc(nQ0))) return rc;
        A.comb_off = comb_off.p;
        P.occ = d_surv.p; Q.occ = d_surv.p + W; P.other = Q.occ; Q.other = P.occ;
        P.tiles = d_surv.p + o_tp; Q.tiles = d_surv.p + o_tq; P.alive = d_bits_p.p; Q.alive = d_bits_q.p;
        P.okeys = pk_c.p; P.ovals = pv_c.p;
        Q.okeys = F.one_stream ? pk_c.p : qk_c.p; Q.ovals = F.one_stream ? pv_c.p : qv_c.p;      // (one list: the kernel puts Q's survivors behind P's)
        return STOCS_OK;
    }

    // -- stages of the reduced form: gather -> occupancy -> survivor counts -> tile scan -> compaction of both lists, and the read-back of the
    //    survivors' offsets and totals.  In every two-list step Q is enqueued first. --
    int zero_fill_and_fork() {
        const ListSide<KeyT>&P = A.side[0], &Q = A.side[1];
        hipLaunchKernelGGL(zero_u32_kernel, dim3((unsigned)((n_surv_words + 255) / 256)), dim3(256), 0, st, d_surv.p, n_surv_words, (uint32_t*)NULL);
        AU.step(F.s0, "zero fill", {}, {{P.occ, LIST_NAMES[0].occ}, {Q.occ, LIST_NAMES[1].occ}, {P.tiles, LIST_NAMES[0].tiles}, {Q.tiles, LIST_NAMES[1].tiles}});
        int rc = clock_stamp(EV_REDUCE_BEGIN, st);
        return rc ? rc : fork();          // the plan upload, the plan kernels and the zero fill are on st
    }
    int gather() {
        // each list's cells are marked behind its gather: the OTHER list's count waits for that (two streams: the cross edges below)
        int rc = issue_lists(c, F, LIST_GATHER, A, 1, [&](int side) -> int {
            return (F.two_streams() || dev_clock) ? stream_edge_record(c, c->ev_t[side ? EV_Q_MARKED : EV_P_MARKED], F.audit_stream(side)) : STOCS_OK;
        });
        if (rc || !F.two_streams()) return rc;
        if ((rc = stream_edge_wait(c, c->ev_t[EV_P_MARKED], F.s1))) return rc;
        return stream_edge_wait(c, c->ev_t[EV_Q_MARKED], F.s0);
    }
    int count() {
        const int rc = issue_lists(c, F, LIST_COUNT, A, 1, [&](int side) -> int { return (side == 1 && F.two_streams()) ? stream_edge_record(c, c->ev_join, F.s1) : STOCS_OK; });
        if (rc || !F.two_streams()) return rc;
        return stream_edge_wait(c, c->ev_join, F.s0);       // the scan below reads both lists' counts
    }
    int tile_scan() {
        const ListSide<KeyT>&P = A.side[0], &Q = A.side[1];
        AU.step(F.s0, "tile scan", {}, {{P.tiles, LIST_NAMES[0].tiles}, {Q.tiles, LIST_NAMES[1].tiles}});
        if (std::max(ntp, ntq) + 1u <= 2u * TSCAN) {
            hipLaunchKernelGGL(survivors_scan_kernel, dim3(2), dim3(1024), 0, st, P.tiles, ntp, Q.tiles, ntq);
            return STOCS_OK;
        }
        // long lists (trial batches): the scan on many workgroups
        const uint32_t pp = (ntp + 1u + TSCAN - 1u) / TSCAN, pq = (ntq + 1u + TSCAN - 1u) / TSCAN;
        DevBuf<uint32_t> d_part;
        const int rc = d_part.alloc((size_t)pp + pq);
        if (rc) return rc;
        hipLaunchKernelGGL(tile_scan_local_kernel, dim3(std::max(pp, pq), 2), dim3(256), 0, st, P.tiles, ntp + 1u, Q.tiles, ntq + 1u, d_part.p, pp);
        hipLaunchKernelGGL(tile_scan_add_kernel, dim3(std::max(pp, pq), 2), dim3(256), 0, st, P.tiles, ntp + 1u, Q.tiles, ntq + 1u, (const uint32_t*)d_part.p, pp);
        return STOCS_OK;
    }
    uint32_t* qoff_pin() const { return (uint32_t*)((char*)c->h_pin + PIN_VAR + 8 * ((size_t)nB + 1)); }
    int base_offsets_and_read_back() {
        const ListSide<KeyT>&P = A.side[0], &Q = A.side[1];
        AU.step(F.s0, "base offsets", {{P.keys, LIST_NAMES[0].keys}, {Q.keys, LIST_NAMES[1].keys}, {P.occ, LIST_NAMES[0].occ}, {Q.occ, LIST_NAMES[1].occ}},
                {{plan.jobs, "base jobs"}, {plan.q_off, "Q offsets per base"}});
        hipLaunchKernelGGL(survivors_base_offsets_kernel<KeyT>, dim3((unsigned)nB, 2), dim3(256), 0, st, (const KeyT*)P.keys, P.n, (const uint32_t*)Q.occ, (const uint32_t*)P.tiles,
                           (const KeyT*)Q.keys, Q.n, (const uint32_t*)P.occ, (const uint32_t*)Q.tiles, nB, S->d_jobs.p, plan.p_off, plan.q_off, d_po);
        STOCS_HIP_CHECK(hipGetLastError());
        // the host sizes the sorts and the join with the survivors' totals and lays the materialise blocks out with their Q offsets
        STOCS_HIP_CHECK(hipMemcpyAsync(qoff_pin(), plan.q_off, 4 * ((size_t)nB + 2), hipMemcpyDeviceToHost, st));   // Q offsets, Q total, P total
        return stream_edge_record(c, c->ev_t[EV_SURVIVORS_READ], F.s0);
    }
    int compact() {
        // the survivors move behind their tiles' offsets while the host waits for the totals
        int rc = fork();                  // tile offsets are scanned on st
        if (rc || (rc = issue_lists(c, F, LIST_COMPACT, A, 1, [](int) -> int { return STOCS_OK; }))) return rc;
        STOCS_HIP_CHECK(hipGetLastError());
        c->timing[TIMING_CONGRUENT].lap("enqueue gather + occupancy + survivor counts");
        return STOCS_OK;
    }
    int deferred_records_and_wait() {
        const int rc = run_deferred("host: cone records of the bases (while the device gathers)");
        if (rc) return rc;
        STOCS_HIP_CHECK(hipEventSynchronize(c->ev_t[EV_SURVIVORS_READ]));   // the read-back, not the compaction behind it
        AU.host_sync_event(c->ev_t[EV_SURVIVORS_READ]);
        c->timing[TIMING_CONGRUENT].lap("wait for the device (survivors)");
        return STOCS_OK;
    }
    // the plan's own totals came with the read-back: were the capacities enough?  If not the streams are idle on return.
    int capacity_check(bool* outgrown) {
        if (!po_pin || !(po_pin->overflow || po_pin->totP > (unsigned long long)nP0 || po_pin->totQ > (unsigned long long)nQ0)) return STOCS_OK;
        STOCS_HIP_CHECK(hipStreamSynchronize(st));            // the compaction behind the read-back: nothing may still touch the arena
        if (F.two_streams()) STOCS_HIP_CHECK(hipStreamSynchronize(F.sq));
        AU.host_sync(F.s0); AU.host_sync(F.s1);
        *outgrown = true;
        return STOCS_OK;
    }
    // S->totP, S->totQ, S->h_qoff of the survivors; S->no_quads when no cell is shared
    int reduce_lists(bool* outgrown) {
        int rc;
        if ((rc = zero_fill_and_fork()) || (rc = gather()) || (rc = count()) || (rc = tile_scan()) || (rc = base_offsets_and_read_back()) || (rc = compact()) ||
            (rc = deferred_records_and_wait()) || (rc = capacity_check(outgrown)) || *outgrown)
            return rc;
        const uint32_t* pin = qoff_pin();
        nP = pin[nB + 1]; nQ = pin[nB];
        memcpy(S->h_qoff.data(), pin, 4 * ((size_t)nB + 1));
        if (dbg) fprintf(stderr, "[stocs congruent] survivors: P %zu of %zu, Q %zu of %zu\n", nP, nP0, nQ, nQ0);
        S->totP = (uint32_t)nP; S->totQ = (uint32_t)nQ;
        if (nP == 0 || nQ == 0) S->no_quads = true;   // no cell is shared: no quads (quad_off is all zero already)
        return STOCS_OK;
    }

    // -- stage: the sorted lists and the sorts that fill them --
    int prepare_sorts() {
        int rc;
        const ListSide<KeyT>&P = A.side[0], &Q = A.side[1];
        const KeyT* pk_in = F.reduce ? P.okeys : P.keys; const uint32_t* pv_in = F.reduce ? P.ovals : P.vals;    // what the sorts read
        const KeyT* qk_in = F.reduce ? Q.okeys : Q.keys; const uint32_t* qv_in = F.reduce ? Q.ovals : Q.vals;
        if (F.one_stream) {   // one sorted list: P's part, then Q's
            if ((rc = S->d_pkeys.alloc((nP + nQ) * sizeof(KeyT))) || (rc = S->d_pvals.alloc(nP + nQ))) return rc;
            S->d_qkeys.p = S->d_pkeys.p + nP * sizeof(KeyT); S->d_qvals.p = S->d_pvals.p + nP;
        } else if ((rc = S->d_pkeys.alloc(nP * sizeof(KeyT))) || (rc = S->d_pvals.alloc(nP)) || (rc = S->d_qkeys.alloc(nQ * sizeof(KeyT))) || (rc = S->d_qvals.alloc(nQ)))
            return rc;
        if ((rc = S->d_prec.alloc(S->close_cells ? 1 : nP)) || (rc = S->d_pdc.alloc(((size_t)nP + 15) & ~(size_t)7))) return rc;
        // one stable sort per list: (base, position cell); inside a cell the entries keep the index order of the gather.  One stream: ONE
        // sort of the combined list, its 2 nB segments P's bases and then Q's.
        const unsigned cb = (unsigned)S->cell_bits;
        if (F.one_stream) sort_p = {true, pk_in, (KeyT*)S->d_pkeys.p, pv_in, S->d_pvals.p, nP + nQ, cb, F.end_bit_p, comb_off.p, 2 * nB, F.s0, 0, false, NULL};
        else sort_p = {true, pk_in, (KeyT*)S->d_pkeys.p, pv_in, S->d_pvals.p, nP, cb, F.end_bit_p, plan.p_off, nB, F.s0, 0, false, NULL};
        sort_q = {!F.one_stream, qk_in, (KeyT*)S->d_qkeys.p, qv_in, S->d_qvals.p, nQ, cb, F.end_bit, plan.q_off, nB, F.s1, 0, false, NULL};
        STOCS_HIP_CHECK(sort_p.bytes_needed(c));
        STOCS_HIP_CHECK(sort_q.bytes_needed(c));
        if ((rc = d_tmp_p.alloc(sort_p.bytes)) || (rc = d_tmp_q.alloc(sort_q.bytes))) return rc;
        return STOCS_OK;
    }
    // The P side (sort, records) and the Q side (sort) are independent until the join: the Q side runs on the pass's second stream next to
    // the P side (a radix pass of 7 M pairs moves ~1.8 TB/s: two of them share the chip).
    // The P side first: it is the longer chain (sort + records: ~100 us at Cm against ~70 us of the Q sort), and whichever side is enqueued second
    // starts ~25 us later -- the host needs that long for the first side's five launches (kernel trace of a trial, round 5)
    int p_side() {
        int rc;
        if (!F.reduce) launch_list_kernel(c, LIST_GATHER, A, 0, 1, F.s0);
        STOCS_HIP_CHECK(hipGetLastError());
        STOCS_HIP_CHECK(sort_p.run(c, 0, d_tmp_p.p));
        if ((rc = clock_stamp(EV_P_SORTED, st))) return rc;
        if (S->use_table) {
            const size_t ncell = (size_t)(S->NC * nB);
            if ((rc = S->d_cfirst.alloc(ncell)) || (rc = S->d_cend.alloc(ncell))) return rc;
            // the table is read at the cells of the Q entries only: in the reduced lists every such cell holds P entries, so the
            // records kernel writes every slot that is read and the 8 bytes per (base, cell) need no zero fill
            if (!F.reduce) hipLaunchKernelGGL(zero_u32_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, st, S->d_cfirst.p, ncell, S->d_cend.p);
        }
        hipLaunchKernelGGL(p_records_kernel<KeyT>, dim3((unsigned)((nP + 1023) / 1024)), dim3(256), 0, st, (const KeyT*)S->d_pkeys.p, S->d_pvals.p, (uint32_t)nP,
                           S->cell_bits, S->NC, S->d_jobs.p, c->d_munit, c->d_mpos, S->nepsilon, S->close_cells ? (float4*)NULL : S->d_prec.p, S->close_cells ? S->d_pdc.p : (uint16_t*)NULL,
                           S->use_table ? S->d_cfirst.p : (uint32_t*)NULL,
                           S->use_table ? S->d_cend.p : (uint32_t*)NULL);
        STOCS_HIP_CHECK(hipGetLastError());
        AU.step(F.s0, "P records", {{S->d_pkeys.p, SORT_NAMES[0].kout}, {S->d_pvals.p, SORT_NAMES[0].vout}, {plan.jobs, "base jobs"}}, {{S->d_prec.p, "P records"}, {S->d_pdc.p, "P direction cells"}});
        return STOCS_OK;
    }
    int q_side_and_join_streams() {
        int rc;
        if (!F.reduce) launch_list_kernel(c, LIST_GATHER, A, 1, 1, F.s1);
        STOCS_HIP_CHECK(sort_q.run(c, 1, d_tmp_q.p));
        if ((rc = clock_stamp(EV_Q_SORTED, F.sq))) return rc;
        if (F.two_streams() && (rc = stream_edge(c, c->ev_join, F.s1, F.s0))) return rc;   // the join needs both sides
        return clock_stamp(EV_SIDES_JOINED, st);
    }
    // join: count pass + exclusive scan.  The quads themselves are produced on demand (materialise / resolve_picks_kernel)
    int join_count_and_scan() {
        int rc;
        AU.step(F.s0, "join count", {{S->d_qkeys.p, SORT_NAMES[1].kout}, {S->d_qvals.p, SORT_NAMES[1].vout}, {plan.jobs, "base jobs"}}, {});
        DevBuf<unsigned long long> d_qcnt;   // 64-bit: the total can exceed 2^32
        if ((rc = d_qcnt.alloc(nQ + 1)) || (rc = S->d_qoffe.alloc(nQ + 1))) return rc;
        hipLaunchKernelGGL(join_count_kernel<KeyT>, dim3((unsigned)((nQ + 255) / 256)), dim3(256), 0, st, S->template args<KeyT>(c), d_qcnt.p);
        STOCS_HIP_CHECK(hipGetLastError());
        if ((rc = clock_stamp(EV_JOIN_COUNTED, st))) return rc;
        size_t tmp_scan = 0;
        STOCS_HIP_CHECK(exclusive_scan(NULL, tmp_scan, d_qcnt.p, S->d_qoffe.p, nQ + 1, st));
        DevBuf<char> d_tmp_scan;
        if ((rc = d_tmp_scan.alloc(tmp_scan))) return rc;
        STOCS_HIP_CHECK(exclusive_scan(d_tmp_scan.p, tmp_scan, d_qcnt.p, S->d_qoffe.p, nQ + 1, st));
        return STOCS_OK;
    }
    unsigned long long* quad_off_pin() const { return (unsigned long long*)((char*)c->h_pin + PIN_VAR); }   // pinned (sized by the caller)
    int enqueue_read_back() {
        int rc;
        // per-base offsets = scan value at the first Q entry of each base
        DevBuf<unsigned long long> d_boff;
        if ((rc = d_boff.alloc(nB + 1))) return rc;
        hipLaunchKernelGGL(base_offsets_kernel, dim3((unsigned)((nB + 1 + 255) / 256)), dim3(256), 0, st, S->d_qoffe.p, S->d_qoff.p, nB + 1, d_boff.p);
        STOCS_HIP_CHECK(hipGetLastError());
        STOCS_HIP_CHECK(hipMemcpyAsync(quad_off_pin(), d_boff.p, 8 * (size_t)(nB + 1), hipMemcpyDeviceToHost, st));
        sort_err_pin = (uint32_t*)((char*)c->h_pin + PIN_CONGRUENT + 128);   // the own sort's error words
        sort_err_pin[0] = sort_err_pin[1] = 0u;
        // (both sorts are joined into st by now)
        STOCS_HIP_CHECK(sort_p.read_error(&sort_err_pin[0], st));
        STOCS_HIP_CHECK(sort_q.read_error(&sort_err_pin[1], st));
        if ((rc = clock_stamp(EV_PASS_END, st))) return rc;
        c->timing[TIMING_CONGRUENT].lap(F.enqueue_label());
        return STOCS_OK;
    }
    int wait_and_clock_rows() {
        STOCS_HIP_CHECK(hipStreamSynchronize(st));
        AU.host_sync(F.s0);
        c->timing[TIMING_CONGRUENT].lap("wait for the device (counts)");
        // the device's own account of that wait (every event has completed: the stream is idle, the Q side was joined into it): a group
        // between two clock stamps per row, named per form (PassForm::clock_label)
        static const struct { CongEvent from, to; const char *all, *red, *one; } groups[] = {
            {EV_REDUCE_BEGIN, EV_SURVIVORS_READ, NULL, "device: gathers + occupancy + survivor counts (both lists)", "device: gathers + occupancy + survivor counts (both lists in every launch)"},
            {EV_SORT_BEGIN, EV_Q_SORTED, "device: Q gather + sort (aux stream, from the fork)", "device: Q sort (aux stream, from the fork; its compaction ran during the wait)", NULL},
            {EV_SORT_BEGIN, EV_P_SORTED, "device: P gather + sort", "device: P sort", "device: sort (P and Q as one list of 2 nB segments)"},
            {EV_P_SORTED, EV_SIDES_JOINED, "device: P records + wait for Q", "device: P records + wait for Q", "device: P records"},
            {EV_SIDES_JOINED, EV_JOIN_COUNTED, "device: join count", "device: join count", "device: join count"},
            {EV_JOIN_COUNTED, EV_PASS_END, "device: scan + offsets + read-back", "device: scan + offsets + read-back", "device: scan + offsets + read-back"}};
        CallTiming& T = c->timing[TIMING_CONGRUENT];
        for (const auto& g : groups) {
            const char* what = F.clock_label(g.all, g.red, g.one);
            if (!dev_clock || !what || T.n >= CallTiming::MAX_STEPS) continue;
            float ms = -1.0f;
            if (hipEventElapsedTime(&ms, c->ev_t[g.from], c->ev_t[g.to]) != hipSuccess) ms = -1.0f;
            T.label[T.n] = what; T.ms[T.n] = (double)ms; ++T.n;
        }
        T.t_last = CallTiming::now_s();
        return STOCS_OK;
    }

    int run(bool* outgrown) {
        *outgrown = false;
        int rc;
        if ((rc = allocate_lists())) return rc;
        if (!F.reduce && (rc = run_deferred("host: cone records of the bases (no survivors pass to hide them behind)"))) return rc;
        if (F.reduce && ((rc = reduce_lists(outgrown)) || *outgrown || S->no_quads)) return rc;
        if ((rc = prepare_sorts())) return rc;
        // device-side clock of the groups below (HIP events on the streams they run on; read after the call's closing
        // synchronisation): a call that takes 70 ms instead of 1 then says which group of kernels it spent them in
        if ((rc = clock_stamp(EV_SORT_BEGIN, st)) || (rc = fork())) return rc;       // (the fork: the upload and the plan are on st)
        if ((rc = p_side()) || (rc = q_side_and_join_streams())) return rc;
        STOCS_TICK("gather+sort+records")
        if ((rc = join_count_and_scan()) || (rc = enqueue_read_back()) || (rc = wait_and_clock_rows())) return rc;
        STOCS_TICK("join count+scan")
        if (sort_err_pin[0] || sort_err_pin[1]) { set_error("stocs_find_congruent_all: the pair-list sort gave up waiting for a tile (sort32.hip)"); return STOCS_ERR_HIP; }
        const unsigned long long* qoff_at = quad_off_pin();
        for (int b = 0; b <= nB; ++b) c->quad_off[b] = qoff_at[b];
        return STOCS_OK;
    }
};

// the pair lists are too long for this call: a piece of a trial batch (too_big != NULL) hears it and splits its base set, any other caller gets an error
static int lists_too_long(int* too_big, const char* why) { if (too_big) *too_big = 1; else set_error("%s", why); return too_big ? STOCS_OK : STOCS_ERR_CAPACITY; }

// One call of stocs_internal_find_congruent without its exit (below): every return of run(), error or not, goes through there.  The body is
// a short list of stages over the state they share.
struct CongruentCall {
    stocs_ctx* const c; const CongruentSwitches& sw; const size_t max_bytes; int* const too_big;
    const bool dbg;
    double tprev;
    CongruentState* S = NULL;
    int nB = 0, egSize = 0;
    float cell = 0, nepsilon = 0;
    KeyLayout K;
    PlanLayout L;
    PlanDev plan;
    char* dpl = NULL;                 // the planning buffer on the device
    PlanOut* po_pin = NULL;           // the plan's totals in the pinned block
    uint64_t totP = 0, totQ = 0;      // the first pass's list sizes: capacities (optimistic) or the plan's own
    bool optimistic = false;

    CongruentCall(stocs_ctx* c_, const CongruentSwitches& sw_, size_t max_bytes_, int* too_big_)
        : c(c_), sw(sw_), max_bytes(max_bytes_), too_big(too_big_), dbg(sw_.debug_timing), tprev(CallTiming::now_s()), L(0) {}

    // -- stage: both streams idle, the audit started, the arena recycled, the pinned block large enough --
    int enter() {
        c->timing[TIMING_CONGRUENT].begin();
        if (!c->index.built) { set_error("stocs_find_congruent_all: PPF index not built"); return STOCS_ERR_STATE; }
        nB = (int)c->bases.size();
        if (!c->cong) c->cong = new CongruentState();
        S = (CongruentState*)c->cong;
        S->valid = false;
        STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));   // the previous trial's buffers are about to be reused
        if (c->aux_stream) STOCS_HIP_CHECK(hipStreamSynchronize(c->aux_stream));   // (idle unless an earlier call failed half way)
        c->audit.on = sw.debug_streams;
        c->audit.host_sync(0); if (c->aux_stream) c->audit.host_sync(1);
        c->audit.retire_all("stocs_find_congruent_all: the arena is recycled");
        c->timing[TIMING_CONGRUENT].lap("entry synchronisation");
        { int rc0 = S->arena_state.reset(); if (rc0) return rc0; }
        tl_arena = &S->arena_state;
        if (!S->d_trig) {   // once per context (synchronous copy from static host memory)
            STOCS_HIP_CHECK(dev_malloc((void**)&S->d_trig, sizeof(float2) * (STOCS_MAX_CONE + 1) * STOCS_MAX_CONE));
            STOCS_HIP_CHECK(hipMemcpy(S->d_trig, cone_trig(), sizeof(float2) * (STOCS_MAX_CONE + 1) * STOCS_MAX_CONE, hipMemcpyHostToDevice));
        }
        // pinned block for everything this call reads back: plan totals, Q offsets (4 B per base), per-base quad offsets (8 B)
        { int rc0 = ensure_pinned(c, (size_t)PIN_VAR + 12 * ((size_t)nB + 1) + 256); if (rc0) return rc0; }
        c->timing[TIMING_CONGRUENT].lap("arena reset + pinned block");
        if (dbg) { const double t_ = CallTiming::now_s(); fprintf(stderr, "[stocs congruent] %-18s %8.3f ms\n", "sync+reset", (t_ - tprev) * 1e3); tprev = t_; }
        return STOCS_OK;
    }

    // the cone record of a base: stocs.cpp:801-803
    void cone_of(int b, BaseJob* J) const {
        const BaseRec& B = c->bases[b];
        J->cos_alpha = dot3(normalized3(c->h_spos[B.ids[1]] - c->h_spos[B.ids[0]]), normalized3(c->h_spos[B.ids[3]] - c->h_spos[B.ids[2]]));
        fill_cone_table(J);
    }

    // -- stage: per base the job record (invariants, cone table), uploaded; then the plan of its two lookups, on the device: 2 x nB small
    //    workgroups probe the bucket table, one workgroup lays the lists out; the host reads back four totals and the Q offsets (it sizes
    //    the sorts with them) -- 0.2 ms of host work per trial otherwise --
    int jobs_and_plan() {
        const PpfIndex& ix = c->index;
        // a batch's bases: the cone records wait until the device is busy (S->deferred, below)
        const bool defer_cone = nB >= 512;
        std::vector<BaseJob> jobs(nB);
        for (int b = 0; b < nB; ++b) {
            const BaseRec& B = c->bases[b];
            BaseJob& J = jobs[b];
            memset(&J, 0, sizeof(J));
            J.inv1 = B.inv1; J.inv2 = B.inv2;
            J.cell = cell; J.egSize = egSize;
            if (!defer_cone) cone_of(b, &J);
        }
        L = PlanLayout(nB);
        if (S->plan_bytes < L.bytes) {
            if (S->d_plan) (void)hipFree(S->d_plan);
            S->d_plan = NULL; S->plan_bytes = 0;
            STOCS_HIP_CHECK(dev_malloc((void**)&S->d_plan, 2 * L.bytes));
            S->plan_bytes = 2 * L.bytes;
        }
        if (S->stage_bytes < L.stage) {
            if (S->h_stage) (void)hipHostFree(S->h_stage);
            S->h_stage = NULL; S->stage_bytes = 0;
            STOCS_HIP_CHECK(pinned_malloc(&S->h_stage, 2 * L.stage));   // counted: a regrow inside a trial must show up
            S->stage_bytes = 2 * L.stage;
        }
        c->timing[TIMING_CONGRUENT].lap("host: jobs + cone tables + buffers");
        char* h = (char*)S->h_stage;
        dpl = S->d_plan;
        plan = {(BaseJob*)(dpl + L.jobs), (Segment*)(dpl + L.pseg), (Segment*)(dpl + L.qseg), (uint32_t*)(dpl + L.qoff), (uint32_t*)(dpl + L.poff),
                (int32_t*)(dpl + L.bids), (unsigned int*)(dpl + L.err), 0, 0};
        S->h_qoff.assign(nB + 1, 0);
        {
            int32_t* bids = (int32_t*)(h + L.bids);
            for (int b = 0; b < nB; ++b) for (int k = 0; k < 4; ++k) bids[4 * b + k] = c->bases[b].ids[k];
            memset(h + L.err, 0, 256);
        }
        memcpy(h + L.jobs, jobs.data(), sizeof(BaseJob) * (size_t)nB);
        STOCS_HIP_CHECK(hipMemcpyAsync(dpl, h, L.up, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(plan_ranges_kernel, dim3((unsigned)nB, 2), dim3(64), 0, c->stream, ix.d_bucket_start, ix.tr, ix.rot, ix.NA, ix.nD, plan.bids,
                           (const float4*)c->d_spos, (const float4*)c->d_snrmw, nB, (uint2*)(dpl + L.rng), (uint32_t*)(dpl + L.nr), (uint32_t*)(dpl + L.tot));
        plan_offsets();
        hipLaunchKernelGGL(plan_segments_kernel, dim3((unsigned)((2 * nB + 3) / 4)), dim3(256), 0, c->stream, nB, (const uint2*)(dpl + L.rng), (const uint32_t*)(dpl + L.nr),
                           (const uint32_t*)(dpl + L.tot), plan.psegs, plan.qsegs, (const uint32_t*)plan.p_off, (const uint32_t*)plan.q_off, (const uint32_t*)(dpl + L.spo),
                           (const uint32_t*)(dpl + L.sqo));
        STOCS_HIP_CHECK(hipGetLastError());
        // read-backs land in the pinned block (a copy into pageable memory -- a stack variable, a std::vector -- takes the
        // runtime's staging path): totals in the fixed slot, the Q offsets behind the per-base quad offsets of the count pass
        static_assert(sizeof(PlanOut) <= 256, "PlanOut must fit its pinned slot");
        po_pin = (PlanOut*)((char*)c->h_pin + PIN_CONGRUENT);
        STOCS_HIP_CHECK(hipMemcpyAsync(po_pin, dpl + L.out, sizeof(PlanOut), hipMemcpyDeviceToHost, c->stream));
        if (!K.reduce) STOCS_HIP_CHECK(hipMemcpyAsync(qoff_pin(), plan.q_off, 4 * ((size_t)nB + 1), hipMemcpyDeviceToHost, c->stream));   // (reduced lists: their own offsets come later)
        c->timing[TIMING_CONGRUENT].lap("enqueue plan upload + kernels + read-back");
        if (defer_cone) {
            // staged in the pinned block behind the upload, uploaded and patched into the device's jobs on the context's stream -- behind
            // the plan kernels, ahead of the join
            float4* hc = (float4*)(h + L.cone);
            BaseJob* dj = plan.jobs;
            S->deferred = [this, hc, dj]() -> int {
                for (int b = 0; b < nB; ++b) {
                    BaseJob J;
                    cone_of(b, &J);
                    float nb_bits; memcpy(&nb_bits, &J.nb, 4);
                    hc[b] = make_float4(J.cos_alpha, J.sin_alpha, nb_bits, 0.f);
                }
                DevBuf<float4> d_cone;
                int rc1 = d_cone.alloc((size_t)nB);
                if (rc1) return rc1;
                STOCS_HIP_CHECK(hipMemcpyAsync(d_cone.p, hc, sizeof(float4) * (size_t)nB, hipMemcpyHostToDevice, c->stream));
                hipLaunchKernelGGL(patch_cone_kernel, dim3((unsigned)((nB + 255) / 256)), dim3(256), 0, c->stream, dj, (const float4*)d_cone.p, nB);
                STOCS_HIP_CHECK(hipGetLastError());
                return STOCS_OK;
            };
        }
        return STOCS_OK;
    }
    uint32_t* qoff_pin() const { return (uint32_t*)((char*)c->h_pin + PIN_VAR + 8 * ((size_t)nB + 1)); }
    // the layout kernel of the plan (again before the redo: the base jobs carry the survivors' offsets by then, its inputs are still in the
    // planning buffer), and what it leaves behind for the passes declared to the stream audit
    void plan_offsets() {
        launch_plan_offsets(c->stream, nB, dpl, L, plan);
        c->audit.step(0, "plan kernels", {}, {{plan.jobs, "base jobs"}, {plan.psegs, "P segments"}, {plan.qsegs, "Q segments"}, {plan.q_off, "Q offsets per base"}});
    }

    // -- stage: the sizes of the first pass.  ONE sizing synchronisation point instead of two (plan totals, then survivors' totals): when an
    //    earlier trial of this scene has shown how long the lists get, buffers and launches are sized by a capacity (1.6 x that, per base),
    //    the kernels read the planned totals from the device, and the plan's totals come back together with the survivors' (the count pass).
    //    A plan beyond the capacity is detected there and redone with exact sizes.  Not for a trial batch under a memory ceiling (its
    //    caller needs the totals first) and not for the first trial of a scene.  *done: the lists are empty or too long. --
    int size_lists(bool* done, int* rc_done) {
        *done = false;
        optimistic = K.reduce && S->hist_nB > 0 && !sw.exact_sizes;
        if (optimistic) {
            const double scale = sw.capacity * (double)nB / (double)S->hist_nB;
            totP = (uint64_t)std::min(4.0e9, (double)S->hist_P * scale + sw.slack);
            totQ = (uint64_t)std::min(4.0e9, (double)S->hist_Q * scale + sw.slack);
            // a piece of a trial batch (too_big: its caller wants to hear when the lists do not fit the ceiling) goes this way only when the
            // capacities are far below the ceiling -- small frames, where the plan's round trip is a tenth of the piece; near the ceiling the
            // totals are read first, as in round 4
            if (too_big && max_bytes && (double)(totP + totQ) * 64.0 + (K.use_table ? (double)(K.NC * nB) * 8.0 : 0.0) + (double)((size_t)nB << K.cell_bits) / 4.0 > 0.25 * (double)max_bytes) {
                optimistic = false; totP = 0; totQ = 0;
            }
        }
        if (!optimistic) {
            STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
            c->timing[TIMING_CONGRUENT].lap("wait for the device (plan)");
            const PlanOut po = *po_pin;
            if (!K.reduce) memcpy(S->h_qoff.data(), qoff_pin(), 4 * ((size_t)nB + 1));
            if (po.overflow) { *done = true; *rc_done = lists_too_long(too_big, "pair lists exceed 2^32 entries"); return STOCS_OK; }
            totP = po.totP; totQ = po.totQ; plan.n_pseg = (int)po.n_pseg; plan.n_qseg = (int)po.n_qseg;
            S->hist_P = po.totP; S->hist_Q = po.totQ; S->hist_nB = nB;
        }
        STOCS_TICK("plan (device)")
        if (dbg) fprintf(stderr, "[stocs congruent] %s totP %llu totQ %llu segs %d %d\n", optimistic ? "capacities" : "planned", (unsigned long long)totP, (unsigned long long)totQ, plan.n_pseg, plan.n_qseg);
        if (totP == 0 || totQ == 0) { *done = true; *rc_done = STOCS_OK; return STOCS_OK; }
        if (K.id_bits > 16) { set_error("|M| = %d: model ids beyond 16 bits do not fit the packed pairs and quads", c->nM); return STOCS_ERR_CAPACITY; }
        return STOCS_OK;
    }

    // everything a pass allocates, estimated up front: one slab, one hipMalloc in a context's lifetime (if sizes stay put)
    int reserve_arena(uint64_t nP, uint64_t nQ, bool* over) {
        const size_t kb = K.wide ? 8 : 4;
        const size_t tables = K.use_table ? (size_t)(K.NC * nB) * 8 : 0;
        const size_t per_entry = 3 * kb + 8 + 16 + 8 + (K.reduce ? kb + 4 : 0);   // (the compacted copies of the reduced form)
        const size_t occ = K.reduce ? 2 * (((size_t)nB << K.cell_bits) / 8 + 8) : 0;
        const size_t need = (size_t)nP * per_entry + (size_t)nQ * per_entry + tables + occ + ((size_t)48 << 20);
        if (max_bytes && need > max_bytes && nB > 1) { *over = true; return STOCS_OK; }
        // (under a ceiling -- a piece of a trial batch -- the slab is 1.5 x the need, not twice it: 40 Cm trials need 36 GB)
        const int rc_r = S->arena_state.reserve(need, (max_bytes && need > ((size_t)4 << 30)) ? 1.5 : 2.0);   // (small pieces: room for the next call's capacities, which follow THIS call's totals)
        if (rc_r == STOCS_ERR_NOMEM && max_bytes && nB > 1) { *over = true; return STOCS_OK; }   // the device is fuller than the ceiling assumes: the caller halves the piece
        return rc_r;
    }

    // -- stage: one count pass over lists of nP and nQ entries (capacities when `with_capacities`): the arena reserved, the state the pass and
    //    the later calls read set, the form decided, the pass run.  The first pass and the redo of an outgrown plan both come through here;
    //    the redo recycles the arena first.  *done: the lists do not fit the ceiling (the caller of a batch's piece splits its base set). --
    int pass(uint64_t nP, uint64_t nQ, bool with_capacities, bool redo, bool* outgrown, bool* done, int* rc_done) {
        *done = false; *outgrown = false;
        if (redo) {
            int rc0 = S->arena_state.reset();
            if (rc0) return rc0;
            tl_arena = &S->arena_state;
        }
        bool over = false;
        int rc = reserve_arena(nP, nQ, &over);
        if (rc) return rc;
        if (over) { *done = true; *rc_done = lists_too_long(too_big, "pair lists beyond the memory ceiling"); return STOCS_OK; }
        const PassForm F = pass_form(c, K, sw, nB, (size_t)(uint32_t)nP, (size_t)(uint32_t)nQ, with_capacities);
        if (!redo) c->timing[TIMING_CONGRUENT].lap(F.reserve_label());   // (names the form)
        S->nB = nB; S->totP = (uint32_t)nP; S->totQ = (uint32_t)nQ; S->nepsilon = nepsilon;
        S->half_inv_neps = (float)(0.5 / (double)nepsilon);
        S->NC = K.NC; S->use_table = K.use_table; S->wide = K.wide; S->reduce = K.reduce;
        {   // two points of one position cell are at most a cell diagonal apart (cell edge = ratio / egSize < 2 epsilon); the
            // float roundings of the two world-space points and of the unit-cube coordinates are far below the 1e-5 m allowed for
            const double cell_world = (double)c->ratio / (double)egSize, diag2 = 3.0 * (cell_world * 1.001 + 1e-5) * (cell_world * 1.001 + 1e-5);
            S->close_cells = diag2 < 0.999 * (double)c->prm.distance_threshold && !sw.distance_gate;
        }
        S->id_bits = K.id_bits; S->base_bits = K.base_bits; S->cell_bits = K.cell_bits;
        S->base_in_key = 4 * K.id_bits + K.base_bits <= 64;
        S->no_quads = false;
        const PlanOut* d_po = F.optimistic ? (const PlanOut*)(dpl + L.out) : NULL;
        const PlanOut* pin = F.optimistic ? po_pin : NULL;
        return K.wide ? CountPass<uint64_t>(c, S, plan, F, dbg, tprev, d_po, pin).run(outgrown) : CountPass<uint32_t>(c, S, plan, F, dbg, tprev, d_po, pin).run(outgrown);
    }

    int run(int64_t* total_quads) {
        int rc = enter();
        if (rc) return rc;
        c->quad_off.assign(nB + 1, 0);
        c->quad_id_bits = 16;
        if (total_quads) *total_quads = 0;
        if (nB == 0) return STOCS_OK;
        if (nB >= (1 << 20)) { set_error("too many bases"); return STOCS_ERR_INVALID; }
        const float eps_unit = c->prm.distance_threshold / c->ratio;  // getNormalizedEpsilon, pairCreationFunctor.h:141-143
        const int gridDepth = (int)(-log2f(eps_unit));                // normalset.h:117
        egSize = (int)pow(2.0, (double)gridDepth);                    // :118
        cell = 1.f / egSize;                                          // :119
        nepsilon = (float)((double)(1.0f / 7.0f) + 0.00001);          // normalset.h:86
        K = key_layout(nB, c->nM, egSize, sw);
        if ((rc = jobs_and_plan())) return rc;
        bool done = false, outgrown = false;
        int rc_done = STOCS_OK;
        if ((rc = size_lists(&done, &rc_done)) || done) return rc ? rc : rc_done;
        if ((rc = pass(totP, totQ, optimistic, false, &outgrown, &done, &rc_done)) || done) return rc ? rc : rc_done;   // (on an error the read-back may not have landed: the capacity history stays as it was)
        if (optimistic) {    // the read-back of the count pass brought the plan's totals
            const PlanOut po = *po_pin;
            if (po.overflow) return lists_too_long(too_big, "pair lists exceed 2^32 entries");
            S->hist_P = po.totP; S->hist_Q = po.totQ; S->hist_nB = nB;
            if (outgrown) {
                // the plan outgrew the capacities: once more with the sizes now known, the planned offsets written into the base jobs again
                c->timing[TIMING_CONGRUENT].lap("plan beyond the capacities: redone with exact sizes");
                plan_offsets();
                STOCS_HIP_CHECK(hipGetLastError());
                plan.n_pseg = (int)po.n_pseg; plan.n_qseg = (int)po.n_qseg;
                if (po.totP == 0 || po.totQ == 0) return STOCS_OK;
                if ((rc = pass(po.totP, po.totQ, false, true, &outgrown, &done, &rc_done)) || done) return rc ? rc : rc_done;
            }
        }
        if (!c->audit.violations.empty()) {   // STOCS_DEBUG_STREAMS: a use without an event edge between the two streams
            set_error("stocs_find_congruent_all: %zu stream-ordering violation(s); first: %s", c->audit.violations.size(), c->audit.violations[0].c_str());
            c->audit.violations.clear();
            return STOCS_ERR_STATE;
        }
        if (S->no_quads) return STOCS_OK;   // as with empty lists: nothing to materialise, every base has zero quads
        S->valid = true;
        c->quad_id_bits = K.id_bits;
        if (total_quads) *total_quads = (int64_t)c->quad_off[nB];
        return STOCS_OK;
    }
};

}  // namespace stocs

using namespace stocs;

extern "C" {

void stocs_internal_free_congruent(stocs_ctx* c) {   // stocs_ctx_destroy: nothing is in flight any more
    if (c && c->cong) {
        CongruentState* S = (CongruentState*)c->cong;
        S->arena_state.destroy(); S->arena_tmp.destroy();
        if (S->h_stage) (void)hipHostFree(S->h_stage);
        if (S->d_plan) (void)hipFree(S->d_plan);
        if (S->d_trig) (void)hipFree(S->d_trig);
        delete S;
        c->cong = NULL;
    }
}

void stocs_internal_invalidate_congruent(stocs_ctx* c) {   // the counted state refers to bases of another scene
    if (c && c->cong) { CongruentState* S = (CongruentState*)c->cong; S->valid = false; S->hist_nB = 0; S->hist_P = S->hist_Q = 0; }
}

// Host evaluation of one cone query with both evaluations of cone_cells.h (no device needed): the direction-cell bitset
// from the reference's arithmetic alone, the one the kernels build (filter first, exact arithmetic where the filter
// cannot decide) and how many of the samples needed the exact path.  The two bitsets must be identical.
int stocs_cone_cells_host(const float* n3, float cos_alpha, uint32_t* exact_bits11, uint32_t* kernel_bits11, int* n_samples, int* n_undecided) {
    if (!n3 || !exact_bits11 || !kernel_bits11) return STOCS_ERR_INVALID;
    BaseJob J;
    memset(&J, 0, sizeof(J));
    J.cos_alpha = cos_alpha;
    fill_cone_table(&J);
    const float nepsilon = (float)((double)(1.0f / 7.0f) + 0.00001);
    const float half_inv_neps = (float)(0.5 / (double)nepsilon);
    for (int k = 0; k < 11; ++k) exact_bits11[k] = kernel_bits11[k] = 0;
    float q[4];
    quat_from_z(mk3(n3[0], n3[1], n3[2]), q);
    const ConeFilter cf = cone_filter_setup(q, J.cos_alpha, half_inv_neps);
    int undecided = 0;
    const float* trig = cone_trig() + (size_t)J.nb * STOCS_MAX_CONE * 2;
    for (int a = 0; a < J.nb; ++a) {
        const V3 d = mk3(J.sin_alpha * trig[2 * a], J.sin_alpha * trig[2 * a + 1], J.cos_alpha);
        const int ie = cone_cell_exact(q, d, nepsilon);
        if (ie >= 0) exact_bits11[ie >> 5] |= 1u << (ie & 31);
        int ik = cone_cell_filtered(cf, d.x, d.y);
        if (ik < 0) { undecided++; ik = ie; }
        if (ik >= 0) kernel_bits11[ik >> 5] |= 1u << (ik & 31);
    }
    if (n_samples) *n_samples = J.nb;
    if (n_undecided) *n_undecided = undecided;
    return STOCS_OK;
}

}  // extern "C"

namespace stocs {

// One cone query as the device sees it: the query direction and the cone fields of its base job (fill_cone_table on the host).
struct ConeQuery { float nx, ny, nz, cos_alpha, sin_alpha; int nb; };

// The colouring of join_one on its own, one lane per query (stocs_cone_cells_device): the same shared functions in the same order --
// quat_from_z, cone_filter_setup, per sample (sin_alpha * trig) cone_cell_filtered and, here for EVERY sample, cone_cell_exact.
// Every lane writes its own rows of the outputs (zeroed by the host) and nothing else.
__global__ __launch_bounds__(256) void cone_cells_kernel(const ConeQuery* __restrict__ qs, int n, const float2* __restrict__ trig, float nepsilon, float half_inv_neps,
                                                         uint32_t* __restrict__ exact_bits, uint32_t* __restrict__ kernel_bits, int32_t* __restrict__ n_undecided,
                                                         float4* __restrict__ quat, int32_t* __restrict__ filt_id, int32_t* __restrict__ exact_id, float* __restrict__ t3) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ConeQuery Q = qs[i];
    float q[4];
    quat_from_z(mk3(Q.nx, Q.ny, Q.nz), q);
    const float dz = Q.cos_alpha;
    const ConeFilter cf = cone_filter_setup(q, dz, half_inv_neps);
    quat[i] = make_float4(q[0], q[1], q[2], q[3]);
    uint32_t* eb = exact_bits + (size_t)i * 11;
    uint32_t* kb = kernel_bits + (size_t)i * 11;
    const float2* tr = trig + (size_t)Q.nb * STOCS_MAX_CONE;
    const float sa = Q.sin_alpha;
    int undecided = 0;
    for (int a = 0; a < Q.nb; ++a) {
        const float2 t = tr[a];
        const float dx = sa * t.x, dy = sa * t.y;
        const size_t o = (size_t)i * STOCS_MAX_CONE + (size_t)a;
        float tx, ty, tz;
        cone_filter_coords(cf, dx, dy, &tx, &ty, &tz);
        t3[3 * o] = tx; t3[3 * o + 1] = ty; t3[3 * o + 2] = tz;
        const int ik = cone_cell_filtered(cf, dx, dy);
        const int ie = cone_cell_exact(q, mk3(dx, dy, dz), nepsilon);
        filt_id[o] = ik; exact_id[o] = ie;
        if (ie >= 0) eb[ie >> 5] |= 1u << (ie & 31);
        int id = ik;
        if (id < 0) { undecided++; id = ie; }   // what `colour` of join_one does
        if (id >= 0) kb[id >> 5] |= 1u << (id & 31);
    }
    n_undecided[i] = undecided;
}

}  // namespace stocs

extern "C" {

// The same query on the device, n at a time: what the join kernels compute for a sample (contract in stocs_hip.h)
int stocs_cone_cells_device(int device, const float* n3, const float* cos_alpha, int n, uint32_t* exact_bits11, uint32_t* kernel_bits11, int32_t* n_samples,
                            int32_t* n_undecided, float* q4, int32_t* filtered_id, int32_t* exact_id, float* t3) {
    if (n < 0 || (n && (!n3 || !cos_alpha || !exact_bits11 || !kernel_bits11 || !n_samples || !n_undecided || !q4 || !filtered_id || !exact_id || !t3))) return STOCS_ERR_INVALID;
    if (n == 0) return STOCS_OK;
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    DeviceGuard dev_guard(device);
    const float nepsilon = (float)((double)(1.0f / 7.0f) + 0.00001);
    const float half_inv_neps = (float)(0.5 / (double)nepsilon);
    std::vector<ConeQuery> hq((size_t)n);
    for (int i = 0; i < n; ++i) {
        BaseJob J;
        memset(&J, 0, sizeof(J));
        J.cos_alpha = cos_alpha[i];
        fill_cone_table(&J);
        const ConeQuery Q = {n3[3 * i], n3[3 * i + 1], n3[3 * i + 2], J.cos_alpha, J.sin_alpha, J.nb};
        hq[i] = Q;
        n_samples[i] = J.nb;
    }
    const size_t nn = (size_t)n, ns = nn * STOCS_MAX_CONE;
    const size_t trig_bytes = sizeof(float2) * (STOCS_MAX_CONE + 1) * STOCS_MAX_CONE;
    ConeQuery* d_q = NULL; float2* d_trig = NULL; uint32_t *d_eb = NULL, *d_kb = NULL; int32_t *d_nu = NULL, *d_fi = NULL, *d_ei = NULL; float4* d_quat = NULL; float* d_t = NULL;
    int rc = STOCS_OK;
#define CC_TRY(x) do { if ((x) != hipSuccess) { set_error("stocs_cone_cells_device: %s", #x); rc = STOCS_ERR_HIP; goto done; } } while (0)
    CC_TRY(hipMalloc((void**)&d_q, nn * sizeof(ConeQuery))); CC_TRY(hipMalloc((void**)&d_trig, trig_bytes));
    CC_TRY(hipMalloc((void**)&d_eb, nn * 44)); CC_TRY(hipMalloc((void**)&d_kb, nn * 44)); CC_TRY(hipMalloc((void**)&d_nu, nn * 4)); CC_TRY(hipMalloc((void**)&d_quat, nn * 16));
    CC_TRY(hipMalloc((void**)&d_fi, ns * 4)); CC_TRY(hipMalloc((void**)&d_ei, ns * 4)); CC_TRY(hipMalloc((void**)&d_t, ns * 12));
    CC_TRY(hipMemcpy(d_q, hq.data(), nn * sizeof(ConeQuery), hipMemcpyHostToDevice)); CC_TRY(hipMemcpy(d_trig, cone_trig(), trig_bytes, hipMemcpyHostToDevice));
    CC_TRY(hipMemset(d_eb, 0, nn * 44)); CC_TRY(hipMemset(d_kb, 0, nn * 44)); CC_TRY(hipMemset(d_t, 0, ns * 12));
    CC_TRY(hipMemset(d_fi, 0xFF, ns * 4)); CC_TRY(hipMemset(d_ei, 0xFF, ns * 4));      // slots beyond a query's samples: -1, t = 0
    cone_cells_kernel<<<(unsigned)((nn + 255) / 256), 256, 0, 0>>>(d_q, n, d_trig, nepsilon, half_inv_neps, d_eb, d_kb, d_nu, d_quat, d_fi, d_ei, d_t);
    CC_TRY(hipGetLastError());
    CC_TRY(hipDeviceSynchronize());
    CC_TRY(hipMemcpy(exact_bits11, d_eb, nn * 44, hipMemcpyDeviceToHost)); CC_TRY(hipMemcpy(kernel_bits11, d_kb, nn * 44, hipMemcpyDeviceToHost));
    CC_TRY(hipMemcpy(n_undecided, d_nu, nn * 4, hipMemcpyDeviceToHost)); CC_TRY(hipMemcpy(q4, d_quat, nn * 16, hipMemcpyDeviceToHost));
    CC_TRY(hipMemcpy(filtered_id, d_fi, ns * 4, hipMemcpyDeviceToHost)); CC_TRY(hipMemcpy(exact_id, d_ei, ns * 4, hipMemcpyDeviceToHost));
    CC_TRY(hipMemcpy(t3, d_t, ns * 12, hipMemcpyDeviceToHost));
done:
#undef CC_TRY
    (void)hipFree(d_q); (void)hipFree(d_trig); (void)hipFree(d_eb); (void)hipFree(d_kb); (void)hipFree(d_nu); (void)hipFree(d_quat); (void)hipFree(d_fi); (void)hipFree(d_ei); (void)hipFree(d_t);
    return rc;
}

int stocs_find_congruent_all(stocs_ctx* c, int64_t* total_quads) { return stocs_internal_find_congruent(c, total_quads, 0, NULL); }

int stocs_internal_find_congruent(stocs_ctx* c, int64_t* total_quads, size_t max_bytes, int* too_big) {
    if (!c) return STOCS_ERR_INVALID;
    if (too_big) *too_big = 0;
    DeviceGuard dev_guard(c->device);
    const CongruentSwitches sw = CongruentSwitches::read();
    const int rc = CongruentCall(c, sw, max_bytes, too_big).run(total_quads);
    // The one exit.  The deferred host work never outlives the call, and a failed call leaves nothing in flight: no read-back still
    // landing in the pinned block (ensure_pinned may free it), nothing still running on the auxiliary stream.  The synchronisation's
    // own status is ignored (the first error message stands); a successful call is synchronised at the next one's entry.
    if (c->cong) ((CongruentState*)c->cong)->deferred = nullptr;
    if (rc != STOCS_OK) {
        (void)hipStreamSynchronize(c->stream);
        if (c->aux_stream) (void)hipStreamSynchronize(c->aux_stream);
        c->audit.host_sync(0); if (c->aux_stream) c->audit.host_sync(1);
    }
    return rc;
}

int stocs_get_quads(stocs_ctx* c, int slot, int32_t* quads4, int64_t cap, int64_t* n) {
    if (!c || !n || slot < 0) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    if (slot + 1 >= (int)c->quad_off.size()) { set_error("stocs_get_quads: no such base slot (call stocs_find_congruent_all first)"); return STOCS_ERR_STATE; }
    *n = (int64_t)(c->quad_off[slot + 1] - c->quad_off[slot]);
    if (!quads4 || *n == 0) return STOCS_OK;
    CongruentState* S = (CongruentState*)c->cong;
    if (!S || !S->valid) { set_error("stocs_get_quads: no congruent state (call stocs_find_congruent_all first)"); return STOCS_ERR_STATE; }
    { int rc0 = S->arena_tmp.reset(); if (rc0) return rc0; }
    tl_arena = &S->arena_tmp;
    S->small_ready = false;
    const int64_t m = std::min<int64_t>(*n, cap);
    std::vector<uint64_t> q((size_t)std::max<int64_t>(m, 0));
    if (m > 0) {
        std::vector<char> sel(S->nB, 0);
        sel[slot] = 1;
        DevBuf<uint64_t> d_sorted;
        std::vector<unsigned long long> off;
        int rc = materialise(c, S, sel, &d_sorted, &off);
        if (rc) return rc;
        STOCS_HIP_CHECK(hipMemcpyAsync(q.data(), d_sorted.p + off[slot], 8 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
        STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    for (int64_t i = 0; i < m; ++i) unpack_quad(q[i], c->quad_id_bits, quads4 + 4 * i);
    return (*n > cap) ? STOCS_ERR_CAPACITY : STOCS_OK;
}

// quads of base `slot` at the given ranks of its WALK order (by position cell of the Q pair, then index position of the
// Q pair, then index position of the P pair; see the head of this file) -- what stocs_make_transforms samples from when
// a base has >= max quads
int stocs_get_quads_at(stocs_ctx* c, int slot, const int64_t* ranks, int n, int32_t* quads4) {
    if (!c || slot < 0 || n < 0 || (n && (!ranks || !quads4))) return STOCS_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    if (slot + 1 >= (int)c->quad_off.size()) { set_error("stocs_get_quads_at: no such base slot (call stocs_find_congruent_all first)"); return STOCS_ERR_STATE; }
    if (n == 0) return STOCS_OK;
    CongruentState* S = (CongruentState*)c->cong;
    const int64_t nq = (int64_t)(c->quad_off[slot + 1] - c->quad_off[slot]);
    std::vector<Pick> picks(n);
    for (int i = 0; i < n; ++i) {
        if (ranks[i] < 0 || ranks[i] >= nq || ranks[i] > 0x7FFFFFFFll) { set_error("stocs_get_quads_at: rank %lld out of range (%lld quads)", (long long)ranks[i], (long long)nq); return STOCS_ERR_INVALID; }
        picks[i].base = slot; picks[i].rank = (int32_t)ranks[i]; picks[i].dst = i; picks[i].sorted = 0;
    }
    if (!S || !S->valid) { set_error("stocs_get_quads_at: no congruent state (call stocs_find_congruent_all first)"); return STOCS_ERR_STATE; }
    { int rc0 = S->arena_tmp.reset(); if (rc0) return rc0; }
    tl_arena = &S->arena_tmp;
    S->small_ready = false;
    DevBuf<Pick> d_picks; DevBuf<uint64_t> d_keys;
    int rc;
    if ((rc = d_picks.alloc(n)) || (rc = d_keys.alloc(n))) return rc;
    if ((rc = ensure_pinned(c, (size_t)PIN_VAR + 8 * (size_t)n + 256))) return rc;
    uint64_t* keys = (uint64_t*)((char*)c->h_pin + PIN_VAR);
    unsigned int* n_err_pin = (unsigned int*)((char*)c->h_pin + PIN_CONGRUENT);
    STOCS_HIP_CHECK(hipMemcpyAsync(d_picks.p, picks.data(), sizeof(Pick) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_resolve_picks(c, S, d_picks.p, n, NULL, NULL, NULL, d_keys.p))) return rc;
    STOCS_HIP_CHECK(hipMemcpyAsync(keys, d_keys.p, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipMemcpyAsync(n_err_pin, S->d_err.p, 4, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    const unsigned int n_err = *n_err_pin;
    if (n_err) { set_error("stocs_get_quads_at: %u ranks could not be resolved (internal inconsistency)", n_err); return STOCS_ERR_STATE; }
    for (int i = 0; i < n; ++i) unpack_quad(keys[i], c->quad_id_bits, quads4 + 4 * (size_t)i);
    return STOCS_OK;
}

// Device side of stocs_make_transforms, in two halves.  First, before the picks exist: the bases used whole (base_used_whole: fewer quads
// than the per-base maximum) are materialised and sorted into the std::set order.  Which bases those are follows from the counts alone,
// so the fill + sort run while the host draws the seeded subsets of the large bases, or next to the draw on the auxiliary stream.
int stocs_internal_prepare_small(stocs_ctx* c, int max_per_base) {
    CongruentState* S = (CongruentState*)c->cong;
    if (!S || !S->valid) { set_error("stocs_make_transforms: no congruent state (call stocs_find_congruent_all first)"); return STOCS_ERR_STATE; }
    { int rc0 = S->arena_tmp.reset(); if (rc0) return rc0; }
    tl_arena = &S->arena_tmp;
    S->small_ready = true; S->small_any = false;
    std::vector<char> sel(S->nB, 0);
    for (int b = 0; b < S->nB; ++b) {
        const unsigned long long nq = c->quad_off[b + 1] - c->quad_off[b];
        if (nq > 0 && base_used_whole((long long)nq, max_per_base)) { sel[b] = 1; S->small_any = true; }
    }
    if (!S->small_any) return STOCS_OK;
    std::vector<unsigned long long>& off = S->h_off;
    int rc;
    if ((rc = materialise(c, S, sel, &S->d_small_sorted, &off)) || (rc = S->d_small_soff.alloc(off.size()))) return rc;
    STOCS_HIP_CHECK(hipMemcpyAsync(S->d_small_soff.p, off.data(), 8 * off.size(), hipMemcpyHostToDevice, c->stream));
    return STOCS_OK;
}

// Second half: n picks -> XformJob records on the device.  The picks are either on the device already (picks_dev, drawn there) or
// uploaded from picks_host; those with sorted != 0 refer to the runs stocs_internal_prepare_small left in the arena, so that call
// must have run since the arena was last reset.  *d_unresolved_out: device counter of the picks the kernel could not resolve (0 while
// counts and join agree); the caller reads it behind its own synchronisation point, this call does not wait for the device.
int stocs_internal_make_jobs(stocs_ctx* c, const Pick* picks_host, const Pick* picks_dev, int n, XformJob* d_jobs_out, const unsigned int** d_unresolved_out) {
    if (d_unresolved_out) *d_unresolved_out = NULL;
    CongruentState* S = (CongruentState*)c->cong;
    const bool prepared = S && S->small_ready;
    if (S) S->small_ready = false;
    if (n <= 0) return STOCS_OK;
    if (!S || !S->valid) { set_error("stocs_make_transforms: no congruent state (call stocs_find_congruent_all first)"); return STOCS_ERR_STATE; }
    if (!prepared) { set_error("internal: device picks without the small bases prepared"); return STOCS_ERR_STATE; }
    tl_arena = &S->arena_tmp;   // the temporaries of stocs_internal_prepare_small are still in it
    int rc;
    if (!picks_dev) {
        DevBuf<Pick> d_picks;
        if ((rc = d_picks.alloc(n))) return rc;
        STOCS_HIP_CHECK(hipMemcpyAsync(d_picks.p, picks_host, sizeof(Pick) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        picks_dev = d_picks.p;
    }
    if ((rc = launch_resolve_picks(c, S, picks_dev, n, S->small_any ? S->d_small_sorted.p : NULL, S->small_any ? S->d_small_soff.p : NULL, d_jobs_out, NULL))) return rc;
    if (d_unresolved_out) *d_unresolved_out = S->d_err.p;
    return STOCS_OK;
}

}  // extern "C"
