// congruent_lists.h -- the pair lists of the congruent phase (congruent.hip) on the device: their records, and the kernels that gather
// both lists of all bases out of the PPF index, mark the (base, cell) values each occupies and reduce each to the entries whose cell the
// other list occupies.  Every list kernel takes the records of BOTH lists (ListSide) and works on list side0 + blockIdx.y, so that one
// kernel serves both lists in one launch and one list per launch.  Included by congruent.hip alone.
#ifndef STOCS_CONGRUENT_LISTS_H
#define STOCS_CONGRUENT_LISTS_H

#include <stdlib.h>

#include <algorithm>

#include "stocs_ctx.h"

namespace stocs {

struct BaseJob {
    float inv1, inv2, cos_alpha;
    float cell;       // _epsilon of the normal set (unit-cube cell edge)
    int egSize;
    int nb;           // cone samples
    uint32_t p_off, p_len, q_off, q_len;   // runs in the gathered P / Q arrays
    float sin_alpha;  // the cone samples of the base are (sin_alpha * cos theta_a, sin_alpha * sin theta_a, cos_alpha), a < nb, with cos / sin of
                      // theta_a = a * angleStep(nb) from ONE table shared by all bases (cone_trig: they depend on nb alone).  Round 3 carried the
                      // 56 products per base in the job record: 808 bytes per base to fill and upload -- 0.7 ms of host time for the 6 000
                      // bases of a 64-trial batch; the one float product per sample is the same IEEE operation on the device.
    float pad;
};

struct Segment { uint32_t src, len, dst, base; };

// Totals and array sizes of a trial's pair lists, read back by the host (the only thing it needs before it can size the sorts)
struct PlanOut { unsigned long long totP, totQ; uint32_t n_pseg, n_qseg, overflow, pad; };


// exclusive scan of a[0 .. n) by one workgroup of 1024, in place; emit(i, offset, value) sees every element
template <class F>
__device__ __forceinline__ void block_scan_1024(uint32_t* __restrict__ a, uint32_t n, uint32_t* s_part, F emit) {
    const uint32_t tid = threadIdx.x, chunk = (n + 1023u) / 1024u;
    const uint32_t lo = min(tid * chunk, n), hi = min(lo + chunk, n);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += a[i];
    __syncthreads();
    s_part[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t v = tid >= d ? s_part[tid - d] : 0u;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    uint32_t run = s_part[tid] - sum;
    for (uint32_t i = lo; i < hi; ++i) { const uint32_t v = a[i]; a[i] = run; emit(i, run, v); run += v; }
}

// normalset.h:97-104 + utils.h:139-148: int truncation of coord/epsilon, x fastest
// (cell = 1 / eg with eg a power of two, normalset.h:117-119: dividing by it and multiplying by eg are the same float)
__device__ __forceinline__ int64_t index_pos(V3 p, float cell, int eg) {
    (void)cell;
    const V3 cp = p * (float)eg;
    return (int64_t)(int)cp.z * eg * eg + ((int64_t)(int)cp.y * eg + (int64_t)(int)cp.x);
}

// Pair lists of all bases out of the device index (a lookup is the union of <= 128 buckets, ppf_index.hip), each entry
// with its sort key (base << cell_bits | position cell).  P entries sit at p1 + inv1 (p2 - p1) (nset.addElement,
// stocs.cpp:810-818), Q entries query at p1 + inv2 (p2 - p1) (stocs.cpp:827-836).  A cell the table cannot hold -- it
// cannot occur for points of the unit cube -- gets the all-ones cell: never queried, never matched.
#define GATHER_EPT 4
#define GATHER_TILE (256u * GATHER_EPT)
// (8 192 since round 5b: with 2 048 -- one round of resident workgroups, each with an eighth of a per cent of the list -- the last of them ran on a
//  half-empty chip: 4.4 wavefronts per SIMD on average over a 42-trial piece; four times as many, shorter workgroups level that: congruent phase -2 %)
static inline unsigned gather_max_wgs() { static const unsigned v = getenv("STOCS_GATHER_WGS") ? (unsigned)std::max(1, atoi(getenv("STOCS_GATHER_WGS"))) : 8192u; return v; }
#define GATHER_MAX_WGS gather_max_wgs()
static inline unsigned gather_grid(unsigned long long total) { const unsigned long long t = (total + GATHER_TILE - 1) / GATHER_TILE; return (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>(t, GATHER_MAX_WGS)); }
// One pair list of a count pass as its kernels see it, built once per side (CountPass::allocate_lists; the unreduced gather fills the
// first line alone): every list kernel takes BOTH records and works on list side0 + blockIdx.y (0 = P, 1 = Q).
template <class KeyT>
struct ListSide {
    const Segment* segs; int nseg; uint32_t n; KeyT* keys; uint32_t* vals;   // the segments the gather walks, entries (or their capacity), gathered keys and pairs
    uint32_t* occ; const uint32_t* other;                                    // occupancy bits: this list's (marked by the gather), the other list's (tested by the count)
    uint32_t* tiles; unsigned long long* alive;                              // survivors per tile (offsets after the scan), one bit per entry: survives
    KeyT* okeys; uint32_t* ovals;                                            // the survivors, compacted
};
// Both lists in ONE launch (gridDim.y == 2, side0 = 0): the one-stream form of a count pass -- P and Q still share the chip, and no event edge
// between two streams (~11 us each on this runtime, five of them in a trial) stands between the steps.  One list per launch (gridDim.y == 1,
// side0 = 0 or 1): the two-stream form, and the unreduced gather (occ == NULL, po == NULL, lds_words == 0).
// po != NULL: the launch was sized by a CAPACITY (the host has not read the plan yet, see stocs_internal_find_congruent): the
// list's length and segment count are the planned ones, read here, and the workgroups beyond them leave at once.
template <class KeyT>
__global__ __launch_bounds__(256) void gather_key_kernel(const uint32_t* __restrict__ pairs, ListSide<KeyT> P, ListSide<KeyT> Q, int side0, const BaseJob* __restrict__ jobs,
                                                         const float4* __restrict__ munit, int cell_bits, long long cell_limit, const PlanOut* __restrict__ po,
                                                         uint32_t lds_words, uint32_t n_bases) {
    const int is_q = side0 + (int)blockIdx.y;
    const Segment* __restrict__ segs = is_q ? Q.segs : P.segs;
    int nseg = is_q ? Q.nseg : P.nseg;
    uint32_t total = is_q ? Q.n : P.n;
    // occ: ONE BIT per (base, cell) value of the key -- which (base, cell) this list occupies.  lds_words > 0 (= 2^cell_bits / 32, the
    // words of one base): the bits of the base the workgroup's current tile starts in are collected in LDS and OR-ed into the table
    // when the workgroup moves on to the next base or ends (a base's stretch is ~88 tiles at Cm: one atomic per word and workgroup
    // instead of one scattered store per entry); entries of another base in the same tile (a boundary tile) go to the table directly.
    extern __shared__ uint32_t s_occ[];
    if (po) {
        if (po->overflow) return;          // >= 2^32 planned entries: the segments' 32-bit destinations have wrapped; the host reports STOCS_ERR_CAPACITY
        const unsigned long long t = is_q ? po->totQ : po->totP;
        total = t < (unsigned long long)total ? (uint32_t)t : total;      // never beyond the buffers (a plan beyond the capacity is redone by the host)
        nseg = (int)(is_q ? po->n_qseg : po->n_pseg);
    }
    // What follows is a lambda for ONE reason: __restrict__ counts on a parameter only, and the three arrays written here must carry it --
    // without it the key / pair stores and the occupancy atomics are ordered against each other and the 32-bit form takes 68 VGPRs for 66.
    [&](KeyT* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ occ) {
        // A workgroup takes a contiguous run of tiles (GATHER_EPT * 256 entries each; a thread GATHER_EPT of them 256 apart, coalesced),
        // the launch at most GATHER_MAX_WGS workgroups: the binary search over the segments (12 scalar loads one after the other) runs once
        // per workgroup, the segment of a wavefront's entries is wave-uniform STATE carried from tile to tile (a segment holds thousands
        // of entries: the next boundary is compared, not loaded), and the workgroup owns the LDS bits of "its" base across its tiles.  The
        // steady state is pair load -> two model points -> stores: three dependent round trips per tile, ~10 us per tile with eight
        // workgroups on a CU (device clock of one workgroup, round 4).  The kernel is bound by the bytes its waves keep in flight (1.5 TB/s
        // over both lists, waves waiting 53 %, no unit above 0.65 busy); by ablation (one list, 9.5 M entries, 103 us): without the
        // occupancy marks 83, without the (key, pair) stores 83, with nothing but the pair load 62.  Prefetching the next tile's pairs,
        // the model in LDS and 64-bit products as shifts were measured and not kept.
        const uint32_t n_tiles = (total + GATHER_TILE - 1u) / GATHER_TILE;
        const uint32_t per_wg = (n_tiles + gridDim.x - 1u) / gridDim.x;
        const uint32_t t_begin = blockIdx.x * per_wg, t_end = min(n_tiles, t_begin + per_wg);
        if (t_begin >= t_end) return;
        const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
        const uint32_t w0 = t_begin * GATHER_TILE + wave * 64u;      // the wavefront's first entry
        const bool mark_lds = occ != NULL && lds_words != 0u;
        if (mark_lds) { for (uint32_t w = threadIdx.x; w < lds_words; w += blockDim.x) s_occ[w] = 0u; __syncthreads(); }
        // the base the current TILE starts in, followed through the base jobs (uniform over the workgroup: it depends on the tile alone)
        uint32_t cur_b = 0, cur_end = 0;
        if (mark_lds) {
            const uint32_t ts = t_begin * GATHER_TILE;
            int blo = 0, bhi = (int)n_bases - 1;       // last base whose stretch begins at or before ts
            while (blo < bhi) {
                const int mid = (blo + bhi + 1) >> 1;
                const uint32_t off = is_q ? jobs[mid].q_off : jobs[mid].p_off;
                if (off <= ts) blo = mid; else bhi = mid - 1;
            }
            cur_b = (uint32_t)blo;
            cur_end = blo + 1 < (int)n_bases ? (is_q ? jobs[blo + 1].q_off : jobs[blo + 1].p_off) : 0xFFFFFFFFu;
        }
        auto flush = [&](uint32_t b) {
            __syncthreads();
            for (uint32_t w = threadIdx.x; w < lds_words; w += blockDim.x) {
                const uint32_t v = s_occ[w];
                if (v) { atomicOr(&occ[(size_t)b * lds_words + w], v); s_occ[w] = 0u; }
            }
            __syncthreads();
        };
        int lo = 0, hi = nseg - 1;                                    // last segment with dst <= w0 (uniform binary search, scalar loads)
        if (w0 < total) {
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (segs[mid].dst <= w0) lo = mid; else hi = mid - 1;
            }
        }
        // wave-uniform segment state
        int sgu = lo;
        uint32_t sg_src = 0, sg_dst = 0, sg_base = 0, next_dst = 0xFFFFFFFFu, gu = 1;
        float ju = 0.0f;
        auto load_segment = [&](int i) {
            const Segment sg = segs[i];
            sg_src = __builtin_amdgcn_readfirstlane(sg.src); sg_dst = __builtin_amdgcn_readfirstlane(sg.dst); sg_base = __builtin_amdgcn_readfirstlane(sg.base);
            next_dst = i + 1 < nseg ? __builtin_amdgcn_readfirstlane(segs[i + 1].dst) : 0xFFFFFFFFu;
            const BaseJob& J = jobs[sg_base];
            ju = is_q ? J.inv2 : J.inv1; gu = (uint32_t)J.egSize;
        };
        if (nseg > 0) load_segment(sgu);
        const KeyT cmask = ((KeyT)1 << cell_bits) - (KeyT)1;
        for (uint32_t tile = t_begin; tile < t_end; ++tile) {
            if (mark_lds && tile * GATHER_TILE >= cur_end) {            // (uniform over the workgroup)
                flush(cur_b);
                while (tile * GATHER_TILE >= cur_end) { ++cur_b; cur_end = cur_b + 1 < n_bases ? (is_q ? jobs[cur_b + 1].q_off : jobs[cur_b + 1].p_off) : 0xFFFFFFFFu; }
            }
            uint32_t e[GATHER_EPT], pr[GATHER_EPT], base[GATHER_EPT];
            bool live[GATHER_EPT];
            float inv[GATHER_EPT]; int eg[GATHER_EPT];
#pragma unroll
            for (int k = 0; k < GATHER_EPT; ++k) {
                const uint32_t ef = tile * GATHER_TILE + (uint32_t)k * 256u + wave * 64u;   // (uniform)
                e[k] = ef + lane;
                live[k] = e[k] < total;
                pr[k] = 0; base[k] = 0; inv[k] = 0.0f; eg[k] = 1;
                if (ef >= total) continue;
                const uint32_t el = min(ef + 63u, total - 1u);
                while (next_dst <= ef) load_segment(++sgu);
                if (el < next_dst) {                    // the 64 entries lie in one segment: nothing but the pair load
                    if (live[k]) { pr[k] = pairs[sg_src + (e[k] - sg_dst)]; base[k] = sg_base; inv[k] = ju; eg[k] = (int)gu; }
                } else if (live[k]) {                   // a wavefront across a boundary: per-lane walk from the uniform segment
                    int sgi = sgu;
                    while (sgi + 1 < nseg && segs[sgi + 1].dst <= e[k]) ++sgi;
                    const Segment sg = segs[sgi];
                    pr[k] = pairs[sg.src + (e[k] - sg.dst)];
                    base[k] = sg.base;
                    const BaseJob& J = jobs[sg.base];
                    inv[k] = is_q ? J.inv2 : J.inv1; eg[k] = J.egSize;
                }
            }
            float4 a1[GATHER_EPT], a2[GATHER_EPT];
#pragma unroll
            for (int k = 0; k < GATHER_EPT; ++k) { a1[k] = munit[pr[k] >> 16]; a2[k] = munit[pr[k] & 0xFFFF]; }
#pragma unroll
            for (int k = 0; k < GATHER_EPT; ++k) {
                if (!live[k]) continue;
                const V3 p1 = mk3(a1[k].x, a1[k].y, a1[k].z), p2 = mk3(a2[k].x, a2[k].y, a2[k].z);
                const int64_t pc = index_pos(p1 + inv[k] * (p2 - p1), 0.0f, eg[k]);
                const bool no_cell = pc < 0 || pc >= cell_limit;
                const KeyT key = ((KeyT)base[k] << cell_bits) | (no_cell ? cmask : (KeyT)pc);
                keys[e[k]] = key;
                vals[e[k]] = pr[k];
                if (occ && !no_cell) {
                    if (mark_lds && base[k] == cur_b) atomicOr(&s_occ[(uint32_t)pc >> 5], 1u << ((uint32_t)pc & 31u));
                    else atomicOr(&occ[(size_t)(key >> 5)], 1u << ((uint32_t)key & 31u));
                }
            }
        }
        if (mark_lds) flush(cur_b);
    }(is_q ? Q.keys : P.keys, is_q ? Q.vals : P.vals, is_q ? Q.occ : P.occ);
}

// ---- survivors ----
// A P entry can only ever be matched by a Q entry of the same (base, position cell) and the other way round (Q9: only the
// query's own cell is inspected), and on the metric workload three entries out of four have no partner cell at all (CPU census
// of a Cm trial: 23 % of 7.9 M Q entries and 27 % of 10 M P entries do).  So each gather also marks the cells its list occupies,
// and both lists are reduced to the entries whose cell the OTHER list occupies -- in gather order, so the stable sorts that
// follow see the same relative order -- before anything is sorted: the sorts, the records and the join work on a quarter of
// the entries.  Entries dropped here have an empty partner run: they contribute no quad and no rank of the walk order.
#define SURV_TILE 1024
template <class KeyT>
__device__ __forceinline__ bool occ_test(const uint32_t* __restrict__ occ, KeyT key) { return (occ[(size_t)(key >> 5)] >> ((uint32_t)key & 31u)) & 1u; }

// per tile of SURV_TILE entries: how many survive.  A workgroup takes a run of consecutive GROUPS of four tiles, wavefront w of it the w-th
// tile of the group: its 16 rows of 64 keys are requested together (the round-4 form took one tile per trip of the whole workgroup -- four
// loads per thread in flight between two barriers, ~10 us per trip: 0.4 TB/s over a 40-trial piece), its count is its own (no reduction
// across wavefronts), its 16 ballots leave as one 128-byte store.  lds_words > 0: the OTHER list's bits of the base that holds the group's
// middle entry sit in LDS (2^cell_bits / 8 bytes, loaded when that base changes -- one barrier per group, two more on a change), so the
// test of an entry of that base is an LDS read -- the byte table of rounds 3-4a was gathered from device memory per entry and missed the
// L2 half of the time (3.2 MB per list and trial against a 4 MB L2 that the lists stream through).  Entries of another base read the
// table directly.
#define SURV_ROWS (SURV_TILE / 64)
template <class KeyT>
__global__ __launch_bounds__(256) void survivors_count_kernel(ListSide<KeyT> P, ListSide<KeyT> Q, int side0, const PlanOut* __restrict__ po, uint32_t lds_words, int cell_bits) {
    const int is_q = side0 + (int)blockIdx.y;
    const KeyT* __restrict__ keys = is_q ? Q.keys : P.keys;
    uint32_t n = is_q ? Q.n : P.n;
    const uint32_t* __restrict__ other = is_q ? Q.other : P.other;
    uint32_t* __restrict__ tile_cnt = is_q ? Q.tiles : P.tiles;
    unsigned long long* __restrict__ alive_bits = is_q ? Q.alive : P.alive;
    extern __shared__ uint32_t s_occ[];
    __shared__ KeyT s_mid[2];
    if (po) { if (po->overflow) return; const unsigned long long t = is_q ? po->totQ : po->totP; n = t < (unsigned long long)n ? (uint32_t)t : n; }   // (overflow: the gather wrote nothing)
    const uint32_t n_tiles = (n + SURV_TILE - 1u) / SURV_TILE, n_groups = (n_tiles + 3u) / 4u;
    const uint32_t per_wg = (n_groups + gridDim.x - 1u) / gridDim.x;
    const uint32_t g_begin = blockIdx.x * per_wg, g_end = min(n_groups, g_begin + per_wg);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const KeyT cmask = ((KeyT)1 << cell_bits) - (KeyT)1;
    KeyT cur = ~(KeyT)0;                 // base whose bits are in LDS
    for (uint32_t g = g_begin; g < g_end; ++g) {
        const uint32_t tile = g * 4u + w, e0 = tile * SURV_TILE + lane;       // (n < 2^32 - 2^16: no wrap; a tile beyond the list loads nothing)
        KeyT key[SURV_ROWS];
#pragma unroll
        for (int k = 0; k < SURV_ROWS; ++k) { const uint32_t e = e0 + (uint32_t)k * 64u; key[k] = (tile < n_tiles && e < n) ? keys[e] : ~(KeyT)0; }
        if (lds_words) {
            // the group's middle entry is row 0, lane 0 of wavefront 2; a group that ends before it takes its first entry (wavefront 0)
            const bool has_mid = g * 4u * SURV_TILE + 2u * SURV_TILE < n;
            if (lane == 0u && w == (has_mid ? 2u : 0u)) s_mid[g & 1u] = key[0] >> cell_bits;
            __syncthreads();                                       // (also: every wavefront is done with the bits of the group before)
            const KeyT tb = s_mid[g & 1u];
            if (tb != cur) {                                       // (uniform)
                cur = tb;
                for (uint32_t i = threadIdx.x; i < lds_words; i += blockDim.x) s_occ[i] = other[(size_t)cur * lds_words + i];
                __syncthreads();
            }
        }
        if (tile >= n_tiles) continue;                             // (wave-uniform; the barriers above are behind it)
        uint32_t cnt = 0;
        unsigned long long mine = 0ull;
#pragma unroll
        for (int k = 0; k < SURV_ROWS; ++k) {
            const uint32_t e = e0 + (uint32_t)k * 64u;
            bool ob;
            if (e >= n) ob = false;
            else if (lds_words && (key[k] >> cell_bits) == cur) { const uint32_t cl = (uint32_t)(key[k] & cmask); ob = (s_occ[cl >> 5] >> (cl & 31u)) & 1u; }
            else ob = occ_test(other, key[k]);
            const unsigned long long am = __ballot(ob);            // (the all-ones cell is never marked)
            // one bit per entry, kept for the compaction: it then reads 8 bytes per row instead of testing again,
            // and loads the keys and pairs of the survivors only (a quarter of the entries)
            if (lane == (uint32_t)k) mine = am;
            cnt += (uint32_t)__popcll(am);
        }
        if (lane < (uint32_t)SURV_ROWS) alive_bits[(size_t)tile * SURV_ROWS + lane] = mine;
        if (lane == 0u) tile_cnt[tile] = cnt;
    }
}

// workgroup 0: P list, workgroup 1: Q list.  Tile counts -> tile offsets (element n_tiles receives the total)
__global__ __launch_bounds__(1024) void survivors_scan_kernel(uint32_t* __restrict__ tiles_p, uint32_t ntp, uint32_t* __restrict__ tiles_q, uint32_t ntq) {
    __shared__ uint32_t s_part[1024];
    const bool q = blockIdx.x == 1;
    block_scan_1024(q ? tiles_q : tiles_p, (q ? ntq : ntp) + 1u, s_part, [](uint32_t, uint32_t, uint32_t) {});
}

// The same scan for long lists (a trial batch: 10^5 tiles), on as many workgroups as it takes -- the single workgroup above walks 137 counts
// per thread, one at a time, for a 16-trial piece (137 us on one CU, 1.4 % of the batch).  Two launches: every workgroup scans its 4 096
// counts (coalesced loads into LDS, 16 per thread there) and writes their sum; then every workgroup adds the sums of the workgroups in
// front of it (a few dozen words, reduced by the workgroup itself) to its counts.  blockIdx.y: 0 = P list, 1 = Q list.
#define TSCAN 4096
__global__ __launch_bounds__(256) void tile_scan_local_kernel(uint32_t* __restrict__ tiles_p, uint32_t np, uint32_t* __restrict__ tiles_q, uint32_t nq, uint32_t* __restrict__ part,
                                                              uint32_t parts_p) {
    __shared__ uint32_t s_v[TSCAN + 16];
    __shared__ uint32_t s_w[4];
    const bool q = blockIdx.y == 1;
    uint32_t* a = q ? tiles_q : tiles_p;
    const uint32_t n = q ? nq : np;
    const uint32_t base = blockIdx.x * TSCAN;
    if (base >= n) return;
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
#pragma unroll
    for (int j = 0; j < TSCAN / 256; ++j) { const uint32_t i = base + (uint32_t)j * 256u + t; s_v[(uint32_t)j * 256u + t] = i < n ? a[i] : 0u; }
    __syncthreads();
    uint32_t v[16], sum = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) { v[j] = s_v[t * 16u + (uint32_t)j]; sum += v[j]; }
    uint32_t inc = sum;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t x = __shfl_up(inc, o, 64); if (lane >= (uint32_t)o) inc += x; }
    if (lane == 63u) s_w[w] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (uint32_t x = 0; x < w; ++x) run += s_w[x];
#pragma unroll
    for (int j = 0; j < 16; ++j) { s_v[t * 16u + (uint32_t)j] = run; run += v[j]; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TSCAN / 256; ++j) { const uint32_t i = base + (uint32_t)j * 256u + t; if (i < n) a[i] = s_v[(uint32_t)j * 256u + t]; }
    if (t == 255u) part[(q ? parts_p : 0u) + blockIdx.x] = run;
}
__global__ __launch_bounds__(256) void tile_scan_add_kernel(uint32_t* __restrict__ tiles_p, uint32_t np, uint32_t* __restrict__ tiles_q, uint32_t nq, const uint32_t* __restrict__ part,
                                                            uint32_t parts_p) {
    __shared__ uint32_t s_w[4];
    const bool q = blockIdx.y == 1;
    uint32_t* a = q ? tiles_q : tiles_p;
    const uint32_t n = q ? nq : np;
    const uint32_t base = blockIdx.x * TSCAN;
    if (base >= n || blockIdx.x == 0) return;
    const uint32_t* mine = part + (q ? parts_p : 0u);
    uint32_t acc = 0;
    for (uint32_t j = threadIdx.x; j < blockIdx.x; j += 256u) acc += mine[j];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    const uint32_t off = s_w[0] + s_w[1] + s_w[2] + s_w[3];
#pragma unroll
    for (int j = 0; j < TSCAN / 256; ++j) { const uint32_t i = base + (uint32_t)j * 256u + threadIdx.x; if (i < n) a[i] += off; }
}

// Where every base's stretch begins and ends in the reduced lists (the lists are base-major, so that is the number of
// survivors in front of the stretch's old bounds: the offset of the tile a bound falls into plus the survivors of that
// tile in front of it), patched into the base jobs and the offset arrays the join reads.  Workgroup (b, list).
template <class KeyT>
__global__ __launch_bounds__(256) void survivors_base_offsets_kernel(const KeyT* __restrict__ pkeys, uint32_t nP, const uint32_t* __restrict__ occ_q,
                                                                     const uint32_t* __restrict__ tiles_p, const KeyT* __restrict__ qkeys, uint32_t nQ,
                                                                     const uint32_t* __restrict__ occ_p, const uint32_t* __restrict__ tiles_q, int nB,
                                                                     BaseJob* __restrict__ jobs, uint32_t* __restrict__ p_off, uint32_t* __restrict__ q_off,
                                                                     const PlanOut* __restrict__ po) {
    __shared__ uint32_t s_w[2][4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool q = blockIdx.y == 1;
    // po != NULL: nP / nQ are the CAPACITIES the key buffers and the tile arrays were sized by, the base jobs carry the PLANNED
    // stretches.  A plan beyond a capacity is redone by the host with exact sizes (CountPass::capacity_check at the read-back), so this
    // launch has nothing to deliver -- and must not follow planned offsets past the gathered keys and the scanned tiles (the
    // unguarded form of round 4 read keys[e] beyond d_pk_raw / d_qk_raw and used what it found there as an occupancy index, up to
    // 512 MB past the table).  The test is uniform over the grid: either every workgroup works or none does.
    if (po && (po->overflow || po->totP > (unsigned long long)nP || po->totQ > (unsigned long long)nQ)) return;
    const KeyT* keys = q ? qkeys : pkeys;
    const uint32_t* other = q ? occ_p : occ_q;
    const uint32_t* tiles = q ? tiles_q : tiles_p;
    const uint32_t cap = q ? nQ : nP;
    uint32_t r0 = q ? jobs[b].q_off : jobs[b].p_off, r1 = r0 + (q ? jobs[b].q_len : jobs[b].p_len);
    r0 = min(r0, cap); r1 = min(max(r1, r0), cap);      // (belt and braces: tiles[] holds cap / SURV_TILE + 1 entries, keys[] cap)
    uint32_t got[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t r = h ? r1 : r0, t0 = (r / SURV_TILE) * SURV_TILE;
        uint32_t cnt = 0;
        for (uint32_t e = t0 + threadIdx.x; e < r; e += 256) cnt += occ_test(other, keys[e]) ? 1u : 0u;
        for (int d = 32; d; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
        if (lane == 0) s_w[h][w] = cnt;
        got[h] = tiles[r / SURV_TILE];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t n0 = got[0] + s_w[0][0] + s_w[0][1] + s_w[0][2] + s_w[0][3], n1 = got[1] + s_w[1][0] + s_w[1][1] + s_w[1][2] + s_w[1][3];
        if (q) { jobs[b].q_off = n0; jobs[b].q_len = n1 - n0; q_off[b] = n0; if (b == nB - 1) q_off[nB] = n1; }
        else   { jobs[b].p_off = n0; jobs[b].p_len = n1 - n0; p_off[b] = n0; if (b == nB - 1) { p_off[nB] = n1; q_off[nB + 1] = n1; } }   // q_off[nB + 1]: P's total rides along with the Q offsets
    }
}

// the survivors of a tile, in order, behind the tile's offset: one WAVEFRONT per tile (four tiles per workgroup), no LDS, no barrier -- the
// tile's 16 ballots arrive as one 128-byte load and are handed out through scalar registers, the 16 rows of the survivors' keys and pairs
// are requested together (the round-4 form: one workgroup per tile, four rows per thread, 75 000 workgroups for a 40-trial piece)
// combined (one launch for both lists, gridDim.y == 3): into ONE list -- P's survivors, then Q's right behind them (q_off[nB + 1] = P's total,
// written by survivors_base_offsets_kernel) -- so that ONE segmented sort over 2 nB segments sorts both (blockIdx.y == 2: its segment offsets,
// P's bases then Q's shifted by P's total).  Not combined: every list into its own buffers, no shift, no third plane.
template <class KeyT>
__global__ __launch_bounds__(256) void survivors_compact_kernel(ListSide<KeyT> P, ListSide<KeyT> Q, int side0, int combined, const PlanOut* __restrict__ po,
                                                                const uint32_t* __restrict__ p_off, const uint32_t* __restrict__ q_off, int nB, uint32_t* __restrict__ comb_off) {
    // A plan beyond the capacities is redone by the host: survivors_base_offsets_kernel wrote nothing then, the tile offsets belong to clamped
    // lists and q_off[nB + 1] is not P's total.  In every form: the two-stream launches leave here as well (they used to clamp and run); the
    // host discards that pass at its read-back (CountPass::capacity_check: *outgrown) whatever was compacted, so no result depends on it.
    if (po && (po->overflow || po->totP > (unsigned long long)P.n || po->totQ > (unsigned long long)Q.n)) return;
    if (combined && blockIdx.y == 2) {
        const uint32_t totP = q_off[nB + 1];
        for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i <= 2u * (uint32_t)nB; i += gridDim.x * 256u) comb_off[i] = i < (uint32_t)nB ? p_off[i] : totP + q_off[i - (uint32_t)nB];
        return;
    }
    // (ONE body for both lists, its arguments selected in front of it: two inlined bodies under an if / else took 248 VGPRs)
    const int is_q = side0 + (int)blockIdx.y;
    const uint32_t shift = (combined && is_q) ? q_off[nB + 1] : 0u;
    const KeyT* __restrict__ keys = is_q ? Q.keys : P.keys;
    const uint32_t* __restrict__ vals = is_q ? Q.vals : P.vals;
    uint32_t n = is_q ? Q.n : P.n;
    const unsigned long long* __restrict__ alive_bits = is_q ? Q.alive : P.alive;
    const uint32_t* __restrict__ tile_off = is_q ? Q.tiles : P.tiles;
    KeyT* __restrict__ okeys = (is_q ? Q.okeys : P.okeys) + shift;
    uint32_t* __restrict__ ovals = (is_q ? Q.ovals : P.ovals) + shift;
    if (po) n = (uint32_t)(is_q ? po->totQ : po->totP);      // the planned length (within the capacity: the test above)
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t tile = blockIdx.x * 4u + w;
    if ((unsigned long long)tile * SURV_TILE >= (unsigned long long)n) return;      // (wave-uniform)
    const unsigned long long mine = lane < (uint32_t)SURV_ROWS ? alive_bits[(size_t)tile * SURV_ROWS + lane] : 0ull;   // the count pass's ballots
    uint32_t base = tile_off[tile];
    const uint32_t e0 = tile * SURV_TILE + lane;
    KeyT key[SURV_ROWS];
    uint32_t val[SURV_ROWS];
    unsigned long long bm[SURV_ROWS];
#pragma unroll
    for (int k = 0; k < SURV_ROWS; ++k) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, k), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), k);
        bm[k] = ((unsigned long long)hi << 32) | lo;
        key[k] = (KeyT)0; val[k] = 0u;
        if ((bm[k] >> lane) & 1ull) { key[k] = keys[e0 + (uint32_t)k * 64u]; val[k] = vals[e0 + (uint32_t)k * 64u]; }       // survivors only (a set bit is an entry below n)
    }
#pragma unroll
    for (int k = 0; k < SURV_ROWS; ++k) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bm[k] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm[k], 0u));
        if ((bm[k] >> lane) & 1ull) { okeys[base + rank] = key[k]; ovals[base + rank] = val[k]; }
        base += (uint32_t)__popcll(bm[k]);
    }
}

}  // namespace stocs
#endif
