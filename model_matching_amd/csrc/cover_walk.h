// cover_walk.h -- the greedy cover walk that instances.hip (rows over scene points) and scene.hip (rows over pixels) share: rows of Wp
// words (a multiple of four, zero padded) are walked in a given order and one is selected when enough of its bits are not in the
// cover of those selected before it.  Once each: the order key, the exclusive count of a row against a cover, the OR of a row into the
// cover, the round loop (a gate in front of the row read is what the two selections differ in), and on the host the ordering sort and
// the read-back region records | selected | count.  The two __global__ select kernels stay in their files and carve their own LDS.
#ifndef STOCS_COVER_WALK_H
#define STOCS_COVER_WALK_H

#include <string.h>

#include "prims.h"
#include "stocs_ctx.h"
#include "wave_bits.h"

namespace stocs {

enum { COVER_WAVES = 16 };   // wavefronts of a select kernel = rows tested per round

struct CoverArgs { int32_t max_selected, min_count; float min_fraction; };

// ~stocs_pack_best(s, h): the ascending stable sort walks the keys downwards, the keys 0 (s not positive) in index order
__device__ __forceinline__ uint64_t cover_order_key(float s, int h) { return ~(s > 0.0f ? (uint64_t)best_key(s, (uint32_t)h) : (uint64_t)0); }

// |row \ cover| by one wavefront, the same in every lane; W4 = Wp / 4
__device__ __forceinline__ int cover_exclusive(const uint4* __restrict__ row, const uint4* cov, int W4, int lane) {
    int ex = 0;
    for (int i = lane; i < W4; i += 64) ex += popc_andnot4(row[i], cov[i]);
    return wave_sum_i(ex);
}

// cover |= row, by the whole workgroup
__device__ __forceinline__ void cover_or(uint4* cov, const uint4* __restrict__ row, int W4, int tid, int threads) {
    for (int i = tid; i < W4; i += threads) { const uint4 e = row[i]; uint4 c = cov[i]; c.x |= e.x; c.y |= e.y; c.z |= e.z; c.w |= e.w; cov[i] = c; }
}

// The walk, by ONE workgroup of COVER_WAVES wavefronts; p (first position of the order not yet decided) and nsel are the same in every
// thread.  Each round wavefront k tests the k-th pending row against the cover; the first that passes is selected, those before it are
// dropped for good (the cover only grows), those behind it stay pending and are tested again.  cov: Wp words of LDS; r: 3 x COVER_WAVES
// words of LDS, the round's results.  gate.open(h) is evaluated wave-uniformly in front of the row read (a closed row is not read and
// does not pass); gate.took(h, k) is called by thread 0 when h, the row of wavefront k, is selected.  Whatever took() writes, open()
// reads in front of the round's first barrier and took() writes behind it.  open() may also leave per-wavefront state in LDS for took(h, k)
// (its own wavefront's word, written by one lane: scene.hip keeps the row's group there); took() runs between the round's two barriers
// and open() is next called behind the second, so such a word needs no barrier of its own.  A wavefront without a row (past the end of the
// order) does not call open(), its word is stale and, as it cannot pass, never read.  Stores rank (-1 for the unselected), excl of the
// selected, the selected list, its length and the final cover; the last barrier of the loop is behind every write of the gate's.
template <class Gate>
__device__ __forceinline__ void cover_walk(const uint32_t* __restrict__ rows, int Wp, const uint32_t* __restrict__ order, const int32_t* __restrict__ own, int n,
                                           const CoverArgs a, Gate gate, uint4* cov, int* r, int32_t* __restrict__ rank, int32_t* __restrict__ excl,
                                           int32_t* __restrict__ selected, int32_t* __restrict__ n_selected, uint32_t* __restrict__ cover_out) {
    int* r_pass = r;
    int* r_excl = r_pass + COVER_WAVES;
    int* r_h = r_excl + COVER_WAVES;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int threads = 64 * COVER_WAVES;
    const int W4 = Wp >> 2;
    for (int i = tid; i < W4; i += threads) cov[i] = make_uint4(0u, 0u, 0u, 0u);
    for (int i = tid; i < n; i += threads) rank[i] = -1;
    __syncthreads();
    int p = 0, nsel = 0;
    while (p < n && nsel < a.max_selected) {
        const int pos = p + wave;
        int h = -1, ex = 0, pass = 0;
        if (pos < n) {   // wave-uniform
            h = (int)order[pos];
            if (gate.open(h)) {
                const int o = own[h];
                ex = cover_exclusive((const uint4*)(rows + (size_t)h * (size_t)Wp), cov, W4, lane);
                pass = (ex >= a.min_count && (float)ex >= a.min_fraction * (float)o) ? 1 : 0;
            }
        }
        if (lane == 0) { r_pass[wave] = pass; r_excl[wave] = ex; r_h[wave] = h; }
        __syncthreads();
        int k = -1;
#pragma unroll
        for (int j = COVER_WAVES - 1; j >= 0; --j) k = r_pass[j] ? j : k;   // the first that passes, in order
        if (k < 0) {
            p += COVER_WAVES;   // all sixteen fail against a subset of their final cover (and gate): dropped
        } else {
            const int hs = r_h[k];
            cover_or(cov, (const uint4*)(rows + (size_t)hs * (size_t)Wp), W4, tid, threads);
            if (tid == 0) { rank[hs] = nsel; excl[hs] = r_excl[k]; selected[nsel] = hs; gate.took(hs, k); }
            ++nsel;
            p += k + 1;   // those in front of it are dropped, those behind it are tested again
        }
        __syncthreads();
    }
    uint4* co = (uint4*)cover_out;
    for (int i = tid; i < W4; i += threads) co[i] = cov[i];
    if (tid == 0) *n_selected = nsel;
}

// first half of the finish kernels: the exclusive count of row h by its wavefront -- against the final cover for an unselected row
// (rank < 0), the walk's own figure for a selected one
__device__ __forceinline__ int cover_final_exclusive(const uint32_t* __restrict__ rows, int Wp, const uint32_t* __restrict__ cover, const int32_t* __restrict__ excl, int h,
                                                     int rank, int lane) {
    if (rank < 0) return cover_exclusive((const uint4*)(rows + (size_t)h * (size_t)Wp), (const uint4*)cover, Wp >> 2, lane);
    return excl[h];
}

// ---- host side: what surrounds the select and finish launches of a call ----
// The read-back region, records | selected | count: the same offsets on the device and in its pinned mirror.
struct CoverBack {
    size_t o_rec, o_sel, o_cnt, total, rec_bytes, sort_bytes;
    // n records of rec_size bytes, at most max_sel selected; the scratch the ordering sort of n keys needs
    int plan(stocs_ctx* c, int n, size_t rec_size, int max_sel) {
        Carve bk;
        rec_bytes = (size_t)n * rec_size;
        o_rec = bk.take(rec_bytes); o_sel = bk.take((size_t)max_sel * 4); o_cnt = bk.take(4);
        total = bk.total;
        sort_bytes = 0;
        STOCS_HIP_CHECK(sort_pairs(NULL, sort_bytes, (const uint64_t*)NULL, (uint64_t*)NULL, (const uint32_t*)NULL, (uint32_t*)NULL, (size_t)n, 0, 64, c->stream));
        return STOCS_OK;
    }
    // one 64-bit radix sort of the complemented keys with the indices as values: ascending and stable
    int order(stocs_ctx* c, void* sort_tmp, const uint64_t* key, uint64_t* key_s, const uint32_t* idx, uint32_t* idx_s, int n) const {
        size_t tb = sort_bytes;
        STOCS_HIP_CHECK(sort_pairs(sort_tmp, tb, key, key_s, idx, idx_s, (size_t)n, 0, 64, c->stream));
        return STOCS_OK;
    }
    // the region into its pinned mirror, the call's ONE synchronisation, results to the caller
    int read_back(stocs_ctx* c, const char* d_back, char* h_back, void* out, int32_t* selected, int* n_selected) const {
        STOCS_HIP_CHECK(hipMemcpyAsync(h_back, d_back, total, hipMemcpyDeviceToHost, c->stream));
        STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
        const int ns = *(const int32_t*)(h_back + o_cnt);
        memcpy(out, h_back + o_rec, rec_bytes);
        memcpy(selected, h_back + o_sel, (size_t)ns * 4);
        *n_selected = ns;
        return STOCS_OK;
    }
};

}  // namespace stocs

#endif
