// refine_robust.h -- the three kernels of the trimmed form of the refinement (keep_ratio < 1).  Part of refine.hip's translation unit,
// included inside its namespace behind the device core (ref_source, ref_walk, ref_within, ref_normals_agree, ref_products, ref_reduce) they are composed
// from; the host side of both forms is refine.hip's.  Per hypothesis and iteration (include/stocs_hip.h states the contract):
//   match   one workgroup per (hypothesis, 256 source points): the walk; a matched pair that passes the double distance test and, with
//           the gate on, the normal test is a CANDIDATE.  Per (hypothesis, source position): the rank word (the bits of the float
//           squared distance the walk minimised; 0xFFFFFFFF for a non-candidate) and the model index.
//   select  one workgroup per live hypothesis: n_cand, k = floor(keep_ratio n_cand), and the k-th smallest (rank word, position) by
//           a radix select -- four passes of eight bits, a 256-bin LDS histogram under integer atomics (order-free), then one pass
//           in source order over the tie group at the cut (ballots and popcounts).  No float comparison, no sort.
//   kept    per (hypothesis, chunk): word < cut || (word == cut && i <= cut_i); the 28 products and their reduction as
//           refine_accumulate_kernel's, into the same partials; refine_solve_kernel consumes them unchanged.
struct RobustSel { uint32_t cut_word; int32_t cut_i, k, ncand; };   // kept: (word, i) <= (cut_word, cut_i); k = 0: cut_i = -1 keeps nothing

struct RobustArgs {
    const float4* snrm;   // the base scene's unit normals (xyz), never an instance-mode override
    int gate;             // 1: the normal test is on
    double min_cos;
    uint32_t* word;       // group x nsrc rank words
    int32_t* match;       // group x nsrc model indices (-1 none)
    RobustSel* sel;       // group
};

struct RobustNoDetail { static constexpr bool on = false; };
struct RobustDetailOut { static constexpr bool on = true; uint8_t* kept; };   // nsrc, preset to 0

// match: the rank word and the model index of every (hypothesis, source position)
template <bool kLds>
__global__ __launch_bounds__(256) void robust_match_kernel(RefArgs a, RobustArgs r, const RefHyp* __restrict__ hyp) {
    extern __shared__ float4 lds_pos[];
    uint32_t* lds_off = (uint32_t*)(lds_pos + a.nM);
    const int hk = blockIdx.x / a.nchunks, ch = blockIdx.x - hk * a.nchunks;
    const RefHyp* H = hyp + hk;
    if (H->frozen) return;
    ref_stage<kLds>(a, lds_pos, lds_off);
    const int i = ch * REFINE_CHUNK + (int)threadIdx.x;
    if (i >= a.nsrc) return;
    const int sidx = a.idx ? a.idx[i] : i;
    const RefSource s = ref_source(a, H, sidx);
    const uint64_t key = ref_walk<kLds>(a, s.fx, s.fy, s.fz, lds_pos, lds_off);
    const uint32_t id = (uint32_t)key;
    const bool cand = id != 0xFFFFFFFFu && ref_within(a, id, s) && (!r.gate || ref_normals_agree(a, r.snrm, r.min_cos, H, id, sidx));
    const size_t at = (size_t)hk * a.nsrc + i;
    r.word[at] = cand ? (uint32_t)(key >> 32) : 0xFFFFFFFFu;   // (a squared distance has its sign bit clear: never this word)
    r.match[at] = (int32_t)id;
}

// select: one workgroup per live hypothesis -> (cut word, cut position, k, n_cand).  Integer logic alone: the histogram's atomics
// commute, the tie pass runs in source order.
__global__ __launch_bounds__(256) void robust_select_kernel(const RefHyp* __restrict__ hyp, int nsrc, float keep, const uint32_t* __restrict__ word,
                                                            RobustSel* __restrict__ sel) {
    const int hk = blockIdx.x;
    if (hyp[hk].frozen) return;
    const uint32_t* W = word + (size_t)hk * nsrc;
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t s_bin, s_before, s_ncand;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t prefix = 0, mask = 0, remaining = 0;
    int k = 0, ncand = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        hist[t] = 0;
        if (pass == 0 && t == 0) s_ncand = 0;
        __syncthreads();
        uint32_t mine = 0;
        for (int i = t; i < nsrc; i += 256) {
            const uint32_t w = W[i];
            if (w == 0xFFFFFFFFu) continue;
            ++mine;
            if ((w & mask) == prefix) atomicAdd(&hist[(w >> shift) & 255u], 1u);
        }
        if (pass == 0 && mine) atomicAdd(&s_ncand, mine);
        __syncthreads();
        if (pass == 0) {
            ncand = (int)s_ncand;
            k = (int)floor((double)keep * (double)ncand);   // exact: a 24-bit times a 31-bit integer
            if (k <= 0) {   // uniform over the workgroup
                if (t == 0) { RobustSel o; o.cut_word = 0; o.cut_i = -1; o.k = 0; o.ncand = ncand; sel[hk] = o; }
                return;
            }
            remaining = (uint32_t)k;
        }
        // inclusive scan of the 256 bins; the bin that holds the remaining-th smallest
        const uint32_t h = hist[t];
        uint32_t inc = h;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        for (int w2 = 0; w2 < wave; ++w2) inc += wsum[w2];
        if (h && inc >= remaining && inc - h < remaining) { s_bin = (uint32_t)t; s_before = inc - h; }
        __syncthreads();
        prefix |= s_bin << shift; mask |= 255u << shift; remaining -= s_before;
        __syncthreads();   // s_bin, wsum and hist are rewritten by the next pass
    }
    // the tie group at the cut, in source order: the remaining-th position whose word is the cut word
    uint32_t running = 0;
    for (int base = 0; base < nsrc; base += 256) {
        const int i = base + t;
        const bool f = i < nsrc && W[i] == prefix;
        const unsigned long long b = __ballot(f);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = running;
        for (int w2 = 0; w2 < wave; ++w2) before += wsum[w2];
        const uint32_t total = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        before += (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (f && before + 1u == remaining) { RobustSel o; o.cut_word = prefix; o.cut_i = i; o.k = k; o.ncand = ncand; sel[hk] = o; }
        running += total;
        __syncthreads();
        if (running >= remaining) break;   // uniform
    }
}

// kept accumulation: the products of the pairs at or below the cut
template <class Detail>
__global__ __launch_bounds__(256) void robust_kept_kernel(RefArgs a, RobustArgs r, const RefHyp* __restrict__ hyp, double* __restrict__ partial, Detail det) {
    const int hk = blockIdx.x / a.nchunks, ch = blockIdx.x - hk * a.nchunks;
    const RefHyp* H = hyp + hk;
    if (H->frozen) return;
    const int i = ch * REFINE_CHUNK + (int)threadIdx.x;
    double v[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) v[k] = 0.0;
    if (i < a.nsrc) {
        const RobustSel s = r.sel[hk];
        const size_t at = (size_t)hk * a.nsrc + i;
        const uint32_t w = r.word[at];
        if (w < s.cut_word || (w == s.cut_word && i <= s.cut_i)) {
            const RefSource src = ref_source(a, H, a.idx ? a.idx[i] : i);
            ref_products(a, (uint32_t)r.match[at], src, v);
            if constexpr (Detail::on) det.kept[i] = 1;
        }
    }
    ref_reduce(v, partial);
}

