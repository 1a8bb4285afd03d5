// refine_robust.h -- the trimmed, normal-gated form of the batched refinement (stocs_refine_poses_robust, stocs_refine_robust_detail).
// Part of refine.hip's translation unit (included at its end): it shares RefHyp, RefArgs, the model grid, the workspace and the
// init / solve / final kernels with the plain form and leaves every one of them as it is.  The walk below is this file's OWN COPY of
// refine_accumulate_kernel's (same octant switch, margins, key and tie rule); the plain kernels are not touched.
//
// Per hypothesis and iteration (include/stocs_hip.h states the contract):
//   match   one workgroup per (hypothesis, 256 source points): the plain walk; a matched pair that passes the double distance test
//           and, with the gate on, the normal test is a CANDIDATE.  Per (hypothesis, source position): the rank word (the bits of
//           the float squared distance the walk minimised; 0xFFFFFFFF for a non-candidate) and the model index.
//   select  one workgroup per live hypothesis: n_cand, k = floor(keep_ratio n_cand), and the k-th smallest (rank word, position) by
//           a radix select -- four passes of eight bits, a 256-bin LDS histogram under integer atomics (order-free), then one pass
//           in source order over the tie group at the cut (ballots and popcounts).  No float comparison, no sort.
//   kept    per (hypothesis, chunk): word < cut || (word == cut && i <= cut_i); the 28 products and their reduction are the plain
//           kernel's expressions in the plain kernel's order, into the same partials; refine_solve_kernel consumes them unchanged.
// keep_ratio == 1 keeps every candidate: match, select and kept fold into ONE launch per iteration (robust_fused_kernel), which with
// the gate off computes bit for bit what refine_accumulate_kernel does.
//
// robust_enqueue is the enqueue form (the counterpart of refine_enqueue) behind stocs_run_trials_post_robust and
// stocs_track_poses_robust: the same launches on device-resident hypotheses, in groups of consecutive hypotheses that share the
// workspace (robust_plan), no copy, no synchronisation.
#include <stdlib.h>

namespace stocs {

struct RobustSel { uint32_t cut_word; int32_t cut_i, k, ncand; };   // kept: (word, i) <= (cut_word, cut_i); k = 0: cut_i = -1 keeps nothing

struct RobustArgs {
    const float4* snrm;   // the base scene's unit normals (xyz), never an instance-mode override
    int gate;             // 1: the normal test is on
    double min_cos;
    uint32_t* word;       // n x nsrc rank words
    int32_t* match;       // n x nsrc model indices (-1 none)
    RobustSel* sel;       // n
};

struct RobustWork { uint32_t* d_word; int32_t* d_match; RobustSel* d_sel; };

struct RobustNoDetail { static constexpr bool on = false; };
struct RobustDetailOut { static constexpr bool on = true; uint8_t* kept; };   // nsrc, preset to 0

// the source point in the model frame: as a caller would hand it over (float), then the running estimate in double
struct RbSource { double sx, sy, sz; float fx, fy, fz; };
__device__ __forceinline__ RbSource rb_source(const RefArgs& a, const RefHyp* H, int sidx) {
    const float4 x = a.spos[sidx];
    const double* Ti = H->Tinv;
    const double* U = H->U;
    const float s0x = (float)(Ti[0] * x.x + Ti[1] * x.y + Ti[2] * x.z + Ti[3]);
    const float s0y = (float)(Ti[4] * x.x + Ti[5] * x.y + Ti[6] * x.z + Ti[7]);
    const float s0z = (float)(Ti[8] * x.x + Ti[9] * x.y + Ti[10] * x.z + Ti[11]);
    RbSource s;
    s.sx = U[0] * s0x + U[1] * s0y + U[2] * s0z + U[3];
    s.sy = U[4] * s0x + U[5] * s0y + U[6] * s0z + U[7];
    s.sz = U[8] * s0x + U[9] * s0y + U[10] * s0z + U[11];
    s.fx = (float)s.sx; s.fy = (float)s.sy; s.fz = (float)s.sz;
    return s;
}

// refine_accumulate_kernel's walk: (squared distance bits, model index) of the nearest model point below the search bound, the
// lowest index on equal distance; the start value (bound, index -1) when there is none or the point lies outside the widened box
template <bool kLds>
__device__ __forceinline__ uint64_t rb_walk(const RefArgs& a, float fx, float fy, float fz, const float4* lds_pos, const uint32_t* lds_off) {
    uint64_t key = ((uint64_t)__float_as_uint(a.max_d2_f) << 32) | 0xFFFFFFFFull;
    if (!(fx >= a.lox && fx <= a.hix && fy >= a.loy && fy <= a.hiy && fz >= a.loz && fz <= a.hiz)) return key;
    const float ux = (fx - a.ox) * a.inv_h, uy = (fy - a.oy) * a.inv_h, uz = (fz - a.oz) * a.inv_h;
    const int cx = min(max((int)floorf(ux), -1), a.nx);
    const int cy = min(max((int)floorf(uy), -1), a.ny);
    const int cz = min(max((int)floorf(uz), -1), a.nz);
    auto gap = [&](float u, float lo, float hi) { return fmaxf(fmaxf(lo - u, u - hi) - a.margin_u, 0.0f); };
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
        for (int o = 0; o < 8; o += a.octants ? 1 : 8) {
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

// a matched pair is a candidate: the plain double distance test and, with the gate on, c = (g.x n.x + g.y n.y) + g.z n.z >= min_cos
// with g = U_R (Tinv_R ns) in double, one operation at a time, left to right (g is not normalised)
__device__ __forceinline__ bool rb_candidate(const RefArgs& a, const RobustArgs& r, const RefHyp* H, uint32_t id, int sidx, const RbSource& s) {
    const float4 t = a.mpos[id];
    const double ddx = s.sx - t.x, ddy = s.sy - t.y, ddz = s.sz - t.z;
    if (!(ddx * ddx + ddy * ddy + ddz * ddz <= a.max_d2)) return false;
    if (!r.gate) return true;
    const float4 ns = r.snrm[sidx], nn = a.mnrm[id];
    const double* Ti = H->Tinv;
    const double* U = H->U;
    const double qx = Ti[0] * ns.x + Ti[1] * ns.y + Ti[2] * ns.z;
    const double qy = Ti[4] * ns.x + Ti[5] * ns.y + Ti[6] * ns.z;
    const double qz = Ti[8] * ns.x + Ti[9] * ns.y + Ti[10] * ns.z;
    const double gx = U[0] * qx + U[1] * qy + U[2] * qz;
    const double gy = U[4] * qx + U[5] * qy + U[6] * qz;
    const double gz = U[8] * qx + U[9] * qy + U[10] * qz;
    const double c = (gx * nn.x + gy * nn.y) + gz * nn.z;
    return c >= r.min_cos;
}

// the 28 products of one kept pair: refine_accumulate_kernel's expressions
__device__ __forceinline__ void rb_products(const RefArgs& a, uint32_t id, const RbSource& s, double* v) {
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

// refine_accumulate_kernel's reduction: lane, butterfly, four waves in order -> one partial per workgroup
__device__ __forceinline__ void rb_reduce(double* v, double* __restrict__ partial) {
    __shared__ double red[REFINE_CHUNK / 64][28];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (__any(v[27] != 0.0)) {
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int k = 0; k < 28; ++k) v[k] += __shfl_xor(v[k], o, 64);
    }
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 28; ++k) red[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 28) partial[(size_t)blockIdx.x * 28 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

template <bool kLds>
__device__ __forceinline__ void rb_stage(const RefArgs& a, float4* lds_pos, uint32_t* lds_off) {
    if (kLds) {
        for (int j = threadIdx.x; j < a.nM; j += REFINE_CHUNK) lds_pos[j] = a.gpos[j];
        for (int j = threadIdx.x; j <= a.nsub; j += REFINE_CHUNK) lds_off[j] = a.off[j];
        __syncthreads();
    }
}

// match: the rank word and the model index of every (hypothesis, source position)
template <bool kLds>
__global__ __launch_bounds__(256) void robust_match_kernel(RefArgs a, RobustArgs r, const RefHyp* __restrict__ hyp) {
    extern __shared__ float4 lds_pos[];
    uint32_t* lds_off = (uint32_t*)(lds_pos + a.nM);
    const int hk = blockIdx.x / a.nchunks, ch = blockIdx.x - hk * a.nchunks;
    const RefHyp* H = hyp + hk;
    if (H->frozen) return;
    rb_stage<kLds>(a, lds_pos, lds_off);
    const int i = ch * REFINE_CHUNK + (int)threadIdx.x;
    if (i >= a.nsrc) return;
    const int sidx = a.idx ? a.idx[i] : i;
    const RbSource s = rb_source(a, H, sidx);
    const uint64_t key = rb_walk<kLds>(a, s.fx, s.fy, s.fz, lds_pos, lds_off);
    const uint32_t id = (uint32_t)key;
    const bool cand = id != 0xFFFFFFFFu && rb_candidate(a, r, H, id, sidx, s);
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

// kept accumulation: the products of the pairs at or below the cut, reduced as the plain kernel reduces
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
            const RbSource src = rb_source(a, H, a.idx ? a.idx[i] : i);
            rb_products(a, (uint32_t)r.match[at], src, v);
            if constexpr (Detail::on) det.kept[i] = 1;
        }
    }
    rb_reduce(v, partial);
}

// keep_ratio == 1: every candidate is kept, so one launch walks, tests and accumulates (gate off: refine_accumulate_kernel's results)
template <bool kLds>
__global__ __launch_bounds__(256) void robust_fused_kernel(RefArgs a, RobustArgs r, const RefHyp* __restrict__ hyp, double* __restrict__ partial) {
    extern __shared__ float4 lds_pos[];
    uint32_t* lds_off = (uint32_t*)(lds_pos + a.nM);
    const int hk = blockIdx.x / a.nchunks, ch = blockIdx.x - hk * a.nchunks;
    const RefHyp* H = hyp + hk;
    if (H->frozen) return;
    rb_stage<kLds>(a, lds_pos, lds_off);
    const int i = ch * REFINE_CHUNK + (int)threadIdx.x;
    double v[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) v[k] = 0.0;
    if (i < a.nsrc) {
        const int sidx = a.idx ? a.idx[i] : i;
        const RbSource s = rb_source(a, H, sidx);
        const uint64_t key = rb_walk<kLds>(a, s.fx, s.fy, s.fz, lds_pos, lds_off);
        const uint32_t id = (uint32_t)key;
        if (id != 0xFFFFFFFFu && rb_candidate(a, r, H, id, sidx, s)) rb_products(a, id, s, v);
    }
    rb_reduce(v, partial);
}

static const char* robust_check_params(const stocs_refine_robust_params* p) {
    if (!p) return "NULL params";
    if (p->max_iterations < 0) return "max_iterations < 0";
    if (!(p->max_correspondence_distance > 0.0f) || !isfinite(p->max_correspondence_distance)) return "correspondence distance must be positive and finite";
    if (!(p->keep_ratio > 0.0f && p->keep_ratio <= 1.0f)) return "keep_ratio must be in (0, 1]";
    if (!(p->min_normal_cos <= 1.0f)) return "min_normal_cos must be <= 1 (below -1: gate off)";
    return NULL;
}

// the robust workspace behind refine_prepare's: rank words | model indices | select results (grow-only, freed with the state)
static int robust_prepare(stocs_ctx* c, int n, int nsrc, RobustWork* rw) {
    RefineState* S = (RefineState*)c->refine;
    const size_t cells = (size_t)n * (size_t)std::max(nsrc, 1);
    Carve cv;
    const size_t o_word = cv.take(cells * 4), o_match = cv.take(cells * 4), o_sel = cv.take((size_t)n * sizeof(RobustSel));
    { const int rc = S->robust.grow(c->stream, cv.total); if (rc) return rc; }
    rw->d_word = Carve::at<uint32_t>(S->robust.p, o_word); rw->d_match = Carve::at<int32_t>(S->robust.p, o_match);
    rw->d_sel = Carve::at<RobustSel>(S->robust.p, o_sel);
    return STOCS_OK;
}

static RobustArgs robust_args(stocs_ctx* c, const RefineWork& w, const RobustWork& rw, const stocs_refine_robust_params* p) {
    RobustArgs r;
    r.snrm = c->d_snrmw; r.gate = p->min_normal_cos >= -1.0f ? 1 : 0; r.min_cos = (double)p->min_normal_cos;
    r.word = rw.d_word; r.match = rw.d_match; r.sel = rw.d_sel;
    return r;
}

// one evaluation's launches in front of the solve: match, select, kept -- or the fused one when everything is kept
template <class Detail>
static int robust_enqueue_iteration(stocs_ctx* c, const RefineWork& w, const RefArgs& a, const RobustArgs& r, size_t lds_bytes, float keep, bool fused, Detail det) {
    const RefHyp* d_hyp = (const RefHyp*)w.d_hyp;
    const dim3 grid((unsigned)(w.n * w.nchunks)), block(REFINE_CHUNK);
    const bool lds = lds_bytes <= REFINE_LDS_BYTES;
    if (fused) {
        if (lds) hipLaunchKernelGGL(HIP_KERNEL_NAME(robust_fused_kernel<true>), grid, block, lds_bytes, c->stream, a, r, d_hyp, w.d_part);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(robust_fused_kernel<false>), grid, block, 0, c->stream, a, r, d_hyp, w.d_part);
        STOCS_HIP_CHECK(hipGetLastError());
        return STOCS_OK;
    }
    if (lds) hipLaunchKernelGGL(HIP_KERNEL_NAME(robust_match_kernel<true>), grid, block, lds_bytes, c->stream, a, r, d_hyp);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(robust_match_kernel<false>), grid, block, 0, c->stream, a, r, d_hyp);
    STOCS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(robust_select_kernel, dim3((unsigned)w.n), dim3(256), 0, c->stream, d_hyp, w.nsrc, keep, (const uint32_t*)r.word, r.sel);
    STOCS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(HIP_KERNEL_NAME(robust_kept_kernel<Detail>), grid, block, 0, c->stream, a, r, d_hyp, w.d_part, det);
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

static int robust_check_call(stocs_ctx* c, const char* who, const int32_t* src_idx, int n_src, const stocs_refine_robust_params* p) {
    if (n_src < 0) { set_error("%s: negative size (n_src %d)", who, n_src); return STOCS_ERR_INVALID; }
    if (const char* why = robust_check_params(p)) { set_error("%s: %s", who, why); return STOCS_ERR_INVALID; }
    if (c->nS <= 0) { set_error("%s: the context has no scene", who); return STOCS_ERR_STATE; }
    if (src_idx)
        for (int i = 0; i < n_src; ++i)
            if (src_idx[i] < 0 || src_idx[i] >= c->nS) { set_error("%s: src_idx[%d] = %d outside [0, %d)", who, i, src_idx[i], c->nS); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}

// The group rule of the enqueue form.  The workspace takes 8 bytes per (hypothesis, source point), and a batch piece's slots are an
// upper bound taken before the counts are known: n hypotheses are refined in groups of consecutive hypotheses, the largest run
// whose demand group x nsrc x 8 stays within STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES and at least one; only a source too large for
// ONE hypothesis is refused.  STOCS_REFINE_ROBUST_GROUP_BYTES (read per call) lowers the limit (tests: forces several groups).
// keep_ratio == 1 stores no rank words: one group.  Grows the workspace (may synchronise: nothing of it may be in flight).
int robust_plan(stocs_ctx* c, const char* who, int n, int nsrc, float keep_ratio, float min_normal_cos, RobustPlan* plan) {
    if (const char* why = robust_setting_error(keep_ratio, min_normal_cos)) { set_error("%s: %s", who, why); return STOCS_ERR_INVALID; }
    const uint64_t per = (uint64_t)std::max(nsrc, 1) * 8u;
    if (per > (uint64_t)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES) {
        set_error("%s: %d source points need %llu workspace bytes for one hypothesis, the limit is %llu", who, nsrc, (unsigned long long)per,
                  (unsigned long long)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES);
        return STOCS_ERR_INVALID;
    }
    uint64_t limit = (uint64_t)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES;
    if (const char* e = getenv("STOCS_REFINE_ROBUST_GROUP_BYTES")) { const long long v = atoll(e); if (v > 0 && (uint64_t)v < limit) limit = (uint64_t)v; }
    const bool fused = keep_ratio == 1.0f;
    const uint64_t fit = std::max<uint64_t>(limit / per, 1);
    plan->group = fused ? std::max(n, 1) : (int)std::min<uint64_t>(fit, (uint64_t)std::max(n, 1));
    plan->keep_ratio = keep_ratio; plan->min_normal_cos = min_normal_cos;
    RobustWork rw;
    return robust_prepare(c, fused ? 1 : plan->group, fused ? 1 : nsrc, &rw);
}

// init (d_live != NULL: hypothesis k takes part only when d_live[k]; a dead one starts frozen and every kernel below, the select
// included, leaves at its first test), then group by group max_iterations x (match, select, kept | fused, solve) on the shared
// workspace, then final and the LCP launch over all n -- on the stream, no copy, no synchronisation.  Input and outputs as
// refine_enqueue (w from refine_prepare over all n; every scene point is the source); w.d_nc is k of the last evaluated iteration.
// A hypothesis's launches see its own RefHyp, partials and workspace rows alone: the results do not depend on the grouping.
int robust_enqueue(stocs_ctx* c, const RefineWork& w, const RobustPlan& plan, const int32_t* d_live, int max_iterations, float max_correspondence_distance,
                   int* n_groups) {
    const int n = w.n;
    RefineState* S = (RefineState*)c->refine;
    const bool fused = plan.keep_ratio == 1.0f;
    const int group = std::max(1, std::min(plan.group, n));
    RobustWork rw;
    {   // robust_plan grew the block: this carves it again and allocates nothing
        const size_t had = S->robust.bytes;
        const int rc = robust_prepare(c, fused ? 1 : group, fused ? 1 : w.nsrc, &rw);
        if (rc) return rc;
        if (S->robust.bytes != had) { set_error("robust_enqueue: the workspace was not planned (robust_plan)"); return STOCS_ERR_STATE; }
    }
    RefHyp* d_hyp = (RefHyp*)w.d_hyp;
    const unsigned hblocks = (unsigned)((n + 63) / 64);
    hipLaunchKernelGGL(refine_init_kernel, dim3(hblocks), dim3(64), 0, c->stream, (const float*)w.d_Tin, n, d_live, d_hyp);
    STOCS_HIP_CHECK(hipGetLastError());
    size_t lds_bytes = 0;
    const RefArgs a = refine_args(c, w, false, max_correspondence_distance, &lds_bytes);
    stocs_refine_robust_params p;
    p.max_iterations = max_iterations; p.max_correspondence_distance = max_correspondence_distance; p.keep_ratio = plan.keep_ratio; p.min_normal_cos = plan.min_normal_cos;
    const RobustArgs r = robust_args(c, w, rw, &p);
    int groups = 0;
    for (int g0 = 0; g0 < n && max_iterations > 0; g0 += group, ++groups) {
        RefineWork v = w;   // the group's view: hypotheses g0 .. g0 + v.n, their partials; the workspace rows start at 0 again
        v.n = std::min(group, n - g0);
        v.d_hyp = d_hyp + g0;
        v.d_part = w.d_part + (size_t)g0 * (size_t)w.nchunks * 28;
        for (int it = 0; it < max_iterations; ++it) {
            if (w.nchunks > 0) {
                const int rc = robust_enqueue_iteration(c, v, a, r, lds_bytes, plan.keep_ratio, fused, RobustNoDetail());
                if (rc) return rc;
            }
            hipLaunchKernelGGL(refine_solve_kernel<RefNoDetail>, dim3((unsigned)v.n), dim3(64), 0, c->stream, (RefHyp*)v.d_hyp, (const double*)v.d_part, w.nchunks,
                               RefNoDetail());
            STOCS_HIP_CHECK(hipGetLastError());
        }
    }
    if (n_groups) *n_groups = groups;
    hipLaunchKernelGGL(refine_final_kernel, dim3(hblocks), dim3(64), 0, c->stream, (const float*)w.d_Tin, (const RefHyp*)d_hyp, n, c->centroid_scene,
                       c->centroid_model, w.d_Tout, w.d_Pout, w.d_nc, w.d_it);
    STOCS_HIP_CHECK(hipGetLastError());
    return launch_lcp(c, w.d_Tout, n, w.d_lcp, NULL, NULL, NULL, 0);
}

}  // namespace stocs

extern "C" int stocs_refine_poses_robust(stocs_ctx* c, const float* T16_in, int n, const int32_t* src_idx, int n_src, const stocs_refine_robust_params* p,
                                         float* T16_out, float* pose16_out, float* lcp_out, int32_t* n_corr_out, int32_t* n_cand_out, int32_t* iterations_out) {
    const char* who = "stocs_refine_poses_robust";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: negative size (n %d)", who, n); return STOCS_ERR_INVALID; }
    if (n > 0 && !T16_in) { set_error("%s: NULL hypotheses", who); return STOCS_ERR_INVALID; }
    { const int rc = robust_check_call(c, who, src_idx, n_src, p); if (rc) return rc; }
    if (n == 0) return STOCS_OK;
    const int nsrc = src_idx ? n_src : c->nS;
    {
        const int nchunks = (nsrc + REFINE_CHUNK - 1) / REFINE_CHUNK;
        if ((int64_t)n * std::max(nchunks, 1) >= ((int64_t)1 << 31)) { set_error("%s: %d hypotheses x %d chunks: too many workgroups", who, n, nchunks); return STOCS_ERR_INVALID; }
        if ((uint64_t)n * (uint64_t)nsrc * 8u > (uint64_t)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES) {
            set_error("%s: %d hypotheses x %d source points need %llu workspace bytes, the limit is %llu", who, n, nsrc, (unsigned long long)n * (unsigned long long)nsrc * 8ull,
                      (unsigned long long)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES);
            return STOCS_ERR_INVALID;
        }
    }
    DeviceGuard dev_guard(c->device);
    begin_scoring_call(c);
    RefineWork w;
    RobustWork rw;
    { const int rc = refine_prepare(c, n, nsrc, p->max_correspondence_distance, &w); if (rc) return rc; }
    const bool fused = p->keep_ratio == 1.0f;
    { const int rc = robust_prepare(c, fused ? 1 : n, fused ? 1 : nsrc, &rw); if (rc) return rc; }
    const size_t out_bytes = w.out_bytes, sel_bytes = (size_t)n * sizeof(RobustSel);
    const size_t in_bytes = al256((size_t)n * 64) + al256((size_t)(src_idx ? nsrc : 0) * 4);
    char* hin; char* hout;
    { const int rc = pinned_for(c, in_bytes, al256(out_bytes) + al256(sel_bytes), &hin, &hout); if (rc) return rc; }
    memcpy(hin, T16_in, (size_t)n * 64);
    if (src_idx && nsrc) memcpy(hin + al256((size_t)n * 64), src_idx, (size_t)nsrc * 4);
    STOCS_HIP_CHECK(hipMemcpyAsync(w.d_Tin, hin, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
    if (src_idx && nsrc) STOCS_HIP_CHECK(hipMemcpyAsync(w.d_idx, hin + al256((size_t)n * 64), (size_t)nsrc * 4, hipMemcpyHostToDevice, c->stream));
    RefHyp* d_hyp = (RefHyp*)w.d_hyp;
    const unsigned hblocks = (unsigned)((n + 63) / 64);
    hipLaunchKernelGGL(refine_init_kernel, dim3(hblocks), dim3(64), 0, c->stream, (const float*)w.d_Tin, n, (const int32_t*)NULL, d_hyp);
    STOCS_HIP_CHECK(hipGetLastError());
    if (!fused) STOCS_HIP_CHECK(hipMemsetAsync(rw.d_sel, 0, sel_bytes, c->stream));   // a hypothesis that is never evaluated: k = n_cand = 0
    size_t lds_bytes = 0;
    const RefArgs a = refine_args(c, w, src_idx != NULL, p->max_correspondence_distance, &lds_bytes);
    const RobustArgs r = robust_args(c, w, rw, p);
    for (int it = 0; it < p->max_iterations; ++it) {
        if (w.nchunks > 0) {
            const int rc = robust_enqueue_iteration(c, w, a, r, lds_bytes, p->keep_ratio, fused, RobustNoDetail());
            if (rc) return rc;
        }
        hipLaunchKernelGGL(refine_solve_kernel<RefNoDetail>, dim3((unsigned)n), dim3(64), 0, c->stream, d_hyp, (const double*)w.d_part, w.nchunks, RefNoDetail());
        STOCS_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(refine_final_kernel, dim3(hblocks), dim3(64), 0, c->stream, (const float*)w.d_Tin, (const RefHyp*)d_hyp, n, c->centroid_scene,
                       c->centroid_model, w.d_Tout, w.d_Pout, w.d_nc, w.d_it);
    STOCS_HIP_CHECK(hipGetLastError());
    { const int rc = launch_lcp(c, w.d_Tout, n, w.d_lcp, NULL, NULL, NULL, 0); if (rc) return rc; }
    STOCS_HIP_CHECK(hipMemcpyAsync(hout, w.d_Tout, out_bytes, hipMemcpyDeviceToHost, c->stream));
    char* hsel = hout + al256(out_bytes);
    if (!fused) STOCS_HIP_CHECK(hipMemcpyAsync(hsel, rw.d_sel, sel_bytes, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    const char* o = hout;
    if (T16_out) memcpy(T16_out, o, (size_t)n * 64);
    if (pose16_out) memcpy(pose16_out, o + (size_t)n * 64, (size_t)n * 64);
    if (lcp_out) memcpy(lcp_out, o + (size_t)n * 128, (size_t)n * 4);
    if (n_corr_out) memcpy(n_corr_out, o + (size_t)n * 132, (size_t)n * 4);
    if (iterations_out) memcpy(iterations_out, o + (size_t)n * 136, (size_t)n * 4);
    if (n_cand_out) {
        if (fused) memcpy(n_cand_out, o + (size_t)n * 132, (size_t)n * 4);   // everything kept: the candidates are the correspondences
        else for (int k = 0; k < n; ++k) n_cand_out[k] = ((const RobustSel*)hsel)[k].ncand;
    }
    return STOCS_OK;
}

extern "C" int stocs_refine_robust_detail(stocs_ctx* c, const float* T16_in, const int32_t* src_idx, int n_src, const stocs_refine_robust_params* p, int32_t* match,
                                          uint8_t* candidate, uint8_t* kept, uint32_t* rank, int32_t* k_out, int32_t* n_cand_out, double* sums28) {
    const char* who = "stocs_refine_robust_detail";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (!T16_in) { set_error("%s: NULL hypothesis", who); return STOCS_ERR_INVALID; }
    { const int rc = robust_check_call(c, who, src_idx, n_src, p); if (rc) return rc; }
    const int nsrc = src_idx ? n_src : c->nS;
    if (nsrc > 0 && (!match || !candidate || !kept || !rank)) { set_error("%s: NULL output", who); return STOCS_ERR_INVALID; }
    if ((uint64_t)nsrc * 8u > (uint64_t)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES) { set_error("%s: %d source points exceed the workspace limit", who, nsrc); return STOCS_ERR_INVALID; }
    DeviceGuard dev_guard(c->device);
    RefineWork w;
    RobustWork rw;
    { const int rc = refine_prepare(c, 1, nsrc, p->max_correspondence_distance, &w); if (rc) return rc; }
    { const int rc = robust_prepare(c, 1, nsrc, &rw); if (rc) return rc; }
    RefineState* S = (RefineState*)c->refine;
    const size_t cells = (size_t)std::max(nsrc, 1);
    Carve cv;
    const size_t o_kept = cv.take(cells), o_sums = cv.take(28 * 8);
    { const int rc = S->detail.grow(c->stream, cv.total); if (rc) return rc; }
    uint8_t* d_kept = Carve::at<uint8_t>(S->detail.p, o_kept);
    double* d_sums = Carve::at<double>(S->detail.p, o_sums);
    // a plain, synchronous path (a test and diagnosis facility): pageable copies, one hypothesis.  Presets: what a hypothesis that
    // is never evaluated (a singular linear part) reports
    STOCS_HIP_CHECK(hipMemcpyAsync(w.d_Tin, T16_in, 64, hipMemcpyHostToDevice, c->stream));
    if (src_idx && nsrc) STOCS_HIP_CHECK(hipMemcpyAsync(w.d_idx, src_idx, (size_t)nsrc * 4, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(rw.d_word, 0xFF, cells * 4, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(rw.d_match, 0xFF, cells * 4, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(rw.d_sel, 0, sizeof(RobustSel), c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(d_kept, 0, cells, c->stream));
    STOCS_HIP_CHECK(hipMemsetAsync(d_sums, 0, 28 * 8, c->stream));
    RefHyp* d_hyp = (RefHyp*)w.d_hyp;
    hipLaunchKernelGGL(refine_init_kernel, dim3(1), dim3(64), 0, c->stream, (const float*)w.d_Tin, 1, (const int32_t*)NULL, d_hyp);
    STOCS_HIP_CHECK(hipGetLastError());
    size_t lds_bytes = 0;
    const RefArgs a = refine_args(c, w, src_idx != NULL, p->max_correspondence_distance, &lds_bytes);
    const RobustArgs r = robust_args(c, w, rw, p);
    RobustDetailOut det;
    det.kept = d_kept;
    if (w.nchunks > 0) {
        const int rc = robust_enqueue_iteration(c, w, a, r, lds_bytes, p->keep_ratio, false, det);   // always match, select, kept
        if (rc) return rc;
    }
    RefDetailOut sd;
    sd.match = NULL; sd.counted = NULL; sd.sums28 = d_sums;
    hipLaunchKernelGGL(refine_solve_kernel<RefDetailOut>, dim3(1), dim3(64), 0, c->stream, d_hyp, (const double*)w.d_part, w.nchunks, sd);
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    RobustSel sel;
    STOCS_HIP_CHECK(hipMemcpy(&sel, rw.d_sel, sizeof(sel), hipMemcpyDeviceToHost));
    if (nsrc) {
        STOCS_HIP_CHECK(hipMemcpy(match, rw.d_match, (size_t)nsrc * 4, hipMemcpyDeviceToHost));
        STOCS_HIP_CHECK(hipMemcpy(rank, rw.d_word, (size_t)nsrc * 4, hipMemcpyDeviceToHost));
        STOCS_HIP_CHECK(hipMemcpy(kept, d_kept, (size_t)nsrc, hipMemcpyDeviceToHost));
        for (int i = 0; i < nsrc; ++i) candidate[i] = rank[i] != 0xFFFFFFFFu ? 1 : 0;   // by definition of the rank word
    }
    if (k_out) *k_out = sel.k;
    if (n_cand_out) *n_cand_out = sel.ncand;
    if (sums28) STOCS_HIP_CHECK(hipMemcpy(sums28, d_sums, 28 * 8, hipMemcpyDeviceToHost));
    return STOCS_OK;
}

extern "C" int stocs_refine_robust_workspace(stocs_ctx* c, void** address, uint64_t* bytes) {
    if (!c) { set_error("stocs_refine_robust_workspace: NULL context"); return STOCS_ERR_INVALID; }
    RefineState* S = (RefineState*)c->refine;
    if (address) *address = S ? (void*)S->robust.p : NULL;
    if (bytes) *bytes = S ? (uint64_t)S->robust.bytes : 0;
    return STOCS_OK;
}
