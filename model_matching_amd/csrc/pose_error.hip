// pose_error.hip -- pose errors against ground truth (stocs_pose_errors, stocs_pose_errors_detail, stocs_model_diameter): per pair of
// camera-frame poses the ADD error (mean distance of every model point under the estimate to the SAME point under the ground truth) and
// the ADD-S error (... to the NEAREST point under the ground truth), their maxima, and the model's diameter.  No reference counterpart;
// the host method this replaces is a kd-tree query plus float64 products per pose (bench.py).  The contract (float order, minimum rule,
// fixed-point sums) is written down at the declaration in include/stocs_hip.h and restated in float32 numpy in tests/pose_error_ref.py.
//
// An exact tiled all-pairs kernel: a search bounded by a radius cannot answer a far-off pose exactly, so this is brute force by design.
//   grid (query chunks of PE_CHUNK points, pairs), workgroups of PE_THREADS threads;
//   a lane keeps up to PE_Q = 4 query points p(i) in registers, i = chunk * PE_CHUNK + q * PE_THREADS + tid; a chunk that holds fewer
//     than four rows of queries runs the tile loop instantiated for that many (a 472-point model: two rows, not four);
//   the targets g(j) are transformed once per workgroup, PE_TILE at a time, into an LDS array of float4; in the tile loop every lane
//     reads the same address (a broadcast: no bank conflicts), and ONE read of an entry feeds the nine float operations (3 sub, 3 mul,
//     2 add, 1 compare-select) of each of the lane's queries: up to 36 VALU operations per LDS read, so the loop is VALU-bound;
//   no FMA anywhere (-ffp-contract=off, and the contract forbids it);
//   a query belongs to one lane, which walks j upwards and updates only on `<`: the minimum is the lowest j that attains it without
//     any key.  The detail form (template switch) carries that j in a register; the shipping form carries no index;
//   sums: q(e_i), q(s_i) as 64-bit integers, wave by shuffles, workgroup through LDS, then ONE 64-bit atomic add per sum and ONE 32-bit
//     atomic max on the float's bits per maximum (non-negative floats order as their bits) into the pair's record, which the call
//     zeroes on the stream first.  Integers and maxima: the record does not depend on any order.
// The diameter is the same tile loop over the untransformed model with a maximum over j > i, once per context.
// Per call, everything on the context's stream: poses up through the pinned block, one memset, the launch (one per 65 535 pairs), one
// copy back into the pinned block, ONE synchronisation.  The means, `valid` and the invalid pairs' records are filled on the host.
// Known limit: a pair is ceil(M / PE_CHUNK) workgroups, so a call of few pairs on a small model is latency-bound.
#include <string.h>

#include "eval_call.h"
#include "pose_error_math.h"

namespace stocs {

enum { PE_THREADS = STOCS_POSE_ERROR_THREADS, PE_Q = 4, PE_CHUNK = STOCS_POSE_ERROR_CHUNK, PE_TILE = STOCS_POSE_ERROR_TILE, PE_MAX_GRID_Y = 65535 };
static_assert(PE_CHUNK == PE_Q * PE_THREADS, "a chunk is PE_Q rows of PE_THREADS queries");
static_assert(PE_TILE % PE_THREADS == 0, "a tile is filled in whole rounds of the workgroup");

struct PoseErrorState {
    static const StateOwner OWNER = OWN_POSE_ERROR;
    DevBlock work;
    bool have_diameter = false;
    float diameter = 0.0f;
    ~PoseErrorState() { work.free(); }
};

// the tile loop: jn targets of the LDS tile against NQ queries in registers.  DETAIL also keeps the tile-global index of the winner
template <int NQ, bool DETAIL>
__device__ __forceinline__ void pe_tile_loop(const float4* __restrict__ tile, int jn, int jbase, const float4* p, float* best, int* arg) {
#pragma unroll 4
    for (int j = 0; j < jn; ++j) {
        const float4 g = tile[j];   // the same address in every lane: one broadcast read (the compiler drops the unused w: ds_read_b96)
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float d = pe_sqdist(p[q], g);
            const bool less = d < best[q];   // false for NaN: a NaN never wins
            best[q] = less ? d : best[q];
            if (DETAIL) arg[q] = less ? jbase + j : arg[q];
        }
    }
}

template <bool DETAIL>
__global__ __launch_bounds__(PE_THREADS) void pose_error_kernel(const float* __restrict__ est, const float* __restrict__ gt, int gt_stride, int pair0,
                                                                const float4* __restrict__ mpos, int nM, stocs_pose_error* __restrict__ rec,
                                                                float* __restrict__ out_e, float* __restrict__ out_s, int32_t* __restrict__ out_nn) {
    __shared__ float4 tile[PE_TILE];
    __shared__ unsigned long long red_sum[2][PE_THREADS / 64];
    __shared__ unsigned red_max[2][PE_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const int pair = pair0 + (int)blockIdx.y;
    const int i0 = (int)blockIdx.x * PE_CHUNK;
    float P[16], G[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { P[k] = est[(size_t)pair * 16 + k]; G[k] = gt[(size_t)pair * (size_t)gt_stride + k]; }   // uniform loads
    // step 5: the host writes the invalid pair's record (workgroup-uniform exit; the detail form judges nothing)
    if (!DETAIL && (!pe_pose_finite(P) || !pe_pose_finite(G) || pe_pose_zero(P))) return;

    float4 p[PE_Q];
    float e[PE_Q], best[PE_Q];
    int arg[PE_Q];
#pragma unroll
    for (int q = 0; q < PE_Q; ++q) {
        const int i = i0 + q * PE_THREADS + tid;
        const float4 m = i < nM ? mpos[i] : make_float4(NAN, NAN, NAN, 0.0f);
        p[q] = pe_transform(P, m);
        e[q] = pe_root(pe_sqdist(p[q], pe_transform(G, m)));   // e_i: the expression of D(i, j) at j = i
        best[q] = INFINITY; arg[q] = -1;
    }
    const int rows = (min(nM - i0, (int)PE_CHUNK) + PE_THREADS - 1) / PE_THREADS;   // rows of queries this chunk holds, 1 .. PE_Q
    for (int jbase = 0; jbase < nM; jbase += PE_TILE) {
        const int jn = min(nM - jbase, (int)PE_TILE);
        __syncthreads();   // the previous tile is read
        for (int k = tid; k < jn; k += PE_THREADS) tile[k] = pe_transform(G, mpos[jbase + k]);
        __syncthreads();
        if (rows == 1) pe_tile_loop<1, DETAIL>(tile, jn, jbase, p, best, arg);
        else if (rows == 2) pe_tile_loop<2, DETAIL>(tile, jn, jbase, p, best, arg);
        else if (rows == 3) pe_tile_loop<3, DETAIL>(tile, jn, jbase, p, best, arg);
        else pe_tile_loop<4, DETAIL>(tile, jn, jbase, p, best, arg);
    }

    unsigned long long sum_e = 0, sum_s = 0;
    unsigned max_e = 0, max_s = 0;
#pragma unroll
    for (int q = 0; q < PE_Q; ++q) {
        const int i = i0 + q * PE_THREADS + tid;
        if (i < nM) {
            const float s = pe_root(best[q]);
            if (DETAIL) {
                if (out_e) out_e[i] = e[q];
                if (out_s) out_s[i] = s;
                if (out_nn) out_nn[i] = arg[q];
            }
            sum_e += pe_fix(e[q]); sum_s += pe_fix(s);
            const unsigned be = __float_as_uint(e[q]), bs = __float_as_uint(s);   // non-negative or +inf: the bits order as the floats
            max_e = be > max_e ? be : max_e; max_s = bs > max_s ? bs : max_s;
        }
    }
    if (DETAIL) return;
    sum_e = wave_sum_u64(sum_e); sum_s = wave_sum_u64(sum_s); max_e = wave_max_u32(max_e); max_s = wave_max_u32(max_s);
    if ((tid & 63) == 0) { red_sum[0][tid >> 6] = sum_e; red_sum[1][tid >> 6] = sum_s; red_max[0][tid >> 6] = max_e; red_max[1][tid >> 6] = max_s; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < PE_THREADS / 64; ++w) {
            sum_e += red_sum[0][w]; sum_s += red_sum[1][w];
            max_e = red_max[0][w] > max_e ? red_max[0][w] : max_e; max_s = red_max[1][w] > max_s ? red_max[1][w] : max_s;
        }
        stocs_pose_error* r = rec + pair;
        atomicAdd((unsigned long long*)&r->add_fix, sum_e);
        atomicAdd((unsigned long long*)&r->adds_fix, sum_s);
        atomicMax((unsigned*)&r->add_max, max_e);
        atomicMax((unsigned*)&r->adds_max, max_s);
    }
}

// step 6: max over j > i of D(i, j) on the untransformed model, NaN counted as +inf; the root is taken on the host side of the word
__global__ __launch_bounds__(PE_THREADS) void model_diameter_kernel(const float4* __restrict__ mpos, int nM, unsigned* __restrict__ out_bits) {
    __shared__ float4 tile[PE_TILE];
    __shared__ unsigned red_max[PE_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const int i0 = (int)blockIdx.x * PE_CHUNK;
    float4 p[PE_Q];
    float best[PE_Q];
#pragma unroll
    for (int q = 0; q < PE_Q; ++q) {
        const int i = i0 + q * PE_THREADS + tid;
        p[q] = i < nM ? mpos[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        best[q] = 0.0f;
    }
    for (int jbase = 0; jbase < nM; jbase += PE_TILE) {
        const int jn = min(nM - jbase, (int)PE_TILE);
        if (jbase + jn - 1 <= i0) continue;   // no j of this tile is above any i of this chunk (workgroup-uniform)
        __syncthreads();
        for (int k = tid; k < jn; k += PE_THREADS) tile[k] = mpos[jbase + k];
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < jn; ++j) {
            const float4 g = tile[j];
#pragma unroll
            for (int q = 0; q < PE_Q; ++q) {
                const int i = i0 + q * PE_THREADS + tid;
                float d = pe_sqdist(p[q], g);
                d = d != d ? INFINITY : d;
                const bool take = (jbase + j > i) && (i < nM) && (d > best[q]);
                best[q] = take ? d : best[q];
            }
        }
    }
    unsigned m = 0;
#pragma unroll
    for (int q = 0; q < PE_Q; ++q) { const unsigned b = __float_as_uint(best[q]); m = b > m ? b : m; }
    m = wave_max_u32(m);
    if ((tid & 63) == 0) red_max[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < PE_THREADS / 64; ++w) m = red_max[w] > m ? red_max[w] : m;
        atomicMax(out_bits, m);
    }
}

}  // namespace stocs

using namespace stocs;

extern "C" int stocs_pose_errors(stocs_ctx* c, const float* est, int n, const float* gt, int n_gt, stocs_pose_error* out) {
    static const char* who = "stocs_pose_errors";
    { int rc; if (check_batch(who, c, n, &rc)) return rc; }
    { const int rc = check_pairs(who, est, n, gt, n_gt, out); if (rc) return rc; }
    { const int rc = check_model(who, c); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    PoseErrorState* S = ctx_state<PoseErrorState>(c);
    TimedCall tc(c, TIMING_POSE_ERRORS);
    Carve cv;
    const size_t o_est = cv.take((size_t)n * 64), o_gt = cv.take((size_t)n_gt * 64), o_rec = cv.take((size_t)n * sizeof(stocs_pose_error));
    { const int rc = S->work.grow(c->stream, cv.total); if (rc) return rc; }
    char* hp;   // the pinned mirror of the three regions, at the same offsets
    { const int rc = pinned_var(c, cv.total, &hp); if (rc) return rc; }
    float* d_est = Carve::at<float>(S->work.p, o_est);
    float* d_gt = Carve::at<float>(S->work.p, o_gt);
    stocs_pose_error* d_rec = Carve::at<stocs_pose_error>(S->work.p, o_rec);
    stocs_pose_error* h_rec = Carve::at<stocs_pose_error>(hp, o_rec);
    tc.start();   // (the first step counts the growing of the two blocks)
    memcpy(hp + o_est, est, (size_t)n * 64);
    memcpy(hp + o_gt, gt, (size_t)n_gt * 64);
    STOCS_HIP_CHECK(hipMemcpyAsync(S->work.p, hp, o_gt + (size_t)n_gt * 64, hipMemcpyHostToDevice, c->stream));   // both pose regions in one copy
    STOCS_HIP_CHECK(hipMemsetAsync(d_rec, 0, (size_t)n * sizeof(stocs_pose_error), c->stream));
    const unsigned chunks = (unsigned)((c->nM + PE_CHUNK - 1) / PE_CHUNK);
    { const int rc = tc.device_begin(); if (rc) return rc; }
    for (int p0 = 0; p0 < n; p0 += PE_MAX_GRID_Y) {
        const int np = n - p0 < PE_MAX_GRID_Y ? n - p0 : PE_MAX_GRID_Y;
        hipLaunchKernelGGL(pose_error_kernel<false>, dim3(chunks, (unsigned)np), dim3(PE_THREADS), 0, c->stream, (const float*)d_est, (const float*)d_gt,
                           n_gt == 1 ? 0 : 16, p0, (const float4*)c->d_mpos_raw, c->nM, d_rec, (float*)NULL, (float*)NULL, (int32_t*)NULL);
        STOCS_HIP_CHECK(hipGetLastError());
    }
    { const int rc = tc.device_end(); if (rc) return rc; }
    STOCS_HIP_CHECK(hipMemcpyAsync(h_rec, d_rec, (size_t)n * sizeof(stocs_pose_error), hipMemcpyDeviceToHost, c->stream));
    { const int rc = tc.enqueued_wait(); if (rc) return rc; }
    for (int k = 0; k < n; ++k) {
        stocs_pose_error r = h_rec[k];
        if (!pair_valid(est, gt, n_gt, k)) {   // step 5 (the kernel left the record zero)
            r.add_fix = r.adds_fix = 0;
            r.add = r.add_max = r.adds = r.adds_max = INFINITY;
            r.valid = 0;
        } else {
            r.add = fix_mean(r.add_fix, c->nM);
            r.adds = fix_mean(r.adds_fix, c->nM);
            r.valid = 1;
        }
        r.reserved = 0;
        out[k] = r;
    }
    return tc.finish();
}

extern "C" int stocs_pose_errors_detail(stocs_ctx* c, const float* est, const float* gt, float* e, float* s, int32_t* nn) {
    if (!c || !est || !gt) { set_error("stocs_pose_errors_detail: NULL context or pose"); return STOCS_ERR_INVALID; }
    { const int rc = check_model("stocs_pose_errors_detail", c); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    PoseErrorState* S = ctx_state<PoseErrorState>(c);
    const size_t M = (size_t)c->nM;
    Carve cv;
    const size_t o_est = cv.take(64), o_gt = cv.take(64), o_e = cv.take(M * 4), o_s = cv.take(M * 4), o_nn = cv.take(M * 4);
    { const int rc = S->work.grow(c->stream, cv.total); if (rc) return rc; }
    char* hp;
    { const int rc = pinned_var(c, cv.total, &hp); if (rc) return rc; }
    memcpy(hp + o_est, est, 64);
    memcpy(hp + o_gt, gt, 64);
    STOCS_HIP_CHECK(hipMemcpyAsync(S->work.p, hp, o_gt + 64, hipMemcpyHostToDevice, c->stream));
    const unsigned chunks = (unsigned)((c->nM + PE_CHUNK - 1) / PE_CHUNK);
    hipLaunchKernelGGL(pose_error_kernel<true>, dim3(chunks, 1u), dim3(PE_THREADS), 0, c->stream, Carve::at<const float>(S->work.p, o_est),
                       Carve::at<const float>(S->work.p, o_gt), 0, 0, (const float4*)c->d_mpos_raw, c->nM, (stocs_pose_error*)NULL,
                       Carve::at<float>(S->work.p, o_e), Carve::at<float>(S->work.p, o_s), Carve::at<int32_t>(S->work.p, o_nn));
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(hipMemcpyAsync(hp + o_e, S->work.p + o_e, cv.total - o_e, hipMemcpyDeviceToHost, c->stream));   // the three outputs in one copy
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (e) memcpy(e, hp + o_e, M * 4);
    if (s) memcpy(s, hp + o_s, M * 4);
    if (nn) memcpy(nn, hp + o_nn, M * 4);
    return STOCS_OK;
}

extern "C" int stocs_model_diameter(stocs_ctx* c, float* diameter) {
    if (!c || !diameter) { set_error("stocs_model_diameter: NULL context or result"); return STOCS_ERR_INVALID; }
    { const int rc = check_model("stocs_model_diameter", c); if (rc) return rc; }
    PoseErrorState* S = ctx_state<PoseErrorState>(c);
    if (!S->have_diameter) {
        DeviceGuard dev_guard(c->device);
        { const int rc = S->work.grow(c->stream, 256); if (rc) return rc; }
        char* hp;
        { const int rc = pinned_var(c, 256, &hp); if (rc) return rc; }
        unsigned* d_bits = (unsigned*)S->work.p;
        STOCS_HIP_CHECK(hipMemsetAsync(d_bits, 0, 4, c->stream));
        hipLaunchKernelGGL(model_diameter_kernel, dim3((unsigned)((c->nM + PE_CHUNK - 1) / PE_CHUNK)), dim3(PE_THREADS), 0, c->stream,
                           (const float4*)c->d_mpos_raw, c->nM, d_bits);
        STOCS_HIP_CHECK(hipGetLastError());
        STOCS_HIP_CHECK(hipMemcpyAsync(hp, d_bits, 4, hipMemcpyDeviceToHost, c->stream));
        STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
        float d2;
        memcpy(&d2, hp, 4);
        S->diameter = stocs_sqrtf(d2);   // the root is monotone and correctly rounded: max r(D) = r(max D)
        S->have_diameter = true;
    }
    *diameter = S->diameter;
    return STOCS_OK;
}
