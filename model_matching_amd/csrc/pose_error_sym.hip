// pose_error_sym.hip -- pose errors under model symmetries (stocs_pose_errors_sym, stocs_pose_errors_sym_detail, stocs_symmetry_set):
// per pair of camera-frame poses and per symmetry k of an explicit set, the largest and the summed distance of every model point under
// the estimate to the SAME point under the ground truth composed with symmetry k, the largest distance of their projections, and the
// minima over k (MSSD, MSPD, symmetric ADD of the BOP benchmark).  No reference counterpart.  The contract (float order, composition,
// fixed-point sums, index-ordered minima) is written down at the declaration in include/stocs_hip.h and restated in float32 numpy in
// tests/pose_error_sym_ref.py; the arithmetic of a point is pose_error_math.h's, shared with pose_error.hip.
//
// n pairs x K symmetries x M points of VALU work with wave-uniform matrices:
//   compose kernel: one thread per (ground truth, k) writes step 0's (C, u) as a 16-float pose into device memory, once per call;
//   main kernel: grid (pairs, symmetry blocks of PS_KB), workgroups of PS_THREADS threads.  A workgroup owns ONE pair and PS_KB
//     symmetries and walks the whole model.  The estimate and the block's composed poses are read through uniform addresses of
//     read-only memory (scalar loads: the matrices sit in scalar registers, a VALU operation takes one as an operand).  A lane takes
//     the points tid, tid + PS_THREADS, ...: it forms p(i), and its projection when asked, ONCE, then loops over the block's symmetries
//     with per-lane accumulators in registers: a 64-bit sum, a maximum of D and (template switch PROJ) a maximum of P per symmetry.
//     PS_KB = 4: the block's 48 matrix entries and the estimate's 12 fit the scalar registers.  At 8 (96 + 12) the compiler parks scalars
//     in vector lanes and reads 45 of them back in every pass of the point loop; timed on 1 024 and 8 192 pairs x 8 and 72 symmetries,
//     4 is 4 - 8 % faster on a 5 000-point model and within 2 % on a 472-point one.
//     The last block of a K that is no multiple of PS_KB runs its spare slots on symmetry K - 1 again and stores nothing for them
//     (no divergence, no out-of-range read);
//   the cross-lane reduction (shuffles, then LDS) runs once per (pair, k) at the end; since one workgroup owns (pair, k) the per-k
//     values are plain stores: no atomics, no memset;
//   the projection costs two correctly rounded divisions per point and symmetry: PROJ = false compiles none of it;
//   min kernel: one wavefront per pair takes step 5: a lane walks k = lane, lane + 64, ... upwards and replaces only on `<`, the
//     lanes are then merged on (value, k) keys, so the lowest k that attains the minimum wins.
//   no FMA anywhere (-ffp-contract=off, and the contract forbids it).
// Per call, everything on the context's stream: poses and symmetries up through the pinned block in one copy, three launches, one copy
// of the n records back, ONE synchronisation.  `add`, `valid` and the invalid pairs' records are filled on the host.
#include <string.h>

#include "eval_call.h"
#include "pose_error_math.h"

namespace stocs {

enum { PS_THREADS = STOCS_POSE_SYM_THREADS, PS_KB = STOCS_POSE_SYM_BLOCK, PS_WAVES = PS_THREADS / 64 };
static_assert(PS_THREADS % 64 == 0 && PS_KB >= 1 && PS_KB <= PS_THREADS, "whole wavefronts; one thread stores one symmetry's values");

struct PoseErrorSymState { static const StateOwner OWNER = OWN_POSE_ERROR_SYM; DevBlock work; ~PoseErrorSymState() { work.free(); } };
struct PsPerK { unsigned long long add_fix; float max3, max2; };   // step 3 / 4 of one (pair, k)
static_assert(sizeof(PsPerK) == 16, "per-k values are 16 bytes");
struct PsCam { float fx, fy, cx, cy; };

// step 0, once per (ground truth, k): (C, u) laid out as a column-major pose, so that step 1 is pe_transform on it.  A kernel of its
// own, not a prologue of every workgroup: with one ground truth for n estimates (the usual call: a trial batch's winners against T_gt)
// the K compositions are done once, not once per pair and block, and the main kernel reads them through uniform addresses as scalars
// without an LDS round trip; the price is a third launch and 64 bytes of workspace per ground truth and symmetry.  Not timed against
// the per-workgroup form.
__global__ __launch_bounds__(PS_THREADS) void pose_sym_compose_kernel(const float* __restrict__ gt, const float* __restrict__ sym, int n_gt, int K,
                                                                     float* __restrict__ comp) {
    const long long t = (long long)blockIdx.x * PS_THREADS + threadIdx.x;
    if (t >= (long long)n_gt * K) return;
    const float* G = gt + (size_t)(t / K) * 16;
    const float* S = sym + (size_t)(t % K) * 16;
    float* C = comp + (size_t)t * 16;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) C[4 * b + a] = G[a] * S[4 * b] + (G[4 + a] * S[4 * b + 1] + G[8 + a] * S[4 * b + 2]);
        C[12 + a] = (G[a] * S[12] + (G[4 + a] * S[13] + G[8 + a] * S[14])) + G[12 + a];
        C[4 * a + 3] = 0.0f;
    }
    C[15] = 1.0f;
}

// a = (fx x_0) / x_2 + cx, b = (fy x_1) / x_2 + cy: project_point's expression before its + 0.5 and floorf
__device__ __forceinline__ float2 ps_project(const PsCam k, const float4 x) { return make_float2((k.fx * x.x) / x.z + k.cx, (k.fy * x.y) / x.z + k.cy); }

// JUDGE (runtime, workgroup-uniform): skip the pairs the host writes as invalid; the detail form judges nothing
template <bool PROJ>
__global__ __launch_bounds__(PS_THREADS) void pose_error_sym_kernel(const float* __restrict__ est, const float* __restrict__ gt, int gt_stride,
                                                                    const float* __restrict__ comp, int comp_pair_stride, int K, PsCam cam,
                                                                    const float4* __restrict__ mpos, int nM, int judge, PsPerK* __restrict__ out) {
    __shared__ unsigned long long red_sum[PS_KB][PS_WAVES];
    __shared__ unsigned red_max3[PS_KB][PS_WAVES];
    __shared__ unsigned red_max2[PS_KB][PS_WAVES];
    const int tid = (int)threadIdx.x;
    const size_t pair = blockIdx.x;
    const int k0 = (int)blockIdx.y * PS_KB;
    float P[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) P[e] = est[pair * 16 + e];   // uniform loads
    if (judge) {
        float G[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) G[e] = gt[pair * (size_t)gt_stride + e];
        if (!pe_pose_finite(P) || !pe_pose_finite(G) || pe_pose_zero(P)) return;   // workgroup-uniform exit
    }
    float C[PS_KB][16];
#pragma unroll
    for (int k = 0; k < PS_KB; ++k) {
        const int kk = min(k0 + k, K - 1);   // spare slots of the last block: symmetry K - 1 again, never stored
        const float* c = comp + pair * (size_t)comp_pair_stride + (size_t)kk * 16;
#pragma unroll
        for (int e = 0; e < 15; ++e)
            if ((e & 3) != 3) C[k][e] = c[e];
    }

    unsigned long long sum[PS_KB];
    float mx3[PS_KB], mx2[PS_KB];
#pragma unroll
    for (int k = 0; k < PS_KB; ++k) { sum[k] = 0; mx3[k] = 0.0f; mx2[k] = 0.0f; }
    for (int i = tid; i < nM; i += PS_THREADS) {
        const float4 m = mpos[i];
        const float4 p = pe_transform(P, m);
        float2 pp = make_float2(0.0f, 0.0f);
        bool p_front = false;
        if (PROJ) { pp = ps_project(cam, p); p_front = p.z > 1e-6f; }
#pragma unroll
        for (int k = 0; k < PS_KB; ++k) {
            const float4 g = pe_transform(C[k], m);
            float D = pe_sqdist(p, g);
            sum[k] += pe_fix(pe_root(D));
            D = D != D ? INFINITY : D;
            mx3[k] = D > mx3[k] ? D : mx3[k];
            if (PROJ) {
                const float2 gp = ps_project(cam, g);
                const float da = pp.x - gp.x, db = pp.y - gp.y;
                float Q = (da * da) + (db * db);
                Q = (!(p_front && g.z > 1e-6f) || Q != Q) ? INFINITY : Q;
                mx2[k] = Q > mx2[k] ? Q : mx2[k];
            }
        }
    }

    // once per (pair, k): wavefront by shuffles, workgroup through LDS.  Non-negative floats or +inf: the bits order as the floats
#pragma unroll
    for (int k = 0; k < PS_KB; ++k) {
        const unsigned long long s = wave_sum_u64(sum[k]);
        const unsigned a = wave_max_u32(__float_as_uint(mx3[k]));
        const unsigned b = PROJ ? wave_max_u32(__float_as_uint(mx2[k])) : 0u;
        if ((tid & 63) == 0) { red_sum[k][tid >> 6] = s; red_max3[k][tid >> 6] = a; red_max2[k][tid >> 6] = b; }
    }
    __syncthreads();
    if (tid < PS_KB && k0 + tid < K) {
        unsigned long long s = red_sum[tid][0];
        unsigned a = red_max3[tid][0], b = red_max2[tid][0];
#pragma unroll
        for (int w = 1; w < PS_WAVES; ++w) {
            s += red_sum[tid][w];
            a = red_max3[tid][w] > a ? red_max3[tid][w] : a;
            b = red_max2[tid][w] > b ? red_max2[tid][w] : b;
        }
        PsPerK r;
        r.add_fix = s;
        r.max3 = stocs_sqrtf(__uint_as_float(a));   // max r(D) = r(max D): the root is monotone and correctly rounded
        r.max2 = PROJ ? stocs_sqrtf(__uint_as_float(b)) : INFINITY;
        out[pair * (size_t)K + (size_t)(k0 + tid)] = r;
    }
}

// the lexicographic minimum of (value, k) over the wavefront
__device__ __forceinline__ void wave_min_key(unsigned long long& v, int& k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        const int j = __shfl_xor(k, o, 64);
        const bool take = w < v || (w == v && (unsigned)j < (unsigned)k);   // -1 (none) orders last
        v = take ? w : v; k = take ? j : k;
    }
}

// step 5: one wavefront per pair.  The host fills add, valid and the invalid pairs' records
__global__ __launch_bounds__(PS_THREADS) void pose_sym_min_kernel(const float* __restrict__ est, const float* __restrict__ gt, int gt_stride, int n, int K,
                                                                 const PsPerK* __restrict__ perk, stocs_pose_error_sym* __restrict__ rec) {
    const size_t pair = (size_t)blockIdx.x * PS_WAVES + (threadIdx.x >> 6);
    const int lane = (int)threadIdx.x & 63;
    if (pair >= (size_t)n) return;   // wave-uniform
    {
        float P[16], G[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) { P[e] = est[pair * 16 + e]; G[e] = gt[pair * (size_t)gt_stride + e]; }
        if (!pe_pose_finite(P) || !pe_pose_finite(G) || pe_pose_zero(P)) return;   // the main kernel stored nothing for this pair
    }
    const unsigned INF_BITS = 0x7f800000u;
    unsigned long long va = ~0ull, v3 = INF_BITS, v2 = INF_BITS;   // the float minima on their bits (non-negative or +inf)
    int ka = -1, k3 = -1, k2 = -1;
    for (int k = lane; k < K; k += 64) {   // upwards, replaced only on `<`: the lowest k of the lane's share
        const PsPerK r = perk[pair * (size_t)K + (size_t)k];
        const unsigned long long b3 = __float_as_uint(r.max3), b2 = __float_as_uint(r.max2);
        if (r.add_fix < va) { va = r.add_fix; ka = k; }
        if (b3 < v3) { v3 = b3; k3 = k; }
        if (b2 < v2) { v2 = b2; k2 = k; }
    }
    wave_min_key(va, ka); wave_min_key(v3, k3); wave_min_key(v2, k2);
    if (lane == 0) {
        stocs_pose_error_sym r;
        r.add_fix = va; r.add = 0.0f; r.mssd = __uint_as_float((unsigned)v3); r.mspd = __uint_as_float((unsigned)v2); r.reserved_f = 0.0f;
        r.k_add = ka; r.k_mssd = k3; r.k_mspd = k2; r.valid = 1;
        rec[pair] = r;
    }
}

// the refusals on the symmetries and the camera, which the two entry points share (K is in range, the pointers are set)
static int check_sym_values(const char* who, const float* sym, int K, const stocs_camera* cam) {
    const int bad = first_nonfinite_pose(sym, K);
    if (bad >= 0) { set_error("%s: symmetry %d has a non-finite entry", who, bad); return STOCS_ERR_INVALID; }
    if (cam && !(host_finite(cam->fx) && host_finite(cam->fy) && host_finite(cam->cx) && host_finite(cam->cy))) {
        set_error("%s: non-finite camera intrinsics", who);
        return STOCS_ERR_INVALID;
    }
    return STOCS_OK;
}

struct PsLayout { Carve cv; size_t o_est, o_gt, o_sym, o_comp, o_perk, o_rec, in_bytes; };
static PsLayout ps_layout(size_t n, size_t n_gt, size_t K) {
    PsLayout L;
    L.o_est = L.cv.take(n * 64); L.o_gt = L.cv.take(n_gt * 64); L.o_sym = L.cv.take(K * 64);
    L.in_bytes = L.cv.total;   // what goes up, contiguous
    L.o_comp = L.cv.take(n_gt * K * 64); L.o_perk = L.cv.take(n * K * sizeof(PsPerK)); L.o_rec = L.cv.take(n * sizeof(stocs_pose_error_sym));
    return L;
}

// compose + main kernel on the context's stream over the staged inputs at the block's base
static int ps_enqueue(stocs_ctx* c, char* base, const PsLayout& L, int n, int n_gt, int K, const stocs_camera* cam, int judge) {
    const float* d_est = Carve::at<const float>(base, L.o_est);
    const float* d_gt = Carve::at<const float>(base, L.o_gt);
    float* d_comp = Carve::at<float>(base, L.o_comp);
    const long long nc = (long long)n_gt * K;
    hipLaunchKernelGGL(pose_sym_compose_kernel, dim3((unsigned)((nc + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0, c->stream, d_gt,
                       Carve::at<const float>(base, L.o_sym), n_gt, K, d_comp);
    STOCS_HIP_CHECK(hipGetLastError());
    const dim3 grid((unsigned)n, (unsigned)((K + PS_KB - 1) / PS_KB));
    const int gt_stride = n_gt == 1 ? 0 : 16, comp_stride = n_gt == 1 ? 0 : K * 16;
    PsCam k = {0.0f, 0.0f, 0.0f, 0.0f};
    if (cam) { k.fx = cam->fx; k.fy = cam->fy; k.cx = cam->cx; k.cy = cam->cy; }
    if (cam) hipLaunchKernelGGL(pose_error_sym_kernel<true>, grid, dim3(PS_THREADS), 0, c->stream, d_est, d_gt, gt_stride, (const float*)d_comp, comp_stride, K, k,
                                (const float4*)c->d_mpos_raw, c->nM, judge, Carve::at<PsPerK>(base, L.o_perk));
    else hipLaunchKernelGGL(pose_error_sym_kernel<false>, grid, dim3(PS_THREADS), 0, c->stream, d_est, d_gt, gt_stride, (const float*)d_comp, comp_stride, K, k,
                            (const float4*)c->d_mpos_raw, c->nM, judge, Carve::at<PsPerK>(base, L.o_perk));
    STOCS_HIP_CHECK(hipGetLastError());
    return STOCS_OK;
}

}  // namespace stocs

using namespace stocs;

extern "C" int stocs_pose_errors_sym(stocs_ctx* c, const float* est, int n, const float* gt, int n_gt, const float* sym, int K, const stocs_camera* cam,
                                     stocs_pose_error_sym* out) {
    const char* who = "stocs_pose_errors_sym";
    { int rc; if (check_batch(who, c, n, &rc)) return rc; }
    if (K < 1 || K > STOCS_POSE_SYM_MAX) { set_error("%s: K = %d symmetries, not 1 .. %d", who, K, (int)STOCS_POSE_SYM_MAX); return STOCS_ERR_INVALID; }
    { const int rc = check_pairs(who, est, n, gt, n_gt, out); if (rc) return rc; }
    if (!sym) { set_error("%s: NULL symmetries", who); return STOCS_ERR_INVALID; }
    { const int rc = check_sym_values(who, sym, K, cam); if (rc) return rc; }
    { const int rc = check_model(who, c); if (rc) return rc; }
    const PsLayout L = ps_layout((size_t)n, (size_t)n_gt, (size_t)K);
    if ((uint64_t)L.cv.total > (uint64_t)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES) {
        set_error("%s: %d pairs x %d symmetries need %llu workspace bytes, the limit is %llu", who, n, K, (unsigned long long)L.cv.total,
                  (unsigned long long)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES);
        return STOCS_ERR_INVALID;
    }
    DeviceGuard dev_guard(c->device);
    PoseErrorSymState* S = ctx_state<PoseErrorSymState>(c);
    TimedCall tc(c, TIMING_POSE_ERRORS_SYM);
    { const int rc = S->work.grow(c->stream, L.cv.total); if (rc) return rc; }
    const size_t rec_bytes = (size_t)n * sizeof(stocs_pose_error_sym);
    char *hin, *hback;
    { const int rc = pinned_for(c, L.in_bytes, rec_bytes, &hin, &hback); if (rc) return rc; }
    tc.start();   // (the first step counts the growing of the two blocks)
    memcpy(hin + L.o_est, est, (size_t)n * 64);
    memcpy(hin + L.o_gt, gt, (size_t)n_gt * 64);
    memcpy(hin + L.o_sym, sym, (size_t)K * 64);
    STOCS_HIP_CHECK(hipMemcpyAsync(S->work.p, hin, L.o_sym + (size_t)K * 64, hipMemcpyHostToDevice, c->stream));   // the three regions in one copy
    { const int rc = tc.device_begin(); if (rc) return rc; }
    { const int rc = ps_enqueue(c, S->work.p, L, n, n_gt, K, cam, 1); if (rc) return rc; }
    stocs_pose_error_sym* d_rec = Carve::at<stocs_pose_error_sym>(S->work.p, L.o_rec);
    hipLaunchKernelGGL(pose_sym_min_kernel, dim3((unsigned)((n + PS_WAVES - 1) / PS_WAVES)), dim3(PS_THREADS), 0, c->stream, Carve::at<const float>(S->work.p, L.o_est),
                       Carve::at<const float>(S->work.p, L.o_gt), n_gt == 1 ? 0 : 16, n, K, Carve::at<const PsPerK>(S->work.p, L.o_perk), d_rec);
    STOCS_HIP_CHECK(hipGetLastError());
    { const int rc = tc.device_end(); if (rc) return rc; }
    STOCS_HIP_CHECK(hipMemcpyAsync(hback, d_rec, rec_bytes, hipMemcpyDeviceToHost, c->stream));
    { const int rc = tc.enqueued_wait(); if (rc) return rc; }
    const stocs_pose_error_sym* h_rec = (const stocs_pose_error_sym*)hback;
    for (int k = 0; k < n; ++k) {
        stocs_pose_error_sym r;
        if (!pair_valid(est, gt, n_gt, k)) {   // step 6 (the kernels stored nothing for this pair)
            r.add_fix = 0;
            r.add = r.mssd = r.mspd = INFINITY;
            r.k_add = r.k_mssd = r.k_mspd = -1;
            r.valid = 0;
        } else {
            r = h_rec[k];
            r.add = fix_mean(r.add_fix, c->nM);
            r.valid = 1;
        }
        r.reserved_f = 0.0f;
        out[k] = r;
    }
    return tc.finish();
}

extern "C" int stocs_pose_errors_sym_detail(stocs_ctx* c, const float* est, const float* gt, const float* sym, int K, const stocs_camera* cam,
                                            uint64_t* add_fix, float* max3, float* max2) {
    const char* who = "stocs_pose_errors_sym_detail";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (K < 1 || K > STOCS_POSE_SYM_MAX) { set_error("%s: K = %d symmetries, not 1 .. %d", who, K, (int)STOCS_POSE_SYM_MAX); return STOCS_ERR_INVALID; }
    if (!est || !gt || !sym) { set_error("%s: NULL pose or symmetries", who); return STOCS_ERR_INVALID; }
    { const int rc = check_sym_values(who, sym, K, cam); if (rc) return rc; }
    { const int rc = check_model(who, c); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    PoseErrorSymState* S = ctx_state<PoseErrorSymState>(c);
    const PsLayout L = ps_layout(1, 1, (size_t)K);
    { const int rc = S->work.grow(c->stream, L.cv.total); if (rc) return rc; }
    const size_t back_bytes = (size_t)K * sizeof(PsPerK);
    char *hin, *hback;
    { const int rc = pinned_for(c, L.in_bytes, back_bytes, &hin, &hback); if (rc) return rc; }
    memcpy(hin + L.o_est, est, 64);
    memcpy(hin + L.o_gt, gt, 64);
    memcpy(hin + L.o_sym, sym, (size_t)K * 64);
    STOCS_HIP_CHECK(hipMemcpyAsync(S->work.p, hin, L.o_sym + (size_t)K * 64, hipMemcpyHostToDevice, c->stream));
    { const int rc = ps_enqueue(c, S->work.p, L, 1, 1, K, cam, 0); if (rc) return rc; }
    STOCS_HIP_CHECK(hipMemcpyAsync(hback, S->work.p + L.o_perk, back_bytes, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    const PsPerK* r = (const PsPerK*)hback;
    for (int k = 0; k < K; ++k) {
        if (add_fix) add_fix[k] = r[k].add_fix;
        if (max3) max3[k] = r[k].max3;
        if (max2) max2[k] = r[k].max2;
    }
    return STOCS_OK;
}

// cos and sin of 360 degrees * num / den: exactly 0 and +-1 at the multiples of 90 degrees
static void turn_cos_sin(int num, int den, double* cs, double* sn) {
    if ((4LL * num) % den == 0) {
        static const double C4[4] = {1.0, 0.0, -1.0, 0.0}, S4[4] = {0.0, 1.0, 0.0, -1.0};
        const int q = (int)((4LL * num / den) % 4);
        *cs = C4[q]; *sn = S4[q];
        return;
    }
    const double a = 6.283185307179586476925286766559 * (double)num / (double)den;
    *cs = cos(a); *sn = sin(a);
}

extern "C" int stocs_symmetry_set(const float sym3[3], int n_continuous, const float* center3, float* out16, int cap, int* K) {
    const char* who = "stocs_symmetry_set";
    if (!K) { set_error("%s: NULL count", who); return STOCS_ERR_INVALID; }
    *K = 0;
    if (!sym3) { set_error("%s: NULL descriptor", who); return STOCS_ERR_INVALID; }
    int cnt[3];
    long long total = 1;
    for (int d = 0; d < 3; ++d) {
        if (sym3[d] == 90.0f) cnt[d] = 4;
        else if (sym3[d] == 180.0f) cnt[d] = 2;
        else if (sym3[d] == 360.0f) {
            if (n_continuous < 1) { set_error("%s: n_continuous = %d steps for a continuous axis", who, n_continuous); return STOCS_ERR_INVALID; }
            cnt[d] = n_continuous;
        } else cnt[d] = 1;
        total *= cnt[d];
        if (total > 0x7fffffffLL) { set_error("%s: more than 2^31 - 1 entries", who); return STOCS_ERR_INVALID; }
    }
    *K = (int)total;
    if (cap < *K || !out16) { set_error("%s: %d entries, room for %d", who, *K, out16 ? cap : 0); return STOCS_ERR_INVALID; }
    double c[3] = {0.0, 0.0, 0.0};
    if (center3) {
        for (int d = 0; d < 3; ++d) {
            if (!host_finite(center3[d])) { set_error("%s: non-finite centre", who); return STOCS_ERR_INVALID; }
            c[d] = (double)center3[d];
        }
    }
    float* o = out16;
    for (int iz = 0; iz < cnt[2]; ++iz) {
        for (int iy = 0; iy < cnt[1]; ++iy) {
            for (int ix = 0; ix < cnt[0]; ++ix, o += 16) {   // the x angle runs fastest
                double ca, sa, cb, sb, cg, sg;
                turn_cos_sin(ix, cnt[0], &ca, &sa); turn_cos_sin(iy, cnt[1], &cb, &sb); turn_cos_sin(iz, cnt[2], &cg, &sg);
                // Rz(gamma) Ry(beta) Rx(alpha)
                const double R[3][3] = {{cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa},
                                        {sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa},
                                        {-sb, cb * sa, cb * ca}};
                for (int a = 0; a < 3; ++a) {
                    for (int b = 0; b < 3; ++b) o[4 * b + a] = (float)(R[a][b] + 0.0);   // (+ 0.0: no -0 entries)
                    o[12 + a] = (float)((c[a] - (R[a][0] * c[0] + R[a][1] * c[1] + R[a][2] * c[2])) + 0.0);   // T(c) R T(-c)
                    o[4 * a + 3] = 0.0f;
                }
                o[15] = 1.0f;
            }
        }
    }
    return STOCS_OK;
}
