// symmetry.hip -- finding a model's symmetries (stocs_symmetry_errors, stocs_symmetry_errors_detail, stocs_symmetry_axes,
// stocs_symmetry_rotation, stocs_symmetry_close, stocs_find_symmetries): the self-distance of the model under K transforms of its own
// frame -- per transform the summed, clamped and the largest distance of every transformed point to the NEAREST untransformed point
// within a reach, the count of points with none, and the count of matched points whose normals disagree -- and the search for axes on
// top of it.  No reference counterpart.  The contract is written down at the declarations in include/stocs_hip.h and restated in
// float32 numpy in tests/symmetry_ref.py; the arithmetic of a point is pose_error_math.h's, so a matched point's distance and
// neighbour equal stocs_pose_errors_detail(S, I)'s bit for bit.
//
// The brute-force kernel (pose_error.hip) would answer one transform in M^2 pairs; a search asks tens of thousands of transforms and
// the target is always the same untransformed model, so the target is binned once per (context, reach) into a uniform grid (symmetry.h:
// the cell expression and why 27 cells suffice) and a query looks at the cells about its own:
//   grid x = transforms, workgroups of SY_THREADS threads.  A workgroup owns ONE transform, read through uniform addresses of read-only
//     memory (scalar loads: the matrix sits in scalar registers).  A lane takes the points tid, tid + SY_THREADS, ...: it forms p(i),
//     its cell, and walks nine runs of the sorted target list (the three cells of a row along x are neighbours in the list, so a row is
//     ONE run between two cell starts) keeping the minimum of (bits(D), j) keys: cells come in no index order, the key makes the lowest
//     j win a tie.  D >= +0 or NaN, whose bits order above +inf: a NaN never wins, as in the brute-force kernel;
//   the two normals of a matched pair are read once per query by index (the model's unit normals of the context), not carried through
//     the grid: 32 bytes per query against 16 more per visited target;
//   per-lane accumulators (a 64-bit sum, the maximum of D on its bits, the two counts packed into one 64-bit word) are reduced once at
//     the end, wave by shuffles, workgroup through LDS, and stored plainly: no atomics, no memset;
//   the grid stays in global memory (about 100 KB for a 5 000-point model, read by every workgroup: L2-resident); no LDS form is built;
//   no FMA anywhere (-ffp-contract=off, and the contract forbids it).
// Per call, everything on the context's stream: transforms up through the pinned block in one copy, one launch per SY_MAX_LAUNCH
// transforms, one copy of the K records back, ONE synchronisation; the first call at a reach also builds and uploads the grid (and
// waits for that copy).  `mean`, `valid` are filled on the host.  The helpers and the search below the entry points are host code.
#include <string.h>

#include "eval_call.h"
#include "pose_error_math.h"
#include "symmetry.h"

namespace stocs {

enum { SY_THREADS = STOCS_SYMMETRY_THREADS, SY_WAVES = SY_THREADS / 64, SY_MAX_LAUNCH = STOCS_SYMMETRY_MAX_LAUNCH, SY_SPAN = STOCS_SYMMETRY_GRID_SPAN,
       SY_MAX_CELLS_AXIS = SY_SPAN + 2 };
static_assert(SY_THREADS % 64 == 0, "whole wavefronts");

struct SymmetryState {
    static const StateOwner OWNER = OWN_SYMMETRY;
    DevBlock grid, work;
    ~SymmetryState() { grid.free(); work.free(); }
    bool have_grid = false;
    float reach = 0.0f;
    SymGrid g;
    size_t o_sorted = 0;   // offset of the sorted targets behind the cell starts
    int n_sorted = 0;
};

template <bool DETAIL>
__global__ __launch_bounds__(SY_THREADS) void symmetry_kernel(const float* __restrict__ sym, SymGrid g, const unsigned* __restrict__ cell_start,
                                                              const float4* __restrict__ sorted, const float4* __restrict__ mpos,
                                                              const float4* __restrict__ mnrm, int nM, float reach, float reach2, float cos_normal,
                                                              stocs_symmetry_error* __restrict__ out, float* __restrict__ out_s,
                                                              int32_t* __restrict__ out_nn, float* __restrict__ out_dot) {
    __shared__ unsigned long long red_sum[SY_WAVES], red_cnt[SY_WAVES];
    __shared__ unsigned red_max[SY_WAVES];
    const int tid = (int)threadIdx.x;
    const float* Sg = sym + (size_t)blockIdx.x * 16;
    float S[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) S[e] = Sg[e];   // uniform loads

    unsigned long long sum = 0, cnt = 0;   // cnt: n_far above bit 32, n_normal_bad below
    unsigned mx = 0;
    for (int i = tid; i < nM; i += SY_THREADS) {
        const float4 p = pe_transform(S, mpos[i]);
        const int cx = sym_cell(p.x, g.ox, g.inv), cy = sym_cell(p.y, g.oy, g.inv), cz = sym_cell(p.z, g.oz, g.inv);
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
        unsigned long long key = (0x7f800000ull << 32) | 0xffffffffull;   // (+inf, none)
        if (x0 <= x1) {
            for (int z = max(cz - 1, 0); z <= min(cz + 1, g.nz - 1); ++z) {
                for (int y = max(cy - 1, 0); y <= min(cy + 1, g.ny - 1); ++y) {
                    const int row = (z * g.ny + y) * g.nx;
                    const unsigned a = cell_start[row + x0], b = cell_start[row + x1 + 1];
                    for (unsigned t = a; t < b; ++t) {
                        const float4 q = sorted[t];
                        const float D = pe_sqdist(p, q);
                        const unsigned long long k = ((unsigned long long)__float_as_uint(D) << 32) | __float_as_uint(q.w);
                        key = k < key ? k : key;
                    }
                }
            }
        }
        const float Dmin = __uint_as_float((unsigned)(key >> 32));
        const int j = (int)(unsigned)key;
        const bool matched = Dmin <= reach2 && Dmin < INFINITY;   // (a reach whose square overflows matches no point that met no target)
        const float s = pe_root(Dmin);
        sum += pe_fix(matched ? s : reach);
        float dot = 0.0f;
        if (matched) {
            const float4 n = mnrm[i], t = mnrm[j];
            const float nx = S[0] * n.x + (S[4] * n.y + S[8] * n.z);
            const float ny = S[1] * n.x + (S[5] * n.y + S[9] * n.z);
            const float nz = S[2] * n.x + (S[6] * n.y + S[10] * n.z);
            dot = nx * t.x + (ny * t.y + nz * t.z);
            const unsigned db = __float_as_uint(Dmin);
            mx = db > mx ? db : mx;
            cnt += !(dot >= cos_normal) ? 1ull : 0ull;
        } else {
            cnt += 1ull << 32;
        }
        if (DETAIL) {
            if (out_s) out_s[i] = matched ? s : INFINITY;
            if (out_nn) out_nn[i] = matched ? j : -1;
            if (out_dot) out_dot[i] = dot;
        }
    }
    if (DETAIL) return;

    sum = wave_sum_u64(sum); cnt = wave_sum_u64(cnt); mx = wave_max_u32(mx);
    if ((tid & 63) == 0) { red_sum[tid >> 6] = sum; red_cnt[tid >> 6] = cnt; red_max[tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < SY_WAVES; ++w) { sum += red_sum[w]; cnt += red_cnt[w]; mx = red_max[w] > mx ? red_max[w] : mx; }
        stocs_symmetry_error r;
        r.sum_fix = sum;
        r.mean = 0.0f;                                   // the host's
        r.max = stocs_sqrtf(__uint_as_float(mx));        // max r(D) = r(max D): the root is monotone and correctly rounded
        r.n_far = (int32_t)(cnt >> 32); r.n_normal_bad = (int32_t)(unsigned)cnt;
        r.valid = 1; r.reserved = 0;
        out[blockIdx.x] = r;
    }
}

static bool sy_finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }

// the grid of the context's model for `reach`: binned on the host with symmetry.h's expression, uploaded, kept until another reach
static int ensure_sym_grid(stocs_ctx* c, SymmetryState* S, float reach) {
    if (S->have_grid && S->reach == reach) return STOCS_OK;
    S->have_grid = false;
    const int M = c->nM;
    const std::vector<V3>& P = c->h_mpos_raw;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    std::vector<int> live;   // a non-finite target is within reach of nothing: it stays out of the grid
    live.reserve((size_t)M);
    for (int i = 0; i < M; ++i) {
        const float v[3] = {P[i].x, P[i].y, P[i].z};
        if (!(host_finite(v[0]) && host_finite(v[1]) && host_finite(v[2]))) continue;
        live.push_back(i);
        for (int a = 0; a < 3; ++a) { mn[a] = v[a] < mn[a] ? v[a] : mn[a]; mx[a] = v[a] > mx[a] ? v[a] : mx[a]; }
    }
    SymGrid g;
    g.nx = g.ny = g.nz = 1;
    g.ox = g.oy = g.oz = 0.0f; g.inv = 1.0f;
    std::vector<int> cell(live.size());
    if (!live.empty()) {
        double ext = 0.0;
        for (int a = 0; a < 3; ++a) ext = std::max(ext, (double)mx[a] - (double)mn[a]);
        float h = (float)std::max((double)reach * 65.0 / 64.0, ext / (double)SY_SPAN);
        h = h > 1e-30f ? h : 1e-30f;   // a larger edge is always safe; 1 / h stays finite
        g.ox = mn[0]; g.oy = mn[1]; g.oz = mn[2]; g.inv = 1.0f / h;
        g.nx = sym_cell(mx[0], g.ox, g.inv) + 1; g.ny = sym_cell(mx[1], g.oy, g.inv) + 1; g.nz = sym_cell(mx[2], g.oz, g.inv) + 1;
        if (g.nx < 1 || g.ny < 1 || g.nz < 1 || g.nx > SY_MAX_CELLS_AXIS || g.ny > SY_MAX_CELLS_AXIS || g.nz > SY_MAX_CELLS_AXIS) {
            set_error("stocs_symmetry_errors: grid of %d x %d x %d cells", g.nx, g.ny, g.nz);
            return STOCS_ERR_STATE;
        }
    }
    const size_t ncell = (size_t)g.nx * g.ny * g.nz;
    std::vector<unsigned> start(ncell + 1, 0u);
    for (size_t k = 0; k < live.size(); ++k) {
        const V3 v = P[live[k]];
        const int x = sym_cell(v.x, g.ox, g.inv), y = sym_cell(v.y, g.oy, g.inv), z = sym_cell(v.z, g.oz, g.inv);   // 0 .. n - 1: monotone, the box ends bin there
        cell[k] = (z * g.ny + y) * g.nx + x;
        ++start[(size_t)cell[k] + 1];
    }
    for (size_t k = 0; k < ncell; ++k) start[k + 1] += start[k];
    std::vector<float4> sorted(std::max<size_t>(live.size(), 1), make_float4(NAN, NAN, NAN, 0.0f));
    {
        std::vector<unsigned> at(start.begin(), start.end() - 1);
        for (size_t k = 0; k < live.size(); ++k) {   // index order inside a cell
            const V3 v = P[live[k]];
            float w;
            const unsigned j = (unsigned)live[k];
            memcpy(&w, &j, 4);
            sorted[at[cell[k]]++] = make_float4(v.x, v.y, v.z, w);
        }
    }
    Carve cv;
    const size_t o_start = cv.take((ncell + 1) * 4), o_sorted = cv.take(sorted.size() * sizeof(float4));
    { const int rc = S->grid.grow(c->stream, cv.total); if (rc) return rc; }
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));   // nothing may still read the old grid
    STOCS_HIP_CHECK(hipMemcpyAsync(S->grid.p + o_start, start.data(), (ncell + 1) * 4, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipMemcpyAsync(S->grid.p + o_sorted, sorted.data(), sorted.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));   // the two vectors leave scope
    S->g = g; S->o_sorted = o_sorted; S->n_sorted = (int)live.size(); S->reach = reach; S->have_grid = true;
    return STOCS_OK;
}

static int check_sym_args(const char* who, const float* sym, int K, const stocs_symmetry_params* p) {
    const int bad = first_nonfinite_pose(sym, K);
    if (bad >= 0) { set_error("%s: transform %d has a non-finite entry", who, bad); return STOCS_ERR_INVALID; }
    if (!(p->reach > 0.0f) || !host_finite(p->reach)) { set_error("%s: reach %g is not a positive finite length", who, (double)p->reach); return STOCS_ERR_INVALID; }
    if (!(p->reach * p->reach >= 1.17549435e-38f)) {   // a square that underflows would match pairs many cells apart (symmetry.h)
        set_error("%s: the square of reach %g is not a normal float", who, (double)p->reach);
        return STOCS_ERR_INVALID;
    }
    return STOCS_OK;
}

// ---- host helpers in double ----
struct M4d { double e[16]; };   // column-major
static M4d m4_identity() { M4d r; for (int i = 0; i < 16; ++i) r.e[i] = (i % 5 == 0) ? 1.0 : 0.0; return r; }
static M4d m4_mul(const M4d& A, const M4d& B) {   // A B, both rigid
    M4d r = m4_identity();
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) r.e[4 * b + a] = A.e[a] * B.e[4 * b] + A.e[4 + a] * B.e[4 * b + 1] + A.e[8 + a] * B.e[4 * b + 2];
        r.e[12 + a] = A.e[a] * B.e[12] + A.e[4 + a] * B.e[13] + A.e[8 + a] * B.e[14] + A.e[12 + a];
    }
    return r;
}
static void m4_round(const M4d& A, float* o) {
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) o[4 * b + a] = (float)(A.e[4 * b + a] + 0.0);   // (+ 0.0: no -0 entries)
        o[12 + a] = (float)(A.e[12 + a] + 0.0);
        o[4 * a + 3] = 0.0f;
    }
    o[15] = 1.0f;
}
static bool normalise3d(double* v) {
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(n > 0.0) || !sy_finite_d(n)) return false;
    v[0] /= n; v[1] /= n; v[2] /= n;
    return true;
}
static const double SY_PI = 3.14159265358979323846264338327950288;

// T(c) R T(-c), R = cs I + sn [a]x + (1 - cs) a a^T; a is a unit vector
static M4d rotation_about(const double a[3], double angle_deg, const double c[3]) {
    double cs, sn;
    const double q = angle_deg / 90.0;
    if (q == floor(q) && fabs(q) < 1e15) {
        static const double C4[4] = {1.0, 0.0, -1.0, 0.0}, S4[4] = {0.0, 1.0, 0.0, -1.0};
        const int k = (int)(((long long)q % 4 + 4) % 4);
        cs = C4[k]; sn = S4[k];
    } else {
        const double r = angle_deg * SY_PI / 180.0;
        cs = cos(r); sn = sin(r);
    }
    const double X[3][3] = {{0.0, -a[2], a[1]}, {a[2], 0.0, -a[0]}, {-a[1], a[0], 0.0}};
    M4d r = m4_identity();
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.e[4 * j + i] = (i == j ? cs : 0.0) + sn * X[i][j] + (1.0 - cs) * a[i] * a[j];
    for (int i = 0; i < 3; ++i) r.e[12 + i] = c[i] - (r.e[i] * c[0] + r.e[4 + i] * c[1] + r.e[8 + i] * c[2]);
    return r;
}

static int rotation16(const float axis3[3], double angle_deg, const float* center3, float out16[16]) {
    double a[3] = {(double)axis3[0], (double)axis3[1], (double)axis3[2]}, c[3] = {0.0, 0.0, 0.0};
    if (center3) for (int d = 0; d < 3; ++d) c[d] = (double)center3[d];
    if (!normalise3d(a) || !sy_finite_d(angle_deg) || !(sy_finite_d(c[0]) && sy_finite_d(c[1]) && sy_finite_d(c[2]))) return STOCS_ERR_INVALID;
    m4_round(rotation_about(a, angle_deg, c), out16);
    return STOCS_OK;
}

// |a . b| of two float directions, in double
static double axis_cos(const float* a, const float* b) {
    return fabs((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1] + (double)a[2] * (double)b[2]);
}

}  // namespace stocs

using namespace stocs;

extern "C" int stocs_symmetry_errors(stocs_ctx* c, const float* sym, int K, const stocs_symmetry_params* p, stocs_symmetry_error* out) {
    const char* who = "stocs_symmetry_errors";
    if (!c) { set_error("%s: NULL context", who); return STOCS_ERR_INVALID; }
    if (K < 0) { set_error("%s: K %d < 0", who, K); return STOCS_ERR_INVALID; }
    if (K == 0) return STOCS_OK;
    if (!sym || !p || !out) { set_error("%s: NULL transforms, parameters or results", who); return STOCS_ERR_INVALID; }
    { const int rc = check_sym_args(who, sym, K, p); if (rc) return rc; }
    Carve cv;
    const size_t o_sym = cv.take((size_t)K * 64), o_rec = cv.take((size_t)K * sizeof(stocs_symmetry_error));
    if ((uint64_t)cv.total > (uint64_t)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES) {
        set_error("%s: %d transforms need %llu workspace bytes, the limit is %llu", who, K, (unsigned long long)cv.total,
                  (unsigned long long)STOCS_REFINE_ROBUST_MAX_WORKSPACE_BYTES);
        return STOCS_ERR_INVALID;
    }
    { const int rc = check_model(who, c); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    SymmetryState* S = ctx_state<SymmetryState>(c);
    TimedCall tc(c, TIMING_SYMMETRY);
    { const int rc = ensure_sym_grid(c, S, p->reach); if (rc) return rc; }
    { const int rc = S->work.grow(c->stream, cv.total); if (rc) return rc; }
    const size_t rec_bytes = (size_t)K * sizeof(stocs_symmetry_error);
    char *hin, *hback;
    { const int rc = pinned_for(c, (size_t)K * 64, rec_bytes, &hin, &hback); if (rc) return rc; }
    tc.start();   // (the first step counts the grid of a new reach and the growing of the blocks)
    memcpy(hin, sym, (size_t)K * 64);
    STOCS_HIP_CHECK(hipMemcpyAsync(S->work.p + o_sym, hin, (size_t)K * 64, hipMemcpyHostToDevice, c->stream));
    { const int rc = tc.device_begin(); if (rc) return rc; }
    stocs_symmetry_error* d_rec = Carve::at<stocs_symmetry_error>(S->work.p, o_rec);
    const float reach2 = p->reach * p->reach;
    for (int k0 = 0; k0 < K; k0 += SY_MAX_LAUNCH) {
        const int nk = K - k0 < SY_MAX_LAUNCH ? K - k0 : SY_MAX_LAUNCH;
        hipLaunchKernelGGL(symmetry_kernel<false>, dim3((unsigned)nk), dim3(SY_THREADS), 0, c->stream, Carve::at<const float>(S->work.p, o_sym) + (size_t)k0 * 16, S->g,
                           Carve::at<const unsigned>(S->grid.p, 0), Carve::at<const float4>(S->grid.p, S->o_sorted), (const float4*)c->d_mpos_raw,
                           (const float4*)c->d_mnrm, c->nM, p->reach, reach2, p->cos_normal, d_rec + k0, (float*)NULL, (int32_t*)NULL, (float*)NULL);
        STOCS_HIP_CHECK(hipGetLastError());
    }
    { const int rc = tc.device_end(); if (rc) return rc; }
    STOCS_HIP_CHECK(hipMemcpyAsync(hback, d_rec, rec_bytes, hipMemcpyDeviceToHost, c->stream));
    { const int rc = tc.enqueued_wait(); if (rc) return rc; }
    const stocs_symmetry_error* h_rec = (const stocs_symmetry_error*)hback;
    for (int k = 0; k < K; ++k) {
        stocs_symmetry_error r = h_rec[k];
        r.mean = fix_mean(r.sum_fix, c->nM);
        r.valid = 1; r.reserved = 0;
        out[k] = r;
    }
    return tc.finish();
}

extern "C" int stocs_symmetry_errors_detail(stocs_ctx* c, const float* sym, const stocs_symmetry_params* p, float* s, int32_t* nn, float* dot) {
    const char* who = "stocs_symmetry_errors_detail";
    if (!c || !sym || !p) { set_error("%s: NULL context, transform or parameters", who); return STOCS_ERR_INVALID; }
    { const int rc = check_sym_args(who, sym, 1, p); if (rc) return rc; }
    { const int rc = check_model(who, c); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    SymmetryState* S = ctx_state<SymmetryState>(c);
    { const int rc = ensure_sym_grid(c, S, p->reach); if (rc) return rc; }
    const size_t M = (size_t)c->nM;
    Carve cv;
    const size_t o_sym = cv.take(64), o_s = cv.take(M * 4), o_nn = cv.take(M * 4), o_dot = cv.take(M * 4);
    { const int rc = S->work.grow(c->stream, cv.total); if (rc) return rc; }
    char* hp;
    { const int rc = pinned_var(c, cv.total, &hp); if (rc) return rc; }
    memcpy(hp + o_sym, sym, 64);
    STOCS_HIP_CHECK(hipMemcpyAsync(S->work.p + o_sym, hp + o_sym, 64, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(symmetry_kernel<true>, dim3(1u), dim3(SY_THREADS), 0, c->stream, Carve::at<const float>(S->work.p, o_sym), S->g,
                       Carve::at<const unsigned>(S->grid.p, 0), Carve::at<const float4>(S->grid.p, S->o_sorted), (const float4*)c->d_mpos_raw,
                       (const float4*)c->d_mnrm, c->nM, p->reach, p->reach * p->reach, p->cos_normal, (stocs_symmetry_error*)NULL,
                       Carve::at<float>(S->work.p, o_s), Carve::at<int32_t>(S->work.p, o_nn), Carve::at<float>(S->work.p, o_dot));
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(hipMemcpyAsync(hp + o_s, S->work.p + o_s, cv.total - o_s, hipMemcpyDeviceToHost, c->stream));   // the three outputs in one copy
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (s) memcpy(s, hp + o_s, M * 4);
    if (nn) memcpy(nn, hp + o_nn, M * 4);
    if (dot) memcpy(dot, hp + o_dot, M * 4);
    return STOCS_OK;
}

extern "C" int stocs_symmetry_axes(int n_axes, float* axes3, int cap, int* n) {
    const char* who = "stocs_symmetry_axes";
    if (!n) { set_error("%s: NULL count", who); return STOCS_ERR_INVALID; }
    *n = 0;
    if (n_axes < 3) { set_error("%s: n_axes = %d, fewer than the three coordinate axes", who, n_axes); return STOCS_ERR_INVALID; }
    *n = n_axes;
    if (cap < n_axes || !axes3) { set_error("%s: %d entries, room for %d", who, n_axes, axes3 ? cap : 0); return STOCS_ERR_INVALID; }
    for (int d = 0; d < 3; ++d)
        for (int e = 0; e < 3; ++e) axes3[3 * d + e] = d == e ? 1.0f : 0.0f;
    const int L = n_axes - 3;
    const double g = SY_PI * (3.0 - sqrt(5.0));
    for (int k = 0; k < L; ++k) {
        const double z = 1.0 - ((double)k + 0.5) / (double)L, r = sqrt(1.0 - z * z), phi = (double)k * g;
        double v[3] = {r * cos(phi), r * sin(phi), z};
        normalise3d(v);
        for (int e = 0; e < 3; ++e) axes3[3 * (3 + k) + e] = (float)(v[e] + 0.0);
    }
    return STOCS_OK;
}

extern "C" int stocs_symmetry_rotation(const float axis3[3], double angle_deg, const float* center3, float out16[16]) {
    if (!axis3 || !out16) { set_error("stocs_symmetry_rotation: NULL axis or result"); return STOCS_ERR_INVALID; }
    if (rotation16(axis3, angle_deg, center3, out16)) { set_error("stocs_symmetry_rotation: a zero or non-finite axis, or a non-finite angle or centre"); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}

extern "C" int stocs_symmetry_close(const float* gen16, int n_gen, float same_deg, float* out16, int cap, int* K, int* truncated) {
    const char* who = "stocs_symmetry_close";
    if (!K || !truncated) { set_error("%s: NULL count or flag", who); return STOCS_ERR_INVALID; }
    *K = 0; *truncated = 0;
    if (n_gen < 0 || (n_gen > 0 && !gen16)) { set_error("%s: %d generators at %p", who, n_gen, (const void*)gen16); return STOCS_ERR_INVALID; }
    if (!out16 || cap < 1 || cap > STOCS_POSE_SYM_MAX) { set_error("%s: room for %d entries, not 1 .. %d", who, out16 ? cap : 0, (int)STOCS_POSE_SYM_MAX); return STOCS_ERR_INVALID; }
    if (!(same_deg >= 0.0f) || !host_finite(same_deg)) { set_error("%s: same_deg %g", who, (double)same_deg); return STOCS_ERR_INVALID; }
    std::vector<M4d> gen((size_t)n_gen);
    double scale = 0.0;
    const int bad = first_nonfinite_pose(gen16, n_gen);
    if (bad >= 0) { set_error("%s: generator %d has a non-finite entry", who, bad); return STOCS_ERR_INVALID; }
    for (int k = 0; k < n_gen; ++k) {
        gen[k] = m4_identity();
        for (int e = 0; e < 15; ++e)
            if ((e & 3) != 3) gen[k].e[e] = (double)gen16[(size_t)k * 16 + e];
        scale = std::max(scale, sqrt(gen[k].e[12] * gen[k].e[12] + gen[k].e[13] * gen[k].e[13] + gen[k].e[14] * gen[k].e[14]));
    }
    const double same_rad = (double)same_deg * SY_PI / 180.0;
    const double min_trace = 1.0 + 2.0 * cos(same_rad), max_shift = same_rad * scale;
    std::vector<M4d> kept;
    kept.push_back(m4_identity());
    bool full = false;
    for (size_t at = 0; at < kept.size() && !full; ++at) {
        for (int h = 0; h < n_gen && !full; ++h) {
            const M4d prod = m4_mul(gen[h], kept[at]);
            bool is_new = true;
            for (size_t k = 0; k < kept.size() && is_new; ++k) {
                const M4d& B = kept[k];
                double tr = 0.0;
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) tr += prod.e[4 * b + a] * B.e[4 * b + a];   // trace of A^T B
                const double dx = prod.e[12] - B.e[12], dy = prod.e[13] - B.e[13], dz = prod.e[14] - B.e[14];
                if (tr >= min_trace && sqrt(dx * dx + dy * dy + dz * dz) <= max_shift) is_new = false;
            }
            if (!is_new) continue;
            if ((int)kept.size() >= cap) { *truncated = 1; full = true; break; }
            kept.push_back(prod);
        }
    }
    for (size_t k = 0; k < kept.size(); ++k) m4_round(kept[k], out16 + k * 16);
    *K = (int)kept.size();
    return STOCS_OK;
}

extern "C" void stocs_default_symmetry_search(stocs_symmetry_search* s) {
    if (!s) return;
    s->tol_max = 0.0f;
    s->cos_normal = 0.8660254037844387f;   // cos 30 degrees
    s->max_normal_bad = 1.0f;
    s->n_axes = 2048; s->max_order = 6; s->n_continuous = 72;
    s->n_refine = 16; s->n_local = 32; s->rounds = 4;
    s->same_deg = 6.0f;
}

namespace {
struct SyCand { float axis[3]; int order; stocs_symmetry_error rec; };
struct SyRank { float mean; int index; };
bool rank_less(const SyRank& a, const SyRank& b) { return a.mean < b.mean || (a.mean == b.mean && a.index < b.index); }
}  // namespace

extern "C" int stocs_find_symmetries(stocs_ctx* c, const stocs_symmetry_search* sp, const float* center3, stocs_symmetry_axis* axes, int cap_axes, int* n_axes_out,
                                     float* set16, int cap_set, int* K, float sym3[3], int* flags) {
    const char* who = "stocs_find_symmetries";
    if (!c || !sp || !n_axes_out || !K || !sym3 || !flags) { set_error("%s: NULL context, search, count, descriptor or flags", who); return STOCS_ERR_INVALID; }
    *n_axes_out = 0; *K = 0; *flags = 0;
    sym3[0] = sym3[1] = sym3[2] = 0.0f;
    if (cap_axes < 0 || (cap_axes > 0 && !axes) || !set16 || cap_set < 1) { set_error("%s: no room for the axes or the set", who); return STOCS_ERR_INVALID; }
    const stocs_symmetry_search s = *sp;
    if (s.n_axes < 3 || s.max_order < 2 || s.n_continuous < 1 || s.n_refine < 1 || s.n_local < 1 || s.rounds < 0 || !(s.same_deg > 0.0f) || !host_finite(s.same_deg) ||
        !host_finite(s.tol_max)) {
        set_error("%s: search parameters out of range", who);
        return STOCS_ERR_INVALID;
    }
    if (center3 && !(host_finite(center3[0]) && host_finite(center3[1]) && host_finite(center3[2]))) { set_error("%s: non-finite centre", who); return STOCS_ERR_INVALID; }
    { const int rc = check_model(who, c); if (rc) return rc; }
    const int M = c->nM, NO = s.max_order - 1;
    float centre[3];
    if (center3) { for (int d = 0; d < 3; ++d) centre[d] = center3[d]; }
    else {
        double sum[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < M; ++i) { sum[0] += (double)c->h_mpos_raw[i].x; sum[1] += (double)c->h_mpos_raw[i].y; sum[2] += (double)c->h_mpos_raw[i].z; }
        for (int d = 0; d < 3; ++d) centre[d] = (float)(sum[d] / (double)M);
        if (!(host_finite(centre[0]) && host_finite(centre[1]) && host_finite(centre[2]))) { set_error("%s: the model's centroid is not finite", who); return STOCS_ERR_INVALID; }
    }
    float tol = s.tol_max;
    if (!(tol > 0.0f)) {
        float d = 0.0f;
        { const int rc = stocs_model_diameter(c, &d); if (rc) return rc; }
        tol = 0.1f * d;
        if (!(tol > 0.0f) || !host_finite(tol)) { set_error("%s: a model of diameter %g has no default tolerance", who, (double)d); return STOCS_ERR_INVALID; }
    }
    stocs_symmetry_params prm;
    prm.reach = tol; prm.cos_normal = s.cos_normal; prm.reserved[0] = prm.reserved[1] = 0;
    const double cos_same = cos((double)s.same_deg * SY_PI / 180.0);

    std::vector<float> T;
    std::vector<stocs_symmetry_error> rec;
    // a batch of (axis, order) pairs through the kernel
    struct Score {
        static int run(stocs_ctx* c, const stocs_symmetry_params& prm, const float* centre, const std::vector<float>& ax, const std::vector<int>& order,
                       std::vector<float>& T, std::vector<stocs_symmetry_error>& rec) {
            const size_t n = order.size();
            T.resize(n * 16); rec.resize(n);
            for (size_t k = 0; k < n; ++k)
                if (rotation16(&ax[3 * k], 360.0 / (double)order[k], centre, &T[16 * k])) { set_error("stocs_find_symmetries: a degenerate candidate axis"); return STOCS_ERR_STATE; }
            return stocs_symmetry_errors(c, T.data(), (int)n, &prm, rec.data());
        }
    };

    // 1. coarse pass
    std::vector<float> dirs((size_t)s.n_axes * 3);
    { int n = 0; const int rc = stocs_symmetry_axes(s.n_axes, dirs.data(), s.n_axes, &n); if (rc) return rc; }
    std::vector<float> ax; std::vector<int> ord;
    ax.reserve((size_t)s.n_axes * NO * 3); ord.reserve((size_t)s.n_axes * NO);
    for (int d = 0; d < s.n_axes; ++d)
        for (int n = 2; n <= s.max_order; ++n) { ax.insert(ax.end(), &dirs[3 * d], &dirs[3 * d] + 3); ord.push_back(n); }
    { const int rc = Score::run(c, prm, centre, ax, ord, T, rec); if (rc) return rc; }
    std::vector<SyRank> rank(ord.size());
    for (size_t k = 0; k < ord.size(); ++k) { rank[k].mean = rec[k].mean; rank[k].index = (int)k; }
    std::sort(rank.begin(), rank.end(), rank_less);

    // 2. refinement
    std::vector<SyCand> kept;
    for (size_t r = 0; r < rank.size() && (int)kept.size() < s.n_refine; ++r) {
        const int k = rank[r].index;
        bool apart = true;
        for (size_t q = 0; q < kept.size() && apart; ++q) apart = axis_cos(kept[q].axis, &ax[3 * k]) < cos_same;
        if (!apart) continue;
        SyCand cd;
        for (int e = 0; e < 3; ++e) cd.axis[e] = ax[3 * k + e];
        cd.order = ord[k]; cd.rec = rec[k];
        kept.push_back(cd);
    }
    const int L = s.n_axes - 3;
    const double spacing = L > 0 ? sqrt(2.0 * SY_PI / (double)L) : SY_PI / 4.0, golden = SY_PI * (3.0 - sqrt(5.0));
    for (int round = 0; round < s.rounds; ++round) {
        const double theta = spacing / (double)(1 << (round < 30 ? round : 30));
        ax.clear(); ord.clear();
        for (size_t q = 0; q < kept.size(); ++q) {
            double a[3] = {(double)kept[q].axis[0], (double)kept[q].axis[1], (double)kept[q].axis[2]};
            int e = 0;
            for (int d = 1; d < 3; ++d) if (fabs(a[d]) < fabs(a[e])) e = d;
            double u[3] = {-a[e] * a[0], -a[e] * a[1], -a[e] * a[2]};
            u[e] += 1.0;
            normalise3d(u);
            const double v[3] = {a[1] * u[2] - a[2] * u[1], a[2] * u[0] - a[0] * u[2], a[0] * u[1] - a[1] * u[0]};
            for (int k = 0; k < s.n_local; ++k) {
                const double t = tan(theta * sqrt(((double)k + 0.5) / (double)s.n_local)), cp = cos((double)k * golden), sn = sin((double)k * golden);
                double w[3];
                for (int d = 0; d < 3; ++d) w[d] = a[d] + t * (cp * u[d] + sn * v[d]);
                normalise3d(w);
                for (int d = 0; d < 3; ++d) ax.push_back((float)(w[d] + 0.0));
                ord.push_back(kept[q].order);
            }
        }
        { const int rc = Score::run(c, prm, centre, ax, ord, T, rec); if (rc) return rc; }
        for (size_t q = 0; q < kept.size(); ++q) {
            for (int k = 0; k < s.n_local; ++k) {
                const size_t at = q * (size_t)s.n_local + (size_t)k;
                if (rec[at].mean < kept[q].rec.mean) {
                    kept[q].rec = rec[at];
                    for (int d = 0; d < 3; ++d) kept[q].axis[d] = ax[3 * at + d];
                }
            }
        }
    }

    // 3. decision
    ax.clear(); ord.clear();
    for (size_t q = 0; q < kept.size(); ++q)
        for (int n = 2; n <= s.max_order; ++n) { ax.insert(ax.end(), kept[q].axis, kept[q].axis + 3); ord.push_back(n); }
    { const int rc = Score::run(c, prm, centre, ax, ord, T, rec); if (rc) return rc; }
    std::vector<stocs_symmetry_axis> found;
    std::vector<SyRank> frank;
    for (size_t q = 0; q < kept.size(); ++q) {
        int best = 0, n_pass = 0;
        for (int n = 2; n <= s.max_order; ++n) {
            const stocs_symmetry_error& r = rec[q * (size_t)NO + (size_t)(n - 2)];
            const bool pass = r.n_far == 0 && r.max <= tol && (float)r.n_normal_bad <= s.max_normal_bad * (float)M;
            if (pass) { best = n; ++n_pass; }
        }
        if (!best) continue;
        const bool continuous = n_pass == NO;
        const stocs_symmetry_error& r = rec[q * (size_t)NO + (size_t)((continuous ? s.max_order : best) - 2)];
        stocs_symmetry_axis A;
        for (int d = 0; d < 3; ++d) A.axis[d] = kept[q].axis[d];
        A.order = continuous ? 0 : best; A.max = r.max; A.mean = r.mean; A.n_normal_bad = r.n_normal_bad; A.reserved = 0;
        SyRank fr; fr.mean = r.mean; fr.index = (int)found.size();
        found.push_back(A); frank.push_back(fr);
    }
    std::sort(frank.begin(), frank.end(), rank_less);
    std::vector<stocs_symmetry_axis> final_axes;
    for (size_t r = 0; r < frank.size(); ++r) {
        const stocs_symmetry_axis& A = found[frank[r].index];
        bool apart = true;
        for (size_t q = 0; q < final_axes.size() && apart; ++q) apart = axis_cos(final_axes[q].axis, A.axis) < cos_same;
        if (apart) final_axes.push_back(A);
    }

    // 4. output
    *n_axes_out = (int)final_axes.size();
    for (int k = 0; k < (int)final_axes.size() && k < cap_axes; ++k) axes[k] = final_axes[k];
    std::vector<float> gens(final_axes.size() * 16);
    bool exact = true;
    float desc[3] = {0.0f, 0.0f, 0.0f};
    bool named[3] = {false, false, false};
    for (size_t k = 0; k < final_axes.size(); ++k) {
        const stocs_symmetry_axis& A = final_axes[k];
        const int n = A.order == 0 ? s.n_continuous : A.order;
        if (rotation16(A.axis, 360.0 / (double)n, centre, &gens[16 * k])) { set_error("%s: a degenerate axis", who); return STOCS_ERR_STATE; }
        int on = -1;
        for (int d = 0; d < 3; ++d) if (fabs((double)A.axis[d]) >= cos_same) on = d;
        const float names = A.order == 0 ? 360.0f : (A.order == 2 ? 180.0f : (A.order == 4 ? 90.0f : 0.0f));
        if (on < 0 || names == 0.0f || named[on]) exact = false;   // (two kept axes on one coordinate axis: the descriptor cannot say so)
        else { desc[on] = names; named[on] = true; }
    }
    if (final_axes.empty()) *flags |= STOCS_SYMMETRY_NOTHING_FOUND;
    else if (!exact) *flags |= STOCS_SYMMETRY_DESCRIPTOR_INEXACT;
    else { sym3[0] = desc[0]; sym3[1] = desc[1]; sym3[2] = desc[2]; }
    const float close_deg = std::min(s.same_deg, 90.0f / (float)s.n_continuous);
    int truncated = 0;
    { const int rc = stocs_symmetry_close(gens.data(), (int)final_axes.size(), close_deg, set16, std::min(cap_set, (int)STOCS_POSE_SYM_MAX), K, &truncated); if (rc) return rc; }
    if (truncated) *flags |= STOCS_SYMMETRY_SET_TRUNCATED;
    return STOCS_OK;
}
