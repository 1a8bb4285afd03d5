// segment_shapes.hip -- the 3-D shape of every labelled region of a depth frame, the size gate between segments and objects, and the
// object-major class stack (stocs_segment_shapes, stocs_points_shape, stocs_segment_assign; no reference counterpart).  The contract is at
// the declaration in include/stocs_hip.h; tests/segment_shapes_ref.py restates it in numpy.  The labels may be anybody's.
//
// Kernels, in launch order (one stream, no host round trip; every sum an integer, every extreme an integer on a monotone map of the float
// bits: order-free).  The two pixel passes are templates on where a point comes from: ShpFrame (depth + labels) or ShpPoints (a point array
// as one label).  Both run one workgroup per SEG_TILE_W x SEG_TILE_H tile, one wavefront per tile row, four rows per wavefront:
//   shp_moments   per row: the lanes that share the first used lane's label reduce their ten int64 terms by shuffles and the leader adds
//                 them to the tile's LDS table (SHP_SLOTS labels, open addressing, 64-bit sums); the other used lanes add their own terms to
//                 the table; a label that finds the table full goes straight to device memory.  Behind the barrier one device atomic per
//                 occupied slot and non-zero moment.  The five counts of the result by ballots (wg_add_counts).
//   shp_shape     one lane per label: centroid and covariance in double from the moments, all three eigenpairs (seg_eigen3, the sibling of
//                 segment.hip's seg_smallest_eigvec: the same sweeps), order, sign, one cast each; the extent words set to their neutral values
//   shp_extents   the second pass: t_k = a_k . (p - c) in float, the same leading-run reduction (wave_min_i / wave_max_i on the keys), the
//                 six extent words per label in the LDS table, one device atomic per occupied slot and word
//   shp_finish    one lane per label: lo, hi, extent from the keys
//   shp_gate      (n_objects > 0) one lane per (object, label): segment_gate.h's rule, the reasons, the label's bit in its "allowed" word
//   shp_stack     (n_objects > 0) one lane per pixel: one gather of the label's allowed word, n_objects coalesced stores
//
// Host: the entry points refuse what they can (the order is at the declaration) and hand a ShpCall to shapes_run, the one launch sequence;
// the thread's arena per device and pinned block are a ThreadCache of this file's own, which stocs_trim gives back (segment_shapes_trim).
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>

#include "segment.h"
#include "segment_gate.h"
#include "segment_rules.h"
#include "stocs_ctx.h"
#include "thread_cache.h"
#include "wave_bits.h"

namespace stocs {

static_assert(sizeof(stocs_segment_shape) == 128 && offsetof(stocs_segment_shape, lo) == 68 && offsetof(stocs_segment_shape, extent) == 92, "stocs_segment_shape is 128 bytes");
static_assert(sizeof(stocs_segment_shapes_result) == 32 && sizeof(stocs_object_size) == 16 && sizeof(stocs_segment_gate_params) == 16, "shape ABI");
// wg_add_counts addresses the five counters as an array
static_assert(offsetof(stocs_segment_shapes_result, n_labelled) == 0 && offsetof(stocs_segment_shapes_result, n_out_of_range) == 16, "shp_moments");

enum { SHP_SLOTS = 32, SHP_SLOT_BITS = 5 };                       // labels a tile's table holds
enum { SHP_NONE = 0, SHP_USED = 1, SHP_INVALID = 2, SHP_FAR = 3, SHP_RANGE = 4 };   // what a lane's pixel is
enum { SHP_KEY_MAX = 0x7FFFFFFF, SHP_KEY_MIN = -0x7FFFFFFF - 1 };

__device__ __forceinline__ int shp_near(V3 p) { return (fabsf(p.x) < 16.0f && fabsf(p.y) < 16.0f && fabsf(p.z) < 16.0f) ? SHP_USED : SHP_FAR; }

// a frame: lane `lane` of tile row r of tile (tx, ty)
struct ShpFrame {
    const uint16_t* depth; const int32_t* labels;
    int W, H, n_labels;
    float fx, cx, fy, cy, depth_scale, max_depth;
    __device__ __forceinline__ int fetch(int tx, int ty, int r, int lane, int* lab, V3* p) const {
        const int x = tx * SEG_TILE_W + lane, y = ty * SEG_TILE_H + r;
        if (x >= W || y >= H) return SHP_NONE;
        const size_t idx = (size_t)y * W + x;
        const int l = labels[idx];
        if (l == 0) return SHP_NONE;
        if (l < 0 || l > n_labels) return SHP_RANGE;
        *lab = l;
        const uint16_t raw = depth[idx];
        const float z = (float)raw * depth_scale;
        if (!(raw != 0 && z <= max_depth)) return SHP_INVALID;
        *p = seg_unproject(y, x, z, fx, cx, fy, cy);
        return shp_near(*p);
    }
};
// a point array as label 1: "tile" tx holds the points tx * 1024 .. + 1023, a tile row 64 of them
struct ShpPoints {
    const float* pos; int n;
    __device__ __forceinline__ int fetch(int tx, int, int r, int lane, int* lab, V3* p) const {
        const long long idx = (long long)tx * (SEG_TILE_W * SEG_TILE_H) + r * SEG_TILE_W + lane;
        if (idx >= n) return SHP_NONE;
        *lab = 1;
        *p = mk3(pos[3 * idx], pos[3 * idx + 1], pos[3 * idx + 2]);
        return shp_near(*p);
    }
};

// the slot of `lab` in a tile's table (keys: 0 = free), claimed when it has none; -1 when the table holds SHP_SLOTS other labels.  No lane
// waits for another: a slot's key is written once, by the compare-and-swap that claims it.
__device__ __forceinline__ int shp_slot(int* keys, int lab) {
    const uint32_t h = ((uint32_t)lab * 2654435761u) >> (32 - SHP_SLOT_BITS);
    for (int i = 0; i < SHP_SLOTS; ++i) {
        const int s = (int)((h + (uint32_t)i) & (SHP_SLOTS - 1));
        const int old = atomicCAS(&keys[s], 0, lab);
        if (old == 0 || old == lab) return s;
    }
    return -1;
}
__device__ __forceinline__ void shp_add(int* keys, unsigned long long (*sums)[10], unsigned long long* mom, int lab, const long long* v) {
    const int s = shp_slot(keys, lab);
    unsigned long long* dst = s >= 0 ? sums[s] : mom + 10 * (size_t)(lab - 1);     // LDS, or device memory when the table is full
#pragma unroll
    for (int k = 0; k < 10; ++k)
        if (v[k]) atomicAdd(dst + k, (unsigned long long)v[k]);
}
__device__ __forceinline__ void shp_minmax(int* keys, int (*words)[6], int* ext, int lab, const int* lo, const int* hi) {
    const int s = shp_slot(keys, lab);
    int* dst = s >= 0 ? words[s] : ext + 6 * (size_t)(lab - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) { atomicMin(dst + k, lo[k]); atomicMax(dst + 3 + k, hi[k]); }
}

// float -> int, monotone: the bits as a signed integer, a negative float's low 31 bits inverted (-0 below +0); and back
__device__ __forceinline__ int shp_key(float t) { const int b = __float_as_int(t); return b >= 0 ? b : b ^ 0x7FFFFFFF; }
__device__ __forceinline__ float shp_unkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7FFFFFFF); }

template <class Src>
__global__ __launch_bounds__(256) void shp_moments_kernel(const Src src, unsigned long long* mom, stocs_segment_shapes_result* res) {
    __shared__ int s_key[SHP_SLOTS];
    __shared__ unsigned long long s_sum[SHP_SLOTS][10];
    __shared__ int s_n[4][5];
    for (int t = threadIdx.x; t < SHP_SLOTS * 10; t += 256) (&s_sum[0][0])[t] = 0ull;
    if (threadIdx.x < SHP_SLOTS) s_key[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int acc[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int lab = 0;
        V3 p = mk3(0.0f, 0.0f, 0.0f);
        const int st = src.fetch(blockIdx.x, blockIdx.y, wave * 4 + k, lane, &lab, &p);
        const bool used = st == SHP_USED;
        const unsigned long long act = __ballot(used);
        acc[0] += __popcll(__ballot(st == SHP_USED || st == SHP_INVALID || st == SHP_FAR)); acc[1] += __popcll(act);
        acc[2] += __popcll(__ballot(st == SHP_INVALID)); acc[3] += __popcll(__ballot(st == SHP_FAR)); acc[4] += __popcll(__ballot(st == SHP_RANGE));
        if (!act) continue;                                             // wave-uniform
        const int first = (int)__ffsll((long long)act) - 1;
        const int lab0 = __shfl(lab, first, 64);
        const bool mine = used && lab == lab0;
        // |v| < 16 m keeps |q| below 2^20 and a product below 2^40: 2^22 pixels sum below 2^62 (seg_refit_kernel's argument)
        const long long x = used ? __double2ll_rn((double)p.x * 65536.0) : 0, y = used ? __double2ll_rn((double)p.y * 65536.0) : 0, z = used ? __double2ll_rn((double)p.z * 65536.0) : 0;
        const long long v[10] = {used ? 1 : 0, x, y, z, x * x, x * y, x * z, y * y, y * z, z * z};
        long long m[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) m[j] = wave_sum_ll(mine ? v[j] : 0);
        if (lane == first) shp_add(s_key, s_sum, mom, lab0, m);
        else if (used && !mine) shp_add(s_key, s_sum, mom, lab, v);
    }
    wg_add_counts<5>(acc, s_n, &res->n_labelled);                      // its barrier: the table is complete behind it
    for (int t = threadIdx.x; t < SHP_SLOTS * 10; t += 256) {
        const int key = s_key[t / 10];
        const unsigned long long sum = s_sum[t / 10][t % 10];
        if (key && sum) atomicAdd(mom + 10 * (size_t)(key - 1) + t % 10, sum);
    }
}

// all three eigenpairs of a symmetric 3x3: seg_smallest_eigvec's cyclic Jacobi in double (pairs (0,1), (0,2), (1,2), SEG_SWEEPS sweeps);
// w[j] = the j-th diagonal entry left, its eigenvector column j of V
__device__ __forceinline__ void seg_eigen3(double a00, double a01, double a02, double a11, double a12, double a22, double w[3], double V[3][3]) {
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SEG_SWEEPS; ++sweep) {
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            if (A[p][q] == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
            const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
        }
    }
    w[0] = A[0][0]; w[1] = A[1][1]; w[2] = A[2][2];
}

struct ShpPair { double w, v0, v1, v2; };
// b in front of a when its eigenvalue is larger (strictly: on equal values the lower column stays first)
__device__ __forceinline__ void shp_order(ShpPair& a, ShpPair& b) {
    if (b.w > a.w) { const ShpPair t = a; a = b; b = t; }
}

// one lane per label: the record up to the axes, from the moments; the extent words and the allowed word to their neutral values
__global__ __launch_bounds__(256) void shp_shape_kernel(const long long* __restrict__ mom, int n_labels, stocs_segment_shape* __restrict__ shapes, int* __restrict__ ext,
                                                        unsigned long long* __restrict__ allowed) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_labels) return;
    const long long* M = mom + 10 * (size_t)l;
#pragma unroll
    for (int k = 0; k < 3; ++k) { ext[6 * (size_t)l + k] = SHP_KEY_MAX; ext[6 * (size_t)l + 3 + k] = SHP_KEY_MIN; }
    if (allowed) allowed[l] = 0ull;
    stocs_segment_shape s;
    memset(&s, 0, sizeof(s));
    if (M[0] == 0) { s.flags = STOCS_SHAPE_EMPTY; shapes[l] = s; return; }
    s.n_used = (int)M[0];
    const double n = (double)M[0], u = 1.0 / 65536.0, uu = u * u;
    const double cx = (double)M[1] / n * u, cy = (double)M[2] / n * u, cz = (double)M[3] / n * u;
    double w[3], V[3][3];
    seg_eigen3((double)M[4] / n * uu - cx * cx, (double)M[5] / n * uu - cx * cy, (double)M[6] / n * uu - cx * cz, (double)M[7] / n * uu - cy * cy,
               (double)M[8] / n * uu - cy * cz, (double)M[9] / n * uu - cz * cz, w, V);
    ShpPair e[3] = {{w[0], V[0][0], V[1][0], V[2][0]}, {w[1], V[0][1], V[1][1], V[2][1]}, {w[2], V[0][2], V[1][2], V[2][2]}};
    shp_order(e[0], e[1]); shp_order(e[1], e[2]); shp_order(e[0], e[1]);
    bool good = isfinite(cx) && isfinite(cy) && isfinite(cz);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double len = sqrt(e[k].v0 * e[k].v0 + (e[k].v1 * e[k].v1 + e[k].v2 * e[k].v2));
        double a0 = e[k].v0 / len, a1 = e[k].v1 / len, a2 = e[k].v2 / len;
        double big = a0;                                                 // the component of largest magnitude, the lowest index on a tie
        if (fabs(a1) > fabs(big)) big = a1;
        if (fabs(a2) > fabs(big)) big = a2;
        if (big < 0) { a0 = -a0; a1 = -a1; a2 = -a2; }
        good = good && isfinite(e[k].w) && isfinite(a0) && isfinite(a1) && isfinite(a2);
        s.eigenvalue[k] = (float)e[k].w;
        s.axis[k][0] = (float)a0; s.axis[k][1] = (float)a1; s.axis[k][2] = (float)a2;
    }
    s.centroid[0] = (float)cx; s.centroid[1] = (float)cy; s.centroid[2] = (float)cz;
    // Not reachable from the entry points, and no test reaches it: n >= 1 and every sum is below 2^62, so centroid and covariance are finite
    // doubles of magnitude below 2^8, a rotation keeps them so (theta may overflow to infinity: then t = 0, c = 1, s = 0), and a column of V
    // has length 1 to rounding.  The branch is the contract's answer should that ever fail to hold; tests/segment_shapes_ref.py restates it.
    if (!good) {
        s.flags = STOCS_SHAPE_NONFINITE;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s.eigenvalue[k] = 0.0f;
            if (!isfinite(s.centroid[k])) s.centroid[k] = 0.0f;
#pragma unroll
            for (int j = 0; j < 3; ++j) s.axis[k][j] = k == j ? 1.0f : 0.0f;
        }
    }
    shapes[l] = s;
}

template <class Src>
__global__ __launch_bounds__(256) void shp_extents_kernel(const Src src, const stocs_segment_shape* __restrict__ shapes, int* ext) {
    __shared__ int s_key[SHP_SLOTS];
    __shared__ int s_ext[SHP_SLOTS][6];
    if (threadIdx.x < SHP_SLOTS) {
        s_key[threadIdx.x] = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { s_ext[threadIdx.x][k] = SHP_KEY_MAX; s_ext[threadIdx.x][3 + k] = SHP_KEY_MIN; }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int lab = 0;
        V3 p = mk3(0.0f, 0.0f, 0.0f);
        const bool used = src.fetch(blockIdx.x, blockIdx.y, wave * 4 + k, lane, &lab, &p) == SHP_USED;
        const unsigned long long act = __ballot(used);
        if (!act) continue;                                             // wave-uniform
        const int first = (int)__ffsll((long long)act) - 1;
        const int lab0 = __shfl(lab, first, 64);
        const bool mine = used && lab == lab0;
        int key[3] = {0, 0, 0};
        if (used) {
            const stocs_segment_shape* s = shapes + (lab - 1);
            const float dx = p.x - s->centroid[0], dy = p.y - s->centroid[1], dz = p.z - s->centroid[2];
#pragma unroll
            for (int j = 0; j < 3; ++j) key[j] = shp_key(s->axis[j][0] * dx + (s->axis[j][1] * dy + s->axis[j][2] * dz));
        }
        int lo[3], hi[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { lo[j] = wave_min_i(mine ? key[j] : (int)SHP_KEY_MAX); hi[j] = wave_max_i(mine ? key[j] : (int)SHP_KEY_MIN); }
        if (lane == first) shp_minmax(s_key, s_ext, ext, lab0, lo, hi);
        else if (used && !mine) shp_minmax(s_key, s_ext, ext, lab, key, key);
    }
    __syncthreads();
    if (threadIdx.x < SHP_SLOTS * 6) {
        const int slot = threadIdx.x / 6, j = threadIdx.x % 6, key = s_key[slot];
        if (key) {
            int* dst = ext + 6 * (size_t)(key - 1) + j;
            if (j < 3) atomicMin(dst, s_ext[slot][j]); else atomicMax(dst, s_ext[slot][j]);
        }
    }
}

__global__ __launch_bounds__(256) void shp_finish_kernel(const int* __restrict__ ext, int n_labels, stocs_segment_shape* __restrict__ shapes) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_labels || shapes[l].n_used == 0) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float lo = shp_unkey(ext[6 * (size_t)l + k]), hi = shp_unkey(ext[6 * (size_t)l + 3 + k]);
        shapes[l].lo[k] = lo; shapes[l].hi[k] = hi; shapes[l].extent[k] = hi - lo;
    }
}

__global__ __launch_bounds__(256) void shp_gate_kernel(const stocs_segment_shape* __restrict__ shapes, int n_labels, const stocs_object_size* __restrict__ objects, int n_objects,
                                                       stocs_segment_gate_params g, uint8_t* __restrict__ reasons, unsigned long long* allowed) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_objects * n_labels) return;
    const int o = t / n_labels, l = t % n_labels;
    const unsigned r = segment_gate_reasons(shapes[l], objects[o], g);
    reasons[t] = (uint8_t)r;
    if (!r) atomicOr(allowed + l, 1ull << o);
}

__global__ __launch_bounds__(256) void shp_stack_kernel(const int32_t* __restrict__ labels, int npix, int n_labels, int n_objects, const unsigned long long* __restrict__ allowed,
                                                        uint16_t* __restrict__ stack) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix) return;
    const int lab = labels[idx];
    const unsigned long long word = (lab >= 1 && lab <= n_labels) ? allowed[lab - 1] : 0ull;
    for (int k = 0; k < n_objects; ++k) stack[(size_t)k * npix + idx] = ((word >> k) & 1ull) ? (uint16_t)10000 : (uint16_t)0;
}

// ---- the calling thread's cached memory (stocs_trim gives it back through segment_trim): the arena per device and the pinned block
static thread_local ThreadCache tl_shp_cache;
// the HIP-event time of the thread's last call under STOCS_SEGMENT_CLOCK=1, from the first memset to the last kernel: plain data
struct ShpClock { hipEvent_t ev[2]; bool made; int dev; float ms; bool valid; };
static thread_local ShpClock tl_shp_clock;

void segment_shapes_trim() {
    tl_shp_cache.trim();
    if (tl_shp_clock.made) { (void)hipEventDestroy(tl_shp_clock.ev[0]); (void)hipEventDestroy(tl_shp_clock.ev[1]); tl_shp_clock.made = false; }
}

// what an entry point hands to the one launch sequence; it has refused what the declaration lists.  A frame (cam, depth, labels) or a
// point array (pos, n: one label)
struct ShpCall {
    const char* who;
    const stocs_camera* cam; const uint16_t* depth; const int32_t* labels; float max_depth;
    const float* pos; int n;
    int n_labels;
    const stocs_object_size* objects; int n_objects; stocs_segment_gate_params gate;
    int device;
    stocs_segment_shape* shapes; int64_t* moments; uint8_t* reasons; uint16_t* stack; stocs_segment_shapes_result* result;
};

static int shapes_run(const ShpCall& c) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available: this library has no CPU fallback"); return STOCS_ERR_NO_DEVICE; }
    if (c.device >= 0) STOCS_HIP_CHECK(hipSetDevice(c.device));
    const bool frame = c.pos == NULL;
    const int W = frame ? c.cam->width : 0, H = frame ? c.cam->height : 0;
    const size_t npix = frame ? (size_t)W * H : (size_t)c.n, nl = (size_t)c.n_labels, no = (size_t)c.n_objects;
    const size_t nl1 = std::max<size_t>(nl, 1);
    hipStream_t st = NULL;
    int rc;
    Arena* ws = NULL;
    if ((rc = tl_shp_cache.begin(c.device, &ws))) return rc;
    tl_shp_clock.valid = false;

    // the block that comes back in one copy: result | shapes | moments | reasons | class stack
    Carve oc;
    const size_t o_res = oc.take(sizeof(stocs_segment_shapes_result)), o_shp = oc.take(sizeof(stocs_segment_shape) * nl1), o_mom = oc.take(80 * nl1);
    const size_t zero_bytes = oc.total;                                 // the counters and the sums start at zero
    const size_t o_rea = oc.take(std::max<size_t>(no * nl, 1)), o_stk = oc.take(std::max<size_t>(2 * no * npix, 1));
    // what goes up, behind it in the pinned block: depth | labels, or the points; the objects
    Carve ic;
    const size_t i_a = ic.take(std::max<size_t>(frame ? 2 * npix : 12 * npix, 1)), i_b = ic.take(std::max<size_t>(frame ? 4 * npix : 0, 1)), i_obj = ic.take(std::max<size_t>(16 * no, 1));
    char* pin = NULL;
    if ((rc = tl_shp_cache.staging(oc.total + ic.total, &pin))) return rc;
    char* pin_in = pin + oc.total;
    char *d_out = NULL, *d_in = NULL; int* ext = NULL; unsigned long long* allowed = NULL;
    if ((rc = ws->take(oc.total, (void**)&d_out)) || (rc = ws->take(ic.total, (void**)&d_in)) || (rc = ws->take(24 * nl1, (void**)&ext)) || (rc = ws->take(8 * nl1, (void**)&allowed))) return rc;
    stocs_segment_shapes_result* d_res = Carve::at<stocs_segment_shapes_result>(d_out, o_res);
    stocs_segment_shape* d_shp = Carve::at<stocs_segment_shape>(d_out, o_shp);
    unsigned long long* d_mom = Carve::at<unsigned long long>(d_out, o_mom);
    uint8_t* d_rea = Carve::at<uint8_t>(d_out, o_rea); uint16_t* d_stk = Carve::at<uint16_t>(d_out, o_stk);
    const stocs_object_size* d_obj = Carve::at<const stocs_object_size>(d_in, i_obj);

    const char* ce = getenv("STOCS_SEGMENT_CLOCK");
    const bool clock = ce != NULL && atoi(ce) == 1;
    ShpClock& ck = tl_shp_clock;
    if (clock) {
        if (ck.made && ck.dev != tl_shp_cache.dev) { (void)hipEventDestroy(ck.ev[0]); (void)hipEventDestroy(ck.ev[1]); ck.made = false; }
        if (!ck.made) { STOCS_HIP_CHECK(hipEventCreate(&ck.ev[0])); STOCS_HIP_CHECK(hipEventCreate(&ck.ev[1])); ck.made = true; ck.dev = tl_shp_cache.dev; }
    }

    if (frame) { memcpy(pin_in + i_a, c.depth, 2 * npix); memcpy(pin_in + i_b, c.labels, 4 * npix); }
    else if (npix) memcpy(pin_in + i_a, c.pos, 12 * npix);
    if (no) memcpy(pin_in + i_obj, c.objects, 16 * no);
    STOCS_HIP_CHECK(hipMemcpyAsync(d_in, pin_in, ic.total, hipMemcpyHostToDevice, st));
    if (clock) STOCS_HIP_CHECK(hipEventRecord(ck.ev[0], st));
    STOCS_HIP_CHECK(hipMemsetAsync(d_out, 0, zero_bytes, st));
    const dim3 B(256), gl((unsigned)((nl1 + 255) / 256));
    if (frame) {
        const ShpFrame src = {Carve::at<const uint16_t>(d_in, i_a), Carve::at<const int32_t>(d_in, i_b), W, H, c.n_labels, c.cam->fx, c.cam->cx, c.cam->fy, c.cam->cy,
                              c.cam->depth_scale, c.max_depth};
        const dim3 gt((unsigned)((W + SEG_TILE_W - 1) / SEG_TILE_W), (unsigned)((H + SEG_TILE_H - 1) / SEG_TILE_H));
        hipLaunchKernelGGL(shp_moments_kernel<ShpFrame>, gt, B, 0, st, src, d_mom, d_res);
        hipLaunchKernelGGL(shp_shape_kernel, gl, B, 0, st, (const long long*)d_mom, c.n_labels, d_shp, ext, allowed);
        if (nl) hipLaunchKernelGGL(shp_extents_kernel<ShpFrame>, gt, B, 0, st, src, d_shp, ext);
    } else {
        const ShpPoints src = {Carve::at<const float>(d_in, i_a), c.n};
        const dim3 gt((unsigned)std::max<size_t>((npix + SEG_TILE_W * SEG_TILE_H - 1) / (SEG_TILE_W * SEG_TILE_H), 1));
        hipLaunchKernelGGL(shp_moments_kernel<ShpPoints>, gt, B, 0, st, src, d_mom, d_res);
        hipLaunchKernelGGL(shp_shape_kernel, gl, B, 0, st, (const long long*)d_mom, c.n_labels, d_shp, ext, allowed);
        hipLaunchKernelGGL(shp_extents_kernel<ShpPoints>, gt, B, 0, st, src, d_shp, ext);
    }
    hipLaunchKernelGGL(shp_finish_kernel, gl, B, 0, st, ext, c.n_labels, d_shp);
    if (no) {
        if (nl) hipLaunchKernelGGL(shp_gate_kernel, dim3((unsigned)((no * nl + 255) / 256)), B, 0, st, d_shp, c.n_labels, d_obj, c.n_objects, c.gate, d_rea, allowed);
        hipLaunchKernelGGL(shp_stack_kernel, dim3((unsigned)((npix + 255) / 256)), B, 0, st, Carve::at<const int32_t>(d_in, i_b), (int)npix, c.n_labels, c.n_objects, allowed, d_stk);
    }
    STOCS_HIP_CHECK(hipGetLastError());
    if (clock) STOCS_HIP_CHECK(hipEventRecord(ck.ev[1], st));
    const size_t back_bytes = no ? oc.total : o_rea;
    STOCS_HIP_CHECK(hipMemcpyAsync(pin, d_out, back_bytes, hipMemcpyDeviceToHost, st));
    STOCS_HIP_CHECK(hipStreamSynchronize(st));
    if (clock) { STOCS_HIP_CHECK(hipEventElapsedTime(&ck.ms, ck.ev[0], ck.ev[1])); ck.valid = true; }

    if (c.result) *c.result = *Carve::at<const stocs_segment_shapes_result>(pin, o_res);
    if (nl) memcpy(c.shapes, pin + o_shp, sizeof(stocs_segment_shape) * nl);
    if (c.moments && nl) memcpy(c.moments, pin + o_mom, 80 * nl);
    if (no && nl) memcpy(c.reasons, pin + o_rea, no * nl);
    if (no && npix) memcpy(c.stack, pin + o_stk, 2 * no * npix);
    return STOCS_OK;
}

static int gate_params_or_defaults(const stocs_segment_gate_params* in, stocs_segment_gate_params* g) {
    if (in) *g = *in; else stocs_default_segment_gate_params(g);
    return stocs_check_segment_gate_params(g);
}
static int check_objects(const char* who, const stocs_object_size* o, int n) {
    for (int k = 0; k < n; ++k) {
        const float v[4] = {o[k].diameter, o[k].extent[0], o[k].extent[1], o[k].extent[2]};
        for (int j = 0; j < 4; ++j)
            if (!(v[j] >= 0) || !std::isfinite(v[j])) { set_error("%s: object %d: %s %g is negative or not finite", who, k, j ? "extent" : "diameter", (double)v[j]); return STOCS_ERR_INVALID; }
    }
    return STOCS_OK;
}

// stocs_segment_assign and stocs_segment_shapes (n_objects 0): the checks in the declaration's order, then the launch sequence
static int assign_checked(const char* who, const stocs_camera* cam, const uint16_t* depth, const int32_t* labels, int n_labels, float max_depth, const stocs_object_size* objects,
                          int n_objects, const stocs_segment_gate_params* gp, int device, stocs_segment_shape* shapes, int64_t* moments, uint8_t* reasons, uint16_t* stack,
                          stocs_segment_shapes_result* result) {
    if (!(cam && depth && labels && result)) { set_error("%s: NULL camera, depth image, label image or result", who); return STOCS_ERR_INVALID; }
    if (n_labels < 0 || n_labels > SEG_MAX_PIX) { set_error("%s: n_labels %d outside 0..2^22", who, n_labels); return STOCS_ERR_INVALID; }
    if (cam->width < 1 || cam->height < 1) { set_error("%s: frame of %d x %d pixels", who, cam->width, cam->height); return STOCS_ERR_INVALID; }
    if ((long long)cam->width * cam->height > (long long)SEG_MAX_PIX) { set_error("%s: %d x %d pixels, above 2^22 (the moments are 64-bit sums)", who, cam->width, cam->height); return STOCS_ERR_CAPACITY; }
    if (n_objects < 0 || n_objects > STOCS_MAX_FRAME_OBJECTS) { set_error("%s: n_objects %d outside 0..%d", who, n_objects, STOCS_MAX_FRAME_OBJECTS); return STOCS_ERR_INVALID; }
    if (n_labels > 0 && !shapes) { set_error("%s: NULL shapes with n_labels %d", who, n_labels); return STOCS_ERR_INVALID; }
    if (n_objects > 0 && (!objects || !stack || (n_labels > 0 && !reasons))) { set_error("%s: NULL objects, reasons or class_stack with n_objects %d", who, n_objects); return STOCS_ERR_INVALID; }
    if (!(max_depth > 0) || !std::isfinite(max_depth)) { set_error("%s: max_depth %g is not finite or not above 0", who, (double)max_depth); return STOCS_ERR_INVALID; }
    ShpCall c = {who, cam, depth, labels, max_depth, NULL, 0, n_labels, objects, n_objects, {0, 0, 0, 0}, device, shapes, moments, reasons, stack, result};
    int rc;
    if (n_objects > 0 && ((rc = gate_params_or_defaults(gp, &c.gate)) || (rc = check_objects(who, objects, n_objects)))) return rc;
    return shapes_run(c);
}

}  // namespace stocs

using namespace stocs;

extern "C" {

void stocs_default_segment_gate_params(stocs_segment_gate_params* g) {
    if (!g) return;
    memset(g, 0, sizeof(*g));
    g->slack = 0.25f; g->min_ratio = 0.5f; g->min_used = 3;      // from the geometry argument at the declaration, not fitted to data
}

int stocs_check_segment_gate_params(const stocs_segment_gate_params* g) {
    if (!g) { set_error("stocs_check_segment_gate_params: NULL params"); return STOCS_ERR_INVALID; }
    if (!(g->slack >= 0) || !std::isfinite(g->slack)) { set_error("segment gate params: slack %g is not finite or below 0", (double)g->slack); return STOCS_ERR_INVALID; }
    if (!(g->min_ratio >= 0 && g->min_ratio <= 1)) { set_error("segment gate params: min_ratio %g outside [0, 1]", (double)g->min_ratio); return STOCS_ERR_INVALID; }
    if (g->min_used < 1) { set_error("segment gate params: min_used %d < 1", g->min_used); return STOCS_ERR_INVALID; }
    if (g->reserved != 0) { set_error("segment gate params: reserved %d is not 0", g->reserved); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}

int stocs_segment_gate(const stocs_segment_shape* shapes, int n_labels, const stocs_object_size* objects, int n_objects, const stocs_segment_gate_params* params, uint8_t* reasons) {
    const char* who = "stocs_segment_gate";
    if (n_labels < 0 || n_objects < 0) { set_error("%s: n_labels %d, n_objects %d", who, n_labels, n_objects); return STOCS_ERR_INVALID; }
    if ((n_labels > 0 && !shapes) || (n_objects > 0 && !objects) || (n_labels > 0 && n_objects > 0 && !reasons)) { set_error("%s: NULL shapes, objects or reasons", who); return STOCS_ERR_INVALID; }
    stocs_segment_gate_params g;
    int rc;
    if ((rc = gate_params_or_defaults(params, &g)) || (rc = check_objects(who, objects, n_objects))) return rc;
    for (int o = 0; o < n_objects; ++o)
        for (int l = 0; l < n_labels; ++l) reasons[(size_t)o * n_labels + l] = (uint8_t)segment_gate_reasons(shapes[l], objects[o], g);
    return STOCS_OK;
}

int stocs_segment_assign(const stocs_camera* cam, const uint16_t* depth, const int32_t* labels, int n_labels, float max_depth, const stocs_object_size* objects, int n_objects,
                         const stocs_segment_gate_params* gate_params, int device, stocs_segment_shape* shapes, int64_t* moments, uint8_t* reasons, uint16_t* class_stack,
                         stocs_segment_shapes_result* result) {
    return assign_checked("stocs_segment_assign", cam, depth, labels, n_labels, max_depth, objects, n_objects, gate_params, device, shapes, moments, reasons, class_stack, result);
}

int stocs_segment_shapes(const stocs_camera* cam, const uint16_t* depth, const int32_t* labels, int n_labels, float max_depth, int device, stocs_segment_shape* shapes,
                         int64_t* moments, stocs_segment_shapes_result* result) {
    return assign_checked("stocs_segment_shapes", cam, depth, labels, n_labels, max_depth, NULL, 0, NULL, device, shapes, moments, NULL, NULL, result);
}

int stocs_points_shape(const float* pos3, int n, int device, stocs_segment_shape* shape, int64_t* moments10) {
    const char* who = "stocs_points_shape";
    if (!shape || (n > 0 && !pos3)) { set_error("%s: NULL points or shape", who); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return STOCS_ERR_INVALID; }
    if (n > SEG_MAX_PIX) { set_error("%s: %d points, above 2^22 (the moments are 64-bit sums)", who, n); return STOCS_ERR_CAPACITY; }
    static const float none[3] = {0.0f, 0.0f, 0.0f};
    const ShpCall c = {who, NULL, NULL, NULL, 0.0f, pos3 ? pos3 : none, n, 1, NULL, 0, {0, 0, 0, 0}, device, shape, moments10, NULL, NULL, NULL};
    return shapes_run(c);
}

int stocs_segment_shapes_table(int* slots) {
    if (slots) *slots = SHP_SLOTS;
    return STOCS_OK;
}

int stocs_segment_shapes_last_device_ms(float* shapes_ms) {
    if (!tl_shp_clock.valid) { set_error("stocs_segment_shapes_last_device_ms: no shapes call of this thread ran with STOCS_SEGMENT_CLOCK=1"); return STOCS_ERR_STATE; }
    if (shapes_ms) *shapes_ms = tl_shp_clock.ms;
    return STOCS_OK;
}

}  // extern "C"
