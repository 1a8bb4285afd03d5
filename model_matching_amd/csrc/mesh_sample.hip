// mesh_sample.hip -- a triangle mesh sampled into an oriented point cloud (stocs_mesh_sample, stocs_preprocess_model_mesh): one sample per
// spacing^2 of area in expectation, whatever the triangle sizes, every normal the facet's.  No reference counterpart.  The contract (the
// float64 order of the count, the counter hashes, the float32 order of the position) is written down at the declarations in
// include/stocs_hip.h and mesh_sample.h; tests/mesh_sample_ref.py restates it in numpy, and counts, areas, positions, normals and indices are
// equal bit for bit.  The entry points live in ingest.hip, beside the workspace and the voxel grid they use; this file holds the kernels.
//   count    mesh_sample_count_kernel: one lane per triangle: the three 128-bit vertex gathers of mesh_render_kernel, the cross product, its
//            length and the area over spacing^2 in double, the dither from the triangle's key; writes the count, the facet normal (float) for
//            the sample pass and, when asked, the area; one atomic per wavefront that has something to report
//   scan     the library's exclusive scan (prims.h), 32-bit counts to 64-bit offsets, over nt + 1 entries: the last one is the total
//   sample   mesh_sample_kernel: one lane per sample k; its triangle is the last t with offs[t] <= k -- triangles without a sample repeat their
//            successor's offset and are stepped over by the search itself.  Two forms (mesh_sample_form below), equal bits:
//              global   every lane searches the whole array in global memory (at most 23 dependent loads that hit the L2): the default
//              window   lanes 0 and 64 of a workgroup search the whole array for the triangles of its first and last sample; one triangle
//                       (thousands of samples on a box's face): no search at all; a range of up to MESH_SAMPLE_WINDOW triangles: their offsets,
//                       relative to the workgroup's first sample, go into LDS and every lane searches there; a longer range (most triangles
//                       empty): every lane searches the range in global memory
//            Measured (profiles/mesh_sample_time.json): the window form wins on the 12-triangle box (17.4 against 20.5 us for 2.5
//            million samples) and loses wherever triangles are many (12.5 against 9.0 us on 409 600 triangles at a coarse spacing): its two
//            serial searches and the barrier stand in front of every lane's own.  Either way the kernel is a few per cent of the call.
//            then the triangle's three gathers, its normal, the hash of (seed, t, j), and three 128-bit (pos, nrm) / 32-bit (tri) stores per
//            lane at consecutive addresses.
#include <stdlib.h>

#include "mesh_sample.h"
#include "stocs_ctx.h"

namespace stocs {

enum { MESH_SAMPLE_WINDOW = 2048 };
enum { MESH_SAMPLE_FORM_GLOBAL = 1, MESH_SAMPLE_FORM_WINDOW = 2 };

__global__ __launch_bounds__(256) void mesh_sample_count_kernel(const float4* __restrict__ verts, const int4* __restrict__ tris, int nt, double h2, uint64_t seed,
                                                                uint32_t* __restrict__ counts, float4* __restrict__ tri_nrm, double* __restrict__ area,
                                                                uint32_t* __restrict__ flags) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    bool skip = false, over = false;
    if (t < nt) {
        const int4 id = tris[t];   // 0 <= id.x, id.y, id.z < nv: the entry points refuse anything else
        const float4 A = verts[id.x], B = verts[id.y], C = verts[id.z];
        const bool finite = isfinite(A.x) && isfinite(A.y) && isfinite(A.z) && isfinite(B.x) && isfinite(B.y) && isfinite(B.z) && isfinite(C.x) && isfinite(C.y) && isfinite(C.z);
        const double e1x = (double)B.x - (double)A.x, e1y = (double)B.y - (double)A.y, e1z = (double)B.z - (double)A.z;
        const double e2x = (double)C.x - (double)A.x, e2y = (double)C.y - (double)A.y, e2z = (double)C.z - (double)A.z;
        const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
        const double len = sqrt(cx * cx + (cy * cy + cz * cz));
        uint32_t n = 0;
        double a = 0.0;
        float4 nn = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!finite || !(len > 0.0)) {
            skip = true;
        } else {
            a = 0.5 * len;
            const double x = a / h2;
            if (x >= 4294967295.0) {
                over = true;
            } else {
                const double fl = floor(x);
                const double d = (double)mesh_dither24(mesh_tri_key(seed, (uint64_t)t)) * (1.0 / 16777216.0);
                n = (uint32_t)fl + (d < x - fl ? 1u : 0u);
            }
            nn = make_float4((float)(cx / len), (float)(cy / len), (float)(cz / len), 0.f);
        }
        counts[t] = n;
        if (tri_nrm) tri_nrm[t] = nn;
        if (area) area[t] = a;
    } else if (t == nt) {
        counts[nt] = 0u;
    }
    const unsigned long long sk = __ballot(skip), ov = __ballot(over);
    if ((threadIdx.x & 63) == 0) {
        if (sk) atomicAdd(&flags[MESH_SAMPLE_FLAG_SKIPPED], (uint32_t)__popcll(sk));
        if (ov) atomicOr(&flags[MESH_SAMPLE_FLAG_OVERFLOW], 1u);
    }
}

// the last t in [lo, hi] with offs[t] <= k; offs[lo] <= k
__device__ __forceinline__ int mesh_sample_tri_of(const unsigned long long* __restrict__ offs, int lo, int hi, unsigned long long k) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (offs[mid] <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void mesh_sample_kernel(const float4* __restrict__ verts, const int4* __restrict__ tris, int nt, const unsigned long long* __restrict__ offs,
                                                          const float4* __restrict__ tri_nrm, uint64_t seed, int orient, unsigned long long total, int form,
                                                          float4* __restrict__ pos, float4* __restrict__ nrm, int32_t* __restrict__ tri) {
    __shared__ uint32_t s_rel[MESH_SAMPLE_WINDOW];
    __shared__ int s_range[2];
    const int tid = (int)threadIdx.x;
    const unsigned long long k0 = (unsigned long long)blockIdx.x * 256ull;   // k0 < total: the grid is ceil(total / 256)
    const unsigned long long k_last = k0 + 255ull < total ? k0 + 255ull : total - 1ull;
    const unsigned long long k = k0 + (unsigned long long)tid, ks = k < total ? k : k_last;   // a lane past the end searches for the last sample
    int t;
    if (form == MESH_SAMPLE_FORM_GLOBAL) {
        t = mesh_sample_tri_of(offs, 0, nt - 1, ks);
    } else {
        if (tid == 0) s_range[0] = mesh_sample_tri_of(offs, 0, nt - 1, k0);
        if (tid == 64) s_range[1] = mesh_sample_tri_of(offs, 0, nt - 1, k_last);
        __syncthreads();
        const int t_lo = s_range[0], t_hi = s_range[1], m = t_hi - t_lo + 1;   // workgroup-uniform, as are the branches below
        if (m == 1) {
            t = t_lo;
        } else if (m <= (int)MESH_SAMPLE_WINDOW) {
            // offs[t_lo] <= k0 < offs[t_lo + i] <= k_last for 0 < i < m: the differences fit 8 bits
            for (int i = tid; i < m; i += 256) s_rel[i] = i == 0 ? 0u : (uint32_t)(offs[t_lo + i] - k0);
            __syncthreads();
            const uint32_t r = (uint32_t)(ks - k0);
            int lo = 0, hi = m - 1;
            while (lo < hi) {
                const int mid = lo + ((hi - lo + 1) >> 1);
                if (s_rel[mid] <= r) lo = mid; else hi = mid - 1;
            }
            t = t_lo + lo;
        } else {
            t = mesh_sample_tri_of(offs, t_lo, t_hi, ks);
        }
    }
    if (k >= total) return;   // behind the last barrier
    const unsigned long long j = k - offs[t];
    uint32_t iu, iv;
    mesh_sample_uv24(mesh_tri_key(seed, (uint64_t)t), j, &iu, &iv);
    const float u = (float)iu * (1.0f / 16777216.0f), v = (float)iv * (1.0f / 16777216.0f);   // exact
    const int4 id = tris[t];
    const float4 A = verts[id.x], B = verts[id.y], C = verts[id.z];
    const V3 p = mk3(A.x + (u * (B.x - A.x) + v * (C.x - A.x)), A.y + (u * (B.y - A.y) + v * (C.y - A.y)), A.z + (u * (B.z - A.z) + v * (C.z - A.z)));
    const float4 n4 = tri_nrm[t];
    V3 n = mk3(n4.x, n4.y, n4.z);
    if (orient == 1 && dot3(n, p) < 0.0f) n = -n;
    pos[k] = make_float4(p.x, p.y, p.z, 0.f);
    nrm[k] = make_float4(n.x, n.y, n.z, 0.f);
    if (tri) tri[k] = t;
}

// STOCS_MESH_SAMPLE_FORM=<n> in the environment forces the sample kernel's form, for measurements and for the tests; no value changes a
// result.  1: global, 2: window; anything else: the default, global.
static int mesh_sample_form() {
    const char* e = getenv("STOCS_MESH_SAMPLE_FORM");
    return e && atoi(e) == MESH_SAMPLE_FORM_WINDOW ? MESH_SAMPLE_FORM_WINDOW : MESH_SAMPLE_FORM_GLOBAL;
}

hipError_t mesh_sample_count_launch(const float4* verts, const int4* tris, int nt, double h, uint64_t seed, uint32_t* counts, float4* tri_nrm, double* area,
                                    uint32_t* flags, hipStream_t st) {
    hipLaunchKernelGGL(mesh_sample_count_kernel, dim3((unsigned)(((size_t)nt + 1 + 255) / 256)), dim3(256), 0, st, verts, tris, nt, h * h, seed, counts, tri_nrm, area, flags);
    return hipGetLastError();
}

hipError_t mesh_sample_launch(const float4* verts, const int4* tris, int nt, const unsigned long long* offs, const float4* tri_nrm, uint64_t seed, int orient,
                              long long total, float4* pos, float4* nrm, int32_t* tri, hipStream_t st) {
    hipLaunchKernelGGL(mesh_sample_kernel, dim3((unsigned)(((unsigned long long)total + 255ull) / 256ull)), dim3(256), 0, st, verts, tris, nt, offs, tri_nrm, seed,
                       orient, (unsigned long long)total, mesh_sample_form(), pos, nrm, tri);
    return hipGetLastError();
}

}  // namespace stocs
