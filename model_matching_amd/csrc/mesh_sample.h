// mesh_sample.h -- the sampling contract's integer half (the counter hashes and the reflected barycentrics), shared by the kernels of
// mesh_sample.hip and any host code, and the device-level entry points of mesh_sample.hip that the ingest layer (ingest.hip) drives out of
// its own workspace.  The contract is written down at stocs_mesh_sample in include/stocs_hip.h and restated in tests/mesh_sample_ref.py.
#ifndef STOCS_MESH_SAMPLE_H
#define STOCS_MESH_SAMPLE_H

#include "stocs_math.h"

namespace stocs {

// The key of triangle t under a seed: the first two stages of rng64(seed, t, .) (stocs_math.h), i.e.
//     key = mix64( mix64(seed + 0x9E3779B97F4A7C15) ^ (t * 0xD1B54A32D192ED03 + 0x8CB92BA72F3D8DD7) )       (all modulo 2^64)
STOCS_HD uint64_t mesh_tri_key(uint64_t seed, uint64_t t) {
    const uint64_t z = mix64(seed + 0x9E3779B97F4A7C15ull);
    return mix64(z ^ (t * 0xD1B54A32D192ED03ull + 0x8CB92BA72F3D8DD7ull));
}
// the dither d_t * 2^24: the key's top 24 bits
STOCS_HD uint32_t mesh_dither24(uint64_t key) { return (uint32_t)(key >> 40); }
// sample j of the triangle: w = mix64(key ^ ((j + 1) * 0xDB4F0B9175AE2165)) = rng64(seed, t, j); iu = w's top 24 bits, iv the 24 below
// them; iu + iv >= 2^24 reflects both (2^24 - 1 - i), so that iu + iv <= 2^24 - 1 always: u + v < 1
STOCS_HD void mesh_sample_uv24(uint64_t key, uint64_t j, uint32_t* iu, uint32_t* iv) {
    const uint64_t w = mix64(key ^ ((j + 1) * 0xDB4F0B9175AE2165ull));
    uint32_t a = (uint32_t)(w >> 40), b = (uint32_t)(w >> 16) & 0xFFFFFFu;
    if (a + b >= (1u << 24)) { a = 0xFFFFFFu - a; b = 0xFFFFFFu - b; }
    *iu = a; *iv = b;
}

#if defined(__HIPCC__)
enum { MESH_SAMPLE_FLAG_OVERFLOW = 0, MESH_SAMPLE_FLAG_SKIPPED = 1, MESH_SAMPLE_FLAG_WORDS = 2 };

// stocs_mesh_check's tests under the caller's name; finite_vertices == false leaves the vertex values unread (mesh.hip)
int mesh_check_as(const char* who, const float* pos3, int nv, const int32_t* tris3, int nt, bool finite_vertices);

// Count pass over nt triangles (verts: x, y, z, 0; tris: i0, i1, i2, 0, every index inside the vertices).  counts: nt + 1 words, counts[nt]
// = 0 closes the scan; tri_nrm (nt, or NULL): the unit normal of the winding, for the sample pass; area (nt doubles, or NULL): 0 for a skipped
// triangle; flags: MESH_SAMPLE_FLAG_WORDS words that the caller zeroed on the stream (a triangle with x >= 2^32 - 1 sets OVERFLOW and counts
// 0; SKIPPED counts the triangles with a non-finite corner or no area)
hipError_t mesh_sample_count_launch(const float4* verts, const int4* tris, int nt, double h, uint64_t seed, uint32_t* counts, float4* tri_nrm, double* area,
                                    uint32_t* flags, hipStream_t st);
// Sample pass: total > 0 samples, sample k on the last triangle t with offs[t] <= k (offs: the exclusive scan of counts, nt + 1 entries,
// offs[nt] = total).  pos, nrm: total float4 (w = 0); tri: total words or NULL.
hipError_t mesh_sample_launch(const float4* verts, const int4* tris, int nt, const unsigned long long* offs, const float4* tri_nrm, uint64_t seed, int orient,
                              long long total, float4* pos, float4* nrm, int32_t* tri, hipStream_t st);
#endif

}  // namespace stocs
#endif
