// wave_bits.h -- the wavefront reductions and bit helpers that several files share: the sum, minimum and maximum of an int over a
// wavefront by shuffles (depth.hip and render.hip: bounds of projected pixels; the bitset walks: counts), the workgroup's tail that
// adds K per-wavefront counts into K device counters (segment.hip), and the popcount of e & ~c over four words (cover_walk.h).
#ifndef STOCS_WAVE_BITS_H
#define STOCS_WAVE_BITS_H

#include <hip/hip_runtime.h>

namespace stocs {

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the 64-bit sum (segment.hip, segment_shapes.hip: integer moments)
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}
// The counting tail of a workgroup of four wavefronts (segment.hip): acc[0 .. K) are a wavefront's own counts (ballot popcounts, the same
// in all its lanes).  Lane 0 of each wavefront leaves them in s_n[wave], and behind the barrier lane k < K adds the four and makes the one
// atomic of the workgroup on dst[k], none when the sum is 0.  Every lane of the workgroup must arrive.
template <int K>
__device__ __forceinline__ void wg_add_counts(const int* acc, int (*s_n)[K], int* dst) {
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < K; ++k) s_n[threadIdx.x >> 6][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < K) {
        const int t = (s_n[0][threadIdx.x] + s_n[1][threadIdx.x]) + (s_n[2][threadIdx.x] + s_n[3][threadIdx.x]);
        if (t) atomicAdd(dst + threadIdx.x, t);
    }
}
__device__ __forceinline__ int popc_andnot4(const uint4 e, const uint4 c) {
    return __popc(e.x & ~c.x) + __popc(e.y & ~c.y) + __popc(e.z & ~c.z) + __popc(e.w & ~c.w);
}

}  // namespace stocs

#endif
