// wave_bits.h -- the wavefront reductions and bit helpers that several files share: the sum, minimum and maximum of an int over a
// wavefront by shuffles (depth.hip and render.hip: bounds of projected pixels; the bitset walks: counts), and the popcount of e & ~c
// over four words (cover_walk.h).
#ifndef STOCS_WAVE_BITS_H
#define STOCS_WAVE_BITS_H

#include <hip/hip_runtime.h>

namespace stocs {

__device__ __forceinline__ int wave_sum_i(int v) {
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
__device__ __forceinline__ int popc_andnot4(const uint4 e, const uint4 c) {
    return __popc(e.x & ~c.x) + __popc(e.y & ~c.y) + __popc(e.z & ~c.z) + __popc(e.w & ~c.w);
}

}  // namespace stocs

#endif
