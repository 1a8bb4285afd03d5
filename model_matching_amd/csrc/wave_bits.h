// wave_bits.h -- the two device helpers the bitset walks share (instances.hip over scene points, scene.hip over pixels): the sum of an
// int over a wavefront, and the popcount of e & ~c over four words.
#ifndef STOCS_WAVE_BITS_H
#define STOCS_WAVE_BITS_H

#include <hip/hip_runtime.h>

namespace stocs {

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int popc_andnot4(const uint4 e, const uint4 c) {
    return __popc(e.x & ~c.x) + __popc(e.y & ~c.y) + __popc(e.z & ~c.z) + __popc(e.w & ~c.w);
}

}  // namespace stocs

#endif
