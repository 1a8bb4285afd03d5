// pose_error_math.h -- the arithmetic that the pose-error kernels share (pose_error.hip: ADD / ADD-S; pose_error_sym.hip: MSSD / MSPD /
// symmetric ADD): steps 1, 2 and 4 of the contract at stocs_pose_errors in include/stocs_hip.h, step 5's validity rule on the device
// (its host twin is eval_call.h's pair_valid), and the wavefront reductions of the integer sums and of the float maxima taken on their bits.  One definition: the
// symmetry-aware records equal the plain ones bit for bit under the identity because both run these very expressions.
#ifndef STOCS_POSE_ERROR_MATH_H
#define STOCS_POSE_ERROR_MATH_H

#include <math.h>

#include "stocs_ctx.h"

namespace stocs {

// step 1: the depth check's expression
__device__ __forceinline__ float4 pe_transform(const float* P, const float4 m) {
    float4 r;
    r.x = (P[0] * m.x + (P[4] * m.y + P[8] * m.z)) + P[12];
    r.y = (P[1] * m.x + (P[5] * m.y + P[9] * m.z)) + P[13];
    r.z = (P[2] * m.x + (P[6] * m.y + P[10] * m.z)) + P[14];
    r.w = 0.0f;
    return r;
}
// step 2
__device__ __forceinline__ float pe_sqdist(const float4 p, const float4 g) {
    const float dx = p.x - g.x, dy = p.y - g.y, dz = p.z - g.z;
    return (dx * dx) + ((dy * dy) + (dz * dz));
}
// r(x): +inf for NaN, else the correctly rounded square root
__device__ __forceinline__ float pe_root(float d) { return d != d ? INFINITY : stocs_sqrtf(d); }
// q(x): 32.32 fixed point of min(x, 32768): the product with 2^32 is exact, the conversion truncates a non-negative value
__device__ __forceinline__ unsigned long long pe_fix(float x) { return (unsigned long long)(fminf(x, 32768.0f) * 4294967296.0f); }

__device__ __forceinline__ bool pe_pose_finite(const float* P) {
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 15; ++i)
        if ((i & 3) != 3) finite = finite && (fabsf(P[i]) <= 3.4028234663852886e38f);
    return finite;
}
__device__ __forceinline__ bool pe_pose_zero(const float* P) {
    bool zero = true;
#pragma unroll
    for (int i = 0; i < 16; ++i) zero = zero && (P[i] == 0.0f);
    return zero;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned w = (unsigned)__shfl_xor((int)v, o, 64); v = w > v ? w : v; }
    return v;
}

}  // namespace stocs

#endif
