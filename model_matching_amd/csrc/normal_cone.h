// normal_cone.h -- the per-cell normal cone of the scene grid: its packing in the cell word, its decoding, and the test
// "can a scene normal of this cell pass the 30-degree test against this rotated model normal at all".
// Shared by the grid build (grid.hip: the half-angle is measured against the axis AS DECODED HERE), the queue kernel's gate and
// the counting kernel of stocs_lcp_gate_count (lcp.hip), host and device.
//
// Packing.  The count word (y) of a cell word keeps the list length in its low 16 bits (a list holds at most 65 535 entries: the
// grid build refuses longer ones), so every reader masks with the CONSTANT STOCS_CONE_COUNT_MASK and no grid is too crowded for
// cones.  Above the count:
//   bits 16..21, 22..27   the axis, octahedral, 6 bits per coordinate (the decoded axis is within ~2 degrees of the mean normal)
//   bits 28..31           the half-angle class k: sin(half-angle) <= k / 16, k = 1..15; 0 = no cone ("no gate": half-angles
//                         of 69.6 degrees and more, normals that are not finite or not of unit length within 1e-4, no axis)
// An empty cell is an all-zero word, as before; a grid built without cones (SceneGrid::has_cones false) has class 0 everywhere.
// (8 + 8 + 6 bits above a 10-bit count would describe the cones ~3 degrees tighter, but the count mask would then depend on the
// grid -- one more uniform value in kernels that have no scalar register to spare, and ungated forms that no longer match the
// code they had before the cones.)
//
// The test.  v = A n_m is the rotated model normal exactly as the normal test computes it (any length: A need not be rigid),
// o the decoded axis (not normalised), delta the half-angle of the class.  Every scene normal n_s of the cell's list has
// angle(n_s, o) <= delta and | |n_s| - 1 | <= 1e-4, so with theta = angle(v, o) > delta
//     v . n_s  <=  |n_s| |v| cos(theta - delta)  =  |n_s| (va cos(delta) + vp sin(delta)),    va = v.o / |o|,  vp = sqrt(|v|^2 - va^2)
// (for a negative right-hand side the factor |n_s| only helps).  theta <= delta is never ruled out.  The lane is ruled out when
//     bound (1 + 1e-4) + m < dot_lo,        bound = va cos(delta) + vp sin(delta),   m = 2e-3 (|vx| + |vy| + |vz|).
// The margin m.  With u = 2^-24:
//   * the kernel's own dot product d = sn.x*nx + (sn.y*ny + sn.z*nz) carries three roundings on terms whose absolute values
//     sum to at most |n_s| |v|: |d - v.n_s| <= 3 u (1 + 1e-4) |v| < 1.8e-7 |v|;
//   * va: the dot product v.o within 3 u |v| |o|, 1/|o| within 4 u (sum of squares, reciprocal square root to an ulp), one
//     product: within 8 u |v|;
//   * vp: |v|^2 within 3 u |v|^2, va^2 within 16 u |v|^2, one rounding more: the radicand within 20 u |v|^2, and
//     |sqrt(x + e) - sqrt(x)| <= sqrt(|e|): vp within sqrt(20 u) |v| < 1.1e-3 |v|, the worst case (vp near zero) included;
//   * sin(delta) = k / 16 is exact, 1 - sin^2 is exact (8 bits), its root and the two operations of `bound` add < 4 u |v|.
// Together less than 1.11e-3 |v| <= 2e-3 |v|_1.  (Underflow adds absolute errors around 1e-38, nothing against dot_lo = 0.866: a
// counted query has |v| >= 0.86.)  What the margin costs: a cone is treated as 0.2 degrees wider than it is.
// NaN and infinity: every comparison below is false for a NaN, and an infinite v makes `bound` + m NaN or +inf: not ruled out.
#ifndef STOCS_NORMAL_CONE_H
#define STOCS_NORMAL_CONE_H

#include "stocs_math.h"

namespace stocs {

#define STOCS_CONE_COUNT_MASK 0xFFFFu
#define STOCS_CONE_MAX_CLASS 15u
#define STOCS_CONE_AXIS_MAX 63u     /* largest value of an axis coordinate's field */
#define STOCS_CONE_SIN_STEPS 16.0f  /* classes per unit of sin(half-angle) */

#if defined(__HIP_DEVICE_COMPILE__)
#define STOCS_NC_FMAF(a, b, c) __fmaf_rn((a), (b), (c))
#define STOCS_NC_SQRTF(a) __builtin_amdgcn_sqrtf(a)
#define STOCS_NC_RSQRTF(a) __builtin_amdgcn_rsqf(a)
#else
#define STOCS_NC_FMAF(a, b, c) fmaf((a), (b), (c))
#define STOCS_NC_SQRTF(a) sqrtf(a)
#define STOCS_NC_RSQRTF(a) (1.0f / sqrtf(a))
#endif

STOCS_HD uint32_t cone_pack(uint32_t u8, uint32_t v8, uint32_t cls) { return (u8 << 16) | (v8 << 22) | (cls << 28); }
STOCS_HD uint32_t cone_class(uint32_t y) { return y >> 28; }

// the axis of the cone in the count word y: exact float operations only (the same triple on host and device), |o|_1 = 1
STOCS_HD void cone_axis(uint32_t yw, float& ox, float& oy, float& oz) {
    float x = STOCS_NC_FMAF((float)((yw >> 16) & 63u), 2.0f / 63.0f, -1.0f);
    float y0 = STOCS_NC_FMAF((float)((yw >> 22) & 63u), 2.0f / 63.0f, -1.0f);
    const float z = (1.0f - fabsf(x)) - fabsf(y0);
    const float t = fmaxf(-z, 0.0f);   // the lower half of the octahedron is folded over the diagonals
    x += x >= 0.0f ? -t : t;
    y0 += y0 >= 0.0f ? -t : t;
    ox = x; oy = y0; oz = z;
}

// true: no scene normal inside the cone of y reaches dot_lo against v (see the derivation above); false also for y without a cone
STOCS_HD bool cone_rules_out(uint32_t y, float vx, float vy, float vz, float dot_lo) {
    float ox, oy, oz;
    cone_axis(y, ox, oy, oz);
    const float S = STOCS_NC_FMAF(ox, ox, STOCS_NC_FMAF(oy, oy, oz * oz));
    const float W = STOCS_NC_FMAF(vx, ox, STOCS_NC_FMAF(vy, oy, vz * oz));
    const float vv = STOCS_NC_FMAF(vx, vx, STOCS_NC_FMAF(vy, vy, vz * vz));
    const float va = W * STOCS_NC_RSQRTF(S);
    const float vp = STOCS_NC_SQRTF(fmaxf(STOCS_NC_FMAF(-va, va, vv), 0.0f));
    const float sd = (float)cone_class(y) * (1.0f / STOCS_CONE_SIN_STEPS);
    const float cd = STOCS_NC_SQRTF(STOCS_NC_FMAF(-sd, sd, 1.0f));
    const float bound = STOCS_NC_FMAF(va, cd, vp * sd);
    const float l1 = fabsf(vx) + (fabsf(vy) + fabsf(vz));
    const bool outside = vp * cd > va * sd;   // theta > delta (tan theta > tan delta, or va < 0)
    return cone_class(y) != 0u && outside && STOCS_NC_FMAF(bound, 1.0001f, 2.0e-3f * l1) < dot_lo;
}

}  // namespace stocs
#endif
