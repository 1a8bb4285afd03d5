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
//
// The packed model normal.  The gate of the queue kernel does not read the exact model normal: the fourth word of a sorted model
// position (d_mpos_s[i].w, ctx.hip) carries the normal in 32 bits and arrives with the position.
//   bits 0..9, 10..19, 20..29   k = round(511 n) per component, clamped to +-511, two's complement
//   bit 30                      zero
//   bit 31                      "no gate for this point": the normal is not finite, or its length is not within 1e-3 of 1 after the
//                               loader's normalisation; such a point is never ruled out (the components are then zero)
// The padding records behind the model keep the word 0.  model_normal_unpack returns the components UNSCALED, the integers k as
// floats: cone_rules_out is homogeneous of degree one in v (bound, m and every rounding term above scale with v), so the factor
// 511 is folded into the threshold and the kernel pays no multiplication for it.
// The margin.  n~ = k / 511, Q = max_i |n~_i - n_i|_2 over the points without the flag: each component is within 0.5 / 511, so
// Q <= sqrt(3) / 1022 < 1.6948e-3 <= STOCS_MODEL_NORMAL_Q = 1.7e-3 (stocs_ctx_create measures Q in double and refuses a model that
// exceeds the constant).  Let f(v) = max { v . n_s : angle(n_s, o) <= delta, | |n_s| - 1 | <= 1e-4 } be the support function of the
// cell's cone: a maximum of linear functions of norm <= 1 + 1e-4, hence (1 + 1e-4)-Lipschitz in v.  The normal test works on
// vt = fl(A n), the gate on vg = fl(A k), v' = vg / 511.  With s >= |A|_2 (linear_norm_bound, stocs_math.h: the square root of the largest
// absolute row sum of A^T A, times 1.00001):
//   * |A n - A n~| <= s Q;
//   * each of the two float products carries three roundings per component on terms that sum to at most (|A| |n|)_i, and
//     | |A| |_2 <= |A|_F <= sqrt(3) |A|_2: |vt - A n| + |v' - A n~| <= 2 * 3 u sqrt(3) * 1.001 s < 6.3e-7 s;
//   * the kernel's dot product on vt rounds within 1.8e-7 |vt| <= 1.8e-7 (|v'| + s (Q + 6.3e-7)); the |v'| part is in m(v') already,
//     the rest is below 4e-10 s.
// So every scene normal of the cell gives, in the kernel's own float expression,
//     d <= f(vt) + 1.8e-7 |vt| <= f(v') + 1.8e-7 |v'| + (1 + 1e-4) s (Q + 6.3e-7) + 4e-10 s <= [bound(v') (1 + 1e-4) + m(v')] + s K,
//     K = STOCS_MODEL_NORMAL_SLACK = Q (1 + 1e-4) + 1e-6,
// and the lane is ruled out when bound(v') (1 + 1e-4) + m(v') < dot_lo - s K; times 511, on the unscaled vg:
//     bound(vg) (1 + 1e-4) + m(vg) < 511 (dot_lo - s K) = the threshold of model_normal_gate_threshold,
// ONE wave-uniform value computed before the walk and rounded downwards (five float roundings, taken off again as 4e-7 of the
// magnitudes).  A threshold that is negative (s > 500: no rigid pose) stays sound: for a negative bound the derivation above uses
// |n_s| >= 1 - 1e-4 where the code multiplies by 1 + 1e-4, a difference of 2e-4 |v| that the slack of m (2e-3 |v|_1 against the
// 1.11e-3 |v| it has to cover) takes.  v' outside the cone while vt is inside it: f is Lipschitz everywhere, the inequality holds.
// A NaN or infinite matrix gives a NaN or infinite s, a threshold that is NaN or -inf, and a comparison that is false: nothing is
// ruled out, as with the exact normal.  (A matrix so small that the squares in s underflow, entries below 1e-19, gives an s that is too
// small by less than 1e-18: absolute errors of that size are nothing against dot_lo, as above.)  What the packed normal costs: the cones act as if 0.1 degrees wider once more.
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

// ---- the packed model normal (see above) ----
#define STOCS_MODEL_NORMAL_SCALE 511.0f
#define STOCS_MODEL_NORMAL_NO_GATE 0x80000000u
#define STOCS_MODEL_NORMAL_Q 1.7e-3f                                             /* >= |unpack(pack(n)) / 511 - n|_2 */
#define STOCS_MODEL_NORMAL_SLACK (STOCS_MODEL_NORMAL_Q * 1.0001f + 1.0e-6f)      /* K of the derivation */

STOCS_HD uint32_t model_normal_pack(float nx, float ny, float nz) {
    const float l2 = nx * nx + (ny * ny + nz * nz);
    // (a NaN or infinite component makes l2 NaN or infinite: both comparisons fail)
    if (!(l2 >= 0.999f * 0.999f && l2 <= 1.001f * 1.001f)) return STOCS_MODEL_NORMAL_NO_GATE;
    const float c[3] = {nx, ny, nz};
    uint32_t w = 0u;
    for (int j = 0; j < 3; ++j) {
        const float r = fminf(fmaxf(rintf(c[j] * STOCS_MODEL_NORMAL_SCALE), -STOCS_MODEL_NORMAL_SCALE), STOCS_MODEL_NORMAL_SCALE);
        w |= ((uint32_t)(int32_t)r & 0x3FFu) << (10 * j);
    }
    return w;
}
// the components as integers (k = 511 n, not scaled back); zeros for a word with the flag
STOCS_HD void model_normal_unpack(uint32_t w, float& x, float& y, float& z) {
    x = (float)((int32_t)(w << 22) >> 22);
    y = (float)((int32_t)(w << 12) >> 22);
    z = (float)((int32_t)(w << 2) >> 22);
}

// the gate's threshold for packed normals under a transform of norm bound s: 511 (dot_lo - s K), rounded downwards
STOCS_HD float model_normal_gate_threshold(float dot_lo, float s) {
    const float sk = s * STOCS_MODEL_NORMAL_SLACK;
    return STOCS_MODEL_NORMAL_SCALE * ((dot_lo - sk) - 4.0e-7f * (fabsf(dot_lo) + sk));
}

// the gate of the queue kernel on the packed normal pw of a model point: rotates the unscaled components exactly as the normal test
// rotates the exact normal, and asks cone_rules_out with the threshold above.  A point with the flag is never ruled out.
STOCS_HD bool cone_rules_out_packed(uint32_t y, uint32_t pw, float t0, float t1, float t2, float t4, float t5, float t6, float t8, float t9, float t10,
                                    float thr511) {
    float kx, ky, kz;
    model_normal_unpack(pw, kx, ky, kz);
    const float nx = t0 * kx + (t4 * ky + t8 * kz);
    const float ny = t1 * kx + (t5 * ky + t9 * kz);
    const float nz = t2 * kx + (t6 * ky + t10 * kz);
    return (int32_t)pw >= 0 && cone_rules_out(y, nx, ny, nz, thr511);
}

}  // namespace stocs
#endif
