// patch_normals.h -- the normal-cone test on the 16-point sub-patches of the shared-list forms of the queue kernel ("lcp_patch_normals"):
// a sub-patch that the sphere test leaves alive is still dead when no scene normal near it can pass the normal test against any of its
// rotated model normals.  The records of both sides, their packing, and the test; shared by the model set-up (ctx.hip), the field build
// (grid.hip: the half-angle is measured against the axis AS DECODED HERE), the prologue of lcp_coopq_kernel's SHARED forms, the counting
// kernel of stocs_lcp_patch_normal_count (lcp.hip) and the host (tests/test_patch_normals_cpu.py through stocs_patch_normal_bound_host).
//
// Model side: one float4 per sub-patch BEHIND the sub-patch spheres (d_msub[4 * steps + q]): a unit axis a (float) and, in w, sb >=
// sin(beta), beta = the largest angle of a member normal against the stored float axis, measured in double and rounded outwards.  w < 0
// (STOCS_PN_NO_TEST): no test -- beta above 45 degrees, a normal that is not finite or not of unit length within 1e-6, the padding.
//
// Scene side: one 32-bit word per cell of the patch test's distance field (SceneGrid::d_dist), behind it in the same block of memory:
//   bits 0..11, 12..23   the axis, octahedral, 12 bits per coordinate
//   bits 24..31          the class k: every scene point within the field's REACH of the cell's centre has a normal n_s with
//                        | |n_s| - 1 | <= 1e-4 and sin(angle(n_s, axis)) <= k / 256, the angle below 90 degrees; k = 1 .. 240.
//                        0: no cone (no point within reach, or not yet built); 241..255: no cone (wider than 69.6 degrees, a normal
//                        that is not finite or not of unit length, no axis)
// The reach R follows the model (prepare_cull_field): the radius that 80 % of the sub-patches stay below + epsilon + half a cell
// diagonal (tools/patch_normal_census.py: 18.5 mm at Cm; a fixed 20 mm could test 2 % of `small`'s sub-patches).  The radius term is
// clamped at STOCS_PN_MAX_REACH_EPS = 4 epsilon (`small` sits at 3.9), so R <= 5.9 cells whatever the model: the fill visits
// (2 ceil(R / g) + 1)^3 cells per scene point, and a model that is sparse against epsilon (sub-patches of 10 to 20 epsilon) would
// otherwise pay tens of milliseconds for cones too wide to rule anything out.  Its sub-patches are beyond the reach: not tested.
//
// The test.  A sub-patch with sphere (c, r) and cone (a, beta) under x -> A x + t; s >= |A|_2 (linear_norm_bound); the cell of
// c' = A c + t, e = |c' - cell centre|.  A model point x of it lands within s r of c', a scene point p that it can be counted with is
// within epsilon of A x + t, hence within s r + epsilon + e of the cell's centre.  When that -- `need`, the sphere test's own value with
// its own rounding margins, plus e -- is at most the reach as the kernel is given it (the radius the build used, shortened by more than
// the build's rounding: pn_reach_for_kernel), p is one of the points the cell's cone was built from.
// A member normal is n_m = |n_m| (cos(phi) a + sin(phi) b), phi <= beta, b a unit vector orthogonal to a, so for every such n_s
//     (A n_m) . n_s = |n_m| (cos(phi) (A a) . n_s + sin(phi) (A b) . n_s) <= |n_m| (cos(phi) X + sin(phi) S),
//     X = the support of the scene cone at v = A a (the `bound` of cone_rules_out, normal_cone.h), S = s (1 + 1e-4) >= |A b| |n_s|.
// X <= |v| (1 + 1e-4) <= S, so X cos(phi) + S sin(phi) = hypot(X, S) cos(phi - psi) with psi = atan2(S, X) >= 45 degrees: it grows with
// phi on [0, 45 degrees], and is at most X cos(beta') + S sin(beta') for every beta' in [beta, 45 degrees] -- for ANY matrix, rigid or
// not.  The sub-patch is ruled out when, in float,
//     (X (1 + 1e-4) + m) cb + s (sb (1 + 2e-4) + 2e-5) < dot_lo,    X = va cd + vp sd,  m = 2e-3 |v|_1,  cb = sqrt(1 - sb^2)
// and v lies outside the scene cone.  Margins: X (1 + 1e-4) + m is normal_cone.h's bound with its own margin (the float evaluation of
// va, vp and X within 1.11e-3 |v| of the truth, |n_s| <= 1 + 1e-4; a negative X leaves 0.9e-3 |v| of m over for the 2e-4 |v| that
// 1 - 1e-4 <= |n_s| takes); cb is within 3 u of its value and multiplies a quantity of at most 1.0025 |v|_1 <= 1.74 s: below 4e-7 s;
// |n_m| <= 1 + 1e-6 (ctx.hip flags the rest) on a left-hand side of at most 2.5 s: 2.5e-6 s; the kernel's own dot product, on
// vt = fl(A n_m) and the float normal test, rounds within 6.3e-7 s + 1.8e-7 |vt| (normal_cone.h): below 1e-6 s.  Together below 4e-6 s
// <= 2e-5 s.  sd = k / 256 and 1 - sd^2 are exact.  A NaN or infinite matrix makes s NaN or infinite and the comparison false: nothing
// is ruled out; a NaN axis or sb likewise.
#ifndef STOCS_PATCH_NORMALS_H
#define STOCS_PATCH_NORMALS_H

#include "normal_cone.h"

namespace stocs {

#define STOCS_PN_NO_TEST (-1.0f)
#define STOCS_PN_MAX_SIN_BETA 0.70710677f   /* fl(sin 45 degrees), rounded downwards */
#define STOCS_PN_MAX_CLASS 240u
#define STOCS_PN_BAD_CLASS 255u
#define STOCS_PN_SIN_STEPS 256.0f
#define STOCS_PN_AXIS_MAX 4095u
#define STOCS_PN_MAX_MODEL 8192             /* the shared-list forms' largest model: no field for a larger one */
#define STOCS_PN_REACH_QUANTILE 0.8
#define STOCS_PN_MAX_REACH_EPS 4.0          /* the radius term of the reach is at most this many epsilon (the fill costs reach^3) */

STOCS_HD uint32_t pn_pack(uint32_t u12, uint32_t v12, uint32_t cls) { return u12 | (v12 << 12) | (cls << 24); }
STOCS_HD uint32_t pn_class(uint32_t w) { return w >> 24; }

// the axis of the cone in a field word: the same float triple on host and device (one fused operation per coordinate), |o|_1 = 1
STOCS_HD void pn_axis(uint32_t w, float& ox, float& oy, float& oz) {
    float x = STOCS_NC_FMAF((float)(w & 4095u), 2.0f / 4095.0f, -1.0f);
    float y0 = STOCS_NC_FMAF((float)((w >> 12) & 4095u), 2.0f / 4095.0f, -1.0f);
    const float z = (1.0f - fabsf(x)) - fabsf(y0);
    const float t = fmaxf(-z, 0.0f);
    x += x >= 0.0f ? -t : t;
    y0 += y0 >= 0.0f ? -t : t;
    ox = x; oy = y0; oz = z;
}

// the reach the kernel may rely on when the build took every point whose float distance from the centre was below rb
inline float pn_reach_for_kernel(float rb) { return (float)fmax((double)rb * (1.0 - 2.0e-6) - 1.0e-6, 0.0); }

// the left-hand side of the test for the rotated axis v = A a, the model record's sb, the field word w (class 1 .. 240) and s;
// *outside: v lies outside the scene cone (only then may the caller rule out)
STOCS_HD float pn_bound(uint32_t w, float vx, float vy, float vz, float sb, float s, bool* outside) {
    float ox, oy, oz;
    pn_axis(w, ox, oy, oz);
    const float S = STOCS_NC_FMAF(ox, ox, STOCS_NC_FMAF(oy, oy, oz * oz));
    const float W = STOCS_NC_FMAF(vx, ox, STOCS_NC_FMAF(vy, oy, vz * oz));
    const float vv = STOCS_NC_FMAF(vx, vx, STOCS_NC_FMAF(vy, vy, vz * vz));
    const float va = W * STOCS_NC_RSQRTF(S);
    const float vp = STOCS_NC_SQRTF(fmaxf(STOCS_NC_FMAF(-va, va, vv), 0.0f));
    const float sd = (float)pn_class(w) * (1.0f / STOCS_PN_SIN_STEPS);
    const float cd = STOCS_NC_SQRTF(STOCS_NC_FMAF(-sd, sd, 1.0f));
    const float X = STOCS_NC_FMAF(va, cd, vp * sd);
    const float l1 = fabsf(vx) + (fabsf(vy) + fabsf(vz));
    const float cb = STOCS_NC_SQRTF(fmaxf(STOCS_NC_FMAF(-sb, sb, 1.0f), 0.0f));
    *outside = vp * cd > va * sd;
    return STOCS_NC_FMAF(STOCS_NC_FMAF(X, 1.0001f, 2.0e-3f * l1), cb, s * STOCS_NC_FMAF(sb, 1.0002f, 2.0e-5f));
}

// true: no point of the sub-patch with normal record (ax, ay, az, sb) can be counted under the linear part t0 .. t10 (column-major) of
// norm bound s, given the word w of a cell whose reach holds every scene point the sub-patch can be counted with (the caller's test)
STOCS_HD bool pn_rules_out(uint32_t w, float ax, float ay, float az, float sb, float s, float t0, float t1, float t2, float t4, float t5, float t6,
                           float t8, float t9, float t10, float dot_lo) {
    const float vx = t0 * ax + (t4 * ay + t8 * az);
    const float vy = t1 * ax + (t5 * ay + t9 * az);
    const float vz = t2 * ax + (t6 * ay + t10 * az);
    bool outside;
    const float b = pn_bound(w, vx, vy, vz, sb, s, &outside);
    const uint32_t k = pn_class(w);
    return k - 1u < STOCS_PN_MAX_CLASS && sb >= 0.0f && sb <= STOCS_PN_MAX_SIN_BETA && outside && b < dot_lo;
}

}  // namespace stocs
#endif
