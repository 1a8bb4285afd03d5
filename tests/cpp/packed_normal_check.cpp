// packed_normal_check.cpp -- host check of the packed model normal and of the queue kernel's gate on it (csrc/normal_cone.h).
// Stand-alone: g++ only, no GPU, no library; may be built with -fsanitize=address,undefined.  Build with -ffp-contract=off (the
// project's numerics contract: the float expressions below are the kernel's own).
//   1. |unpack(pack(n)) / 511 - n|_2 <= STOCS_MODEL_NORMAL_Q over 1e6 random unit normals, the six axis directions, and normals with
//      a component exactly on a code value and exactly halfway between two codes;
//   2. zero, NaN, infinite and half-length normals get bit 31, bit 30 is never set, a flagged word is never ruled out;
//   3. soundness: random cone words of every class, random linear parts (rigid, scaled by 1e-3 and 1e3, sheared, mirrored), random
//      model normals -- half of them aimed within a degree of the angle at which the gate starts to rule out.  Whenever the gate on
//      the packed normal rules out, the kernel's dot product  sn.x*nx + (sn.y*ny + sn.z*nz)  on the EXACT rotated normal is below
//      dot_lo for scene normals inside the cone: its boundary towards v at lengths 1 - 1e-4, 1, 1 + 1e-4, the axis, the boundary at
//      other azimuths and the interior.  At least a fifth of the trials must be ruled out by the exact-normal gate and by the packed
//      one, so that a dead gate cannot pass; a matrix that is not finite rules nothing out.
//   4. the margin of the packed normal itself.  The margin m of cone_rules_out has room to spare (2e-3 |v|_1 against a proven
//      1.11e-3 |v|, and far less on a host), so the samples of 3 would also pass with the term s K missing.  The two inequalities of
//      the derivation in normal_cone.h are therefore asserted as they stand, in double, with f the support function of the cone
//      (lengths 1 +- 1e-4 included), vt the float rotation of the exact normal and v' = vg / 511 the float rotation of the codes:
//        A (every trial)           f(vt) + 1.8e-7 |vt|  <=  f(v') + 1.8e-7 |v'| + s K
//        B (packed gate rules out) bound(v') (1 + 1e-4) + 2e-3 |v'|_1 - 1.12e-3 (1 + 1e-4) |v'|  <  dot_lo - s K
//      A fails for a K that is smaller than the quantisation moves v (K = 0: half of the trials; K = Q / 2: a few per cent); B lets
//      the float evaluation err by its proven rounding and no more, and fails when the threshold does not carry the whole s K.
// Prints its counts; exit status 0 when every check holds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>

#include "../../model_matching_amd/csrc/normal_cone.h"

using namespace stocs;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

static double pack_error(float x, float y, float z, uint32_t* word) {
    const uint32_t w = model_normal_pack(x, y, z);
    *word = w;
    float kx, ky, kz;
    model_normal_unpack(w, kx, ky, kz);
    const double dx = (double)kx / 511.0 - (double)x, dy = (double)ky / 511.0 - (double)y, dz = (double)kz / 511.0 - (double)z;
    return sqrt(dx * dx + dy * dy + dz * dz);
}

struct D3 { double x, y, z; };
static D3 d3(double x, double y, double z) { D3 r = {x, y, z}; return r; }
static double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static D3 dscale(D3 a, double s) { return d3(a.x * s, a.y * s, a.z * s); }
static D3 dadd(D3 a, D3 b) { return d3(a.x + b.x, a.y + b.y, a.z + b.z); }
static D3 dcross(D3 a, D3 b) { return d3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static D3 dunit(D3 a) { return dscale(a, 1.0 / sqrt(ddot(a, a))); }
// a unit vector perpendicular to the unit vector a
static D3 dperp(D3 a) { return dunit(dcross(a, fabs(a.x) < 0.6 ? d3(1, 0, 0) : d3(0, 1, 0))); }

static double dnorm(D3 a) { return sqrt(ddot(a, a)); }
// the angle between v and the unit axis o
static double angle_to(D3 v, D3 o) { return atan2(dnorm(dcross(v, o)), ddot(v, o)); }
// `bound` of normal_cone.h in double: |v| cos(theta - delta) (theta <= delta, which the gate never rules out: |v|)
static double cone_bound(D3 v, D3 o, double delta) { return dnorm(v) * cos(fmax(angle_to(v, o) - delta, 0.0)); }
// f of normal_cone.h: the support function of { n_s : angle(n_s, o) <= delta, | |n_s| - 1 | <= 1e-4 }; without a cone, of every such n_s
static double cone_support(D3 v, D3 o, double delta, bool has_cone) {
    const double c = has_cone ? cone_bound(v, o, delta) : dnorm(v);
    return c >= 0.0 ? c * (1.0 + 1.0e-4) : c * (1.0 - 1.0e-4);
}

typedef std::mt19937_64 Rng;
static double uni(Rng& g, double lo, double hi) { return lo + (hi - lo) * ((double)(g() >> 11) * (1.0 / 9007199254740992.0)); }
static D3 random_unit(Rng& g) {
    for (;;) {
        const D3 v = d3(uni(g, -1, 1), uni(g, -1, 1), uni(g, -1, 1));
        const double l = ddot(v, v);
        if (l > 1e-4 && l <= 1.0) return dscale(v, 1.0 / sqrt(l));
    }
}
// the loader's normalisation (stocs_math.h normalized3), in float
static V3 f_unit(D3 v) { return normalized3(mk3((float)v.x, (float)v.y, (float)v.z)); }

// a rotation matrix, rows r[0..2]
static void random_rotation(Rng& g, double r[3][3]) {
    const D3 a = random_unit(g), b0 = dperp(a);
    const double phi = uni(g, 0.0, 6.283185307179586);
    const D3 b = dadd(dscale(b0, cos(phi)), dscale(dcross(a, b0), sin(phi))), c = dcross(a, b);
    r[0][0] = a.x; r[0][1] = a.y; r[0][2] = a.z; r[1][0] = b.x; r[1][1] = b.y; r[1][2] = b.z; r[2][0] = c.x; r[2][1] = c.y; r[2][2] = c.z;
}

static void check_pack_error() {
    Rng g(12345);
    double worst = 0.0;
    uint32_t w;
    for (int i = 0; i < 1000000; ++i) {
        const V3 n = f_unit(random_unit(g));
        const double e = pack_error(n.x, n.y, n.z, &w);
        worst = fmax(worst, e);
        CHECK(e <= (double)STOCS_MODEL_NORMAL_Q, "random normal %d: error %.6g", i, e);
        CHECK((w & 0xC0000000u) == 0u, "random normal %d: word %08x has a high bit", i, w);
    }
    for (int ax = 0; ax < 3; ++ax)
        for (int sg = -1; sg <= 1; sg += 2) {
            const float c[3] = {ax == 0 ? (float)sg : 0.f, ax == 1 ? (float)sg : 0.f, ax == 2 ? (float)sg : 0.f};
            const double e = pack_error(c[0], c[1], c[2], &w);
            CHECK(e == 0.0 && (w & 0xC0000000u) == 0u, "axis %d sign %d: error %.6g word %08x", ax, sg, e, w);
            float kx, ky, kz;
            model_normal_unpack(w, kx, ky, kz);
            CHECK(kx == 511.f * c[0] && ky == 511.f * c[1] && kz == 511.f * c[2], "axis %d sign %d unpacks to %g %g %g", ax, sg, kx, ky, kz);
        }
    // one component on a code value k / 511 or halfway between two, (k + 0.5) / 511, the other two completing it to unit length
    for (int k = -511; k <= 511; ++k)
        for (int half = 0; half < 2; ++half)
            for (int ax = 0; ax < 3; ++ax) {
                const double cv = ((double)k + 0.5 * half) / 511.0;
                if (fabs(cv) > 1.0) continue;
                const double rest = sqrt(fmax(1.0 - cv * cv, 0.0)), phi = uni(g, 0.0, 6.283185307179586);
                double c[3];
                c[ax] = cv; c[(ax + 1) % 3] = rest * cos(phi); c[(ax + 2) % 3] = rest * sin(phi);
                // (not renormalised in float: the component has to stay on its value; the length is 1 within 2e-7)
                const double e = pack_error((float)c[0], (float)c[1], (float)c[2], &w);
                worst = fmax(worst, e);
                CHECK(e <= (double)STOCS_MODEL_NORMAL_Q && (w & 0xC0000000u) == 0u, "code value %d (+%d/2) axis %d: error %.6g word %08x", k, half, ax, e, w);
            }
    printf("pack: worst |unpack(pack(n)) / 511 - n| = %.6g (bound %.6g)\n", worst, (double)STOCS_MODEL_NORMAL_Q);
    CHECK(worst > 1.0e-3, "the worst error %.6g is implausibly small: nothing was measured", worst);
}

static void check_flags() {
    const float inf = INFINITY, nan = NAN;
    const float bad[][3] = {{0.f, 0.f, 0.f}, {nan, 0.f, 1.f}, {0.f, nan, 0.f}, {nan, nan, nan}, {inf, 0.f, 0.f}, {0.f, -inf, 0.f}, {0.f, 0.f, 0.5f},
                            {0.3f, 0.3f, 0.264575f}, {0.f, 2.f, 0.f}, {0.998f, 0.f, 0.f}, {0.f, 0.f, -1.002f}, {3e38f, 3e38f, 0.f}, {1e-30f, 0.f, 0.f}};
    const float idt[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (size_t i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
        const uint32_t w = model_normal_pack(bad[i][0], bad[i][1], bad[i][2]);
        CHECK((w & STOCS_MODEL_NORMAL_NO_GATE) != 0u && (w & 0x40000000u) == 0u, "bad normal %zu: word %08x", i, w);
        // never ruled out, whatever the cell's cone: every class, axis +z and -z, a threshold nothing passes
        for (uint32_t cls = 0; cls <= 15; ++cls)
            for (uint32_t u8 = 0; u8 < 64; u8 += 9)
                CHECK(!cone_rules_out_packed(cone_pack(u8, 31u, cls), w, idt[0], idt[1], idt[2], idt[3], idt[4], idt[5], idt[6], idt[7], idt[8], 1.0e30f),
                      "bad normal %zu is ruled out (class %u)", i, cls);
    }
    // lengths just inside the window are packed
    CHECK((model_normal_pack(0.9995f, 0.f, 0.f) & STOCS_MODEL_NORMAL_NO_GATE) == 0u, "0.9995 is flagged");
    CHECK((model_normal_pack(0.f, -1.0005f, 0.f) & STOCS_MODEL_NORMAL_NO_GATE) == 0u, "1.0005 is flagged");
    CHECK(model_normal_pack(0.f, -1.0005f, 0.f) == ((uint32_t)(-511 & 0x3FF) << 10), "1.0005 is not clamped to -511");
}

static void check_soundness() {
    Rng g(777);
    const float dot_lo = 0.8660254f;   // cos 30 degrees (compute_thresholds)
    const int trials = 1000000;
    long n_exact = 0, n_packed = 0, n_samples = 0, n_by_kind[5] = {0, 0, 0, 0, 0}, n_by_class[16];
    double closest = 1e30, worst_share = -1e30, tightest = 1e30;
    memset(n_by_class, 0, sizeof(n_by_class));
    for (int it = 0; it < trials; ++it) {
        const uint32_t cls = (uint32_t)(g() % 16u), u8 = (uint32_t)(g() % 64u), v8 = (uint32_t)(g() % 64u);
        const uint32_t yw = cone_pack(u8, v8, cls) | (uint32_t)(g() % 65536u);
        float oxf, oyf, ozf;
        cone_axis(yw, oxf, oyf, ozf);
        const D3 o = dunit(d3(oxf, oyf, ozf));
        const double delta = asin((double)cls / 16.0);
        // the linear part
        const int kind = it % 5;   // rigid, * 1e-3, * 1e3, sheared, mirrored
        double R[3][3], A[3][3];
        random_rotation(g, R);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) A[r][c] = R[r][c];
        if (kind == 1 || kind == 2) { const double s = kind == 1 ? 1.0e-3 : 1.0e3; for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) A[r][c] *= s; }
        if (kind == 3) {
            double S[3][3];
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) S[r][c] = (r == c ? 1.0 : 0.0) + uni(g, -0.6, 0.6);
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) A[r][c] = R[r][0] * S[0][c] + R[r][1] * S[1][c] + R[r][2] * S[2][c];
        }
        if (kind == 4) for (int r = 0; r < 3; ++r) A[r][1] = -A[r][1];
        // column-major entries as the kernel names them: t0 t1 t2 = column 0, t4 t5 t6 = column 1, t8 t9 t10 = column 2
        const float t0 = (float)A[0][0], t1 = (float)A[1][0], t2 = (float)A[2][0], t4 = (float)A[0][1], t5 = (float)A[1][1], t6 = (float)A[2][1],
                    t8 = (float)A[0][2], t9 = (float)A[1][2], t10 = (float)A[2][2];
        // the model normal: random, or (orthogonal linear parts) aimed so that A n lies within a degree of 30 degrees + delta from the axis
        D3 nd = random_unit(g);
        if ((it / 5) % 2 == 0 && (kind == 0 || kind == 4)) {
            const double theta = delta + (30.0 + uni(g, -1.0, 1.0)) * 0.017453292519943295, phi = uni(g, 0.0, 6.283185307179586);
            const D3 e1 = dperp(o), e2 = dcross(o, e1);
            const D3 v = dadd(dscale(o, cos(theta)), dscale(dadd(dscale(e1, cos(phi)), dscale(e2, sin(phi))), sin(theta)));
            nd = d3(A[0][0] * v.x + A[1][0] * v.y + A[2][0] * v.z, A[0][1] * v.x + A[1][1] * v.y + A[2][1] * v.z, A[0][2] * v.x + A[1][2] * v.y + A[2][2] * v.z);   // A^T v
        }
        const V3 n = f_unit(nd);
        const uint32_t pw = model_normal_pack(n.x, n.y, n.z);
        CHECK((pw & STOCS_MODEL_NORMAL_NO_GATE) == 0u, "trial %d: a unit normal is flagged", it);
        // the normal test's rotated normal, in the kernel's float expression
        const float nx = t0 * n.x + (t4 * n.y + t8 * n.z), ny = t1 * n.x + (t5 * n.y + t9 * n.z), nz = t2 * n.x + (t6 * n.y + t10 * n.z);
        if (cone_rules_out(yw, nx, ny, nz, dot_lo)) ++n_exact;
        const float s = linear_norm_bound(t0, t1, t2, t4, t5, t6, t8, t9, t10);
        const float thr = model_normal_gate_threshold(dot_lo, s);
        // 4 A: what the quantisation (and the two float rotations) can add to the support function is within s K
        float kx, ky, kz;
        model_normal_unpack(pw, kx, ky, kz);
        const float gx = t0 * kx + (t4 * ky + t8 * kz), gy = t1 * kx + (t5 * ky + t9 * kz), gz = t2 * kx + (t6 * ky + t10 * kz);   // as cone_rules_out_packed
        const D3 vt = d3(nx, ny, nz), vq = dscale(d3(gx, gy, gz), 1.0 / 511.0);
        const double sK = (double)s * (double)STOCS_MODEL_NORMAL_SLACK;
        {
            const double moved = (cone_support(vt, o, delta, cls != 0u) + 1.8e-7 * dnorm(vt)) - (cone_support(vq, o, delta, cls != 0u) + 1.8e-7 * dnorm(vq));
            worst_share = fmax(worst_share, moved / sK);
            CHECK(moved <= sK * (1.0 + 1.0e-9), "trial %d (kind %d, class %u): the packed normal moves the cone's support function by %.6g, s K = %.6g", it, kind, cls, moved, sK);
        }
        if (!cone_rules_out_packed(yw, pw, t0, t1, t2, t4, t5, t6, t8, t9, t10, thr)) continue;
        ++n_packed; ++n_by_kind[kind]; ++n_by_class[cls];
        CHECK(cls != 0u, "trial %d: ruled out without a cone", it);
        {   // 4 B: the float decision, allowed its proven rounding and no more, implies the inequality with the whole s K
            const double lhs = cone_bound(vq, o, delta) * (1.0 + 1.0e-4) + 2.0e-3 * (fabs(vq.x) + fabs(vq.y) + fabs(vq.z)) - 1.12e-3 * (1.0 + 1.0e-4) * dnorm(vq);
            tightest = fmin(tightest, ((double)dot_lo - sK) - lhs);
            CHECK(lhs < (double)dot_lo - sK, "trial %d (kind %d, class %u): ruled out with bound (1 + 1e-4) + m - rounding = %.9g, dot_lo - s K = %.9g", it, kind, cls, lhs, (double)dot_lo - sK);
        }
        // scene normals inside the cone
        const D3 v = d3(nx, ny, nz);
        D3 side = dadd(v, dscale(o, -ddot(v, o)));   // the direction from the axis towards v
        side = ddot(side, side) > 0.0 ? dunit(side) : dperp(o);
        const D3 e2 = dcross(o, side);
        for (int k = 0; k < 12; ++k) {
            double ang = delta, phi = 0.0, len = 1.0;
            if (k == 0) len = 1.0 - 1.0e-4;                 // the boundary towards v
            else if (k == 2) len = 1.0 + 1.0e-4;
            else if (k == 3) ang = 0.0;                       // the axis
            else if (k < 8) { phi = uni(g, -3.141592653589793, 3.141592653589793); len = 1.0 + uni(g, -1.0e-4, 1.0e-4); }   // the boundary elsewhere
            else { phi = uni(g, -0.3, 0.3); ang = delta * sqrt(uni(g, 0.0, 1.0)); len = 1.0 + uni(g, -1.0e-4, 1.0e-4); }     // the interior, on v's side
            const D3 dir = dadd(dscale(o, cos(ang)), dscale(dadd(dscale(side, cos(phi)), dscale(e2, sin(phi))), sin(ang)));
            const float sx = (float)(dir.x * len), sy = (float)(dir.y * len), sz = (float)(dir.z * len);
            const float d = sx * nx + (sy * ny + sz * nz);
            ++n_samples;
            closest = fmin(closest, (double)dot_lo - (double)d);
            CHECK(d < dot_lo, "trial %d (kind %d, class %u): ruled out, but a scene normal of the cone (sample %d) reaches d = %.9g >= %.9g", it, kind, cls, k, (double)d, (double)dot_lo);
        }
    }
    printf("gate: %d trials, ruled out by the exact-normal gate %ld, by the packed one %ld (rigid %ld, *1e-3 %ld, *1e3 %ld, sheared %ld, mirrored %ld); %ld cone samples, closest %.3g below dot_lo\n",
           trials, n_exact, n_packed, n_by_kind[0], n_by_kind[1], n_by_kind[2], n_by_kind[3], n_by_kind[4], n_samples, closest);
    printf("margin: the packed normal moved the support function by at most %.4f of s K; the tightest ruled-out trial kept %.3g of dot_lo - s K beyond the float rounding\n", worst_share, tightest);
    CHECK(worst_share > 0.5, "no trial used more than half of s K (%.4f): the margin was not exercised", worst_share);
    // (a host evaluates `bound` within ~1e-6, so the allowance of 1.12e-3 |v'| stays unused: the closest trial sits about that far off)
    CHECK(tightest < 1.2e-3, "no ruled-out trial came within the rounding allowance of the threshold (%.3g): the threshold was not exercised", tightest);
    CHECK(5 * n_exact >= trials, "the exact-normal gate ruled out %ld of %d trials: less than a fifth", n_exact, trials);
    CHECK(5 * n_packed >= trials, "the packed gate ruled out %ld of %d trials: less than a fifth", n_packed, trials);
    CHECK(n_packed <= n_exact + trials / 100, "the packed gate ruled out %ld trials, the exact one %ld", n_packed, n_exact);
    for (uint32_t c = 1; c <= 15; ++c) CHECK(n_by_class[c] > 0, "class %u was never ruled out", c);
    for (int k = 0; k < 5; ++k) if (k != 2) CHECK(n_by_kind[k] > 0, "kind %d was never ruled out", k);

    // a linear part that is not finite rules nothing out
    const uint32_t pw = model_normal_pack(0.f, 0.f, 1.f), yw = cone_pack(31u, 31u, 1u) | 5u;
    const float inf = INFINITY, nan = NAN;
    for (int which = 0; which < 9; ++which)
        for (int val = 0; val < 3; ++val) {
            float t[9] = {1, 0, 0, 0, 0, 1, 0, -1, 0};   // turns +z onto -y: ruled out against an axis of +z
            CHECK(cone_rules_out_packed(yw, pw, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8],
                                        model_normal_gate_threshold(dot_lo, linear_norm_bound(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]))),
                  "the finite matrix is not ruled out");
            t[which] = val == 0 ? nan : (val == 1 ? inf : -inf);
            const float s = linear_norm_bound(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]);
            CHECK(!cone_rules_out_packed(yw, pw, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], model_normal_gate_threshold(dot_lo, s)),
                  "entry %d = %g: ruled out", which, (double)t[which]);
        }
}

int main() {
    check_pack_error();
    check_flags();
    check_soundness();
    if (g_fail) { printf("packed_normal_check: %d checks FAILED\n", g_fail); return 1; }
    printf("packed_normal_check: ok\n");
    return 0;
}
