// patch_normals_check.cpp -- host check of the sub-patch normal-cone test of the shared-list forms (csrc/patch_normals.h).
// Stand-alone: g++ only, no GPU, no library; may be built with -fsanitize=address,undefined.  Build with -ffp-contract=off (the
// project's numerics contract: the float expressions below are the kernel's own).
//   1. soundness against a brute-force maximum: random field words of every class, random model cones (beta up to 45 degrees), random
//      linear parts (rigid, scaled by 1e-3 and 1e3, sheared, mirrored), half of the orthogonal ones aimed within a degree of the angle at
//      which the test starts to rule out.  Over members n_m of the model cone (the boundary towards the scene cone, the boundary at 64
//      azimuths, the axis, the interior; lengths 1 +- 1e-6) and members n_s of the scene cone (the boundary towards v at lengths
//      1 - 1e-4, 1, 1 + 1e-4, the boundary at 64 azimuths, the axis, the interior) the kernel's own float dot product
//      sn.x*nx + (sn.y*ny + sn.z*nz) on vt = fl(A n_m) never exceeds pn_bound when v lies outside the scene cone, and stays below dot_lo
//      whenever pn_rules_out says so.  At least a tenth of the trials must be ruled out, in every kind and in classes low and high, so
//      that a dead test cannot pass.
//   2. the bound is the derivation's: within 2.2e-3 |v|_1 + 3e-4 s above X cos(beta') + s sin(beta') evaluated in double.
//   3. nothing is ruled out by a word without a cone (class 0, 241 .. 255), a record without a test (sb < 0, sb > sin 45 degrees, NaN),
//      a rotated axis inside the scene cone, or a linear part that is not finite.
// Prints its counts; exit status 0 when every check holds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>

#include "../../model_matching_amd/csrc/patch_normals.h"

using namespace stocs;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

struct D3 { double x, y, z; };
static D3 d3(double x, double y, double z) { D3 r = {x, y, z}; return r; }
static double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static D3 dscale(D3 a, double s) { return d3(a.x * s, a.y * s, a.z * s); }
static D3 dadd(D3 a, D3 b) { return d3(a.x + b.x, a.y + b.y, a.z + b.z); }
static D3 dcross(D3 a, D3 b) { return d3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static double dnorm(D3 a) { return sqrt(ddot(a, a)); }
static D3 dunit(D3 a) { return dscale(a, 1.0 / dnorm(a)); }
static D3 dperp(D3 a) { return dunit(dcross(a, fabs(a.x) < 0.6 ? d3(1, 0, 0) : d3(0, 1, 0))); }
static double angle_to(D3 v, D3 o) { return atan2(dnorm(dcross(v, o)), ddot(v, o)); }
// the unit vector at angle `ang` from the unit axis o, at azimuth phi counted from the direction `side` (unit, orthogonal to o)
static D3 on_cone(D3 o, D3 side, double ang, double phi) {
    const D3 e2 = dcross(o, side);
    return dadd(dscale(o, cos(ang)), dscale(dadd(dscale(side, cos(phi)), dscale(e2, sin(phi))), sin(ang)));
}
// the unit direction from the axis o towards v (any perpendicular when v lies on the axis)
static D3 towards(D3 o, D3 v) {
    const D3 s = dadd(v, dscale(o, -ddot(v, o)));
    return ddot(s, s) > 1e-24 ? dunit(s) : dperp(o);
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
static void random_rotation(Rng& g, double r[3][3]) {
    const D3 a = random_unit(g), b0 = dperp(a);
    const double phi = uni(g, 0.0, 6.283185307179586);
    const D3 b = dadd(dscale(b0, cos(phi)), dscale(dcross(a, b0), sin(phi))), c = dcross(a, b);
    r[0][0] = a.x; r[0][1] = a.y; r[0][2] = a.z; r[1][0] = b.x; r[1][1] = b.y; r[1][2] = b.z; r[2][0] = c.x; r[2][1] = c.y; r[2][2] = c.z;
}

static const float DOT_LO = 0.8660254f;   // cos 30 degrees (compute_thresholds)

static void check_soundness() {
    Rng g(4242);
    const int trials = 60000;
    long n_out = 0, n_outside = 0, n_samples = 0, n_kind[5] = {0, 0, 0, 0, 0}, n_low = 0, n_high = 0;
    double closest = 1e30, least_room = 1e30, loosest = 0.0;
    for (int it = 0; it < trials; ++it) {
        const uint32_t cls = 1u + (uint32_t)(g() % 240u);
        const uint32_t w = pn_pack((uint32_t)(g() % 4096u), (uint32_t)(g() % 4096u), cls);
        float oxf, oyf, ozf;
        pn_axis(w, oxf, oyf, ozf);
        const D3 o = dunit(d3(oxf, oyf, ozf));
        const double delta = asin((double)cls / 256.0);
        const double beta = uni(g, 0.0, 1.0) < 0.7 ? uni(g, 0.0, 0.35) : uni(g, 0.0, 0.785);
        const float sb = nextafterf((float)(sin(beta) * (1.0 + 1.0e-6) + 1.0e-7), 2.0f);
        if (!(sb <= STOCS_PN_MAX_SIN_BETA)) { --it; continue; }
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
        const float t0 = (float)A[0][0], t1 = (float)A[1][0], t2 = (float)A[2][0], t4 = (float)A[0][1], t5 = (float)A[1][1], t6 = (float)A[2][1],
                    t8 = (float)A[0][2], t9 = (float)A[1][2], t10 = (float)A[2][2];
        // the model axis: random, or (orthogonal linear parts) aimed so that the bound X cos(beta) + sin(beta) lands within a degree of dot_lo
        D3 ad = random_unit(g);
        if ((it / 5) % 2 == 0 && (kind == 0 || kind == 4)) {
            // X = cos(theta - delta) solves X cos(beta) + sin(beta) = cos(30 degrees + jitter)
            const double X = (cos((30.0 + uni(g, -1.0, 1.0)) * 0.017453292519943295) - sin(beta)) / cos(beta);
            const double theta = delta + acos(fmax(fmin(X, 1.0), -1.0));
            const D3 v = on_cone(o, dperp(o), theta, uni(g, 0.0, 6.283185307179586));
            ad = d3(A[0][0] * v.x + A[1][0] * v.y + A[2][0] * v.z, A[0][1] * v.x + A[1][1] * v.y + A[2][1] * v.z, A[0][2] * v.x + A[1][2] * v.y + A[2][2] * v.z);   // A^T v
        }
        const V3 af = normalized3(mk3((float)ad.x, (float)ad.y, (float)ad.z));
        const D3 a = dunit(d3(af.x, af.y, af.z));
        const float s = linear_norm_bound(t0, t1, t2, t4, t5, t6, t8, t9, t10);
        const float vx = t0 * af.x + (t4 * af.y + t8 * af.z), vy = t1 * af.x + (t5 * af.y + t9 * af.z), vz = t2 * af.x + (t6 * af.y + t10 * af.z);
        bool outside = false;
        const float b = pn_bound(w, vx, vy, vz, sb, s, &outside);
        const bool out = pn_rules_out(w, af.x, af.y, af.z, sb, s, t0, t1, t2, t4, t5, t6, t8, t9, t10, DOT_LO);
        CHECK(!out || (outside && b < DOT_LO), "trial %d: ruled out with outside %d, bound %.9g", it, (int)outside, (double)b);
        if (!outside) continue;
        ++n_outside;
        const D3 v = d3(vx, vy, vz);
        {   // 2: the float bound against the derivation's expression in double
            const double th = angle_to(v, o), X = dnorm(v) * cos(fmax(th - delta, 0.0)), bp = asin((double)sb);
            const double exact = X * cos(bp) + (double)s * sin(bp);
            const double room = (double)b - exact, l1 = fabs(v.x) + fabs(v.y) + fabs(v.z);
            least_room = fmin(least_room, room / (double)s);
            loosest = fmax(loosest, room / (2.2e-3 * l1 + 3.0e-4 * (double)s));
            CHECK(room > 0.0, "trial %d (kind %d): the bound %.9g is below X cos(beta) + s sin(beta) = %.9g", it, kind, (double)b, exact);
            CHECK(room <= 2.2e-3 * l1 + 3.0e-4 * (double)s, "trial %d (kind %d): the bound %.9g is %.3g above the derivation's %.9g", it, kind, (double)b, room, exact);
        }
        if (out) { ++n_out; ++n_kind[kind]; if (cls <= 40u) ++n_low; if (cls >= 160u) ++n_high; }
        // 1: the brute-force maximum of the kernel's dot product over members of both cones
        const D3 At_o = d3(A[0][0] * o.x + A[1][0] * o.y + A[2][0] * o.z, A[0][1] * o.x + A[1][1] * o.y + A[2][1] * o.z, A[0][2] * o.x + A[1][2] * o.y + A[2][2] * o.z);
        const D3 m_side = towards(a, At_o);
        float dmax = -INFINITY;
        for (int km = 0; km < 70; ++km) {
            double ang = beta, phi = 0.0, len = 1.0;
            if (km == 0) len = 1.0 + 1.0e-6;
            else if (km == 1) len = 1.0 - 1.0e-6;
            else if (km == 2) ang = 0.0;
            else if (km < 67) phi = (km - 3) * (6.283185307179586 / 64.0);
            else { phi = uni(g, -0.5, 0.5); ang = beta * sqrt(uni(g, 0.0, 1.0)); }
            const D3 nm = dscale(on_cone(a, m_side, ang, phi), len);
            const float mx = (float)nm.x, my = (float)nm.y, mz = (float)nm.z;
            const float nx = t0 * mx + (t4 * my + t8 * mz), ny = t1 * mx + (t5 * my + t9 * mz), nz = t2 * mx + (t6 * my + t10 * mz);   // the normal test's rotation
            const D3 vt = d3(nx, ny, nz);
            const D3 s_side = towards(o, vt);
            for (int ks = 0; ks < 12; ++ks) {
                double sang = delta, sphi = 0.0, slen = 1.0;
                if (ks == 0) slen = 1.0 - 1.0e-4;
                else if (ks == 2) slen = 1.0 + 1.0e-4;
                else if (ks == 3) sang = 0.0;
                else if (ks < 9) { sphi = uni(g, -3.141592653589793, 3.141592653589793); slen = 1.0 + uni(g, -1.0e-4, 1.0e-4); }
                else { sphi = uni(g, -0.3, 0.3); sang = delta * sqrt(uni(g, 0.0, 1.0)); slen = 1.0 + uni(g, -1.0e-4, 1.0e-4); }
                // (the member of the cone closest to vt is vt's own direction when vt lies inside it)
                const double tv = angle_to(vt, o);
                const D3 dir = (ks < 3 && tv < delta) ? dunit(vt) : on_cone(o, s_side, sang, sphi);
                const float sx = (float)(dir.x * slen), sy = (float)(dir.y * slen), sz = (float)(dir.z * slen);
                const float d = sx * nx + (sy * ny + sz * nz);
                dmax = fmaxf(dmax, d);
                ++n_samples;
            }
        }
        CHECK(dmax <= b, "trial %d (kind %d, class %u, beta %.3f): a pair of members reaches d = %.9g above the bound %.9g", it, kind, cls, beta, (double)dmax, (double)b);
        if (out) {
            closest = fmin(closest, (double)DOT_LO - (double)dmax);
            CHECK(dmax < DOT_LO, "trial %d (kind %d, class %u, beta %.3f): ruled out, but a pair of members reaches d = %.9g", it, kind, cls, beta, (double)dmax);
        }
    }
    printf("test: %d trials, %ld with v outside the scene cone, ruled out %ld (rigid %ld, *1e-3 %ld, *1e3 %ld, sheared %ld, mirrored %ld; classes <= 40: %ld, >= 160: %ld); %ld member pairs, closest %.3g below dot_lo\n",
           trials, n_outside, n_out, n_kind[0], n_kind[1], n_kind[2], n_kind[3], n_kind[4], n_low, n_high, n_samples, closest);
    printf("bound: at least %.3g s and at most %.3f of its allowance above the derivation's expression\n", least_room, loosest);
    CHECK(10 * n_out >= trials, "ruled out %ld of %d trials: less than a tenth", n_out, trials);
    for (int k = 0; k < 5; ++k) CHECK(n_kind[k] > 0, "kind %d was never ruled out", k);
    CHECK(n_low > 0 && n_high > 0, "classes low (%ld) or high (%ld) were never ruled out", n_low, n_high);
    CHECK(closest < 0.02, "no ruled-out trial came within 0.02 of dot_lo (%.3g): the threshold was not exercised", closest);
}

static void check_no_test() {
    // +z turned onto -y against a scene axis of +z: ruled out as it stands
    const uint32_t up = pn_pack(2048u, 2048u, 8u);
    float ox, oy, oz;
    pn_axis(up, ox, oy, oz);
    CHECK(fabsf(ox) < 1e-3f && fabsf(oy) < 1e-3f && oz > 0.99f, "the word's axis is %g %g %g", ox, oy, oz);
    const float t[9] = {1, 0, 0, 0, 0, 1, 0, -1, 0};
    const float s1 = linear_norm_bound(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]);
    CHECK(pn_rules_out(up, 0.f, 0.f, 1.f, 0.1f, s1, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], DOT_LO), "the plain case is not ruled out");
    for (uint32_t cls = 0; cls < 256u; ++cls) {
        const bool out = pn_rules_out(pn_pack(2048u, 2048u, cls), 0.f, 0.f, 1.f, 0.1f, s1, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], DOT_LO);
        if (cls == 0u || cls > STOCS_PN_MAX_CLASS) CHECK(!out, "class %u rules out", cls);
    }
    const float sbs[] = {STOCS_PN_NO_TEST, -0.0001f, 0.7072f, 1.0f, 2.0f, NAN, INFINITY, -INFINITY};
    for (size_t i = 0; i < sizeof(sbs) / sizeof(sbs[0]); ++i)
        CHECK(!pn_rules_out(up, 0.f, 0.f, 1.f, sbs[i], s1, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], DOT_LO), "sb = %g rules out", (double)sbs[i]);
    CHECK(!pn_rules_out(up, NAN, 0.f, 1.f, 0.1f, s1, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], DOT_LO), "a NaN axis rules out");
    // the rotated axis inside the scene cone: never, whatever dot_lo
    const float id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    CHECK(!pn_rules_out(up, 0.f, 0.f, 1.f, 0.1f, 1.00001f, id[0], id[1], id[2], id[3], id[4], id[5], id[6], id[7], id[8], 1.0e30f), "an axis inside the scene cone rules out");
    // a zero matrix: v = 0 lies in no direction, nothing is ruled out
    CHECK(!pn_rules_out(up, 0.f, 0.f, 1.f, 0.1f, 0.f, 0, 0, 0, 0, 0, 0, 0, 0, 0, DOT_LO), "the zero matrix rules out");
    const float inf = INFINITY, nan = NAN;
    for (int which = 0; which < 9; ++which)
        for (int val = 0; val < 4; ++val) {
            float m[9];
            memcpy(m, t, sizeof(m));
            m[which] = val == 0 ? nan : (val == 1 ? inf : (val == 2 ? -inf : 3.0e38f));
            const float s = linear_norm_bound(m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8]);
            CHECK(!pn_rules_out(up, 0.f, 0.f, 1.f, 0.1f, s, m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], DOT_LO), "entry %d = %g: ruled out", which, (double)m[which]);
        }
    CHECK(pn_reach_for_kernel(0.02f) < 0.02f && pn_reach_for_kernel(0.02f) > 0.0199f && pn_reach_for_kernel(0.f) == 0.f, "pn_reach_for_kernel");
}

int main() {
    check_soundness();
    check_no_test();
    if (g_fail) { printf("patch_normals_check: %d checks FAILED\n", g_fail); return 1; }
    printf("patch_normals_check: ok\n");
    return 0;
}
