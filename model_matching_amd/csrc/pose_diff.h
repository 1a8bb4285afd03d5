// pose_diff.h -- get_pose_diff and quaternion_to_euler of the reference (src/pose_clustering.cpp:27-71, 5-25), one routine for
// the host clustering (stocs_cluster_poses) and the device clustering of trial batches (cluster.hip): the same float and double
// operations in the same order on both sides (every translation unit is built with -ffp-contract=off; float divide and sqrt are
// IEEE on both).  The double atan2 / asin are the one place where the two sides use different libraries (glibc, the device
// libm): both are within an ulp of the true value, and the result is rounded to float before any decision.
#ifndef STOCS_POSE_DIFF_H
#define STOCS_POSE_DIFF_H

#include <math.h>

#include "stocs_math.h"

namespace stocs {

struct HM3 { float m[3][3]; };
STOCS_HD HM3 hmul(const HM3& A, const HM3& B) {
    HM3 C;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C.m[i][j] = A.m[i][0] * B.m[0][j] + (A.m[i][1] * B.m[1][j] + A.m[i][2] * B.m[2][j]);
    return C;
}
STOCS_HD HM3 hinverse(const HM3& a) {  // cofactor inverse, as Eigen does for fixed 3x3
    HM3 r;
    const float c00 = a.m[1][1] * a.m[2][2] - a.m[1][2] * a.m[2][1];
    const float c01 = a.m[1][2] * a.m[2][0] - a.m[1][0] * a.m[2][2];
    const float c02 = a.m[1][0] * a.m[2][1] - a.m[1][1] * a.m[2][0];
    const float det = a.m[0][0] * c00 + (a.m[0][1] * c01 + a.m[0][2] * c02);
    const float inv = 1.0f / det;
    r.m[0][0] = c00 * inv; r.m[1][0] = c01 * inv; r.m[2][0] = c02 * inv;
    r.m[0][1] = (a.m[0][2] * a.m[2][1] - a.m[0][1] * a.m[2][2]) * inv;
    r.m[1][1] = (a.m[0][0] * a.m[2][2] - a.m[0][2] * a.m[2][0]) * inv;
    r.m[2][1] = (a.m[0][1] * a.m[2][0] - a.m[0][0] * a.m[2][1]) * inv;
    r.m[0][2] = (a.m[0][1] * a.m[1][2] - a.m[0][2] * a.m[1][1]) * inv;
    r.m[1][2] = (a.m[0][2] * a.m[1][0] - a.m[0][0] * a.m[1][2]) * inv;
    r.m[2][2] = (a.m[0][0] * a.m[1][1] - a.m[0][1] * a.m[1][0]) * inv;
    return r;
}
STOCS_HD void mat_to_quat(const HM3& a, float q[4] /*x,y,z,w*/) {  // Eigen Quaternion(Matrix3)
    float t = a.m[0][0] + a.m[1][1] + a.m[2][2];
    if (t > 0.0f) {
        t = sqrtf(t + 1.0f);
        q[3] = 0.5f * t;
        t = 0.5f / t;
        q[0] = (a.m[2][1] - a.m[1][2]) * t;
        q[1] = (a.m[0][2] - a.m[2][0]) * t;
        q[2] = (a.m[1][0] - a.m[0][1]) * t;
    } else {
        int i = 0;
        if (a.m[1][1] > a.m[0][0]) i = 1;
        if (a.m[2][2] > a.m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrtf(a.m[i][i] - a.m[j][j] - a.m[k][k] + 1.0f);
        q[i] = 0.5f * t;
        t = 0.5f / t;
        q[3] = (a.m[k][j] - a.m[j][k]) * t;
        q[j] = (a.m[j][i] + a.m[i][j]) * t;
        q[k] = (a.m[k][i] + a.m[i][k]) * t;
    }
}
STOCS_HD float fmin_std(float a, float b) { return (b < a) ? b : a; }   // std::min / std::max, NaN behaviour included
STOCS_HD float fmax_std(float a, float b) { return (a < b) ? b : a; }

// the inverse of the test pose's rotation (3x3 of a column-major 4x4): the same bits for every cluster it is compared with
STOCS_HD HM3 pose_inverse_rotation(const float* test) {
    HM3 t;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) t.m[i][j] = test[j * 4 + i];
    return hinverse(t);
}

// rotation part of get_pose_diff(test, base): degrees, folded by sym_info; test_inv = pose_inverse_rotation(test)
STOCS_HD float pose_rot_err(const HM3& test_inv, const float* base, const float* sym) {
    HM3 b;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) b.m[i][j] = base[j * 4 + i];
    const HM3 diff = hmul(test_inv, b);
    float q[4], e[3];
    mat_to_quat(diff, q);
    // quaternion_to_euler, pose_clustering.cpp:5-25 (float products promoted to double)
    const double sinr = +2.0 * (double)(q[3] * q[0] + q[1] * q[2]);
    const double cosr = +1.0 - 2.0 * (double)(q[0] * q[0] + q[1] * q[1]);
    e[0] = (float)atan2(sinr, cosr);
    const double sinp = +2.0 * (double)(q[3] * q[1] - q[2] * q[0]);
    if (fabs(sinp) >= 1) e[1] = (float)copysign(M_PI / 2, sinp);
    else e[1] = (float)asin(sinp);
    const double siny = +2.0 * (double)(q[3] * q[2] + q[0] * q[1]);
    const double cosy = +1.0 - 2.0 * (double)(q[1] * q[1] + q[2] * q[2]);
    e[2] = (float)atan2(siny, cosy);
    for (int d = 0; d < 3; ++d) {
        e[d] = (float)((double)e[d] * 180.0 / M_PI);
        e[d] = fabsf(e[d]);
        if (sym[d] == 90) {
            e[d] = fabsf(e[d] - 90);
            e[d] = fmin_std(e[d], 90 - e[d]);
        } else if (sym[d] == 180) {
            e[d] = fmin_std(e[d], 180 - e[d]);
        } else if (sym[d] == 360) {
            e[d] = 0;
        }
    }
    return fmax_std(fmax_std(e[0], e[1]), e[2]);
}

// translation part: |t_base - t_test| in double.  The reference squares with pow(d, 2); d is a float difference, so d * d is exact
// in double and equals what any pow within an ulp returns
STOCS_HD float pose_trans_err3(const float* test_t, const float* base_t) {   // the translations alone
    const double dx = (double)(base_t[0] - test_t[0]), dy = (double)(base_t[1] - test_t[1]), dz = (double)(base_t[2] - test_t[2]);
    return (float)sqrt(dx * dx + dy * dy + dz * dz);
}
STOCS_HD float pose_trans_err(const float* test, const float* base) { return pose_trans_err3(test + 12, base + 12); }

}  // namespace stocs

#endif
