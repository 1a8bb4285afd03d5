// solve6.h -- the 6x6 solve of the linearised point-to-plane step A^T A x = A^T b, shared by refine.hip (refine_solve_kernel, on the
// device) and icp.hip (its host loop).
#pragma once
#include <math.h>

#include "stocs_math.h"

namespace stocs {

// Gaussian elimination with partial pivoting (first largest pivot), unrolled so that on the device the system stays in registers: the
// row swap is a select on every candidate row instead of an indexed access
STOCS_HD bool solve6(double A[6][6], double b[6], double x[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        int p = c;
        double pv = fabs(A[c][c]);
#pragma unroll
        for (int r = c + 1; r < 6; ++r) { const double v = fabs(A[r][c]); if (v > pv) { pv = v; p = r; } }
        if (pv < 1e-300) return false;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            const bool sw = r == p;
#pragma unroll
            for (int k = 0; k < 6; ++k) { const double t = A[r][k]; A[r][k] = sw ? A[c][k] : t; A[c][k] = sw ? t : A[c][k]; }
            const double t = b[r]; b[r] = sw ? b[c] : t; b[c] = sw ? t : b[c];
        }
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            const double f = A[r][c] / A[c][c];
#pragma unroll
            for (int k = c; k < 6; ++k) A[r][k] -= f * A[c][k];
            b[r] -= f * b[c];
        }
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double s = b[r];
#pragma unroll
        for (int k = r + 1; k < 6; ++k) s -= A[r][k] * x[k];
        x[r] = s / A[r][r];
    }
    return true;
}

}  // namespace stocs
