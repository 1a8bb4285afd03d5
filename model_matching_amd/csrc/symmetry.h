// symmetry.h -- the cell expression of the self-distance grid (stocs_symmetry_errors, include/stocs_hip.h), shared by the host, which
// bins the targets with it, and the device, which bins the queries with it, and the argument why 27 cells suffice.
#ifndef STOCS_SYMMETRY_H
#define STOCS_SYMMETRY_H

#include "stocs_math.h"

namespace stocs {

// origin (the box minimum), 1 / h and the cell counts of the grid
struct SymGrid { float ox, oy, oz, inv; int nx, ny, nz; };

// The continuous cell coordinate along one axis: ONE float subtraction and ONE float product.  Both are monotone in x, so is u.
//
// Why the 27 cells about floor(u(p)) hold every target m with computed D(p, m) <= reach * reach (per axis; o <= m_a, so u(m) >= 0):
//   * the computed D is at least (1 - 2^-21) times the exact squared distance (three subtractions, three squares and two sums of
//     non-negative terms, each within 2^-24 relative), so |p_a - m_a| <= reach (1 + 2^-21);
//   * u(x) = fl(fl(x - o) inv) with inv = fl(1 / h): |u(x) - (x - o) / h| <= 3 * 2^-24 |u(x)| (plus nothing for underflow that matters:
//     a subnormal product is below one cell by far).  The grid has at most STOCS_SYMMETRY_GRID_SPAN + 2 cells per axis and a query that
//     has such a target lies within one cell of the box, so |u| < 64 for both and each error is below 2^-16;
//   * h >= fl(reach * 65 / 64) >= reach (65 / 64) (1 - 2^-24), so |u(p) - u(m)| <= (64 / 65) (1 + 2^-20) + 2^-15 < 0.985 < 1,
//     and two numbers less than 1 apart have floors at most 1 apart.
// The first step needs squares that do not underflow: the entry points refuse a reach whose square is below the smallest normal float, so
// a pair whose exact squared distance exceeds reach * reach has its largest square at or above a third of that, where even a
// subnormal's rounding is within 2^-22 of it: its computed D cannot fall to reach * reach by underflow.
// A query whose u is NaN or far outside is clamped to a cell index outside the grid: it meets no cell.
STOCS_HD float sym_cell_coord(float x, float o, float inv) { return (x - o) * inv; }
STOCS_HD int sym_cell(float x, float o, float inv) {
    const float u = floorf(sym_cell_coord(x, o, inv));
    return u >= -2.0f ? (u <= 1024.0f ? (int)u : 1025) : -2;   // NaN: -2
}

}  // namespace stocs

#endif
