// grid_geometry.h -- the host geometry of the scene brick grid (grid.hip): from the bounding box of the centred scene,
// epsilon and the cell edge to the origin, the cells and bricks per axis, the inclusion radius and the slack of the dominance pruning.
// Plain C++ in double, no HIP: tests/cpp/grid_geometry_check.cpp compiles it alone and tests/grid_ref.py restates it (geometry,
// inclusion_radius), bit for bit.
#ifndef STOCS_GRID_GEOMETRY_H
#define STOCS_GRID_GEOMETRY_H

#include <math.h>
#include <stdint.h>

namespace stocs {

enum { STOCS_GRID_MAX_BRICKS = 400 * 1000 * 1000 };   // entries of the top-level brick table a build accepts

struct GridBox {
    double h, r, pad;      // cell edge, inclusion radius, margin between the scene's box and the grid's faces
    float of[3];           // origin as the scan kernels use it (the build's kernels use exactly this float, widened)
    float hf, inv_h;       // cell edge and its inverse as the scan kernels receive them
    int n[3], nb[3];       // cells and bricks per axis
    int64_t n_top;         // bricks of the top-level table
    int cell_bits;         // bits of a cell key (brick << 9 | local cell); 0 when the table is too large to build
    double qscale;         // quantisation of a listed point's distance to its cell centre to 16 bits (centre-sorted lists)
    double hh, margin;     // dominance pruning: half edge of the widened cell box, margin of the squared-distance comparison
    double oct_hw;         // ... half edge of the widened octant box (octant_lists.h)
};

// mn, mx: the bounding box of the centred scene (0, 0 for an empty one); h = eps / div
inline GridBox grid_geometry(const double mn[3], const double mx[3], double eps, int div) {
    GridBox B;
    const double h = eps / div;
    const double r0 = eps * 1.001;  // safety margin >> float rounding of the device cell computation -- on scenes of ordinary extent
    // The scan kernels compute floor((q - o_f) * inv_h) in float: the subtraction, the float inv_h and the product each contribute up to
    // 2^-24 of the offset from the origin, so the face they see can lie 3 * 2^-24 * span from the box face used here (measured: up to
    // 1.5e-3 eps at an extent of 31 000 eps, 1.1e-2 eps at 262 000).  The margin grows with the extent once 2^-21 of it exceeds the
    // thousandth of epsilon -- from about 2 100 epsilons on; below that r is what it always was
    double ext = 0;
    for (int k = 0; k < 3; ++k) ext = fmax(ext, mx[k] - mn[k]);
    const double span = ext + 2.0 * (r0 + 2 * h) + h;   // the largest offset from the origin inside the grid
    const double r = fmax(r0, eps + span * (1.0 / 2097152.0));
    const double pad = r + 2 * h;  // a query outside the grid is farther than epsilon from every point
    B.h = h; B.r = r; B.pad = pad;
    for (int k = 0; k < 3; ++k) {
        const double o = mn[k] - pad;
        B.n[k] = (int)floor((mx[k] + pad - o) / h) + 1;
        B.nb[k] = (B.n[k] + 7) / 8;
        B.of[k] = (float)o;
    }
    B.hf = (float)h;
    B.inv_h = (float)(1.0 / h);
    B.n_top = (int64_t)B.nb[0] * B.nb[1] * B.nb[2];
    B.cell_bits = 0;
    if (B.n_top <= (int64_t)STOCS_GRID_MAX_BRICKS) {
        B.cell_bits = 1;
        while (((int64_t)1 << B.cell_bits) < B.n_top * 512) B.cell_bits++;
    }
    B.qscale = 65535.0 / (r + h * 0.8660254037844387 + 1e-9);   // a listed point is at most r + half a cell diagonal from the centre
    // positions the kernels assign to a cell lie inside its box up to the float rounding of floor((q - o) * inv_h): 3 ulp of the
    // offset from the origin; squared distances are evaluated in float with a relative error below 4e-7 each
    double side = 0;
    for (int k = 0; k < 3; ++k) side = fmax(side, (double)B.n[k] * h);
    const double reach = r + 2.0 * h;
    B.hh = 0.5 * h + 2.0e-6 * (side + 1.0) * 0.5 + 1.0e-7;
    B.margin = 4.0e-6 * reach * reach;
    B.oct_hw = 0.25 * h + (B.hh - 0.5 * h);   // the octant box, widened by the slack of the cell box
    return B;
}

}  // namespace stocs

#endif
