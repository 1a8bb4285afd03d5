// The host geometry of the scene grid (csrc/grid_geometry.h), alone: no GPU, no library, no HIP header.
// Stand-alone: g++ only; tests/test_grid_geometry_cpu.py builds it with -fsanitize=address,undefined and -ffp-contract=off (the
// library's own setting) and runs it directly.
// stdin: one build per line -- the bounding box of the centred scene (min x y z, max x y z) and epsilon as hexadecimal doubles, then div.
// stdout: per line the bits of the float origin, of h and of inv_h, the cells and bricks per axis, then r, pad, the prune slack
// (hh, margin, octant half-width) as hexadecimal doubles and the bits of a cell key.
#include <stdio.h>
#include <string.h>

#include "../../model_matching_amd/csrc/grid_geometry.h"

static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

int main() {
    double mn[3], mx[3], eps;
    int div, lines = 0;
    while (scanf("%la %la %la %la %la %la %la %d", &mn[0], &mn[1], &mn[2], &mx[0], &mx[1], &mx[2], &eps, &div) == 8) {
        const stocs::GridBox B = stocs::grid_geometry(mn, mx, eps, div);
        printf("%08x %08x %08x %08x %08x %d %d %d %d %d %d %a %a %a %a %a %d\n", bits(B.of[0]), bits(B.of[1]), bits(B.of[2]), bits(B.hf), bits(B.inv_h), B.n[0], B.n[1],
               B.n[2], B.nb[0], B.nb[1], B.nb[2], B.r, B.pad, B.hh, B.margin, B.oct_hw, B.cell_bits);
        lines++;
    }
    return lines ? 0 : 1;
}
