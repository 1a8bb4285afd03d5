// segment_gate.h -- the size gate between a segment's shape and an object's size (include/stocs_hip.h, stocs_segment_gate), one routine
// for the host entry point (stocs_segment_gate) and the device pass of stocs_segment_assign (segment_shapes.hip): the same float
// operations in the same order on both sides (every translation unit is built with -ffp-contract=off).  The rule rests on two facts of
// geometry, not on data: no view of a body is wider than its diameter, and an unoccluded view of a box shows at least its middle extent.
#ifndef STOCS_SEGMENT_GATE_H
#define STOCS_SEGMENT_GATE_H

#include "stocs_hip.h"
#include "stocs_math.h"

namespace stocs {

// e[0 .. 3) in descending order of value into s
STOCS_HD void gate_sort3(const float* e, float* s) {
    float a = e[0], b = e[1], c = e[2], t;
    if (a < b) { t = a; a = b; b = t; }
    if (b < c) { t = b; b = c; c = t; }
    if (a < b) { t = a; a = b; b = t; }
    s[0] = a; s[1] = b; s[2] = c;
}

// the reason bits (STOCS_GATE_*) that keep a segment from an object; 0: compatible.  A comparison with NaN is false.
STOCS_HD unsigned segment_gate_reasons(const stocs_segment_shape& s, const stocs_object_size& o, const stocs_segment_gate_params& g) {
    float e[3], m[3];
    gate_sort3(s.extent, e);
    gate_sort3(o.extent, m);
    const float widest = (1.0f + g.slack) * o.diameter;
    const float least = g.min_ratio * m[1];
    unsigned r = 0;
    if (e[0] > widest) r |= STOCS_GATE_TOO_LARGE;
    if (e[0] < least) r |= STOCS_GATE_TOO_SMALL;
    if (s.n_used < g.min_used || s.flags != 0) r |= STOCS_GATE_NO_SHAPE;
    return r;
}

}  // namespace stocs

#endif
