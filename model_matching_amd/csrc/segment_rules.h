// segment_rules.h -- what segment.hip (labels of a depth frame) and segment_shapes.hip (shapes of labelled regions) must agree on: the
// limits and the tile, and step 1's one expression for a pixel's point (include/stocs_hip.h, stocs_segment_frame step 1).
#ifndef STOCS_SEGMENT_RULES_H
#define STOCS_SEGMENT_RULES_H

#include "stocs_math.h"

namespace stocs {

enum { SEG_MAX_BEND = 8, SEG_MAX_SMOOTH = 4, SEG_TILE_W = 64, SEG_TILE_H = 16, SEG_SCORE_PTS = 1024, SEG_SCORE_HYP = 64, SEG_SWEEPS = 12, SEG_MAX_HYP = 1 << 20, SEG_MAX_PIX = 1 << 22 };

// pixel (row i, column j) at depth z -> x, y: in double, one cast each.  The smoothed points are formed by the same expression
// (tests/segment_convex_ref.py relies on the two being equal bit for bit)
__device__ __forceinline__ V3 seg_unproject(int i, int j, float z, float fx, float cx, float fy, float cy) {
    return mk3((float)(((double)j - (double)cx) * (double)z / (double)fx), (float)(((double)i - (double)cy) * (double)z / (double)fy), z);
}

}  // namespace stocs

#endif
