// render_rules.h -- the rules of the render and depth-check contracts (include/stocs_hip.h) that more than one file applies: which poses
// touch nothing, the splat radius of an in_image point and the walk over its square, and steps 5-6 of the depth-check contract for a
// surface at depth z seen at a pixel; on the host, the check of stocs_render_params and the render arguments.  Included by depth.hip
// (pose_finite, classify_pixel), render.hip (stocs_render_poses and its kin) and scene.hip (stocs_scene_footprints).  The frame itself,
// its checks and its arguments are depth_frame.h's.
#ifndef STOCS_RENDER_RULES_H
#define STOCS_RENDER_RULES_H

#include <math.h>

#include "depth_frame.h"

namespace stocs {

enum { RENDER_MAX_SPLAT = 16 };

struct RenderArgs {
    float point_radius;
    int max_splat_px, id_base;
};

// the twelve entries the contract reads are finite (false for NaN); P is the same in every lane
__device__ __forceinline__ bool pose_finite(const float* P) {
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 15; ++i)
        if ((i & 3) != 3) finite = finite && (fabsf(P[i]) <= 3.4028234663852886e38f);
    return finite;
}

// the splat rule: half-width in pixels of the square an in_image point at depth z touches
__device__ __forceinline__ int splat_radius(float z, const DepthArgs& a, const RenderArgs& r) {
    return (int)fminf(floorf((a.fx * r.point_radius) / z + 0.5f), (float)r.max_splat_px);
}

// the splat walk: f(row, col) for every pixel of the square of half-width splat_radius around the in_image point p that lies inside the
// image; returns the first and the last row of the square
template <class F>
__device__ __forceinline__ int2 splat_square(const Projected& p, const DepthArgs& a, const RenderArgs& ra, F f) {
    const int s = splat_radius(p.z, a, ra);
    const int r0 = p.row - s > 0 ? p.row - s : 0, r1 = p.row + s < a.H - 1 ? p.row + s : a.H - 1;
    const int c0 = p.col - s > 0 ? p.col - s : 0, c1 = p.col + s < a.W - 1 ? p.col + s : a.W - 1;
    for (int r = r0; r <= r1; ++r)
        for (int c = c0; c <= c1; ++c) f(r, c);
    return make_int2(r0, r1);
}

// steps 5-6 of the depth-check contract for a surface at depth z seen at pixel px: 1 no_depth, 2 agree, 3 in_front, 4 behind, + 16 on_mask
__device__ __forceinline__ int classify_pixel(float z, size_t px, const uint16_t* __restrict__ depth, const uint16_t* __restrict__ prob, const DepthArgs& a) {
    const uint16_t raw = depth[px];
    if (raw == 0) return 1;
    const float zo = (float)raw * a.depth_scale;
    const float d = z - zo;
    if (fabsf(d) <= a.tolerance) {
        if (prob) {
            const float cp = (float)((double)prob[px] * (1.0 / 10000));
            if (!(cp < a.class_threshold)) return 2 + 16;
        }
        return 2;
    }
    if (d < -a.tolerance) return 3;
    if (d > a.tolerance) return 4;
    return 0;   // d is NaN: unreachable, z is a finite p_2 > 1e-6 and zo is finite
}

// ---- host side: the parameter check and the kernel arguments of the render entry points ----
// the two fields the classification reads: all that the mesh forms (render_mesh.hip) read and check of stocs_render_params
static int check_classify_params(const char* who, const stocs_render_params* p) {
    if (!(p->tolerance > 0.0f) || !isfinite(p->tolerance)) { set_error("%s: tolerance %g must be positive and finite", who, (double)p->tolerance); return STOCS_ERR_INVALID; }
    if (!isfinite(p->class_threshold)) { set_error("%s: class_threshold is not finite", who); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}
static int check_params(const char* who, const stocs_render_params* p) {
    if (!(p->point_radius >= 0.0f) || !isfinite(p->point_radius)) { set_error("%s: point_radius %g must be >= 0 and finite", who, (double)p->point_radius); return STOCS_ERR_INVALID; }
    if (p->max_splat_px < 0 || p->max_splat_px > RENDER_MAX_SPLAT) { set_error("%s: max_splat_px %d outside 0..%d", who, p->max_splat_px, (int)RENDER_MAX_SPLAT); return STOCS_ERR_INVALID; }
    return check_classify_params(who, p);
}

static DepthArgs frame_args(const DepthState* S, const stocs_render_params* prm) { return frame_args(S, prm->tolerance, prm->class_threshold); }
static RenderArgs render_args(const stocs_render_params* prm, int id_base) {
    RenderArgs r;
    r.point_radius = prm->point_radius; r.max_splat_px = prm->max_splat_px; r.id_base = id_base;
    return r;
}

}  // namespace stocs

#endif
