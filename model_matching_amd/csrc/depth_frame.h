// depth_frame.h -- what the entry points that work on the frame of stocs_ctx_set_frame share: the frame's state on the context
// (depth.hip owns it: stocs_ctx_set_frame fills it, stocs_internal_free_depth frees it), the kernel arguments that describe the camera,
// and steps 1-3 of the depth-check contract (include/stocs_hip.h).  Included by depth.hip (stocs_depth_check_poses) and, through
// render_rules.h, by render.hip (stocs_render_poses and its kin) and scene.hip (stocs_scene_footprints); all project a model point with the
// one project_point below.
#ifndef STOCS_DEPTH_FRAME_H
#define STOCS_DEPTH_FRAME_H

#include "stocs_ctx.h"

namespace stocs {

struct DepthState {
    DevBlock frame;   // depth (npix uint16) | class probabilities (npix uint16), grow-only
    DevBlock work;    // poses (n x 16 float) | records (n x stocs_depth_result), grow-only
    bool has_frame, has_prob;
    size_t npix;      // pixels uploaded
    stocs_camera cam;
};

struct DepthArgs {
    float fx, cx, fy, cy, depth_scale;
    int W, H;
    float tolerance, class_threshold, margin;
    int self_occlusion, cell_px;
};

// steps 1-3 of the contract for model point i under pose P (wave-uniform, in scalar registers): facing, in_image, p_2, col, row
struct Projected { bool facing, in_image; float z; int col, row; };
__device__ __forceinline__ Projected project_point(const float* P, const float4 m, const float4 k, const DepthArgs& a) {
    Projected r;
    const float p0 = (P[0] * m.x + (P[4] * m.y + P[8] * m.z)) + P[12];
    const float p1 = (P[1] * m.x + (P[5] * m.y + P[9] * m.z)) + P[13];
    const float p2 = (P[2] * m.x + (P[6] * m.y + P[10] * m.z)) + P[14];
    const float q0 = P[0] * k.x + (P[4] * k.y + P[8] * k.z);
    const float q1 = P[1] * k.x + (P[5] * k.y + P[9] * k.z);
    const float q2 = P[2] * k.x + (P[6] * k.y + P[10] * k.z);
    r.facing = (q0 * p0 + (q1 * p1 + q2 * p2)) < 0.0f && p2 > 1e-6f;
    const float u = floorf(((a.fx * p0) / p2 + a.cx) + 0.5f);
    const float v = floorf(((a.fy * p1) / p2 + a.cy) + 0.5f);
    r.in_image = r.facing && u >= 0.0f && u < (float)a.W && v >= 0.0f && v < (float)a.H;
    r.z = p2;
    r.col = r.in_image ? (int)u : 0;
    r.row = r.in_image ? (int)v : 0;
    return r;
}

}  // namespace stocs

#endif
