// depth_frame.h -- what the entry points that work on the frame of stocs_ctx_set_frame share: the frame's state on the context
// (depth.hip owns it: stocs_ctx_set_frame fills it, the context's registry deletes it), the kernel arguments that describe the camera,
// steps 1-3 of the depth-check contract (include/stocs_hip.h), and on the host the checks of the frame, the fill of the arguments and the
// pointers to its two images.  Included through render_rules.h by depth.hip (stocs_depth_check_poses), render.hip (stocs_render_poses and
// its kin) and scene.hip (stocs_scene_footprints); all project a model point with the one project_point below.
#ifndef STOCS_DEPTH_FRAME_H
#define STOCS_DEPTH_FRAME_H

#include "stocs_ctx.h"

namespace stocs {

struct DepthState {
    static const StateOwner OWNER = OWN_DEPTH;
    DevBlock frame;   // depth (npix uint16) | class probabilities (npix uint16), grow-only
    DevBlock work;    // poses (n x 16 float) | records (n x stocs_depth_result), grow-only
    bool has_frame = false, has_prob = false;
    size_t npix = 0;  // pixels uploaded
    stocs_camera cam = {};
    ~DepthState() { frame.free(); work.free(); }
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

// ---- host side: the frame as every entry point on it requires it, and the kernel arguments from it ----
static int check_frame(const char* who, stocs_ctx* c, DepthState** frame) {
    DepthState* S = ctx_state_if<DepthState>(c);
    if (!S || !S->has_frame) { set_error("%s: no frame (stocs_ctx_set_frame)", who); return STOCS_ERR_STATE; }
    if (S->cam.width < 1 || S->cam.height < 1) { set_error("%s: image of %d x %d pixels", who, S->cam.width, S->cam.height); return STOCS_ERR_INVALID; }
    if ((size_t)S->cam.width * (size_t)S->cam.height != S->npix) {
        set_error("%s: the camera's %d x %d pixels are not the %zu uploaded", who, S->cam.width, S->cam.height, S->npix);
        return STOCS_ERR_STATE;
    }
    *frame = S;
    return STOCS_OK;
}

// the camera and the two thresholds; no self-occlusion test (margin 0, one pixel per cell) unless the caller sets those three fields
static DepthArgs frame_args(const DepthState* S, float tolerance, float class_threshold) {
    DepthArgs a;
    a.fx = S->cam.fx; a.cx = S->cam.cx; a.fy = S->cam.fy; a.cy = S->cam.cy; a.depth_scale = S->cam.depth_scale; a.W = S->cam.width; a.H = S->cam.height;
    a.tolerance = tolerance; a.class_threshold = class_threshold; a.margin = 0.0f; a.self_occlusion = 0; a.cell_px = 1;
    return a;
}
static const uint16_t* frame_depth(const DepthState* S) { return (const uint16_t*)S->frame.p; }
static const uint16_t* frame_prob(const DepthState* S) { return S->has_prob ? (const uint16_t*)(S->frame.p + al256(S->npix * 2)) : (const uint16_t*)NULL; }

}  // namespace stocs

#endif
