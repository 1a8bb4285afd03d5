// vsd_shared.h -- what vsd.hip (surfels) and mesh.hip (triangles) share: the z-buffer protocol of a rendered pose and the two call bodies
// of vsd.hip behind a renderer.  A renderer only fills z-buffers; the chunking (STOCS_VSD_CHUNK), the per-pose rectangle slots, the clears,
// the compare launch (vsd_compare_kernel, vsd.hip's own) and the record read-back are vsd.hip's and the same for both.
#ifndef STOCS_VSD_SHARED_H
#define STOCS_VSD_SHARED_H

#include "depth_frame.h"

namespace stocs {

// A rendered pose's bounding rectangle, the union of its surfels' clipped squares (of its triangles' clamped boxes), as four maxima
// (-c0, c1, -r0, r1) so that one byte pattern clears it (0x80: every entry far below any pixel) and one atomicMax per entry and
// wavefront fills it.  Nothing rendered: it stays cleared, and c1 < c0.
enum { VB_NEG_C0 = 0, VB_C1, VB_NEG_R0, VB_R1, VSD_BOX_WORDS = 4 };

__device__ __forceinline__ float lane_f(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
__device__ __forceinline__ int lane_i(int v, int src) { return __builtin_amdgcn_readlane(v, src); }

// render(c, self, d_pose, m, a, d_z, d_box) enqueues on c->stream the render of the m poses at d_pose (16 floats each) into the m cleared
// z-buffers at d_z (a.W * a.H uint32 float bits each, empty = all ones, a minimum per pixel) and their cleared rectangles at d_box
struct VsdRenderer {
    int (*render)(stocs_ctx* c, const void* self, const float* d_pose, int m, const DepthArgs& a, uint32_t* d_z, int32_t* d_box);
    const void* self;
};

// the bodies of stocs_render_depth and stocs_pose_errors_vsd behind their argument checks (F: the checked frame; timing_slot: the
// CallTiming of the context that the call records into)
int vsd_render_depth_with(stocs_ctx* c, DepthState* F, const VsdRenderer& rd, const float* poses, int n, float* depth);
int vsd_pose_errors_with(stocs_ctx* c, DepthState* F, TimingSlot timing_slot, const VsdRenderer& rd, const float* est, int n, const float* gt, int n_gt,
                         const stocs_vsd_params* prm, stocs_vsd_record* out);
// delta, n_tau and the taus of stocs_vsd_params as stocs_check_vsd_params judges them (not the two surfel fields)
int vsd_check_compare_params(const char* who, const stocs_vsd_params* p);

}  // namespace stocs

#endif
