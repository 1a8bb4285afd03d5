// render_shared.h -- what render_mesh.hip (the joint renderer and the scene footprints on a triangle mesh) takes from the files that
// own the pieces, the way vsd_shared.h serves mesh.hip: render.hip's call layout, pose upload, clear, labels launch and read-back;
// scene.hip's chunk loop with its classify launch behind a z-buffer filler; mesh.hip's rasteriser in its two forms.  Each piece is
// defined once, in the file that owns it, and the splat entry points run through the same ones.
#ifndef STOCS_RENDER_SHARED_H
#define STOCS_RENDER_SHARED_H

#include "render_rules.h"
#include "vsd_shared.h"

namespace stocs {

// ---- render.hip ----
// One call's layout.  The device block holds a key buffer of the context's own first (own_key pixels, 0 for the entry points that work
// on a caller's buffer), then the regions below, then `tail` bytes that stay on the device (o_tail; z-buffers and rectangles of the mesh
// forms); the pinned block mirrors the regions alone, at the same offsets behind PIN_VAR.  Records, labels and state lie one behind the
// other, so one copy reads back whatever a call produced.
struct RenderLayout {
    size_t key_bytes, o_pose, o_res, o_lab, o_state, o_tail, total;
    char* d; char* h;   // bases of the regions on the device and in the pinned block
};
int render_layout(stocs_ctx* c, DevBlock* work, size_t own_key, int n, size_t label_px, size_t tail, RenderLayout* L);
int render_upload_poses(stocs_ctx* c, const RenderLayout& L, const float* poses, int n);
int render_enqueue_clear(stocs_ctx* c, const DepthState* S, void* d_zkey);
// labels and state of the key buffer into the layout's regions; tolerance and class_threshold are all the labels read
int render_enqueue_labels(stocs_ctx* c, const DepthState* S, const RenderLayout& L, float tolerance, float class_threshold, const void* d_zkey);
// one copy of [from, to) of the regions into the pinned block, one synchronisation
int render_read_back(stocs_ctx* c, const RenderLayout& L, size_t from, size_t to);
int render_check_ids(const char* who, int n, int id_base);

// ---- scene.hip ----
// fill(c, self, d_pose, m, a, d_z, d_side) enqueues on c->stream the render of the m poses at d_pose into the m cleared z-buffers at d_z
// (a.W * a.H uint32 float bits each, empty = all ones); d_side: side_bytes per pose of the chunk for the filler's own use (not cleared)
struct SceneFill {
    int (*fill)(stocs_ctx* c, const void* self, const float* d_pose, int m, const DepthArgs& a, uint32_t* d_z, void* d_side);
    const void* self;
    size_t side_bytes;
};
// the body of stocs_scene_footprints behind its argument checks (F: the checked frame; work: the entry point's own block): the chunk
// loop (STOCS_SCENE_CHUNK), the clears, the classify launch, the record read-back
int scene_footprints_with(stocs_ctx* c, DepthState* F, DevBlock* work, const SceneFill& fill, const float* poses, int n, int slot_base, float tolerance,
                          float class_threshold, int claim, void* d_rows, stocs_scene_record* out);
int scene_check_pixels(const char* who, size_t npix);

// ---- mesh.hip ----
int mesh_check_present(const char* who, stocs_ctx* c);
int mesh_triangles(const stocs_ctx* c);
// the m poses at d_pose into their m cleared z-buffers at d_z and their cleared rectangles at d_box (mesh_render_kernel's depth sink)
int mesh_enqueue_depth(stocs_ctx* c, const float* d_pose, int m, const DepthArgs& a, uint32_t* d_z, int32_t* d_box);
// ... all into the ONE key buffer at d_zkey, pose h under id id_base + h (the key sink); d_box as above
int mesh_enqueue_keys(stocs_ctx* c, const float* d_pose, int m, const DepthArgs& a, int id_base, unsigned long long* d_zkey, int32_t* d_box);
// ... pose h into its OWN key buffer at d_zkey + h * npix, the key's low word the winning triangle's index (the triangle-key sink); m <= 65 535
int mesh_enqueue_tri_keys(stocs_ctx* c, const float* d_pose, int m, const DepthArgs& a, unsigned long long* d_zkey, int32_t* d_box);
// the mesh's arrays on the device: float4 vertices (x, y, z, 0), int4 triangles (i0, i1, i2, 0)
void mesh_device_arrays(const stocs_ctx* c, const float4** verts, const int4** tris);

}  // namespace stocs

#endif
