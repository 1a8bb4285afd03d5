// depth.hip -- depth-image verification of pose hypotheses (stocs_ctx_set_frame, stocs_depth_check_poses): every model point of every
// hypothesis is projected into the frame's own depth image and counted as agreeing, in front of the measured surface (a free-space
// violation), behind it, hidden by the model itself, or without evidence.  No reference counterpart (the reference scores by LCP alone);
// the host restatement it replaces on the hot path is tools/pose_check.py::depth_agreement.  The contract (float order, comparisons,
// z-buffer cells) is written down at the declaration in include/stocs_hip.h.
//
// Per call, everything on the context's stream: the poses go up through the pinned block, ONE launch of depth_check_kernel (a
// workgroup of 256 threads per hypothesis), one copy of the records back into the pinned block, ONE synchronisation.
//
// The kernel walks the model up to three times per hypothesis, in rounds of 256 points, and recomputes the projection in every pass
// (two float4 loads and ~40 float operations per point: cheaper than keeping 65 535 points' worth of state, and the model stays in
// the caches):
//   pass 1 (self-occlusion only)  bounds of the projected pixels: wave min / max by shuffles, then four LDS words;
//   pass 2 (self-occlusion only)  the 64 x 64 z-buffer in LDS: atomicMin on the bits of p_2, which is positive there, so the order of
//                                 the bits is the order of the floats and the minimum does not depend on the execution order;
//   pass 3                        classification: one gathered uint16 of the depth image (and of the class image) per point that is in
//                                 the image and not hidden, classified by classify_pixel (render_rules.h); every count is a __ballot +
//                                 __popcll per wavefront, kept in wave-uniform registers, added to eight LDS words at the end; thread 0
//                                 stores the record.
// The frame's checks, arguments and image pointers are depth_frame.h's (this file owns the frame), pose_finite and classify_pixel are
// render_rules.h's, the wavefront reductions wave_bits.h's, the pinned staging pinned_var (stocs_ctx.h).
// Known limit: one workgroup per hypothesis -- with far fewer hypotheses than compute units the launch is latency-bound.
#include <math.h>
#include <string.h>

#include "render_rules.h"
#include "wave_bits.h"

namespace stocs {

enum { DC_FACING = 0, DC_IN_IMAGE, DC_SELF_OCC, DC_NO_DEPTH, DC_AGREE, DC_IN_FRONT, DC_BEHIND, DC_ON_MASK, DC_COUNTS };

__global__ __launch_bounds__(256) void depth_check_kernel(const float* __restrict__ poses, const float4* __restrict__ mpos, const float4* __restrict__ mnrm, int nM,
                                                          const uint16_t* __restrict__ depth, const uint16_t* __restrict__ prob, DepthArgs a,
                                                          stocs_depth_result* __restrict__ out) {
    __shared__ uint32_t zbuf[64 * 64];
    __shared__ int box[4];              // c0, c1, r0, r1
    __shared__ int cnt[DC_COUNTS];
    const int tid = (int)threadIdx.x;
    const int h = (int)blockIdx.x;
    float P[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = poses[(size_t)h * 16 + i];   // the same address in every lane: uniform loads
    if (tid < DC_COUNTS) cnt[tid] = 0;
    if (!pose_finite(P)) {   // a non-finite pose: a zero record (wave-uniform exit: P is the same in every lane)
        if (tid == 0) {
            stocs_depth_result r;
            r.facing = r.in_image = r.self_occluded = r.no_depth = r.agree = r.in_front = r.behind = r.on_mask = 0;
            r.score = 0.0f; r.violation = 0.0f;
            out[h] = r;
        }
        return;
    }
    const bool zb = a.self_occlusion != 0;
    int c0 = 0, r0 = 0, s = 1;
    bool any_in = false;
    if (zb) {
        for (int i = tid; i < 64 * 64; i += 256) zbuf[i] = 0xFFFFFFFFu;
        if (tid == 0) { box[0] = 0x7FFFFFFF; box[1] = -1; box[2] = 0x7FFFFFFF; box[3] = -1; }
        __syncthreads();
        // pass 1: bounds of the in-image pixels
        int mnc = 0x7FFFFFFF, mxc = -1, mnr = 0x7FFFFFFF, mxr = -1;
        for (int base = 0; base < nM; base += 256) {
            const int i = base + tid;
            if (i < nM) {
                const Projected p = project_point(P, mpos[i], mnrm[i], a);
                if (p.in_image) {
                    mnc = p.col < mnc ? p.col : mnc; mxc = p.col > mxc ? p.col : mxc;
                    mnr = p.row < mnr ? p.row : mnr; mxr = p.row > mxr ? p.row : mxr;
                }
            }
        }
        mnc = wave_min_i(mnc); mxc = wave_max_i(mxc); mnr = wave_min_i(mnr); mxr = wave_max_i(mxr);
        if ((tid & 63) == 0) { atomicMin(&box[0], mnc); atomicMax(&box[1], mxc); atomicMin(&box[2], mnr); atomicMax(&box[3], mxr); }
        __syncthreads();
        c0 = box[0]; r0 = box[2];
        const int c1 = box[1], r1 = box[3];
        any_in = c1 >= c0;   // some point is in the image (then r1 >= r0 too)
        if (any_in) {
            const int ext = (c1 - c0 + 1) > (r1 - r0 + 1) ? (c1 - c0 + 1) : (r1 - r0 + 1);
            const int need = (ext + 63) / 64;
            s = a.cell_px > need ? a.cell_px : need;   // ext <= 64 s: every cell index below stays inside the 64 x 64 grid
            // pass 2: nearest p_2 per cell
            for (int base = 0; base < nM; base += 256) {
                const int i = base + tid;
                if (i < nM) {
                    const Projected p = project_point(P, mpos[i], mnrm[i], a);
                    if (p.in_image) atomicMin(&zbuf[((p.row - r0) / s) * 64 + (p.col - c0) / s], __float_as_uint(p.z));
                }
            }
        }
        __syncthreads();
    } else {
        __syncthreads();   // cnt zeroed
    }
    // pass 3: classification; the loop bounds are wave-uniform, so every __ballot sees the whole wavefront
    int n_face = 0, n_in = 0, n_self = 0, n_nod = 0, n_agree = 0, n_front = 0, n_behind = 0, n_mask = 0;
    for (int base = 0; base < nM; base += 256) {
        const int i = base + tid;
        bool facing = false, in_image = false, self_occ = false;
        int cls = 0;   // steps 5-6: 1 no_depth, 2 agree, 3 in_front, 4 behind, + 16 on_mask
        if (i < nM) {
            const Projected p = project_point(P, mpos[i], mnrm[i], a);
            facing = p.facing; in_image = p.in_image;
            if (in_image) {
                if (zb) {
                    const float zmin = __uint_as_float(zbuf[((p.row - r0) / s) * 64 + (p.col - c0) / s]);
                    self_occ = p.z > zmin + a.margin;
                }
                if (!self_occ) cls = classify_pixel(p.z, (size_t)p.row * (size_t)a.W + (size_t)p.col, depth, prob, a);
            }
        }
        n_face += __popcll(__ballot(facing)); n_in += __popcll(__ballot(in_image)); n_self += __popcll(__ballot(self_occ));
        n_nod += __popcll(__ballot((cls & 15) == 1)); n_agree += __popcll(__ballot((cls & 15) == 2)); n_front += __popcll(__ballot((cls & 15) == 3));
        n_behind += __popcll(__ballot((cls & 15) == 4)); n_mask += __popcll(__ballot((cls & 16) != 0));
    }
    if ((tid & 63) == 0) {
        atomicAdd(&cnt[DC_FACING], n_face); atomicAdd(&cnt[DC_IN_IMAGE], n_in); atomicAdd(&cnt[DC_SELF_OCC], n_self); atomicAdd(&cnt[DC_NO_DEPTH], n_nod);
        atomicAdd(&cnt[DC_AGREE], n_agree); atomicAdd(&cnt[DC_IN_FRONT], n_front); atomicAdd(&cnt[DC_BEHIND], n_behind); atomicAdd(&cnt[DC_ON_MASK], n_mask);
    }
    __syncthreads();
    if (tid == 0) {
        stocs_depth_result r;
        r.facing = cnt[DC_FACING]; r.in_image = cnt[DC_IN_IMAGE]; r.self_occluded = cnt[DC_SELF_OCC]; r.no_depth = cnt[DC_NO_DEPTH];
        r.agree = cnt[DC_AGREE]; r.in_front = cnt[DC_IN_FRONT]; r.behind = cnt[DC_BEHIND]; r.on_mask = cnt[DC_ON_MASK];
        r.score = r.facing > 0 ? (float)r.agree / (float)r.facing : 0.0f;
        r.violation = r.facing > 0 ? (float)r.in_front / (float)r.facing : 0.0f;
        out[h] = r;
    }
}

static int check_params(const stocs_depth_params* p) {
    if (!(p->tolerance > 0.0f) || !isfinite(p->tolerance)) { set_error("stocs_depth_check_poses: tolerance %g must be positive and finite", (double)p->tolerance); return STOCS_ERR_INVALID; }
    if (!isfinite(p->class_threshold)) { set_error("stocs_depth_check_poses: class_threshold is not finite"); return STOCS_ERR_INVALID; }
    if (p->self_occlusion != 0 && p->self_occlusion != 1) { set_error("stocs_depth_check_poses: self_occlusion %d is neither 0 nor 1", p->self_occlusion); return STOCS_ERR_INVALID; }
    if (p->cell_px < 1) { set_error("stocs_depth_check_poses: cell_px %d < 1", p->cell_px); return STOCS_ERR_INVALID; }
    if (!(p->occlusion_margin >= 0.0f) || !isfinite(p->occlusion_margin)) {
        set_error("stocs_depth_check_poses: occlusion_margin %g must be >= 0 and finite", (double)p->occlusion_margin);
        return STOCS_ERR_INVALID;
    }
    return STOCS_OK;
}

}  // namespace stocs

using namespace stocs;

extern "C" void stocs_default_depth_params(stocs_depth_params* p) {
    if (!p) return;
    p->tolerance = 0.01f; p->class_threshold = 0.10f; p->self_occlusion = 1; p->cell_px = 8; p->occlusion_margin = 0.01f;
}

extern "C" int stocs_ctx_set_frame(stocs_ctx* c, const stocs_camera* cam, const uint16_t* depth, const uint16_t* class_prob) {
    if (!c || !cam || !depth) { set_error("stocs_ctx_set_frame: NULL context, camera or depth image"); return STOCS_ERR_INVALID; }
    if (cam->width < 1 || cam->height < 1) { set_error("stocs_ctx_set_frame: image of %d x %d pixels", cam->width, cam->height); return STOCS_ERR_INVALID; }
    DeviceGuard dev_guard(c->device);
    DepthState* S = ctx_state<DepthState>(c);
    const size_t npix = (size_t)cam->width * (size_t)cam->height;
    const size_t img = al256(npix * 2);
    S->has_frame = false;
    { const int rc = S->frame.grow(c->stream, 2 * img); if (rc) return rc; }
    char* hp;
    { const int rc = pinned_var(c, 2 * img, &hp); if (rc) return rc; }
    memcpy(hp, depth, npix * 2);
    if (class_prob) memcpy(hp + img, class_prob, npix * 2);
    STOCS_HIP_CHECK(hipMemcpyAsync(S->frame.p, hp, class_prob ? 2 * img : img, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));   // the pinned block is free for the next call
    S->cam = *cam; S->npix = npix; S->has_prob = class_prob != NULL; S->has_frame = true;
    return STOCS_OK;
}

extern "C" int stocs_depth_check_poses(stocs_ctx* c, const float* poses, int n, const stocs_depth_params* prm, stocs_depth_result* out) {
    if (!c) { set_error("stocs_depth_check_poses: NULL context"); return STOCS_ERR_INVALID; }
    if (n < 0) { set_error("stocs_depth_check_poses: n %d < 0", n); return STOCS_ERR_INVALID; }
    if (n == 0) return STOCS_OK;
    if (!poses || !prm || !out) { set_error("stocs_depth_check_poses: NULL poses, parameters or results"); return STOCS_ERR_INVALID; }
    { const int rc = check_params(prm); if (rc) return rc; }
    DepthState* S = NULL;
    { const int rc = check_frame("stocs_depth_check_poses", c, &S); if (rc) return rc; }
    DeviceGuard dev_guard(c->device);
    Carve cv;
    const size_t o_pose = cv.take((size_t)n * 64), o_res = cv.take((size_t)n * sizeof(stocs_depth_result));
    { const int rc = S->work.grow(c->stream, cv.total); if (rc) return rc; }
    char* hp;   // the pinned mirror of the two regions, at the same offsets
    { const int rc = pinned_var(c, cv.total, &hp); if (rc) return rc; }
    float* d_pose = Carve::at<float>(S->work.p, o_pose);
    stocs_depth_result* d_res = Carve::at<stocs_depth_result>(S->work.p, o_res);
    float* h_pose = Carve::at<float>(hp, o_pose);
    stocs_depth_result* h_res = Carve::at<stocs_depth_result>(hp, o_res);
    memcpy(h_pose, poses, (size_t)n * 64);
    STOCS_HIP_CHECK(hipMemcpyAsync(d_pose, h_pose, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
    DepthArgs a = frame_args(S, prm->tolerance, prm->class_threshold);
    a.margin = prm->occlusion_margin; a.self_occlusion = prm->self_occlusion; a.cell_px = prm->cell_px;
    hipLaunchKernelGGL(depth_check_kernel, dim3((unsigned)n), dim3(256), 0, c->stream, (const float*)d_pose, (const float4*)c->d_mpos_raw, (const float4*)c->d_mnrm,
                       c->nM, frame_depth(S), frame_prob(S), a, d_res);
    STOCS_HIP_CHECK(hipGetLastError());
    STOCS_HIP_CHECK(hipMemcpyAsync(h_res, d_res, (size_t)n * sizeof(stocs_depth_result), hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    memcpy(out, h_res, (size_t)n * sizeof(stocs_depth_result));
    return STOCS_OK;
}
