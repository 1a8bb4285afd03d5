// eval_call.h -- the host frame that the pose-evaluation entry points share (pose_error.hip, pose_error_sym.hip, symmetry.hip, vsd.hip and
// the VSD entry points of mesh.hip): the argument refusals of a batch of pose pairs, step 5's validity rule on the host and the
// fixed-point mean of the record loops, and TimedCall, which owns the CallTiming record of one such call.  Host code only, a header of its
// own rather than a part of pose_error_math.h: that one is the arithmetic the kernels share.  DESIGN.md 7.20.
#ifndef STOCS_EVAL_CALL_H
#define STOCS_EVAL_CALL_H

#include <math.h>

#include "stocs_ctx.h"

namespace stocs {

// ---- refusals, in the order documented at the entry points (include/stocs_hip.h) ----
// A NULL context and n < 0 are STOCS_ERR_INVALID; n == 0 then ends the call with STOCS_OK.  True: the call ends here with *rc
static bool check_batch(const char* who, const stocs_ctx* c, int n, int* rc) {
    *rc = STOCS_ERR_INVALID;
    if (!c) { set_error("%s: NULL context", who); return true; }
    if (n < 0) { set_error("%s: n %d < 0", who, n); return true; }
    *rc = STOCS_OK;
    return n == 0;
}
// ... with n > 0: the (est, gt, n_gt, out) of n pairs against one ground truth or n
static int check_pairs(const char* who, const void* est, int n, const void* gt, int n_gt, const void* out) {
    if (!est || !gt || !out) { set_error("%s: NULL estimates, ground truth or results", who); return STOCS_ERR_INVALID; }
    if (n_gt != 1 && n_gt != n) { set_error("%s: n_gt %d is neither 1 nor n = %d", who, n_gt, n); return STOCS_ERR_INVALID; }
    return STOCS_OK;
}
static int check_model(const char* who, const stocs_ctx* c) {
    if (c->nM < 1) { set_error("%s: the context has no model", who); return STOCS_ERR_STATE; }
    return STOCS_OK;
}

// ---- the record loops ----
static bool host_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }
// the twelve used entries of a 16-float pose are finite
static bool host_pose_finite(const float* P) {
    for (int i = 0; i < 15; ++i)
        if ((i & 3) != 3 && !host_finite(P[i])) return false;
    return true;
}
// the index of the first of n poses that is not, -1: none (what the refusals of a set of transforms name)
static int first_nonfinite_pose(const float* poses, int n) {
    int k = 0;
    while (k < n && host_pose_finite(poses + (size_t)k * 16)) ++k;
    return k < n ? k : -1;
}
static bool host_pose_zero(const float* P) {
    for (int i = 0; i < 16; ++i)
        if (!(P[i] == 0.0f)) return false;
    return true;
}
// the ground truth of pair k
static const float* pair_gt(const float* gt, int n_gt, int k) { return gt + (size_t)(n_gt == 1 ? 0 : k) * 16; }
// step 5 of stocs_pose_errors, the host twin of the kernels' pe_pose_finite / pe_pose_zero test (pose_error_math.h)
static bool pair_valid(const float* est, const float* gt, int n_gt, int k) {
    const float* P = est + (size_t)k * 16;
    return first_nonfinite_pose(P, 1) < 0 && first_nonfinite_pose(pair_gt(gt, n_gt, k), 1) < 0 && !host_pose_zero(P);
}
// the mean of M terms from their 32.32 fixed-point sum
static float fix_mean(uint64_t fix, int M) { return (float)((double)fix / 4294967296.0 / (double)M); }

// The CallTiming record of one evaluation call and, with the "device_clock" option on, the HIP-event time of its launches.  Made at the
// call's entry; start() once nothing can refuse the call any more (a refused call leaves the last call's record as it was), the first
// step still counted from the entry; device_begin() / device_end() around the launches; enqueued_wait() in place of the synchronisation;
// finish() behind the record loop.
struct TimedCall {
    stocs_ctx* c; CallTiming& tm; const double t_entry; const bool dev_clock;
    // dev_clock is opt-in: an event between two operations of a stream leaves the queue idle for a few microseconds
    TimedCall(stocs_ctx* ctx, TimingSlot slot) : c(ctx), tm(ctx->timing[slot]), t_entry(CallTiming::now_s()), dev_clock(ctx->device_clock != 0) {}
    void start() { tm.begin(); tm.t_last = t_entry; }
    int mark(hipEvent_t ev) { if (dev_clock) STOCS_HIP_CHECK(hipEventRecord(ev, c->stream)); return STOCS_OK; }
    int device_begin() { return mark(c->ev0); }
    int device_end() { return mark(c->ev1); }
    int enqueued_wait() {
        tm.lap("stage and enqueue");
        STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
        tm.lap("wait for the device");
        return STOCS_OK;
    }
    int finish() {
        tm.lap("records");
        if (dev_clock) {
            float ms = 0.0f;
            STOCS_HIP_CHECK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
            tm.label[tm.n] = "device: kernel"; tm.ms[tm.n] = (double)ms; ++tm.n;
        }
        return STOCS_OK;
    }
};

}  // namespace stocs

#endif
