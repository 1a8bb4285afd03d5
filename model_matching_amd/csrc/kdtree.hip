// kdtree.hip -- host construction of the reference-order kd-tree (kdtree.h), its device copy for the "exact_ties" mode, and the
// host entry point stocs_kdtree_nn_host (tests).
#include <string.h>

#include "kdtree.h"
#include "stocs_ctx.h"

namespace stocs {

namespace {

struct KdBuilder {
    std::vector<float> p;        // xyz per point, physically partitioned as the reference partitions mPoints
    std::vector<int32_t> idx;    // mIndices
    std::vector<KdNodeP> nodes;

    float at(int i, unsigned dim) const { return p[3 * (size_t)i + dim]; }
    void swap_pts(int a, int b) {
        for (int k = 0; k < 3; ++k) std::swap(p[3 * (size_t)a + k], p[3 * (size_t)b + k]);
        std::swap(idx[a], idx[b]);
    }

    // the in-place partition of kdtree.h:522-538: points below the split value to the front; the physical order it leaves inside a
    // leaf decides which of two tied points the query visits last
    unsigned split(int start, int end, unsigned dim, float split_value) {
        int l = start, r = end - 1;
        for (; l < r; ++l, --r) {
            while (l < end && at(l, dim) < split_value) l++;
            while (r >= start && at(r, dim) >= split_value) r--;
            if (l > r) break;
            swap_pts(l, r);
        }
        // (l == end only when every point lies below the midpoint of its own box, which finite coordinates never give; the reference
        //  would read one past the range there)
        return (unsigned)((l < end && at(l, dim) < split_value) ? l + 1 : l);
    }

    // createTree (kdtree.h:560-641): the points' box, the widest axis (first maximum of the half diagonal), its midpoint as the split
    void create(unsigned node_id, unsigned start, unsigned end, unsigned level) {
        const float big = 3.40282347e38f / 2;   // AABB(): min = max() / 2, max = -max() / 2 (bbox.h:65-66)
        float mn[3] = {big, big, big}, mx[3] = {-big, -big, -big};
        for (unsigned i = start; i < end; ++i)
            for (int k = 0; k < 3; ++k) {
                const float v = at((int)i, (unsigned)k);
                if (v < mn[k]) mn[k] = v;
                if (v > mx[k]) mx[k] = v;
            }
        float diag[3];
        for (int k = 0; k < 3; ++k) diag[k] = 0.5f * (mx[k] - mn[k]);
        unsigned dim = 0;
        if (diag[1] > diag[dim]) dim = 1;
        if (diag[2] > diag[dim]) dim = 2;
        const float split_value = mn[dim] + ((mx[dim] - mn[dim]) / 2.0f);   // AABB::center (bbox.h:91-92)
        nodes[node_id].split = split_value;
        nodes[node_id].dim = dim;
        const unsigned mid = split((int)start, (int)end, dim, split_value);
        const unsigned first = (unsigned)nodes.size();
        nodes[node_id].first = first;
        nodes.push_back(KdNodeP{0.f, 0u, 0u, 0u});
        nodes.push_back(KdNodeP{0.f, 0u, 0u, 0u});
        const unsigned lo[2] = {start, mid}, hi[2] = {mid, end};
        for (int c = 0; c < 2; ++c) {
            const unsigned child = first + (unsigned)c;
            if (hi[c] - lo[c] <= (unsigned)KD_POINTS_PER_CELL || level >= (unsigned)KD_MAX_DEPTH) {
                nodes[child].dim = KD_LEAF;
                nodes[child].first = lo[c];
                nodes[child].size = hi[c] - lo[c];
            } else {
                create(child, lo[c], hi[c], level + 1);
            }
        }
    }
};

}  // namespace

void kd_build_host(const float* pos3, int n, KdTreeHost* t) {
    t->nodes.clear();
    t->pts.clear();
    if (n <= 0) return;
    KdBuilder b;
    b.p.assign(pos3, pos3 + 3 * (size_t)n);
    b.idx.resize((size_t)n);
    for (int i = 0; i < n; ++i) b.idx[i] = i;
    b.nodes.reserve(4 * (size_t)n / KD_POINTS_PER_CELL + 16);
    b.nodes.push_back(KdNodeP{0.f, 0u, 0u, 0u});   // the root is always split (finalize: createTree(0, 0, n, 1))
    b.create(0, 0, (unsigned)n, 1);
    t->nodes.swap(b.nodes);
    t->pts.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        int32_t id = b.idx[i];
        float w;
        memcpy(&w, &id, 4);
        t->pts[i] = make_float4(b.p[3 * (size_t)i], b.p[3 * (size_t)i + 1], b.p[3 * (size_t)i + 2], w);
    }
}

// The context's tree for its current scene (exact_ties): built on the host from the centred scene positions -- the coordinates the
// reference's kdtree_initialize sees after centroid_shift (stocs.cpp:966-980) -- and copied to the device behind the tie counters.
// One grow-only device block: a scene no larger than any before it allocates nothing.  Synchronises the context's stream.
int ensure_kdtree(stocs_ctx* c) {
    if (c->kd_ready) return STOCS_OK;
    std::vector<float> p3((size_t)c->nS * 3);
    for (int i = 0; i < c->nS; ++i) { p3[3 * (size_t)i] = c->h_spos[i].x; p3[3 * (size_t)i + 1] = c->h_spos[i].y; p3[3 * (size_t)i + 2] = c->h_spos[i].z; }
    kd_build_host(p3.data(), c->nS, &c->kd_host);
    const size_t nb = al256(c->kd_host.nodes.size() * sizeof(KdNodeP)), pb = c->kd_host.pts.size() * sizeof(float4);
    const size_t need = 256 + nb + pb;
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));   // nothing may still read the old tree (nor the counters)
    const size_t had = c->kd.bytes;
    { const int rc = c->kd.grow(c->stream, need); if (rc) return rc; }
    if (c->kd.bytes != had) STOCS_HIP_CHECK(hipMemsetAsync(c->kd.p, 0, 256, c->stream));   // a new block: the counters start at 0
    c->d_ties = (unsigned long long*)c->kd.p;
    c->d_kd_nodes = c->kd_host.nodes.empty() ? NULL : (const KdNodeP*)(c->kd.p + 256);
    c->d_kd_pts = (const float4*)(c->kd.p + 256 + nb);
    if (nb) STOCS_HIP_CHECK(hipMemcpyAsync(c->kd.p + 256, c->kd_host.nodes.data(), c->kd_host.nodes.size() * sizeof(KdNodeP), hipMemcpyHostToDevice, c->stream));
    if (pb) STOCS_HIP_CHECK(hipMemcpyAsync(c->kd.p + 256 + nb, c->kd_host.pts.data(), pb, hipMemcpyHostToDevice, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));   // (pageable sources)
    c->kd_ready = true;
    return STOCS_OK;
}

}  // namespace stocs

using namespace stocs;

extern "C" {

int stocs_kdtree_nn_host(const float* pos3, int n, const float* q3, int nq, float sqdist, int32_t* idx) {
    if (n < 0 || nq < 0 || (n && !pos3) || (nq && (!q3 || !idx))) { set_error("stocs_kdtree_nn_host: invalid argument"); return STOCS_ERR_INVALID; }
    KdTreeHost t;
    kd_build_host(pos3, n, &t);
    const KdNodeP* nodes = t.nodes.empty() ? NULL : t.nodes.data();
    for (int i = 0; i < nq; ++i) idx[i] = kd_query_closest(nodes, t.pts.data(), q3[3 * (size_t)i], q3[3 * (size_t)i + 1], q3[3 * (size_t)i + 2], sqdist);
    return STOCS_OK;
}

int stocs_last_tie_counts(stocs_ctx* c, int64_t* flagged, int64_t* changed) {
    if (!c || !flagged || !changed) return STOCS_ERR_INVALID;
    *flagged = 0; *changed = 0;
    if (!c->ties_started || !c->d_ties) return STOCS_OK;
    DeviceGuard dev_guard(c->device);
    unsigned long long h[2] = {0ull, 0ull};
    STOCS_HIP_CHECK(hipMemcpyAsync(h, c->d_ties, 16, hipMemcpyDeviceToHost, c->stream));
    STOCS_HIP_CHECK(hipStreamSynchronize(c->stream));
    *flagged = (int64_t)h[0]; *changed = (int64_t)h[1];
    return STOCS_OK;
}

}  // extern "C"
