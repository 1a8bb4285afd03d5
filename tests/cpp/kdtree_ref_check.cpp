// kdtree_ref_check.cpp -- the product's host kd-tree (csrc/kdtree.h: kd_build_host, kd_query_closest) next to the reference's own
// header (super4pcs/accelerators/kdtree.h over oracle/eigen_standin), on the two clouds where both run to their limits: 200 coincident
// points (every split degenerate, the recursion ends at depth 32, a leaf of 200) and a collinear cloud with five copies per site.
// A stand-alone host program for the address and undefined-behaviour sanitizers (tests/test_ref_accel_cpu.py builds it with g++
// against the HIP headers; no HIP library call is made, no device is touched, nothing is preloaded).  Prints "kdtree_ref_check: ok".
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

// The tree's construction lives in kdtree.hip next to the context's device copy (ensure_kdtree, stocs_last_tie_counts), which this
// program never calls: the HIP calls of that part are replaced by one stub that ends the program, as tests/cpp/thread_cache_check.cpp
// replaces the allocation calls.
static hipError_t stub_never(...) { fprintf(stderr, "kdtree_ref_check: a HIP call was reached\n"); abort(); }
static const char* stub_error_string(hipError_t) { return "stub"; }
#define hipMalloc stub_never
#define hipFree stub_never
#define hipGetDevice stub_never
#define hipSetDevice stub_never
#define hipMemcpyAsync stub_never
#define hipMemsetAsync stub_never
#define hipStreamSynchronize stub_never
#define hipGetErrorString stub_error_string

#include "kdtree.hip"

namespace stocs {
unsigned long long g_dev_allocs = 0;
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
}  // namespace stocs

// (after the product: the reference's header defines KD_MAX_DEPTH as a macro, the product's an enumerator of that name)
#include "Eigen/Core"
#include "super4pcs/accelerators/kdtree.h"

namespace {

const float H = 1.0f / 512.0f;

int compare(const char* name, const std::vector<float>& pos, const std::vector<float>& q, const std::vector<float>& radii) {
    const int n = (int)(pos.size() / 3), nq = (int)(q.size() / 3);
    Super4PCS::KdTree<float> ref((unsigned)n);
    for (int i = 0; i < n; ++i) ref.add(Super4PCS::KdTree<float>::VectorType(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]));
    ref.finalize();
    stocs::KdTreeHost own;
    stocs::kd_build_host(pos.data(), n, &own);
    int bad = 0, found = 0;
    for (float sq : radii)
        for (int i = 0; i < nq; ++i) {
            const int a = ref.doQueryRestrictedClosestIndex(Super4PCS::KdTree<float>::VectorType(q[3 * i], q[3 * i + 1], q[3 * i + 2]), sq);
            const int b = stocs::kd_query_closest(own.nodes.data(), own.pts.data(), q[3 * i], q[3 * i + 1], q[3 * i + 2], sq);
            if (a != b) {
                if (!bad) printf("%s: query %d (%g %g %g) sqdist %g: reference %d, product %d\n", name, i, q[3 * i], q[3 * i + 1], q[3 * i + 2], sq, a, b);
                ++bad;
            }
            found += a >= 0;
        }
    printf("%s: %d points, %d nodes, %d queries x %d radii, %d found, %d differ\n", name, n, (int)own.nodes.size(), nq, (int)radii.size(), found, bad);
    return bad + (found == 0);
}

}  // namespace

int main() {
    int bad = 0;
    const std::vector<float> radii = {H * H, 0.25f * H * H, 4.0f * H * H, 0.0f};
    {
        std::vector<float> pos(3 * 200, 0.0f);
        const std::vector<float> q = {0, 0, 0, H, 0, 0, 0, 0, -H, 0, H / 2, 0, 1, 1, 1};
        bad += compare("coincident", pos, q, radii);
    }
    {
        std::vector<float> pos, q;
        unsigned s = 12345u;
        for (int i = -40; i <= 40; ++i)
            for (int c = 0; c < 5; ++c) { pos.push_back(i * H); pos.push_back(0.0f); pos.push_back(0.0f); }
        for (int i = (int)(pos.size() / 3) - 1; i > 0; --i) {   // a fixed shuffle of the index order
            s = s * 1664525u + 1013904223u;
            const int j = (int)((s >> 8) % (unsigned)(i + 1));
            for (int k = 0; k < 3; ++k) std::swap(pos[3 * i + k], pos[3 * j + k]);
        }
        for (int i = -82; i <= 82; ++i) {                        // sites and midpoints, on the line and half a cell off it
            q.push_back(i * (H / 2)); q.push_back(0.0f); q.push_back(0.0f);
            q.push_back(i * (H / 2)); q.push_back((i % 3 - 1) * (H / 2)); q.push_back(((i + 1) % 3 - 1) * (H / 2));
        }
        bad += compare("collinear", pos, q, radii);
    }
    if (bad) { printf("kdtree_ref_check: FAILED\n"); return 1; }
    printf("kdtree_ref_check: ok\n");
    return 0;
}
