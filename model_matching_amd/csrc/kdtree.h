// kdtree.h -- the reference's kd-tree in its own visiting order, for the opt-in "exact_ties" mode of the scoring kernels.
//
// The scan kernels answer the radius-epsilon nearest-neighbour query of LCP verification from the scene grid and break an exact
// float32 distance tie towards the larger scene index (lcp.hip, take_if_better).  The reference's KdTree::doQueryRestrictedClosestIndex
// (include/super4pcs/accelerators/kdtree.h:394-459) keeps the point it visits LAST among the tied ones (`<=` at :424), and its
// visiting order follows the tree's in-place partition and its stack discipline (divergence Q11).  In exact mode the
// scoring kernels send every tied query here.  The tree is built on the host exactly as the reference builds it (construction below);
// the query is one __host__ __device__ function, so the host entry point stocs_kdtree_nn_host runs the very code the device runs.
#ifndef STOCS_KDTREE_H
#define STOCS_KDTREE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace stocs {

enum { KD_POINTS_PER_CELL = 64, KD_MAX_DEPTH = 32, KD_STACK = 64 };   // kdtree.h:60,63 and the member stack mNodeStack[64]

// one node, 16 bytes: an inner node holds its split value, split axis (0-2) and the id of its first child (the second child
// follows it); a leaf (axis word KD_LEAF) holds the range [start, start + size) of its points in tree order
enum : uint32_t { KD_LEAF = 3u };
struct KdNodeP {
    float split;
    uint32_t dim;     // 0, 1, 2 or KD_LEAF
    uint32_t first;   // inner: first child id; leaf: start
    uint32_t size;    // leaf: number of points
};

// doQueryRestrictedClosestIndex restated: the explicit (node, sq) stack, "replace the top by one child, push the other", pruning on
// qnode.sq < cl_dist (strict), acceptance on sqdist <= cl_dist (inclusive: the point visited last wins a tie).  pts: positions in
// tree order with the original scene index in w.  The squared norm is evaluated as the scan kernels and the oracle evaluate it
// (x^2 + (y^2 + z^2), no contraction: the library is built with -ffp-contract=off).  Returns the original index, -1 for none.
__host__ __device__ inline int kd_query_closest(const KdNodeP* __restrict__ nodes, const float4* __restrict__ pts, float qx, float qy, float qz,
                                                float sqdist) {
    if (!nodes) return -1;
    uint32_t st_node[KD_STACK];
    float st_sq[KD_STACK];
    int cl_id = -1;
    float cl_dist = sqdist;
    st_node[0] = 0u;
    st_sq[0] = 0.f;
    unsigned count = 1;
    while (count) {
        const unsigned top = count - 1;
        const KdNodeP node = nodes[st_node[top]];
        if (st_sq[top] < cl_dist) {
            if (node.dim == KD_LEAF) {
                --count;   // pop
                const int end = (int)(node.first + node.size);
                for (int i = (int)node.first; i < end; ++i) {
                    const float4 p = pts[i];
                    const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
                    const float d = dx * dx + (dy * dy + dz * dz);
                    if (d <= cl_dist) {
                        cl_dist = d;
                        cl_id = __builtin_bit_cast(int, p.w);
                    }
                }
            } else {
                const float qd = node.dim == 0 ? qx : (node.dim == 1 ? qy : qz);
                const float new_off = qd - node.split;
                // the stack top becomes the far child, the near child goes on top of it
                if (new_off < 0.) {
                    st_node[count] = node.first;
                    st_node[top] = node.first + 1u;
                } else {
                    st_node[count] = node.first + 1u;
                    st_node[top] = node.first;
                }
                st_sq[count] = st_sq[top];
                st_sq[top] = new_off * new_off;
                ++count;
            }
        } else {
            --count;   // pop
        }
    }
    return cl_id;
}

// the tree on the host: nodes and the points in tree order (xyz, original index bits in w)
struct KdTreeHost {
    std::vector<KdNodeP> nodes;
    std::vector<float4> pts;
};
// KdTree(n), add() of every point in index order, finalize() (kdtree.h:355-370, 522-641); n == 0 gives an empty tree
void kd_build_host(const float* pos3, int n, KdTreeHost* t);

}  // namespace stocs

#endif
