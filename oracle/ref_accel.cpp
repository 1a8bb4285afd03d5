/*
 * ref_accel.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT.
 *
 * A C ABI around the reference's two header-only accelerators, compiled UNCHANGED from the reference tree (oracle/Makefile,
 * target _ref/libref_accel.so; -I$(REFERENCE)/include, nothing of it is copied):
 *   super4pcs/accelerators/kdtree.h (+ bbox.h)            build, split, doQueryRestrictedClosestIndex
 *   super4pcs/accelerators/normalset.h/.hpp (+ utils.h)   position and normal cell indexing, _nepsilon, the epsilon correction,
 *                                                         the order of a cell's list
 * Eigen is absent; oracle/eigen_standin/ holds the 3-vector these headers need (its one assumption, the order of the three-term
 * sum, is stated there).  This file includes and calls; it restates nothing.  What it answers is the reference's own code, so
 * tests/test_ref_accel_cpu.py and tests/test_ref_accel_gpu.py can hold oracle/stocs_oracle.cpp and the product to it.
 *
 * Not thread-safe per tree: the reference keeps its query stack in a member (kdtree.h:311), so one tree answers one query at a
 * time.  No OpenMP here.
 */
#include <math.h>
#include <stdint.h>

#include <set>

// kdtree.h includes bbox.h before Eigen/Core, and bbox.h names Eigen::Matrix: the stand-in goes first
#include "Eigen/Core"
#include "Eigen/Geometry"

#include "super4pcs/accelerators/kdtree.h"

// indexPos, indexNormal, _epsilon and _egSize are private members
#define private public
#include "super4pcs/accelerators/normalset.h"
#undef private

namespace {

typedef Super4PCS::KdTree<float> Tree;                     // stocs.hpp: KdTree<Scalar>, Scalar = float
typedef Tree::VectorType Vec;
typedef Super4PCS::IndexedNormalSet<Vec, 3, 7, float> NSet;   // as stocs.cpp:791-796 instantiates it

inline Vec ld(const float* p) { return Vec(p[0], p[1], p[2]); }

struct NSetHandle {
    NSet set;
    int cells;   // _egSize^3: the bound the reference does not test
    explicit NSetHandle(float eps) : set(eps), cells(set._egSize * set._egSize * set._egSize) {}
    bool pos_in_range(const Vec& p) const { const int i = set.indexPos(p); return i >= 0 && i < cells; }
    bool nrm_in_range(const Vec& n) const { const int i = set.indexNormal(n); return i >= 0 && i < 343; }
};

}  // namespace

extern "C" {

/* ---- kd-tree: built as stocs.cpp:973-979 builds it ---- */
void* ref_kd_create(const float* pos3, int n) {
    if (n <= 0 || !pos3) return NULL;   // (finalize() on an empty tree reads mPoints[0])
    Tree* t = new Tree((unsigned)n);
    for (int i = 0; i < n; ++i) t->add(ld(pos3 + 3 * (size_t)i));
    t->finalize();
    return t;
}

void ref_kd_nn(void* h, const float* q3, int nq, float sqdist, int32_t* idx_out) {
    Tree* t = (Tree*)h;
    for (int i = 0; i < nq; ++i)
        idx_out[i] = t ? (int32_t)t->doQueryRestrictedClosestIndex(ld(q3 + 3 * (size_t)i), sqdist) : -1;
}

void ref_kd_free(void* h) { delete (Tree*)h; }

/* ---- normal set ---- */
/* the corrected epsilon (_epsilon) and the grid size (_egSize) of IndexedNormalSet(eps), normalset.h:114-122 */
int ref_nset_params(float eps, int* egSize, float* cell) {
    NSet s(eps);
    if (egSize) *egSize = s._egSize;
    if (cell) *cell = s._epsilon;
    return 0;
}

float ref_nepsilon(void) { return NSet::_nepsilon; }

int ref_index_pos(float eps, const float* p3) { NSet s(eps); return s.indexPos(ld(p3)); }

int ref_index_normal(const float* n3) { NSet s(0.5f); return s.indexNormal(ld(n3)); }   // (the normal cell does not depend on eps)

/* the same for n rows, one set for all of them */
void ref_index_pos_n(float eps, const float* p3, int n, int32_t* out) {
    NSet s(eps);
    for (int i = 0; i < n; ++i) out[i] = s.indexPos(ld(p3 + 3 * (size_t)i));
}
void ref_index_normal_n(const float* n3, int n, int32_t* out) {
    NSet s(0.5f);
    for (int i = 0; i < n; ++i) out[i] = s.indexNormal(ld(n3 + 3 * (size_t)i));
}

/* addElement(pos[i], nrm[i], i) for i = 0..n-1.  An element whose position or normal cell lies outside the grid is left out (the
 * reference does not test the position bound and throws on the normal bound); *n_added receives how many went in. */
void* ref_nset_fill(float eps, const float* pos3, const float* nrm3, int n, int* n_added) {
    NSetHandle* h = new NSetHandle(eps);
    int added = 0;
    for (int i = 0; i < n; ++i) {
        const Vec p = ld(pos3 + 3 * (size_t)i), nn = ld(nrm3 + 3 * (size_t)i);
        if (!h->pos_in_range(p) || !h->nrm_in_range(nn)) continue;
        added += h->set.addElement(p, nn, (unsigned)i) ? 1 : 0;
    }
    if (n_added) *n_added = added;
    return h;
}

/* getNeighbors(p, n) -- one normal cell of p's position cell -- or, with n3 == NULL, getNeighbors(p): the whole position cell.
 * Returns the length of the list and writes its first `cap` ids, in the order the reference stores them. */
int ref_nset_cell(void* hv, const float* p3, const float* n3, uint32_t* out, int cap) {
    NSetHandle* h = (NSetHandle*)hv;
    const Vec p = ld(p3);
    if (!h->pos_in_range(p)) return -1;
    std::vector<unsigned int> nei;
    if (n3) {
        const Vec nn = ld(n3);
        if (!h->nrm_in_range(nn)) return -1;
        h->set.getNeighbors(p, nn, nei);
    } else {
        h->set.getNeighbors(p, nei);
    }
    for (size_t i = 0; i < nei.size() && (int)i < cap; ++i) out[i] = nei[i];
    return (int)nei.size();
}

void ref_nset_free(void* h) { delete (NSetHandle*)h; }

}  // extern "C"
