"""ctypes binding of oracle/_ref/libref_accel.so -- TEST INFRASTRUCTURE, NOT PRODUCT.

The library is the reference's own kd-tree and normal-set headers, compiled unchanged behind oracle/ref_accel.cpp (oracle/Makefile builds
it where the reference tree is at hand).  At run time only the library is read, never the reference tree.  Only tests/ may
import this module.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(_HERE, "_ref", "libref_accel.so")
_LIB = None


def reference_dir() -> str:
    """where oracle/Makefile looks for the reference tree (its REFERENCE variable)"""
    return os.environ.get("REFERENCE", "/root/reference")


def reference_present() -> bool:
    return os.path.exists(os.path.join(reference_dir(), "include", "super4pcs", "accelerators", "kdtree.h"))


def available() -> bool:
    return os.path.exists(SO)


def lib():
    global _LIB
    if _LIB is None:
        if not available():
            raise RuntimeError("%s is missing: run `make -C oracle` on a machine that has the reference tree (%s)" % (SO, reference_dir()))
        L = C.CDLL(SO)
        fp, ip, vp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p
        L.ref_kd_create.argtypes = [fp, C.c_int]
        L.ref_kd_create.restype = vp
        L.ref_kd_nn.argtypes = [vp, fp, C.c_int, C.c_float, ip]
        L.ref_kd_nn.restype = None
        L.ref_kd_free.argtypes = [vp]
        L.ref_kd_free.restype = None
        L.ref_nset_params.argtypes = [C.c_float, C.POINTER(C.c_int), fp]
        L.ref_nepsilon.argtypes = []
        L.ref_nepsilon.restype = C.c_float
        L.ref_index_pos.argtypes = [C.c_float, fp]
        L.ref_index_pos.restype = C.c_int
        L.ref_index_normal.argtypes = [fp]
        L.ref_index_normal.restype = C.c_int
        L.ref_index_pos_n.argtypes = [C.c_float, fp, C.c_int, ip]
        L.ref_index_pos_n.restype = None
        L.ref_index_normal_n.argtypes = [fp, C.c_int, ip]
        L.ref_index_normal_n.restype = None
        L.ref_nset_fill.argtypes = [C.c_float, fp, fp, C.c_int, C.POINTER(C.c_int)]
        L.ref_nset_fill.restype = vp
        L.ref_nset_cell.argtypes = [vp, fp, fp, C.POINTER(C.c_uint32), C.c_int]
        L.ref_nset_cell.restype = C.c_int
        L.ref_nset_free.argtypes = [vp]
        L.ref_nset_free.restype = None
        _LIB = L
    return _LIB


def _f(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


class KdTree:
    """Super4PCS::KdTree<float> over pos (n, 3), built as the reference's kdtree_initialize builds it.  One query at a time."""

    def __init__(self, pos):
        self.pos, pp = _f(np.asarray(pos, np.float32).reshape(-1, 3))
        assert len(self.pos) > 0
        self.h = lib().ref_kd_create(pp, len(self.pos))

    def nn(self, queries, sqdist):
        """doQueryRestrictedClosestIndex per row of queries (q, 3): scene indices, -1 for none"""
        q, pq = _f(np.asarray(queries, np.float32).reshape(-1, 3))
        out = np.full(max(len(q), 1), -2, np.int32)
        lib().ref_kd_nn(self.h, pq, len(q), float(sqdist), out.ctypes.data_as(C.POINTER(C.c_int32)))
        return out[:len(q)]

    def close(self):
        if self.h:
            lib().ref_kd_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NormalSet:
    """IndexedNormalSet<Vector3f, 3, 7, float>(eps) filled with addElement(pos[i], nrm[i], i) in index order"""

    def __init__(self, eps, pos, nrm):
        self.pos, pp = _f(np.asarray(pos, np.float32).reshape(-1, 3))
        self.nrm, pn = _f(np.asarray(nrm, np.float32).reshape(-1, 3))
        assert len(self.pos) == len(self.nrm)
        k = C.c_int(0)
        self.h = lib().ref_nset_fill(float(eps), pp, pn, len(self.pos), C.byref(k))
        self.n_added = k.value

    def cell(self, p3, n3=None):
        """getNeighbors(p, n), or getNeighbors(p) when n3 is None: the ids in the order the reference stores them"""
        p, pp = _f(p3)
        pn = None
        if n3 is not None:
            n, pn = _f(n3)
        out = np.zeros(max(len(self.pos), 1), np.uint32)
        k = lib().ref_nset_cell(self.h, pp, pn, out.ctypes.data_as(C.POINTER(C.c_uint32)), len(out))
        assert 0 <= k <= len(out), k
        return out[:k]

    def close(self):
        if self.h:
            lib().ref_nset_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RefAccel:
    """The reference's accelerators: kd-trees, normal sets and the stateless cell functions."""

    def __init__(self):
        self.L = lib()

    def kdtree(self, pos) -> KdTree:
        return KdTree(pos)

    def normalset(self, eps, pos, nrm) -> NormalSet:
        return NormalSet(eps, pos, nrm)

    def nset_params(self, eps):
        """(_egSize, _epsilon) after the power-of-two correction of the constructor"""
        g = C.c_int(0); c = C.c_float(0)
        self.L.ref_nset_params(float(eps), C.byref(g), C.byref(c))
        return g.value, c.value

    def nepsilon(self):
        return self.L.ref_nepsilon()

    def index_pos(self, eps, p3):
        p, pp = _f(p3)
        return self.L.ref_index_pos(float(eps), pp)

    def index_normal(self, n3):
        n, pn = _f(n3)
        return self.L.ref_index_normal(pn)

    def index_pos_rows(self, eps, p):
        p, pp = _f(np.asarray(p, np.float32).reshape(-1, 3))
        out = np.zeros(max(len(p), 1), np.int32)
        self.L.ref_index_pos_n(float(eps), pp, len(p), out.ctypes.data_as(C.POINTER(C.c_int32)))
        return out[:len(p)]

    def index_normal_rows(self, n):
        n, pn = _f(np.asarray(n, np.float32).reshape(-1, 3))
        out = np.zeros(max(len(n), 1), np.int32)
        self.L.ref_index_normal_n(pn, len(n), out.ctypes.data_as(C.POINTER(C.c_int32)))
        return out[:len(n)]
