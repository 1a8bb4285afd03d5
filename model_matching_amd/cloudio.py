"""Flat cloud files (.stcl) consumed by the C++ driver model_matching_amd/apps/stocs_single.cpp.

Layout: 8-byte magic "STOCSCL1", int32 n, int32 flags (bit 0: class probability present, bit 1:
pixels present), float32 pos[3n], float32 nrm[3n], [float32 prob[n]], [int32 pixel[2n]].
These replace the reference's PLY / PNG / Boost-archive inputs (out of the hot-path scope).

Triangle meshes travel as PLY: read_ply_mesh / write_ply_mesh go through the library's own reader and writer
(stocs_ply_read_mesh, stocs_ply_write_mesh)."""
import ctypes as C
import struct

import numpy as np

MAGIC = b"STOCSCL1"


def write_stcl(path, pos, nrm, prob=None, pixel=None):
    pos = np.ascontiguousarray(pos, np.float32)
    nrm = np.ascontiguousarray(nrm, np.float32)
    n = len(pos)
    flags = (1 if prob is not None else 0) | (2 if pixel is not None else 0)
    with open(path, "wb") as f:
        f.write(MAGIC)
        f.write(struct.pack("<ii", n, flags))
        f.write(pos.tobytes())
        f.write(nrm.tobytes())
        if prob is not None:
            f.write(np.ascontiguousarray(prob, np.float32).tobytes())
        if pixel is not None:
            f.write(np.ascontiguousarray(pixel, np.int32).tobytes())


def read_stcl(path):
    with open(path, "rb") as f:
        if f.read(8) != MAGIC:
            raise ValueError("not a .stcl file: %s" % path)
        n, flags = struct.unpack("<ii", f.read(8))
        pos = np.frombuffer(f.read(12 * n), np.float32).reshape(n, 3).copy()
        nrm = np.frombuffer(f.read(12 * n), np.float32).reshape(n, 3).copy()
        prob = np.frombuffer(f.read(4 * n), np.float32).copy() if flags & 1 else None
        pixel = np.frombuffer(f.read(8 * n), np.int32).reshape(n, 2).copy() if flags & 2 else None
    return pos, nrm, prob, pixel


def read_ply_mesh(path):
    """the vertices and triangles of a PLY file (ascii or binary_little_endian; polygons are fanned from their corner 0) ->
    (vertices (nv, 3) float32, triangles (nt, 3) int32); a file without faces gives nt = 0"""
    from . import capi
    L = capi.load()
    nv, nt = C.c_int(0), C.c_int(0)
    capi.check(L.stocs_ply_read_mesh(str(path).encode(), None, 0, C.byref(nv), None, 0, C.byref(nt)))
    pos = np.zeros((nv.value, 3), np.float32)
    tri = np.zeros((nt.value, 3), np.int32)
    capi.check(L.stocs_ply_read_mesh(str(path).encode(), pos.ctypes.data_as(capi._fp), nv.value, C.byref(nv), tri.ctypes.data_as(capi._ip), nt.value, C.byref(nt)))
    return pos, tri


def write_ply_mesh(path, pos, tris):
    from . import capi
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    capi.check(capi.load().stocs_ply_write_mesh(str(path).encode(), pos.ctypes.data_as(capi._fp), len(pos), tris.ctypes.data_as(capi._ip), len(tris)))
