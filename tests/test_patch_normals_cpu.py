"""The sub-patch normal-cone test of the queue kernel's shared-list forms (csrc/patch_normals.h, "lcp_patch_normals"), on the host.
  * tests/cpp/patch_normals_check.cpp is compiled with g++ against the header alone and run, once plainly and once under the address and
    undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded): the bound against a brute-force maximum of the kernel's
    own float dot product over members of both cones, the derivation's expression in double, and everything that must rule nothing out.
  * The same bound through the library (stocs_patch_normal_bound_host, the function the kernel runs) against a brute-force maximum in
    numpy, float32 in the kernel's order of operations.
  * The model records of stocs_model_subpatch_normals against float64: every member normal inside its sub-patch's cone, the records
    that must carry "no test"."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "patch_normals_check.cpp")
DOT_LO = np.float32(0.8660254)


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_patch_normals_check(tmp_path, flags):
    exe = str(tmp_path / "patch_normals_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", *flags, "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "patch_normals_check: ok" in r.stdout
    m = re.search(r"test: (\d+) trials, (\d+) with v outside the scene cone, ruled out (\d+)", r.stdout)
    assert m, r.stdout
    trials, outside, out = (int(x) for x in m.groups())
    assert trials >= 60000 and 10 * out >= trials and out < outside


def _lib():
    from model_matching_amd import capi
    return capi, capi.load()


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _cone_members(axis, ang, towards, n_az=48):
    """unit vectors at `ang` from the unit `axis`: the one towards `towards` first, then n_az azimuths, then the axis itself"""
    side = towards - axis * (towards @ axis)
    side = _unit(side) if np.linalg.norm(side) > 1e-12 else _unit(np.cross(axis, [1.0, 0.0, 0.0] if abs(axis[0]) < 0.6 else [0.0, 1.0, 0.0]))
    e2 = np.cross(axis, side)
    phi = np.concatenate([[0.0], np.arange(n_az) * (2 * np.pi / n_az)])
    ring = np.cos(ang) * axis + np.sin(ang) * (np.cos(phi)[:, None] * side + np.sin(phi)[:, None] * e2)
    return np.concatenate([ring, axis[None]])


def test_bound_through_the_library_against_brute_force():
    capi, L = _lib()
    rng = np.random.default_rng(11)
    n_out = 0; n_outside = 0
    for it in range(400):
        cls = int(rng.integers(1, 241)); word = int(rng.integers(0, 4096)) | (int(rng.integers(0, 4096)) << 12) | (cls << 24)
        beta = float(rng.uniform(0.0, 0.35 if it % 3 else 0.78))
        sb = np.nextafter(np.float32(np.sin(beta) * (1 + 1e-6) + 1e-7), np.float32(2))
        if sb > np.float32(0.70710677):
            continue
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        A = Q * (1.0 if it % 4 else rng.uniform(0.5, 2.0))
        if it % 5 == 0:
            A = A @ (np.eye(3) + rng.uniform(-0.4, 0.4, (3, 3)))
        A32 = A.astype(np.float32)
        a = _unit(rng.normal(size=3)).astype(np.float32)
        a = (a / np.float32(np.sqrt(np.float32(a @ a)))).astype(np.float32)
        G = (A32.astype(np.float64).T @ A32.astype(np.float64)); ag = np.abs(G)
        s = np.float32(np.sqrt(max(G[0, 0] + ag[0, 1] + ag[0, 2], G[1, 1] + ag[0, 1] + ag[1, 2], G[2, 2] + ag[0, 2] + ag[1, 2])) * 1.00002)   # >= linear_norm_bound
        # v = A a in the kernel's order: t0 * ax + (t4 * ay + t8 * az) per row
        v = (A32[:, 0] * a[0] + (A32[:, 1] * a[1] + A32[:, 2] * a[2])).astype(np.float32)
        outside = C.c_int(0); axis = np.zeros(3, np.float32)
        b = L.stocs_patch_normal_bound_host(C.c_uint32(word), v.ctypes.data_as(capi._fp), C.c_float(float(sb)), C.c_float(float(s)), C.byref(outside),
                                            axis.ctypes.data_as(capi._fp))
        if not outside.value:
            continue
        n_outside += 1
        o = _unit(axis.astype(np.float64)); delta = np.arcsin(cls / 256.0); a64 = _unit(a.astype(np.float64))
        dmax = -np.inf
        for nm in _cone_members(a64, beta, A.T @ o):
            nm32 = nm.astype(np.float32)
            vt = (A32[:, 0] * nm32[0] + (A32[:, 1] * nm32[1] + A32[:, 2] * nm32[2])).astype(np.float32)
            ns = _cone_members(o, delta, vt.astype(np.float64))
            if np.arccos(np.clip(_unit(vt.astype(np.float64)) @ o, -1, 1)) < delta:
                ns = np.concatenate([ns, _unit(vt.astype(np.float64))[None]])
            for length in (1.0 - 1e-4, 1.0 + 1e-4):
                n32 = (ns * length).astype(np.float32)
                d = n32[:, 0] * vt[0] + (n32[:, 1] * vt[1] + n32[:, 2] * vt[2])   # the kernel's dot product, float32
                dmax = max(dmax, float(d.max()))
        assert dmax <= b, (it, cls, beta, dmax, b)
        n_out += b < DOT_LO
    assert n_outside >= 200 and n_out >= 40, (n_outside, n_out)


def _records(pos, nrm):
    capi, L = _lib()
    n = len(pos)
    pos = np.ascontiguousarray(pos, np.float32); nrm = np.ascontiguousarray(nrm, np.float32)
    perm = np.zeros(n, np.int32); rec = np.zeros(((n + 15) // 16, 4), np.float32)
    assert L.stocs_model_subpatch_normals(pos.ctypes.data_as(capi._fp), nrm.ctypes.data_as(capi._fp), n, perm.ctypes.data_as(capi._ip), rec.ctypes.data_as(capi._fp)) == 0
    perm2 = np.zeros(n, np.int32); sub = np.zeros(((n + 15) // 16, 4), np.float32)
    assert L.stocs_model_subpatches(pos.ctypes.data_as(capi._fp), n, perm2.ctypes.data_as(capi._ip), sub.ctypes.data_as(capi._fp)) == 0
    assert np.array_equal(perm, perm2)
    return perm, rec


@pytest.mark.parametrize("n", [16, 1008, 1040, 5000])
def test_model_records_hold_their_normals(n):
    from model_matching_amd import synth
    m = synth.make_model(n, seed=77 + n)
    perm, rec = _records(m.pos, m.nrm)
    nrm = _unit(m.nrm.astype(np.float64))[perm]
    tested = 0
    for q in range(len(rec)):
        mem = nrm[16 * q:16 * q + 16]
        ax = rec[q, :3].astype(np.float64); sb = float(rec[q, 3])
        if sb < 0:
            # no test: only for a cone wider than 45 degrees about the members' mean direction (a little less counts too: the stored axis is a float)
            mean = _unit(mem.sum(0))
            assert np.arccos(np.clip(mem @ mean, -1, 1)).max() > np.deg2rad(44.9), q
            continue
        tested += 1
        assert abs(np.linalg.norm(ax) - 1.0) < 1e-6 and sb <= 0.70710678
        sin_ang = np.linalg.norm(np.cross(mem, _unit(ax)), axis=1)
        assert (mem @ ax > 0).all() and sin_ang.max() <= sb, (q, sin_ang.max(), sb)
        assert sb - sin_ang.max() < 1e-5, (q, sin_ang.max(), sb)       # rounded outwards, not padded
    # (16 points spread over the whole solid span every direction; from a thousand points on a sub-patch is a piece of surface)
    assert n == 16 or tested >= (len(rec) + 1) // 2


def test_model_records_without_a_test():
    rng = np.random.default_rng(3)
    pos = rng.uniform(-0.05, 0.05, (64, 3)).astype(np.float32)
    nrm = np.tile([0.0, 0.0, 1.0], (64, 1)).astype(np.float32)
    perm, rec = _records(pos, nrm)
    assert (rec[:, 3] >= 0).all() and (rec[:, 3] < 1e-5).all() and np.allclose(rec[:, :3], [0, 0, 1])
    inv = np.argsort(perm)            # slot of model point i
    for kind, value in (("nan", [np.nan, 0.0, 1.0]), ("zero", [0.0, 0.0, 0.0]), ("inf", [np.inf, 0.0, 0.0]), ("opposite", [0.0, 0.0, -1.0]), ("wide", [1.0, 0.0, 0.05])):
        bad = nrm.copy(); bad[5] = value
        _, r = _records(pos, bad)
        q = inv[5] // 16
        assert r[q, 3] < 0, kind
        assert (np.delete(r[:, 3], q) >= 0).all(), kind
    # a normal of any finite length is normalised by the loader first: still tested
    scaled = nrm.copy(); scaled[7] *= 3.0; scaled[9] *= 1e-3
    _, r = _records(pos, scaled)
    assert (r[:, 3] >= 0).all()
