"""CPU-side checks of the instance-selection C ABI (stocs_select_instances, stocs_select_instances_rows, stocs_default_instance_params):
the library exports them, the header that declares them still compiles as C99, the ctypes structs match the C layout, and the
argument checks that need no device answer before anything touches one.  No GPU compute here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from model_matching_amd.capi import InstanceParams, InstanceResult   # not there before the feature: the module fails to import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("stocs_select_instances", "stocs_select_instances_rows", "stocs_default_instance_params")
INVALID = -1


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def test_library_exports_the_symbols(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def test_defaults(capi):
    p = InstanceParams()
    capi.load().stocs_default_instance_params(C.byref(p))
    assert (p.max_instances, p.min_points, p.min_exclusive_fraction) == (16, 20, 0.5)
    capi.load().stocs_default_instance_params(None)   # tolerated


def test_header_declares_the_calls_as_c99(tmp_path):
    src = tmp_path / "instances_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const float* T, int n, const int32_t* hit, const uint8_t* counted, const float* lcp, stocs_instance_result* out, int32_t* sel) {\n"
        "    stocs_instance_params p;\n"
        "    int rc, k = 0;\n"
        "    stocs_default_instance_params(&p);\n"
        "    p.max_instances = 4; p.min_points = 10; p.min_exclusive_fraction = 0.25f;\n"
        "    rc = stocs_select_instances(c, T, n, &p, out, sel, &k);\n"
        "    rc = rc ? rc : stocs_select_instances_rows(c, hit, counted, lcp, n, 64, 1000, &p, out, sel, &k);\n"
        "    return rc ? rc : k + out->rank + out->own + out->exclusive + (int)out->lcp;\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _c_layout(tmp_path, struct, fields):
    """sizeof and offsetof of a struct of stocs_hip.h, from a small C program compiled with the system compiler"""
    src = tmp_path / ("layout_%s.c" % struct)
    body = "".join('    printf("%%zu\\n", offsetof(%s, %s));\n' % (struct, f) for f in fields)
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\nint main(void) {\n"
                   '    printf("%%zu\\n", sizeof(%s));\n%s    return 0;\n}\n' % (struct, body))
    exe = tmp_path / ("layout_%s" % struct)
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    return out[0], out[1:]


@pytest.mark.parametrize("struct,cls,size", [("stocs_instance_params", InstanceParams, 12), ("stocs_instance_result", InstanceResult, 16)])
def test_ctypes_structs_match_the_c_layout(tmp_path, struct, cls, size):
    fields = [f[0] for f in cls._fields_]
    c_size, offs = _c_layout(tmp_path, struct, fields)
    assert C.sizeof(cls) == c_size == size
    assert [getattr(cls, f).offset for f in fields] == offs


def test_capi_and_estimator_bind_the_calls(capi):
    L = capi.load()
    assert L.stocs_select_instances.restype is C.c_int and len(L.stocs_select_instances.argtypes) == 7
    assert L.stocs_select_instances_rows.restype is C.c_int and len(L.stocs_select_instances_rows.argtypes) == 11
    assert L.stocs_default_instance_params.restype is None and len(L.stocs_default_instance_params.argtypes) == 1
    from model_matching_amd.estimator import StocsEstimator, _INSTANCE_DTYPE
    assert _INSTANCE_DTYPE.itemsize == C.sizeof(InstanceResult)
    assert list(_INSTANCE_DTYPE.names) == [f[0] for f in InstanceResult._fields_]
    assert callable(getattr(StocsEstimator, "select_instances")) and callable(getattr(StocsEstimator, "select_instances_rows"))
    import sys
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    import instances_ref
    assert instances_ref.DTYPE == _INSTANCE_DTYPE


def _args(n=2, nM=4):
    out = (InstanceResult * max(n, 1))()
    sel = (C.c_int32 * 16)()
    k = C.c_int(-7)
    T = (C.c_float * (16 * max(n, 1)))()
    hit = (C.c_int32 * (max(n, 1) * nM))()
    counted = (C.c_uint8 * (max(n, 1) * nM))()
    lcp = (C.c_float * max(n, 1))()
    return out, sel, k, T, hit, counted, lcp


def test_null_context_is_invalid(capi):
    L = capi.load()
    p = InstanceParams(16, 20, 0.5)
    out, sel, k, T, hit, counted, lcp = _args()
    assert L.stocs_select_instances(None, T, 2, C.byref(p), out, sel, C.byref(k)) == INVALID
    assert L.stocs_select_instances_rows(None, hit, counted, lcp, 2, 4, 10, C.byref(p), out, sel, C.byref(k)) == INVALID
    assert b"NULL context" in L.stocs_last_error()


def test_argument_errors_answer_before_the_context_is_read(capi):
    """Every check of the arguments themselves comes before the first look into the context, so none needs a device: the context here
    is a block of zeros that is never a real one (read as a context it has no scene, which would be STOCS_ERR_STATE, not INVALID)."""
    L = capi.load()
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    out, sel, k, T, hit, counted, lcp = _args()
    ok = InstanceParams(16, 20, 0.5)

    def poses(n=2, p=ok, T=T, out=out, sel=sel, kp=C.byref(k)):
        return L.stocs_select_instances(ctx, T, n, C.byref(p) if p is not None else None, out, sel, kp)

    def rows(n=2, nM=4, nS=10, p=ok, hit=hit, counted=counted, lcp=lcp, out=out, sel=sel, kp=C.byref(k)):
        return L.stocs_select_instances_rows(ctx, hit, counted, lcp, n, nM, nS, C.byref(p) if p is not None else None, out, sel, kp)

    for call in (poses, rows):
        assert call(n=-1) == INVALID
        assert call(p=None) == INVALID
        assert call(kp=None) == INVALID
        assert call(out=None) == INVALID
        assert call(sel=None) == INVALID
        for bad in (InstanceParams(0, 20, 0.5), InstanceParams(16, 0, 0.5), InstanceParams(16, 20, 0.0), InstanceParams(16, 20, -0.5),
                    InstanceParams(16, 20, float(np.nextafter(np.float32(1), np.float32(2)))), InstanceParams(16, 20, float("nan")),
                    InstanceParams(16, 20, float("inf"))):
            assert call(p=bad) == INVALID, (bad.max_instances, bad.min_points, bad.min_exclusive_fraction)
    assert poses(T=None) == INVALID
    assert rows(hit=None) == INVALID and rows(counted=None) == INVALID and rows(lcp=None) == INVALID
    assert rows(nM=0) == INVALID and rows(nS=0) == INVALID
    # a counted hit outside the scene is found on the host; an uncounted one is not an error (it comes next: the size limits)
    counted[5] = 1
    hit[5] = 10
    assert rows() == INVALID and b"hit[5] = 10" in L.stocs_last_error()
    hit[5] = -1
    assert rows() == INVALID
    assert rows(n=16385) == INVALID and poses(n=16385) == INVALID   # n is checked before the rows are walked
    # the rows form with nothing to do never reaches a device either
    assert rows(n=0) == 0 and k.value == 0
