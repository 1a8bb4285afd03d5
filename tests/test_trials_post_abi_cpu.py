"""CPU-side checks of the trial batches' post-processing ABI (stocs_run_trials_post, stocs_trials_get_hypotheses): the library
exports both entry points, the header that declares them still compiles as C99, the ctypes structs have the C layout (sizes and
offsets from a probe compiled against the header), and the Python layers bind them.  No GPU compute here."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def test_library_exports_post_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("stocs_run_trials_post", "stocs_trials_get_hypotheses", "stocs_run_trials"):
        assert hasattr(lib, name), name


def test_header_declares_post_as_c99(tmp_path):
    src = tmp_path / "post_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const uint64_t* seeds, stocs_trial_result* out) {\n"
        "    stocs_trial_post p = {0.8f, 10, 0.02f, 15.0f, {0.0f, 0.0f, 180.0f}, 5, 0.035f};\n"
        "    stocs_trial_hypothesis h[4]; int n = 0;\n"
        "    int rc = stocs_run_trials_post(c, 0, 2, seeds, 100, 0.9f, 200, 0, &p, out);\n"
        "    if (rc) return rc;\n"
        "    rc = stocs_run_trials_post(c, 0, 2, seeds, 100, 0.9f, 200, 0, NULL, out);\n"
        "    return rc ? rc : stocs_trials_get_hypotheses(c, 0, h, 4, &n);\n"
        "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _c_layout(tmp_path, struct, fields):
    src = tmp_path / ("probe_%s.c" % struct)
    body = "".join('    printf("%%s %%zu\\n", "%s", offsetof(%s, %s));\n' % (f, struct, f) for f in fields)
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"stocs_hip.h\"\nint main(void) {\n"
                   '    printf("sizeof %%zu\\n", sizeof(%s));\n%s    return 0;\n}\n' % (struct, body))
    exe = tmp_path / ("probe_%s" % struct)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    return {k: int(v) for k, v in (line.split() for line in out if line)}


@pytest.mark.parametrize("struct,cls", [("stocs_trial_post", "TrialPost"), ("stocs_trial_hypothesis", "TrialHypothesis")])
def test_ctypes_layout_matches_c(capi, tmp_path, struct, cls):
    S = getattr(capi, cls)
    names = [f[0] for f in S._fields_]
    lay = _c_layout(tmp_path, struct, names)
    assert lay["sizeof"] == C.sizeof(S)
    for f in names:
        assert lay[f] == getattr(S, f).offset, f


def test_python_layers_bind_post(capi):
    L = capi.load()
    assert L.stocs_run_trials_post.restype is C.c_int and len(L.stocs_run_trials_post.argtypes) == 10
    assert L.stocs_trials_get_hypotheses.restype is C.c_int and len(L.stocs_trials_get_hypotheses.argtypes) == 5
    from model_matching_amd.estimator import _HYP_DTYPE, StocsEstimator, trial_post
    assert "post" in inspect.signature(StocsEstimator.run_trials).parameters
    assert inspect.signature(StocsEstimator.run_trials).parameters["post"].default is None
    assert callable(getattr(StocsEstimator, "trials_get_hypotheses"))
    p = trial_post(sym3=(0, 0, 180), refine_iterations=5)
    assert (p.acceptable_fraction, p.maximum_pose_count, list(p.sym3), p.refine_iterations) == (pytest.approx(0.8), 10, [0.0, 0.0, 180.0], 5)
    assert _HYP_DTYPE.itemsize == C.sizeof(capi.TrialHypothesis)
    for name in _HYP_DTYPE.names:
        assert _HYP_DTYPE.fields[name][1] == getattr(capi.TrialHypothesis, name).offset, name


def test_post_arguments_rejected_without_a_context(capi):
    """a NULL context is STOCS_ERR_INVALID before anything else (no device needed)"""
    L = capi.load()
    p = capi.TrialPost(0.8, 10, 0.02, 15.0, (C.c_float * 3)(0, 0, 0), 0, 0.035)
    seeds = (C.c_uint64 * 1)(1)
    assert L.stocs_run_trials_post(None, 0, 1, seeds, 10, 0.9, 200, 0, C.byref(p), None) == capi.ERR_INVALID
    n = C.c_int(0)
    assert L.stocs_trials_get_hypotheses(None, 0, None, 0, C.byref(n)) == -5
