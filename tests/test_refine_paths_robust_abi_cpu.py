"""CPU-side checks of the robust refinement behind trial batches and the tracker (stocs_run_trials_post_robust,
stocs_track_poses_robust): the library exports both, the header declares them as C99 with the argument lists the ctypes binding
gives them, and the Python wrappers take the plain entry points for None and build the float cosine as refine_poses_robust does.
No GPU compute here."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include")]
NAMES = ("stocs_run_trials_post_robust", "stocs_track_poses_robust")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from model_matching_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        g.build()
    return m


def test_library_exports_both_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name


def test_header_declares_them_as_c99(tmp_path):
    src = tmp_path / "refine_paths_robust_c99.c"
    src.write_text(
        "#include <stddef.h>\n#include \"stocs_hip.h\"\n"
        "int call(stocs_ctx* c, const uint64_t* seeds, const float* priors, const stocs_trial_post* post, const stocs_track_params* prm,\n"
        "         stocs_trial_result* a, stocs_track_result* b) {\n"
        "    int (*f)(stocs_ctx*, int, int, const uint64_t*, int, float, int, int, const stocs_trial_post*, float, float, stocs_trial_result*) = stocs_run_trials_post_robust;\n"
        "    int (*g)(stocs_ctx*, const float*, int, const stocs_track_params*, float, float, stocs_track_result*) = stocs_track_poses_robust;\n"
        "    return f(c, 0, 4, seeds, 100, 0.9f, 200, 0, post, 0.7f, 0.8660254f, a) + g(c, priors, 1, prm, 0.7f, -2.0f, b);\n"
        "}\n")
    r = subprocess.run(GCC + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ctypes_signatures_match_the_header(capi):
    L = capi.load()
    u64p, fp = C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    want = {
        "stocs_run_trials_post_robust": [C.c_void_p, C.c_int, C.c_int, u64p, C.c_int, C.c_float, C.c_int, C.c_int, C.POINTER(capi.TrialPost), C.c_float, C.c_float,
                                         C.POINTER(capi.TrialResult)],
        "stocs_track_poses_robust": [C.c_void_p, fp, C.c_int, C.POINTER(capi.TrackParams), C.c_float, C.c_float, C.POINTER(capi.TrackResult)],
    }
    for name, args in want.items():
        assert name in capi.SIGNATURES
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    # the robust forms are the plain ones with the two floats in front of the output
    plain_b, plain_t = capi.SIGNATURES["stocs_run_trials_post"][1], capi.SIGNATURES["stocs_track_poses"][1]
    assert want["stocs_run_trials_post_robust"] == plain_b[:-1] + [C.c_float, C.c_float] + plain_b[-1:]
    assert want["stocs_track_poses_robust"] == plain_t[:-1] + [C.c_float, C.c_float] + plain_t[-1:]
    # no context: INVALID, never a crash; a NULL post is refused by the batch form
    assert L.stocs_run_trials_post_robust(None, 0, 0, None, 0, 0.9, 1, 0, None, 0.7, 0.5, None) == capi.ERR_INVALID
    assert b"post" in L.stocs_last_error()
    assert L.stocs_track_poses_robust(None, None, 0, None, 0.7, 0.5, None) == capi.ERR_INVALID


class _Recorder:
    """stands in for the loaded library: records (name, args) and answers STOCS_OK"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _bare_estimator():
    from model_matching_amd.estimator import StocsEstimator
    est = StocsEstimator.__new__(StocsEstimator)
    est.L, est.h = _Recorder(), None
    return est


def test_wrappers_route_none_to_the_plain_entry_points(capi):
    from model_matching_amd.estimator import StocsEstimator
    cos30 = StocsEstimator.robust_params(5, 0.035, 0.7, 30.0).min_normal_cos        # what refine_poses_robust hands to the library
    assert cos30 == C.c_float(math.cos(30.0 * math.pi / 180.0)).value
    est = _bare_estimator()
    prior = np.eye(4, dtype=np.float32).reshape(1, 16)
    est.track_poses(prior)
    est.track_poses(prior, refine_iterations=5, keep_ratio=0.7, max_normal_deg=30.0)
    est.track_poses(prior, refine_iterations=5, keep_ratio=0.5)
    est.track_poses(prior, refine_iterations=5, max_normal_deg=0.0)
    names = [c[0] for c in est.L.calls]
    assert names == ["stocs_track_poses", "stocs_track_poses_robust", "stocs_track_poses_robust", "stocs_track_poses_robust"]
    assert len(est.L.calls[0][1]) == 5 and len(est.L.calls[1][1]) == 7
    f32 = lambda x: C.c_float(x).value
    assert (f32(est.L.calls[1][1][4]), f32(est.L.calls[1][1][5])) == (f32(0.7), cos30)
    assert f32(est.L.calls[2][1][4]) == f32(0.5) and est.L.calls[2][1][5] < -1.0      # no angle: gate off
    assert (est.L.calls[3][1][4], est.L.calls[3][1][5]) == (1.0, 1.0)                    # no ratio: everything kept; 0 degrees: cosine 1
    est = _bare_estimator()
    est.run_trials([1, 2])
    est.run_trials([1, 2], post=dict(refine_iterations=5))
    est.run_trials([1, 2], post=dict(refine_iterations=5), robust=dict(keep_ratio=0.7, max_normal_deg=30.0))
    est.run_trials([1, 2], post=dict(refine_iterations=5), robust=dict())
    est.run_trials([1, 2], post=dict(refine_iterations=5), robust=dict(keep_ratio=1.0, max_normal_deg=None))
    names = [c[0] for c in est.L.calls]
    assert names == ["stocs_run_trials", "stocs_run_trials_post", "stocs_run_trials_post_robust", "stocs_run_trials_post_robust", "stocs_run_trials_post_robust"]
    assert len(est.L.calls[1][1]) == 10 and len(est.L.calls[2][1]) == 12
    for k in (2, 3):                                                                       # the defaults are 0.7 and 30 degrees
        assert (f32(est.L.calls[k][1][9]), f32(est.L.calls[k][1][10])) == (f32(0.7), cos30)
    assert est.L.calls[4][1][9] == 1.0 and est.L.calls[4][1][10] < -1.0
    with pytest.raises(ValueError):
        est.run_trials([1], robust=dict(keep_ratio=0.7))                                   # nothing to refine without post
    with pytest.raises(ValueError):
        est.run_trials([1], post=dict(refine_iterations=5), robust=dict(trim=0.7))
