"""The queue kernel's normal-cone gate reads the model normal from the fourth word of the sorted position: three signed 10-bit
components and a "no gate" flag (csrc/normal_cone.h), with the quantisation bound folded into one threshold per wavefront.  The
normal test still reads the exact normal, so every score must stay the same BITWISE with the gate on, off and from the plain kernel:
in every form the option reaches, under odd matrices, with model normals that sit half a code step from a code value about the
30-degree threshold, with model normals that cannot be packed, and in millimetres.  stocs_lcp_gate_count runs the kernel's own gate
on the kernel's own packed word and threshold: it never rules out a point the detail form counts, and it keeps ruling out."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DOT_LO = np.float32(np.cos(np.deg2rad(30.0)))
HALF_STEP = 0.5 / 511.0


def _estimator(spos, snrm, mpos, mnrm, **prm):
    from model_matching_amd import capi
    from model_matching_amd.estimator import StocsEstimator
    params = capi.default_params(**prm) if prm else None
    return StocsEstimator(spos.astype(np.float32), snrm.astype(np.float32), np.full(len(spos), 0.5, np.float32), np.zeros((len(spos), 2), np.int32),
                          mpos.astype(np.float32), mnrm.astype(np.float32), params=params, build_index=False)


def _workload(name, scale=1.0, model_nrm=None, **prm):
    from model_matching_amd import capi, synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, k = synth.workload(name)
    est = StocsEstimator(s.pos * np.float32(scale), s.nrm, s.prob, s.pixel, m.pos * np.float32(scale), m.nrm if model_nrm is None else model_nrm(m.nrm),
                         params=capi.default_params(**prm) if prm else None, build_index=False)
    cs = est.get_scene_centroid().astype(np.float64); cm = est.get_model_centroid().astype(np.float64)
    T = synth.make_candidates(synth.centred_gt(s.T_gt, cs / scale, cm / scale), min(k, 1024))
    T[:, 12:15] *= np.float32(scale)
    return est, T


def _odd(near, rng):
    """matrices the gate's margin has to hold for: scaled up and down (the norm bound s of the threshold), sheared, mirrored, and
    with NaN and infinite entries (a threshold that is NaN or -inf: nothing is ruled out)"""
    odd = near[:48].reshape(48, 4, 4).copy()
    for i in range(48):
        A = odd[i, :3, :3].T.astype(np.float64)
        kind = i % 6
        if kind == 0: A = A * 2.0
        elif kind == 1: A = A @ (np.eye(3) + rng.uniform(-0.6, 0.6, (3, 3)))
        elif kind == 2: A = A @ np.diag([1.0, -1.0, 1.0])
        elif kind == 3: A = A * rng.uniform(0.3, 0.95)
        elif kind == 4: A = A * 600.0      # s K > dot_lo: a negative threshold
        else: A = A * 1.0e-3
        odd[i, :3, :3] = A.T.astype(np.float32)
    bad = near[:8].copy()
    bad[0, 0] = np.nan; bad[1, 5] = np.nan; bad[2, 10] = np.inf; bad[3, 9] = -np.inf; bad[4, 12] = np.nan; bad[5, :] = 0.0; bad[6, 0:3] = 3e38; bad[7, 8:11] = np.nan
    return np.concatenate([odd.reshape(48, 16), bad])


def _three_ways(est, T):
    """scores with the gate off, on, and from the plain kernel; asserts they are bitwise equal and returns them"""
    est.set_option("lcp_variant", 99)
    est.set_option("lcp_normal_gate", 0); off = est.score_transforms(T)
    est.set_option("lcp_normal_gate", 1); on = est.score_transforms(T)
    est.set_option("lcp_variant", 0); plain = est.score_transforms(T)
    est.set_option("lcp_variant", 99)
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
    assert np.array_equal(on.view(np.uint32), plain.view(np.uint32))
    return on


def _gate_count(est, T):
    dT = est.dev_alloc(T.nbytes)
    est.dev_upload(dT, T)
    out = est.lcp_gate_count(dT, len(T))
    est.dev_free(dT)
    return out


def _every_form(est, T):
    base = None
    for split in (1, 0):
        for flat in (1, 0):
            for cull, unit in ((2, 16), (2, 64), (0, 64)):
                est.set_option("lcp_split", split); est.set_option("lcp_flat", flat); est.set_option("lcp_cull", cull); est.set_option("lcp_cull_unit", unit)
                s = _three_ways(est, T)
                base = s if base is None else base
                assert np.array_equal(s.view(np.uint32), base.view(np.uint32)), (split, flat, cull, unit)
    return base


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_scores_bitwise_equal_in_every_form(name):
    est, near = _workload(name)
    T = np.concatenate([near, _odd(near, np.random.default_rng(15))])
    s = _every_form(est, T)
    assert s[: len(near)].max() > 0.05
    q, ruled, wrong = _gate_count(est, T)
    assert wrong == 0 and 0 < ruled < q
    if name == "small":
        # the share the gate on exact normals had to reach (tests/test_normal_gate_gpu.py); the CPU census with 10-bit normals: 38 %
        qn, rn, wn = _gate_count(est, near)
        print("small: %d of %d queries ruled out" % (rn, qn))
        assert wn == 0 and rn >= 0.25 * qn, (qn, rn)


# ---- hand-built scenes --------------------------------------------------------------------------------------------------
def _plane(n=25, step=0.002):
    g = (np.arange(n) - (n - 1) / 2.0) * step
    x, y = np.meshgrid(g, g)
    return np.stack([x.ravel(), y.ravel(), np.zeros(n * n)], 1)


def _line(n=121, step=0.0003):
    x = (np.arange(n) - (n - 1) / 2.0) * step
    return np.stack([x, np.zeros(n), np.zeros(n)], 1)


def _rot_x(deg, ty=0.0):
    """column-major centred transform: rotation about x (the line of the model), translation along y"""
    c, s = np.float32(np.cos(np.deg2rad(deg))), np.float32(np.sin(np.deg2rad(deg)))
    T = np.zeros((4, 4), np.float32)
    T[0, 0] = 1; T[1, 1] = c; T[1, 2] = -s; T[2, 1] = s; T[2, 2] = c; T[1, 3] = ty; T[3, 3] = 1
    return T.T.reshape(16)


FAR = (40.0, 60.0, 90.0, 120.0, 150.0, 180.0, -40.0, -90.0)


def _tilted_normal(axis, sign):
    """(0, 0, 1) moved by half a code step of the packing along one coordinate: the quantised normal is a full half step from the
    true one, on one side or the other of it as seen from the plane's normal"""
    if axis == 2:   # z half a step below 1: the code is 510 or 511; the rest of the length goes to y
        z = 1.0 - HALF_STEP
        return np.array([0.0, sign * np.sqrt(1.0 - z * z), z])
    n = np.zeros(3)
    n[axis] = sign * HALF_STEP
    n[2] = np.sqrt(1.0 - HALF_STEP * HALF_STEP)
    return n


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_half_a_code_step_about_the_threshold(axis, sign):
    spos = _plane(); snrm = np.tile([0.0, 0.0, 1.0], (len(spos), 1))
    mpos = _line(); mnrm = np.tile(_tilted_normal(axis, sign), (len(mpos), 1))
    est = _estimator(spos, snrm, mpos, mnrm)
    # the dot product with the plane's normal passes cos 30 degrees within this band whichever way the model normal is tilted:
    # steps of 0.01 degrees across +-0.4 degrees on either side (half a code step is 0.056 degrees, the tilt in y up to 2.5)
    about = np.concatenate([sg * (30.0 + off + np.arange(-0.4, 0.4001, 0.01)) for sg in (1.0, -1.0) for off in (0.0, 0.056, -0.056, 2.53, -2.53)])
    T = np.stack([_rot_x(d, ty) for ty in (0.0, 0.0013, -0.0101) for d in list(about) + [0.0, 25.0, 33.0, 35.0] + list(FAR)])
    for split in (1, 0):
        est.set_option("lcp_split", split)
        s = _three_ways(est, T)
    assert s.max() > 0.4 and s.min() == 0.0      # the threshold is straddled
    q, ruled, wrong = _gate_count(est, T)
    assert wrong == 0 and ruled > 0
    # well past 30 degrees plus the cone (class 1: 3.6 degrees, its axis within 2) plus the margins: every query with a list is ruled out
    Tfar = np.stack([_rot_x(d, ty) for ty in (0.0, 0.0013) for d in FAR])
    qf, rf, wf = _gate_count(est, Tfar)
    assert wf == 0 and qf > 0 and rf == qf, (qf, rf)


def _break_normals(nrm):
    nrm = np.array(nrm, np.float32, copy=True)
    nrm[3::17] = 0.0; nrm[5::19] = np.nan; nrm[7::23] *= 0.5; nrm[11::29] = np.inf
    return nrm


def test_model_normals_that_cannot_be_packed():
    """zero and NaN model normals (flagged: never ruled out, and never counted by the normal test either) and half-length ones (the
    loader normalises them: packed like any other) -- on the plane, where every query meets the gate, and on `small`"""
    spos = _plane(); snrm = np.tile([0.0, 0.0, 1.0], (len(spos), 1))
    mpos = _line(); mnrm = _break_normals(np.tile([0.0, 0.0, 1.0], (len(mpos), 1)))
    est = _estimator(spos, snrm, mpos, mnrm)
    T = np.stack([_rot_x(d, ty) for ty in (0.0, 0.0013) for d in (0.0, 10.0, 29.0, 31.0, 35.0) + FAR])
    for split in (1, 0):
        est.set_option("lcp_split", split)
        s = _three_ways(est, T)
    assert s[0] > 0.3
    q, ruled, wrong = _gate_count(est, T)
    assert wrong == 0 and ruled > 0
    # past the threshold every packed point is ruled out and no flagged one (zero, NaN, infinite) is
    n_flag = len(set(range(3, 121, 17)) | set(range(5, 121, 19)) | set(range(11, 121, 29)))
    qf, rf, wf = _gate_count(est, np.stack([_rot_x(d) for d in FAR]))
    assert wf == 0 and qf == len(FAR) * 121 and rf == len(FAR) * (121 - n_flag), (qf, rf, n_flag)

    est, near = _workload("small", model_nrm=_break_normals)
    s = _every_form(est, np.concatenate([near, _odd(near, np.random.default_rng(16))]))
    assert s.max() > 0.05
    q, ruled, wrong = _gate_count(est, near)
    assert wrong == 0 and ruled > 0


def test_millimetres():
    est_m, Tm = _workload("small")
    ref = _three_ways(est_m, Tm)
    est, T = _workload("small", scale=1000.0, distance_threshold=5.0)
    s = _three_ways(est, T)
    assert s.max() > 0.05 and abs(float(s.max()) - float(ref.max())) < 0.05
    q, ruled, wrong = _gate_count(est, T)
    assert wrong == 0 and ruled >= 0.25 * q
