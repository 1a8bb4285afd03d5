"""The device's matched scene index per (candidate, model point) against the reference's own kd-tree header (oracle/_ref/libref_accel.so,
oracle/ref_accel.cpp) -- directly, with no restatement in between: the oracle only hands over the centred floats here and is not
compared.  tests/test_ref_accel_cpu.py holds the oracle and the product's host tree to the same header.

exact_ties = 1: the hit equals the reference's answer for every model point of every candidate, in the automatic form and in every
kernel form of test_exact_ties_gpu.FORMS.  No allowance.
exact_ties = 0: a hit may differ from the reference's only as the declared rule Q11 says: both found, both at the same
float32 squared distance within the radius, and the product's is the larger index.

The fixture is test_exact_ties_gpu's lattice scene (12 005 points) and its 600-point model on tie positions.  Only the library is read at
run time, never the reference tree."""
import os
import sys

import numpy as np
import pytest

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grid_ref  # noqa: E402
from test_exact_ties_gpu import FORM_DEFAULTS, FORMS, lattice  # noqa: E402,F401  (lattice: the fixture, sparse and dense layouts)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    from oracle import pyref
    if not pyref.available():
        if pyref.reference_present():
            pytest.fail("the reference tree is at %s but %s is missing: `make -C oracle` builds it" % (pyref.reference_dir(), pyref.SO))
        pytest.skip("neither the reference tree (%s) nor %s exists" % (pyref.reference_dir(), pyref.SO))
    return pyref.RefAccel()


class Pin:
    """the reference tree over the centred scene, and its answers for candidates T (n, 16)"""

    def __init__(self, ref, orc, T):
        self.sc, self.mc = orc.scene_centred(), orc.model_centred()
        self.sq = grid_ref.sq_eps(orc.prm.distance_threshold)
        self.T = T
        tree = ref.kdtree(self.sc)
        self.q = [grid_ref.transform(t, self.mc) for t in T]
        self.want = [tree.nn(q, self.sq) for q in self.q]
        tree.close()
        assert sum(int((w >= 0).sum()) for w in self.want) > 0

    def exact(self, est, what):
        for c, t in enumerate(self.T):
            hit = est.lcp_detail(t)[0]
            bad = np.nonzero(hit != self.want[c])[0]
            assert len(bad) == 0, "%s, candidate %d: %d of %d model points differ from the reference header, first %d: device %d reference %d" % (
                what, c, len(bad), len(hit), bad[0], hit[bad[0]], self.want[c][bad[0]])

    def default_rule(self, est):
        """-> number of (candidate, model point) pairs whose hit differs from the reference's; each of them checked against Q11"""
        n = 0
        for c, t in enumerate(self.T):
            hit, want, q = est.lcp_detail(t)[0], self.want[c], self.q[c]
            for i in np.nonzero(hit != want)[0]:
                g, r = int(hit[i]), int(want[i])
                assert g >= 0 and r >= 0, (c, i, g, r)
                dg = grid_ref.d2_f32(q[i:i + 1], self.sc[g:g + 1])[0, 0]
                dr = grid_ref.d2_f32(q[i:i + 1], self.sc[r:r + 1])[0, 0]
                assert dg.view(np.uint32) == dr.view(np.uint32) and dg <= self.sq, (c, i, g, r, float(dg), float(dr), float(self.sq))
                assert g > r, (c, i, g, r)
                n += 1
        return n


def test_exact_ties_equals_the_reference_header_in_every_form(lattice, ref):
    est, orc, T = lattice
    pin = Pin(ref, orc, T[:16])
    est.set_option("exact_ties", 1)
    pin.exact(est, "automatic form")
    for opts in FORMS:
        for k, v in opts.items():
            est.set_option(k, v)
        pin.exact(est, str(opts))
        for k, v in FORM_DEFAULTS:
            est.set_option(k, v)


def test_default_mode_differs_from_the_reference_header_only_by_q11(lattice, ref):
    est, orc, T = lattice
    pin = Pin(ref, orc, T[:16])
    n = pin.default_rule(est)
    assert n > 0, "%d hits of 16 candidates differ from the reference header: the fixture no longer exercises Q11" % n
    print("hits that differ from the reference header under the largest-index rule: %d of %d" % (n, 16 * len(pin.mc)))


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_synth_workloads_against_the_reference_header(name, oracle_lib, ref):
    from model_matching_amd import synth
    from model_matching_amd.estimator import StocsEstimator
    m, s, k = synth.workload(name)
    est = StocsEstimator(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    orc = oracle_lib.Oracle(s.pos, s.nrm, s.prob, s.pixel, m.pos, m.nrm, build_index=False)
    cs, cm = orc.centroids()
    T = synth.make_candidates(synth.centred_gt(s.T_gt, cs.astype(np.float64), cm.astype(np.float64)), k)
    best = int(np.argmax(est.score_transforms(T)))
    pin = Pin(ref, orc, T[list(range(12)) + [best]])
    assert int((pin.want[-1] >= 0).sum()) > 0                          # the best candidate matches model points
    n = pin.default_rule(est)
    print("%s: hits that differ from the reference header under the largest-index rule: %d" % (name, n))
    est.set_option("exact_ties", 1)
    pin.exact(est, name)
    est.close()
