"""The congruent-set join on models built to sit on its edges (congruent_cases.py; what each case reaches is asserted on the CPU by
test_congruent_cases_cpu.py): intersection points exactly on position-cell faces, pair directions exactly along the axes (the exactly
anti-parallel branch of quat_from_z), the first and last position cell of every axis, P runs of 63 / 64 / 65, 255 / 256 / 260 and
65 535 / 65 536 entries in one position cell, coincident, planar and collinear models.  Every case runs in the default form, with the
distance gate evaluated per couple (STOCS_CONGRUENT_DISTANCE_GATE) and with the lists kept whole (STOCS_CONGRUENT_KEEP_ALL); per base the
quads, their count and every rank of the walk order equal the oracle's bit for bit, and the candidates of make_transforms are the same
bits in all three forms."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import congruent_cases as cases  # noqa: E402
from test_congruent_forms_gpu import _check_quads, _set_switches  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = ({}, {"STOCS_CONGRUENT_DISTANCE_GATE": "1"}, {"STOCS_CONGRUENT_KEEP_ALL": "1"})


class _Cache:
    def __init__(self, orc):
        self.orc, self.memo = orc, {}

    def get(self, ids, inv):
        key = (tuple(int(x) for x in ids), np.asarray(inv, np.float32).tobytes())
        if key not in self.memo:
            self.memo[key] = (self.orc.find_congruent(ids, float(inv[0]), float(inv[1])), self.orc.find_congruent_seq(ids, float(inv[0]), float(inv[1])))
        return self.memo[key]


@pytest.mark.parametrize("name", cases.NAMES)
def test_edge_case_equals_the_oracle_in_every_form(oracle_lib, monkeypatch, name):
    from model_matching_amd.estimator import StocsEstimator
    case = cases.build(name)
    orc = cases.make_oracle(oracle_lib, case)
    cache = _Cache(orc)
    ids, inv = case["ids"], case["inv"]
    est = StocsEstimator(case["spos"], case["snrm"], case["sprob"], case["spix"], case["mpos"], case["mnrm"], build_index=True)
    try:
        assert np.array_equal(est.get_model_centroid(), np.zeros(3, np.float32))        # centring changes nothing: the cells are the designed ones
        rng = np.random.default_rng(len(name))
        cands = []
        for env in FORMS:
            _set_switches(monkeypatch, env)
            est.set_bases(ids, inv)
            total = est.find_congruent_all()
            _check_quads(est, cache, ids, inv, total, rng, (name, env))
            assert [est.num_quads(k) for k in range(len(ids))] == list(case["expect_quads"]), (name, env)
            n = est.make_transforms(40, 20261021)
            T, P, _, b = est.get_pose_candidates()
            cands.append((n, T.view(np.uint32).copy(), P.view(np.uint32).copy(), b.copy()))
        for c in cands[1:]:
            assert c[0] == cands[0][0] and all(np.array_equal(x, y) for x, y in zip(c[1:], cands[0][1:])), name
        # the bases once more in reverse order, default form: per-base results do not depend on their slot
        _set_switches(monkeypatch, {})
        est.set_bases(ids[::-1], inv[::-1])
        _check_quads(est, cache, ids[::-1], inv[::-1], est.find_congruent_all(), rng, (name, "reversed"))
    finally:
        est.close()
