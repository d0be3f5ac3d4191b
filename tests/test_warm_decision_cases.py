"""The inputs and starts of tests/warm_decision_cases.py do what they are there for, established with tests/warm_ref.py alone: every
component lies in the intended kernel class, the reference converges everywhere, rejects steps, contracts line searches and projects
coordinates onto the bound as often as the case requires, and few components sit on a rounding-level decision.  Without this a
change of synthetic.generate or of a seed could turn tests/test_gpu_warm_decisions.py into a test that passes without reaching
anything."""
import collections

import numpy as np
import pytest

import lm_decision_cases as LC
import warm_decision_cases as WC
from lfr_amd import capi

ABOVE_192 = sorted(n for n in WC.CASES if n in WC.THIN_PLAN)


@pytest.mark.parametrize("name", sorted(WC.CASES))
def test_case_reaches_its_decisions(name):
    ma, start, comps, ref_pos, ref_infos, sensitive = WC.reference(name)
    census = collections.Counter(LC.kernel_class(2 * prob.nv, len(prob.edges)) for _, prob in comps.values())
    got = WC.decision_counts(comps, ref_pos, ref_infos, sensitive)
    print("%s: start seed %d, %d components %s, %d rounding-sensitive, decisions %s (all components: %s)"
          % (name, WC.START_SEED[name], len(comps), dict(census), len(sensitive), got, WC.decision_counts(comps, ref_pos, ref_infos)))
    assert set(census) == WC.CLASSES[name], census
    assert (np.abs(start) > 1.0).sum() >= 4 and (start > 1.0).any() and (start < -1.0).any()      # the start leaves the box on either side
    assert all(i["termination"] == capi.TERM_CONVERGENCE for i in ref_infos.values())
    assert len(sensitive) <= WC.MAX_SENSITIVE_FRACTION * len(comps)
    for k, n in WC.REQUIRED[name].items():
        assert n >= 1 and got[k] >= n, (k, got[k], n)
    for k in WC.UNREACHED.get(name, ()):                 # (a cell that turns up after all should become a required one)
        assert k not in WC.REQUIRED[name]
    assert set(WC.REQUIRED[name]) | set(WC.UNREACHED.get(name, ())) == set(WC.DECISIONS)


def test_the_warm_solution_is_not_the_cold_one():
    """from the hard start the reference ends in another local minimum than from the origin: no kernel passes by giving the cold answer"""
    _, _, comps, warm, _, _ = WC.reference("packed_24_32")
    _, _, _, cold, _, _ = WC.reference("packed_24_32", zero_start=True)
    assert np.abs(warm - cold).max() > 1.0


@pytest.mark.parametrize("name", ABOVE_192)
def test_plans_above_192_rows_take_the_intended_schedule(lfr_lib, name):
    ma = WC.generate(name)
    ref = WC.labels(ma)
    _, _, comps, _, _, _ = WC.reference(name)
    assert sorted(comps) == np.nonzero(ref["comp_nvar"] > 0)[0].tolist()
    for c, (var_nodes, prob) in comps.items():
        n_var, words = LC.plan_words(ma, ref, c)
        assert n_var == prob.nv > LC.MAX_BLOCK_ROWS // 2 and len(words) == len(prob.edges)
        blob, _ = capi.tree_plan(n_var, words)
        assert bool(blob[28]) == WC.THIN_PLAN[name], c
