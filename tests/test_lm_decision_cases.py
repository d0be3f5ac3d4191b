"""The inputs of tests/lm_decision_cases.py do what they are there for, established with the oracle alone: every component lies in the
intended kernel class, the oracle rejects steps, contracts line searches and projects coordinates onto the bound as often as the
case requires, and few components sit on a rounding-level decision.  Without this a change of synthetic.generate could turn
tests/test_gpu_lm_decisions.py into a test that passes without reaching anything."""
import collections

import numpy as np
import pytest

import backward_ref as BR
import lm_decision_cases as LC


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_case_reaches_its_decisions(name):
    ma, ref, sensitive = LC.reference(name)
    assert ref["rc"] == 0
    solved = np.nonzero(ref["comp_nvar"] > 0)[0]
    census = collections.Counter(LC.kernel_class(2 * ref["comp_nvar"][c], ref["comp_nedges"][c]) for c in solved)
    got = LC.decision_counts(ref, sensitive)
    print("%s: %d components %s, %d rounding-sensitive, decisions %s (all components: %s)"
          % (name, len(solved), dict(census), len(sensitive), got, LC.decision_counts(ref)))
    assert set(census) == LC.CLASSES[name], census
    assert (ref["infos"]["termination"][solved] == 0).all()
    assert len(sensitive) <= LC.MAX_SENSITIVE_FRACTION * len(solved)
    for k, n in LC.REQUIRED[name].items():
        if k != "backward":
            assert got[k] >= n, (k, got[k], n)
    for k in LC.UNREACHED.get(name, ()):                 # (a cell that turns up after all should become a required one)
        assert k not in LC.REQUIRED[name]
    if "long_search" in LC.REQUIRED[name]:
        assert got["long_search"] >= 1


@pytest.mark.parametrize("name", sorted(LC.THIN_PLAN))
def test_plans_above_192_rows_take_the_intended_schedule(lfr_lib, name):
    from lfr_amd import capi
    ma, ref, _ = LC.reference(name)
    for c in np.nonzero(ref["comp_nvar"] > 0)[0]:
        n_var, words = LC.plan_words(ma, ref, c)
        assert n_var == ref["comp_nvar"][c] and len(words) == ref["comp_nedges"][c]
        blob, _ = capi.tree_plan(n_var, words)
        assert bool(blob[28]) == LC.THIN_PLAN[name], c


def checkable_backward_components(name):
    """Components outside the sensitive set with a coordinate at the bound and a positive-definite reduced Hessian (fixed
    coordinates' rows and columns replaced by the identity) at the oracle's positions: where a backward pass has a gradient to give."""
    ma, ref, sensitive = LC.reference(name)
    which = set(np.setdiff1d(LC.components_at_bound(ref), sensitive).tolist())
    idx = {n: i for i, n in enumerate(ma.image_names)}
    node_image = np.array([idx[n] for n in ref["image_names"]], np.int32)[ref["node_image"]]
    comps = BR.graph_components(ma, ref["track"], ref["is_root"], ref["comp"], node_image, ref["node_feat"], which=which)
    out = []
    for c, (var_nodes, cp) in comps.items():
        x = ref["positions"][var_nodes].reshape(-1)
        fr = cp.free(x)
        assert not fr.all()
        H = cp.hessian(x)
        H[~fr, :] = 0.0
        H[:, ~fr] = 0.0
        H[~fr, ~fr] = 1.0
        try:
            np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            continue
        out.append(c)
    return out, len(which)


@pytest.mark.parametrize("name", sorted(n for n in LC.REQUIRED if "backward" in LC.REQUIRED[n]))
def test_backward_has_components_at_the_bound_to_check(name):
    ok, n_at_bound = checkable_backward_components(name)
    print("%s: %d components with a coordinate at the bound, %d of them with a positive-definite reduced Hessian" % (name, n_at_bound, len(ok)))
    assert len(ok) >= LC.REQUIRED[name]["backward"] >= 5
