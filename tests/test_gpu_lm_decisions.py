"""Rejected steps, contracting line searches and the projection onto the bound inside the workgroup kernels (three LDS footprints,
the elimination-tree kernel on both of its schedules) and the 24- and 32-row packed classes: the inputs of tests/lm_decision_cases.py
(tests/test_lm_decision_cases.py establishes on the CPU that the oracle does take those decisions on them) against the C oracle,
decision for decision - iterations, termination, the evaluation counts of the line searches and candidates, and the exact set of
coordinates that sit ON the bound.  Components whose trajectory changes with the oracle's own summation order (lm_decision_cases.
sensitive_components; at most 5 % of a case, none at the present seeds) are left out of the trajectory checks, never of the positions.

Also the backward pass on components with coordinates at the bound (the fixed rows of its Hessian) against tests/backward_ref.py."""
import numpy as np
import pytest

import lm_decision_cases as LC
from test_gpu_backward import _check_against_reference, _ubar      # (imports torch: before the library is loaded)
from lfr_amd import capi
from test_gpu_parity import TOL_UNITS

pytestmark = pytest.mark.gpu
NAMES = sorted(LC.CASES)
_solved = {}


def solved(name):
    """(graph, problem, batch, stats and positions of the first solve), once per case"""
    if name not in _solved:
        ma, _, _ = LC.reference(name)
        g = capi.Graph.from_arrays(ma)
        p = capi.Problem(g)
        b = capi.Batch(p, 0)
        st = b.solve()
        _solved[name] = (g, p, b, st, b.download().copy())
    return _solved[name]


@pytest.mark.parametrize("name", NAMES)
def test_decisions_match_the_oracle(lfr_lib, name):
    ma, ref, sensitive = LC.reference(name)
    g, p, b, st, pos = solved(name)
    assert (ref["comp"] == p.labels()[2]).all()
    info = b.component_info()
    comp = info["component"]
    assert sorted(comp.tolist()) == np.nonzero(ref["comp_nvar"] > 0)[0].tolist()
    assert (info["n_var_nodes"] == ref["comp_nvar"][comp]).all() and (info["n_edges"] == ref["comp_nedges"][comp]).all()
    assert {LC.kernel_class(2 * v, e) for v, e in zip(info["n_var_nodes"], info["n_edges"])} == LC.CLASSES[name]
    oi = ref["infos"][comp]
    firm = ~np.isin(comp, sensitive)
    err = np.abs(pos - ref["positions"]).max()
    ne = info["n_edges"].astype(np.int64)
    want_jac, want_cost = int((oi["n_jac_evals"] * ne).sum()), int((oi["n_cost_evals"] * ne).sum())
    firm_node = ~np.isin(ref["comp"], sensitive)
    got_mask, want_mask = LC.bound_mask(pos)[firm_node], LC.bound_mask(ref["positions"])[firm_node]
    print("%s: %d components (%d sensitive), max |dx| %.3e, iterations differ in %d, bound mask differs in %d of %d coordinates at the bound, "
          "jacobian passes x edges %d (oracle %d), cost passes x edges %d (oracle %d)"
          % (name, len(comp), len(sensitive), err, int((oi["iterations"] != info["iterations"])[firm].sum()),
             int((got_mask != want_mask).sum()), int(want_mask.sum()), st["ref_jacobian_passes_edges"], want_jac, st["ref_cost_passes_edges"], want_cost))
    assert st["n_failed"] == 0 and st["n_components"] == len(comp)
    assert (oi["termination"] == info["termination"]).all()
    assert (oi["iterations"] == info["iterations"])[firm].all()
    assert err <= TOL_UNITS
    assert (got_mask == want_mask).all()                         # ON the bound: 1 - 1e-16 or 1 + ulp is a mismatch
    assert np.abs(pos).max() <= 1.0
    if len(sensitive) == 0:
        assert st["ref_jacobian_passes_edges"] == want_jac and st["ref_cost_passes_edges"] == want_cost
    else:
        assert st["ref_jacobian_passes_edges"] == pytest.approx(want_jac, rel=1e-3)
        assert st["ref_cost_passes_edges"] == pytest.approx(want_cost, rel=1e-3)
    assert b.spin_timeouts() == 0


@pytest.mark.parametrize("name", NAMES)
def test_second_solve_is_bitwise_the_first(lfr_lib, name):
    _, _, b, _, pos = solved(name)
    b.solve()
    assert np.array_equal(b.download(), pos)
    assert b.spin_timeouts() == 0


@pytest.mark.parametrize("name", sorted(LC.THIN_PLAN))
def test_components_above_192_rows_took_the_tree_kernel(lfr_lib, name):
    _, _, b, _, _ = solved(name)
    ts = b.tree_stats()
    rows = 2 * b.component_info()["n_var_nodes"]
    assert (rows > LC.MAX_BLOCK_ROWS).all()
    assert (ts["columns"] >= (rows + 15) // 16).all() and (ts["tiles"] >= ts["columns"]).all() and (ts["levels"] >= 1).all()
    dense = ts["tiles"] == ts["columns"] * (ts["columns"] + 1) // 2
    assert dense.all() if not LC.THIN_PLAN[name] else not dense.any()          # (a complete track fills every tile, a ring few)
    assert b.spin_timeouts() == 0


def test_device_assembly_is_bitwise_the_host_assembly(lfr_lib):
    g, _, bh, _, pos = solved("block_m")
    pd = capi.Problem(g, device_graph_stage=0)
    bd = capi.Batch(pd, 0)
    bd.solve()
    ih, idv = bh.component_info(), bd.component_info()
    for k in ("component", "n_var_nodes", "n_edges", "iterations", "termination"):
        assert (ih[k] == idv[k]).all(), k
    assert np.array_equal(bd.download(), pos)


@pytest.mark.parametrize("name", sorted(n for n in LC.REQUIRED if "backward" in LC.REQUIRED[n]))
def test_backward_at_the_bound(lfr_lib, name):
    ma, ref, sensitive = LC.reference(name)
    g, p, b, _, pos = solved(name)
    at_bound = LC.bound_mask(pos)
    which = np.setdiff1d(np.unique(p.labels()[2][at_bound.any(axis=1)]), sensitive).tolist()
    n, st, _ = _check_against_reference(ma, g, p, b, _ubar(g.n_nodes, 3), which)
    print("%s: %d components with a coordinate at the bound, %d checked (the others' Hessians are indefinite: zeros on both sides), "
          "%d coordinates at a bound" % (name, len(which), n, st["n_bound_coordinates"]))
    assert st["n_bound_coordinates"] == int(at_bound.sum()) >= 1
    assert n >= LC.REQUIRED[name]["backward"]
