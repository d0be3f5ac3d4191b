"""tests/warm_ref.py, the reference of lfr_batch_solve_from, without a GPU: at a zero start it IS lfr_ref.solve_problem (positions
bitwise, info equal, traces equal entry for entry); the projection of the start; the cost never rises above the start's; a start near
the solution needs fewer iterations; and the C ABI declares the entry."""
import os
import re

import numpy as np
import pytest

import class_limit_cases as CL
import lfr_ref as R
import warm_ref as W
from lfr_amd import capi, synthetic, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BELOW_TREE = [n for n in CL.NAMES if n not in CL.TREE]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_is_solve_problem(comps):
    assert comps
    for c, (var_nodes, prob) in comps.items():
        ta, tb = [], []
        xa, ia = R.solve_problem(W.fresh(prob), ta)
        xb, ib = W.solve_from(W.fresh(prob), np.zeros(2 * prob.nv), tb)
        assert np.array_equal(_bits(xa), _bits(xb)), c
        assert ia == ib, c
        assert len(ta) == len(tb) and all(a == b for a, b in zip(ta, tb)), c


@pytest.mark.parametrize("name", BELOW_TREE)
def test_zero_start_is_solve_problem_on_every_class_limit(name):
    comps, _ = W.components(CL.alone(name))
    assert len(comps) == 1
    _assert_is_solve_problem(comps)


@pytest.mark.parametrize("name", ["clean", "bounds"])
def test_zero_start_is_solve_problem_on_golden(name):
    pairs = wire.decode_matching_file(open(os.path.join(GOLD, name + ".pb"), "rb").read())
    comps, _ = W.components(synthetic.pairs_to_arrays(pairs))
    _assert_is_solve_problem(comps)


def _first_graph():
    return synthetic.generate(seed=5, n_images=12, n_tracks=60)


def test_start_is_projected_and_nan_reads_as_zero():
    comps, _ = W.components(_first_graph())
    var_nodes, prob = max(comps.values(), key=lambda v: v[1].nv)
    assert prob.nv >= 3
    x0 = np.zeros(2 * prob.nv)
    x0[0], x0[1], x0[2], x0[3] = 1.5, -1.5, np.nan, np.inf
    tr = []
    p = W.fresh(prob)
    W.solve_from(p, x0, tr)
    want = np.zeros(2 * prob.nv)
    want[0], want[1], want[2], want[3] = 1.0, -1.0, 0.0, 1.0
    assert tr[0]["cost"] == W.fresh(prob).evaluate(want, True)[0]          # iteration 0 is evaluated at the projected start, bit for bit


def test_final_cost_is_at_most_the_cost_of_the_projected_start():
    comps, n = W.components(_first_graph())
    start = np.random.default_rng(3).normal(0.0, 0.6, size=(n, 2))          # (some coordinates beyond the box)
    assert (np.abs(start) > 1.0).any()
    for c, (var_nodes, prob) in comps.items():
        x0 = start[var_nodes].reshape(-1)
        _, info = W.solve_from(W.fresh(prob), x0)
        assert info["final_cost"] <= W.fresh(prob).evaluate(prob.project(x0), False)[0], c


def _perturbed(ma, seed=1):
    import dataclasses
    rng = np.random.default_rng(seed)
    return dataclasses.replace(ma, disp1=(ma.disp1 + rng.normal(0.0, 0.002, ma.disp1.shape)).astype(np.float32),
                               disp2=(ma.disp2 + rng.normal(0.0, 0.002, ma.disp2.shape)).astype(np.float32))


def test_warm_start_after_a_small_flow_change_takes_fewer_iterations():
    ma = _first_graph()
    comps, n = W.components(ma)
    first, infos0 = W.solve_graph(comps, n, None)
    comps2, n2 = W.components(_perturbed(ma))
    assert n2 == n and sorted(comps2) == sorted(comps)
    assert all(np.array_equal(comps[c][0], comps2[c][0]) for c in comps)      # the structure stayed
    _, cold = W.solve_graph(comps2, n, None)
    _, warm = W.solve_graph(comps2, n, first)
    n_cold, n_warm = sum(i["iterations"] for i in cold.values()), sum(i["iterations"] for i in warm.values())
    print("LM iterations over %d components: cold %d, warm %d" % (len(comps), n_cold, n_warm))
    assert n_warm < n_cold


def test_resolve_at_the_solution_takes_at_most_the_cold_iterations():
    comps, n = W.components(_first_graph())
    first, cold = W.solve_graph(comps, n, None)
    _, again = W.solve_graph(comps, n, first)
    for c in comps:
        assert again[c]["iterations"] <= cold[c]["iterations"], c
        assert again[c]["termination"] == R.TERM_CONVERGENCE


def test_header_declares_and_binding_exports_solve_from():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfr.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+lfr_batch_solve_from\s*\(\s*lfr_batch\s*\*\s*b\s*,\s*const\s+double\s*\*\s*initial_positions_device\s*,"
                     r"\s*void\s*\*\s*hip_stream\s*,\s*lfr_solve_stats\s*\*\s*stats\s*\)\s*;", text)
    assert "lfr_batch_solve_from" in capi.EXPORTS
    assert hasattr(capi.Batch, "solve_from")
