"""The LM step solve of the elimination-tree kernel (components above 192 rows: the level-scheduled sparse LDL^T of solve_tree_component),
(A + D) y = g, against an extended-precision reference (tests/linsolve_ref.py) through lfr_debug_solve_tree: the probe runs the
device code of the solve - column tasks with their left-looking updates on the matrix cores, the barrier-free schedule of thin plans
with the tiles finished behind the elimination, the barrier schedule with tile and extra-row tasks, the back substitution - on given
matrices, one workgroup per system, in a workspace that reads as NaN wherever the kernel's prologue did not initialise it.

The end-to-end tests of this kernel (tests/test_gpu_sparse.py) allow 6.25e-6 units and a trust-region loop corrects an inaccurate step:
they cannot see a solve that is wrong at 1e-8.  Here the forward error is held to max(16 x that of a float64 LAPACK solve,
4 n u kappa |y|) and the backward error to 8 n u, n = n_pad - the criteria of the workgroup solvers in tests/test_gpu_linear_solve.py.
tests/tree_solve_cases.py builds the systems; tests/test_linsolve_ref.py checks on the CPU that they reach every path of the kernel
and that the float64 emulator of the plan (tests/tree_plan_emul.py) meets the same bounds."""
import numpy as np
import pytest

import linsolve_ref as R
import tree_solve_cases as C
from lfr_amd import capi

pytestmark = pytest.mark.gpu


def _launch(pls, cases):
    """One launch over cases = [(structure, (A, damp, g))]."""
    blobs = [pls[name].blob for name, _ in cases]
    tiles = [R.to_tiles(pls[name], s[0]) for name, s in cases]
    return capi.solve_tree_hip(blobs, tiles, [s[1] for _, s in cases], [s[2] for _, s in cases])


@pytest.fixture(scope="module")
def tree(lfr_lib):
    structs = C.structures()
    pls = C.plans(structs)
    spd = C.corpus(structs, pls)
    bad = C.bad_pivot_cases(structs, pls)
    good = [(name, s) for name, _, s in spd]
    alone = _launch(pls, good)                                                   # without the systems that are not positive definite
    runs = [_launch(pls, good + [(name, s) for name, _, _, s in bad]) for _ in range(3)]      # everything in flight at once, three times
    return dict(structs=structs, pls=pls, spd=spd, bad=bad, alone=alone, runs=runs)


def test_tree_solve_reaches_every_path(tree):
    """Both schedules, 0-3 carried tiles, tiles finished behind the elimination, tile and extra-row tasks, half-filled and one-node
    blocks, update entries beyond the two in the descriptor, one level and many, fewer columns than waves and more: from the plans."""
    C.assert_coverage(tree["pls"])


def test_tree_solve_forward_and_backward_error(tree):
    """Every SPD system: valid, no NaN, y exactly 0.0 at padding rows, forward error <= max(16 x LAPACK's, 4 n u kappa |y|), backward
    error <= 8 n u (n = n_pad).  The worst ratios per structure family are printed."""
    y, st = tree["runs"][0]
    worst, fails = {}, []
    for i, (name, kind, sysm) in enumerate(tree["spd"]):
        pl = tree["pls"][name]
        assert st[i] == 0, (name, kind, st[i])
        assert not np.isnan(y[i]).any(), (name, kind)
        pad = y[i][~R.real_rows(pl)]
        assert not pad.any() and not np.signbit(pad).any(), (name, kind)
        f, b = C.errors(pl, C.reference(pl, sysm), y[i])
        w = worst.setdefault(C.FAMILY[name], [0.0, 0.0])
        w[0], w[1] = max(w[0], f), max(w[1], b)
        if not (f <= 1.0 and b <= 1.0):
            fails.append((name, kind, f, b))
    for fam, (f, b) in worst.items():
        print("%-22s worst forward error %.3f of its bound, worst backward error %.3f of 8 n u" % (fam, f, b))
    assert not fails, fails


def test_tree_solve_repeatable_and_no_spin_timeouts(tree):
    """Bitwise equal over three launches of the whole corpus (the dependency-counter schedule hands columns to whichever wave is
    ready; every tile is still written by one wave in a fixed order); no bounded spin-wait ran out."""
    runs = tree["runs"]
    for y, st in runs + [tree["alone"]]:
        assert not np.any(st & 2), np.nonzero(st & 2)
    for y, st in runs[1:]:
        assert np.array_equal(st, runs[0][1])
        for i, (a, b) in enumerate(zip(y, runs[0][0])):
            assert np.array_equal(a, b, equal_nan=True), i


def test_tree_solve_rejects_non_positive_pivots(tree):
    """A zero or negative pivot in a first-level column, in the root column, in a half-filled block and in a row whose pivot is
    negative only through a tile its column does not carry: the invalid bit (and nothing else) for that system alone, its y NaN;
    every other system of the launch bitwise as in the launch without them."""
    y, st = tree["runs"][0]
    y0, st0 = tree["alone"]
    n = len(tree["spd"])
    wheres = {w.replace("_zero", "") for _, w, _, _ in tree["bad"]}
    assert wheres == {"first_level", "root", "half_filled", "through_tile"} and len(tree["bad"]) >= 16
    thin_tile = [name for name, w, _, _ in tree["bad"] if w == "through_tile" and tree["pls"][name].blob[28] != 0]
    thick_tile = [name for name, w, _, _ in tree["bad"] if w == "through_tile" and tree["pls"][name].blob[28] == 0]
    assert thin_tile and thick_tile                                              # finish_extra, and tile + extra-row tasks
    for j, (name, where, row, _) in enumerate(tree["bad"]):
        assert st[n + j] == 1, (name, where, row, st[n + j])
        assert np.isnan(y[n + j]).all(), (name, where, row)
    assert np.array_equal(st[:n], st0) and not st0.any()
    for i in range(n):
        assert np.array_equal(y[i], y0[i]), tree["spd"][i][:2]
