"""The LM step solves of the solver kernels, (A + D) y = g, against an extended-precision reference (tests/linsolve_ref.py), through
lfr_debug_solve_damped: the packed classes' Gauss-Jordan elimination in registers at every row count each class admits, alone in its
wave and beside a larger neighbour, and the workgroup classes' blocked LDL^T + back substitution at every even row count up to the
class limit.  The end-to-end parity tests allow 6.25e-6 units; a trust-region loop corrects an inaccurate step, so they cannot see a
solve that is wrong at 1e-8.  These tests can: the forward error is held to 16 times that of a float64 LAPACK solve (or the textbook
bound 4 n u kappa |y|), and the workgroup solves to a backward error of 8 n u."""
import numpy as np
import pytest

import linsolve_ref as R
from lfr_amd import capi

pytestmark = pytest.mark.gpu

RELS = (1e-22, 1e-12, 1e-6, 1e-2, 1.0, 1e8, 1e32, 1e64)     # dd / a_ii: Ceres' diag in [1e-6, 1e32], radius in [1e-32, 1e16]
SPD_KINDS = ("normal", "normal_hi", "disconnected", "graded2", "graded6", "graded12", "cond1e4", "cond1e10", "identity", "diagonal")


def _system(rng, n, kind, solver, serial):
    """(A, damp, g) of one SPD test system."""
    rel = RELS[serial % len(RELS)]
    if kind == "normal":
        A = R.normal_matrix(rng, n)
    elif kind == "normal_hi":
        A, rel = R.normal_matrix(rng, n), (1e-22, 1e64)[serial % 2]          # both ends of the damping's range
    elif kind == "disconnected":
        A = R.normal_matrix(rng, n, disconnected=True)
    elif kind.startswith("graded"):
        A, rel = R.graded(rng, n, 10.0 ** int(kind[6:])), 1e-22
    elif kind.startswith("cond"):
        A, rel = R.spd_with_cond(rng, n, float(kind[4:])), 1e-22
    elif kind == "identity":
        A, rel = np.eye(n), 0.0
    else:
        A = np.diag(10.0 ** rng.uniform(-3, 3, n))
    damp = R.damping_for(rng, A, solver, rel)
    g = rng.normal(0, 1, n) * (10.0 ** rng.uniform(-2, 2))
    return A, damp, g


def _run(solver, slots):
    """slots: (A, damp, g) or None (an empty packed group) per system, in wave order.  Returns (list of y or None, status)."""
    n_rows = np.array([0 if s is None else s[0].shape[0] for s in slots], np.int32)
    A = np.concatenate([np.zeros(0)] + [R.to_tri(s[0]) for s in slots if s is not None])
    damp = np.concatenate([np.zeros(0)] + [s[1] for s in slots if s is not None])
    g = np.concatenate([np.zeros(0)] + [s[2] for s in slots if s is not None])
    y, status = capi.solve_damped_hip(solver, n_rows, A, damp, g)
    out, k = [], 0
    for n in n_rows:
        out.append(y[k:k + n] if n else None)
        k += n
    return out, status


def _check_solution(solver, sysm, y, what):
    A, damp, g = sysm
    M = R.damped(A, damp, solver)
    y_ref = R.solve_ld(M, g)
    err, bound = R.forward_error(y, y_ref), R.forward_bound(M, g, y_ref)
    assert err <= bound, "%s: forward error %.3e > bound %.3e (|y| = %.3e)" % (what, err, bound, float(np.max(np.abs(y_ref))))
    if solver in R.BLOCK:
        n = A.shape[0]
        be = R.backward_error(M, y, g)
        assert be <= 8 * n * R.U, "%s: backward error %.3e > 8 n u = %.3e" % (what, be, 8 * n * R.U)


# ---------------------------------------------------------------------------------------------------------------------------
# packed classes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def packed(lfr_lib):
    res = {}
    for si, solver in enumerate(R.PACKED):
        rng = np.random.default_rng(4100 + si)
        G, lim = R.GROUPS[solver], capi.SOLVER_MAX_ROWS[solver]
        systems = [(n, kind, _system(rng, n, kind, solver, serial))
                   for n in range(2, lim + 1, 2) for serial, kind in enumerate(SPD_KINDS)]
        # alone: one system per wave, in group position i % G, the other groups empty
        alone_slots, pos = [], []
        for i, (_, _, s) in enumerate(systems):
            w = [None] * G
            w[i % G] = s
            pos.append(len(alone_slots) + i % G)
            alone_slots += w
        y_all, st_all = _run(solver, alone_slots)
        alone = [y_all[p] for p in pos]
        alone_status = [int(st_all[p]) for p in pos]
        # beside a larger neighbour (the class's largest system) in another group of the same wave
        beside = beside_status = None
        if G > 1:
            big = _system(rng, lim, "normal", solver, 3)
            slots, pos = [], []
            for i, (_, _, s) in enumerate(systems):
                w = [None] * G
                w[i % G] = s
                w[(i + 1) % G] = big
                pos.append(len(slots) + i % G)
                slots += w
            y_b, st_b = _run(solver, slots)
            beside = [y_b[p] for p in pos]
            beside_status = [int(st_b[p]) for p in pos]
        res[solver] = dict(systems=systems, alone=alone, alone_status=alone_status, beside=beside, beside_status=beside_status)
    return res


@pytest.mark.parametrize("solver", R.PACKED)
def test_packed_solve_forward_error(packed, solver):
    r = packed[solver]
    assert r["alone_status"] == [0] * len(r["systems"])
    for (n, kind, s), y in zip(r["systems"], r["alone"]):
        _check_solution(solver, s, y, "%s n=%d %s" % (solver, n, kind))


@pytest.mark.parametrize("solver", R.PACKED)
def test_packed_solve_covers_every_instantiation(packed, solver):
    """Every CL branch of the dispatch ran: the sizes alone in their waves select each of them."""
    cls = {R.packed_cl(solver, n) for n, _, _ in packed[solver]["systems"]}
    want = {"g8": {2, 4, 6, 8}, "g16": {10, 12, 14, 16}, "g64_2": {18, 20, 22, 24},
            "g64_4": {("lpr2", 10), ("lpr2", 12), ("lpr2", 14), ("lpr2", 16)}}[solver]
    assert cls == want


@pytest.mark.parametrize("solver", [s for s in R.PACKED if R.GROUPS[s] > 1])
def test_packed_solve_independent_of_neighbours(packed, solver):
    """A system's y is bitwise the same alone in its wave and beside the class's largest system (a larger CL, more elimination
    steps through its padded rows): padded rows and columns contribute exact zeros."""
    r = packed[solver]
    assert r["beside_status"] == [0] * len(r["systems"])
    for (n, kind, _), ya, yb in zip(r["systems"], r["alone"], r["beside"]):
        assert np.array_equal(ya, yb), "%s n=%d %s: max |diff| %.3e" % (solver, n, kind, np.max(np.abs(ya - yb)))


@pytest.mark.parametrize("solver", R.PACKED)
def test_packed_solve_rejects_non_positive_pivots(lfr_lib, solver):
    """A pivot that is zero or negative first at step 0 or n-1 sets the invalid bit (and nothing else) of that system only; the
    other systems of its wave come out bitwise as they do without it.  Also the same position in every system of a wave."""
    rng = np.random.default_rng(4200 + R.PACKED.index(solver))
    G, lim = R.GROUPS[solver], capi.SOLVER_MAX_ROWS[solver]
    good = [_system(rng, n, "normal", solver, n) for n in range(2, lim + 1, 2)]
    alone = []
    for s in good:
        alone += [s] + [None] * (G - 1)
    y_good, st_good = _run(solver, alone)
    y_good = [y for y in y_good if y is not None]
    assert list(st_good[::G]) == [0] * len(good)
    for n in range(2, lim + 1, 2):
        for k in sorted({0, n - 1}):
            for zero in (False, True):
                bad = (R.not_pd(rng, n, k, zero), np.zeros(n), rng.normal(0, 1, n))
                slots = [bad] + [good[(n // 2 - 1 + j) % len(good)] for j in range(1, G)]
                y, st = _run(solver, slots)
                assert st[0] == 1 and np.all(np.isnan(y[0])), (solver, n, k, zero, st)
                for j in range(1, G):
                    assert st[j] == 0 and np.array_equal(y[j], y_good[(n // 2 - 1 + j) % len(good)]), (solver, n, k, zero, j)
                # every system of the wave invalid at the same step
                y, st = _run(solver, [(R.not_pd(rng, n, k, zero), np.zeros(n), rng.normal(0, 1, n)) for _ in range(G)])
                assert list(st) == [1] * G, (solver, n, k, zero, st)


# ---------------------------------------------------------------------------------------------------------------------------
# workgroup classes
# ---------------------------------------------------------------------------------------------------------------------------
def _block_corpus(solver, rng):
    lim = capi.SOLVER_MAX_ROWS[solver]
    spd, bad = [], []
    for n in range(2, lim + 1, 2):
        kinds = ["normal", SPD_KINDS[1 + n // 2 % (len(SPD_KINDS) - 1)]]
        for serial, kind in enumerate(kinds):
            spd.append((n, kind, _system(rng, n, kind, solver, n // 2 + serial)))
        if n % 16 in (0, 2, 14) or n <= 18:
            last_panel = 16 * ((n - 1) // 16)
            for k in sorted({0, n - 1, 15, 16, last_panel}):
                if k < n:
                    zero = (n // 2 + k) % 2 == 0
                    bad.append((n, k, zero, (R.not_pd(rng, n, k, zero), np.zeros(n), rng.normal(0, 1, n))))
    return spd, bad


@pytest.fixture(scope="module")
def block(lfr_lib):
    res = {}
    for si, solver in enumerate(R.BLOCK):
        spd, bad = _block_corpus(solver, np.random.default_rng(4300 + si))
        slots = [s for _, _, s in spd] + [s for _, _, _, s in bad]
        runs = [_run(solver, slots) for _ in range(3)]       # every size in flight at once, three times
        res[solver] = dict(spd=spd, bad=bad, runs=runs)
    return res


@pytest.mark.parametrize("solver", R.BLOCK)
def test_block_solve_forward_and_backward_error(block, solver):
    r = block[solver]
    y, st = r["runs"][0]
    sizes = {n for n, _, _ in r["spd"]}
    assert sizes == set(range(2, capi.SOLVER_MAX_ROWS[solver] + 1, 2))        # every n = 0 and 14 (mod 16) among them
    for i, (n, kind, s) in enumerate(r["spd"]):
        assert st[i] == 0, (solver, n, kind, st[i])
        _check_solution(solver, s, y[i], "%s n=%d %s" % (solver, n, kind))


@pytest.mark.parametrize("solver", R.BLOCK)
def test_block_solve_repeatable_and_no_spin_timeouts(block, solver):
    """Bitwise equal over three launches of the whole corpus; no bounded spin-wait of the factorization ran out."""
    runs = block[solver]["runs"]
    for y, st in runs:
        assert not np.any(st & 2), np.nonzero(st & 2)
    for y, st in runs[1:]:
        assert np.array_equal(st, runs[0][1])
        for i, (a, b) in enumerate(zip(y, runs[0][0])):
            assert np.array_equal(a, b, equal_nan=True), (solver, i)


@pytest.mark.parametrize("solver", R.BLOCK)
def test_block_solve_rejects_non_positive_pivots(block, solver):
    """A zero or negative pivot first at step 0, 15, 16, the first column of the last panel or n-1 sets the invalid bit only."""
    r = block[solver]
    y, st = r["runs"][0]
    off = len(r["spd"])
    assert len(r["bad"]) > 20
    for j, (n, k, zero, _) in enumerate(r["bad"]):
        assert st[off + j] == 1, (solver, n, k, zero, st[off + j])
        assert np.all(np.isnan(y[off + j]))
