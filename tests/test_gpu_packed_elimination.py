"""The elimination of the 8- and 16-row packed classes issues every step's rank-1 update as one asm statement with a single hazard pad
in front (lfr_device.hpp: fmac_bcast_step).  A missing wait state between a VALU write and the DPP read of the same register does not
fault: it hands some lanes a stale pivot row on some launches.  So every case here runs 256 full waves through the packed solve probe
(C entry lfr_debug_solve_damped, kernels debug_solve_packed_kernel<8,1> / <16,1>, which call packed_step) three times - a fixed count - and asks that the three launches agree
bit for bit and that every solution lies within the forward-error bound tests/test_gpu_linear_solve.py uses for this probe.  The row
counts are mixed inside each wave: its largest system selects the CL instantiation (one case per instantiation), the other groups hold
every smaller even row count, so their padded rows and the steps that run through them are exercised beside live ones.
The last test solves a small config 4 twice through the whole kernel and compares the positions bitwise."""
import numpy as np
import pytest

import linsolve_ref as R
from lfr_amd import capi, synthetic

pytestmark = pytest.mark.gpu

WAVES = 256
LAUNCHES = 3
# (solver, largest row count of every wave): the four CL instantiations of each DPP class (R.packed_cl)
CASES = [("g8", m) for m in (2, 4, 6, 8)] + [("g16", m) for m in (10, 12, 14, 16)]


def _spd(rng, n):
    """A seeded SPD system of n rows: B B^T + I scaled over six decades, LM damping of 1e-6 .. 1 of the diagonal, a right-hand side."""
    B = rng.normal(0, 1, (n, n))
    A = (B @ B.T + np.eye(n)) * 10.0 ** rng.uniform(-3, 3)
    damp = 10.0 ** rng.uniform(-6, 0, n) * np.diag(A)
    return A, damp, rng.normal(0, 1, n)


def _row_counts(solver, n_max, wave):
    """The even row counts of one wave's groups: n_max in a rotating group, the others cycle through 2 .. n_max."""
    G = R.GROUPS[solver]
    sizes = list(range(2, n_max + 1, 2))
    rows = [sizes[(wave + j) % len(sizes)] for j in range(G)]
    rows[wave % G] = n_max
    return rows


@pytest.fixture(scope="module", params=CASES, ids=["%s-max%d" % c for c in CASES])
def case(request, lfr_lib):
    solver, n_max = request.param
    rng = np.random.default_rng(8100 + 100 * R.PACKED.index(solver) + n_max)
    systems = [_spd(rng, n) for w in range(WAVES) for n in _row_counts(solver, n_max, w)]
    n_rows = np.array([s[0].shape[0] for s in systems], np.int32)
    A = np.concatenate([R.to_tri(s[0]) for s in systems])
    damp = np.concatenate([s[1] for s in systems])
    g = np.concatenate([s[2] for s in systems])
    runs = [capi.solve_damped_hip(solver, n_rows, A, damp, g) for _ in range(LAUNCHES)]
    return dict(solver=solver, n_max=n_max, systems=systems, n_rows=n_rows, runs=runs)


def test_case_layout(case):
    """256 full waves; every wave's largest system is n_max (so the case runs the CL instantiation it is named for) and every even row
    count up to n_max sits in some group beside it."""
    solver, n_max, n_rows = case["solver"], case["n_max"], case["n_rows"]
    G = R.GROUPS[solver]
    per_wave = n_rows.reshape(WAVES, G)
    assert np.all(per_wave.max(axis=1) == n_max)
    assert R.packed_cl(solver, n_max) == n_max
    assert set(n_rows.tolist()) == set(range(2, n_max + 1, 2))
    if n_max > 2:
        assert np.all((per_wave != n_max).any(axis=1))          # a smaller neighbour in every wave


def test_three_launches_bitwise_equal(case):
    y0, st0 = case["runs"][0]
    assert not np.any(st0), np.nonzero(st0)
    for y, st in case["runs"][1:]:
        assert np.array_equal(st, st0)
        diff = np.nonzero(y.view(np.uint64) != y0.view(np.uint64))[0]
        assert diff.size == 0, "%s max %d: %d values differ between launches, first at %d" % (case["solver"], case["n_max"], diff.size, diff[0])


def test_solutions_within_forward_bound(case):
    solver = case["solver"]
    y, _ = case["runs"][0]
    k = 0
    for i, (A, damp, g) in enumerate(case["systems"]):
        n = A.shape[0]
        M = R.damped(A, damp, solver)
        y_ref = R.solve_ld(M, g)
        err, bound = R.forward_error(y[k:k + n], y_ref), R.forward_bound(M, g, y_ref)
        assert err <= bound, "%s system %d (n = %d, wave %d): forward error %.3e > bound %.3e" % (solver, i, n, i // R.GROUPS[solver], err, bound)
        k += n


def test_whole_kernel_twice_bitwise(lfr_lib):
    """Config 4 at 600 tracks through solve_packed_kernel twice (the packed classes share the one launch): the same positions bit for
    bit.  The census is taken from the problem itself, so a change of the synthetic config that empties a class fails here: by row
    count (2 x variable nodes; include/lfr.h) components of the 8-row, the 16-row and a 32-row class must all be present."""
    p = capi.Problem(capi.Graph.from_arrays(synthetic.config4(n_tracks=600)))
    pos1, st1 = p.solve_hip(device=0)
    pos2, st2 = p.solve_hip(device=0)
    _, is_root, comp = p.labels()
    rows = 2 * np.bincount(comp[(comp >= 0) & ~is_root])
    rows = rows[rows > 0]
    assert np.any(rows <= 8) and np.any((rows >= 10) & (rows <= 16)) and np.any((rows >= 18) & (rows <= 32)), np.bincount(rows)
    assert st1["n_components"] > 0 and st1["n_failed"] == 0 and st2["n_failed"] == 0
    assert st1["dominant_kernel_edges"] > 0
    assert st1["sum_iterations"] == st2["sum_iterations"]
    assert np.isfinite(pos1).all()
    assert np.array_equal(pos1.view(np.uint64), pos2.view(np.uint64))
