"""The extended-precision reference of tests/test_gpu_linear_solve.py checked on the CPU: against mpmath at 50 digits on small
systems, against numpy.linalg.solve on well-conditioned ones, and the damped diagonal formed as each kernel forms it."""
import numpy as np
import pytest

import linsolve_ref as R

mpmath = pytest.importorskip("mpmath")


def _mp_solve(M, g):
    with mpmath.workdps(50):
        y = mpmath.lu_solve(mpmath.matrix(M.tolist()), mpmath.matrix(g.tolist()))
        return [y[i] for i in range(M.shape[0])]


@pytest.mark.parametrize("kind", ["normal", "graded", "cond1e8"])
def test_reference_matches_mpmath(kind):
    rng = np.random.default_rng(11)
    for n in (2, 4, 6, 10, 16):
        A = {"normal": lambda: R.normal_matrix(rng, n), "graded": lambda: R.graded(rng, n, 1e3, 1e3),
             "cond1e8": lambda: R.spd_with_cond(rng, n, 1e8)}[kind]()
        solver = "g16" if n % 4 else "block_s"
        M = R.damped(A, R.damping_for(rng, A, solver, 1e-3), solver)
        g = rng.normal(0, 1, n)
        y = R.solve_ld(M, g)
        ym = _mp_solve(M, g)
        kappa = float(np.linalg.cond(M, np.inf))
        with mpmath.workdps(50):
            err = max(abs(_mp_exact(y[i]) - ym[i]) for i in range(n))
            ynorm = max(abs(v) for v in ym)
        # longdouble: unit roundoff 2^-64; the elimination's forward error stays below a few n u_ld kappa
        assert float(err / ynorm) <= 4 * n * 2.0 ** -64 * kappa, (n, float(err / ynorm), kappa)


def _mp_exact(v):
    """A longdouble as an mpf, exactly (the float64 head and the remainder, which has at most 11 significant bits)."""
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - np.longdouble(hi)))


def test_reference_matches_lapack_when_well_conditioned():
    rng = np.random.default_rng(12)
    for n in (2, 8, 32, 88, 130):
        A = R.spd_with_cond(rng, n, 1e2)
        g = rng.normal(0, 1, n)
        y = R.solve_ld(A, g)
        y64 = np.linalg.solve(A, g)
        assert np.max(np.abs(y64 - y.astype(np.float64))) <= 1e-13 * np.max(np.abs(y64))
        assert R.backward_error(A, y.astype(np.float64), g) <= 2 * n * R.U


def test_damped_diagonal_as_the_kernels_form_it():
    a = np.array([[1.0, 0.5], [0.5, 3.0]])
    d = np.array([0.1, 1e-9])
    Mp = R.damped(a, d, "g16")
    assert Mp[0, 0] == 1.0 + 0.1 and Mp[1, 1] == 3.0 + 1e-9 and Mp[0, 1] == 0.5
    Mb = R.damped(a, np.array([1.0 + 2.0 ** -30, 3.0]), "block_m")
    # one rounding of a_ii + d^2: the product alone would round 2^-60 away
    assert Mb[0, 0] == 2.0 + 2.0 ** -29
    assert Mb[1, 1] == 12.0


def test_tri_layout_round_trip_and_systems():
    rng = np.random.default_rng(13)
    A = R.normal_matrix(rng, 12)
    assert np.array_equal(R.from_tri(R.to_tri(A), 12), A)
    assert np.all(np.linalg.eigvalsh(A) > 0)
    B = R.normal_matrix(rng, 10, disconnected=True)
    assert np.count_nonzero(B[:2, 2:]) == 0
    G = R.graded(rng, 20, 1e6)
    assert np.all(np.linalg.eigvalsh(G / np.sqrt(np.outer(np.diag(G), np.diag(G)))) > 0)
    for zero in (False, True):
        N = R.not_pd(rng, 8, 3, zero)
        # elimination without pivoting: pivots 0..2 positive, pivot 3 zero or negative
        W = N.copy()
        for k in range(3):
            assert W[k, k] > 0
            W[k + 1:, k:] -= np.outer(W[k + 1:, k] / W[k, k], W[k, k:])
        assert (W[3, 3] == 0.0) if zero else (W[3, 3] < -0.1)


def test_cl_dispatch_replica():
    assert [R.packed_cl("g8", n) for n in (2, 4, 6, 8)] == [2, 4, 6, 8]
    assert [R.packed_cl("g16", n) for n in (2, 10, 12, 14, 16)] == [10, 10, 12, 14, 16]
    assert [R.packed_cl("g64_2", n) for n in (2, 18, 20, 22, 24)] == [18, 18, 20, 22, 24]
    assert R.packed_cl("g64_4", 32) == ("lpr2", 16)
