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


# ---------------------------------------------------------------------------------------------------------------------------
# the elimination-tree kernel's solve (tests/test_gpu_tree_solve.py): reference, tile layout, and the inputs checked before a GPU sees them
# ---------------------------------------------------------------------------------------------------------------------------
def test_tree_damping_as_the_column_task_forms_it():
    a = np.array([[2.0 ** 24, 0.5], [0.5, 3.0]])
    d = np.array([1.0 + 2.0 ** -30, 3.0])
    # two roundings: the product (1 + 2^-30)^2 loses its 2^-60, and the sum 2^24 + 1 + 2^-29 is then a tie that goes to even; the
    # workgroup solvers' single rounding sees the 2^-60 and goes up
    Mt = R.damped(a, d, "tree")
    assert Mt[0, 0] == 2.0 ** 24 + 1.0 and Mt[1, 1] == 12.0 and Mt[0, 1] == 0.5
    assert R.damped(a, d, "block_m")[0, 0] == 2.0 ** 24 + 1.0 + 2.0 ** -28


@pytest.mark.parametrize("kind", ["normal", "graded", "cond1e8"])
def test_refined_solve_matches_the_elimination_in_longdouble(kind):
    """solve_refined (float64 Cholesky + longdouble refinement) against solve_ld, and against mpmath on the small sizes."""
    rng = np.random.default_rng(21)
    for n in (2, 6, 16, 40, 130):
        A = {"normal": lambda: R.normal_matrix(rng, n), "graded": lambda: R.graded(rng, n, 1e3, 1e3),
             "cond1e8": lambda: R.spd_with_cond(rng, n, 1e8)}[kind]()
        M = R.damped(A, np.sqrt(1e-3 * np.diag(A)), "tree")
        g = rng.normal(0, 1, n)
        y, yl = R.solve_refined(M, g), R.solve_ld(M, g)
        kappa = float(np.linalg.cond(M, np.inf))
        ynorm = float(np.max(np.abs(yl)))
        assert float(np.max(np.abs(y - yl))) <= 8 * n * 2.0 ** -64 * kappa * ynorm, (n, kappa)
        if n <= 16:
            ym = _mp_solve(M, g)
            with mpmath.workdps(50):
                err = max(abs(_mp_exact(y[i]) - ym[i]) for i in range(n))
            assert float(err) <= 4 * n * 2.0 ** -64 * kappa * ynorm, (n, float(err), kappa)


@pytest.fixture(scope="module")
def tree_cases(lfr_lib):
    import tree_solve_cases as C
    structs = C.structures()
    return C, structs, C.plans(structs)


def test_tile_layout_round_trip(tree_cases):
    C, structs, pls = tree_cases
    for name in ("dense_track", "chords", "comb"):
        pl = pls[name]
        A, _ = C.jtj(pl, *structs[name], np.random.default_rng(31))
        tiles = R.to_tiles(pl, A)
        assert tiles.shape == (pl.n_tiles, 16, 16) and np.array_equal(R.from_tiles(pl, tiles), A)
        assert not np.triu(tiles[pl.colptr[0]], 1).any()                       # of a diagonal tile the lower triangle
        real = R.real_rows(pl)
        assert not A[~real].any() and (np.diag(A)[real] > 0).all()
        B = A.copy()
        far = [(i, j) for i in range(pl.NB) for j in range(i) if j not in pl.rowsof[pl.colptr[j]:pl.colptr[j + 1]].tolist()
               and i not in pl.rowsof[pl.colptr[j]:pl.colptr[j + 1]].tolist()]
        if far:
            i, j = far[0]
            B[16 * i, 16 * j] = B[16 * j, 16 * i] = 1.0
            with pytest.raises(ValueError):
                R.to_tiles(pl, B)


def test_tree_structures_reach_every_path_of_the_kernel(tree_cases):
    """What tests/test_gpu_tree_solve.py relies on, from the plans' words (it asserts the same on the GPU box)."""
    C, structs, pls = tree_cases
    C.assert_coverage(pls)


def test_tree_emulator_meets_the_bounds_of_the_gpu_test(tree_cases):
    """scatter -> Plan.factor -> Plan.back_substitute in float64 (the kernel's algorithm in plain numpy) reproduces the reference
    within the bounds the GPU test asserts: the systems are well posed before any GPU sees them."""
    C, structs, pls = tree_cases
    worst = {}
    for name, kind, sysm in C.corpus(structs, pls):
        pl = pls[name]
        y = R.emulate_tree(pl, *sysm)
        assert not y[~R.real_rows(pl)].any()
        f, b = C.errors(pl, C.reference(pl, sysm), y)
        w = worst.setdefault(C.FAMILY[name], [0.0, 0.0])
        w[0], w[1] = max(w[0], f), max(w[1], b)
        print("%-14s %-9s forward %.3f of its bound, backward %.3f of 8 n u" % (name, kind, f, b))
        assert f <= 1.0 and b <= 1.0, (name, kind, f, b)
    print(worst)


def test_bad_pivot_cases_have_the_pivot_they_claim(tree_cases):
    """Eliminating the real rows in matrix order: every pivot before the chosen row is positive, the chosen one is not."""
    C, structs, pls = tree_cases
    cases = C.bad_pivot_cases(structs, pls)
    assert {w.replace("_zero", "") for _, w, _, _ in cases} == {"first_level", "root", "half_filled", "through_tile"}
    assert any(w.endswith("_zero") for _, w, _, _ in cases)
    for name, where, row, (A, damp, g) in cases:
        pl = pls[name]
        real = R.real_rows(pl)
        idx = np.nonzero(real)[0]
        W = R.damped(A, damp, "tree")[np.ix_(idx, idx)]
        k = int(np.nonzero(idx == row)[0][0])
        for j in range(k):
            assert W[j, j] > 0, (name, where, j)
            W[j + 1:, j:] -= np.outer(W[j + 1:, j] / W[j, j], W[j, j:])
        assert (W[k, k] == 0.0) if where.endswith("_zero") else (W[k, k] < 0), (name, where, W[k, k])
