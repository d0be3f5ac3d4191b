"""tests/hessian_solve_ref.py pinned without a GPU: its solutions against dense solves with the matrices of backward_ref /
backward_gn_ref, the measurements behind TRUE_RESIDUAL_OVER_TOL_CPU and ITERATIONS_OVER_ROWS_CPU, the negative-curvature sets the GPU
test relies on, the ring of 6146 rows within half its iteration cap, and hand-made facts (b = 0, a bound row, a saturated Tukey edge,
damping, negative curvature on the first direction)."""
import dataclasses

import numpy as np

import class_limit_cases as CL
import cost_ref as CR
import hessian_product_ref as HR
import hessian_solve_ref as SR
from test_evaluate_ref import _tukey_at_work, inputs
from test_hessian_product_ref import _component, _dense

LD = CR.LD
TOL = 1e-10


def _kappa_bound(H, y_star, res_bound):
    """|y - y*| <= |A^-1| |b - A y| <= kappa_2(A) (|b - A y| / |b|) |y*| for a symmetric positive definite A"""
    ev = np.linalg.eigvalsh(H)
    return float(ev[-1] / ev[0]) * res_bound * float(np.linalg.norm(y_star))


# --------------------------------------------------------------------------------- 1. dense solves and the measured constants
def test_solutions_agree_with_dense_solves_and_the_constants_are_as_recorded():
    worst_res = worst_it = 0.0
    n_ok = 0
    n_neg = {}
    for label, variant, comps, sets in inputs():
        bs = SR.rhs(len(sets["a"]), 1)[0]
        for which, pos in sets.items():
            for gn in (True, False):
                neg = 0
                for c, (var_nodes, ed) in comps.items():
                    x, b = pos[var_nodes], bs[var_nodes]
                    s64 = SR.solve(ed, x, b, variant, gn, False, 0.0, TOL, dtype=np.float64)
                    assert s64.iterations <= 8 * ed.nv and s64.status in (SR.OK, SR.NEGATIVE_CURVATURE), (label, which, gn, c, s64.status)
                    if s64.status == SR.NEGATIVE_CURVATURE:
                        assert not gn
                        neg += 1
                        continue
                    res, bn = SR.true_residual(ed, x, b, s64.y, variant, gn)
                    assert s64.residual <= TOL
                    worst_res = max(worst_res, float(res / (TOL * bn)))
                    worst_it = max(worst_it, s64.iterations / (2.0 * ed.nv))
                    H = _dense(_component(ed, variant), x, gn, False)
                    if np.linalg.eigvalsh(H)[0] > 0:
                        y_star = np.linalg.solve(H, b.reshape(-1))
                        bound = _kappa_bound(H, y_star, SR.TRUE_RESIDUAL_OVER_TOL_CPU * TOL)
                        assert np.linalg.norm(s64.y.reshape(-1) - y_star) <= bound, (label, which, gn, c)
                    n_ok += 1
                n_neg[(label, variant, which, gn)] = neg
                print("%-14s %-6s (%s) %-12s negative curvature on %d of %d components" % (label, variant, which, "gauss-newton" if gn else "exact", neg, len(comps)))
    print("TRUE_RESIDUAL_OVER_TOL_CPU: measured %.4f over %d solves, recorded %.4g" % (worst_res, n_ok, SR.TRUE_RESIDUAL_OVER_TOL_CPU))
    print("ITERATIONS_OVER_ROWS_CPU: measured %.4f, recorded %.4g" % (worst_it, SR.ITERATIONS_OVER_ROWS_CPU))
    assert 0.5 * SR.TRUE_RESIDUAL_OVER_TOL_CPU <= worst_res <= SR.TRUE_RESIDUAL_OVER_TOL_CPU
    assert 0.5 * SR.ITERATIONS_OVER_ROWS_CPU <= worst_it <= SR.ITERATIONS_OVER_ROWS_CPU
    # the sets the GPU test uses: Gauss-Newton converges everywhere; the exact Hessian converges at the oracle's positions on the
    # class-limit shapes and meets negative curvature on every component at positions_b
    for (label, variant, which, gn), neg in n_neg.items():
        if gn:
            assert neg == 0
        elif label == "class_limits":
            assert neg == (0 if which == "a" else len(CL.NAMES)), (which, neg)


def test_longdouble_and_float64_agree():
    label, variant, comps, sets = inputs()[0]
    bs = SR.rhs(len(sets["a"]), 1)[0]
    for c, (var_nodes, ed) in list(comps.items())[:6]:
        x, b = sets["a"][var_nodes], bs[var_nodes]
        ld, f64 = SR.solve(ed, x, b, variant, True), SR.solve(ed, x, b, variant, True, dtype=np.float64)
        assert ld.status == f64.status == SR.OK and abs(ld.iterations - f64.iterations) <= 2
        H = _dense(_component(ed, variant), x, True, False)
        y_star = np.linalg.solve(H, b.reshape(-1))
        assert np.linalg.norm(ld.y.astype(np.float64).reshape(-1) - y_star) <= _kappa_bound(H, y_star, SR.TRUE_RESIDUAL_OVER_TOL_CPU * TOL)


# ------------------------------------------------------------------------------------------------------------ 2. the large ring
def test_the_ring_of_6146_rows_converges_within_half_its_cap():
    """the condition of the GPU test's largest case: Gauss-Newton, max_iterations = 4 x rows, the float64 restatement converges in at
    most half of that at SR.RING_DAMPING (a cap, not a measurement)"""
    import lfr_oracle as O
    from lfr_amd import synthetic
    ma = synthetic.generate(seed=31, n_images=3074, n_tracks=1, len_dist="uniform", len_lo=3074, len_hi=3074, track_degree=2)      # test_gpu_class_limits._ring(3074)
    ref = O.run(ma, n_threads=4)
    assert ref["rc"] == 0
    comps = CR.oracle_components(ma, ref)
    (var_nodes, ed), = comps.values()
    assert 2 * ed.nv == 6146
    b = SR.rhs(len(ref["positions"]), 1)[0][var_nodes]
    s = SR.solve(ed, ref["positions"][var_nodes], b, gauss_newton=True, damping=SR.RING_DAMPING, rel_tolerance=TOL, max_iterations=2 * 6146, dtype=np.float64)
    print("ring of 6146 rows: status %d after %d steps (cap %d, half of it %d)" % (s.status, s.iterations, 4 * 6146, 2 * 6146))
    assert s.status == SR.OK and s.iterations <= 2 * 6146


# ------------------------------------------------------------------------------------------------------------ 3. hand-made facts
def test_zero_bound_saturated_damping_and_first_direction():
    ed, x = _tukey_at_work(600)
    rng = np.random.default_rng(9420)
    b = rng.standard_normal((2, 2))
    for gn in (False, True):
        z = SR.solve(ed, x, np.zeros((2, 2)), gauss_newton=gn)
        assert z.status == SR.OK and z.iterations == 0 and z.residual == 0 and not z.y.any()
    # a saturated Tukey edge taken out changes nothing, bit for bit
    far = CR.Edges(1, np.array([0]), np.array([-1]), np.array([1.0], LD), np.array([CR.KIND_INTER]), np.zeros((1, 9, 2), LD), np.array([0]))
    assert not HR.product(far, [[0.3, 0.0]], [[1.0, -2.0]]).hv.any()
    cauchy = dataclasses.replace(ed, kind=np.full(len(ed), CR.KIND_INTRA))
    xs = np.array(x, np.float64)
    one = SR.solve(cauchy, xs, b, gauss_newton=True, dtype=np.float64)
    sat = CR.Edges(ed.nv, np.append(cauchy.src, 0), np.append(cauchy.dst, -1), np.append(cauchy.w, LD(1)), np.append(cauchy.kind, CR.KIND_INTER),
                   np.concatenate([cauchy.flow, np.zeros((1, 9, 2), cauchy.flow.dtype)]), np.append(cauchy.eids, 0))
    xfar = xs.copy()
    xfar[0] = [0.3, 0.0]                                      # 0.3 from the constant at the origin: beyond the Tukey radius of 0.25
    with_edge, without = (SR.solve(e_, xfar, b, gauss_newton=True, dtype=np.float64) for e_ in (sat, cauchy))
    assert with_edge.status == without.status == SR.OK and with_edge.iterations == without.iterations and np.array_equal(with_edge.y, without.y)
    # a bound row: y_i = b_i, the very bits, and b_i moves no other row
    xb = xs.copy()
    xb[0, 1] = 1.0
    a = SR.solve(cauchy, xb, b, gauss_newton=True, free_set=True, dtype=np.float64)
    b2 = b.copy()
    b2[0, 1] = 7.0
    c = SR.solve(cauchy, xb, b2, gauss_newton=True, free_set=True, dtype=np.float64)
    keep = np.ones((2, 2), bool)
    keep[0, 1] = False
    assert a.status == c.status == SR.OK and a.n_bound == 1 and a.y[0, 1] == b[0, 1] and c.y[0, 1] == 7.0
    assert np.array_equal(a.y[keep], c.y[keep]) and a.iterations == c.iterations
    assert one.status == SR.OK and not np.array_equal(one.y[keep], a.y[keep])
    # damping shifts the spectrum: (H + d I) y = b against the dense matrix
    H = _dense(_component(cauchy, "ceres1"), xs, True, False)
    for d in (0.0, 0.5, 40.0):
        s = SR.solve(cauchy, xs, b, gauss_newton=True, damping=d, dtype=np.float64)
        y_star = np.linalg.solve(H + d * np.eye(4), b.reshape(-1))
        assert s.status == SR.OK and np.linalg.norm(s.y.reshape(-1) - y_star) <= _kappa_bound(H + d * np.eye(4), y_star, SR.TRUE_RESIDUAL_OVER_TOL_CPU * TOL)
    # negative curvature on the first direction returns zeros: one node held to a constant by a Cauchy edge far out on its loss,
    # where rho' + 2 rho'' s < 0 along the residual; damping above -lambda_min cures it
    one_edge = CR.Edges(1, np.array([0]), np.array([-1]), np.array([1.0], LD), np.array([CR.KIND_INTRA]), np.zeros((1, 9, 2), LD), np.array([0]))
    xo, bo = np.array([[0.9, 0.0]]), np.array([[1.0, 0.0]])
    Ho = _dense(_component(one_edge, "ceres1"), xo, False, False)
    lam = np.linalg.eigvalsh(Ho)
    assert lam[0] < 0
    s = SR.solve(one_edge, xo, bo, dtype=np.float64)
    assert s.status == SR.NEGATIVE_CURVATURE and s.iterations == 0 and not s.y.any() and s.residual == 1
    cured = SR.solve(one_edge, xo, bo, damping=float(-lam[0]) + 0.5, dtype=np.float64)
    assert cured.status == SR.OK and np.allclose(cured.y.reshape(-1), np.linalg.solve(Ho + (0.5 - lam[0]) * np.eye(2), bo.reshape(-1)), rtol=1e-9, atol=0)
