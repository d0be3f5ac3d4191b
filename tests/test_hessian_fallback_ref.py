"""The CPU reference of the Gauss-Newton fallback (tests/hessian_fallback_ref.py): which of the three outcomes it picks, that it returns
the named reference's values unchanged, and the adjoint identity between its backward and its jvp in every outcome.  No GPU."""
import numpy as np
import pytest

import backward_gn_ref as GN
import backward_ref as BR
import hessian_fallback_ref as FR
import jvp_ref as JR
from test_jvp_ref import _bound_component, _tangent


def _indefinite():
    """test_backward_ref.test_indefinite_hessian_gives_zero's program: a Tukey edge where rho is concave in x"""
    return BR.Component(1, [(0, -1, 1.0, 1, np.zeros(18))]), np.array([0.06, 0.0])


def _positive_definite():
    """test_backward_ref.test_implicit_gradient_with_an_active_bound's program (Cauchy edges, one coordinate at the bound)"""
    return _bound_component(np.random.default_rng(3))


def _weight0_leaf():
    """node 0 tied to the root by a Cauchy match, node 1 tied to node 0 by a match of similarity 0 only: its rows of both matrices
    are zero"""
    rng = np.random.default_rng(5)
    flow = lambda c: np.tile(np.asarray(c, np.float64), 9) + rng.uniform(-0.02, 0.02, 18)
    edges = [(-1, 0, 0.9, 0, flow([0.2, 0.1])), (0, -1, 0.9, 0, flow([-0.2, -0.1])),
             (0, 1, 0.0, 0, flow([0.1, -0.2])), (1, 0, 0.0, 0, flow([-0.1, 0.2]))]
    return BR.Component(2, edges), np.array([0.19, 0.11, 0.3, -0.1])


def test_indefinite_exact_hessian_takes_the_gauss_newton_reference():
    comp, x = _indefinite()
    ubar = np.ones(2)
    assert comp.backward(x, ubar)[2] == 2
    gf, gw, status, kappa = FR.backward(comp, x, ubar)
    wf, ww, ws = GN.Component.of(comp).backward(x, ubar)
    assert status == FR.FALLBACK == 3 and ws == 0
    assert np.array_equal(gf, wf) and np.array_equal(gw, ww) and gf.any() and gw.any()
    assert kappa == GN.Component.of(comp).kappa2(x) and np.isfinite(kappa)
    # the Gauss-Newton view of the same component gives the same composition
    gf2, gw2, status2, _ = FR.backward(GN.Component.of(comp), x, ubar)
    assert status2 == 3 and np.array_equal(gf, gf2) and np.array_equal(gw, gw2)
    fd, sd = np.ones((1, 18)), np.ones(1)
    xdot, js, _ = FR.jvp(comp, x, fd, sd)
    want, wjs = JR.jvp(comp, x, fd, sd, gauss_newton=True)
    assert js == 3 and wjs == 0 and np.array_equal(xdot, want) and xdot.any()


def test_positive_definite_hessian_takes_the_exact_reference():
    comp, x = _positive_definite()
    ubar = np.random.default_rng(0).standard_normal(len(x))
    gf, gw, status, kappa = FR.backward(comp, x, ubar)
    wf, ww, ws = comp.backward(x, ubar)
    assert status == FR.OK == 0 and ws == 0 and np.array_equal(gf, wf) and np.array_equal(gw, ww) and gf.any()
    assert 1.0 <= kappa < np.inf
    nf, _, _ = GN.Component.of(comp).backward(x, ubar)
    assert not np.array_equal(gf, nf)                            # (the two modes differ here: the composition did pick one)
    fd, sd = _tangent(comp, np.random.default_rng(1))
    xdot, js, _ = FR.jvp(comp, x, fd, sd)
    want, wjs = JR.jvp(comp, x, fd, sd)
    assert js == 0 and wjs == 0 and np.array_equal(xdot, want) and xdot[0] == 0.0 and xdot[1:].all()


def test_weight0_leaf_fails_both_factorizations():
    comp, x = _weight0_leaf()
    ubar = np.ones(4)
    assert comp.backward(x, ubar)[2] == 2 and GN.Component.of(comp).backward(x, ubar)[2] == 2
    gf, gw, status, kappa = FR.backward(comp, x, ubar)
    assert status == FR.INDEFINITE == 2 and not gf.any() and not gw.any() and kappa == np.inf
    assert gf.shape == (4, 18) and gw.shape == (4,)
    xdot, js, _ = FR.jvp(comp, x, *_tangent(comp, np.random.default_rng(2)))
    assert js == 2 and not xdot.any() and xdot.shape == (4,)


@pytest.mark.parametrize("case,want", [(_indefinite, 3), (_positive_definite, 0), (_weight0_leaf, 2)], ids=["fallback", "exact", "zeros"])
def test_adjoint_identity_between_the_two_compositions(case, want):
    """ubar . (J thetadot) = (J^T ubar) . thetadot to 1e-12 relative, with equal statuses (test_jvp_ref's bound)"""
    comp, x = case()
    rng = np.random.default_rng(7)
    fd, sd = _tangent(comp, rng)
    ubar = rng.standard_normal(len(x))
    gf, gw, rs, _ = FR.backward(comp, x, ubar)
    xdot, js, _ = FR.jvp(comp, x, fd, sd)
    assert rs == js == want
    many = FR.jvp_many([(comp, x, fd, sd)])
    assert many[0][1] == js and np.linalg.norm(many[0][0] - xdot) <= 1e-12 * np.linalg.norm(xdot)
    fr = comp.free(x)
    lhs = float(ubar[fr] @ xdot[fr])
    rhs = float((gf * fd).sum() + (gw * sd).sum())
    scale = np.linalg.norm(ubar[fr]) * np.linalg.norm(xdot) + np.linalg.norm(np.concatenate([gf.ravel(), gw])) * np.linalg.norm(np.concatenate([fd.ravel(), sd]))
    assert abs(lhs - rhs) <= 1e-12 * scale
    assert (lhs != 0.0) == (want != 2)
