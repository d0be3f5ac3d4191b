"""The CPU reference of the forward-mode sensitivity (tests/jvp_ref.py): the adjoint identity with the references of the backward
(tests/backward_ref.py, tests/backward_gn_ref.py), central finite differences of a Newton-polished optimum, and the bounds.  No GPU."""
import numpy as np
import pytest

import backward_gn_ref as GN
import backward_ref as BR
import jvp_ref as JR
import lfr_ref as R
from lfr_amd import synthetic
from test_backward_ref import _components


def _tangent(comp, rng):
    E = len(comp.src)
    return rng.standard_normal((E, 18)), rng.standard_normal(E)


@pytest.mark.parametrize("gauss_newton", [False, True], ids=["exact", "gauss_newton"])
@pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
def test_adjoint_identity_with_the_backward_reference(variant, gauss_newton):
    """ubar . (J thetadot) = (J^T ubar) . thetadot to 1e-12 relative: the two references share H and nothing else."""
    ma = synthetic.generate(seed=9, n_images=8, n_tracks=30, eps_out=0.1, sigma_noise=0.04)
    rng = np.random.default_rng(2)
    n, kinds, worst = 0, set(), 0.0
    for comp, x, info in _components(ma, variant, max_nv=10):
        if info["termination"] == R.TERM_FAILURE:
            continue
        fd, sd = _tangent(comp, rng)
        ubar = rng.standard_normal(len(x))
        back = GN.Component.of(comp) if gauss_newton else comp
        gf, gw, rs = back.backward(x, ubar)
        xdot, js = JR.jvp(comp, x, fd, sd, gauss_newton=gauss_newton)
        assert js == rs
        if rs != 0:
            assert not xdot.any()
            continue
        fr = comp.free(x)
        lhs = float(ubar[fr] @ xdot[fr])
        rhs = float((gf * fd).sum() + (gw * sd).sum())
        scale = np.linalg.norm(ubar[fr]) * np.linalg.norm(xdot) + np.linalg.norm(np.concatenate([gf.ravel(), gw])) * np.linalg.norm(np.concatenate([fd.ravel(), sd]))
        worst = max(worst, abs(lhs - rhs) / scale)
        assert abs(lhs - rhs) <= 1e-12 * scale
        kinds |= set(comp.kind.tolist())
        n += 1
    print("%s/%s: %d components, worst |lhs - rhs| / scale %.3e" % (variant, "gn" if gauss_newton else "exact", n, worst))
    assert n >= 8 and kinds == {0, 1}


def test_many_components_at_once_equal_one_at_a_time():
    ma = synthetic.generate(seed=9, n_images=8, n_tracks=30, eps_out=0.1, sigma_noise=0.04)
    rng = np.random.default_rng(4)
    items = [(comp, x) + _tangent(comp, rng) for comp, x, info in _components(ma, max_nv=10) if info["termination"] != R.TERM_FAILURE]
    assert len(items) >= 8
    for gn in (False, True):
        many = JR.jvp_many(items, gauss_newton=gn)
        statuses = set()
        for it, (xdot, status) in zip(items, many):
            ref, rs = JR.jvp(*it, gauss_newton=gn)
            assert status == rs and np.linalg.norm(xdot - ref) <= 1e-12 * np.linalg.norm(ref)
            statuses.add(rs)
        assert 0 in statuses


def _check_fd(comp, x_hat, rng, n_probe=3):
    """xdot at the polished optimum against central differences of the polished optimum along thetadot: h and the tolerance of
    test_backward_ref._check_implicit (h = 1e-6; rel 1e-4, abs 1e-7 per coordinate)."""
    x, gn = comp.newton_polish(x_hat)
    assert gn < 1e-12
    fr = comp.free(x)
    h = 1e-6
    for _ in range(n_probe):
        fd, sd = _tangent(comp, rng)
        xdot, status = JR.jvp(comp, x, fd, sd)
        assert status == 0
        xs = []
        for sgn in (1.0, -1.0):
            flow = comp.flow + sgn * h * BR.torch.as_tensor(fd)
            sim = comp.sim + sgn * h * BR.torch.as_tensor(sd)
            xp, gp = comp.newton_polish(x, flow=flow, sim=sim)
            assert gp < 1e-11 and (comp.free(xp) == fr).all()
            xs.append(xp)
        want = (xs[0] - xs[1]) / (2 * h)
        assert xdot.any()
        for got, ref in zip(xdot, want):
            assert got == pytest.approx(ref, rel=1e-4, abs=1e-7)
    return fr


@pytest.mark.parametrize("variant,sigma,eps", [("ceres1", 0.04, 0.1), ("ceres2", 0.04, 0.1), ("ceres1", 0.0, 0.0)])
def test_jvp_matches_central_finite_differences(variant, sigma, eps):
    """components with no coordinate at a bound and a definite H: Cauchy edges, both Tukey flavours, the noise-free case"""
    ma = synthetic.generate(seed=9, n_images=8, n_tracks=30, eps_out=eps, sigma_noise=sigma)
    rng = np.random.default_rng(1)
    comps = sorted(_components(ma, variant, max_nv=8), key=lambda t: -int((t[0].kind == 1).any()))      # Tukey edges first
    n = 0
    for comp, x, info in comps:
        if info["termination"] == R.TERM_FAILURE or not comp.free(x).all():
            continue
        try:
            np.linalg.cholesky(comp.hessian(comp.newton_polish(x)[0]))
        except np.linalg.LinAlgError:
            continue
        assert _check_fd(comp, x, rng).all()
        n += 1
        if n == 4:
            break
    assert n == 4


def _bound_component(rng):
    """test_backward_ref.test_implicit_gradient_with_an_active_bound's program: a flow pushes node 0 past +1"""
    flow = lambda c: np.tile(np.asarray(c, np.float64), 9) + rng.uniform(-0.02, 0.02, 18)
    edges = [(-1, 0, 0.9, 0, flow([1.4, 0.1])), (0, -1, 0.9, 0, flow([-1.4, -0.1])),
             (-1, 1, 0.8, 0, flow([0.2, -0.3])), (1, -1, 0.8, 0, flow([-0.2, 0.3])),
             (0, 1, 0.7, 0, flow([-1.2, -0.4])), (1, 0, 0.7, 0, flow([1.2, 0.4]))]
    x, info = R.solve_problem(R.Problem(2, edges))
    assert info["termination"] != R.TERM_FAILURE and x[0] == 1.0
    return BR.Component(2, edges), x


@pytest.mark.parametrize("gauss_newton", [False, True], ids=["exact", "gauss_newton"])
def test_a_bound_coordinate_gets_an_exact_zero(gauss_newton):
    rng = np.random.default_rng(3)
    comp, x = _bound_component(rng)
    fr = comp.free(x)
    assert not fr[0] and fr[1:].all()
    fd, sd = _tangent(comp, rng)
    xdot, status = JR.jvp(comp, x, fd, sd, gauss_newton=gauss_newton)
    assert status == 0 and xdot[0] == 0.0 and xdot[1:].all()
    if not gauss_newton:                 # and the free coordinates are the finite differences' with the bound held
        assert (_check_fd(comp, x, rng) == fr).all()
    # an indefinite H: zero tangent, status 2 (test_backward_ref.test_indefinite_hessian_gives_zero's program)
    bad = BR.Component(1, [(0, -1, 1.0, 1, np.zeros(18))])
    xdot, status = JR.jvp(bad, np.array([0.06, 0.0]), np.ones((1, 18)), np.ones(1))
    assert status == 2 and not xdot.any()
