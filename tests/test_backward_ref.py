"""The CPU reference of the implicit-gradient backward (tests/backward_ref.py) against the oracle and against finite differences of
a Newton-polished optimum.  No GPU."""
import numpy as np
import pytest
import torch

import backward_ref as BR
import lfr_ref as R
from lfr_amd import capi, synthetic


def _components(ma, variant="ceres1", max_nv=None):
    pairs = ma.to_pairs()
    res = R.solve_pairs(pairs, tukey_variant=variant, bisect_fn=capi.bisect_graph)
    g = R.MatchGraph(pairs)
    nodes_in = {}
    for n, c in enumerate(res["comp"]):
        nodes_in.setdefault(c, []).append(n)
    out = []
    for c, info in res["infos"].items():
        var_nodes, edges = R.assemble_component(g, res["track"], res["is_root"], res["comp"], nodes_in[c])
        if not var_nodes or (max_nv and len(var_nodes) > max_nv):
            continue
        comp = BR.Component(len(var_nodes), [e for e in edges if not (e[0] < 0 and e[1] < 0)], variant)
        out.append((comp, res["positions"][var_nodes].reshape(-1), info))
    return out


def test_torch_cost_equals_oracle_final_cost():
    ma = synthetic.generate(seed=4, n_images=8, n_tracks=30, eps_out=0.05)
    comps = _components(ma)
    assert len(comps) >= 10
    for comp, x, info in comps:
        if info["termination"] == R.TERM_FAILURE:
            continue
        assert float(comp.cost(x)) == pytest.approx(info["final_cost"], rel=1e-12, abs=1e-18)


def test_gradient_matches_finite_differences():
    ma = synthetic.generate(seed=6, n_images=6, n_tracks=12, eps_out=0.1)
    rng = np.random.default_rng(0)
    for comp, x, _ in _components(ma)[:6]:
        x = x + rng.uniform(-0.05, 0.05, x.shape)
        g = comp.grad(x)
        h = 1e-6
        fd = np.array([(float(comp.cost(x + h * e)) - float(comp.cost(x - h * e))) / (2 * h) for e in np.eye(len(x))])
        assert np.abs(g - fd).max() <= 1e-6 * (1 + np.abs(fd).max())


def _check_implicit(comp, x_hat, rng, n_probe=6):
    x, gn = comp.newton_polish(x_hat)
    assert gn < 1e-12
    fr = comp.free(x)
    ubar = rng.standard_normal(len(x))
    gf, gw, status = comp.backward(x, ubar)
    assert status == 0
    E = len(comp.src)

    def loss(flow=None, sim=None):
        xs, gn2 = comp.newton_polish(x, flow=flow, sim=sim)
        assert gn2 < 1e-11
        assert (comp.free(xs) == fr).all()
        return float(ubar[fr] @ xs[fr])

    h = 1e-6
    checked = 0
    for e in rng.choice(E, size=min(n_probe, E), replace=False):
        k = int(rng.integers(18))
        fp, fm = comp.flow.clone(), comp.flow.clone()
        fp[e, k] += h
        fm[e, k] -= h
        fd = (loss(flow=fp) - loss(flow=fm)) / (2 * h)
        assert fd == pytest.approx(gf[e, k], rel=1e-4, abs=1e-7)
        sp, sm = comp.sim.clone(), comp.sim.clone()
        sp[e] += h
        sm[e] -= h
        fd = (loss(sim=sp) - loss(sim=sm)) / (2 * h)
        assert fd == pytest.approx(gw[e], rel=1e-4, abs=1e-7)
        checked += 1
    return checked, fr


@pytest.mark.parametrize("variant,sigma,eps", [("ceres1", 0.04, 0.1), ("ceres2", 0.04, 0.1), ("ceres1", 0.0, 0.0)])
def test_implicit_gradient_matches_finite_differences(variant, sigma, eps):
    """Cauchy edges, both Tukey flavours (inter-track edges from wrong matches), and the noise-free case."""
    ma = synthetic.generate(seed=9, n_images=8, n_tracks=30, eps_out=eps, sigma_noise=sigma)
    rng = np.random.default_rng(1)
    n = 0
    kinds = set()
    comps = sorted(_components(ma, variant, max_nv=8), key=lambda t: -int((t[0].kind == 1).any()))      # Tukey edges first
    for comp, x, info in comps[:5]:
        if info["termination"] == R.TERM_FAILURE:
            continue
        kinds |= set(comp.kind.tolist())
        n += _check_implicit(comp, x, rng)[0]
    assert n >= 10
    if eps > 0:
        assert kinds == {0, 1}


def test_implicit_gradient_with_an_active_bound():
    """A flow that pushes a node past +1: that coordinate is held at the bound and gets no gradient through it."""
    rng = np.random.default_rng(3)
    flow = lambda c: np.tile(np.asarray(c, np.float64), 9) + rng.uniform(-0.02, 0.02, 18)
    edges = [(-1, 0, 0.9, 0, flow([1.4, 0.1])), (0, -1, 0.9, 0, flow([-1.4, -0.1])),
             (-1, 1, 0.8, 0, flow([0.2, -0.3])), (1, -1, 0.8, 0, flow([-0.2, 0.3])),
             (0, 1, 0.7, 0, flow([-1.2, -0.4])), (1, 0, 0.7, 0, flow([1.2, 0.4]))]
    comp = BR.Component(2, edges)
    x, info = R.solve_problem(R.Problem(2, edges))
    assert info["termination"] != R.TERM_FAILURE
    assert x[0] == 1.0
    checked, fr = _check_implicit(comp, x, rng, n_probe=6)
    assert not fr[0] and fr[1:].all() and checked == 6


def test_indefinite_hessian_gives_zero():
    """A Tukey edge at a maximum of its loss: H is not positive definite, the gradient is zero and reported."""
    edges = [(0, -1, 1.0, 1, np.zeros(18))]
    comp = BR.Component(1, edges)
    x = np.array([0.06, 0.0])          # |r| just below the Tukey radius, where rho is concave in x
    H = comp.hessian(x)
    assert np.linalg.eigvalsh(H).min() < 0
    gf, gw, status = comp.backward(x, np.ones(2))
    assert status == 2 and not gf.any() and not gw.any()
    assert torch.isfinite(torch.as_tensor(gf)).all()
