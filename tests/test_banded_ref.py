"""tests/banded_ref.py against the dense references it stands in for (backward_ref, jvp_ref, covariance_ref), on a ring small enough for
both, at the oracle's positions: the 6144-row tests of tests/test_gpu_class_limits.py and tests/test_gpu_jvp_class_limits.py rest on it."""
import copy

import numpy as np
import pytest

import backward_gn_ref as GN
import backward_ref as BR
import banded_ref as BD
import covariance_ref as CR
import jvp_ref as JR
import lfr_oracle as O
from lfr_amd import synthetic


@pytest.fixture(scope="module", params=["ceres1", "ceres2"])
def ring(request):
    n = 61
    ma = synthetic.generate(seed=31, n_images=n, n_tracks=1, len_dist="uniform", len_lo=n, len_hi=n, track_degree=2)
    ref = O.run(ma, n_threads=1, tukey_variant=request.param)
    assert ref["rc"] == 0 and ref["n_components"] == 1 and ref["comp_nvar"][0] == n - 1
    idx = {name: i for i, name in enumerate(ma.image_names)}
    ni = np.array([idx[name] for name in ref["image_names"]], np.int32)[ref["node_image"]]
    var_nodes, cp = BR.graph_components(ma, ref["track"], ref["is_root"], ref["comp"], ni, ref["node_feat"], request.param)[0]
    return cp, ref["positions"][var_nodes].reshape(-1)


def test_backward_equals_the_dense_reference(ring):
    cp, x = ring
    ubar = np.random.default_rng(1).standard_normal(len(x))
    gf, gw, rs = cp.backward(x, ubar)
    bf, bw, bs = BD.backward(cp, x, ubar)
    assert rs == bs == 0
    ref, got = np.concatenate([gf.ravel(), gw]), np.concatenate([bf.ravel(), bw])
    assert np.linalg.norm(got - ref) <= 1e-11 * np.linalg.norm(ref)          # two backward-stable float64 solves of one system
    assert np.abs(BD.sparse_hessian(cp, x).toarray() - cp.hessian(x)).max() <= 1e-12 * np.abs(cp.hessian(x)).max()
    # a coordinate held at the bound: its row and column leave the system on both sides
    xb = x.copy()
    xb[5] = 1.0
    gf, gw, rs = cp.backward(xb, ubar)
    bf, bw, bs = BD.backward(cp, xb, ubar)
    assert rs == bs
    assert np.linalg.norm(np.concatenate([(bf - gf).ravel(), bw - gw])) <= 1e-11 * np.linalg.norm(np.concatenate([gf.ravel(), gw]))


@pytest.mark.parametrize("gn", [False, True], ids=["exact", "gauss_newton"])
def test_jvp_equals_the_dense_reference(ring, gn):
    """banded_ref.jvp against jvp_ref.jvp at the agreement demanded of banded_ref.backward above: the same right-hand side, two
    backward-stable solves of one system (float64 dense, longdouble banded)"""
    cp, x = ring
    rng = np.random.default_rng(2)
    E = len(cp.src)
    fdot, sdot = rng.standard_normal((E, 18)), rng.standard_normal(E)
    H = GN.Component.of(cp).hessian(x) if gn else cp.hessian(x)
    assert np.abs(BD.sparse_hessian(cp, x, gn).toarray() - H).max() <= 1e-12 * np.abs(H).max()
    ref, rs = JR.jvp(cp, x, fdot, sdot, gauss_newton=gn)
    got, bs = BD.jvp(cp, x, fdot, sdot, gauss_newton=gn)
    assert rs == bs == 0 and ref.any() and got.dtype == np.float64
    assert np.linalg.norm(got - ref) <= 1e-11 * np.linalg.norm(ref)
    # coordinates held at the bound: identity rows on both sides, exact zeros in both tangents
    xb = x.copy()
    xb[5], xb[40] = 1.0, -1.0
    ref, rs = JR.jvp(cp, xb, fdot, sdot, gauss_newton=gn)
    got, bs = BD.jvp(cp, xb, fdot, sdot, gauss_newton=gn)
    assert rs == bs
    assert np.linalg.norm(got - ref) <= 1e-11 * np.linalg.norm(ref)
    assert not got[[5, 40]].any() and not ref[[5, 40]].any()
    red = BD.reduced_hessian(cp, xb, gn).toarray()
    assert red[5, 5] == red[40, 40] == 1.0 and np.count_nonzero(red[5]) == np.count_nonzero(red[:, 40]) == 1
    # a matrix that is not positive definite: zeros and status 2 on both sides
    cn = copy.copy(cp)
    cn.sim = -cp.sim
    ref, rs = JR.jvp(cn, x, fdot, sdot, gauss_newton=gn)
    got, bs = BD.jvp(cn, x, fdot, sdot, gauss_newton=gn)
    assert rs == bs == 2 and not ref.any() and not got.any()


def test_inverse_and_bound_equal_the_dense_reference(ring):
    cp, x = ring
    problem = CR.problem_of(cp)
    A = CR.normal_matrix(problem, x)
    As = BD.normal_matrix(problem, x, chunk=32)
    assert np.abs(As.toarray() - A).max() <= 1e-13 * np.abs(A).max()
    n = A.shape[0]
    inv = BD.Inverse(As)
    cols = [0, 1, 2 * 17, 2 * 17 + 1, n - 2, n - 1]
    X = inv.columns(cols)
    want = CR.inverse_refined(A, cols)
    assert float(np.max(np.abs(X - want))) <= 64 * n * 2.0 ** -64 * inv.norm_inf * inv.inv_norm_inf * float(np.max(np.abs(want)))
    # the bound: kappa_inf and kappa_2 as the dense reference computes them; the float64-inverse term may differ (another stable solver)
    ev = np.linalg.eigvalsh(A)
    assert inv.kappa2 == pytest.approx(ev[-1] / ev[0], rel=1e-6)
    kinf = float(np.max(np.sum(np.abs(A), 1))) * float(np.max(np.sum(np.abs(np.linalg.inv(A)), 1)))
    assert inv.norm_inf * inv.inv_norm_inf == pytest.approx(kinf, rel=1e-9)
    assert inv.bound(X, cols) == pytest.approx(CR.component_bound(A, want, cols), rel=1e-3)
    with pytest.raises(np.linalg.LinAlgError):
        BD.Inverse(As - 2.0 * ev[-1] * __import__("scipy.sparse").sparse.identity(n))
