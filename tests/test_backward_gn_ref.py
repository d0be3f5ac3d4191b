"""The CPU reference of the backward's Gauss-Newton mode (tests/backward_gn_ref.py) tied to the references the project already has,
and the inputs tests/test_gpu_backward_gn.py leans on checked for what they are there for.  No GPU."""
import numpy as np
import pytest

import backward_gn_ref as GN
import backward_ref as BR
import class_limit_cases as CL
import covariance_ref as CR
import lfr_oracle as O
import lm_decision_cases as LC


def _oracle_components(ma, ref, which=None, variant="ceres1"):
    """{component: (var_nodes, exact-mode Component)} from the oracle's labels"""
    idx = {n: i for i, n in enumerate(ma.image_names)}
    node_image = np.array([idx[n] for n in ref["image_names"]], np.int32)[ref["node_image"]]
    return BR.graph_components(ma, ref["track"], ref["is_root"], ref["comp"], node_image, ref["node_feat"], variant, which=which)


def test_gauss_newton_matrix_is_the_covariance_references_normal_matrix():
    """H_GN summed per edge in torch against J^T J of oracle/lfr_ref.py's corrected Jacobian (covariance_ref.normal_matrix) at the
    oracle's positions: two restatements of the same matrix, each entry a sum of at most 16 products with a few roundings each -
    1e-12 of the largest entry is the parity the project holds its device-assembled matrices to (covariance_ref.PARITY)"""
    ma = CL.alone("k5")
    ref = O.run(ma, n_threads=2)
    assert ref["rc"] == 0
    (var_nodes, cp), = _oracle_components(ma, ref).values()
    x = ref["positions"][var_nodes].reshape(-1)
    assert len(x) == 8 and np.abs(x).max() < 1.0
    H = GN.Component.of(cp).hessian(x)
    A = CR.normal_matrix(CR.problem_of(cp), x)
    err = np.abs(H - A).max()
    print("k5: max |H_GN - J^T J| = %.3e, max |J^T J| = %.3e" % (err, np.abs(A).max()))
    assert err <= CR.PARITY * np.abs(A).max()
    assert np.array_equal(H, H.T) or np.abs(H - H.T).max() <= 1e-15 * np.abs(H).max()
    assert GN.Component.of(cp).is_positive_definite(x)


def test_gauss_newton_equals_exact_where_the_residuals_vanish():
    """flows without noise and without an affine part are consistent: at the minimum every residual is 0 (to the float32 rounding of
    the flows), the exact Hessian loses its rho'' and second-derivative terms, and both references give the same gradient"""
    ma = CL.tracks(41, [6, (9, 12, 2), 4], sigma_noise=0.0, sigma_A=0.0)
    ref = O.run(ma, n_threads=2)
    assert ref["rc"] == 0
    comps = _oracle_components(ma, ref)
    assert len(comps) == 3
    rng = np.random.default_rng(42)
    for c, (var_nodes, cp) in comps.items():
        x, g = cp.newton_polish(ref["positions"][var_nodes].reshape(-1))
        assert g < 1e-12 and np.abs(x).max() < 1.0
        z = cp._z(x)
        r = (z[:, 2:] - z[:, :2] - BR.interpolate(cp.flow, z[:, 0], z[:, 1])).numpy()
        assert np.abs(r).max() < 1e-6
        ubar = rng.standard_normal(len(x))
        ef, ew, es = cp.backward(x, ubar)
        gf, gw, gs = GN.Component.of(cp).backward(x, ubar)
        assert es == 0 and gs == 0 and ef.any() and ew.any()
        exact, gn = np.concatenate([ef.ravel(), ew]), np.concatenate([gf.ravel(), gw])
        rel = np.linalg.norm(gn - exact) / np.linalg.norm(exact)
        print("component %d: max |r| %.2e, |GN - exact| / |exact| = %.2e" % (c, np.abs(r).max(), rel))
        assert rel <= 1e-6


def test_singular_component_is_status_2():
    """a leaf tied in by one match of similarity 0: its rows of H_GN vanish, the reference reports 2 and zeros"""
    import lfr_ref as R
    z = np.zeros(18)
    edges = [(-1, 0, 0.9, R.KIND_INTRA, z), (0, -1, 0.9, R.KIND_INTRA, z), (0, 1, 0.0, R.KIND_INTRA, z), (1, 0, 0.0, R.KIND_INTRA, z)]
    cp = GN.Component(2, edges)
    gf, gw, st = cp.backward(np.array([0.01, -0.02, 0.03, 0.0]), np.ones(4))
    assert st == 2 and not gf.any() and not gw.any()


@pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
def test_every_class_limit_shape_is_positive_definite(variant):
    ma, feats = CL.all_shapes()
    ref = O.run(ma, n_threads=4, tukey_variant=variant)
    assert ref["rc"] == 0
    comps = _oracle_components(ma, ref, variant=variant)
    assert len(comps) == len(CL.NAMES)
    for c, (var_nodes, cp) in comps.items():
        assert GN.Component.of(cp).is_positive_definite(ref["positions"][var_nodes].reshape(-1)), c


@pytest.mark.parametrize("name", ["packed_24_32", "block_m"])
def test_decision_cases_hold_components_at_the_bound_to_check(name):
    """every component is a single-track ring of Cauchy edges (rho' > 0) with a root: H_GN is positive definite analytically; asserted
    anyway, with the count of non-sensitive components that have a coordinate at the bound"""
    ma, ref, sensitive = LC.reference(name)
    comps = _oracle_components(ma, ref)
    at_bound = set(np.setdiff1d(LC.components_at_bound(ref), sensitive).tolist())
    n = 0
    for c, (var_nodes, cp) in comps.items():
        x = ref["positions"][var_nodes].reshape(-1)
        assert (cp.kind.numpy() == 0).all()
        assert GN.Component.of(cp).is_positive_definite(x), c
        if c in at_bound:
            assert not cp.free(x).all()
            n += 1
    print("%s: %d components, %d outside the sensitive set with a coordinate at the bound, all positive definite" % (name, len(comps), n))
    assert n >= 5
