"""The CPU reference of the per-keypoint covariance (tests/covariance_ref.py) pinned by known answers, and the host-side parts of the
feature (lfr_keypoint_covariances, the exported ABI).  No GPU."""
import numpy as np
import pytest

import backward_ref as BR
import covariance_ref as CR
import lfr_ref as R
import linsolve_ref as LS
from lfr_amd import capi, synthetic


def _two_node(w):
    """One root (constant) and one variable node joined by one match with all-zero flows: both directed edges have r = 0."""
    z = np.zeros(18)
    return R.Problem(1, [(-1, 0, w, R.KIND_INTRA, z), (0, -1, w, R.KIND_INTRA, z)])


@pytest.mark.parametrize("w", [0.25, 0.7, 1.0, 3.0])
def test_two_node_known_answer(w):
    """rho'(0) = 1 (Cauchy), J = sqrt(w) (+-I) per edge: A = 2 w I, C = I / (2 w)."""
    A = CR.normal_matrix(_two_node(w), np.zeros(2))
    assert np.allclose(A, 2 * w * np.eye(2), rtol=4e-16, atol=0)
    C = CR.inverse_ld(A)
    assert np.allclose(C.astype(np.float64), np.eye(2) / (2 * w), rtol=1e-15, atol=0)
    assert np.allclose(CR.node_blocks(C, [0, 1]).astype(np.float64), [[1 / (2 * w), 0.0, 1 / (2 * w)]], rtol=1e-15)


def _zero_residual_component(rng, nv=5):
    """A chain root - 0 - 1 - ... with flows f(x) = c constant (all nine grid values equal), placed so that every residual is 0."""
    x = rng.uniform(-0.3, 0.3, (nv, 2))
    xe = np.vstack([x, np.zeros((1, 2))])
    edges = []
    for a, b in [(-1, 0)] + [(i, i + 1) for i in range(nv - 1)] + [(0, nv - 1)]:
        for s, d in ((a, b), (b, a)):
            c = xe[d] - xe[s]                                   # r = x_dst - x_src - f = 0
            edges.append((s, d, float(rng.uniform(0.2, 1.0)), R.KIND_INTRA if a < 0 or b == a + 1 else R.KIND_INTER,
                          np.tile(c, 9)))
    return x.reshape(-1), edges


def test_normal_matrix_is_the_backward_reference_hessian_at_zero_residuals():
    """With r = 0 the exact Hessian loses its rho'' r r^T and r . d2f terms: what remains is J^T J."""
    rng = np.random.default_rng(3)
    x, edges = _zero_residual_component(rng)
    A = CR.normal_matrix(R.Problem(5, edges), x)
    H = BR.Component(5, edges).hessian(x)
    assert np.abs(A - H).max() <= 1e-13 * np.abs(H).max()
    assert CR.is_positive_definite(A)
    assert np.abs(CR.normal_matrix(R.Problem(5, edges), x, chunk=3) - A).max() <= 1e-15 * np.abs(A).max()


def test_isolated_node_is_singular():
    """A leaf held by one match of similarity 0: its two rows of A are zero."""
    rng = np.random.default_rng(4)
    x, edges = _zero_residual_component(rng, nv=3)
    z = np.zeros(18)
    edges += [(2, 3, 0.0, R.KIND_INTRA, z), (3, 2, 0.0, R.KIND_INTRA, z)]
    A = CR.normal_matrix(R.Problem(4, edges), np.concatenate([x, [0.1, -0.1]]))
    assert not A[6:].any() and not CR.is_positive_definite(A)
    assert CR.is_positive_definite(A[:6, :6])


def test_refined_inverse_is_the_longdouble_inverse():
    rng = np.random.default_rng(5)
    for n, kind in ((12, "normal"), (40, "normal"), (24, "cond")):
        A = LS.normal_matrix(rng, n) if kind == "normal" else LS.spd_with_cond(rng, n, 1e8)
        cols = [0, 1, n - 2, n - 1]
        full = CR.inverse_ld(A)
        ref = CR.inverse_refined(A, cols)
        kinf = float(np.linalg.cond(A, np.inf))                  # both are longdouble-stable solves: forward errors <= ~n kappa 2^-64
        assert float(np.max(np.abs(ref - full[:, cols]))) <= 8 * n * kinf * 2.0 ** -64 * float(np.max(np.abs(full)))
        assert (CR.node_blocks(full[:, cols], cols) == CR.node_blocks(full, range(n))[[0, n // 2 - 1]]).all()
        assert CR.inverse_bound(A, full[:, cols], cols) <= CR.inverse_bound(A, full)


def test_cov_cl_replica():
    assert {CR.cov_cl("g8", n) for n in range(2, 9, 2)} == {2, 4, 6, 8}
    assert {CR.cov_cl("g64_4", n) for n in range(2, 33, 2)} == {20, 26, 28, 30, 32}


def test_keypoint_covariances_mapping(lfr_lib):
    """Hand-made case: two images, fact 1 and 0.5; pixels = (16 fact)^2, (x, y) = (dj, di)."""
    ma = synthetic.generate(seed=2, n_images=3, n_tracks=6, eps_out=0.0)
    ma.facts = np.array([1.0, 0.5, 2.0], np.float32)
    g = capi.Graph.from_arrays(ma)
    ni, nf = g.nodes()
    cov = np.zeros((g.n_nodes, 3))
    cov[:] = np.arange(1, g.n_nodes + 1)[:, None] * np.array([1.0, -0.25, 3.0])      # C(di,di), C(di,dj), C(dj,dj)
    cov[0] = 0.0                                                                      # "no covariance for this node"
    names, facts = g.image_names(), g.image_facts()
    nfeat = int(nf.max()) + 3
    for im, name in enumerate(names):
        out = g.keypoint_covariances(cov, name, nfeat)
        assert out.dtype == np.float32 and out.shape == (nfeat, 3)
        assert (out == CR.keypoint_covariances(cov, ni, nf, im, facts[im], nfeat)).all()
        n = int(np.nonzero(ni == im)[0][-1])
        s = (16.0 * facts[im]) ** 2
        assert out[nf[n]].tolist() == [np.float32(s * cov[n, 2]), np.float32(s * cov[n, 1]), np.float32(s * cov[n, 0])]
        assert not out[nfeat - 1].any()                          # a feature the graph does not know
    assert not g.keypoint_covariances(cov, "no such image", 4).any()
    with pytest.raises(capi.LfrError):
        g.keypoint_covariances(cov, names[0], 1 if nf[ni == 0].max() >= 1 else 0)


def test_abi_lists_the_covariance_symbols(lfr_lib):
    for name in ("lfr_batch_covariance", "lfr_batch_covariance_status", "lfr_keypoint_covariances", "lfr_debug_invert_spd"):
        assert name in capi.EXPORTS and hasattr(lfr_lib, name)
    assert (capi.COVARIANCE_OK, capi.COVARIANCE_NOT_USABLE, capi.COVARIANCE_SINGULAR) == (0, 1, 2)
