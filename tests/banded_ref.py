"""backward_ref's, jvp_ref's and covariance_ref's references for ONE large sparse component (a ring of thousands of nodes), where
their dense factorizations, inverses and eigenvalues take minutes: the same quantities from a banded Cholesky after a reverse
Cuthill-McKee ordering (a ring without its root is a path: block tridiagonal).  Test infrastructure; tests/test_banded_ref.py pins
every function here to its dense counterpart on a ring small enough for both.

  backward(cp, x, ubar)        backward_ref.Component.backward with H^-1 ubar from the banded Cholesky of the exact Hessian
  jvp(cp, x, flow_dot, sim_dot, gauss_newton=False)
                               jvp_ref.jvp: its right-hand side (jvp_ref.rhs), H^-1 b from the longdouble banded Cholesky of
                               reduced_hessian(cp, x, gauss_newton), the matrix of either mode with the identity on bound rows
  normal_matrix(problem, x)    covariance_ref.normal_matrix as a sparse matrix
  Inverse(A)                   what test_gpu_covariance's comparison needs of A^-1: columns in np.longdouble (a longdouble banded
                               Cholesky, accepted by covariance_ref.inverse_refined's own residual criterion) and
                               covariance_ref.component_bound's terms - the float64 inverse is the banded Cholesky's instead of
                               numpy.linalg.inv's (both backward stable), kappa_inf from that full inverse, kappa_2 from the
                               extreme eigenvalues of the band matrix."""
import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import reverse_cuthill_mckee
from torch.func import hessian, vmap

import backward_gn_ref as GN
import backward_ref as BR
import covariance_ref as CR
import jvp_ref as JR
import lfr_ref as R
import linsolve_ref as LS

LD = LS.LD
MAX_HALF_BANDWIDTH = 16


def band(S):
    """(perm, ab, b) of a sparse symmetric matrix: S[perm][:, perm] in LAPACK's lower band storage ab[i - j, j], half bandwidth b"""
    S = sp.csr_matrix(S)
    S.sum_duplicates()
    n = S.shape[0]
    perm = np.asarray(reverse_cuthill_mckee(S, symmetric_mode=True), np.int64)
    P = S[perm][:, perm].tocoo()
    b = int(np.max(np.abs(P.row - P.col), initial=0))
    assert b <= MAX_HALF_BANDWIDTH, "not a banded system: half bandwidth %d" % b
    ab = np.zeros((b + 1, n))
    low = P.row >= P.col
    ab[P.row[low] - P.col[low], P.col[low]] = P.data[low]
    return perm, ab, b


def sparse_hessian(cp, x, gauss_newton=False):
    """backward_ref.Component.hessian (gauss_newton: backward_gn_ref.Component.hessian) as a sparse matrix"""
    if gauss_newton:
        he = GN.Component.of(cp).edge_blocks(x)
    else:
        f = lambda z, fl, w, k: BR.edge_cost(z, fl, w, k, cp.variant)
        he = vmap(hessian(f))(cp._z(x), cp.flow, cp.sim, cp.kind).numpy()        # [E, 4, 4]
    n = 2 * cp.nv
    idx = np.stack([2 * cp.src, 2 * cp.src + 1, 2 * cp.dst, 2 * cp.dst + 1], 1)
    idx[idx < 0] += n + 2                                                        # constant node -> the two spare rows
    rows = np.repeat(idx[:, :, None], 4, 2).reshape(-1)
    cols = np.repeat(idx[:, None, :], 4, 1).reshape(-1)
    return sp.coo_matrix((he.reshape(-1), (rows, cols)), shape=(n + 2, n + 2)).tocsr()[:n, :n]


def reduced_hessian(cp, x, gauss_newton=False):
    """sparse_hessian with the rows and columns of the bound coordinates replaced by the identity's: the matrix both passes factor"""
    x = np.asarray(x, np.float64).reshape(-1)
    fr = cp.free(x)
    keep = sp.diags(fr.astype(np.float64))
    return (keep @ sparse_hessian(cp, x, gauss_newton) @ keep + sp.diags((~fr).astype(np.float64))).tocsr()


def jvp(cp, x, flow_dot, sim_dot, gauss_newton=False):
    """(xdot [2 nv], status) as jvp_ref.jvp: the right-hand side is jvp_ref.rhs, the solve the longdouble banded Cholesky of
    reduced_hessian; status 2 (zeros) where that matrix is not positive definite.  Bound coordinates get an exact 0."""
    x = np.asarray(x, np.float64).reshape(-1)
    fr = cp.free(x)
    b = np.where(fr, JR.rhs(cp, x, flow_dot, sim_dot), 0.0)
    perm, ab, _ = band(reduced_hessian(cp, x, gauss_newton))
    try:
        L = _cholesky_ld(ab)
    except np.linalg.LinAlgError:
        return np.zeros(len(x)), 2
    xdot = np.zeros(len(x))
    xdot[perm] = _solve_ld(L, b[perm][:, None])[:, 0].astype(np.float64)
    xdot[~fr] = 0.0
    return xdot, 0


def backward(cp, x, ubar):
    """(grad_flow [E, 18], grad_sim [E], status) as backward_ref.Component.backward: status 2 (zeros) where H is not positive definite"""
    x = np.asarray(x, np.float64).reshape(-1)
    fr = cp.free(x)
    H = reduced_hessian(cp, x)
    rhs = np.where(fr, np.asarray(ubar, np.float64).reshape(-1), 0.0)
    E = len(cp.src)
    perm, ab, _ = band(H)
    try:
        c = sla.cholesky_banded(ab, lower=True)
    except np.linalg.LinAlgError:
        return np.zeros((E, 18)), np.zeros(E), 2
    v = np.zeros(len(x))
    v[perm] = sla.cho_solve_banded((c, True), rhs[perm])
    flow = cp.flow.clone().requires_grad_(True)
    sim = cp.sim.clone().requires_grad_(True)
    z = cp._z(x).requires_grad_(True)
    gz, = torch.autograd.grad(BR.edge_cost(z, flow, sim, cp.kind, cp.variant).sum(), z, create_graph=True)
    ve = torch.as_tensor(np.concatenate([v, np.zeros(2)]).reshape(-1, 2), dtype=torch.float64)
    V = torch.cat([ve[torch.as_tensor(cp.src)], ve[torch.as_tensor(cp.dst)]], 1)
    gf, gw = torch.autograd.grad((gz * V).sum(), (flow, sim), allow_unused=True)
    gf = torch.zeros_like(flow) if gf is None else gf
    gw = torch.zeros_like(sim) if gw is None else gw
    return -gf.detach().numpy(), -gw.detach().numpy(), 0


def normal_matrix(problem, x, chunk=256):
    """covariance_ref.normal_matrix, sparse: J^T J summed over the residual blocks `chunk` at a time"""
    x = np.asarray(x, np.float64).reshape(-1)
    n = 2 * problem.nv
    A = sp.csr_matrix((n, n))
    for i in range(0, len(problem.edges), chunk):
        _, _, J, _ = R.Problem(problem.nv, problem.edges[i:i + chunk], problem.tukey_variant).evaluate(x, True)
        Js = sp.csr_matrix(J)
        A = A + Js.T @ Js
    return A.tocsr()


def _cholesky_ld(ab):
    """lower band Cholesky factor in np.longdouble (same storage); LinAlgError at a pivot that is not positive"""
    b, n = ab.shape[0] - 1, ab.shape[1]
    a = ab.astype(LD)
    L = np.zeros_like(a)
    for j in range(n):
        m = min(b, j)
        d = a[0, j] - sum((L[k, j - k] * L[k, j - k] for k in range(1, m + 1)), LD(0))
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[0, j] = np.sqrt(d)
        for i in range(1, min(b, n - 1 - j) + 1):
            s = a[i, j] - sum((L[i + k, j - k] * L[k, j - k] for k in range(1, min(b - i, j) + 1)), LD(0))
            L[i, j] = s / L[0, j]
    return L


def _solve_ld(L, rhs):
    """(L L^T)^-1 rhs, rhs [n, m] in np.longdouble"""
    b, n = L.shape[0] - 1, L.shape[1]
    y = rhs.astype(LD).copy()
    for j in range(n):
        for k in range(1, min(b, j) + 1):
            y[j] -= L[k, j - k] * y[j - k]
        y[j] /= L[0, j]
    for j in range(n - 1, -1, -1):
        for k in range(1, min(b, n - 1 - j) + 1):
            y[j] -= L[k, j] * y[j + k]
        y[j] /= L[0, j]
    return y


def _band_matvec_ld(ab, X):
    """the band matrix (lower storage, symmetric) times X [n, m] in np.longdouble"""
    a = ab.astype(LD)
    n = a.shape[1]
    out = a[0][:, None] * X
    for k in range(1, a.shape[0]):
        out[k:] += a[k, :n - k][:, None] * X[:n - k]
        out[:n - k] += a[k, :n - k][:, None] * X[k:]
    return out


class Inverse:
    """Of a sparse symmetric positive definite A (LinAlgError otherwise): .columns(cols) -> those columns of A^-1 in np.longdouble,
    .bound(inv_cols_ld, cols) -> covariance_ref.component_bound(A, inv_cols_ld, cols)."""

    def __init__(self, A):
        self.n = A.shape[0]
        self.perm, self.ab, _ = band(A)
        self.rank = np.empty(self.n, np.int64)
        self.rank[self.perm] = np.arange(self.n)
        self.c64 = sla.cholesky_banded(self.ab, lower=True)
        self.L = _cholesky_ld(self.ab)
        self.norm_inf = float(np.max(np.asarray(abs(sp.csr_matrix(A)).sum(1))))
        ev = [float(sla.eigvals_banded(self.ab, lower=True, select="i", select_range=(i, i))[0]) for i in (0, self.n - 1)]
        self.kappa2 = ev[1] / ev[0]

    @functools.cached_property
    def _inv64(self):
        """the full float64 inverse in the band's order: only the covariance's bound needs it, the jvp's kappa_2 does not"""
        return sla.cho_solve_banded((self.c64, True), np.eye(self.n))

    @functools.cached_property
    def inv_norm_inf(self):
        return float(np.max(np.sum(np.abs(self._inv64), 1)))                         # (in the band's order; the norm does not care)

    def columns(self, cols):
        cols = list(cols)
        rhs = np.zeros((self.n, len(cols)), LD)
        rhs[self.rank[cols], range(len(cols))] = 1.0
        X = _solve_ld(self.L, rhs)
        res = float(np.max(np.abs(rhs - _band_matvec_ld(self.ab, X))))
        if not res <= 16.0 * self.n * 2.0 ** -64 * self.norm_inf * float(np.max(np.abs(X))):          # covariance_ref.inverse_refined's criterion
            raise np.linalg.LinAlgError("the longdouble banded solve did not reach a longdouble-stable residual")
        return X[self.rank]

    def bound(self, inv_cols_ld, cols):
        cols = list(cols)
        inv64 = self._inv64[np.ix_(self.rank, self.rank[cols])]
        lap = float(np.max(np.abs(inv64.astype(LD) - inv_cols_ld)))
        big = float(np.max(np.abs(inv_cols_ld)))
        probe = max(16.0 * lap, 4.0 * self.n * CR.U * self.norm_inf * self.inv_norm_inf * big)
        return probe + 2.0 * self.kappa2 * CR.PARITY * big
