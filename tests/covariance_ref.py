"""CPU reference of the per-keypoint covariance (lfr_batch_covariance, include/lfr.h): A = J^T J of oracle/lfr_ref.py's Problem at a
given x (the loss-corrected Jacobian, no damping, no scaling), its inverse in np.longdouble, and the bounds the GPU tests assert.
Test infrastructure."""
import numpy as np

import lfr_ref as R
import linsolve_ref as LS

LD = LS.LD
U = LS.U
PARITY = 1e-12            # tolerance the project holds lfr_debug_eval_edges to: device-assembled against oracle-assembled A


def problem_of(cp):
    """lfr_ref.Problem from a backward_ref.Component (what backward_ref.graph_components returns)."""
    flow = cp.flow.numpy()
    edges = [(int(s), int(d), float(w), int(k), flow[i]) for i, (s, d, w, k) in
             enumerate(zip(cp.src, cp.dst, cp.sim.numpy(), cp.kind.numpy()))]
    return R.Problem(cp.nv, edges, cp.variant)


def normal_matrix(problem, x, chunk=256):
    """J.T @ J of problem.evaluate(x, True); the residual blocks are taken `chunk` at a time (the sum over blocks is the same, the
    dense Jacobian of a 2000-row component would not fit)."""
    x = np.asarray(x, np.float64).reshape(-1)
    A = np.zeros((2 * problem.nv, 2 * problem.nv))
    for i in range(0, len(problem.edges), chunk):
        _, _, J, _ = R.Problem(problem.nv, problem.edges[i:i + chunk], problem.tukey_variant).evaluate(x, True)
        A += J.T @ J
    return A


def is_positive_definite(A):
    if not np.isfinite(A).all():
        return False
    try:
        np.linalg.cholesky(A)
        return True
    except np.linalg.LinAlgError:
        return False


def inverse_ld(A, cols=None):
    """Columns `cols` (None: all) of A^-1 in np.longdouble through linsolve_ref.solve_ld on identity columns."""
    n = A.shape[0]
    cols = range(n) if cols is None else cols
    out = np.zeros((n, len(cols)), LD)
    for k, c in enumerate(cols):
        e = np.zeros(n)
        e[c] = 1.0
        out[:, k] = LS.solve_ld(A, e)
    return out


def inverse_refined(A, cols, rounds=8):
    """The same columns for systems where an elimination in longdouble per column is out of reach (thousands of rows): a float64
    factorization, then iterative refinement with longdouble residuals and updates until the correction stops shrinking.  Accepted
    when the longdouble residual is that of a backward-stable longdouble solve, |e - A x| <= 16 n 2^-64 |A| |x| (max norms) - the
    quality solve_ld's elimination has; raises otherwise.  tests/test_covariance_ref.py pins it to inverse_ld."""
    import scipy.linalg as sla
    n = A.shape[0]
    lu = sla.lu_factor(A)
    Ald = A.astype(LD)
    rhs = np.zeros((n, len(cols)), LD)
    rhs[list(cols), range(len(cols))] = 1.0
    X = sla.lu_solve(lu, rhs.astype(np.float64)).astype(LD)
    prev = np.inf
    for _ in range(rounds):
        dx = sla.lu_solve(lu, (rhs - Ald @ X).astype(np.float64)).astype(LD)
        X = X + dx
        size = float(np.max(np.abs(dx)))
        if size <= 2.0 ** -62 * float(np.max(np.abs(X))) or size > 0.25 * prev:
            break
        prev = size
    res = float(np.max(np.abs(rhs - Ald @ X)))
    if not res <= 16.0 * n * 2.0 ** -64 * float(np.max(np.sum(np.abs(A), 1))) * float(np.max(np.abs(X))):
        raise np.linalg.LinAlgError("iterative refinement did not reach a longdouble-stable residual")
    return X


def node_blocks(Cinv_cols, cols):
    """[C(2l,2l), C(2l,2l+1), C(2l+1,2l+1)] per node l from the inverse's columns (cols = 2l, 2l+1 pairs in order)."""
    cols = list(cols)
    out = np.zeros((len(cols) // 2, 3), LD)
    for k in range(0, len(cols), 2):
        i = cols[k]
        out[k // 2] = (Cinv_cols[i, k], Cinv_cols[i, k + 1], Cinv_cols[i + 1, k + 1])
    return out


def inverse_bound(A, inv_cols_ld, cols=None):
    """The probe's bound, entry-wise in the max norm (linsolve_ref.forward_bound's form): max(16 |inv_numpy - inv_ld|,
    4 n u kappa_inf(A) |inv_ld|), both maxima over the columns given (all, or `cols`: then the bound is no wider)."""
    n = A.shape[0]
    inv64 = np.linalg.inv(A)
    if cols is not None:
        inv64 = inv64[:, list(cols)]
    lap = float(np.max(np.abs(inv64.astype(LD) - inv_cols_ld)))
    kinf = float(np.max(np.sum(np.abs(A), 1))) * float(np.max(np.sum(np.abs(np.linalg.inv(A)), 1)))
    return max(16.0 * lap, 4.0 * n * U * kinf * float(np.max(np.abs(inv_cols_ld))))


def component_bound(A, inv_cols_ld, cols=None):
    """End to end: the probe's bound plus 2 kappa_2(A) 1e-12 max|C_ref| for the device-assembled against the oracle-assembled A."""
    ev = np.linalg.eigvalsh(A)
    return inverse_bound(A, inv_cols_ld, cols) + 2.0 * float(ev[-1] / ev[0]) * PARITY * float(np.max(np.abs(inv_cols_ld)))


def keypoint_covariances(cov, node_image, node_feature, image, fact, num_features):
    """The contract's pixel mapping in numpy: (16 fact)^2 [[C(dj,dj), C(di,dj)], [C(di,dj), C(di,di)]] as (xx, xy, yy) rows."""
    out = np.zeros((num_features, 3), np.float32)
    s = (16.0 * float(fact)) ** 2
    for n in np.nonzero(node_image == image)[0]:
        out[node_feature[n]] = (s * cov[n, 2], s * cov[n, 1], s * cov[n, 0])
    return out


def cov_cl(solver, n_max):
    """The column-count instantiation cov_invert picks for the largest system of a wave (a replica of its dispatch)."""
    table = {"g8": (2, 4, 6, 8), "g16": (10, 12, 14, 16), "g64_2": (18, 20, 22, 24), "g64_4": (20, 26, 28, 30, 32)}[solver]
    return [c for c in table if n_max <= c or c == table[-1]][0]
