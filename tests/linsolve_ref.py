"""Extended-precision reference for the LM step solves of the solver kernels (lfr_debug_solve_damped, lfr_debug_solve_tree), and the
systems the GPU tests feed them.

The kernels solve the damped normal equations (A + D) y = g.  The damped matrix is formed here in float64 exactly as each kernel
forms it - packed classes: a_ii + dd (one addition), workgroup classes: a_ii + d_i * d_i (one fused multiply-add, one rounding) -
elimination-tree kernel ("tree"): a_ii + round(d_i * d_i), the column task's product and sum, two roundings -
and then solved in np.longdouble (80-bit on x86-64: a 64-bit mantissa, 2^11 times finer than float64) by Gaussian elimination with
partial pivoting, so that the reference's own error lies three orders of magnitude below any float64 solve of the same system."""
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53                    # unit roundoff of float64
PACKED = ("g8", "g16", "g64_2", "g64_4")
BLOCK = ("block_s", "block_m", "block_l")
GROUPS = {"g8": 8, "g16": 4, "g64_2": 2, "g64_4": 1}          # systems per wave of a packed class


# ---- layout ----
def to_tri(M):
    """Lower triangle of a square matrix, packed row by row: (i, j), j <= i, at i (i + 1) / 2 + j."""
    n = M.shape[0]
    return np.concatenate([M[i, :i + 1] for i in range(n)]) if n else np.zeros(0)


def from_tri(t, n):
    M = np.zeros((n, n))
    k = 0
    for i in range(n):
        M[i, :i + 1] = t[k:k + i + 1]
        k += i + 1
    return M + np.tril(M, -1).T


# ---- the damped matrix, as the kernels form it ----
def damped(A, damp, solver):
    """float64 A + D: packed solvers add damp_i to a_ii, the workgroup solvers damp_i * damp_i with one rounding, the elimination-tree
    kernel ("tree") the rounded product damp_i * damp_i."""
    M = np.array(A, np.float64, copy=True)
    if solver == "tree":
        d = np.asarray(damp, np.float64)
        M[np.diag_indices_from(M)] = np.diag(M) + d * d
        return M
    for i in range(M.shape[0]):
        if solver in PACKED:
            M[i, i] = M[i, i] + damp[i]
        else:
            M[i, i] = float(Fraction(float(M[i, i])) + Fraction(float(damp[i])) ** 2)
    return M


# ---- the solve ----
def solve_ld(M, g):
    """(M) y = g in np.longdouble: Gaussian elimination with partial pivoting, M and g taken exactly.  Returns longdouble y."""
    n = M.shape[0]
    W = np.empty((n, n + 1), LD)
    W[:, :n] = np.asarray(M, np.float64).astype(LD)
    W[:, n] = np.asarray(g, np.float64).astype(LD)
    for k in range(n):
        p = k + int(np.argmax(np.abs(W[k:, k])))
        if W[p, k] == 0:
            raise np.linalg.LinAlgError("singular")
        if p != k:
            W[[k, p]] = W[[p, k]]
        f = W[k + 1:, k] / W[k, k]
        W[k + 1:, k:] -= np.outer(f, W[k, k:])
    y = np.zeros(n, LD)
    for k in range(n - 1, -1, -1):
        y[k] = (W[k, n] - np.dot(W[k, k + 1:n], y[k + 1:])) / W[k, k]
    return y


def solve_refined(M, g, rounds=8):
    """The same solution for SPD systems of thousands of rows, where solve_ld's elimination in longdouble is out of reach: a float64
    LAPACK Cholesky factorization, then iterative refinement with longdouble residuals and updates until the correction stops
    shrinking (as covariance_ref.inverse_refined).  Accepted when the longdouble residual is that of a backward-stable longdouble
    solve, |g - M y| <= 16 n 2^-64 (|M| |y| + |g|) in max norms; raises otherwise.  tests/test_linsolve_ref.py pins it to solve_ld."""
    import scipy.linalg as sla
    n = M.shape[0]
    M = np.asarray(M, np.float64)
    c = sla.cho_factor(M, lower=True)
    Mld, gld = M.astype(LD), np.asarray(g, np.float64).astype(LD)
    y = sla.cho_solve(c, np.asarray(g, np.float64)).astype(LD)
    prev = np.inf
    for _ in range(rounds):
        dy = sla.cho_solve(c, (gld - Mld @ y).astype(np.float64)).astype(LD)
        y = y + dy
        size = float(np.max(np.abs(dy)))
        if size <= 2.0 ** -62 * float(np.max(np.abs(y))) or size > 0.25 * prev:
            break
        prev = size
    res = float(np.max(np.abs(gld - Mld @ y)))
    if not res <= 16.0 * n * 2.0 ** -64 * (float(np.max(np.sum(np.abs(M), 1))) * float(np.max(np.abs(y))) + float(np.max(np.abs(g)))):
        raise np.linalg.LinAlgError("iterative refinement did not reach a longdouble-stable residual")
    return y


def residual_ld(M, y, g):
    """g - M y in np.longdouble (M, y, g taken exactly)."""
    return np.asarray(g, np.float64).astype(LD) - np.asarray(M, np.float64).astype(LD) @ np.asarray(y, np.float64).astype(LD)


# ---- the bounds the GPU tests assert (constants from the error analysis, not from the GPU's output) ----
def forward_bound(M, g, y_ref):
    """max(16 |y_lapack - y|, 4 n u kappa_inf(M) |y|) in the max norm: no worse than 16 times a plain float64 solve, or than the
    textbook bound where that solve happens to be lucky."""
    n = M.shape[0]
    y_lap = np.linalg.solve(M, g)
    ynorm = float(np.max(np.abs(y_ref)))
    lap = float(np.max(np.abs(y_lap.astype(LD) - y_ref)))
    return max(16.0 * lap, 4.0 * n * U * float(np.linalg.cond(M, np.inf)) * ynorm)


def forward_error(y, y_ref):
    return float(np.max(np.abs(np.asarray(y, np.float64).astype(LD) - y_ref)))


def backward_error(M, y, g):
    """|g - M y| / (|M| |y| + |g|), max norms, residual in np.longdouble."""
    r = residual_ld(M, y, g)
    den = float(np.max(np.sum(np.abs(M), axis=1))) * float(np.max(np.abs(y))) + float(np.max(np.abs(g)))
    return float(np.max(np.abs(r))) / den


# ---- systems ----
def normal_matrix(rng, n, disconnected=False):
    """J^T J over a random track graph of n / 2 nodes (2x2 blocks), like a component's: every node is matched to a constant
    (the fixed anchor of its track) and to a few other nodes; disconnected: no node pairs at all (block diagonal)."""
    m = n // 2
    A = np.zeros((n, n))
    for v in range(m):
        J = rng.normal(0, 1, (2, 2))
        A[2 * v:2 * v + 2, 2 * v:2 * v + 2] += J.T @ J
    if not disconnected and m > 1:
        for _ in range(2 * m):
            a, b = rng.choice(m, 2, replace=False)
            J = np.hstack([rng.normal(0, 1, (2, 2)), rng.normal(0, 1, (2, 2))]) * rng.uniform(0.1, 1.0)
            idx = [2 * a, 2 * a + 1, 2 * b, 2 * b + 1]
            A[np.ix_(idx, idx)] += J.T @ J
    return A


def spd_with_cond(rng, n, kappa):
    """Q diag(lambda) Q^T, lambda log-spaced over [1, kappa]."""
    Q, _ = np.linalg.qr(rng.normal(0, 1, (n, n)))
    lam = np.logspace(0, np.log10(kappa), n) if n > 1 else np.ones(1)
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


def graded(rng, n, kappa, span=1e6):
    """S B S with S spanning 1/span .. span (shuffled) and kappa_2(B) = kappa."""
    s = np.logspace(-np.log10(span), np.log10(span), n)
    rng.shuffle(s)
    A = s[:, None] * spd_with_cond(rng, n, kappa) * s[None, :]
    return 0.5 * (A + A.T)


def not_pd(rng, n, k, zero=False):
    """Symmetric, positive definite in its leading k x k block, the k-th pivot of an elimination without pivoting zero (row and
    column k zero) or negative (L D L^T with d_k = -1)."""
    L = np.tril(rng.normal(0, 0.3, (n, n)), -1) + np.eye(n)
    d = rng.uniform(0.5, 2.0, n)
    if zero:
        A = (L * d) @ L.T
        A[k, :] = 0.0
        A[:, k] = 0.0
        return A
    d[k] = -1.0
    A = (L * d) @ L.T
    return 0.5 * (A + A.T)


def damping_for(rng, A, solver, rel):
    """The per-row damping argument of lfr_debug_solve_damped for dd_i = rel_i * a_ii (rel may be an array): dd itself for the
    packed solvers, sqrt(dd) (the kernels' D / s) for the workgroup solvers."""
    dd = np.asarray(rel, np.float64) * np.maximum(np.diag(A), 1e-300)
    return dd if solver in PACKED else np.sqrt(dd)


def packed_cl(solver, nv2_max):
    """The CL instantiation solve_group_body's dispatch picks for the largest system of a wave (a replica of the dispatch)."""
    if solver == "g8":
        return [c for c in (2, 4, 6, 8) if nv2_max <= c or c == 8][0]
    if solver == "g16":
        return [c for c in (10, 12, 14, 16) if nv2_max <= c or c == 16][0]
    if solver == "g64_2":
        return [c for c in (18, 20, 22, 24) if nv2_max <= c or c == 24][0]
    c_hi = (nv2_max + 1) // 2                      # <32,2,5>: two lanes per row
    return ("lpr2", [c for c in (10, 12, 14, 16) if c_hi <= c or c == 16][0])


# ---- the elimination-tree kernel's tile layout (plan: tree_plan_emul.Plan) ----
def to_tiles(plan, M):
    """A dense symmetric matrix in the plan's (padded) matrix order -> [n_tiles, 16, 16]: tile t holds rows of block rowsof[t] and
    columns of the block J with colptr[J] <= t < colptr[J + 1]; of a diagonal tile the lower triangle, as the sweep stores it.  Raises
    when M has an entry outside the plan's tiles."""
    M = np.asarray(M, np.float64)
    tiles = np.zeros((plan.n_tiles, 16, 16))
    for J in range(plan.NB):
        for t in range(plan.colptr[J], plan.colptr[J + 1]):
            I = int(plan.rowsof[t])
            blk = M[16 * I:16 * I + 16, 16 * J:16 * J + 16]
            tiles[t] = np.tril(blk) if I == J else blk
    if not np.array_equal(from_tiles(plan, tiles), M):
        raise ValueError("the matrix is not symmetric with the plan's block sparsity")
    return tiles


def from_tiles(plan, tiles):
    """The inverse of to_tiles: the dense symmetric matrix of [n_tiles, 16, 16] tiles."""
    L = np.zeros((plan.n_pad, plan.n_pad))
    for J in range(plan.NB):
        for t in range(plan.colptr[J], plan.colptr[J + 1]):
            I = int(plan.rowsof[t])
            L[16 * I:16 * I + 16, 16 * J:16 * J + 16] = tiles[t]
    return L + np.tril(L, -1).T


def real_rows(plan):
    """Mask over the n_pad matrix rows: True at the two rows of every node position that holds a node (the rest is padding)."""
    return np.repeat(plan.ipos != 0xFFFFFFFF, 2)


def solve_ref(M, g):
    """solve_ld up to 200 rows, solve_refined above."""
    return solve_ld(M, g) if M.shape[0] <= 200 else solve_refined(M, g)


def emulate_tree(plan, A, damp, g):
    """The plan executed in float64 on the CPU (tree_plan_emul: the kernel's algorithm, plain numpy): y of (A + D) y = g, n_pad long."""
    tiles = to_tiles(plan, damped(A, damp, "tree"))
    ft, w, inv = plan.factor(tiles, np.asarray(g, np.float64))
    return plan.back_substitute(ft, w, inv)
