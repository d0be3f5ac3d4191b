"""Restatement in numpy of what lfr_batch_hessian_solve returns (include/lfr.h): per component (H + damping I) y = b by block-Jacobi
preconditioned conjugate gradients on hessian_product_ref.product, with the call's stop, negative-curvature and non-finite rules.
dtype=np.longdouble is the reference, dtype=np.float64 the restatement of the kernels' arithmetic (same algorithm, numpy's summation
orders).  Not a test: tests/test_hessian_solve_ref.py pins it against dense solves and measures the constants below.

The algorithm, over the component's variable coordinates that are not bound (a bound coordinate: y_i = b_i, out of every row and norm):
  y = 0, r = b, z = B^-1 r, p = z                      B: per node its 2x2 diagonal block of A, the identity where that block is not
  per step:  q = A p;  p.q not finite -> status 3;  p.q <= 0 -> status 2 (y stays)       finite or has a00 <= 0 or det <= 0
             alpha = r.z / p.q;  y += alpha p;  r -= alpha q;  |r|^2 not finite -> status 3
             |r|_2 <= rel_tolerance |b|_2 -> status 0;  z = B^-1 r;  p = z + (r.z / previous r.z) p
  status 1 after max_iterations steps;  b = 0: status 0 at once;  b or a record not finite: status 3 at once
"""
import dataclasses

import numpy as np

import cost_ref as CR
import hessian_product_ref as HR

LD = CR.LD
OK, MAX_ITERATIONS, NEGATIVE_CURVATURE, NONFINITE = 0, 1, 2, 3

# Measured by tests/test_hessian_solve_ref.py (it prints the measurements and fails if one exceeds its constant or falls below half of
# it), float64 restatement, rel_tolerance 1e-10, on the components of test_evaluate_ref.inputs():
# the largest true |b - A y|_2 / (rel_tolerance |b|_2) at status 0, the residual evaluated in longdouble: measured 0.9766 over 2607
# solves (the recurrence's residual passes its test at <= 1 and the true residual follows it closely), rounded up to two digits;
TRUE_RESIDUAL_OVER_TOL_CPU = 0.98
# the largest iterations / rows at status 0: measured 1.2577, rounded up to two digits
ITERATIONS_OVER_ROWS_CPU = 1.3
GPU_FACTOR = HR.GPU_FACTOR
# the ring of 6146 rows (class_limit_cases' ring of 3074 nodes), Gauss-Newton, damping 0, at the solve's positions: the float64
# restatement converges in 418 steps, far below half of 4 x rows = 12292, so the GPU test runs it undamped
RING_DAMPING = 0.0
# |GPU iterations - float64 restatement's| allowed per component.  Measured on an MI355X by tests/test_gpu_hessian_solve.py's
# class-limit cases (33 components, 8 to 244 steps, one right-hand side): 0 (Gauss-Newton and exact at the solve's positions) and 1
# (Gauss-Newton at positions_b) - the two run the same recurrence with different summation orders, so a residual that lands within
# rounding of the threshold stops one step apart.  Twice the measurement.
ITERATION_SPREAD_GPU = 2

SEED_B = 9400


@dataclasses.dataclass
class Solve:
    y: np.ndarray            # [nv, 2]
    status: int
    iterations: int
    residual: object         # |r|_2 / |b|_2 of the recurrence
    n_bound: int


def node_blocks(ed, x, variant="ceres1", gauss_newton=False, dtype=LD):
    """[nv, 2, 2]: every variable node's diagonal block of H.  Each edge gets private copies of its two nodes, so that four products
    with unit vectors on the copies read the edge's own two diagonal blocks; they are added to the nodes in record order."""
    x = np.asarray(x).astype(dtype).reshape(-1, 2)
    E = len(ed.src)
    e = np.arange(E)
    src = np.where(ed.src >= 0, 2 * e, -1)
    dst = np.where(ed.dst >= 0, 2 * e + 1, -1)
    xe = np.concatenate([x, np.zeros((1, 2), dtype)])
    xx = np.zeros((2 * E, 2), dtype)
    xx[0::2], xx[1::2] = xe[ed.src], xe[ed.dst]
    ex = CR.Edges(2 * E, src, dst, ed.w, ed.kind, ed.flow, ed.eids)
    blocks = np.zeros((ed.nv + 1, 2, 2), dtype)
    for side, idx in ((0, ed.src), (1, ed.dst)):
        for c in range(2):
            v = np.zeros((2 * E, 2), dtype)
            v[side::2, c] = 1
            col = HR.product(ex, xx, v, variant, gauss_newton, False, dtype).hv[side::2]        # column c of every edge's block
            np.add.at(blocks[:, :, c], idx, col)
    return blocks[:ed.nv]


def _inverse_blocks(blocks, bound, damping, dtype):
    a00 = np.where(bound[:, 0], dtype(1), blocks[:, 0, 0] + damping)
    a11 = np.where(bound[:, 1], dtype(1), blocks[:, 1, 1] + damping)
    a01 = np.where(bound.any(1), dtype(0), blocks[:, 1, 0])
    with np.errstate(all="ignore"):
        det = a00 * a11 - a01 * a01
        ok = np.isfinite(a00) & np.isfinite(a01) & np.isfinite(a11) & np.isfinite(det) & (a00 > 0) & (det > 0)
        d = np.where(ok, det, dtype(1))
        return np.where(ok, a11 / d, dtype(1)), np.where(ok, -a01 / d, dtype(0)), np.where(ok, a00 / d, dtype(1))


def solve(ed, x, b, variant="ceres1", gauss_newton=False, free_set=False, damping=0.0, rel_tolerance=1e-10, max_iterations=None,
          dtype=LD):
    x = np.asarray(x).astype(dtype).reshape(-1, 2)
    b = np.asarray(b).astype(dtype).reshape(-1, 2)
    assert len(x) == ed.nv == len(b)
    damping, tol = dtype(damping), dtype(rel_tolerance)
    if max_iterations is None:
        max_iterations = 8 * ed.nv
    bound = (np.abs(x) >= 1) if free_set else np.zeros(x.shape, bool)
    zero = dtype(0)

    def A(p):
        hv = HR.product(ed, x, p, variant, gauss_newton, free_set, dtype).hv
        return np.where(bound, zero, hv + damping * p)

    with np.errstate(all="ignore"):
        i00, i01, i11 = _inverse_blocks(node_blocks(ed, x, variant, gauss_newton, dtype), bound, damping, dtype)

        def precond(r):
            return np.stack([i00 * r[:, 0] + i01 * r[:, 1], i01 * r[:, 0] + i11 * r[:, 1]], -1)

        y = np.zeros_like(b)
        r = np.where(bound, zero, b)
        bb = rr = (r * r).sum()
        done = lambda status, it: Solve(np.where(bound, b, y), status, it, (np.sqrt(rr) / np.sqrt(bb)) if bb != 0 else zero, int(bound.sum()))
        records_finite = np.isfinite(HR.product(ed, x, np.zeros_like(x), variant, gauss_newton, False, dtype).hv).all()
        if not np.isfinite(bb) or not records_finite:
            return done(NONFINITE, 0)
        if bb == 0:
            return done(OK, 0)
        z = precond(r)
        rz = (r * z).sum()
        p = z
        for it in range(max_iterations):
            q = A(p)
            pq = (p * q).sum()
            if not np.isfinite(pq):
                return done(NONFINITE, it)
            if pq <= 0:
                return done(NEGATIVE_CURVATURE, it)
            alpha = rz / pq
            y = y + alpha * p
            r = r - alpha * q
            rr = (r * r).sum()
            if not np.isfinite(rr):
                return done(NONFINITE, it + 1)
            if np.sqrt(rr) <= tol * np.sqrt(bb):
                return done(OK, it + 1)
            z = precond(r)
            rz_new = (r * z).sum()
            p = z + (rz_new / rz) * p
            rz = rz_new
        return done(MAX_ITERATIONS, max_iterations)


def true_residual(ed, x, b, y, variant="ceres1", gauss_newton=False, free_set=False, damping=0.0):
    """|b - A y|_2 and |b|_2 over the free coordinates, in longdouble, for any y ([nv, 2])"""
    x = np.asarray(x).astype(LD).reshape(-1, 2)
    b, y = np.asarray(b).astype(LD).reshape(-1, 2), np.asarray(y).astype(LD).reshape(-1, 2)
    bound = (np.abs(x) >= 1) if free_set else np.zeros(x.shape, bool)
    ay = HR.product(ed, x, y, variant, gauss_newton, free_set).hv + LD(damping) * y
    res = np.where(bound, LD(0), b - ay)
    return np.sqrt((res * res).sum()), np.sqrt((np.where(bound, LD(0), b) ** 2).sum())


def rhs(n_nodes, k=4, seed=SEED_B):
    """the k right-hand sides the tests solve against, for every node of a graph: standard normal from a fixed seed"""
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((k, n_nodes, 2))
