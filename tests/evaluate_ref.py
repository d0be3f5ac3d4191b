"""Extended-precision restatement of what lfr_batch_evaluate returns (include/lfr.h): per component, at given positions, the gradient
dF/dx per variable coordinate, the raw residual and rho' per edge, and the first-order error units the tolerances of
tests/test_gpu_evaluate.py are multiples of.  numpy np.longdouble written from the formulas, as tests/cost_ref.py is (which supplies
Edges, components, the basis, the constants and the cost with ITS unit, Cost.tol).  Not a test: tests/test_evaluate_ref.py pins it
and measures the GAMMA_*_CPU constants below.

  r_e = x_dst - x_src - f(x_src; phi_e),  s_e = |r_e|^2,  F_c = sum_e 1/2 w_e rho_e(s_e)
  dF/dx_dst += w rho' r,   dF/dx_src += -w rho' P^T r,   P = I + df/dx_src
the derivative of the interpolant zeroed outside [-0.5, 0.5] and kept at exactly +-0.5 (cost.cc:38-43).

Error units (M_{e,k} = |x_dst,k| + |x_src,k| + sum_j |b_j phi_{j,k}|, the magnitude cost_ref.evaluate uses):
  residual r_{e,k}        2^-53 M_{e,k}
  weight rho'_e           2^-53 (rho'_e + 2 |rho''_e| sum_k |r_{e,k}| M_{e,k})     (the second term: the cancellation in Tukey's 1 - s / a^2
                                                                                    and the residual's own rounding)
  gradient coordinate i   2^-53 (A_i + n_i |g_i|), n_i the number of incident edges,
                          A_i = sum over the edges at i of |w_e| (rho'_e + 2 |rho''_e| s_e) sum_k |P_e|_{k,i} M_{e,k}, on the source side
                          plus |w_e| rho'_e sum_k |r_{e,k}| D_{e,k,i} (D the absolute-value sum of the interpolant's derivative terms);
                          on the destination side |P| = I.
"""
import dataclasses

import numpy as np

import cost_ref as CR

LD = CR.LD
U = CR.U

# The largest |fp64 evaluator - longdouble| / unit over every component of class_limit_cases.all_shapes(), cost_ref.TUKEY_GRAPH (both
# Tukey variants) and cost_ref.BOUNDS_GRAPH at the two position sets of tests/test_gpu_evaluate.py - (a) a solve's positions (the
# oracle's here), (b) positions_b() below.  The evaluators: this module's evaluate() run in numpy float64 (residuals, weights,
# gradient) and torch autograd of backward_ref.Component.cost (gradient).  Rounded up to two digits; tests/test_evaluate_ref.py prints
# the measurements and fails if one exceeds its constant or falls below half of it.  Measured 1.1497 (gradient), 3.3939 (residual: the
# nine products of the interpolant summed one after the other) and 1.9774 (weight).
GAMMA_GRAD_CPU = 1.2
GAMMA_RES_CPU = 3.4
GAMMA_W_CPU = 2.0
# the kernels contract to FMA, sum the interpolant separably and the gradient in another order: cost_ref.GAMMA_GPU's factor and reason
GPU_FACTOR = 8

SEED_B = 9100


@dataclasses.dataclass
class Eval:
    cost: CR.Cost
    r: np.ndarray            # [E, 2] raw residuals
    rho1: np.ndarray         # [E] rho'(s)
    grad: np.ndarray         # [nv, 2] dF/dx
    r_unit: np.ndarray       # [E, 2]
    w_unit: np.ndarray       # [E]
    g_unit: np.ndarray       # [nv, 2]


def _dbasis(x, dtype):
    """d basis / d x [n, 3]: zero outside [-0.5, 0.5], kept at exactly +-0.5"""
    h = dtype(0.5)
    t = np.clip(x, -h, h)
    inside = ((x >= -h) & (x <= h)).astype(dtype)
    return np.stack([4 * t - 1, -8 * t, 4 * t + 1], -1) * inside[:, None]


def _basis(x, dtype):
    if dtype is LD:
        return CR._basis(x)
    h = dtype(0.5)
    t = np.clip(x, -h, h)
    return np.stack([2 * t * (t - h), -4 * (t - h) * (t + h), 2 * t * (t + h)], -1)


def evaluate(ed, x, variant="ceres1", dtype=LD):
    """Eval of the component at x ([nv, 2] or flat).  dtype=np.float64: the same formulas in fp64 (an fp64 evaluator for the measured
    constants; its units are not meant to be used)"""
    assert variant in ("ceres1", "ceres2")
    x = np.asarray(x).astype(dtype).reshape(-1, 2)
    assert len(x) == ed.nv
    xe = np.concatenate([x, np.zeros((1, 2), dtype)])                            # index -1: the constant node
    xs, xd = xe[ed.src], xe[ed.dst]
    flow, w = ed.flow.astype(dtype), ed.w.astype(dtype)
    lr, lc, dlr, dlc = _basis(xs[:, 0], dtype), _basis(xs[:, 1], dtype), _dbasis(xs[:, 0], dtype), _dbasis(xs[:, 1], dtype)
    b = (lr[:, :, None] * lc[:, None, :]).reshape(-1, 9)
    br = (dlr[:, :, None] * lc[:, None, :]).reshape(-1, 9)
    bc = (lr[:, :, None] * dlc[:, None, :]).reshape(-1, 9)
    bf, brf, bcf = b[:, :, None] * flow, br[:, :, None] * flow, bc[:, :, None] * flow          # [E, 9, 2]
    r = xd - xs - bf.sum(1)
    s = (r * r).sum(1)
    a2, cb = CR.TUKEY_A2.astype(dtype), CR.CAUCHY_B.astype(dtype)
    k = a2 / (6 if variant == "ceres1" else 3)
    inside = s <= a2
    v = 1 - np.minimum(s, a2) / a2
    intra = ed.kind == CR.KIND_INTRA
    inv = 1 / (1 + s / cb)
    rho1 = np.where(intra, inv, 3 * k / a2 * v * v)
    rho2 = np.where(intra, -inv * inv / cb, np.where(inside, -6 * k / (a2 * a2) * v, 0))
    # P[e, k, i] = d r_k / d x_src,i negated: I + df_k / dx_i
    P = np.stack([brf.sum(1), bcf.sum(1)], -1)                                   # [E, k, i]
    P = P + np.eye(2, dtype=dtype)[None]
    c = w * rho1
    gd = c[:, None] * r
    gs = -c[:, None] * np.einsum("eki,ek->ei", P, r)
    g = np.zeros((ed.nv + 1, 2), dtype)
    np.add.at(g, ed.dst, gd)
    np.add.at(g, ed.src, gs)
    # units
    mag = np.abs(xd) + np.abs(xs) + np.abs(bf).sum(1)                            # M [E, 2]
    r_unit = U * mag
    w_unit = U * (rho1 + 2 * np.abs(rho2) * (np.abs(r) * mag).sum(1))
    lossf = np.abs(w) * (rho1 + 2 * np.abs(rho2) * s)
    D = np.stack([np.abs(brf).sum(1), np.abs(bcf).sum(1)], -1)                   # [E, k, i]
    a_src = lossf[:, None] * np.einsum("eki,ek->ei", np.abs(P), mag) + (np.abs(w) * rho1)[:, None] * np.einsum("eki,ek->ei", D, np.abs(r))
    a_dst = lossf[:, None] * mag
    A = np.zeros((ed.nv + 1, 2), dtype)
    np.add.at(A, ed.dst, a_dst)
    np.add.at(A, ed.src, a_src)
    n_inc = np.zeros(ed.nv + 1, np.int64)
    np.add.at(n_inc, ed.dst, 1)
    np.add.at(n_inc, ed.src, 1)
    g_unit = U * (A + n_inc[:, None] * np.abs(g))
    return Eval(CR.evaluate(ed, x, variant), r, rho1, g[:ed.nv], r_unit, w_unit, g_unit[:ed.nv])


def positions_b(comps, n_nodes, seed=SEED_B):
    """position set (b) of tests/test_gpu_evaluate.py: uniform in [-1.2, 1.2] from a fixed seed for every node of the graph, the first
    variable node of every component at exactly (0.5, -0.5) and the second, where there is one, at (0, 0.75): clamped, kink and
    interior arguments in every class.  comps: {component: (variable nodes, Edges)}"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = rng.uniform(-1.2, 1.2, size=(n_nodes, 2))
    for c in sorted(comps):
        var_nodes = comps[c][0]
        pos[var_nodes[0]] = (0.5, -0.5)
        if len(var_nodes) > 1:
            pos[var_nodes[1]] = (0.0, 0.75)
    return pos


def at_positions(comps, positions, variant="ceres1"):
    """{component id: Eval} of {id: (variable nodes, Edges)} at positions [n_nodes, 2] of the whole graph"""
    return {c: evaluate(ed, positions[var_nodes], variant) for c, (var_nodes, ed) in comps.items()}


def match_layout(comps, evals, n_matches, dtype=np.float64):
    """(residuals [n_matches, 2, 2], weights [n_matches, 2], their units) in lfr_batch_evaluate's match layout: directed edge 2 m is
    node1 -> node2 of match m; directions that are no residual block read residual 0, weight -1 (unit 0)"""
    res, wts = np.zeros((2 * n_matches, 2), dtype), np.full(2 * n_matches, -1.0, dtype)
    res_u, wts_u = np.zeros((2 * n_matches, 2)), np.zeros(2 * n_matches)
    for c, (_, ed) in comps.items():
        ev = evals[c]
        assert (wts[ed.eids] == -1.0).all()
        res[ed.eids], wts[ed.eids] = ev.r.astype(dtype), ev.rho1.astype(dtype)
        res_u[ed.eids], wts_u[ed.eids] = ev.r_unit.astype(np.float64), ev.w_unit.astype(np.float64)
    return res.reshape(-1, 2, 2), wts.reshape(-1, 2), res_u.reshape(-1, 2, 2), wts_u.reshape(-1, 2)
