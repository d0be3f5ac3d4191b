"""Extended-precision restatement of what lfr_batch_evaluate_vjp returns (include/lfr.h): per component, at given positions and for given
bars of the cost (cbar, one per component), the raw residuals (rbar, two per edge) and the weights (wbar, one per edge), the gradient
of  cbar F + sum_e rbar_e . r_e + sum_e wbar_e rho'_e  with respect to the positions, the flows and the similarities, and the
first-order error units the tolerances of tests/test_gpu_evaluate_vjp.py are multiples of.  numpy np.longdouble written from the
formulas, on top of cost_ref.Edges and the quantities of evaluate_ref.evaluate (r, rho', rho'', P, the units of r and rho').  Not a
test: tests/test_evaluate_vjp_ref.py pins it to torch autograd and measures the GAMMA_*_CPU constants below.

  q_e = c_e r_e + rbar_e,   c_e = cbar w_e rho'_e + wbar_e 2 rho''_e          (the bar of the raw residual)
  dL/dx_dst += q_e,   dL/dx_src += -P_e^T q_e,   dL/dphi_e[3 i + j, k] = -Lr_i Lc_j q_k,   dL/dw_e = cbar 1/2 rho_e(s_e)

Error units (M_{e,k}, r_unit and w_unit: evaluate_ref's; rho''' = d rho'' / d s):
  rho''_e                 2^-53 (|rho''| + 2 |rho'''| sum_k |r_k| M_k)
  c_e                     |cbar w| w_unit + 2 |wbar| unit(rho'') + 2^-53 (|cbar w rho'| + 2 |wbar rho''|)
  q_{e,k}                 unit(c) |r_k| + |c| r_unit_k + 2^-53 (|c r_k| + |rbar_k|)
  flow gradient           |b_ij| (2^-53 |q_k| + unit(q_k)),  b_ij = Lr_i Lc_j
  position coordinate i   the sum over the edges at i of unit(q_i) on the destination side and of sum_k (|P_ki| unit(q_k) + 2^-53 |q_k|
                          (|P_ki| + D_ki)) on the source side (D the absolute-value sum of the interpolant's derivative terms), plus
                          2^-53 n_i |g_i| for the n_i additions: evaluate_ref's g_unit with q in the place of w rho' r
  similarity, direction   2^-53 |cbar| (1/2 rho + rho' |r| sum_k M_k), cost_ref.Cost's scale of one term without its weight, plus on
                          intra-track edges 2^-53 |cbar| b / 2: forming 1 + s / b in fp64 errs by up to 2^-53 however small s is and
                          moves rho by b times that (cost_ref, "What S_c leaves out" - a per-edge output cannot restrict its inputs)
  similarity, match       the two directions' units plus 2^-53 times the sum's magnitude
"""
import dataclasses

import numpy as np

import cost_ref as CR
import evaluate_ref as ER

LD = CR.LD
U = CR.U

# The largest |fp64 evaluator - longdouble| / unit over every component of class_limit_cases.all_shapes(), cost_ref.TUKEY_GRAPH (both
# Tukey variants) and cost_ref.BOUNDS_GRAPH at the two position sets of tests/test_gpu_evaluate_vjp.py and its three bar sets (BAR_SETS).
# The evaluators: vjp() below run in numpy float64 and torch float64 autograd of backward_ref's cost and of the residuals and weights
# restated in torch.  Rounded up to two digits; tests/test_evaluate_vjp_ref.py prints the measurements and fails if one exceeds its
# constant or falls below half of it.  Measured 1.0063 (positions), 2.6726 (flows: the two roundings of each basis value and of their
# product, which the flow unit leaves to the constant) and 1.7295 (similarities, per directed edge).
GAMMA_VJP_X_CPU = 1.1
GAMMA_VJP_FLOW_CPU = 2.7
GAMMA_VJP_SIM_CPU = 1.8
GPU_FACTOR = ER.GPU_FACTOR

SEED_BARS = 9200
BAR_SETS = ("c", "crw", "r")          # cbar alone, all three, rbar alone


def bars(n_components, n_matches, which, seed=SEED_BARS):
    """(cbar [n_components], rbar [n_matches, 2, 2], wbar [n_matches, 2]) of bar set `which`, N(0, 1) from a fixed seed; None = absent.
    The same draws whatever the set, so "crw" extends "c"."""
    assert which in BAR_SETS
    rng = np.random.Generator(np.random.PCG64(seed))
    cbar, rbar, wbar = rng.normal(size=n_components), rng.normal(size=(n_matches, 2, 2)), rng.normal(size=(n_matches, 2))
    return (cbar if "c" in which else None, rbar if "r" in which else None, wbar if "w" in which else None)


@dataclasses.dataclass
class Vjp:
    q: np.ndarray            # [E, 2]
    gx: np.ndarray           # [nv, 2]
    gflow: np.ndarray        # [E, 9, 2]
    gsim: np.ndarray         # [E] per directed edge
    nonzero_loss: np.ndarray  # [E] bool: rho' > 0 (a saturated Tukey edge passes rbar only)
    q_unit: np.ndarray
    gx_unit: np.ndarray
    gflow_unit: np.ndarray
    gsim_unit: np.ndarray


def vjp(ed, x, cbar=0.0, rbar=None, wbar=None, variant="ceres1", dtype=LD):
    """Vjp of the component at x ([nv, 2] or flat): cbar a scalar, rbar [E, 2] and wbar [E] in the order of ed's edges (None = 0).
    dtype=np.float64: the same formulas in fp64 (an fp64 evaluator for the measured constants; its units are not meant to be used)"""
    assert variant in ("ceres1", "ceres2")
    x = np.asarray(x).astype(dtype).reshape(-1, 2)
    assert len(x) == ed.nv
    E = len(ed)
    cbar = dtype(cbar)
    rbar = np.zeros((E, 2), dtype) if rbar is None else np.asarray(rbar).astype(dtype).reshape(E, 2)
    wbar = np.zeros(E, dtype) if wbar is None else np.asarray(wbar).astype(dtype).reshape(E)
    xe = np.concatenate([x, np.zeros((1, 2), dtype)])                            # index -1: the constant node
    xs, xd = xe[ed.src], xe[ed.dst]
    flow, w = ed.flow.astype(dtype), ed.w.astype(dtype)
    lr, lc = ER._basis(xs[:, 0], dtype), ER._basis(xs[:, 1], dtype)
    dlr, dlc = ER._dbasis(xs[:, 0], dtype), ER._dbasis(xs[:, 1], dtype)
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
    rho0 = np.where(intra, cb * np.log1p(s / cb), k * (1 - v * v * v))
    rho1 = np.where(intra, inv, 3 * k / a2 * v * v)
    rho2 = np.where(intra, -inv * inv / cb, np.where(inside, -6 * k / (a2 * a2) * v, 0))
    rho3 = np.where(intra, 2 * inv * inv * inv / (cb * cb), np.where(inside, 6 * k / (a2 * a2 * a2), 0))
    P = np.stack([brf.sum(1), bcf.sum(1)], -1) + np.eye(2, dtype=dtype)[None]   # [E, k, i] = I + df_k / dx_i
    c = cbar * w * rho1 + wbar * 2 * rho2
    q = c[:, None] * r + rbar
    gs = -np.einsum("eki,ek->ei", P, q)
    g = np.zeros((ed.nv + 1, 2), dtype)
    np.add.at(g, ed.dst, q)
    np.add.at(g, ed.src, gs)
    gflow = -b[:, :, None] * q[:, None, :]
    gsim = cbar * (rho0 / 2)
    # units
    mag = np.abs(xd) + np.abs(xs) + np.abs(bf).sum(1)                            # M [E, 2]
    rm = (np.abs(r) * mag).sum(1)
    r_unit = U * mag
    w_unit = U * (rho1 + 2 * np.abs(rho2) * rm)
    rho2_unit = U * (np.abs(rho2) + 2 * np.abs(rho3) * rm)
    c_unit = np.abs(cbar * w) * w_unit + 2 * np.abs(wbar) * rho2_unit + U * (np.abs(cbar * w * rho1) + 2 * np.abs(wbar * rho2))
    q_unit = c_unit[:, None] * np.abs(r) + np.abs(c)[:, None] * r_unit + U * (np.abs(c[:, None] * r) + np.abs(rbar))
    gflow_unit = np.abs(b)[:, :, None] * (U * np.abs(q) + q_unit)[:, None, :]
    D = np.stack([np.abs(brf).sum(1), np.abs(bcf).sum(1)], -1)                   # [E, k, i]
    a_src = np.einsum("eki,ek->ei", np.abs(P), q_unit) + U * np.einsum("eki,ek->ei", np.abs(P) + D, np.abs(q))
    A = np.zeros((ed.nv + 1, 2), dtype)
    np.add.at(A, ed.dst, q_unit)
    np.add.at(A, ed.src, a_src)
    n_inc = np.zeros(ed.nv + 1, np.int64)
    np.add.at(n_inc, ed.dst, 1)
    np.add.at(n_inc, ed.src, 1)
    gx_unit = A + U * n_inc[:, None] * np.abs(g)
    gsim_unit = U * np.abs(cbar) * (rho0 / 2 + rho1 * np.sqrt(s) * mag.sum(1) + np.where(intra, cb / 2, 0))
    return Vjp(q, g[:ed.nv], gflow, gsim, rho1 > 0, q_unit, gx_unit[:ed.nv], gflow_unit, gsim_unit)


def component_bars(ed, i, cbar, rbar, wbar):
    """the bars of one component (row i of component_info, edges ed) out of the match-layout arrays of bars()"""
    return (0.0 if cbar is None else cbar[i], None if rbar is None else rbar.reshape(-1, 2)[ed.eids],
            None if wbar is None else wbar.reshape(-1)[ed.eids])


def at_positions(comps, order, positions, cbar, rbar, wbar, variant="ceres1", dtype=LD):
    """{component id: Vjp} of {id: (variable nodes, Edges)} at positions [n_nodes, 2] of the whole graph; order: the component ids in
    the order of cbar (lfr_batch_component_info's); rbar, wbar in the match layout"""
    return {c: vjp(comps[c][1], positions[comps[c][0]], *component_bars(comps[c][1], i, cbar, rbar, wbar), variant=variant, dtype=dtype)
            for i, c in enumerate(order)}


def match_layout(comps, vjps, n_nodes, n_matches, dtype=np.float64):
    """the four outputs in lfr_batch_evaluate_vjp's layout and their units: positions [n_nodes, 2], disp1 / disp2 [n_matches, 18], sim
    [n_matches]; nodes that are not variable and directions that are no residual block read 0 (unit 0).  Returns (values, units),
    two dicts."""
    gx, gx_u = np.zeros((n_nodes, 2), dtype), np.zeros((n_nodes, 2))
    fl, fl_u = np.zeros((2 * n_matches, 18), dtype), np.zeros((2 * n_matches, 18))
    sd, sd_u = np.zeros(2 * n_matches, dtype), np.zeros(2 * n_matches)
    for c, (var_nodes, ed) in comps.items():
        if c not in vjps:
            continue
        v = vjps[c]
        gx[var_nodes], gx_u[var_nodes] = v.gx.astype(dtype), v.gx_unit.astype(np.float64)
        fl[ed.eids], fl_u[ed.eids] = v.gflow.reshape(-1, 18).astype(dtype), v.gflow_unit.reshape(-1, 18).astype(np.float64)
        sd[ed.eids], sd_u[ed.eids] = v.gsim.astype(dtype), v.gsim_unit.astype(np.float64)
    sim = sd[0::2] + sd[1::2]
    sim_u = sd_u[0::2] + sd_u[1::2] + float(U) * np.abs(sim).astype(np.float64)
    # directed edge 2 m is node1 -> node2: its flow is disp2[m]; 2 m + 1 is node2 -> node1: disp1[m]
    return ({"positions": gx, "disp1": fl[1::2], "disp2": fl[0::2], "sim": sim},
            {"positions": gx_u, "disp1": fl_u[1::2], "disp2": fl_u[0::2], "sim": sim_u})
