"""Extended-precision restatement of what lfr_batch_hessian_product returns (include/lfr.h): per component, at given positions, H v
over the coordinates of its variable nodes and the curvature v . H v, for the exact Hessian of evaluate_ref's objective and for its
loss-corrected Gauss-Newton matrix, with and without the free set, and the first-order error units the tolerances of
tests/test_gpu_hessian_product.py are multiples of.  numpy np.longdouble written from the formulas and applied edge block by edge
block - nothing dense, so a component of any size costs its edges.  Not a test: tests/test_hessian_product_ref.py pins it against the
dense matrices of backward_ref / backward_gn_ref and measures the GAMMA_*_CPU constants below.

Per edge e = (src -> dst), with r, rho', rho'' and P = I + df/dx_src of evaluate_ref (the interpolant's first derivative zeroed outside
[-0.5, 0.5] and kept at exactly +-0.5, its second derivative with it):
  M = w (rho' I + 2 rho'' r r^T)   (Gauss-Newton: w rho' I),   S = w rho' sum_k r_k d2f_k   (Gauss-Newton: 0)
  u = v_dst - P v_src,   t = M u,   (H v)_dst += t,   (H v)_src += -P^T t - S v_src
Free set: a coordinate with |x| >= 1 reads as v = 0 in every edge and gets (H v)_i = v_i.

Error units, first order, every quantity with the unit evaluate_ref gives it (M_{e,k}: the magnitude behind the residual's unit):
  dr_k = 2^-53 M_{e,k}                                  residual
  drho' = 2^-53 (rho' + 2 |rho''| sum_k |r_k| M_{e,k})      weight (evaluate_ref's w_unit)
  drho'' = 2^-53 (|rho''| + 2 |rho'''| sum_k |r_k| M_{e,k})   the same one derivative up: rho''' = 2 rho'^3 / b^2 (Cauchy), 6 k / a^6 (Tukey)
  dP = 2^-53 (D + I)                                    D the absolute-value sum of the interpolant's derivative terms
  dM = |w| (drho' I + 2 drho'' |r||r|^T + 2 |rho''| (dr |r|^T + |r| dr^T)) + 2^-53 |M|,   |M| = |w| (rho' I + 2 |rho''| |r||r|^T)
  dS = |w| drho' sum_k |r_k| |d2f_k| + |w| rho' sum_k (dr_k |d2f_k| + 2^-53 |r_k| D2_k) + 2^-53 |S|     (D2 as D, second derivatives)
  |u| = |v_dst| + |P| |v_src|,   du = 2^-53 |u| + dP |v_src|
  destination rows: dt = dM |u| + |M| du
  source rows:      |P|^T dt + (dP^T + 2^-53 |P|^T) |M| |u| + (dS + 2^-53 |S|) |v_src|
  coordinate i:     the sum of those over its edges + 2^-53 n_i |(H v)_i|, n_i the number of incident edges
  curvature:        sum_i |v_i| unit_i + 2^-53 2 nv sum_i |v_i (H v)_i|    (a sum of 2 nv terms in any order)
"""
import dataclasses

import numpy as np

import cost_ref as CR
import evaluate_ref as ER

LD = CR.LD
U = CR.U

# The largest |fp64 evaluator - longdouble| / unit over every component of class_limit_cases.all_shapes(), cost_ref.TUKEY_GRAPH (both
# Tukey variants) and cost_ref.BOUNDS_GRAPH at the two position sets (the oracle's, evaluate_ref.positions_b), both matrices, with and
# without the free set, for the vectors of vectors() below.  The evaluators: product() run in numpy float64 and the dense matrices of
# backward_ref.Component.hessian / backward_gn_ref times the vector.  Rounded up to two digits; tests/test_hessian_product_ref.py
# prints the measurements and fails if one exceeds its constant or falls below half of it.  Measured 0.5207 (product: the dense matrix
# on cost_ref.BOUNDS_GRAPH; the float64 restatement 0.3872) and 0.2957 (curvature: the dense matrix on cost_ref.TUKEY_GRAPH).
GAMMA_HVP_CPU = 0.53
GAMMA_CURV_CPU = 0.30
# The round trip of tests/test_gpu_hessian_product.py on the CPU: xdot from a numpy solve of the reduced matrix against jvp_ref.rhs,
# then product(xdot, free set) in float64 against that right-hand side; the largest |H xdot - b|_2 / |b|_2 over the components of
# class_limit_cases.all_shapes() at the oracle's positions, both matrices.  Same rule: rounded up, checked by the same test.
# Measured 2.627e-15 (exact), 1.050e-15 (Gauss-Newton).
ROUND_TRIP_REL_CPU = 2.7e-15
GPU_FACTOR = ER.GPU_FACTOR

SEED_V = 9200


@dataclasses.dataclass
class Hvp:
    hv: np.ndarray           # [nv, 2]
    curvature: object        # scalar
    hv_unit: np.ndarray      # [nv, 2]
    curv_unit: object
    n_bound: int             # coordinates treated as bound (0 without the free set)


def _d2basis(x, dtype):
    h = dtype(0.5)
    inside = ((x >= -h) & (x <= h)).astype(dtype)
    return np.stack([4 * inside, -8 * inside, 4 * inside], -1)


def _mv(A, x):
    return np.einsum("eij,ej->ei", A, x)


def _mtv(A, x):
    return np.einsum("eji,ej->ei", A, x)


def product(ed, x, v, variant="ceres1", gauss_newton=False, free_set=False, dtype=LD):
    """Hvp of the component at x ([nv, 2] or flat) for one vector v (same shape).  dtype=np.float64: the same formulas in fp64 (an fp64
    evaluator for the measured constants; its units are not meant to be used)"""
    assert variant in ("ceres1", "ceres2")
    x = np.asarray(x).astype(dtype).reshape(-1, 2)
    v = np.asarray(v).astype(dtype).reshape(-1, 2)
    assert len(x) == ed.nv == len(v)
    bound = (np.abs(x) >= 1) if free_set else np.zeros(x.shape, bool)
    vm = np.where(bound, dtype(0), v)
    zero = np.zeros((1, 2), dtype)
    xe, ve = np.concatenate([x, zero]), np.concatenate([vm, zero])                # index -1: the constant node
    xs, xd, vs, vd = xe[ed.src], xe[ed.dst], ve[ed.src], ve[ed.dst]
    flow, w = ed.flow.astype(dtype), ed.w.astype(dtype)
    lr, lc = ER._basis(xs[:, 0], dtype), ER._basis(xs[:, 1], dtype)
    dlr, dlc = ER._dbasis(xs[:, 0], dtype), ER._dbasis(xs[:, 1], dtype)
    d2lr, d2lc = _d2basis(xs[:, 0], dtype), _d2basis(xs[:, 1], dtype)

    def terms(a, b):
        return (a[:, :, None] * b[:, None, :]).reshape(-1, 9)[:, :, None] * flow      # [E, 9, 2]

    bf, brf, bcf = terms(lr, lc), terms(dlr, lc), terms(lr, dlc)
    brr, brc, bcc = terms(d2lr, lc), terms(dlr, dlc), terms(lr, d2lc)
    r = xd - xs - bf.sum(1)
    s = (r * r).sum(1)
    a2, cb = CR.TUKEY_A2.astype(dtype), CR.CAUCHY_B.astype(dtype)
    k = a2 / (6 if variant == "ceres1" else 3)
    inside = s <= a2
    tv = 1 - np.minimum(s, a2) / a2
    intra = ed.kind == CR.KIND_INTRA
    inv = 1 / (1 + s / cb)
    rho1 = np.where(intra, inv, 3 * k / a2 * tv * tv)
    rho2 = np.where(intra, -inv * inv / cb, np.where(inside, -6 * k / (a2 * a2) * tv, 0))
    rho3 = np.where(intra, 2 * inv * inv * inv / (cb * cb), np.where(inside, 6 * k / (a2 * a2 * a2), 0))
    eye = np.eye(2, dtype=dtype)[None]
    P = np.stack([brf.sum(1), bcf.sum(1)], -1) + eye                              # [E, k, i]
    rr = r[:, :, None] * r[:, None, :]
    c = w * rho1
    if gauss_newton:
        M = c[:, None, None] * eye
        S = np.zeros((len(s), 2, 2), dtype)
    else:
        M = w[:, None, None] * (rho1[:, None, None] * eye + 2 * rho2[:, None, None] * rr)
        d2 = np.stack([np.stack([brr.sum(1), brc.sum(1)], -1), np.stack([brc.sum(1), bcc.sum(1)], -1)], -1)      # [E, k, i, j]
        S = c[:, None, None] * np.einsum("ek,ekij->eij", r, d2)
    u = vd - _mv(P, vs)
    t = _mv(M, u)
    hs = -_mtv(P, t) - _mv(S, vs)
    hv = np.zeros((ed.nv + 1, 2), dtype)
    np.add.at(hv, ed.dst, t)
    np.add.at(hv, ed.src, hs)
    hv = np.where(bound, v, hv[:ed.nv])
    curvature = (v * hv).sum()
    # units
    aw, ar = np.abs(w), np.abs(r)
    mag = np.abs(xd) + np.abs(xs) + np.abs(bf).sum(1)                             # M_{e,k}
    dr = U * mag
    rm = (ar * mag).sum(1)
    drho1 = U * (rho1 + 2 * np.abs(rho2) * rm)
    drho2 = U * (np.abs(rho2) + 2 * np.abs(rho3) * rm)
    D = np.stack([np.abs(brf).sum(1), np.abs(bcf).sum(1)], -1)
    dP = U * (D + eye)
    aP = np.abs(P)
    arr = ar[:, :, None] * ar[:, None, :]
    if gauss_newton:
        aM = (aw * rho1)[:, None, None] * eye
        dM = (aw * drho1)[:, None, None] * eye + U * aM
        aS = dS = np.zeros((len(s), 2, 2), dtype)
    else:
        aM = aw[:, None, None] * (rho1[:, None, None] * eye + 2 * np.abs(rho2)[:, None, None] * arr)
        drr = dr[:, :, None] * ar[:, None, :] + ar[:, :, None] * dr[:, None, :]
        dM = aw[:, None, None] * (drho1[:, None, None] * eye + 2 * drho2[:, None, None] * arr + 2 * np.abs(rho2)[:, None, None] * drr) + U * aM
        ad2 = np.abs(d2)
        D2 = np.stack([np.stack([np.abs(brr).sum(1), np.abs(brc).sum(1)], -1), np.stack([np.abs(brc).sum(1), np.abs(bcc).sum(1)], -1)], -1)
        aS = (aw * rho1)[:, None, None] * np.einsum("ek,ekij->eij", ar, ad2)
        dS = ((aw * drho1)[:, None, None] * np.einsum("ek,ekij->eij", ar, ad2)
              + (aw * rho1)[:, None, None] * (np.einsum("ek,ekij->eij", dr, ad2) + U * np.einsum("ek,ekij->eij", ar, D2)) + U * aS)
    avs, avd = np.abs(vs), np.abs(vd)
    au = avd + _mv(aP, avs)
    du = U * au + _mv(dP, avs)
    dt = _mv(dM, au) + _mv(aM, du)
    at = _mv(aM, au)
    dhs = _mtv(aP, dt) + _mtv(dP, at) + U * _mtv(aP, at) + _mv(dS, avs) + U * _mv(aS, avs)
    A = np.zeros((ed.nv + 1, 2), dtype)
    np.add.at(A, ed.dst, dt)
    np.add.at(A, ed.src, dhs)
    n_inc = np.zeros(ed.nv + 1, np.int64)
    np.add.at(n_inc, ed.dst, 1)
    np.add.at(n_inc, ed.src, 1)
    hv_unit = np.where(bound, dtype(0), A[:ed.nv] + U * n_inc[:ed.nv, None] * np.abs(hv))
    curv_unit = (np.abs(v) * hv_unit).sum() + U * (2 * ed.nv) * np.abs(v * hv).sum()
    return Hvp(hv, curvature, hv_unit, curv_unit, int(bound.sum()))


def vectors(n_nodes, k=4, seed=SEED_V):
    """the k vectors the tests multiply with, for every node of a graph: standard normal from a fixed seed"""
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((k, n_nodes, 2))


def at_positions(comps, positions, v, variant="ceres1", **kw):
    """{component id: Hvp} of {id: (variable nodes, Edges)} at positions [n_nodes, 2] for the vector v [n_nodes, 2] of the whole graph"""
    return {c: product(ed, positions[var_nodes], v[var_nodes], variant, **kw) for c, (var_nodes, ed) in comps.items()}
