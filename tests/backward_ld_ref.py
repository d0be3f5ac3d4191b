"""Extended-precision restatement of what lfr_batch_backward and lfr_batch_jvp return (include/lfr.h): per component, at given positions,
lambda = H^-1 ubar swept into the gradients of the flows and the similarities, and xdot = H^-1 b for tangents of the flows and the
similarities, in the three Hessian modes, with the first-order error unit of every output entry - what the tolerances of
tests/test_gpu_backward_entrywise.py are multiples of.  numpy np.longdouble written from the formulas on top of cost_ref.Edges, the basis of
evaluate_ref and the edge blocks and units of hessian_product_ref (its docstring: r, rho', rho'', P, M, S and dr, drho', drho'', dP, dM,
dS).  Not a test: tests/test_backward_ld_ref.py pins it against backward_ref / backward_gn_ref / hessian_fallback_ref / jvp_ref and
measures the GAMMA_*_CPU constants below.

H, dense over the 2 nv coordinates, per edge e = (src -> dst):
  H_dd += M,   H_ds += -M P,   H_sd += -P^T M,   H_ss += P^T M P - S          (Gauss-Newton: M = w rho' I, S = 0)
then every coordinate with |x| >= 1 becomes an identity row and column (the free set of hessian_product_ref).  MODES: "exact",
"gauss_newton", "fallback" - the exact matrix where this module's Cholesky of it succeeds (status 0), else the Gauss-Newton one (status
3); a matrix the Cholesky rejects in the other two modes, or both in this one: status 2, every output zero (hessian_fallback_ref).

lambda = H^-1 ubar with ubar read as 0 on bound coordinates; the sweep, with u = lambda_dst - P lambda_src and t = M u:
  g_flow[3 i + j, k] = b_ij t_k + w rho' r_k (grad b_ij . lambda_src),   b_ij = Lr_i Lc_j, grad b_ij = (dLr_i Lc_j, Lr_i dLc_j)
  g_sim (directed edge) = -rho' (r . u);   per match the sum of its two directions
M of the SWEEP is the exact w (rho' I + 2 rho'' r r^T) and the second flow term stays in every mode: the Gauss-Newton mode replaces H
only (backward_gn_ref inherits backward_ref's autograd sweep, and the pin of tests/test_backward_ld_ref.py holds entry by entry).
jvp: with rdot_k = -sum_ij b_ij phidot_ijk, Pdot_ki = sum_ij (grad b_ij)_i phidot_ijk and qdot = wdot rho' r + M rdot
  b_dst += -qdot,   b_src += P^T qdot + w rho' Pdot^T r,   b = 0 on bound coordinates,   xdot = H^-1 b
(lfr.h's "destination's rows take -[wdot rho' r + w (rho'' sdot r + rho' rdot)]": M rdot is its second term with sdot = 2 r . rdot).

The linear algebra: H is assembled in longdouble; linsolve_ref.solve_ld (up to 64 rows) and solve_refined (above) take a float64
matrix, so they solve with round(H) and the solution is refined against the longdouble H with longdouble residuals (three rounds: each
gains 53 bits less log2 kappa).  |H^-1|, for the units only, from covariance_ref.inverse_ld / inverse_refined of round(H).

Error units, first order, one per output entry (n = 2 nv rows, |.| entrywise, the edge quantities' units hessian_product_ref's):
  rhs_unit      0 for ubar (taken exactly); for the jvp's b, per edge
                dqdot = |wdot| (drho' |r| + rho' dr) + dM |rdot| + |M| drdot + 2^-53 (|wdot rho' r| + |M| |rdot|),  drdot_k = 2^-53 sum_ij |b_ij phidot_ijk|
                destination rows dqdot; source rows |P|^T dqdot + (dP^T + 2^-53 |P|^T) |qdot| + |w| drho' |Pdot|^T |r|
                + |w| rho' (dPdot^T |r| + |Pdot|^T dr + 2^-53 2 |Pdot|^T |r|),  dPdot = 2^-53 sum_ij |(grad b_ij)_i phidot_ijk|;
                coordinate i: the sum over its edges + 2^-53 n_i |b_i|
  lam_unit      |H^-1| (hv_unit(lambda) + rhs_unit + 2^-53 n |H| |lambda|): hessian_product_ref's unit of H lambda (the assembly's
                rounding), the right-hand side's, the factorization's.  0 on bound coordinates.  The unit of xdot is this one.
  sweep, at exact lambda:  |u| = |lambda_dst| + |P| |lambda_src|,  du = 2^-53 |u| + dP |lambda_src|,  dt = dM |u| + |M| du
    flow        |b_ij| (2^-53 |t_k| + dt_k)                                                     (evaluate_vjp_ref's gflow_unit, t for q)
                + (|w| (drho' |r_k| + rho' dr_k) + 2^-53 3 |w rho' r_k|) |grad b_ij| . |lambda_src| + 2^-53 |g_flow|
    similarity  drho' |r| . |u| + rho' (dr . |u| + |r| . du) + 2^-53 2 rho' |r| . |u|
  sweep, lambda's own error dlam = lam_unit:  ddu = dlam_dst + |P| dlam_src
    flow        |b_ij| (|M| ddu)_k + |w rho' r_k| |grad b_ij| . dlam_src
    similarity  rho' |r| . ddu
  similarity per match: the two directions' units plus 2^-53 times the sum's magnitude (evaluate_vjp_ref.match_layout)
The roundings of the basis values themselves are left to the constants, as evaluate_vjp_ref leaves them.
"""
import dataclasses
import types

import numpy as np

import cost_ref as CR
import covariance_ref as CV
import evaluate_ref as ER
import hessian_product_ref as HR
import linsolve_ref as LS

LD = CR.LD
U = CR.U
EXACT, GAUSS_NEWTON, FALLBACK = "exact", "gauss_newton", "fallback"
MODES = (EXACT, GAUSS_NEWTON, FALLBACK)
OK, INDEFINITE, FELL_BACK = 0, 2, 3
MAX_DENSE_ROWS = 400
LD_SOLVE_ROWS = 64             # linsolve_ref.solve_ld / covariance_ref.inverse_ld up to here, the refined forms above

# The largest |fp64 evaluator - longdouble| / unit over the inputs of tests/test_backward_ld_ref.py: every component of
# class_limit_cases.all_shapes() at the oracle's positions in both Tukey variants and the components with a coordinate at the bound of
# lm_decision_cases' packed_24_32 and block_m, in every mode.  The evaluators: this module at dtype=np.float64 and the torch / numpy
# references backward_ref, backward_gn_ref, hessian_fallback_ref and jvp_ref.  Rounded up to two digits; the test prints the
# measurements and fails if one exceeds its constant or falls below half of it.  The modes differ by less than 2 x: one constant each.
# Measured 0.4853 (flows: backward_gn_ref on the class-limit shapes; exact mode 0.4421, the float64 restatement 0.2848), 0.4099
# (similarities per directed edge: backward_gn_ref on packed_24_32; exact mode 0.3416) and 0.1583 (lambda and xdot against lam_unit:
# lambda of the exact mode on packed_24_32; Gauss-Newton 0.1049; xdot alone 0.0817) - lam_unit carries the factorization's n |H| |lambda|,
# a worst case over elimination orders that a Cholesky of these matrices stays well inside.
GAMMA_BWD_FLOW_CPU = 0.49
GAMMA_BWD_SIM_CPU = 0.41
GAMMA_JVP_CPU = 0.16
GPU_FACTOR = ER.GPU_FACTOR


@dataclasses.dataclass
class Backward:
    status: int              # OK / INDEFINITE / FELL_BACK
    lam: np.ndarray          # [nv, 2]
    gflow: np.ndarray        # [E, 9, 2]
    gsim: np.ndarray         # [E] per directed edge
    lam_unit: np.ndarray
    gflow_unit: np.ndarray
    gsim_unit: np.ndarray
    n_bound: int


@dataclasses.dataclass
class Jvp:
    status: int
    xdot: np.ndarray         # [nv, 2]
    b: np.ndarray            # [nv, 2] the right-hand side (0 on bound coordinates)
    xdot_unit: np.ndarray
    b_unit: np.ndarray
    n_bound: int


def _mv(A, x):
    return np.einsum("eij,ej->ei", A, x)


def _mtv(A, x):
    return np.einsum("eji,ej->ei", A, x)


def edge_terms(ed, x, variant="ceres1", dtype=LD):
    """every per-edge quantity of the module's docstring at x and its unit, hessian_product_ref.product's lines: r, rho1, rho2, b [E, 9],
    gb [E, 9, 2], P [E, k, i], M / S (exact) and Mg (Gauss-Newton), dr, drho1, dP, aP, aM, dM"""
    assert variant in ("ceres1", "ceres2")
    x = np.asarray(x).astype(dtype).reshape(-1, 2)
    assert len(x) == ed.nv
    xe = np.concatenate([x, np.zeros((1, 2), dtype)])                             # index -1: the constant node
    xs, xd = xe[ed.src], xe[ed.dst]
    flow, w = ed.flow.astype(dtype), ed.w.astype(dtype)
    lr, lc = ER._basis(xs[:, 0], dtype), ER._basis(xs[:, 1], dtype)
    dlr, dlc = ER._dbasis(xs[:, 0], dtype), ER._dbasis(xs[:, 1], dtype)
    d2lr, d2lc = HR._d2basis(xs[:, 0], dtype), HR._d2basis(xs[:, 1], dtype)

    def outer(a, c):
        return (a[:, :, None] * c[:, None, :]).reshape(-1, 9)

    b = outer(lr, lc)
    gb = np.stack([outer(dlr, lc), outer(lr, dlc)], -1)                           # [E, 9, i]
    bf = b[:, :, None] * flow
    brf, bcf = gb[:, :, 0, None] * flow, gb[:, :, 1, None] * flow
    brr, brc, bcc = outer(d2lr, lc)[:, :, None] * flow, outer(dlr, dlc)[:, :, None] * flow, outer(lr, d2lc)[:, :, None] * flow
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
    c = w * rho1
    M = w[:, None, None] * (rho1[:, None, None] * eye + 2 * rho2[:, None, None] * (r[:, :, None] * r[:, None, :]))
    Mg = c[:, None, None] * eye
    d2 = np.stack([np.stack([brr.sum(1), brc.sum(1)], -1), np.stack([brc.sum(1), bcc.sum(1)], -1)], -1)          # [E, k, i, j]
    S = c[:, None, None] * np.einsum("ek,ekij->eij", r, d2)
    # units
    aw, ar = np.abs(w), np.abs(r)
    mag = np.abs(xd) + np.abs(xs) + np.abs(bf).sum(1)
    dr = U * mag
    rm = (ar * mag).sum(1)
    drho1 = U * (rho1 + 2 * np.abs(rho2) * rm)
    drho2 = U * (np.abs(rho2) + 2 * np.abs(rho3) * rm)
    dP = U * (np.stack([np.abs(brf).sum(1), np.abs(bcf).sum(1)], -1) + eye)
    arr = ar[:, :, None] * ar[:, None, :]
    aM = aw[:, None, None] * (rho1[:, None, None] * eye + 2 * np.abs(rho2)[:, None, None] * arr)
    drr = dr[:, :, None] * ar[:, None, :] + ar[:, :, None] * dr[:, None, :]
    dM = aw[:, None, None] * (drho1[:, None, None] * eye + 2 * drho2[:, None, None] * arr + 2 * np.abs(rho2)[:, None, None] * drr) + U * aM
    n_inc = np.zeros(ed.nv + 1, np.int64)
    np.add.at(n_inc, ed.dst, 1)
    np.add.at(n_inc, ed.src, 1)
    return types.SimpleNamespace(ed=ed, x=x, dtype=dtype, variant=variant, w=w, aw=aw, r=r, ar=ar, rho1=rho1, b=b, gb=gb, flow=flow, P=P,
                                 M=M, Mg=Mg, S=S, dr=dr, drho1=drho1, dP=dP, aP=np.abs(P), aM=aM, dM=dM, n_inc=n_inc[:ed.nv],
                                 bound=np.abs(x) >= 1)


def hessian(T, gauss_newton=False):
    """the reduced matrix of the module's docstring, dense [2 nv, 2 nv] in T's dtype"""
    ed, n = T.ed, 2 * T.ed.nv
    assert n <= MAX_DENSE_ROWS
    M = T.Mg if gauss_newton else T.M
    MP = np.einsum("eij,ejk->eik", M, T.P)
    blocks = np.zeros((len(ed), 4, 4), T.dtype)                                   # over (x_src, x_dst)
    blocks[:, 2:, 2:] = M
    blocks[:, 2:, :2] = -MP
    blocks[:, :2, 2:] = -np.swapaxes(MP, 1, 2)
    blocks[:, :2, :2] = np.einsum("eji,ejk->eik", T.P, MP) - (0 if gauss_newton else T.S)
    H = np.zeros((n + 2, n + 2), T.dtype)
    idx = np.stack([2 * ed.src, 2 * ed.src + 1, 2 * ed.dst, 2 * ed.dst + 1], 1)
    idx[idx < 0] += n + 2                                                         # constant node -> the two spare rows
    for p in range(4):
        for q in range(4):
            np.add.at(H, (idx[:, p], idx[:, q]), blocks[:, p, q])
    H = H[:n, :n].copy()
    fixed = T.bound.reshape(-1)
    H[fixed, :] = 0
    H[:, fixed] = 0
    H[fixed, fixed] = 1
    return H


def cholesky_succeeds(H):
    """whether the Cholesky factorization of H in its own dtype meets positive pivots only (float64: numpy's, as backward_ref)"""
    if H.dtype == np.float64:
        try:
            np.linalg.cholesky(H)
            return True
        except np.linalg.LinAlgError:
            return False
    L = H.copy()
    for k in range(len(L)):
        if not L[k, k] > 0:
            return False
        L[k, k] = np.sqrt(L[k, k])
        L[k + 1:, k] /= L[k, k]
        L[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    return True


class Component:
    """One component at x in one mode: the edge terms, the matrix the mode factors, its status and |H^-1|, computed once;
    backward(ubar) and jvp(flow_dot, sim_dot) solve with it.  dtype=np.float64: the same formulas in fp64 with numpy's Cholesky solve
    (an fp64 evaluator for the measured constants; its units are not meant to be used)"""

    def __init__(self, ed, x, variant="ceres1", mode=EXACT, dtype=LD):
        assert mode in MODES
        self.ed, self.variant, self.mode, self.dtype = ed, variant, mode, dtype
        self.T = T = edge_terms(ed, x, variant, dtype)
        self.n_bound = int(T.bound.sum())
        self.gauss_newton = mode == GAUSS_NEWTON
        self.H = hessian(T, self.gauss_newton)
        self.status = OK if cholesky_succeeds(self.H) else INDEFINITE
        if self.status != OK and mode == FALLBACK:
            self.gauss_newton = True
            self.H = hessian(T, True)
            self.status = FELL_BACK if cholesky_succeeds(self.H) else INDEFINITE
        self._abs_inv = None

    # ---- linear algebra
    def solve(self, g):
        """H^-1 g, g [nv, 2] already 0 on bound coordinates"""
        g = g.reshape(-1)
        if self.dtype is not LD:
            L = np.linalg.cholesky(self.H)
            return np.linalg.solve(L.T, np.linalg.solve(L, g)).reshape(-1, 2)
        H64 = self.H.astype(np.float64)
        one = LS.solve_ld if len(g) <= LD_SOLVE_ROWS else LS.solve_refined
        y = np.zeros(len(g), LD)
        for _ in range(3):
            y = y + one(H64, (g - self.H @ y).astype(np.float64))
        return y.reshape(-1, 2)

    def abs_inverse(self):
        if self._abs_inv is None:
            H64, n = self.H.astype(np.float64), len(self.H)
            inv = CV.inverse_ld(H64) if n <= LD_SOLVE_ROWS else CV.inverse_refined(H64, list(range(n)))
            self._abs_inv = np.abs(inv)
        return self._abs_inv

    def solution_unit(self, y, rhs_unit):
        """lam_unit of the docstring for the solution y of H y = g"""
        hv_unit = HR.product(self.ed, self.T.x, y, self.variant, self.gauss_newton, True).hv_unit
        n = len(self.H)
        inner = hv_unit.reshape(-1) + rhs_unit.reshape(-1) + U * n * (np.abs(self.H) @ np.abs(y.reshape(-1)))
        return (self.abs_inverse() @ inner).reshape(-1, 2)

    # ---- the two passes
    def backward(self, ubar):
        T, ed, dt = self.T, self.ed, self.dtype
        if self.status == INDEFINITE:
            z = np.zeros
            return Backward(INDEFINITE, z((ed.nv, 2), dt), z((len(ed), 9, 2), dt), z(len(ed), dt), z((ed.nv, 2), dt), z((len(ed), 9, 2), dt),
                            z(len(ed), dt), self.n_bound)
        g = np.where(T.bound, dt(0), np.asarray(ubar).astype(dt).reshape(-1, 2))
        lam = np.where(T.bound, dt(0), self.solve(g))
        lam_unit = self.solution_unit(lam, np.zeros_like(lam)) if dt is LD else np.zeros_like(lam)
        gflow, gsim, fu, su = sweep(T, lam, lam_unit)
        return Backward(self.status, lam, gflow, gsim, lam_unit, fu, su, self.n_bound)

    def jvp(self, flow_dot, sim_dot):
        T, ed, dt = self.T, self.ed, self.dtype
        if self.status == INDEFINITE:
            z = np.zeros((ed.nv, 2), dt)
            return Jvp(INDEFINITE, z, z.copy(), z.copy(), z.copy(), self.n_bound)
        b, b_unit = rhs(T, flow_dot, sim_dot)
        xdot = np.where(T.bound, dt(0), self.solve(b))
        unit = self.solution_unit(xdot, b_unit) if dt is LD else np.zeros_like(xdot)
        return Jvp(self.status, xdot, b, unit, b_unit, self.n_bound)


def sweep(T, lam, lam_unit=None):
    """(g_flow [E, 9, 2], g_sim [E], their units) of the docstring for lambda [nv, 2] with error lam_unit (None: exact)"""
    ed, dt = T.ed, T.dtype
    lam = np.asarray(lam).astype(dt).reshape(-1, 2)
    zero = np.zeros((1, 2), dt)
    le = np.concatenate([lam, zero])
    ls, ld_ = le[ed.src], le[ed.dst]
    u = ld_ - _mv(T.P, ls)
    t = _mv(T.M, u)
    c = T.w * T.rho1
    gl = np.einsum("eji,ei->ej", T.gb, ls)                                        # grad b_ij . lambda_src
    cr = c[:, None] * T.r
    gflow = T.b[:, :, None] * t[:, None, :] + gl[:, :, None] * cr[:, None, :]
    gsim = -T.rho1 * (T.r * u).sum(1)
    # units at exact lambda
    als = np.abs(ls)
    au = np.abs(ld_) + _mv(T.aP, als)
    du = U * au + _mv(T.dP, als)
    dtt = _mv(T.dM, au) + _mv(T.aM, du)
    agl = np.einsum("eji,ei->ej", np.abs(T.gb), als)
    dcr = T.aw[:, None] * (T.drho1[:, None] * T.ar + T.rho1[:, None] * T.dr) + 3 * U * np.abs(cr)
    fu = np.abs(T.b)[:, :, None] * (U * np.abs(t) + dtt)[:, None, :] + agl[:, :, None] * dcr[:, None, :] + U * np.abs(gflow)
    su = T.drho1 * (T.ar * au).sum(1) + T.rho1 * ((T.dr * au).sum(1) + (T.ar * du).sum(1)) + 2 * U * T.rho1 * (T.ar * au).sum(1)
    if lam_unit is not None:
        de = np.concatenate([np.asarray(lam_unit).astype(dt).reshape(-1, 2), zero])
        dls = de[ed.src]
        ddu = de[ed.dst] + _mv(T.aP, dls)
        dgl = np.einsum("eji,ei->ej", np.abs(T.gb), dls)
        fu = fu + np.abs(T.b)[:, :, None] * _mv(T.aM, ddu)[:, None, :] + dgl[:, :, None] * np.abs(cr)[:, None, :]
        su = su + T.rho1 * (T.ar * ddu).sum(1)
    return gflow, gsim, fu, su


def rhs(T, flow_dot, sim_dot):
    """(b [nv, 2], its unit) of the jvp for the tangents of the component's edges, flow_dot [E, 18] (or [E, 9, 2]) and sim_dot [E]
    (None = 0), in the order of the edges; 0 on bound coordinates"""
    ed, dt = T.ed, T.dtype
    E = len(ed)
    fd = np.zeros((E, 9, 2), dt) if flow_dot is None else np.asarray(flow_dot).astype(dt).reshape(E, 9, 2)
    wd = np.zeros(E, dt) if sim_dot is None else np.asarray(sim_dot).astype(dt).reshape(E)
    bfd = T.b[:, :, None] * fd
    rdot, ardot = -bfd.sum(1), np.abs(bfd).sum(1)
    gfd = T.gb[:, :, None, :] * fd[:, :, :, None]                                 # [E, 9, k, i]
    Pdot, aPdot = gfd.sum(1), np.abs(gfd).sum(1)
    wr = wd[:, None] * T.rho1[:, None] * T.r
    qdot = wr + _mv(T.M, rdot)
    c = T.w * T.rho1
    bs = _mtv(T.P, qdot) + c[:, None] * _mtv(Pdot, T.r)
    b = np.zeros((ed.nv + 1, 2), dt)
    np.add.at(b, ed.dst, -qdot)
    np.add.at(b, ed.src, bs)
    # units
    awd, aq = np.abs(wd)[:, None], np.abs(qdot)
    dq = (awd * (T.drho1[:, None] * T.ar + T.rho1[:, None] * T.dr) + _mv(T.dM, np.abs(rdot)) + _mv(T.aM, U * ardot)
          + U * (np.abs(wr) + _mv(T.aM, np.abs(rdot))))
    ac = np.abs(c)[:, None]
    dbs = (_mtv(T.aP, dq) + _mtv(T.dP, aq) + U * _mtv(T.aP, aq) + (T.aw * T.drho1)[:, None] * _mtv(aPdot, T.ar)
           + ac * (U * _mtv(aPdot, T.ar) + _mtv(aPdot, T.dr) + 2 * U * _mtv(aPdot, T.ar)))
    A = np.zeros((ed.nv + 1, 2), dt)
    np.add.at(A, ed.dst, dq)
    np.add.at(A, ed.src, dbs)
    b = np.where(T.bound, dt(0), b[:ed.nv])
    unit = np.where(T.bound, dt(0), A[:ed.nv] + U * T.n_inc[:, None] * np.abs(b))
    return b, unit


def edge_tangents(ed, tan_disp1, tan_disp2, tan_sim):
    """(flow_dot [E, 18], sim_dot [E]) of a component's edges out of the match layout: directed edge 2 m reads tan_disp2[m], 2 m + 1
    tan_disp1[m], both tan_sim[m]"""
    m, odd = ed.eids >> 1, (ed.eids & 1) == 1
    return np.where(odd[:, None], tan_disp1.reshape(-1, 18)[m], tan_disp2.reshape(-1, 18)[m]), tan_sim[m]


def component_layout(ed, res):
    """one component's backward as the per-component tests compare it: (flow rows [E, 18], similarity gradient per match [n], their
    units, the matches [n]) - a match's similarity gradient is the sum of its directions in the component, its unit theirs plus 2^-53
    times the sum's magnitude"""
    m, k = np.unique(ed.eids >> 1, return_inverse=True)
    sim, unit = np.zeros(len(m), res.gsim.dtype), np.zeros(len(m), res.gsim.dtype)
    np.add.at(sim, k, res.gsim)
    np.add.at(unit, k, res.gsim_unit)
    return res.gflow.reshape(-1, 18), sim, res.gflow_unit.reshape(-1, 18), unit + U * np.abs(sim), m


def match_layout(comps, results, n_matches, dtype=np.float64):
    """the backward's three outputs in lfr_batch_backward's layout and their units from {component: Backward}: grad_disp1 / grad_disp2
    [n_matches, 18], grad_sim [n_matches]; directions that are no residual block of a component in `results` read 0 (unit 0).
    Returns (values, units, in_program): two dicts and the mask [2 n_matches] of the directed edges covered"""
    fl, fl_u = np.zeros((2 * n_matches, 18), dtype), np.zeros((2 * n_matches, 18))
    sd, sd_u = np.zeros(2 * n_matches, LD), np.zeros(2 * n_matches, LD)
    covered = np.zeros(2 * n_matches, bool)
    for c, res in results.items():
        ed = comps[c][1]
        assert not covered[ed.eids].any()
        covered[ed.eids] = True
        fl[ed.eids], fl_u[ed.eids] = res.gflow.reshape(-1, 18).astype(dtype), res.gflow_unit.reshape(-1, 18).astype(np.float64)
        sd[ed.eids], sd_u[ed.eids] = res.gsim, res.gsim_unit
    sim = sd[0::2] + sd[1::2]
    sim_u = sd_u[0::2] + sd_u[1::2] + U * np.abs(sim)
    # directed edge 2 m is node1 -> node2: its flow is disp2[m]; 2 m + 1 is node2 -> node1: disp1[m]
    return ({"disp1": fl[1::2], "disp2": fl[0::2], "sim": sim.astype(dtype)},
            {"disp1": fl_u[1::2], "disp2": fl_u[0::2], "sim": sim_u.astype(np.float64)}, covered)
