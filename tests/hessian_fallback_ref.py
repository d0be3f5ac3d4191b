"""CPU reference of the Gauss-Newton fallback of the backward and the jvp (LFR_BACKWARD_FALLBACK_GAUSS_NEWTON,
LFR_JVP_FALLBACK_GAUSS_NEWTON, include/lfr.h), composed from the references the two pure modes already have: per component the exact
result of backward_ref / jvp_ref with status 0; where the exact Hessian is indefinite the Gauss-Newton result of backward_gn_ref /
jvp_ref with status 3; where J^T J fails too, zeros with status 2.  Nothing is restated here - the three references decide (numpy's
Cholesky) and compute.  Test infrastructure."""
import numpy as np

import backward_gn_ref as GN
import backward_ref as BR
import jvp_ref as JR

OK, INDEFINITE, FALLBACK = 0, 2, 3


def exact_view(cp):
    """The exact-mode view of a component, whichever view `cp` is (shares its arrays)."""
    out = BR.Component.__new__(BR.Component)
    out.__dict__.update(cp.__dict__)
    return out


def kappa2(cp, x, status):
    """kappa_2 of the matrix the composition used for status 0 or 3 (bound rows and columns the identity's); inf for status 2."""
    if status == INDEFINITE:
        return np.inf
    if status == FALLBACK:
        return GN.Component.of(cp).kappa2(x)
    x = np.asarray(x, np.float64).reshape(-1)
    fr = cp.free(x)
    H = exact_view(cp).hessian(x)
    H[~fr, :] = 0.0
    H[:, ~fr] = 0.0
    H[~fr, ~fr] = 1.0
    ev = np.linalg.eigvalsh(H)
    return float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf


def backward(cp, x, ubar):
    """(grad_flow [E, 18], grad_sim [E], status, kappa_2): the exact reference's gradient with status 0, else the Gauss-Newton
    reference's with status 3, else zeros with status 2."""
    gf, gw, rs = exact_view(cp).backward(x, ubar)
    status = OK
    if rs != 0:
        gf, gw, rs = GN.Component.of(cp).backward(x, ubar)
        status = FALLBACK if rs == 0 else INDEFINITE
    return gf, gw, status, kappa2(cp, x, status)


def jvp(cp, x, flow_dot, sim_dot):
    """(xdot [2 nv], status, kappa_2): jvp_ref.jvp with the exact H, else with J^T J (status 3), else zeros (status 2)."""
    xdot, rs = JR.jvp(exact_view(cp), x, flow_dot, sim_dot)
    status = OK
    if rs != 0:
        xdot, rs = JR.jvp(cp, x, flow_dot, sim_dot, gauss_newton=True)
        status = FALLBACK if rs == 0 else INDEFINITE
    return xdot, status, kappa2(cp, x, status)


def jvp_many(items):
    """jvp() of many components at once: items = [(comp, x, flow_dot, sim_dot)] -> [(xdot, status)] (jvp_ref.jvp_many: one torch
    program for the exact pass over all of them, one for the Gauss-Newton pass over those the exact pass left indefinite)."""
    out = [(xdot, OK if rs == 0 else INDEFINITE) for xdot, rs in JR.jvp_many(items)]
    again = [k for k, (_, s) in enumerate(out) if s != OK]
    for k, (xdot, rs) in zip(again, JR.jvp_many([items[k] for k in again], gauss_newton=True)):
        out[k] = (xdot, FALLBACK if rs == 0 else INDEFINITE)
    return out
