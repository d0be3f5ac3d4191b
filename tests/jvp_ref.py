"""CPU reference of the forward-mode sensitivity (lfr_batch_jvp, include/lfr.h) on top of backward_ref.Component: the right-hand side
b = -d/d eps [grad_x F(x; theta + eps thetadot)] by torch double-backward, the dense H of Component.backward (the Gauss-Newton one from
backward_gn_ref) with the identity on bound rows, and a Cholesky solve.  Test infrastructure."""
import numpy as np
import torch
from torch.func import hessian, vmap

import backward_gn_ref as GN
import backward_ref as BR

_D = torch.float64


def rhs(comp, x, flow_dot, sim_dot):
    """b over all 2 nv coordinates: flow_dot [E, 18], sim_dot [E] are the tangents of the component's edges (in its edge order)."""
    flow = comp.flow.clone().requires_grad_(True)
    sim = comp.sim.clone().requires_grad_(True)
    z = comp._z(x).requires_grad_(True)
    gz, = torch.autograd.grad(BR.edge_cost(z, flow, sim, comp.kind, comp.variant).sum(), z, create_graph=True)
    # forward mode by double-backward: d/d eps gz = d/d lam [ (d/d theta (lam . gz)) . thetadot ]
    lam = torch.zeros_like(gz).requires_grad_(True)
    gf, gw = torch.autograd.grad((gz * lam).sum(), (flow, sim), create_graph=True, allow_unused=True)
    s = torch.zeros((), dtype=_D)
    if gf is not None:
        s = s + (gf * torch.as_tensor(np.asarray(flow_dot, np.float64).reshape(-1, 18), dtype=_D)).sum()
    if gw is not None:
        s = s + (gw * torch.as_tensor(np.asarray(sim_dot, np.float64).reshape(-1), dtype=_D)).sum()
    if not s.requires_grad:
        return np.zeros(2 * comp.nv)
    dz, = torch.autograd.grad(s, lam)
    dz = dz.detach().numpy()
    b = np.zeros((comp.nv + 1, 2))
    np.add.at(b, comp.src, dz[:, :2])
    np.add.at(b, comp.dst, dz[:, 2:])
    return -b[:comp.nv].reshape(-1)


def _solve(H, b, fr):
    H[~fr, :] = 0.0
    H[:, ~fr] = 0.0
    H[~fr, ~fr] = 1.0
    b = np.where(fr, b, 0.0)
    try:
        L = np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return np.zeros(len(b)), 2
    xdot = np.linalg.solve(L.T, np.linalg.solve(L, b))
    xdot[~fr] = 0.0
    return xdot, 0


def jvp_many(items, gauss_newton=False):
    """jvp() of many components at once: items = [(comp, x, flow_dot, sim_dot)] of one Tukey variant -> [(xdot, status)].  The
    components are independent, so their edges go through torch as ONE program (one double-backward, one batch of per-edge Hessian
    blocks); the dense H, its bounds and its Cholesky stay per component."""
    if not items:
        return []
    all_ = BR.Component.__new__(BR.Component)
    off = np.cumsum([0] + [c.nv for c, _, _, _ in items])
    all_.nv, all_.variant, all_.eids = int(off[-1]), items[0][0].variant, None
    shift = lambda a, o: np.where(a >= 0, a + o, -1)
    all_.src = np.concatenate([shift(c.src, o) for (c, _, _, _), o in zip(items, off)])
    all_.dst = np.concatenate([shift(c.dst, o) for (c, _, _, _), o in zip(items, off)])
    all_.sim = torch.cat([c.sim for c, _, _, _ in items])
    all_.kind = torch.cat([c.kind for c, _, _, _ in items])
    all_.flow = torch.cat([c.flow for c, _, _, _ in items])
    x = np.concatenate([np.asarray(x, np.float64).reshape(-1) for _, x, _, _ in items])
    b = rhs(all_, x, np.concatenate([np.asarray(f, np.float64).reshape(-1, 18) for _, _, f, _ in items]),
            np.concatenate([np.asarray(s, np.float64).reshape(-1) for _, _, _, s in items]))
    if gauss_newton:
        he = GN.Component.of(all_).edge_blocks(x)
    else:
        f = lambda z, fl, w, k: BR.edge_cost(z, fl, w, k, all_.variant)
        he = vmap(hessian(f))(all_._z(x), all_.flow, all_.sim, all_.kind).numpy()
    out, e0 = [], 0
    for (c, _, _, _), o in zip(items, off):
        E, n = len(c.src), 2 * c.nv
        H = np.zeros((n + 2, n + 2))
        idx = np.stack([2 * c.src, 2 * c.src + 1, 2 * c.dst, 2 * c.dst + 1], 1)
        idx[idx < 0] += n + 2                                                        # constant node -> the two spare rows
        for p in range(4):
            for q in range(4):
                np.add.at(H, (idx[:, p], idx[:, q]), he[e0:e0 + E, p, q])
        xs = x[2 * o:2 * o + n]
        out.append(_solve(H[:n, :n], b[2 * o:2 * o + n], c.free(xs)))
        e0 += E
    return out


def jvp(comp, x, flow_dot, sim_dot, gauss_newton=False):
    """(xdot [2 nv], status): status 0 ok, 2 indefinite (zero tangent) - lfr.h's contract.  Bound coordinates get an exact 0."""
    x = np.asarray(x, np.float64).reshape(-1)
    H = GN.Component.of(comp).hessian(x) if gauss_newton else BR.Component.hessian(comp, x)      # (whichever view `comp` is)
    return _solve(H, rhs(comp, x, flow_dot, sim_dot), comp.free(x))
