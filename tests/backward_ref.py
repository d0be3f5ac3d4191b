"""CPU reference of the implicit-gradient backward (lfr_batch_backward, include/lfr.h): the cost F of a component restated in torch
fp64 from oracle/lfr_ref.py's interpolant and losses, H from per-edge torch.func Hessians solved with numpy, the vector-Jacobian
product by autograd.  Test infrastructure."""
import numpy as np
import torch
from torch.func import hessian, vmap

import lfr_ref as R

_D = torch.float64


def _basis(t):
    t = torch.clamp(t, -0.5, 0.5)           # (clamp's derivative is 1 on [-0.5, 0.5] inclusive, 0 outside: cost.cc:38-43)
    return torch.stack([2.0 * t * (t - 0.5), -4.0 * (t - 0.5) * (t + 0.5), 2.0 * t * (t + 0.5)], -1)


def interpolate(flow, row, col):
    """lfr_ref.interpolate in torch, batched: flow [..., 18], row / col [...] -> f [..., 2]."""
    lr, lc = _basis(row), _basis(col)
    w = (lr[..., :, None] * lc[..., None, :]).reshape(*lr.shape[:-1], 9)
    return (w[..., :, None] * flow.reshape(*flow.shape[:-1], 9, 2)).sum(-2)


def rho(s, kind, variant):
    """Unscaled loss: kind 0 Cauchy(0.25), kind 1 Tukey(0.0625) (lfr_ref.cauchy_loss / tukey_loss)."""
    b = R.CAUCHY_A ** 2
    cauchy = b * torch.log1p(s / b)
    a2 = R.TUKEY_A ** 2
    k = a2 / 6.0 if variant == "ceres1" else a2 / 3.0
    v = 1.0 - torch.clamp(s, max=a2) / a2
    tukey = k * (1.0 - v ** 3)
    return torch.where(kind == 0, cauchy, tukey)


def edge_cost(z, flow, w, kind, variant):
    """1/2 w rho(|r|^2), z = (x_src, x_dst) [..., 4]."""
    r = z[..., 2:] - z[..., :2] - interpolate(flow, z[..., 0], z[..., 1])
    return 0.5 * w * rho((r * r).sum(-1), kind, variant)


class Component:
    """One component's reduced program: nv variable nodes, edges (src, dst, sim, kind, flow18) with -1 = constant node (as
    lfr_ref.assemble_component), optional graph edge ids."""

    def __init__(self, nv, edges, variant="ceres1", eids=None):
        self.nv = nv
        self.variant = variant
        self.src = np.array([e[0] for e in edges], np.int64)
        self.dst = np.array([e[1] for e in edges], np.int64)
        self.sim = torch.tensor([float(e[2]) for e in edges], dtype=_D)
        self.kind = torch.tensor([int(e[3]) for e in edges], dtype=torch.int64)
        self.flow = torch.tensor(np.array([np.asarray(e[4], np.float64) for e in edges]).reshape(-1, 18), dtype=_D)
        self.eids = None if eids is None else np.asarray(eids, np.int64)

    def _z(self, x):
        x = torch.as_tensor(np.asarray(x, np.float64).reshape(-1, 2), dtype=_D)
        xe = torch.cat([x, torch.zeros((1, 2), dtype=_D)])          # index -1: constant node at 0
        return torch.cat([xe[torch.as_tensor(self.src)], xe[torch.as_tensor(self.dst)]], 1)

    def cost(self, x, flow=None, sim=None):
        return edge_cost(self._z(x), self.flow if flow is None else flow, self.sim if sim is None else sim, self.kind,
                         self.variant).sum()

    def grad(self, x):
        z = self._z(x).requires_grad_(True)
        edge_cost(z, self.flow, self.sim, self.kind, self.variant).sum().backward()
        g = np.zeros((self.nv + 1, 2))
        np.add.at(g, self.src, z.grad[:, :2].numpy())
        np.add.at(g, self.dst, z.grad[:, 2:].numpy())
        return g[:self.nv].reshape(-1)

    def hessian(self, x, flow=None, sim=None):
        """Exact Hessian over all 2 nv coordinates (dense)."""
        flow = self.flow if flow is None else flow
        sim = self.sim if sim is None else sim
        f = lambda z, fl, w, k: edge_cost(z, fl, w, k, self.variant)
        he = vmap(hessian(f))(self._z(x), flow, sim, self.kind).numpy()            # [E, 4, 4]
        n = 2 * self.nv
        H = np.zeros((n + 2, n + 2))
        idx = np.stack([2 * self.src, 2 * self.src + 1, 2 * self.dst, 2 * self.dst + 1], 1)
        idx[idx < 0] += n + 2                                                        # constant node -> the two spare rows
        for a in range(4):
            for b in range(4):
                np.add.at(H, (idx[:, a], idx[:, b]), he[:, a, b])
        return H[:n, :n]

    def free(self, x):
        return np.abs(np.asarray(x, np.float64).reshape(-1)) < R.BOUND

    def backward(self, x, ubar):
        """(grad_flow [E, 18], grad_sim [E], status): status 0 ok, 2 indefinite (zero gradient) - lfr.h's contract."""
        x = np.asarray(x, np.float64).reshape(-1)
        fr = self.free(x)
        H = self.hessian(x)
        H[~fr, :] = 0.0
        H[:, ~fr] = 0.0
        H[~fr, ~fr] = 1.0
        rhs = np.where(fr, np.asarray(ubar, np.float64).reshape(-1), 0.0)
        E = len(self.src)
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            return np.zeros((E, 18)), np.zeros(E), 2
        v = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
        flow = self.flow.clone().requires_grad_(True)
        sim = self.sim.clone().requires_grad_(True)
        z = self._z(x).requires_grad_(True)
        gz, = torch.autograd.grad(edge_cost(z, flow, sim, self.kind, self.variant).sum(), z, create_graph=True)
        ve = torch.as_tensor(np.concatenate([v, np.zeros(2)]).reshape(-1, 2), dtype=_D)
        V = torch.cat([ve[torch.as_tensor(self.src)], ve[torch.as_tensor(self.dst)]], 1)
        G = (gz * V).sum()
        gf, gw = torch.autograd.grad(G, (flow, sim), allow_unused=True)
        gf = torch.zeros_like(flow) if gf is None else gf
        gw = torch.zeros_like(sim) if gw is None else gw
        return -gf.detach().numpy(), -gw.detach().numpy(), 0

    def newton_polish(self, x, iters=50, tol=1e-12, flow=None, sim=None):
        """Newton on the free coordinates (bound coordinates stay) to |g| < tol."""
        x = np.asarray(x, np.float64).reshape(-1).copy()
        fr = self.free(x)
        saved = (self.flow, self.sim)
        if flow is not None:
            self.flow = flow
        if sim is not None:
            self.sim = sim
        try:
            for _ in range(iters):
                g = self.grad(x)[fr]
                if np.abs(g).max(initial=0.0) < tol:
                    break
                H = self.hessian(x)[np.ix_(fr, fr)]
                x[fr] -= np.linalg.solve(H, g)
            return x, float(np.abs(self.grad(x)[fr]).max(initial=0.0))
        finally:
            self.flow, self.sim = saved


def graph_components(ma, track, is_root, comp, node_image, node_feature, variant="ceres1", which=None):
    """The reduced programs of the graph's components from its labels (lfr_ref.assemble_component, vectorised over the matches):
    {component id: (var_nodes, Component with graph edge ids)} for the components in `which` (None: all with a variable)."""
    key = node_image.astype(np.int64) << 32 | node_feature.astype(np.int64)
    order = np.argsort(key)
    P = len(ma.pair_img1)
    pi = np.repeat(np.arange(P), np.diff(ma.pair_off))
    k1 = ma.pair_img1[pi].astype(np.int64) << 32 | ma.feat1.astype(np.int64)
    k2 = ma.pair_img2[pi].astype(np.int64) << 32 | ma.feat2.astype(np.int64)
    n1 = order[np.searchsorted(key[order], k1)]
    n2 = order[np.searchsorted(key[order], k2)]
    M = len(n1)
    src = np.stack([n1, n2], 1).reshape(-1)                 # directed edge 2m: n1 -> n2 (disp2), 2m+1: n2 -> n1 (disp1)
    dst = np.stack([n2, n1], 1).reshape(-1)
    flows = np.stack([np.asarray(ma.disp2, np.float32).reshape(M, 18), np.asarray(ma.disp1, np.float32).reshape(M, 18)], 1).reshape(-1, 18)
    sims = np.repeat(np.asarray(ma.sim, np.float32), 2)
    intra = track[src] == track[dst]
    kept = intra | (comp[src] == comp[dst])
    eid = np.nonzero(kept)[0]
    by_comp = {}
    cs = comp[src[eid]]
    o = np.argsort(cs, kind="stable")
    bounds = np.searchsorted(cs[o], np.unique(cs))
    for k, c in enumerate(np.unique(cs)):
        if which is not None and c not in which:
            continue
        ids = eid[o[bounds[k]:bounds[k + 1] if k + 1 < len(bounds) else len(o)]]
        ids = ids[np.lexsort((ids, src[ids]))]              # residual-block order: by source node, then edge id
        nodes = np.unique(np.concatenate([src[ids], dst[ids]]))
        var_nodes = [int(n) for n in nodes if not is_root[n]]
        if not var_nodes:
            continue
        vidx = {n: i for i, n in enumerate(var_nodes)}
        edges = [(vidx.get(int(src[e]), -1), vidx.get(int(dst[e]), -1), float(sims[e]), R.KIND_INTRA if intra[e] else R.KIND_INTER,
                  flows[e].astype(np.float64)) for e in ids]
        by_comp[int(c)] = (np.array(var_nodes), Component(len(var_nodes), edges, variant, eids=ids))
    return by_comp


def scatter(n_matches, comps_grads):
    """[(eids, grad_flow [E, 18], grad_sim [E])] -> (grad_disp1, grad_disp2, grad_sim) in the match layout."""
    g1 = np.zeros((n_matches, 18))
    g2 = np.zeros((n_matches, 18))
    gs = np.zeros(n_matches)
    for eids, gf, gw in comps_grads:
        m = eids >> 1
        odd = (eids & 1) == 1
        g1[m[odd]] = gf[odd]
        g2[m[~odd]] = gf[~odd]
        np.add.at(gs, m, gw)
    return g1, g2, gs
