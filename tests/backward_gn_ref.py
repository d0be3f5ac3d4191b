"""CPU reference of the Gauss-Newton mode of the implicit-gradient backward (LFR_BACKWARD_GAUSS_NEWTON, include/lfr.h), built on
backward_ref.Component: H_GN = sum_e w rho' J^T J with J = [-(I + df/dx_src), I] per edge from torch fp64 (the interpolant's Jacobian
by autograd: clamp's derivative is the reference's zeroing outside [-0.5, 0.5]; rho' by autograd of the unscaled loss), then the bound
handling, the Cholesky solve and the autograd sweep of Component.backward unchanged - only H differs.  Test infrastructure."""
import numpy as np
import torch
from torch.func import jacrev, vmap

import backward_ref as BR

_D = torch.float64


class Component(BR.Component):
    """backward_ref.Component whose `hessian` is the loss-corrected Gauss-Newton matrix: backward() (bounds, Cholesky, status 2 on
    LinAlgError, the exact sweep) is inherited and therefore the Gauss-Newton mode's."""

    @classmethod
    def of(cls, cp):
        """The Gauss-Newton view of an exact-mode component (shares its arrays)."""
        out = cls.__new__(cls)
        out.__dict__.update(cp.__dict__)
        return out

    def edge_blocks(self, x, flow=None, sim=None):
        """w rho' J^T J per edge over (x_src, x_dst): [E, 4, 4]."""
        flow = self.flow if flow is None else flow
        sim = self.sim if sim is None else sim
        z = self._z(x)
        f = lambda p, fl: BR.interpolate(fl, p[0], p[1])
        dfdx = vmap(jacrev(f))(z[:, :2], flow)                                     # [E, 2 (k), 2 (row, col)]
        r = z[:, 2:] - z[:, :2] - BR.interpolate(flow, z[:, 0], z[:, 1])
        s = (r * r).sum(-1).detach().requires_grad_(True)
        rho1, = torch.autograd.grad(BR.rho(s, self.kind, self.variant).sum(), s)
        eye = torch.eye(2, dtype=_D).expand(len(s), 2, 2)
        J = torch.cat([-(eye + dfdx), eye], 2)                                      # [E, 2, 4]
        return ((sim * rho1)[:, None, None] * (J.transpose(1, 2) @ J)).detach().numpy()

    def hessian(self, x, flow=None, sim=None):
        """H_GN over all 2 nv coordinates (dense), summed per edge."""
        he = self.edge_blocks(x, flow, sim)
        n = 2 * self.nv
        H = np.zeros((n + 2, n + 2))
        idx = np.stack([2 * self.src, 2 * self.src + 1, 2 * self.dst, 2 * self.dst + 1], 1)
        idx[idx < 0] += n + 2                                                        # constant node -> the two spare rows
        for a in range(4):
            for b in range(4):
                np.add.at(H, (idx[:, a], idx[:, b]), he[:, a, b])
        return H[:n, :n]

    def reduced(self, x):
        """H_GN with the rows and columns of the bound coordinates replaced by the identity's: the matrix backward() factors."""
        x = np.asarray(x, np.float64).reshape(-1)
        fr = self.free(x)
        H = self.hessian(x)
        H[~fr, :] = 0.0
        H[:, ~fr] = 0.0
        H[~fr, ~fr] = 1.0
        return H

    def is_positive_definite(self, x):
        try:
            np.linalg.cholesky(self.reduced(x))
            return True
        except np.linalg.LinAlgError:
            return False

    def kappa2(self, x):
        ev = np.linalg.eigvalsh(self.reduced(x))
        return float(ev[-1] / ev[0])


def graph_components(*args, **kw):
    """backward_ref.graph_components with Gauss-Newton components."""
    return {c: (var_nodes, Component.of(cp)) for c, (var_nodes, cp) in BR.graph_components(*args, **kw).items()}
