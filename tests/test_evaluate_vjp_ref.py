"""tests/evaluate_vjp_ref.py pinned without a GPU: its four gradients against torch float64 autograd - of backward_ref's cost for the
cost bar, of the residuals and weights restated in torch for their bars - and the measurements behind GAMMA_VJP_X_CPU /
GAMMA_VJP_FLOW_CPU / GAMMA_VJP_SIM_CPU (the method of tests/test_evaluate_ref.py), on every component of that file's inputs at both
position sets and the three bar sets of tests/test_gpu_evaluate_vjp.py."""
import numpy as np
import torch

import backward_ref as BR
import cost_ref as CR
import evaluate_vjp_ref as VR
import lfr_ref as R
from test_evaluate_ref import _ratio, inputs

LD = CR.LD
_D = torch.float64


def _torch_grads(ed, x, variant, cbar, rbar, wbar):
    """(dL/dx [nv, 2], dL/dflow [E, 9, 2], dL/dsim [E]) of L = cbar F + sum rbar . r + sum wbar rho' by torch float64 autograd: F is
    backward_ref.Component.cost(x, flow, sim) (its edge_cost over the component's z), r and rho' are written out here"""
    cp = BR.Component(ed.nv, list(zip(ed.src.tolist(), ed.dst.tolist(), ed.w.astype(np.float64), ed.kind.tolist(),
                                      ed.flow.astype(np.float64).reshape(-1, 18))), variant)
    xt = torch.tensor(np.asarray(x, np.float64).reshape(-1, 2), dtype=_D, requires_grad=True)
    flow, sim = cp.flow.clone().requires_grad_(True), cp.sim.clone().requires_grad_(True)
    xe = torch.cat([xt, torch.zeros((1, 2), dtype=_D)])
    z = torch.cat([xe[torch.as_tensor(cp.src)], xe[torch.as_tensor(cp.dst)]], 1)
    L = float(cbar) * BR.edge_cost(z, flow, sim, cp.kind, variant).sum()
    if rbar is not None or wbar is not None:
        r = z[:, 2:] - z[:, :2] - BR.interpolate(flow, z[:, 0], z[:, 1])
        s = (r * r).sum(-1)
        b, a2 = R.CAUCHY_A ** 2, R.TUKEY_A ** 2
        k = a2 / 6.0 if variant == "ceres1" else a2 / 3.0
        v = 1.0 - torch.clamp(s, max=a2) / a2
        rho1 = torch.where(cp.kind == 0, 1.0 / (1.0 + s / b), 3.0 * k / a2 * v * v)
        if rbar is not None:
            L = L + (torch.as_tensor(np.asarray(rbar, np.float64)) * r).sum()
        if wbar is not None:
            L = L + (torch.as_tensor(np.asarray(wbar, np.float64)) * rho1).sum()
    L.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return zero(xt).numpy(), zero(flow).numpy().reshape(-1, 9, 2), zero(sim).numpy()


def test_reference_agrees_with_autograd_and_the_gammas_are_as_recorded():
    """(i) the longdouble reference against torch autograd and (ii) against its own formulas in numpy float64, both in the reference's
    units: every error within the recorded constant, the largest one not below half of it (the constants stay measurements)"""
    worst = {"x": 0.0, "x_torch": 0.0, "flow": 0.0, "flow_torch": 0.0, "sim": 0.0, "sim_torch": 0.0}
    n = n_sat = 0
    for label, variant, comps, sets in inputs():
        w_in = dict.fromkeys(worst, 0.0)
        order = sorted(comps)
        n_matches = 1 + max(int(ed.eids.max()) for _, ed in comps.values()) // 2
        for which, pos in sets.items():
            for bset in VR.BAR_SETS:
                cbar, rbar, wbar = VR.bars(len(order), n_matches, bset)
                for i, c in enumerate(order):
                    var_nodes, ed = comps[c]
                    x = pos[var_nodes]
                    cb, rb, wb = VR.component_bars(ed, i, cbar, rbar, wbar)
                    ref = VR.vjp(ed, x, cb, rb, wb, variant)
                    v64 = VR.vjp(ed, x, cb, rb, wb, variant, dtype=np.float64)
                    tx, tf, ts = _torch_grads(ed, x, variant, cb, rb, wb)
                    for key, got, want, unit in (("x", v64.gx, ref.gx, ref.gx_unit), ("x_torch", tx, ref.gx, ref.gx_unit),
                                                 ("flow", v64.gflow, ref.gflow, ref.gflow_unit), ("flow_torch", tf, ref.gflow, ref.gflow_unit),
                                                 ("sim", v64.gsim, ref.gsim, ref.gsim_unit), ("sim_torch", ts, ref.gsim, ref.gsim_unit)):
                        w_in[key] = max(w_in[key], _ratio(np.abs(np.asarray(got).astype(LD) - want), unit))
                    if bset == "r" and not ref.nonzero_loss.all():          # a saturated Tukey edge passes rbar and nothing else
                        sat = ~ref.nonzero_loss
                        assert ref.gflow[sat].any() and not VR.vjp(ed, x, cbar=1.0, wbar=np.ones(len(ed)), variant=variant).gflow[sat].any()
                        n_sat += 1
                    n += 1
        print("%-14s %-6s largest error / unit: positions %.4f (numpy) %.4f (torch), flows %.4f %.4f, similarities %.4f %.4f"
              % (label, variant, w_in["x"], w_in["x_torch"], w_in["flow"], w_in["flow_torch"], w_in["sim"], w_in["sim_torch"]))
        for key in worst:
            worst[key] = max(worst[key], w_in[key])
    measured = {"GAMMA_VJP_X_CPU": max(worst["x"], worst["x_torch"]), "GAMMA_VJP_FLOW_CPU": max(worst["flow"], worst["flow_torch"]),
                "GAMMA_VJP_SIM_CPU": max(worst["sim"], worst["sim_torch"])}
    for name, m in measured.items():
        print("%s: measured %.4f over %d component sweeps, recorded %.4g, on the GPU %d x" % (name, m, n, getattr(VR, name), VR.GPU_FACTOR))
    assert n_sat >= 2
    for name, m in measured.items():
        assert 0.5 * getattr(VR, name) <= m <= getattr(VR, name), (name, m)          # (the constants stay measurements)
    assert VR.GPU_FACTOR == 8


def test_cost_bar_one_gives_evaluate_refs_gradient():
    """cbar = 1 and no other bar: dL/dx is dF/dx, the reference lfr_batch_evaluate's gradient is held to"""
    import evaluate_ref as ER
    label, variant, comps, sets = inputs()[0]
    for c in sorted(comps)[:12]:
        var_nodes, ed = comps[c]
        x = sets["b"][var_nodes]
        ev = ER.evaluate(ed, x, variant)                                          # (two longdouble evaluations: 2^-11 of an fp64 unit apart at most)
        assert (np.abs(VR.vjp(ed, x, 1.0, variant=variant).gx - ev.grad) <= ev.g_unit / 256).all(), c
