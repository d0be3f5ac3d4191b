"""lfr_batch_backward and lfr_batch_jvp held entry by entry to the extended-precision reference of tests/backward_ld_ref.py, at the GPU's
own positions: every flow-gradient entry of every kept directed edge, every match's similarity gradient, every coordinate of xdot and
every status, in the three Hessian modes, on the 33 shapes of tests/class_limit_cases.py (every launch class at its row and edge
limits; ring98 / k98: H in the HBM workspace) and on the components of lm_decision_cases' packed_24_32 and block_m with a coordinate at
the bound.  The normwise tests (test_gpu_backward, _gn, test_gpu_hessian_fallback, test_gpu_class_limits, test_gpu_jvp_class_limits:
1e-8 |ref|_2 + 1e-14 per component) stay; tests/test_backward_ld_ref.py shows on the CPU what they cannot see and this criterion does -
a float32 row, similarity gradients off by 3e-7, one coordinate of lambda off by 1e-9.

Tolerance per entry: evaluate_ref.GPU_FACTOR (8) x the constant measured on the CPU (GAMMA_BWD_FLOW_CPU, GAMMA_BWD_SIM_CPU,
GAMMA_JVP_CPU) x the entry's first-order unit; an entry whose unit is 0 (a match outside the program, a flow entry whose basis value is
exactly 0, a root, a bound coordinate, a component with status 2) is exactly 0.  The references are computed once per (mode, inputs,
positions) and shared; a shape draws its dL/dx and its tangents from streams of its own, so it has the same ones in every batch."""
import numpy as np
import pytest
import torch

import backward_ld_ref as BL
import class_limit_cases as CL
import cost_ref as CR
import lm_decision_cases as LC
from test_backward_ld_ref import BOUND_COUNTS
from test_gpu_backward import _nodes, _ubar
from test_gpu_class_limits import N, all_solved, alone_solved
from test_gpu_jvp import _tangents
from test_gpu_jvp_class_limits import _shape_tangents, _twice
from test_gpu_lm_decisions import solved
from lfr_amd import capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LD = CR.LD
MODE_KW = {BL.EXACT: {}, BL.GAUSS_NEWTON: dict(gauss_newton=True), BL.FALLBACK: dict(gn_fallback=True)}
THREE_MODES = pytest.mark.parametrize("mode", list(BL.MODES))
TOL = {"flow": BL.GPU_FACTOR * BL.GAMMA_BWD_FLOW_CPU, "sim": BL.GPU_FACTOR * BL.GAMMA_BWD_SIM_CPU, "xdot": BL.GPU_FACTOR * BL.GAMMA_JVP_CPU}
UBAR_SEED = 7700       # shape k of CL.NAMES draws its dL/dx from seed UBAR_SEED + k
_reference = {}
_runs = {}


def _shape_ubar(n_nodes, nodes_list):
    """dL/dx [n_nodes, 2] of a batch of shapes: every shape's nodes (class_limit_cases' order, the same in every batch) from its own stream"""
    ub = np.zeros((n_nodes, 2))
    for nodes in nodes_list:
        for name, idx in nodes.items():
            ub[idx] = np.random.default_rng(UBAR_SEED + CL.NAMES.index(name)).standard_normal((len(idx), 2))
    return ub


def _component_reference(variant, mode, ed, x, ub, fdot, sdot):
    """(Backward, Jvp) of the longdouble reference, once per (mode, component inputs, positions, dL/dx, tangents).  A component
    without an inter-track edge is the same under both Tukey variants; the fallback mode IS the exact mode where that factors"""
    f64 = lambda a: np.ascontiguousarray(a, np.float64).tobytes()
    key = (variant if (ed.kind == CR.KIND_INTER).any() else "", mode, ed.src.tobytes(), ed.dst.tobytes(), f64(ed.flow), f64(ed.w),
           f64(x), f64(ub), f64(fdot), f64(sdot))
    if key not in _reference:
        if mode == BL.FALLBACK:
            exact = _component_reference(variant, BL.EXACT, ed, x, ub, fdot, sdot)
            if exact[0].status == BL.OK:
                _reference[key] = exact
                return exact
        cp = BL.Component(ed, x, variant, mode)
        _reference[key] = (cp.backward(ub), cp.jvp(fdot, sdot))
    return _reference[key]


def _gpu(b, ub, ts, mode):
    """one backward and one jvp of the batch in `mode`, float64 in and out: outputs, stats and per-component statuses"""
    g1, g2, gs, bst = b.backward(torch.as_tensor(ub, device=DEV), f64=True, want_stats=True, **MODE_KW[mode])
    out = dict(disp1=g1.cpu().numpy(), disp2=g2.cpu().numpy(), sim=gs.cpu().numpy(), bst=bst, bstat=b.backward_status().copy())
    xdot, jst = b.jvp(*[torch.as_tensor(t, device=DEV) for t in ts], f64=True, want_stats=True, **MODE_KW[mode])
    out.update(xdot=xdot.cpu().numpy(), jst=jst, jstat=b.jvp_status().copy())
    assert all(out[k].dtype == np.float64 for k in ("disp1", "disp2", "sim", "xdot"))
    return out


def _worst(got, ref, unit, factor, what):
    """largest |got - ref| / (factor unit) over the entries with a unit; the others are exactly 0"""
    got, ref, unit = np.asarray(got).astype(LD).reshape(-1), np.asarray(ref, LD).reshape(-1), np.asarray(unit, LD).reshape(-1)
    exact = unit == 0
    assert not got[exact].any() and not ref[exact].any(), what
    return float((np.abs(got - ref)[~exact] / (factor * unit[~exact])).max(initial=0.0))


def _compare(ma, g, p, b, pos, out, ub, ts, variant, mode, which=None):
    """Every output entry of the components `which` (None: all, and then every entry of the whole arrays) against the reference at
    `pos` -> dict(flow, sim, xdot: worst error / tolerance; status: {component: reference status}; adjoint: worst mismatch / bound and
    the worst relative mismatch; n: components compared)"""
    track, root, comp = p.labels()
    comps = CR.components(ma, track, root, comp, *_nodes(g, ma), which=None if which is None else set(which))
    info = b.component_info()
    order = info["component"].tolist()
    bstat, jstat = dict(zip(order, out["bstat"].tolist())), dict(zip(order, out["jstat"].tolist()))
    assert sorted(comps) == sorted(order if which is None else which)
    w = dict(flow=0.0, sim=0.0, xdot=0.0, adjoint=0.0, adjoint_rel=0.0, status={}, n=0)
    covered, variable = np.zeros(2 * len(ma.sim), bool), np.zeros(len(pos), bool)
    for c, (var_nodes, ed) in comps.items():
        x = pos[var_nodes]
        fdot, sdot = BL.edge_tangents(ed, *ts)
        rb, rj = _component_reference(variant, mode, ed, x, ub[var_nodes], fdot, sdot)
        assert rb.status == rj.status and bstat[c] == jstat[c] == rb.status, "component %d: status %d / %d, reference %d" % (c, bstat[c], jstat[c], rb.status)
        w["status"][c] = rb.status
        assert rb.n_bound == int((np.abs(x) >= 1).sum())
        m, odd = ed.eids >> 1, (ed.eids & 1) == 1
        rf, rs, fu, su, mm = BL.component_layout(ed, rb)
        gf, gs, gx = np.where(odd[:, None], out["disp1"][m], out["disp2"][m]), out["sim"][mm], out["xdot"][var_nodes]
        what = "component %d" % c
        w["flow"] = max(w["flow"], _worst(gf, rf, fu, TOL["flow"], what))
        w["sim"] = max(w["sim"], _worst(gs, rs, su, TOL["sim"], what))
        w["xdot"] = max(w["xdot"], _worst(gx, rj.xdot, rj.xdot_unit, TOL["xdot"], what))
        assert not covered[ed.eids].any()
        covered[ed.eids], variable[var_nodes] = True, True
        if rb.status != BL.INDEFINITE:
            # the adjoint identity at float64, both sides the GPU's: ubar . xdot against sum gradient . tangent, in longdouble
            free = np.abs(x) < 1
            lhs = (np.where(free, ub[var_nodes], 0.0).astype(LD) * gx.astype(LD)).sum()
            rhs = (gf.astype(LD) * fdot).sum() + (gs.astype(LD) * ts[2][mm]).sum()
            bound = (TOL["xdot"] * (np.abs(ub[var_nodes]) * rj.xdot_unit).sum() + TOL["flow"] * (np.abs(fdot) * fu).sum()
                     + TOL["sim"] * (np.abs(ts[2][mm]) * su).sum())
            scale = (np.linalg.norm(ub[var_nodes][free]) * np.linalg.norm(gx) + np.sqrt((gf ** 2).sum() + (gs ** 2).sum())
                     * np.sqrt((fdot ** 2).sum() + (ts[2][mm] ** 2).sum()))
            w["adjoint"] = max(w["adjoint"], float(abs(lhs - rhs) / bound))
            w["adjoint_rel"] = max(w["adjoint_rel"], float(abs(lhs - rhs)) / scale)
            w["n"] += 1
    if which is None:                                             # everything outside the components' programs reads exact zeros
        assert not out["disp2"][~covered[0::2]].any() and not out["disp1"][~covered[1::2]].any()
        assert not out["sim"][~(covered[0::2] | covered[1::2])].any() and not out["xdot"][~variable].any() and root[~variable].all()
    return w


def _shape_run(s, mode, nodes_list=None):
    """the GPU's outputs for a batch of shapes under the shapes' own dL/dx and tangents, once per (batch, mode)"""
    key = (id(s.b), mode)
    if key not in _runs:
        views = [s] if nodes_list is None else nodes_list
        ub = _shape_ubar(s.g.n_nodes, [v.nodes for v in views])
        ts = _shape_tangents(s.ma, [v.feats for v in views])
        _runs[key] = (ub, ts, _gpu(s.b, ub, ts, mode))
    return _runs[key]


def _assert_all_ok(out, n):
    assert len(out["bstat"]) == n and (out["bstat"] == capi.BACKWARD_OK).all() and (out["jstat"] == capi.JVP_OK).all()
    for st in (out["bst"], out["jst"]):
        assert st["n_differentiated"] == n and st["n_not_usable"] == 0 and st["n_indefinite"] == 0 and st["n_bound_coordinates"] == 0


# --------------------------------------------------------------- 1.-3. every class at its limits: backward, jvp, adjoint identity
@pytest.mark.parametrize("device_assembly", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
@THREE_MODES
def test_every_entry_on_every_shape(lfr_lib, mode, variant, device_assembly):
    """all 33 shapes compared, status 0 everywhere: every flow row, similarity gradient and xdot coordinate inside its tolerance, the
    rest of the four arrays exactly 0, and the two passes' adjoint identity ubar . xdot = sum gradient . tangent inside the sum of the
    two sides' tolerances.  The 3.6e-9 that test_gpu_jvp_class_limits reported for this identity is a mismatch / bound with the bound
    1e-8 (|ubar| |xdot| + |g| |thetadot|): a relative mismatch of 3.6e-17, which is what is measured here (4e-17 .. 7e-17) - both
    passes are at float64 level and no digits are lost on either side."""
    s = all_solved(device_assembly, variant)
    ub, ts, out = _shape_run(s, mode)
    _assert_all_ok(out, N)
    w = _compare(s.ma, s.g, s.p, s.b, s.pos, out, ub, ts, variant, mode)
    print("entrywise %s/%s/%s: %d components, worst error / tolerance: flow %.4f, similarity %.4f, xdot %.4f; adjoint identity "
          "worst mismatch / bound %.4f, relative to |ubar| |xdot| + |g| |thetadot| %.3e (test_gpu_jvp_class_limits: 3.6e-9 x 1e-8)"
          % (mode, variant, "device" if device_assembly else "host", w["n"], w["flow"], w["sim"], w["xdot"], w["adjoint"], w["adjoint_rel"]))
    assert w["n"] == N and set(w["status"].values()) == {BL.OK}
    assert max(w["flow"], w["sim"], w["xdot"], w["adjoint"]) <= 1.0
    assert s.b.spin_timeouts() == 0


# ------------------------------------------------------------------------------------------------------------------ 4. bounds
@pytest.mark.parametrize("name", ["packed_24_32", "block_m"])
def test_components_at_the_bound(lfr_lib, name):
    """the components with a coordinate at +-1, the rounding-sensitive ones set aside: Gauss-Newton and fallback mode for all of them,
    the exact mode for those whose H the reference factors (the others: status 2 and zeros on both sides); a status-3 component of the
    fallback mode against the Gauss-Newton reference; bound coordinates exact zeros; the counts those of the CPU test"""
    ma, _, sensitive = LC.reference(name)
    g, p, b, _, pos = solved(name)
    at_bound = LC.bound_mask(pos)
    comp = p.labels()[2]
    which = np.setdiff1d(np.unique(comp[at_bound.any(axis=1)]), sensitive).tolist()
    ub, ts = _ubar(g.n_nodes, 3).cpu().numpy(), _tangents(ma, 33)
    selected, factored = BOUND_COUNTS[name]
    assert len(which) == selected
    for mode in BL.MODES:
        out = _gpu(b, ub, ts, mode)
        w = _compare(ma, g, p, b, pos, out, ub, ts, "ceres1", mode, which)
        st = list(w["status"].values())
        print("bounds %s %s: %d components (%d status 0, %d status 3, %d status 2), worst error / tolerance: flow %.4f, similarity %.4f, "
              "xdot %.4f, adjoint %.4f" % (name, mode, len(st), st.count(BL.OK), st.count(BL.FELL_BACK), st.count(BL.INDEFINITE),
                                           w["flow"], w["sim"], w["xdot"], w["adjoint"]))
        want = {BL.EXACT: (factored, 0, selected - factored), BL.GAUSS_NEWTON: (selected, 0, 0), BL.FALLBACK: (factored, selected - factored, 0)}[mode]
        assert (st.count(BL.OK), st.count(BL.FELL_BACK), st.count(BL.INDEFINITE)) == want
        assert max(w["flow"], w["sim"], w["xdot"], w["adjoint"]) <= 1.0
        assert out["bst"]["n_bound_coordinates"] == out["jst"]["n_bound_coordinates"] == int(at_bound.sum()) >= 1
        assert not out["xdot"][np.abs(pos) >= 1.0].any()
    assert b.spin_timeouts() == 0


# --------------------------------------------------------------------------------------------------------------- 5. placement
@pytest.mark.parametrize("mode", [BL.EXACT, BL.GAUSS_NEWTON])
def test_every_entry_wherever_the_shape_is_placed(lfr_lib, mode):
    """the same per-entry check with every shape alone in its batch and in the batch that holds every shape twice (among the
    others: the test above): a full last slot that leaked into its neighbour would show here far below the normwise 1e-8"""
    worst = dict(flow=0.0, sim=0.0, xdot=0.0, adjoint=0.0)
    for name in CL.NAMES:
        o = alone_solved(name)
        ub, ts, out = _shape_run(o, mode)
        _assert_all_ok(out, 1)
        w = _compare(o.ma, o.g, o.p, o.b, o.pos, out, ub, ts, "ceres1", mode)
        assert w["n"] == 1, name
        for k in worst:
            worst[k] = max(worst[k], w[k])
            assert w[k] <= 1.0, (name, k, w[k])
    t0, t1 = _twice()
    ub, ts, out = _shape_run(t0, mode, [t0, t1])
    _assert_all_ok(out, 2 * N)
    w = _compare(t0.ma, t0.g, t0.p, t0.b, t0.pos, out, ub, ts, "ceres1", mode)
    print("placement %s: alone worst error / tolerance flow %.4f, similarity %.4f, xdot %.4f, adjoint %.4f; twice %.4f, %.4f, %.4f, %.4f"
          % (mode, worst["flow"], worst["sim"], worst["xdot"], worst["adjoint"], w["flow"], w["sim"], w["xdot"], w["adjoint"]))
    assert w["n"] == 2 * N and max(w["flow"], w["sim"], w["xdot"], w["adjoint"]) <= 1.0
