"""tests/evaluate_ref.py pinned without a GPU: its gradient against central differences of tests/cost_ref.py's objective, the kink
semantics of the interpolant's derivative on hand-made two-node cases, the measurements behind GAMMA_GRAD_CPU / GAMMA_RES_CPU /
GAMMA_W_CPU (the method of tests/test_cost_ref.py for GAMMA_CPU_MEASURED), and the validity of the cost tolerance on every input and
position set tests/test_gpu_evaluate.py uses."""
import numpy as np
import pytest

import backward_ref as BR
import class_limit_cases as CL
import cost_ref as CR
import evaluate_ref as ER
import lfr_oracle as O
from lfr_amd import synthetic

LD = CR.LD
_inputs = None


def inputs():
    """[(label, variant, {component: (variable nodes, Edges)}, {"a": oracle positions, "b": positions_b})]"""
    global _inputs
    if _inputs is None:
        _inputs = []
        for label, ma, variants in (("class_limits", CL.all_shapes()[0], ("ceres1",)), ("tukey", synthetic.generate(**CR.TUKEY_GRAPH), ("ceres1", "ceres2")),
                                    ("bounds", synthetic.generate(**CR.BOUNDS_GRAPH), ("ceres1",))):
            for variant in variants:
                ref = O.run(ma, n_threads=4, tukey_variant=variant)
                assert ref["rc"] == 0
                comps = CR.oracle_components(ma, ref)
                _inputs.append((label, variant, comps, {"a": ref["positions"], "b": ER.positions_b(comps, len(ref["positions"]))}))
    return _inputs


def _single(x, flow, kind=CR.KIND_INTRA, w=1.0, src_variable=True):
    """one edge between a variable node at x and a constant node"""
    ed = CR.Edges(1, np.array([0 if src_variable else -1]), np.array([-1 if src_variable else 0]), np.array([w], LD), np.array([kind]),
                  np.asarray(flow, np.float32).astype(LD).reshape(1, 9, 2), np.array([0]))
    return ER.evaluate(ed, np.asarray(x, np.float64))


# --------------------------------------------------------------------------------------------- 1. gradient against differences
def test_gradient_agrees_with_central_differences():
    """longdouble central differences of cost_ref.evaluate, step 1e-9, at random positions in [-1.2, 1.2] (clamped and interior
    arguments) that keep 1e-4 away from the kinks +-0.5 and 1e-3 a^2 from Tukey's saturation radius.  The bound: truncation
    h^2 |F'''| / 6 <= 1e-18 * 1e6 and rounding 2^-63 |F| / h <= 1e-10 |F|, F <= 100: 1e-7 is above both and many orders below a wrong
    term (the gradients are O(0.1 .. 10))"""
    h = LD(1e-9)
    n = n_inter = 0
    for label, variant, comps, sets in inputs():
        rng = np.random.Generator(np.random.PCG64(515))
        todo = [(c, None) for c in sorted(comps)] + [(c, sets["a"]) for c in sorted(comps) if (comps[c][1].kind == CR.KIND_INTER).any()]
        if label == "tukey":                                # (the graph's wrong matches are saturated at either set: hand-made ones are not)
            made = {-1 - k: _tukey_at_work(600 + k) for k in range(4)}
            comps = {**comps, **{c: (np.arange(2), ed) for c, (ed, _) in made.items()}}
            todo += [(c, x) for c, (_, x) in made.items()]
        for c, at in todo:
            var_nodes, ed = comps[c]
            if ed.nv > 17 or (label != "tukey" and n > 40 and ed.nv > 4):
                continue
            x = rng.uniform(-1.2, 1.2, size=(ed.nv, 2)) if at is None else at[var_nodes].copy()
            x[np.abs(np.abs(x) - 0.5) < 1e-4] += 1e-3
            ev = ER.evaluate(ed, x, variant)
            s = (ev.r * ev.r).sum(1)
            inter = ed.kind == CR.KIND_INTER
            if (np.abs(s[inter] - CR.TUKEY_A2) < 1e-3 * CR.TUKEY_A2).any():
                continue
            xl = x.astype(LD)
            for i in range(ed.nv):
                for k in range(2):
                    xp, xm = xl.copy(), xl.copy()
                    xp[i, k] += h
                    xm[i, k] -= h
                    fd = (CR.evaluate(ed, xp, variant).cost - CR.evaluate(ed, xm, variant).cost) / (2 * h)
                    assert abs(float(fd - ev.grad[i, k])) <= 1e-7, (label, variant, c, i, k, float(fd), float(ev.grad[i, k]))
            n += 1
            n_inter += int(inter.any() and (s[inter] < CR.TUKEY_A2).any())
    print("%d components differenced, %d with an unsaturated inter-track edge" % (n, n_inter))
    assert n >= 20 and n_inter >= 2


def _tukey_at_work(seed):
    """two variable nodes and a constant one joined by six inter-track edges whose flows are the true offsets plus noise well inside
    Tukey's radius 0.0625: every weight is strictly between 0 and its value at a zero residual"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(-0.3, 0.3, size=(3, 2))
    x[2] = 0.0
    src, dst = np.array([0, 1, 0, -1, 1, -1]), np.array([1, 0, -1, 0, -1, 1])
    flow = (x[dst] - x[src])[:, None, :] + rng.normal(0.0, 0.01, size=(6, 9, 2))
    ed = CR.Edges(2, src, dst, rng.uniform(0.8, 1.0, size=6).astype(np.float32).astype(LD), np.full(6, CR.KIND_INTER),
                  flow.astype(np.float32).astype(LD), np.arange(6))
    return ed, x[:2]


# ------------------------------------------------------------------------------------------------------- 2. kink semantics
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_derivative_is_kept_at_the_kink_and_zero_outside(axis, sign):
    """a flow that is linear in one axis, f_0 = 2 alpha t: d f_0 / dt = 2 alpha on [-0.5, 0.5] INCLUSIVE, 0 outside.  One Cauchy edge
    from the variable node at x to a constant node: r = -x - f, dF/dx = -c P^T r, c = w / (1 + s / b)"""
    alpha = 0.125
    t = (np.arange(3) - 1.0)
    flow = np.zeros((3, 3, 2))
    if axis == 0:
        flow[:, :, 0] = alpha * t[:, None]
    else:
        flow[:, :, 0] = alpha * t[None, :]
    b = 0.0625
    for off, slope in ((0.0, 2 * alpha), (2.0 ** -30, 0.0), (-0.25, 2 * alpha), (0.25, 0.0)):
        x = np.zeros(2)
        x[axis] = sign * (0.5 + off)
        ev = _single(x, flow.reshape(9, 2))
        f0 = 2 * alpha * sign * min(0.5 + off, 0.5)
        r = np.array([-x[0] - f0, -x[1]])
        c = 1.0 / (1.0 + (r * r).sum() / b)
        want = -c * r                     # dF/dx_src = -c P^T r = -c (r + slope r_0 e_axis)
        want[axis] -= c * slope * r[0]
        assert np.allclose(ev.r.astype(np.float64)[0], r, rtol=0, atol=1e-15), (off, ev.r, r)
        assert np.allclose(ev.grad.astype(np.float64)[0], want, rtol=1e-14, atol=1e-16), (off, ev.grad, want)
        assert abs(float(ev.rho1[0]) - c) <= 1e-15
        # the same edge seen from its destination: no P
        evd = _single(x, flow.reshape(9, 2), src_variable=False)
        rd = np.array([x[0] - flow[1, 1, 0], x[1]])
        cd = 1.0 / (1.0 + (rd * rd).sum() / b)
        assert np.allclose(evd.grad.astype(np.float64)[0], cd * rd, rtol=1e-14, atol=1e-16)


def test_saturated_tukey_edge_has_weight_zero_and_no_gradient():
    ev = _single([0.3, 0.0], np.zeros((9, 2)), kind=CR.KIND_INTER)
    assert float(ev.rho1[0]) == 0.0 and not ev.grad.any() and float(ev.w_unit[0]) == 0.0
    ev = _single([0.03, 0.0], np.zeros((9, 2)), kind=CR.KIND_INTER)
    v = 1.0 - 0.03 ** 2 / 0.0625 ** 2
    assert abs(float(ev.rho1[0]) - 0.5 * v * v) <= 1e-15 and abs(float(ev.grad[0, 0]) - 0.5 * v * v * 0.03) <= 1e-15


# -------------------------------------------------------------------------------------------------- 3. the measured constants
def _ratio(err, unit):
    err, unit = np.asarray(err, LD), np.asarray(unit, LD)
    assert (err[unit == 0] == 0).all()                       # (a saturated Tukey edge: weight 0 exactly, on every evaluator)
    return float((err[unit > 0] / unit[unit > 0]).max(initial=0.0))


def test_fp64_evaluators_agree_and_the_gammas_are_as_recorded():
    worst = {"grad": 0.0, "grad_torch": 0.0, "res": 0.0, "w": 0.0}
    n = 0
    for label, variant, comps, sets in inputs():
        w_in = dict.fromkeys(worst, 0.0)
        for which, pos in sets.items():
            for c, (var_nodes, ed) in comps.items():
                x = pos[var_nodes]
                ev, e64 = ER.evaluate(ed, x, variant), ER.evaluate(ed, x, variant, dtype=np.float64)
                cp = BR.Component(ed.nv, list(zip(ed.src.tolist(), ed.dst.tolist(), ed.w.astype(np.float64), ed.kind.tolist(),
                                                  ed.flow.astype(np.float64).reshape(-1, 18))), variant)
                gt = cp.grad(x).reshape(-1, 2)
                for key, err, unit in (("grad", np.abs(e64.grad.astype(LD) - ev.grad), ev.g_unit), ("grad_torch", np.abs(gt.astype(LD) - ev.grad), ev.g_unit),
                                       ("res", np.abs(e64.r.astype(LD) - ev.r), ev.r_unit), ("w", np.abs(e64.rho1.astype(LD) - ev.rho1), ev.w_unit)):
                    w_in[key] = max(w_in[key], _ratio(err, unit))
                n += 1
        print("%-14s %-6s largest error / unit: gradient %.4f (numpy) %.4f (torch), residual %.4f, weight %.4f"
              % (label, variant, w_in["grad"], w_in["grad_torch"], w_in["res"], w_in["w"]))
        for key in worst:
            worst[key] = max(worst[key], w_in[key])
    measured = {"GAMMA_GRAD_CPU": max(worst["grad"], worst["grad_torch"]), "GAMMA_RES_CPU": worst["res"], "GAMMA_W_CPU": worst["w"]}
    for name, m in measured.items():
        print("%s: measured %.4f over %d component evaluations, recorded %.4g, on the GPU %d x" % (name, m, n, getattr(ER, name), ER.GPU_FACTOR))
    for name, m in measured.items():
        assert 0.5 * getattr(ER, name) <= m <= getattr(ER, name), (name, m)          # (the constants stay measurements)
    assert ER.GPU_FACTOR == 8 and CR.GAMMA_GPU == ER.GPU_FACTOR * CR.GAMMA_CPU_MEASURED


# ------------------------------------------------------------------------------------------------------- 4. input validity
def test_the_gpu_tests_inputs_lie_where_the_cost_tolerance_is_valid():
    """cost_ref, "What S_c leaves out": the worst case of rounding 1 + s / b is within tol_c for every component of every input at both
    position sets (the GPU test asserts the same at the kernels' positions)"""
    for label, variant, comps, sets in inputs():
        for which, pos in sets.items():
            worst = 0.0
            for c, (var_nodes, ed) in comps.items():
                k = CR.evaluate(ed, pos[var_nodes], variant)
                worst = max(worst, k.arg_rounding / k.tol())
            print("%-14s %-6s set (%s): worst case of rounding 1 + s / b: %.3f tol_c" % (label, variant, which, worst))
            assert worst <= 1.0, (label, variant, which)


def test_position_set_b_holds_clamped_kink_and_interior_arguments():
    for label, variant, comps, sets in inputs():
        pos = sets["b"]
        for c, (var_nodes, ed) in comps.items():
            assert tuple(pos[var_nodes[0]]) == (0.5, -0.5)
            if len(var_nodes) > 1:
                assert tuple(pos[var_nodes[1]]) == (0.0, 0.75)
        assert (np.abs(pos) > 1.0).any() and (np.abs(pos) < 0.5).any() and np.abs(pos).max() <= 1.2
