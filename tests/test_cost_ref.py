"""The extended-precision objective of tests/cost_ref.py against the two fp64 evaluators the project has (backward_ref's torch cost,
the C oracle's final_cost), the measurement behind GAMMA_CPU_MEASURED, and the proof that the tolerance tests/test_gpu_final_cost.py
works with tells a right final_cost from a wrong one: the cost of the iterate before the last accepted step, of a rejected or
discarded candidate, of the other Tukey variant, of the component less one edge.  No GPU."""
import numpy as np
import pytest
import torch

import backward_ref as BR
import class_limit_cases as CL
import cost_ref as CR
import lfr_oracle as O
import lm_decision_cases as LC
from lfr_amd import synthetic
from test_oracle_kat import CASES as KAT_CASES

TERM_FAILURE = 2
MAX_TRACED = 6                 # components per lm_decision_cases case whose trajectory is traced (one oracle run each)
_inputs = None


def _has_inter(comps):
    return any((ed.kind == CR.KIND_INTER).any() for _, ed in comps.values())


def inputs():
    """[(label, variant, MatchArrays, oracle result, {component: (variable nodes, Edges)})]: every shape of class_limit_cases, every
    case of lm_decision_cases, test_oracle_kat's `outliers` and `bounds`; in both Tukey variants where inter-track edges exist"""
    global _inputs
    if _inputs is None:
        _inputs = []
        graphs = [("class_limits", CL.all_shapes()[0], None)]
        graphs += [("lm/" + n, LC.reference(n)[0], LC.reference(n)[1]) for n in LC.CASES]
        graphs += [("kat/" + n, synthetic.generate(**KAT_CASES[n]), None) for n in ("outliers", "bounds")]
        for label, ma, ref in graphs:
            if ref is None:
                ref = O.run(ma, n_threads=4)
                assert ref["rc"] == 0
            comps = CR.oracle_components(ma, ref)
            assert sorted(comps) == np.nonzero(ref["comp_nvar"] > 0)[0].tolist()
            _inputs.append((label, "ceres1", ma, ref, comps))
            if _has_inter(comps):
                ref2 = O.run(ma, n_threads=4, tukey_variant="ceres2")
                assert ref2["rc"] == 0 and (ref2["comp"] == ref["comp"]).all()
                _inputs.append((label, "ceres2", ma, ref2, comps))
    return _inputs


def _torch_cost(ed, x, variant):
    cp = BR.Component(ed.nv, list(zip(ed.src.tolist(), ed.dst.tolist(), ed.w.astype(np.float64), ed.kind.tolist(),
                                      ed.flow.astype(np.float64).reshape(-1, 18))), variant)
    return float(cp.cost(x))


def test_both_variants_are_covered():
    labels = [(l, v) for l, v, _, _, _ in inputs()]
    assert ("class_limits", "ceres2") in labels and ("kat/outliers", "ceres2") in labels          # (the two-root shape; the wrong matches)
    assert len(labels) >= 2 + len(LC.CASES) + 2


def test_fp64_evaluators_agree_and_gamma_is_as_recorded():
    """backward_ref.Component.cost and the C oracle's final_cost, at the oracle's positions, within GAMMA_CPU_MEASURED units of
    2^-53 (S_c + E_c cost_c) of the longdouble value on every component; the largest figure is the constant's provenance"""
    worst = {"oracle": (0.0, None), "torch": (0.0, None)}
    n = 0
    for label, variant, ma, ref, comps in inputs():
        w_in = {"oracle": 0.0, "torch": 0.0}
        for c, (var_nodes, ed) in comps.items():
            oi = ref["infos"][c]
            assert oi["termination"] != TERM_FAILURE, (label, c)
            assert ed.nv == ref["comp_nvar"][c] and len(ed) == ref["comp_nedges"][c], (label, c)
            x = ref["positions"][var_nodes]
            k = CR.evaluate(ed, x, variant)
            unit = k.tol(gamma=1.0)
            for who, value in (("oracle", oi["final_cost"]), ("torch", _torch_cost(ed, x, variant))):
                err = abs(float(CR.LD(value) - k.cost)) / unit
                assert err <= CR.GAMMA_CPU_MEASURED, (label, variant, c, who, err, value, k.cost64)
                w_in[who] = max(w_in[who], err)
                if err > worst[who][0]:
                    worst[who] = (err, "%s/%s component %d (%d rows, %d edges)" % (label, variant, c, 2 * ed.nv, len(ed)))
            n += 1
        print("%-20s %-6s %4d components: largest error / (2^-53 (S + E cost)): oracle %.4f, torch %.4f"
              % (label, variant, len(comps), w_in["oracle"], w_in["torch"]))
    measured = max(worst["oracle"][0], worst["torch"][0])
    print("GAMMA_CPU_MEASURED: measured %.4f over %d components (oracle %.4f on %s; torch %.4f on %s), recorded %.4g, GAMMA_GPU %.4g"
          % (measured, n, *worst["oracle"], *worst["torch"], CR.GAMMA_CPU_MEASURED, CR.GAMMA_GPU))
    assert 0.5 * CR.GAMMA_CPU_MEASURED <= measured <= CR.GAMMA_CPU_MEASURED          # (the constant stays a measurement)
    assert CR.GAMMA_GPU == 8 * CR.GAMMA_CPU_MEASURED


def test_cost_never_rises_above_the_start():
    """LM accepts decreases only and starts at the origin: F_c(oracle positions) <= F_c(0) + tol_c, and the oracle's initial_cost is
    F_c(0)"""
    for label, variant, ma, ref, comps in inputs():
        for c, (var_nodes, ed) in comps.items():
            k, k0 = CR.evaluate(ed, ref["positions"][var_nodes], variant), CR.evaluate(ed, np.zeros((ed.nv, 2)), variant)
            assert k.cost <= k0.cost + k.tol(), (label, variant, c)
            assert abs(ref["infos"][c]["initial_cost"] - k0.cost64) <= k0.tol(), (label, variant, c)


def _traced(name):
    """components of a case to trace: those that rejected a step first, then those that contracted one, then the others"""
    _, ref, _ = LC.reference(name)
    oi = ref["infos"]
    solved = np.nonzero(ref["comp_nvar"] > 0)[0]
    it = oi["iterations"][solved]
    rejected = solved[oi["n_successful"][solved] < it - 1]
    contracted = solved[oi["n_ls_evals"][solved] > it]
    order = list(rejected) + [c for c in contracted if c not in set(rejected)]
    order += [c for c in solved if c not in set(order)]
    return [int(c) for c in order[:MAX_TRACED]]


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_tolerance_tells_the_final_cost_from_the_other_costs_of_the_trajectory(name):
    """the oracle's trace (it, cost, cost_cand, rel, radius, alpha, gmax, flags: 1 accepted, 2 rejected, 8 / 16 candidate discarded by
    the parameter / function tolerance): the cost of the iterate before the last accepted step, of every rejected candidate and of
    the candidate the stop discarded lie more than 100 tol_c from final_cost - for at least 90 % of the traced components that
    have such a cost"""
    ma, ref, _ = LC.reference(name)
    comps = CR.oracle_components(ma, ref)
    count = {"previous": [0, 0], "rejected": [0, 0], "discarded": [0, 0]}
    for c in _traced(name):
        tr = O.run(ma, n_threads=4, trace_comp=c)
        assert tr["rc"] == 0 and np.array_equal(tr["positions"], ref["positions"])
        rows = tr["trace"]
        flags = rows[:, 7].astype(int)
        final = ref["infos"][c]["final_cost"]
        var_nodes, ed = comps[c]
        k = CR.evaluate(ed, ref["positions"][var_nodes])
        tol = k.tol()
        accepted = rows[flags == 1, 1]
        assert accepted[-1] == final and abs(final - k.cost64) <= tol
        other = {"previous": accepted[-2:-1], "rejected": rows[flags == 2, 2], "discarded": rows[(flags == 8) | (flags == 16), 2]}
        for what, costs in other.items():
            if len(costs):
                count[what][1] += 1
                count[what][0] += int((np.abs(costs - final) > 100 * tol).all())
        print("%s component %d: final cost %.17g, tol_c %.3e; nearest other cost, in tol_c: %s"
              % (name, c, final, tol, ", ".join("%s %.3e" % (w, np.abs(v - final).min() / tol) for w, v in other.items() if len(v))))
    print("%s: separated by more than 100 tol_c: %s" % (name, ", ".join("%s %d of %d" % (w, a, b) for w, (a, b) in count.items())))
    assert count["previous"][1] >= 1 and count["discarded"][1] >= 1
    if LC.REQUIRED[name].get("rejected"):
        assert count["rejected"][1] >= LC.REQUIRED[name]["rejected"] or count["rejected"][1] == MAX_TRACED
    for what, (a, b) in count.items():
        assert a >= 0.9 * b, (what, a, b)


def test_tolerance_tells_the_tukey_variants_apart():
    n = 0
    for label, variant, ma, ref, comps in inputs():
        if variant != "ceres1":
            continue
        for c, (var_nodes, ed) in comps.items():
            inter = ed.kind == CR.KIND_INTER
            k1, k2 = (CR.evaluate(ed, ref["positions"][var_nodes], v) for v in ("ceres1", "ceres2"))
            if not inter.any() or not k1.terms[inter].any():
                assert k1.cost == k2.cost
                continue
            assert float(k2.cost - k1.cost) == pytest.approx(float(k1.terms[inter].sum()), rel=1e-15)      # (twice the inter-track terms)
            assert abs(float(k2.cost - k1.cost)) > 100 * max(k1.tol(), k2.tol()), (label, c)
            n += 1
    print("components with inter-track edges whose two variants' costs are told apart: %d" % n)
    assert n >= 2


def test_tolerance_sees_every_single_edge():
    """the cost of a component less any one edge whose term is not zero lies more than tol_c from the cost"""
    n_edges = n_zero = 0
    nearest = np.inf
    for label, variant, ma, ref, comps in inputs():
        for c, (var_nodes, ed) in comps.items():
            x = ref["positions"][var_nodes]
            k = CR.evaluate(ed, x, variant)
            tol = k.tol()
            nz = np.nonzero(k.terms)[0]
            n_zero += len(ed) - len(nz)
            n_edges += len(nz)
            assert (np.abs(k.terms[nz]) > tol).all(), (label, variant, c, float(np.abs(k.terms[nz]).min()), tol)
            nearest = min(nearest, float(np.abs(k.terms[nz]).min()) / tol)
            if len(ed) <= 64:                               # (the sum less a term, evaluated as such)
                for e in nz:
                    assert abs(float(CR.evaluate(ed.without(e), x, variant).cost - k.cost)) > tol, (label, variant, c, e)
    print("%d edges with a nonzero term (%d with a zero term), the smallest term is %.3e tol_c" % (n_edges, n_zero, nearest))
    assert n_edges > 10000


def test_the_gpu_tests_inputs_lie_where_the_tolerance_is_valid():
    """cost_ref, "What S_c leaves out": on every input tests/test_gpu_final_cost.py holds the kernels to tol_c, the worst case of rounding
    1 + s / b is within tol_c for every component (at the oracle's positions; the GPU test asserts the same at the kernels')"""
    from test_gpu_packed_rounds import HARD
    graphs = [(label, ma, ref) for label, variant, ma, ref, _ in inputs() if variant == "ceres1" and not label.startswith("kat/")]
    graphs += [(label, synthetic.generate(**kw), None) for label, kw in (("hard", HARD), ("tukey", CR.TUKEY_GRAPH), ("bounds", CR.BOUNDS_GRAPH))]
    for label, ma, ref in graphs:
        if ref is None:
            ref = O.run(ma, n_threads=4)
            assert ref["rc"] == 0
        worst = 0.0
        for c, (var_nodes, ed) in CR.oracle_components(ma, ref).items():
            k = CR.evaluate(ed, ref["positions"][var_nodes])
            worst = max(worst, k.arg_rounding / k.tol())
        print("%-16s worst case of rounding 1 + s / b: %.3f tol_c" % (label, worst))
        assert worst <= 1.0, label
