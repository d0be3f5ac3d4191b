"""tests/backward_ld_ref.py pinned without a GPU: its lambda, flow gradients, similarity gradients and xdot entry by entry against
backward_ref, backward_gn_ref, hessian_fallback_ref and jvp_ref (torch autograd sweeps, numpy Cholesky) and against its own float64
restatement, in the three Hessian modes; the measurements behind GAMMA_BWD_FLOW_CPU / GAMMA_BWD_SIM_CPU / GAMMA_JVP_CPU (the rule of
tests/test_hessian_product_ref.py); the conditions under which tests/test_gpu_backward_entrywise.py compares every component; and the
power of the per-entry criterion over the normwise one, 1e-8 |ref|_2 + 1e-14 per component, on three defects planted in the float64
evaluator's output.

Inputs: class_limit_cases.all_shapes() at the oracle's positions in both Tukey variants; lm_decision_cases' packed_24_32 and block_m,
their components with a coordinate at the bound that are not rounding-sensitive.  ubar ~ N(0, 1) from seed 0 over the graph's nodes,
the tangents N(0, 1) from seed 41 in the match layout."""
import numpy as np
import pytest

import backward_gn_ref as GN
import backward_ld_ref as BL
import backward_ref as BR
import class_limit_cases as CL
import cost_ref as CR
import hessian_fallback_ref as FR
import jvp_ref as JR
import lfr_oracle as O
import lm_decision_cases as LC

LD = CR.LD
BOUND_CASES = ("packed_24_32", "block_m")
# components with a coordinate at the bound, not rounding-sensitive, at the oracle's positions: (selected, exact H factors in longdouble)
BOUND_COUNTS = {"packed_24_32": (37, 26), "block_m": (34, 11)}
_inputs = {}
_results = {}


def inputs(label, variant="ceres1"):
    """(label, variant, {component: (variable nodes, Edges)}, positions, ubar, tangents, {component: name}): computed once, left unchanged"""
    if (label, variant) not in _inputs:
        if label == "class_limits":
            ma, feats = CL.all_shapes()
            ref = O.run(ma, n_threads=4, tukey_variant=variant)
            assert ref["rc"] == 0
            comps = CR.oracle_components(ma, ref)
            names = {c: name for name, c in CL.components_of(feats, ref["node_feat"], ref["comp"]).items()}
            assert sorted(names) == sorted(comps) and len(comps) == 33
        else:
            assert variant == "ceres1"
            ma, ref, sensitive = LC.reference(label)
            which = np.setdiff1d(LC.components_at_bound(ref), sensitive).tolist()
            comps = CR.oracle_components(ma, ref, which=set(which))
            assert sorted(comps) == which
            names = {c: "%s/%d" % (label, c) for c in comps}
        n, m = len(ref["positions"]), len(ma.sim)
        rng = np.random.default_rng(41)
        ts = (rng.standard_normal((m, 18)), rng.standard_normal((m, 18)), rng.standard_normal(m))
        _inputs[(label, variant)] = (comps, ref["positions"], np.random.default_rng(0).standard_normal((n, 2)), ts, names)
    return _inputs[(label, variant)]


def ALL_INPUTS():
    return [("class_limits", "ceres1"), ("class_limits", "ceres2")] + [(name, "ceres1") for name in BOUND_CASES]


def _component(ed, variant):
    return BR.Component(ed.nv, list(zip(ed.src.tolist(), ed.dst.tolist(), ed.w.astype(np.float64), ed.kind.tolist(),
                                        ed.flow.astype(np.float64).reshape(-1, 18))), variant)


def _ratio(err, unit):
    err, unit = np.asarray(err, LD).reshape(-1), np.asarray(unit, LD).reshape(-1)
    assert (err[unit == 0] == 0).all()                       # (bound coordinates, basis values that are exactly 0, status 2: exact)
    return float((err[unit > 0] / unit[unit > 0]).max(initial=0.0))


def results(label, variant, mode):
    """per component of an input: the longdouble result, the float64 restatement's and the torch reference's, backward and jvp"""
    key = (label, variant, mode)
    if key in _results:
        return _results[key]
    comps, pos, ubar, ts, names = inputs(label, variant)
    out = {}
    for c, (var_nodes, ed) in comps.items():
        x, ub = pos[var_nodes], ubar[var_nodes]
        fdot, sdot = BL.edge_tangents(ed, *ts)
        ref, r64 = BL.Component(ed, x, variant, mode), BL.Component(ed, x, variant, mode, dtype=np.float64)
        cp = _component(ed, variant)
        xf, uf = x.reshape(-1), ub.reshape(-1)
        if mode == BL.EXACT:
            gf, gw, st = cp.backward(xf, uf)
            xdot, sj = JR.jvp(cp, xf, fdot, sdot)
        elif mode == BL.GAUSS_NEWTON:
            gf, gw, st = GN.Component.of(cp).backward(xf, uf)
            xdot, sj = JR.jvp(cp, xf, fdot, sdot, gauss_newton=True)
        else:
            gf, gw, st, _ = FR.backward(cp, xf, uf)
            xdot, sj, _ = FR.jvp(cp, xf, fdot, sdot)
        # lambda of the torch reference: its dense matrix through its numpy Cholesky solve (backward() does not return it)
        lam = np.zeros(2 * ed.nv)
        if st != BL.INDEFINITE:
            gn = mode == BL.GAUSS_NEWTON or st == BL.FELL_BACK
            H = (GN.Component.of(cp) if gn else cp).hessian(xf)
            fr = cp.free(xf)
            lam, _ = JR._solve(H, uf.copy(), fr)
        out[c] = dict(ed=ed, ref_b=ref.backward(ub), ref_j=ref.jvp(fdot, sdot), r64_b=r64.backward(ub), r64_j=r64.jvp(fdot, sdot),
                      torch=(gf.reshape(-1, 9, 2), gw, lam.reshape(-1, 2), xdot.reshape(-1, 2), st, sj), ld=ref)
    _results[key] = out
    return out


# ------------------------------------------------------------------------------------ 1. the pin and the measured constants
def test_reference_agrees_with_the_torch_references_and_the_gammas_are_as_recorded():
    worst = {}
    n = 0
    for label, variant in ALL_INPUTS():
        for mode in BL.MODES:
            w_in = dict.fromkeys(("flow", "flow_torch", "sim", "sim_torch", "lam", "lam_torch", "xdot", "xdot_torch"), 0.0)
            for c, res in results(label, variant, mode).items():
                rb, rj, fb, fj = res["ref_b"], res["ref_j"], res["r64_b"], res["r64_j"]
                gf, gw, lam, xdot, st, sj = res["torch"]
                assert rb.status == rj.status == fb.status == fj.status == st == sj, (label, variant, mode, c)
                for key, got, want, unit in (("flow", fb.gflow, rb.gflow, rb.gflow_unit), ("flow_torch", gf, rb.gflow, rb.gflow_unit),
                                             ("sim", fb.gsim, rb.gsim, rb.gsim_unit), ("sim_torch", gw, rb.gsim, rb.gsim_unit),
                                             ("lam", fb.lam, rb.lam, rb.lam_unit), ("lam_torch", lam, rb.lam, rb.lam_unit),
                                             ("xdot", fj.xdot, rj.xdot, rj.xdot_unit), ("xdot_torch", xdot, rj.xdot, rj.xdot_unit)):
                    w_in[key] = max(w_in[key], _ratio(np.abs(np.asarray(got).astype(LD) - want), unit))
                n += 1
            print("%-13s %-6s %-12s largest error / unit: flow %.4f (numpy) %.4f (torch), similarity %.4f %.4f, lambda %.4f %.4f, xdot %.4f %.4f"
                  % ((label, variant, mode) + tuple(w_in[k] for k in ("flow", "flow_torch", "sim", "sim_torch", "lam", "lam_torch", "xdot", "xdot_torch"))))
            for k, v in w_in.items():
                worst[(mode, k)] = max(worst.get((mode, k), 0.0), v)
    per_mode = {name: {mode: max(worst[(mode, k)] for k in keys) for mode in BL.MODES}
                for name, keys in (("GAMMA_BWD_FLOW_CPU", ("flow", "flow_torch")), ("GAMMA_BWD_SIM_CPU", ("sim", "sim_torch")),
                                   ("GAMMA_JVP_CPU", ("lam", "lam_torch", "xdot", "xdot_torch")))}
    for name, by_mode in per_mode.items():
        m = max(by_mode.values())
        print("%s: measured %.4f over %d component results (%s), recorded %.4g, on the GPU %d x"
              % (name, m, n, ", ".join("%s %.4f" % kv for kv in by_mode.items()), getattr(BL, name), BL.GPU_FACTOR))
    for name, by_mode in per_mode.items():
        m = max(by_mode.values())
        assert m <= 2.0 * min(by_mode.values()), name            # (one constant serves the three modes)
        assert 0.5 * getattr(BL, name) <= m <= getattr(BL, name), (name, m)
    assert BL.GPU_FACTOR == 8


# ------------------------------------------------------------------------------------------------- 2. coverage conditions
@pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
def test_every_shape_is_differentiated_in_every_mode(variant):
    """the 33 shapes: status 0 in the three modes, no coordinate at the bound, outputs that are not zero - the GPU test compares all"""
    comps, pos, _, _, names = inputs("class_limits", variant)
    assert sorted(names.values()) == sorted(CL.NAMES)
    for mode in BL.MODES:
        for c, res in results("class_limits", variant, mode).items():
            rb, rj, ed = res["ref_b"], res["ref_j"], res["ed"]
            assert (2 * ed.nv, len(ed)) == (CL.SHAPES[names[c]]["rows"], CL.SHAPES[names[c]]["edges"]), names[c]
            assert rb.status == rj.status == BL.OK and rb.n_bound == 0 and (np.abs(pos[comps[c][0]]) < 1).all(), (names[c], mode)
            assert rb.gflow.any() and rb.gsim.any() and rj.xdot.all() and (rb.gflow_unit > 0).any() and (rj.xdot_unit > 0).all(), (names[c], mode)


@pytest.mark.parametrize("name", BOUND_CASES)
def test_components_at_the_bound_are_compared_as_counted(name):
    """the Gauss-Newton mode leaves none out, the exact mode those whose H the longdouble Cholesky rejects, the fallback mode takes
    the Gauss-Newton matrix for exactly those; bound coordinates read exact zeros with unit 0"""
    comps, pos, _, _, _ = inputs(name)
    selected, factored = BOUND_COUNTS[name]
    st = {mode: {c: r["ref_b"].status for c, r in results(name, "ceres1", mode).items()} for mode in BL.MODES}
    print("%s: %d components with a coordinate at the bound, exact mode factors %d" % (name, len(comps), list(st[BL.EXACT].values()).count(BL.OK)))
    assert len(comps) == selected
    assert all(s == BL.OK for s in st[BL.GAUSS_NEWTON].values())
    assert sorted(st[BL.EXACT].values()) == [BL.OK] * factored + [BL.INDEFINITE] * (selected - factored)
    for c in comps:
        assert st[BL.FALLBACK][c] == (BL.OK if st[BL.EXACT][c] == BL.OK else BL.FELL_BACK)
        for mode in BL.MODES:
            res = results(name, "ceres1", mode)[c]
            rb, rj = res["ref_b"], res["ref_j"]
            at = np.abs(pos[comps[c][0]]) >= 1
            assert at.any() and rb.n_bound == int(at.sum())
            for a in (rb.lam, rb.lam_unit, rj.xdot, rj.xdot_unit, rj.b, rj.b_unit):
                assert not a[at].any()
            if rb.status == BL.INDEFINITE:
                assert not rb.gflow.any() and not rb.gsim.any() and not rj.xdot.any()
            elif mode == BL.FALLBACK:                              # the pure mode's numbers, whichever matrix was taken
                pure = results(name, "ceres1", BL.GAUSS_NEWTON if rb.status == BL.FELL_BACK else BL.EXACT)[c]
                assert np.array_equal(rb.gflow, pure["ref_b"].gflow) and np.array_equal(rj.xdot, pure["ref_j"].xdot)


# ------------------------------------------------------------------------------------------------------------- 3. power
def _old_accepts(got, ref):
    """the normwise criterion of tests/test_gpu_backward.py on a component's flow rows and per-match similarity gradients"""
    return np.linalg.norm(got - ref) <= 1e-8 * np.linalg.norm(ref) + 1e-14


def _new_violations(flow, sim, ref):
    """entries outside the per-entry criterion at the GPU tolerance; ref = component_layout of the longdouble result"""
    rf, rs, fu, su, _ = ref
    return (int((np.abs(flow.astype(LD) - rf) > BL.GPU_FACTOR * BL.GAMMA_BWD_FLOW_CPU * fu).sum()),
            int((np.abs(sim.astype(LD) - rs) > BL.GPU_FACTOR * BL.GAMMA_BWD_SIM_CPU * su).sum()))


def test_per_entry_criterion_rejects_what_the_normwise_one_accepts():
    """The float64 evaluator's backward of every shape (exact mode, ceres1) with one defect at a time:
      1. one directed edge's 18-entry row rounded to float32 - every row in turn;
      2. every similarity gradient times (1 + 1e-6), and times (1 + d) with d the relative error the normwise criterion admits on the
         shape's similarity gradients, 0.9e-8 |ref|_2 / |sim part|_2 (2.6e-7 .. 9.2e-7);
      3. lambda's largest coordinate times (1 + 1e-9) before the sweep.
    The normwise criterion accepts 1 for at least 40 % of the rows of every shape, 90 % from k9_full to k98 and every row of the
    complete tracks from k45 on; accepts 2 at 1e-6 exactly where 1e-6 |sim part| stays below its bound (|sim part| / |flow part| is
    0.0098 .. 0.035) and at d on every shape; accepts 3 on every shape.  The per-entry criterion at the GPU's tolerance accepts the
    evaluator and rejects every one of them."""
    comps, pos, ubar, _, names = inputs("class_limits")
    res = results("class_limits", "ceres1", BL.EXACT)
    by_name = {name: c for c, name in names.items()}
    n_rows = n_sim_accepted = 0
    for k, name in enumerate(CL.NAMES):
        c = by_name[name]
        var_nodes, ed = comps[c]
        ref = BL.component_layout(ed, res[c]["ref_b"])
        got = res[c]["r64_b"]
        gf, gs, _, _, _ = BL.component_layout(ed, got)
        rf, rs = ref[0].astype(np.float64), ref[1].astype(np.float64)
        whole = lambda f, s: np.concatenate([f.ravel(), s])
        assert _new_violations(gf, gs, ref) == (0, 0) and _old_accepts(whole(gf, gs), whole(rf, rs)), name
        # 1. a row in float32
        live = np.nonzero(rf.any(1))[0]
        assert len(live) >= len(rf) - 2                          # (a saturated inter-track edge has a zero row: two_roots_8's wrong match)
        g32 = gf.astype(np.float32).astype(np.float64)        # (row e replaced: the squared error changes by that row's alone)
        err2 = ((gf - rf) ** 2).sum() + ((gs - rs) ** 2).sum() - ((gf - rf) ** 2).sum(1) + ((g32 - rf) ** 2).sum(1)
        accepted = np.sqrt(err2) <= 1e-8 * np.linalg.norm(whole(rf, rs)) + 1e-14
        bad = gf.copy()
        bad[live[0]] = g32[live[0]]
        assert accepted[live[0]] == _old_accepts(whole(bad, gs), whole(rf, rs))
        rejected = (np.abs(g32.astype(LD) - ref[0]) > BL.GPU_FACTOR * BL.GAMMA_BWD_FLOW_CPU * ref[2]).any(1)
        assert rejected[live].all(), (name, live[~rejected[live]])
        share = accepted[live].mean()
        n_rows += len(live)
        assert share >= 0.4, name
        if CL.NAMES.index("k9_full") <= k <= CL.NAMES.index("k98"):
            assert share >= 0.9, name
        if name in ("k45", "k46", "k66", "k67", "k97", "k98"):
            assert share == 1.0, name
        # 2. the similarity gradients
        ratio = np.linalg.norm(rs) / np.linalg.norm(rf)
        assert 0.009 <= ratio <= 0.036, name
        admitted = 0.9e-8 * np.linalg.norm(whole(rf, rs)) / np.linalg.norm(rs)
        assert 2.5e-7 <= admitted <= 1e-6
        for d, want in ((1e-6, None if 0.8 * admitted <= 1e-6 <= 1.25 * admitted else admitted >= 1e-6), (admitted, True)):
            bad = gs * (1.0 + d)
            old = bool(_old_accepts(whole(gf, bad), whole(rf, rs)))
            assert want is None or old == want, (name, d)
            n_sim_accepted += old and d == 1e-6
            # (of those that are not zero; not every one: where a match's two directions cancel, the sum's unit exceeds d times the sum)
            assert _new_violations(gf, bad, ref)[1] >= 0.95 * np.count_nonzero(rs) >= 0.8 * len(rs), (name, d)
        # 3. lambda
        lam = got.lam.copy().reshape(-1)
        lam[np.argmax(np.abs(lam))] *= 1.0 + 1e-9
        T = BL.edge_terms(ed, pos[var_nodes], "ceres1", np.float64)
        bf, bs, _, _ = BL.sweep(T, lam)
        bf, bs, _, _, _ = BL.component_layout(ed, BL.Backward(0, lam, bf, bs, None, np.zeros_like(bf), np.zeros_like(bs), 0))
        assert _old_accepts(whole(bf, bs), whole(rf, rs)), name
        assert sum(_new_violations(bf, bs, ref)) >= 18, name
        print("%-18s normwise accepts %5.1f %% of %4d float32 rows; similarity part / flow part %.4f, admits a relative %.2e"
              % (name, 100 * share, len(live), ratio, admitted))
    print("%d rows rounded in turn, the per-entry criterion rejected every one; similarities x (1 + 1e-6) accepted normwise on %d shapes"
          % (n_rows, n_sim_accepted))
    assert n_sim_accepted >= 1
