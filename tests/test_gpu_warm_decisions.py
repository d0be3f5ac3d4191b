"""Rejected steps, contracting line searches and the projection onto the bound inside the WARM instantiations of the solve kernels
(lfr_batch_solve_from: the four packed classes, the three LDS footprints, the elimination-tree kernel alone and as a team, on both
of its schedules): the inputs and starts of tests/warm_decision_cases.py (tests/test_warm_decision_cases.py establishes on the CPU
that the reference does take those decisions from them) against tests/warm_ref.py, decision for decision - iterations, termination,
the evaluation counts of the line searches and candidates, and the exact set of coordinates that sit ON the bound.  The criteria are
those of tests/test_gpu_lm_decisions.py for the cold kernels.  Components whose trajectory changes with the reference's own summation
order (warm_decision_cases.solve_both_orders; at most 5 % of a case, none at the present seeds) are left out of the trajectory
checks, never of the positions or terminations."""
import copy

import numpy as np
import pytest

import cost_ref as CR
import lm_decision_cases as LC
import warm_decision_cases as WC
from test_gpu_warm_start import _assert_bitwise, _fresh, _result, _t      # (imports torch: before the library is loaded)
from test_gpu_backward import _nodes
from test_gpu_parity import TOL_UNITS
from test_gpu_set_inputs import _bits
from lfr_amd import capi

pytestmark = pytest.mark.gpu
NAMES = sorted(WC.CASES)
_solved = {}
_labels = {}


def labels(name):
    if name not in _labels:
        _labels[name] = WC.labels(WC.reference(name)[0])
    return _labels[name]


def solved(name):
    """(graph, problem, batch, result of solve_from(start) as the FIRST solve of the batch), once per case"""
    if name not in _solved:
        ma, start = WC.reference(name)[:2]
        g, p, b = _fresh(ma)
        _solved[name] = (g, p, b, _result(b, b.solve_from(_t(start))))
        assert b.spin_timeouts() == 0
    return _solved[name]


def check_decisions(what, name, p, b, res, comps, ref_pos, ref_infos, sensitive):
    """the criteria of test_gpu_lm_decisions.test_decisions_match_the_oracle, against warm_ref's (positions, infos)"""
    comp_of_node = labels(name)["comp"]
    st, pos, info = res["st"], res["pos"], res["info"]
    assert (comp_of_node == p.labels()[2]).all()
    comp = info["component"]
    assert sorted(comp.tolist()) == sorted(comps)
    nv, ne = np.array([comps[c][1].nv for c in comp.tolist()]), np.array([len(comps[c][1].edges) for c in comp.tolist()], np.int64)
    assert (info["n_var_nodes"] == nv).all() and (info["n_edges"] == ne).all()
    assert {LC.kernel_class(2 * v, e) for v, e in zip(nv, ne)} == WC.CLASSES[name]
    want = {k: np.array([ref_infos[c][k] for c in comp.tolist()]) for k in ("termination", "iterations", "n_jac_evals", "n_cost_evals")}
    firm = ~np.isin(comp, sensitive)
    err = np.abs(pos - ref_pos).max()
    want_jac, want_cost = int((want["n_jac_evals"] * ne).sum()), int((want["n_cost_evals"] * ne).sum())
    firm_node = ~np.isin(comp_of_node, sensitive)
    got_mask, want_mask = LC.bound_mask(pos)[firm_node], LC.bound_mask(ref_pos)[firm_node]
    print("%s: %d components (%d sensitive), max |dx| %.3e, iterations differ in %d, bound mask differs in %d of %d coordinates at the bound, "
          "jacobian passes x edges %d (reference %d), cost passes x edges %d (reference %d)"
          % (what, len(comp), len(sensitive), err, int((want["iterations"] != info["iterations"])[firm].sum()),
             int((got_mask != want_mask).sum()), int(want_mask.sum()), st["ref_jacobian_passes_edges"], want_jac, st["ref_cost_passes_edges"], want_cost))
    assert st["n_failed"] == 0 and st["n_components"] == len(comp)
    assert (want["termination"] == info["termination"]).all()
    assert (want["iterations"] == info["iterations"])[firm].all()
    assert err <= TOL_UNITS
    assert (got_mask == want_mask).all()                         # ON the bound: 1 - 1e-16 or 1 + ulp is a mismatch
    assert np.abs(pos).max() <= 1.0
    if len(sensitive) == 0:
        assert st["ref_jacobian_passes_edges"] == want_jac and st["ref_cost_passes_edges"] == want_cost
    else:
        assert st["ref_jacobian_passes_edges"] == pytest.approx(want_jac, rel=1e-3)
        assert st["ref_cost_passes_edges"] == pytest.approx(want_cost, rel=1e-3)
    assert b.spin_timeouts() == 0


# --------------------------------------------------------------------------------------------------------- a. the decisions
@pytest.mark.parametrize("name", NAMES)
def test_decisions_match_the_restatement(lfr_lib, name):
    _, _, comps, ref_pos, ref_infos, sensitive = WC.reference(name)
    g, p, b, res = solved(name)
    check_decisions(name, name, p, b, res, comps, ref_pos, ref_infos, sensitive)


# --------------------------------------------------------------------------------------------------------------- b. the cost
@pytest.mark.parametrize("name", NAMES)
def test_final_cost_is_the_cost_at_the_positions(lfr_lib, name):
    """test_gpu_warm_start's test of the same name on trajectories that rejected steps (min_cost / best_x are then not the current
    cost / x): final_cost against cost_ref at the written positions by its tol_c, against lfr_batch_evaluate there, and it does not
    exceed the cost at the projected start"""
    ma, start = WC.reference(name)[:2]
    g, p, b, res = solved(name)
    info = res["info"]
    comps = CR.components(ma, *p.labels(), *_nodes(g, ma))
    at_x = b.evaluate(_t(res["pos"]), grad=False, residuals=False, weights=False)["cost"].cpu().numpy()
    at_x0 = b.evaluate(_t(np.clip(start, -1.0, 1.0)), grad=False, residuals=False, weights=False)["cost"].cpu().numpy()
    for i, c in enumerate(info["component"].tolist()):
        k = CR.evaluate(comps[c][1], res["pos"][comps[c][0]])
        assert k.arg_rounding <= k.tol(), c
        assert abs(float(CR.LD(info["final_cost"][i]) - k.cost)) <= k.tol(), (c, info["final_cost"][i], k.cost64)
        assert abs(info["final_cost"][i] - at_x[i]) <= 2 * k.tol(), (c, info["final_cost"][i], at_x[i])
        assert info["final_cost"][i] <= at_x0[i] + k.tol(), (c, info["final_cost"][i], at_x0[i])


# ------------------------------------------------------------------------------------------------------------ c. repeatable
@pytest.mark.parametrize("name", NAMES)
def test_second_warm_solve_is_bitwise_the_first(lfr_lib, name):
    start = WC.reference(name)[1]
    _, _, b, res = solved(name)
    _assert_bitwise(_result(b, b.solve_from(_t(start))), res, name)
    assert b.spin_timeouts() == 0


# ------------------------------------------------------------------------------------------------------- d. device assembly
@pytest.mark.parametrize("name", ["packed_24_32", "block_m"])
def test_device_assembly_is_bitwise_the_host_assembly(lfr_lib, name):
    """device-assembled from host labels, and the fused batch of the device graph stage, which writes its records before a warm
    FIRST solve"""
    ma, start = WC.reference(name)[:2]
    res = solved(name)[3]
    for how in ("labels", True):
        g, p, b = _fresh(ma, how)
        got = _result(b, b.solve_from(_t(start)))
        for k in ("n_var_nodes", "n_edges"):
            assert np.array_equal(got["info"][k], res["info"][k]), (how, k)
        _assert_bitwise(got, res, "%s, device-assembled (%s)" % (name, how))
        assert b.spin_timeouts() == 0


# ------------------------------------------------------------------------------------------------------------ e. mixed waves
@pytest.mark.parametrize("name", ["packed_8_16", "packed_24_32"])
def test_mixed_waves(lfr_lib, name):
    """every second component of the batch (component_info order) starts at the origin, the others at the case's start: packed
    wavefronts hold both kinds side by side and take the general first sweep for all of their groups (the closed form at the origin
    is chosen per wavefront).  A component that kept its start is bitwise its result in the run from the full start; one that starts
    at the origin is held to warm_ref from the origin - agreement with lfr_batch_solve only "to rounding" is all that include/lfr.h
    promises for it - with the sensitive set of that run."""
    ma, start, comps, hard_pos, hard_infos, hard_sensitive = WC.reference(name)
    _, _, _, zero_pos, zero_infos, zero_sensitive = WC.reference(name, zero_start=True)
    full = solved(name)[3]
    order = full["info"]["component"].tolist()
    at_zero = set(order[1::2])
    mixed, ref_pos, ref_infos = start.copy(), hard_pos.copy(), dict(hard_infos)
    for c in at_zero:
        mixed[comps[c][0]] = 0.0
        ref_pos[comps[c][0]] = zero_pos[comps[c][0]]
        ref_infos[c] = zero_infos[c]
    sensitive = np.array([c for c in order if c in (set(zero_sensitive.tolist()) if c in at_zero else set(hard_sensitive.tolist()))], np.int64)
    g, p, b = _fresh(ma)
    res = _result(b, b.solve_from(_t(mixed)))
    assert res["info"]["component"].tolist() == order
    kept = np.array([c not in at_zero for c in order])
    assert 0 < kept.sum() < len(order)
    for k in ("iterations", "termination"):
        assert np.array_equal(res["info"][k][kept], full["info"][k][kept]), k
    assert np.array_equal(_bits(res["info"]["final_cost"][kept]), _bits(full["info"]["final_cost"][kept]))
    kept_nodes = np.concatenate([comps[c][0] for c in order if c not in at_zero])
    assert np.array_equal(_bits(res["pos"][kept_nodes]), _bits(full["pos"][kept_nodes]))
    check_decisions("%s, every second component from the origin" % name, name, p, b, res, comps, ref_pos, ref_infos, sensitive)


# ------------------------------------------------------------------------------------------------------------------ f. teams
def test_teams_from_a_hard_warm_start(lfr_lib, monkeypatch):
    """`tree` (rings of 98..160 nodes: hand-out keys 97..159) by teams of two (thresholds 50,1000) and of four (50,60) workgroups
    against one workgroup per component, by the criterion of test_team_against_team_of_one_from_a_warm_start: same terminations and
    iterations, positions to 1e-9 (the reductions meet in another order), bitwise repeatable, no wait gave up - and each setting
    against warm_ref"""
    ma, start, comps, ref_pos, ref_infos, sensitive = WC.reference("tree")
    keys = np.array([prob.nv for _, prob in comps.values()])
    assert keys.min() >= 60 and keys.max() < 1000
    start_t = _t(start)
    out = {}
    for setting in ("0", "50,1000", "50,60"):
        monkeypatch.setenv("LFR_TREE_TEAM", setting)
        g, p, b = _fresh(ma)
        res = _result(b, b.solve_from(start_t))
        assert res["st"]["n_failed"] == 0 and b.spin_timeouts() == 0, setting
        assert (b.team_runs() > 0) == (setting != "0"), setting
        assert b.team_fallbacks() == 0, setting
        again = _result(b, b.solve_from(start_t))
        _assert_bitwise(again, res, "LFR_TREE_TEAM=%s twice" % setting)
        assert b.spin_timeouts() == 0 and b.team_fallbacks() == 0, setting
        check_decisions("tree, LFR_TREE_TEAM=%s" % setting, "tree", p, b, res, comps, ref_pos, ref_infos, sensitive)
        out[setting] = res
    firm = ~np.isin(out["0"]["info"]["component"], sensitive)
    for setting in ("50,1000", "50,60"):
        d = np.abs(out[setting]["pos"] - out["0"]["pos"]).max()
        print("LFR_TREE_TEAM=%s: max difference to one workgroup %.3e" % (setting, d))
        assert d <= 1e-9, setting
        assert np.array_equal(out[setting]["info"]["component"], out["0"]["info"]["component"])
        assert np.array_equal(out[setting]["info"]["termination"][firm], out["0"]["info"]["termination"][firm])
        assert np.array_equal(out[setting]["info"]["iterations"][firm], out["0"]["info"]["iterations"][firm])


# ---------------------------------------------------------------------------------------------------------------- g. FAILURE
@pytest.mark.parametrize("name", ["packed_24_32", "block_s"])
def test_a_failed_component_among_hard_neighbours(lfr_lib, name):
    """one NaN flow entry in one component (test_gpu_warm_start.test_failure_keeps_the_projected_start's, among components that
    reject and contract steps): the victim terminates FAILURE and holds the projected start bitwise; every other component, wave
    neighbours included, is bitwise the clean run"""
    ma, start, comps = WC.reference(name)[:3]
    clean = solved(name)[3]
    order = clean["info"]["component"].tolist()
    victim = order[len(order) // 2]
    lab = labels(name)
    node = {k: i for i, k in enumerate(lab["key"])}
    pair = np.repeat(np.arange(len(ma.pair_img1)), np.diff(ma.pair_off))
    n1 = np.array([node[ma.image_names[i], f] for i, f in zip(ma.pair_img1[pair].tolist(), ma.feat1.tolist())])
    bad = copy.deepcopy(ma)
    bad.disp2[np.nonzero(lab["comp"][n1] == victim)[0][3], 4, 1] = np.nan
    g, p, b = _fresh(bad)
    res = _result(b, b.solve_from(_t(start)))
    assert res["info"]["component"].tolist() == order
    assert res["st"]["n_failed"] == 1 and np.isfinite(res["pos"]).all()
    row = order.index(victim)
    assert res["info"]["termination"][row] == capi.TERM_FAILURE
    var = comps[victim][0]
    assert np.array_equal(_bits(res["pos"][var]), _bits(np.clip(start, -1.0, 1.0)[var]))
    others = np.ones(len(start), bool)
    others[var] = False
    assert np.array_equal(_bits(res["pos"][others]), _bits(clean["pos"][others]))
    keep = np.arange(len(order)) != row
    for k in ("iterations", "termination"):
        assert np.array_equal(res["info"][k][keep], clean["info"][k][keep]), k
    assert np.array_equal(_bits(res["info"]["final_cost"][keep]), _bits(clean["info"]["final_cost"][keep]))
    assert b.spin_timeouts() == 0
