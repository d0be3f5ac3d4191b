"""lfr_batch_solve_from (include/lfr.h): the batched LM solve started at given positions, on the shapes of tests/class_limit_cases.py -
every kernel class at its row and edge limits, the smallest elimination-tree components included.

The reference is tests/warm_ref.py, the restatement of lfr_ref.solve_problem that tests/test_warm_ref.py pins to it at a zero start.
Tolerances are the project's: positions to TOL_UNITS, terminations and iteration counts equal (tests/test_gpu_class_limits.py holds
the cold start to the same), final costs by tests/cost_ref.py's tol_c.  Everything that the contract calls "the same" is compared
bit for bit."""
import copy
import dataclasses

import numpy as np
import pytest
import torch

import cost_ref as CR
import class_limit_cases as CL
import test_gpu_class_limits as TCL
import warm_ref as W
from test_gpu_backward import _check_against_reference as backward_check, _nodes, _ubar
from test_gpu_backward_gn import _check_against_reference as backward_gn_check
from test_gpu_covariance import _check_against_reference as covariance_check
from test_gpu_parity import TOL_UNITS
from test_gpu_set_inputs import _bits, _dev
from lfr_amd import capi, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N = len(CL.NAMES)
START_SEED = 1            # N(0, 0.05) per coordinate; chosen on the CPU: warm_ref converges on every shape from it (asserted below)
FLOW_SEED = 2             # the training step's flow perturbation, N(0, 0.002)
PASS_KEYS = ("ref_jacobian_passes_edges", "ref_cost_passes_edges", "exec_passes_edges", "ref_passes_nodes")
_cache = {}


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x, np.float64)).to(DEV)


def _fresh(ma, how=False, variant="ceres1"):
    """an UNSOLVED batch: how = False (host), "labels" (device-assembled from host labels), True (device graph stage: fused)"""
    g = capi.Graph.from_arrays(ma)
    p = (capi.Problem(g, device_assembly=True) if how == "labels" else capi.Problem(g, device_graph_stage=0) if how else capi.Problem(g))
    return g, p, capi.Batch(p, 0, tukey_variant=variant)


def _result(b, st):
    return dict(st=st, pos=b.download().copy(), info=b.component_info())


def _assert_bitwise(x, y, what):
    """two solves' results: positions, final costs bitwise, iterations, terminations and pass counts equal"""
    assert np.array_equal(x["info"]["component"], y["info"]["component"]), what
    for k in ("iterations", "termination"):
        assert np.array_equal(x["info"][k], y["info"][k]), (what, k)
    assert np.array_equal(_bits(x["info"]["final_cost"]), _bits(y["info"]["final_cost"])), what
    assert np.array_equal(_bits(x["pos"]), _bits(y["pos"])), "%s: positions differ by %.3g" % (what, np.abs(x["pos"] - y["pos"]).max())
    for k in PASS_KEYS + ("n_components", "n_failed", "sum_iterations"):
        assert x["st"][k] == y["st"][k], (what, k)


def _reference(key, ma, start, variant="ceres1"):
    if key not in _cache:
        comps, n = W.components(ma, variant, bisect_fn=capi.bisect_graph)
        _cache[key] = (comps,) + W.solve_graph(comps, n, start)
    return _cache[key]


def _start(n_nodes):
    return np.random.default_rng(START_SEED).normal(0.0, 0.05, size=(n_nodes, 2))


def _assert_matches_reference(s, res, ref_pos, ref_infos, what):
    """the criteria of test_every_shape_matches_the_oracle, against warm_ref"""
    info = res["info"]
    for name in CL.NAMES:
        c, r = s.comp[name], s.row[name]
        ri = ref_infos[c]
        assert ri["termination"] == capi.TERM_CONVERGENCE, (what, name)             # of the input: the reference converges from this start
        err = np.abs(res["pos"][s.nodes[name]] - ref_pos[s.nodes[name]]).max()
        print("%s %-18s max |dx| %.3e, iterations %d (reference %d)" % (what, name, err, info["iterations"][r], ri["iterations"]))
        assert err <= TOL_UNITS, (what, name)
        assert info["termination"][r] == ri["termination"], (what, name)
        assert info["iterations"][r] == ri["iterations"], (what, name)


# ------------------------------------------------------------------------------------------------- 1. zero start is the cold solve
@pytest.mark.parametrize("how", [False, "labels", True], ids=["host", "host_labels", "device_graph_stage"])
def test_zero_start_is_the_cold_solve(lfr_lib, how):
    """an explicit all-zero array: the bits of lfr_batch_solve - for the packed classes the closed-form first sweep against the general
    one.  device_graph_stage: a fused batch whose FIRST solve is the warm one (its records are written first)"""
    cold = TCL.all_solved(how)
    ma, _ = CL.all_shapes()
    g, p, b = _fresh(ma, how)
    zeros = torch.zeros((g.n_nodes, 2), dtype=torch.float64, device=DEV)
    warm = _result(b, b.solve_from(zeros))
    assert warm["st"]["n_components"] == N and warm["st"]["n_failed"] == 0
    _assert_bitwise(warm, dict(st=cold.st, pos=cold.pos, info=cold.info), "zero start/%s" % how)
    assert b.spin_timeouts() == 0
    _, _, class_edges = b.timing()
    assert class_edges.sum() == warm["st"]["n_edges"]                                # lfr_batch_timing serves it: every launch recorded


# ------------------------------------------------------------------------------------------------- 2. against the restatement
def test_random_start_matches_the_restatement(lfr_lib):
    s = TCL.all_solved()
    start = _start(s.g.n_nodes)
    comps, ref_pos, ref_infos = _reference("start", s.ma, start)
    g, p, b = _fresh(s.ma)
    res = _result(b, b.solve_from(_t(start)))
    assert res["st"]["n_failed"] == 0
    _assert_matches_reference(s, res, ref_pos, ref_infos, "N(0, 0.05) start")
    ne = res["info"]["n_edges"].astype(np.int64)
    assert res["st"]["ref_jacobian_passes_edges"] == int(sum(ref_infos[c]["n_jac_evals"] * e for c, e in zip(res["info"]["component"], ne)))
    assert res["st"]["ref_cost_passes_edges"] == int(sum(ref_infos[c]["n_cost_evals"] * e for c, e in zip(res["info"]["component"], ne)))
    assert b.spin_timeouts() == 0


def _graph_against_restatement(label, kw, start_of, variant):
    """a synthetic graph from `start_of(n_nodes)` against warm_ref: the criteria of tests/test_gpu_parity.py's graphs with every
    component held to equal iterations - positions to TOL_UNITS, terminations and iterations equal"""
    ma = synthetic.generate(**kw)
    g, p, b = _fresh(ma, variant=variant)
    start = start_of(g.n_nodes)
    comps, ref_pos, ref_infos = _reference((label, variant), ma, start, variant)
    assert g.n_nodes == len(ref_pos)
    res = _result(b, b.solve_from(_t(start)))
    info = res["info"]
    assert sorted(info["component"].tolist()) == sorted(comps)
    assert all(ref_infos[c]["termination"] == capi.TERM_CONVERGENCE for c in comps)      # of the input: the reference converges
    ref_it = np.array([ref_infos[c]["iterations"] for c in info["component"].tolist()])
    err = np.abs(res["pos"] - ref_pos).max()
    print("%s/%s: %d components, max |dx| %.3e, iterations up to %d, %d components differ in iterations"
          % (label, variant, len(comps), err, ref_it.max(), (ref_it != info["iterations"]).sum()))
    assert res["st"]["n_failed"] == 0 and np.isfinite(res["pos"]).all()
    assert err <= TOL_UNITS
    assert (info["termination"] == capi.TERM_CONVERGENCE).all()
    assert np.array_equal(info["iterations"], ref_it)
    assert b.spin_timeouts() == 0
    return res, ref_pos


def _bounds_start(n):
    """N(0, 0.05), some coordinates beyond the box on either side, some nodes NaN / +inf"""
    s = _start(n)
    s[0::7, 0] = 1.5
    s[3::11, 1] = -1.5
    s[5::13] = (np.nan, np.inf)
    return s


def test_start_beyond_the_box_and_not_finite_matches_the_restatement(lfr_lib):
    """cost_ref.BOUNDS_GRAPH: the start is clamped, NaN reads as 0, +inf as 1, and the solve converges with coordinates at the bound"""
    res, ref_pos = _graph_against_restatement("bounds", CR.BOUNDS_GRAPH, _bounds_start, "ceres1")
    assert (np.abs(res["pos"]) == 1.0).sum() >= 10 and (np.abs(ref_pos) == 1.0).sum() >= 10      # active bounds at the solution
    assert np.abs(res["pos"]).max() <= 1.0


@pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
def test_tukey_graph_matches_the_restatement(lfr_lib, variant):
    _graph_against_restatement("tukey", CR.TUKEY_GRAPH, _start, variant)


# ------------------------------------------------------------------------------------------------------- 3. the training step
def _perturbed(ma):
    rng = np.random.default_rng(FLOW_SEED)
    return dataclasses.replace(ma, disp1=(ma.disp1 + rng.normal(0.0, 0.002, ma.disp1.shape)).astype(np.float32),
                               disp2=(ma.disp2 + rng.normal(0.0, 0.002, ma.disp2.shape)).astype(np.float32))


def _training_step(how):
    """cold solve, new flows, solve_from(NULL) -> (batch, first positions, result)"""
    ma, _ = CL.all_shapes()
    mb = _perturbed(ma)
    g, p, b = _fresh(ma, how)
    b.solve()
    first = b.download().copy()
    b.set_inputs(_dev(mb.disp1), _dev(mb.disp2))
    return b, mb, first, _result(b, b.solve_from(None))


def test_training_step(lfr_lib):
    s = TCL.all_solved()
    b, mb, first, null = _training_step(False)
    assert np.array_equal(_bits(first), _bits(s.pos))
    comps, ref_pos, ref_infos = _reference("step", mb, first)
    _assert_matches_reference(s, null, ref_pos, ref_infos, "training step")
    explicit = _result(b, b.solve_from(_t(first)))                                   # an explicit copy of the first positions
    _assert_bitwise(explicit, null, "explicit copy against NULL")
    again = _result(b, b.solve_from(_t(first)))
    _assert_bitwise(again, explicit, "two warm calls from the same start")
    for how in ("labels", True):
        bd, _, first_d, null_d = _training_step(how)
        assert np.array_equal(_bits(first_d), _bits(first))
        _assert_bitwise(null_d, null, "device-assembled (%s) against host-assembled" % how)
        assert bd.spin_timeouts() == 0
    assert b.spin_timeouts() == 0


# ----------------------------------------------------------------------------------------------------------------- 4. cost
def test_final_cost_is_the_cost_at_the_positions(lfr_lib):
    """final_cost of the warm solve against lfr_batch_evaluate at the positions it wrote, by cost_ref's tol_c (valid where
    arg_rounding <= tol_c: asserted of the input); and it does not exceed the cost at the projected start by more than that"""
    s = TCL.all_solved()
    start = _start(s.g.n_nodes)
    g, p, b = _fresh(s.ma)
    res = _result(b, b.solve_from(_t(start)))
    info = res["info"]
    comps = CR.components(s.ma, *p.labels(), *_nodes(g, s.ma))
    at_x = b.evaluate(None, grad=False, residuals=False, weights=False)["cost"].cpu().numpy()
    at_x0 = b.evaluate(_t(np.clip(start, -1.0, 1.0)), grad=False, residuals=False, weights=False)["cost"].cpu().numpy()
    for i, c in enumerate(info["component"].tolist()):
        k = CR.evaluate(comps[c][1], res["pos"][comps[c][0]])
        assert k.arg_rounding <= k.tol(), c
        assert abs(float(CR.LD(info["final_cost"][i]) - k.cost)) <= k.tol(), (c, info["final_cost"][i], k.cost64)
        assert abs(info["final_cost"][i] - at_x[i]) <= 2 * k.tol(), (c, info["final_cost"][i], at_x[i])
        assert info["final_cost"][i] <= at_x0[i] + k.tol(), (c, info["final_cost"][i], at_x0[i])


# ---------------------------------------------------------------------------------------------------- 5. FAILURE keeps the start
def test_failure_keeps_the_projected_start(lfr_lib):
    """one NaN flow entry in a packed and in a workgroup component: a defined outcome (tests/test_gpu_undefined_inputs.py) - FAILURE,
    the projected start bitwise; every other component, wave neighbours included, is bitwise the run without the NaN"""
    ma, feats = CL.all_shapes()
    s = TCL.all_solved()
    start = _start(s.g.n_nodes)
    start[s.nodes["k6"][1]] = (1.5, -1.5)                                             # the projection shows in what a FAILURE writes
    start[s.nodes["ring45"][2]] = (np.nan, np.inf)
    g, p, b = _fresh(ma)
    clean = _result(b, b.solve_from(_t(start)))
    assert clean["st"]["n_failed"] == 0
    bad = copy.deepcopy(ma)
    victims = ("k6", "ring45")                                                        # 16-row packed class, 88-row LDS class
    for name in victims:
        m = np.nonzero(np.isin(ma.feat1, feats[name]))[0][3]
        bad.disp2[m, 4, 1] = np.nan
    g2, p2, b2 = _fresh(bad)
    res = _result(b2, b2.solve_from(_t(start)))
    assert res["st"]["n_failed"] == len(victims) and np.isfinite(res["pos"]).all()
    x0 = np.clip(np.nan_to_num(start, nan=0.0, posinf=np.inf, neginf=-np.inf), -1.0, 1.0)
    others = np.ones(s.g.n_nodes, bool)
    for name in victims:
        r = s.row[name]
        assert res["info"]["termination"][r] == capi.TERM_FAILURE, name
        var = s.nodes[name][np.abs(clean["pos"][s.nodes[name]]).sum(axis=1) > 0]      # (the root is constant: 0)
        assert len(var) == CL.SHAPES[name]["rows"] // 2
        assert np.array_equal(_bits(res["pos"][var]), _bits(x0[var])), name
        others[s.nodes[name]] = False
    assert np.array_equal(_bits(res["pos"][others]), _bits(clean["pos"][others]))
    keep = ~np.isin(np.arange(N), [s.row[v] for v in victims])
    for k in ("iterations", "termination"):
        assert np.array_equal(res["info"][k][keep], clean["info"][k][keep]), k
    assert np.array_equal(_bits(res["info"]["final_cost"][keep]), _bits(clean["info"]["final_cost"][keep]))


# ------------------------------------------------------------------------------------------------------------ 6. unread entries
def test_constants_and_unsolved_nodes_are_not_read(lfr_lib):
    s = TCL.all_solved()
    start = _start(s.g.n_nodes)
    g, p, b = _fresh(s.ma)
    ref = _result(b, b.solve_from(_t(start)))
    is_var = np.zeros(s.g.n_nodes, bool)
    for var_nodes, _ in CR.components(s.ma, *p.labels(), *_nodes(g, s.ma)).values():
        is_var[var_nodes] = True
    assert (~is_var).sum() >= N and np.asarray(p.labels()[1], bool)[~is_var].any()     # every shape has its root
    poisoned = start.copy()
    poisoned[~is_var] = 7.0
    res = _result(b, b.solve_from(_t(poisoned)))
    _assert_bitwise(res, ref, "7.0 at roots and unsolved nodes")
    assert not res["pos"][~is_var].any()


@pytest.mark.parametrize("kind", ["lpt_shard", "device_shard"])
def test_entries_outside_the_shard_are_not_read(lfr_lib, kind):
    """shard 0 of 2 of a host-assembled and of a device-assembled problem: entries of the start array at every node the shard does
    not solve (the other shard's, roots) set to 7.0 change nothing, and the positions there stay 0"""
    ma, _ = CL.all_shapes()
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g) if kind == "lpt_shard" else capi.Problem(g, device_graph_stage=0)
    b = capi.Batch(p, 0, 0, 2)
    start = _start(g.n_nodes)
    ref = _result(b, b.solve_from(_t(start)))
    n_comp = ref["st"]["n_components"]
    assert 0 < n_comp < N and ref["st"]["n_failed"] == 0                               # a part of the graph, not all of it
    is_var = ref["pos"].any(axis=1)                                                  # (a variable node's solution is not exactly 0)
    assert is_var.sum() == int(ref["info"]["n_var_nodes"].sum())
    poisoned = start.copy()
    poisoned[~is_var] = 7.0
    res = _result(b, b.solve_from(_t(poisoned)))
    _assert_bitwise(res, ref, "7.0 outside the shard (%s)" % kind)
    assert not res["pos"][~is_var].any()
    # what the shard solves is what the whole batch solves from the same start
    gw, pw, bw = _fresh(ma)
    whole = _result(bw, bw.solve_from(_t(start)))
    assert np.abs(res["pos"][is_var] - whole["pos"][is_var]).max() <= TOL_UNITS      # (other wave neighbours than in the whole batch)


# ------------------------------------------------------------------------------------------------------- 7. after a warm solve
def _class_edges_of_all(serial=False):
    """what lfr_batch_timing reports for ALL: per class; the launch plan times the packed classes as ONE launch, in the slot of the
    largest packed class present (slot 4 here)"""
    want = np.zeros(capi.NUM_KERNEL_CLASSES, np.int64)
    for sh in CL.SHAPES.values():
        want[CL.CLASS_SLOT[sh["cls"]]] += sh["edges"]
    if not serial:
        packed = want[:5].sum()
        want[:5] = 0
        want[4] = packed
    return want


@pytest.mark.parametrize("how", [False, True], ids=["host", "device_graph_stage"])
def test_backward_covariance_and_timing_after_a_warm_solve(lfr_lib, how):
    """the FIRST solve of the batch is the warm one (device_graph_stage: a fused batch that writes its records first): backward in
    both modes and the covariance meet the reference checks of their own tests on a packed and an LDS-class shape; after set_inputs
    they refuse (LFR_ERR_ARG) until solve_from has run; lfr_batch_timing reports every class's launch"""
    s = TCL.all_solved()
    ma, _ = CL.all_shapes()
    g, p, b = _fresh(ma, how)
    gp = _ubar(g.n_nodes, 31)
    for call in (lambda: b.backward(gp), lambda: b.covariance()):                    # nothing solved yet
        with pytest.raises(capi.LfrError):
            call()
    st = b.solve_from(_t(_start(g.n_nodes)))
    assert st["n_failed"] == 0
    which = [s.comp["k9_full"], s.comp["ring45"]]                                     # 16-row packed class (re-read slots), 88-row LDS class

    def passes(m):
        n, bst, _ = backward_check(m, g, p, b, gp, which)
        assert n == 2 and (b.backward_status() == capi.BACKWARD_OK).all()
        n, _, _, worst, _ = backward_gn_check(m, g, p, b, gp, which)
        assert n == 2
        n, cst, worst = covariance_check(m, g, p, b, which)
        assert n == 2 and (b.covariance_status() == capi.COVARIANCE_OK).all()

    passes(ma)
    total_ms, class_ms, class_edges = b.timing()
    assert class_edges.tolist() == _class_edges_of_all().tolist()
    assert total_ms > 0 and (class_ms[4:] > 0).all() and not class_ms[:4].any()        # the packed launch, the four workgroup launches
    mb = _perturbed(ma)
    b.set_inputs(_dev(mb.disp1), _dev(mb.disp2))
    for call in (lambda: b.backward(gp), lambda: b.backward(gp, gauss_newton=True), lambda: b.covariance()):
        with pytest.raises(capi.LfrError) as e:
            call()
        assert e.value.code == -1 and "inputs changed" in str(e.value)                # LFR_ERR_ARG
    st = b.solve_from(None)
    assert st["n_failed"] == 0
    passes(mb)
    assert b.timing()[2].tolist() == _class_edges_of_all().tolist()
    assert b.spin_timeouts() == 0


# ------------------------------------------------------------------------------------------------------------------- 8. teams
def test_team_against_team_of_one_from_a_warm_start(lfr_lib, monkeypatch):
    """the thin elimination-tree shape (ring98: 97 variable nodes, one root - hand-out key 97) solved by a team of two and of four
    workgroups against one workgroup, warm from the same start, by the criterion of test_teams_of_workgroups_per_component: same
    terminations and iterations, positions to 1e-9 (the reductions meet in another order), bitwise repeatable, no wait gave up"""
    ma, _ = CL.all_shapes()
    s = TCL.all_solved()
    start = _t(_start(s.g.n_nodes))
    out = {}
    for setting in ("0", "50,1000", "50,60"):
        monkeypatch.setenv("LFR_TREE_TEAM", setting)
        g, p, b = _fresh(ma)
        res = _result(b, b.solve_from(start))
        assert res["st"]["n_failed"] == 0 and b.spin_timeouts() == 0, setting
        assert (b.team_runs() > 0) == (setting != "0"), setting
        assert b.team_fallbacks() == 0, setting
        for _ in range(2):
            again = _result(b, b.solve_from(start))
            assert np.array_equal(_bits(again["pos"]), _bits(res["pos"])) and b.spin_timeouts() == 0, setting
        out[setting] = res
    nodes = s.nodes["ring98"]
    for setting in ("50,1000", "50,60"):
        d = np.abs(out[setting]["pos"] - out["0"]["pos"]).max()
        print("LFR_TREE_TEAM=%s: max difference to one workgroup %.3e" % (setting, d))
        assert d <= 1e-9, setting
        assert np.array_equal(out[setting]["info"]["termination"], out["0"]["info"]["termination"])
        assert np.array_equal(out[setting]["info"]["iterations"], out["0"]["info"]["iterations"])
        others = np.ones(s.g.n_nodes, bool)
        others[nodes] = False
        assert np.array_equal(_bits(out[setting]["pos"][others]), _bits(out["0"]["pos"][others]))      # only the team's component may differ


def test_serial_classes_are_the_same_warm_solve(lfr_lib, monkeypatch):
    """LFR_SERIAL_CLASSES=1: every class in a launch of its own - for the packed classes the one warm kernel with every block in the
    class's range - gives the bits of the launch plan"""
    ma, _ = CL.all_shapes()
    g, p, b = _fresh(ma)
    start = _t(_start(g.n_nodes))
    plan = _result(b, b.solve_from(start))
    monkeypatch.setenv("LFR_SERIAL_CLASSES", "1")
    g2, p2, b2 = _fresh(ma)
    serial = _result(b2, b2.solve_from(start))
    _assert_bitwise(serial, plan, "serial classes")
    assert b2.timing()[2].tolist() == _class_edges_of_all(serial=True).tolist() and b2.spin_timeouts() == 0


# ------------------------------------------------------------------------------------------------- 9. Refiner(warm_start=True)
def _refiner_inputs(ma):
    kw = dict(image_names=ma.image_names, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off, feat1=ma.feat1,
              feat2=ma.feat2, image_facts=ma.facts)
    return _dev(ma.disp1), _dev(ma.disp2), torch.as_tensor(ma.sim).to(DEV), kw


def test_refiner_warm_start(lfr_lib):
    from lfr_amd.autograd import Refiner
    ma, _ = CL.all_shapes()
    mb = _perturbed(ma)
    d1, d2, sim, kw = _refiner_inputs(ma)
    e1, e2 = _dev(mb.disp1), _dev(mb.disp2)
    warm, cold = Refiner(d1, d2, sim, warm_start=True, **kw), Refiner(d1, d2, sim, **kw)
    w1, c1 = warm(d1, d2).detach().cpu().numpy(), cold(d1, d2).detach().cpu().numpy()
    assert np.array_equal(_bits(w1), _bits(c1))                                       # the first forward is cold
    e1g = e1.clone().requires_grad_(True)
    w2t = warm(e1g, e2)
    w2 = w2t.detach().cpu().numpy()
    # an identically built batch: device graph stage, cold solve, new flows, solve_from(None)
    _, _, _, null = _training_step(True)
    assert np.array_equal(_bits(w2), _bits(null["pos"]))
    c2 = cold(e1, e2).detach().cpu().numpy()
    # the gradient is the implicit one at the warm solution: backward_ref's check (tests/test_gpu_backward.py) on the Refiner's own
    # batch, every component, and what autograd delivers is that gradient rounded to float32
    gp = _ubar(w2.shape[0], 5)
    (w2t * gp).sum().backward()
    rb = warm._batch
    comps = rb.component_info()["component"].tolist()
    n, _, (g1, _, _) = backward_check(mb, rb.problem.graph, rb.problem, rb, gp, comps)
    assert n == len(comps) == N
    assert e1g.grad is not None and g1.any() and np.array_equal(e1g.grad.cpu().numpy().reshape(g1.shape), g1.astype(np.float32))
    warm.reset_start()
    w3 = warm(e1, e2).detach().cpu().numpy()
    assert np.array_equal(_bits(w3), _bits(c2))                                       # reset_start: the cold Refiner's bits
    warm.close()
    cold.close()
