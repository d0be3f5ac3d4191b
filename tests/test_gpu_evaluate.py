"""lfr_batch_evaluate (include/lfr.h) against tests/evaluate_ref.py: cost, dF/dx, raw residuals and loss weights of every kernel class
at two position sets - (a) the solve's own, (b) evaluate_ref.positions_b: uniform in [-1.2, 1.2] with a kink and a clamped argument
in every component - and the call's contract: NULL positions, constants, isolation inside a wave, repeatability, assembly kinds,
lfr_batch_set_inputs and its event waits, shards, arguments, Refiner.evaluate.

Tolerances: the cost within cost_ref.Cost.tol(); gradient, residuals and weights within 8 x the fp64 constants measured by
tests/test_evaluate_ref.py, in the units of tests/evaluate_ref.py."""
import numpy as np
import pytest
import torch

import class_limit_cases as CL
import cost_ref as CR
import evaluate_ref as ER
import test_gpu_class_limits as TCL
from test_gpu_backward import _nodes
from test_gpu_set_inputs import _build, _dev, _flows18, _meta
from lfr_amd import capi, synthetic
from lfr_amd.autograd import Refiner, _kept_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = ("cost", "grad", "residuals", "weights")
_cache = {}


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _ev(b, pos=None, **kw):
    out = b.evaluate(None if pos is None else torch.as_tensor(np.ascontiguousarray(pos, np.float64), device=DEV), **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _assert_same(x, y, what=""):
    for k in KEYS:
        assert (k in x) == (k in y), (what, k)
        if k in x:
            assert x[k].dtype == y[k].dtype and np.array_equal(_raw(x[k]), _raw(y[k])), (what, k)


def _components(ma, g, p, info=None):
    comps = CR.components(ma, *p.labels(), *_nodes(g, ma))
    return comps if info is None else {int(c): comps[int(c)] for c in info["component"]}


def _check(out, info, comps, pos, n_nodes, n_matches, variant, what):
    """every output of one evaluate (float64) against the reference at pos; returns the largest error of each in its tolerance"""
    evals = ER.at_positions(comps, pos, variant)
    worst = dict.fromkeys(KEYS, 0.0)
    is_var = np.zeros(n_nodes, bool)
    for i, c in enumerate(info["component"].tolist()):
        var_nodes, ed = comps[c]
        ev = evals[c]
        is_var[var_nodes] = True
        assert ev.cost.arg_rounding <= ev.cost.tol(), (what, c)                    # the tolerance is valid here (cost_ref's text)
        e = abs(float(CR.LD(out["cost"][i]) - ev.cost.cost)) / ev.cost.tol()
        assert np.isfinite(out["cost"][i]) and e <= 1.0, "%s, component %d: cost %.17g, reference %.17g, %.3g tol_c" % (what, c, out["cost"][i], ev.cost.cost64, e)
        worst["cost"] = max(worst["cost"], e)
        err = np.abs(out["grad"][var_nodes].astype(CR.LD) - ev.grad)
        tol = ER.GPU_FACTOR * ER.GAMMA_GRAD_CPU * ev.g_unit
        assert (err <= tol).all(), "%s, component %d: gradient off by %.3g tolerances" % (what, c, float((err[tol > 0] / tol[tol > 0]).max()))
        worst["grad"] = max(worst["grad"], float((err[tol > 0] / tol[tol > 0]).max(initial=0.0)))
    assert not out["grad"][~is_var].any(), what                                     # constants, unsolved nodes, other shards: exactly 0
    res, wts, res_u, wts_u = ER.match_layout(comps, evals, n_matches, CR.LD)
    for key, got, want, tol in (("residuals", out["residuals"], res, ER.GPU_FACTOR * ER.GAMMA_RES_CPU * res_u),
                                ("weights", out["weights"], wts, ER.GPU_FACTOR * ER.GAMMA_W_CPU * wts_u)):
        err = np.abs(got.astype(CR.LD) - want).astype(np.float64)
        assert got.shape == want.shape and (err <= tol).all(), "%s: %s off by %.3g tolerances" % (what, key, (err[tol > 0] / tol[tol > 0]).max(initial=0.0))
        worst[key] = max(worst[key], float((err[tol > 0] / tol[tol > 0]).max(initial=0.0)))
    assert np.array_equal(out["weights"] == -1.0, wts == -1.0) and (out["weights"] >= 0.0).sum() == sum(len(ed) for _, ed in comps.values()), what
    print("%s: largest error in its tolerance: cost %.4f, gradient %.4f, residuals %.4f, weights %.4f"
          % (what, worst["cost"], worst["grad"], worst["residuals"], worst["weights"]))
    return worst


def _check_f32(b, pos, out64, what):
    out32 = _ev(b, pos, f64=False)
    for k in ("residuals", "weights"):
        assert out32[k].dtype == np.float32 and np.array_equal(_raw(out32[k]), _raw(out64[k].astype(np.float32))), (what, k)
    for k in ("cost", "grad"):
        assert np.array_equal(_raw(out32[k]), _raw(out64[k])), (what, k)


def _positions_b(s):
    return ER.positions_b(_components(s.ma, s.g, s.p), s.g.n_nodes)


def class_limit_outputs(device_assembly, which):
    """one evaluate of the solved class-limit batch per (assembly, position set), shared by the tests below"""
    key = ("cl", device_assembly, which)
    if key not in _cache:
        s = TCL.all_solved(device_assembly)
        pos = s.pos if which == "a" else _positions_b(s)
        _cache[key] = (s, pos, _ev(s.b, pos))
    return _cache[key]


def _small(kw, variant="ceres1", cap=0):
    ma = synthetic.generate(**kw)
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g, max_nodes_in_component=cap)
    b = capi.Batch(p, 0, tukey_variant=variant)
    st = b.solve()
    return ma, g, p, b, st, b.download().copy()


# ------------------------------------------------------------------------------------------ 1. every kernel class at its limits
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("device_assembly", [False, True], ids=["host", "device"])
def test_every_class_at_its_limits(lfr_lib, device_assembly, which):
    s, pos, out = class_limit_outputs(device_assembly, which)
    comps = _components(s.ma, s.g, s.p, s.info)
    assert len(out["cost"]) == len(CL.NAMES) and out["residuals"].shape == (s.g.n_edges // 2, 2, 2)
    _check(out, s.info, comps, pos, s.g.n_nodes, s.g.n_edges // 2, "ceres1", "class limits/%s/(%s)" % (device_assembly, which))
    _check_f32(s.b, pos, out, "class limits")
    if which == "a":
        evals = ER.at_positions(comps, pos)
        for i, c in enumerate(s.info["component"].tolist()):
            if s.info["termination"][i] in (capi.TERM_CONVERGENCE, capi.TERM_NO_CONVERGENCE):
                assert abs(out["cost"][i] - s.info["final_cost"][i]) <= 2 * evals[c].cost.tol(), (c, out["cost"][i], s.info["final_cost"][i])
    else:
        assert (np.abs(pos) > 1.0).any()                                             # nothing is clamped to the box: the reference was not


# --------------------------------------------------------------------------------------------- 2. losses at work and bounds
@pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
def test_tukey_weights_tell_off_from_absent(lfr_lib, variant):
    """cost_ref.TUKEY_GRAPH at the solve's positions: its wrong matches are saturated, weight exactly 0.  The graph stage keeps every
    one of its edges, so no direction of it reads -1; the same graph under a size cap of 12 nodes per component has components cut
    and their joining matches dropped: those read -1.  Both facts are asserted of the input before the outputs are looked at."""
    for cap, want_absent in ((0, False), (12, True)):
        ma, g, p, b, st, pos = _small(CR.TUKEY_GRAPH, variant, cap)
        info = b.component_info()
        comps = _components(ma, g, p, info)
        out = _ev(b, pos)
        evals = ER.at_positions(comps, pos, variant)
        assert any((ev.rho1[comps[c][1].kind == CR.KIND_INTER] == 0).any() for c, ev in evals.items())
        assert (sum(len(ed) for _, ed in comps.values()) < g.n_edges) == want_absent
        _check(out, info, comps, pos, g.n_nodes, g.n_edges // 2, variant, "tukey/%s/cap %d" % (variant, cap))
        assert (out["weights"] == 0.0).any() and out["residuals"][out["weights"] == 0.0].any()
        assert (out["weights"] == -1.0).any() == want_absent and not out["residuals"][out["weights"] == -1.0].any()


def test_coordinates_at_the_bound_carry_their_gradient(lfr_lib):
    ma, g, p, b, st, pos = _small(CR.BOUNDS_GRAPH)
    info = b.component_info()
    comps = _components(ma, g, p, info)
    out = _ev(b, pos)
    _check(out, info, comps, pos, g.n_nodes, g.n_edges // 2, "ceres1", "bounds")
    at_bound = np.abs(pos) == 1.0
    assert at_bound.sum() >= 10 and (out["grad"][at_bound] != 0.0).all()             # not projected, not zeroed


# ------------------------------------------------------------------------------------ 3. NULL means the batch's positions
def test_null_positions_are_the_batchs(lfr_lib):
    s, pos, out = class_limit_outputs(False, "a")
    _assert_same(_ev(s.b, None), out, "evaluate(None) against evaluate(downloaded positions)")
    ma, _ = CL.all_shapes()
    g, p, b, _ = _build(ma, "host")
    with pytest.raises(capi.LfrError) as e:
        b.evaluate()
    assert e.value.code == -1
    comps = _components(ma, g, p)
    posb = ER.positions_b(comps, g.n_nodes)
    _check(_ev(b, posb), b.component_info(), comps, posb, g.n_nodes, g.n_edges // 2, "ceres1", "explicit positions before the first solve")


# ------------------------------------------------------------------------------------------------------ 4. constants read 0
def test_constants_and_unsolved_nodes_are_not_read(lfr_lib):
    for kw, label in ((None, "class limits"), (CR.TUKEY_GRAPH, "tukey")):
        if kw is None:
            s, pos, out = class_limit_outputs(False, "b")
            ma, g, p, b = s.ma, s.g, s.p, s.b
        else:
            ma, g, p, b, st, _ = _small(kw)
            pos = ER.positions_b(_components(ma, g, p), g.n_nodes)
            out = _ev(b, pos)
        is_var = np.zeros(g.n_nodes, bool)
        for var_nodes, _ in _components(ma, g, p, b.component_info()).values():
            is_var[var_nodes] = True
        assert (~is_var).sum() >= 1 and np.asarray(p.labels()[1], bool)[~is_var].any()
        poisoned = pos.copy()
        poisoned[~is_var] = np.nan                                                   # every root, every node outside solved components
        _assert_same(_ev(b, poisoned), out, label)


# ------------------------------------------------------------------------------------------------------------- 5. isolation
def _twice():
    if "twice" not in _cache:
        mt, feats2 = CL.all_twice()
        g, p, b, _ = _build(mt, "host")
        comps = _components(mt, g, p)
        names = [CL.components_of(f, g.nodes()[1], p.labels()[2]) for f in feats2]
        _cache["twice"] = (mt, g, p, b, comps, names, ER.positions_b(comps, g.n_nodes))
    return _cache["twice"]


def _assert_others_unchanged(x, y, info, comps, victims, n_nodes, what):
    rows = ~np.isin(info["component"], victims)
    assert np.array_equal(_raw(x["cost"][rows]), _raw(y["cost"][rows])), what
    nodes, dirs = np.ones(n_nodes, bool), np.ones(x["weights"].size, bool)
    for c in victims:
        nodes[comps[c][0]] = False
        dirs[comps[c][1].eids] = False
    assert np.array_equal(_raw(x["grad"][nodes]), _raw(y["grad"][nodes])), what
    assert np.array_equal(_raw(x["weights"].reshape(-1)[dirs]), _raw(y["weights"].reshape(-1)[dirs])), what
    assert np.array_equal(_raw(x["residuals"].reshape(-1, 2)[dirs]), _raw(y["residuals"].reshape(-1, 2)[dirs])), what
    return rows


def test_components_of_a_wave_do_not_influence_each_other(lfr_lib):
    mt, g, p, b, comps, names, pos = _twice()
    info = b.component_info()
    out = _ev(b, pos)
    victims = [names[0]["k5"], names[1]["k6"], names[0]["k10"], names[1]["k14"]]     # one component per packed class
    moved = pos.copy()
    for c in victims:
        moved[comps[c][0]] += 0.0625
    out2 = _ev(b, moved)
    rows = _assert_others_unchanged(out, out2, info, comps, victims, g.n_nodes, "perturbed positions")
    assert (out["cost"][~rows] != out2["cost"][~rows]).all()


def test_a_nan_flow_fails_its_component_alone(lfr_lib):
    mt, g, p, b, comps, names, pos = _twice()
    info = b.component_info()
    out = _ev(b, pos, want_stats=True)
    assert out["stats"]["n_nonfinite"] == 0 and out["stats"]["n_components"] == len(info["component"])
    seq = 0.0
    for v in out["cost"]:
        seq += float(v)
    assert out["stats"]["sum_cost"] == seq
    for victim in (names[1]["k7_first_reread"], names[0]["ring46"]):                 # a packed group in the middle of a wave, a workgroup
        eid = int(comps[victim][1].eids[3])
        d1, d2 = _flows18(mt.disp1).copy(), _flows18(mt.disp2).copy()
        (d1 if eid & 1 else d2)[eid >> 1, 8] = np.nan
        b.set_inputs(_dev(d1), _dev(d2))
        bad = _ev(b, pos, want_stats=True)
        b.set_inputs(_dev(mt.disp1), _dev(mt.disp2))
        r = int(np.nonzero(info["component"] == victim)[0][0])
        assert not np.isfinite(bad["cost"][r]) and bad["stats"]["n_nonfinite"] == 1
        rows = _assert_others_unchanged(out, bad, info, comps, [victim], g.n_nodes, "NaN flow")
        seq = 0.0
        for v in bad["cost"][rows]:
            seq += float(v)
        assert bad["stats"]["sum_cost"] == seq
    _assert_same(_ev(b, pos), out, "the clean flows again")


# ------------------------------------------------------------------------------------------- 6. repeatability and assembly
def test_repeatable_and_the_same_for_every_assembly(lfr_lib):
    for which in ("a", "b"):
        s, pos, out = class_limit_outputs(False, which)
        _assert_same(_ev(s.b, pos), out, "second call")
    h, posb, outh = class_limit_outputs(False, "b")
    d, _, outd = class_limit_outputs(True, "b")
    assert sorted(h.info["component"]) == sorted(d.info["component"])
    order = [int(np.nonzero(d.info["component"] == c)[0][0]) for c in h.info["component"]]
    assert np.array_equal(_raw(outh["cost"]), _raw(outd["cost"][order]))
    for k in KEYS[1:]:
        assert np.array_equal(_raw(outh[k]), _raw(outd[k])), k
    # a device-assembled whole batch: its packed records are gathered from the graph's arrays until something writes them
    ma, _ = CL.all_shapes()
    _, _, fused, _ = _build(ma, "fused")
    fused.solve()
    first = _ev(fused, posb)                           # this call materialises the records
    _, _, twice, _ = _build(ma, "fused")
    twice.solve()
    twice.solve()                                      # the second solve did
    _assert_same(first, _ev(twice, posb), "materialised by the evaluate / by the second solve")
    _assert_same(first, outd, "fused")
    x = fused.download().copy()
    fused.solve()                                      # the solve after the evaluate reads the records the evaluate wrote
    assert np.array_equal(_raw(fused.download()), _raw(x))


# ------------------------------------------------------------------------------------------------------- 7. with set_inputs
def test_new_flows_at_the_old_positions(lfr_lib):
    ma, _ = CL.all_shapes()
    mb = CL.second_inputs()
    g, p, b, _ = _build(ma, "host")
    b.solve()
    x0 = b.download().copy()
    info = b.component_info()
    new = [_dev(mb.disp1), _dev(mb.disp2), _dev(mb.sim, flows=False)]
    old = [_dev(ma.disp1), _dev(ma.disp2), _dev(ma.sim, flows=False)]
    b.set_inputs(*new)
    out = _ev(b, None)
    _check(out, info, _components(mb, g, p, info), x0, g.n_nodes, g.n_edges // 2, "ceres1", "new flows at the old positions")
    with pytest.raises(capi.LfrError) as e:
        b.backward(torch.zeros((g.n_nodes, 2), dtype=torch.float64, device=DEV))
    assert e.value.code == -1 and "inputs changed since the latest solve" in str(e.value)
    # the synchronous sequence, then the same on two streams without a host synchronisation in between: the event waits order them
    b.solve()
    want = _ev(b, None)
    b.set_inputs(*old)
    b.solve()
    assert not np.array_equal(_raw(_ev(b, None)["cost"]), _raw(want["cost"]))
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    b.set_inputs(*new, stream=s1.cuda_stream)
    b.solve(stream=s2.cuda_stream, want_stats=False)
    got = b.evaluate(None, stream=s1.cuda_stream)
    b.set_inputs(*old, stream=s2.cuda_stream)          # waits for the evaluate: the records it read are the new ones
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    comp_of = CL.components_of(CL.all_shapes()[1], g.nodes()[1], p.labels()[2])
    tree = np.isin(info["component"], [comp_of[n] for n in CL.TREE])
    assert np.array_equal(_raw(got["cost"][~tree]), _raw(want["cost"][~tree]))
    assert np.allclose(got["cost"][tree], want["cost"][tree], rtol=1e-6, atol=0)      # (team shapes: equal to rounding, include/lfr.h)


# ------------------------------------------------------------------------------------------------- 8. shards and arguments
def test_shards_cover_the_matches_once(lfr_lib):
    s, pos, out = class_limit_outputs(False, "a")
    seen = np.zeros(out["weights"].shape, bool)
    for rank in range(2):
        b = capi.Batch(s.p, 0, rank, 2)
        info = b.component_info()
        posb = _positions_b(s)
        o = _ev(b, posb)
        _check(o, info, _components(s.ma, s.g, s.p, info), posb, s.g.n_nodes, s.g.n_edges // 2, "ceres1", "shard %d of 2" % rank)
        assert not (seen & (o["weights"] >= 0)).any()
        seen |= o["weights"] >= 0
    assert np.array_equal(seen, out["weights"] >= 0) and seen.any()


def test_arguments(lfr_lib):
    s, pos, out = class_limit_outputs(False, "a")
    L = capi.lib()
    with pytest.raises(capi.LfrError) as e:
        s.b.evaluate(cost=False, grad=False, residuals=False, weights=False)
    assert e.value.code == -1
    cost = torch.zeros(len(out["cost"]), dtype=torch.float64, device=DEV)
    assert L.lfr_batch_evaluate(s.b._h, None, cost.data_ptr(), None, None, None, 2, None, None) == -1
    assert L.lfr_batch_evaluate(None, None, cost.data_ptr(), None, None, None, 0, None, None) == -1
    assert L.lfr_batch_evaluate(s.b._h, None, cost.data_ptr(), None, None, None, 0, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_raw(cost.cpu().numpy()), _raw(out["cost"]))
    only = _ev(s.b, pos, grad=False, residuals=False)                                 # any subset of the outputs: the same bits
    assert sorted(only) == ["cost", "weights"]
    assert np.array_equal(_raw(only["cost"]), _raw(out["cost"])) and np.array_equal(_raw(only["weights"]), _raw(out["weights"]))
    # a batch over one rank's connected components numbers its matches by itself
    mc = synthetic.generate(seed=32, n_images=48, n_tracks=3000, eps_out=0.002)
    g2 = capi.Graph.from_arrays(mc)
    p2 = capi.Problem(g2, device_graph_stage=0, shard=(0, 2))
    assert p2.cc_sharded
    b2 = capi.Batch(p2, 0)
    zeros = torch.zeros((g2.n_nodes, 2), dtype=torch.float64, device=DEV)
    for kw in (dict(), dict(residuals=False), dict(weights=False)):
        with pytest.raises(capi.LfrError) as e:
            b2.evaluate(zeros, **kw)
        assert e.value.code == -5
    o = _ev(b2, zeros.cpu().numpy(), residuals=False, weights=False, want_stats=True)
    assert np.isfinite(o["cost"]).all() and o["stats"]["n_nonfinite"] == 0 and o["grad"].any() and o["stats"]["kernel_ms"] > 0


# ------------------------------------------------------------------------------------------------------ 9. Refiner.evaluate
def test_refiner_evaluate_scatters_to_the_callers_rows(lfr_lib):
    ma = synthetic.generate(seed=41, n_images=12, n_tracks=120)
    banned = ("000005.png",)
    r = Refiner(_dev(ma.disp1), _dev(ma.disp2), _dev(ma.sim, flows=False), banned=banned, **_meta(ma))
    r(_dev(ma.disp1), _dev(ma.disp2))
    out = r.evaluate()
    inner = r._batch.evaluate()
    torch.cuda.synchronize()
    rows = _kept_rows(ma.pair_img1, ma.pair_img2, ma.pair_off, list(ma.image_names), banned)
    gone = np.ones(ma.n_matches, bool)
    gone[rows] = False
    assert gone.any() and out["weights"].shape == (ma.n_matches, 2) and out["residuals"].shape == (ma.n_matches, 2, 2)
    assert bool((out["weights"][gone] == -1).all()) and not bool(out["residuals"][gone].any())
    for k in ("weights", "residuals"):
        assert torch.equal(out[k][~torch.as_tensor(gone)], inner[k]) and not out[k].requires_grad
    assert torch.equal(out["cost"], inner["cost"]) and torch.equal(out["grad"], inner["grad"]) and bool((out["weights"] >= 0).any())
    r.close()
