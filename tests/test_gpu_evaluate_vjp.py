"""lfr_batch_evaluate_vjp (include/lfr.h) against tests/evaluate_vjp_ref.py: the gradients of the cost, residual and weight bars with
respect to the positions, the flows and the similarities, for every kernel class at the two position sets of
tests/test_gpu_evaluate.py and three bar sets (cost bar alone, all three, residual bar alone), and the call's contract: exact zeros,
float32, repeatability, isolation inside a wave, lfr_batch_set_inputs and its event waits, shards, arguments, Refiner.objective.

Tolerances: 8 x the fp64 constants measured by tests/test_evaluate_vjp_ref.py, in the units of tests/evaluate_vjp_ref.py; with a cost
bar of 1 alone the position gradient is also held to lfr_batch_evaluate's gradient tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import class_limit_cases as CL
import cost_ref as CR
import evaluate_ref as ER
import evaluate_vjp_ref as VR
import test_gpu_class_limits as TCL
from test_gpu_evaluate import _components, _positions_b, _raw, _small, _twice
from test_gpu_set_inputs import _build, _dev, _meta
from lfr_amd import capi, synthetic
from lfr_amd.autograd import Refiner, _kept_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OUT = ("positions", "disp1", "disp2", "sim")
GAMMA = {"positions": VR.GAMMA_VJP_X_CPU, "disp1": VR.GAMMA_VJP_FLOW_CPU, "disp2": VR.GAMMA_VJP_FLOW_CPU, "sim": VR.GAMMA_VJP_SIM_CPU}


def _t(a, dtype=np.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype), device=DEV)


def _vjp(b, pos, cbar=None, rbar=None, wbar=None, f64=True, **kw):
    dt = np.float64 if f64 else np.float32
    out = b.evaluate_vjp(_t(pos), cost_bar=_t(cbar), residuals_bar=_t(rbar, dt), weights_bar=_t(wbar, dt), f64=f64, **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _assert_same(x, y, what=""):
    for k in OUT:
        assert x[k].dtype == y[k].dtype and np.array_equal(_raw(x[k]), _raw(y[k])), (what, k)


def _bars_for(info, n_matches, which):
    """bars of set `which`: the cost bar is drawn per COMPONENT ID, so that batches that order their components differently (device
    assembly, shards) get the same bar for the same component"""
    comp = np.asarray(info["component"])
    pool = 2 * n_matches + 2                                                         # (a fixed pool: the draws of rbar and wbar do not move with the batch)
    assert len(comp) and 0 <= comp.min() and comp.max() < pool
    cbar, rbar, wbar = VR.bars(pool, n_matches, which)
    return (None if cbar is None else cbar[comp], rbar, wbar)


def _check(out, info, comps, pos, n_nodes, n_matches, variant, bars, what):
    """all four outputs of one call (float64) against the reference at pos; prints the largest error of each in its tolerance"""
    vj = VR.at_positions(comps, info["component"].tolist(), pos, *bars, variant=variant)
    want, unit = VR.match_layout(comps, vj, n_nodes, n_matches, CR.LD)
    worst = {}
    for k in OUT:
        err = np.abs(out[k].astype(CR.LD) - want[k]).astype(np.float64)
        tol = VR.GPU_FACTOR * GAMMA[k] * unit[k]
        ratio = float((err[tol > 0] / tol[tol > 0]).max(initial=0.0))
        worst[k] = ratio
        assert out[k].shape == want[k].shape and np.isfinite(out[k]).all(), (what, k)
        assert (err <= tol).all(), "%s: %s off by %.3g tolerances (%d entries with a zero unit are not 0)" % (what, k, ratio, int((err[tol == 0] != 0).sum()))
    is_var, is_block = np.zeros(n_nodes, bool), np.zeros(2 * n_matches, bool)
    for c in info["component"].tolist():
        is_var[comps[c][0]] = True
        is_block[comps[c][1].eids] = True
    assert (~is_var).any() and not out["positions"][~is_var].any(), what             # constants, unsolved nodes, other shards: exactly 0
    assert not out["disp2"][~is_block[0::2]].any() and not out["disp1"][~is_block[1::2]].any(), what      # directions with weight -1
    assert not out["sim"][~(is_block[0::2] | is_block[1::2])].any(), what
    print("%s: largest error in its tolerance: positions %.4f, disp1 %.4f, disp2 %.4f, sim %.4f"
          % (what, worst["positions"], worst["disp1"], worst["disp2"], worst["sim"]))
    return vj


# ------------------------------------------------------------------------------------------ 1. every kernel class at its limits
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("device_assembly", [False, True], ids=["host", "device"])
def test_every_class_at_its_limits(lfr_lib, device_assembly, which):
    s = TCL.all_solved(device_assembly)
    pos = s.pos if which == "a" else _positions_b(s)
    comps = _components(s.ma, s.g, s.p, s.info)
    M = s.g.n_edges // 2
    assert len(s.info["component"]) == len(CL.NAMES)
    for bset in VR.BAR_SETS:
        bars = _bars_for(s.info, M, bset)
        out = _vjp(s.b, pos, *bars)
        assert out["disp1"].shape == (M, 18) and out["sim"].shape == (M,) and out["positions"].shape == (s.g.n_nodes, 2)
        _check(out, s.info, comps, pos, s.g.n_nodes, M, "ceres1", bars, "class limits/%s/(%s)/%s" % (device_assembly, which, bset))
        if bset == "r":
            assert not out["sim"].any()                                              # residuals do not depend on the similarity
    if which == "b":
        assert (np.abs(pos) > 1.0).any()                                             # nothing is clamped to the box: the reference was not


# ------------------------------------------------------------------------------------------------- 2. a cost bar of 1 alone
def test_cost_bar_one_is_the_evaluates_gradient(lfr_lib):
    s = TCL.all_solved(False)
    comps = _components(s.ma, s.g, s.p, s.info)
    for pos in (s.pos, _positions_b(s)):
        out = _vjp(s.b, pos, np.ones(len(s.info["component"])), want=("positions",))
        assert sorted(out) == ["positions"]
        evals = ER.at_positions(comps, pos)
        for c in s.info["component"].tolist():
            var_nodes, ed = comps[c]
            err = np.abs(out["positions"][var_nodes].astype(CR.LD) - evals[c].grad)
            assert (err <= ER.GPU_FACTOR * ER.GAMMA_GRAD_CPU * evals[c].g_unit).all(), c


# --------------------------------------------------------------------------------------------- 3. losses at work and bounds
@pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
def test_saturated_tukey_edges_pass_the_residual_bar_only(lfr_lib, variant):
    """cost_ref.TUKEY_GRAPH at the solve's positions, whole and under a cap of 12 nodes per component: saturated inter-track edges
    (rho' = 0) and, under the cap, dropped directions - both asserted of the input before the outputs are looked at"""
    for cap, want_absent in ((0, False), (12, True)):
        ma, g, p, b, st, pos = _small(CR.TUKEY_GRAPH, variant, cap)
        info = b.component_info()
        comps = _components(ma, g, p, info)
        M = g.n_edges // 2
        evals = ER.at_positions(comps, pos, variant)
        sat = np.zeros(2 * M, bool)
        for c, ev in evals.items():
            sat[comps[c][1].eids[(ev.rho1 == 0) & (comps[c][1].kind == CR.KIND_INTER)]] = True
        assert sat.any()
        assert (sum(len(ed) for _, ed in comps.values()) < g.n_edges) == want_absent
        bars = _bars_for(info, M, "crw")
        _check(_vjp(b, pos, *bars), info, comps, pos, g.n_nodes, M, variant, bars, "tukey/%s/cap %d" % (variant, cap))
        rows = lambda o: np.where((np.arange(2 * M) % 2 == 0)[:, None], np.repeat(o["disp2"], 2, 0), np.repeat(o["disp1"], 2, 0))      # per directed edge
        cw = _vjp(b, pos, bars[0], None, bars[2])
        assert not rows(cw)[sat].any() and rows(cw)[~sat].any()
        r = _vjp(b, pos, None, bars[1], None)
        assert (np.abs(rows(r)[sat]).sum(1) > 0).all()


def test_coordinates_beyond_the_kink_and_the_box_follow_the_reference(lfr_lib):
    ma, g, p, b, st, pos = _small(CR.BOUNDS_GRAPH)
    info = b.component_info()
    comps = _components(ma, g, p, info)
    M = g.n_edges // 2
    assert (np.abs(pos) == 1.0).sum() >= 10 and (np.abs(pos) > 0.5).any()
    posb = ER.positions_b(comps, g.n_nodes)
    assert (np.abs(posb) > 1.0).any()
    bars = _bars_for(info, M, "crw")
    for x, label in ((pos, "solve"), (posb, "b")):
        out = _vjp(b, x, *bars)
        _check(out, info, comps, x, g.n_nodes, M, "ceres1", bars, "bounds/%s" % label)
    assert (out["positions"][np.abs(posb) > 1.0] != 0).any()                         # not projected, not zeroed


# ------------------------------------------------------------------------------------------------------------ 4. float32
def test_float32_is_the_float64_result_rounded_once(lfr_lib):
    s = TCL.all_solved(False)
    pos = _positions_b(s)
    cbar, rbar, wbar = _bars_for(s.info, s.g.n_edges // 2, "crw")
    rbar, wbar = rbar.astype(np.float32), wbar.astype(np.float32)                  # the float32 call's bars, exactly
    o64 = _vjp(s.b, pos, cbar, rbar.astype(np.float64), wbar.astype(np.float64))
    o32 = _vjp(s.b, pos, cbar, rbar, wbar, f64=False)
    for k in ("disp1", "disp2", "sim"):
        assert o32[k].dtype == np.float32 and np.array_equal(_raw(o32[k]), _raw(o64[k].astype(np.float32))), k
    assert o32["positions"].dtype == np.float64 and np.array_equal(_raw(o32["positions"]), _raw(o64["positions"]))


# ------------------------------------------------------------------------------------------- 5. repeatability and assembly
def test_repeatable_and_the_same_for_every_assembly(lfr_lib):
    h, d = TCL.all_solved(False), TCL.all_solved(True)
    posb = _positions_b(h)
    M = h.g.n_edges // 2
    assert sorted(h.info["component"]) == sorted(d.info["component"])
    outh = _vjp(h.b, posb, *_bars_for(h.info, M, "crw"))
    _assert_same(_vjp(h.b, posb, *_bars_for(h.info, M, "crw")), outh, "second call")
    _assert_same(_vjp(d.b, posb, *_bars_for(d.info, M, "crw")), outh, "device assembly")
    # a device-assembled whole batch: its packed records are gathered from the graph's arrays until something writes them
    ma, _ = CL.all_shapes()
    _, _, fused, _ = _build(ma, "fused")
    fused.solve()
    first = _vjp(fused, posb, *_bars_for(fused.component_info(), M, "crw"))         # this call materialises the records
    _, _, twice, _ = _build(ma, "fused")
    twice.solve()
    twice.solve()                                                                    # the second solve did
    _assert_same(first, _vjp(twice, posb, *_bars_for(twice.component_info(), M, "crw")), "materialised by the call / by the second solve")
    _assert_same(first, outh, "fused")
    x = fused.download().copy()
    fused.solve()                                                                    # the solve after the call reads the records it wrote
    assert np.array_equal(_raw(fused.download()), _raw(x))


# ------------------------------------------------------------------------------------------------------------- 6. isolation
def _assert_others_unchanged(x, y, comps, victim, n_nodes, what):
    """every output outside component `victim` bitwise equal; returns whether anything of the victim is not finite in y"""
    M = x["sim"].shape[0]
    nodes, dirs = np.ones(n_nodes, bool), np.ones(2 * M, bool)
    nodes[comps[victim][0]] = False
    dirs[comps[victim][1].eids] = False
    assert np.array_equal(_raw(x["positions"][nodes]), _raw(y["positions"][nodes])), what
    assert np.array_equal(_raw(x["disp2"][dirs[0::2]]), _raw(y["disp2"][dirs[0::2]])), what
    assert np.array_equal(_raw(x["disp1"][dirs[1::2]]), _raw(y["disp1"][dirs[1::2]])), what
    clean = dirs[0::2] & dirs[1::2]
    assert np.array_equal(_raw(x["sim"][clean]), _raw(y["sim"][clean])), what
    for k in OUT:
        assert np.isfinite(x[k]).all(), (what, k)
    return not all(np.isfinite(y[k]).all() for k in OUT)


def test_a_nan_bar_fails_its_component_alone(lfr_lib):
    mt, g, p, b, comps, names, pos = _twice()
    info = b.component_info()
    M = g.n_edges // 2
    cbar, rbar, wbar = _bars_for(info, M, "crw")
    out = _vjp(b, pos, cbar, rbar, wbar, want_stats=True)
    assert out["stats"]["n_nonfinite"] == 0 and out["stats"]["n_components"] == len(info["component"]) and out["stats"]["kernel_ms"] > 0
    for victim in (names[1]["k7_first_reread"], names[0]["ring46"]):                 # a packed group in the middle of a wave, a workgroup
        eid = int(comps[victim][1].eids[3])
        bad_r = rbar.copy()
        bad_r.reshape(-1, 2)[eid] = np.nan
        bad = _vjp(b, pos, cbar, bad_r, wbar, want_stats=True)
        assert _assert_others_unchanged(out, bad, comps, victim, g.n_nodes, "NaN residual bar") and bad["stats"]["n_nonfinite"] == 1
        row = (bad["disp1"] if eid & 1 else bad["disp2"])[eid >> 1]
        assert np.isnan(row[row != 0]).all() and np.isnan(row).any()
        bad_c = cbar.copy()
        bad_c[int(np.nonzero(info["component"] == victim)[0][0])] = np.nan
        bad = _vjp(b, pos, bad_c, rbar, wbar, want_stats=True)
        assert _assert_others_unchanged(out, bad, comps, victim, g.n_nodes, "NaN cost bar") and bad["stats"]["n_nonfinite"] == 1
        assert np.isnan(bad["positions"][comps[victim][0]]).all()
    _assert_same(_vjp(b, pos, cbar, rbar, wbar), out, "the clean bars again")


# ------------------------------------------------------------------------------------------------------- 7. with set_inputs
def test_new_flows_at_given_positions_and_the_event_waits(lfr_lib):
    ma, _ = CL.all_shapes()
    mb = CL.second_inputs()
    g, p, b, _ = _build(ma, "host")
    b.solve()
    x0 = b.download().copy()
    info = b.component_info()
    M = g.n_edges // 2
    bars = _bars_for(info, M, "crw")
    new = [_dev(mb.disp1), _dev(mb.disp2), _dev(mb.sim, flows=False)]
    old = [_dev(ma.disp1), _dev(ma.disp2), _dev(ma.sim, flows=False)]
    before = _vjp(b, x0, *bars)
    # a fresh batch with the new values from the start (class_limit_cases.second_inputs keeps the structure)
    g2, p2, b2, _ = _build(mb, "host")
    assert np.array_equal(b2.component_info()["component"], info["component"])
    want = _vjp(b2, x0, *bars)
    assert not np.array_equal(_raw(want["disp1"]), _raw(before["disp1"]))
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    tb = [_t(x0)] + [_t(a) for a in bars]
    torch.cuda.synchronize()
    b.set_inputs(*new, stream=s1.cuda_stream)
    got = b.evaluate_vjp(tb[0], cost_bar=tb[1], residuals_bar=tb[2], weights_bar=tb[3], stream=s2.cuda_stream)     # waits for the new inputs
    b.set_inputs(*old, stream=s1.cuda_stream)                                        # waits for the call: the records it read are the new ones
    torch.cuda.synchronize()
    _assert_same({k: v.cpu().numpy() for k, v in got.items()}, want, "new flows on another stream, no solve in between")
    _check(want, info, _components(mb, g, p, info), x0, g.n_nodes, M, "ceres1", bars, "new flows at the old positions")
    _assert_same(_vjp(b, x0, *bars), before, "the old flows again")


# ------------------------------------------------------------------------------------------------- 8. shards and cc-sharding
def test_shards_cover_the_outputs_once(lfr_lib):
    s = TCL.all_solved(False)
    posb = _positions_b(s)
    M = s.g.n_edges // 2
    full = _vjp(s.b, posb, *_bars_for(s.info, M, "crw"))
    total = {k: np.zeros_like(full[k]) for k in OUT}
    comps = _components(s.ma, s.g, s.p)
    for rank in range(2):
        b = capi.Batch(s.p, 0, rank, 2)
        info = b.component_info()
        bars = _bars_for(info, M, "crw")
        o = _vjp(b, posb, *bars)
        _check(o, info, comps, posb, s.g.n_nodes, M, "ceres1", bars, "shard %d of 2" % rank)
        for k in OUT:
            assert not ((total[k] != 0) & (o[k] != 0)).any(), (rank, k)
            total[k] += o[k]
    for k in OUT:
        assert np.array_equal(total[k], full[k]) and full[k].any(), k                # (x + 0 is exact: bitwise per component)


def test_cc_sharded_batches_serve_the_cost_bar_alone(lfr_lib):
    mc = synthetic.generate(seed=32, n_images=48, n_tracks=3000, eps_out=0.002)
    g2 = capi.Graph.from_arrays(mc)
    p2 = capi.Problem(g2, device_graph_stage=0, shard=(0, 2))
    assert p2.cc_sharded
    b2 = capi.Batch(p2, 0)
    M = g2.n_edges // 2
    zeros = np.zeros((g2.n_nodes, 2))
    cbar = np.ones(len(b2.component_info()["component"]))
    for kw in (dict(want=("positions", "disp")), dict(want=("sim",)), dict(want=("positions",), rbar=np.zeros((M, 2, 2))),
               dict(want=("positions",), wbar=np.zeros((M, 2)))):
        with pytest.raises(capi.LfrError) as e:
            _vjp(b2, zeros, cbar, **kw)
        assert e.value.code == -5
    o = _vjp(b2, zeros, cbar, want=("positions",), want_stats=True)
    assert np.isfinite(o["positions"]).all() and o["positions"].any() and o["stats"]["n_nonfinite"] == 0
    ev = b2.evaluate(_t(zeros), residuals=False, weights=False)
    assert np.allclose(o["positions"], ev["grad"].cpu().numpy(), rtol=1e-12, atol=1e-15)


# --------------------------------------------------------------------------------------------------------- 9. arguments
def test_argument_errors_come_before_any_output_is_touched(lfr_lib):
    s = TCL.all_solved(False)
    L = capi.lib()
    N, M, nc = s.g.n_nodes, s.g.n_edges // 2, len(s.info["component"])
    sent = 7.0
    gp, g1, g2, gs = (torch.full(shape, sent, dtype=torch.float64, device=DEV) for shape in ((N, 2), (M, 18), (M, 18), (M,)))
    cb, rb, wb = torch.ones(nc, dtype=torch.float64, device=DEV), torch.zeros((M, 4), dtype=torch.float64, device=DEV), torch.zeros((M, 2), dtype=torch.float64, device=DEV)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    call = lambda h, pos, c, r, w, o0, o1, o2, o3, flags: L.lfr_batch_evaluate_vjp(h, ptr(pos), ptr(c), ptr(r), ptr(w), ptr(o0), ptr(o1), ptr(o2), ptr(o3), flags, None, None)
    ma, _ = CL.all_shapes()
    _, _, unsolved, _ = _build(ma, "host")
    cases = {
        "no batch": (None, None, cb, rb, wb, gp, g1, g2, gs, 1),
        "unknown flag bit": (s.b._h, None, cb, rb, wb, gp, g1, g2, gs, 1 | 2),
        "all three bars NULL": (s.b._h, None, None, None, None, gp, g1, g2, gs, 1),
        "all four outputs NULL": (s.b._h, None, cb, rb, wb, None, None, None, None, 1),
        "grad_disp1 without grad_disp2": (s.b._h, None, cb, rb, wb, gp, g1, None, gs, 1),
        "grad_disp2 without grad_disp1": (s.b._h, None, cb, rb, wb, gp, None, g2, gs, 1),
        "NULL positions before the first solve": (unsolved._h, None, cb, rb, wb, gp, g1, g2, gs, 1),
    }
    for what, args in cases.items():
        assert call(*args) == -1, what
        torch.cuda.synchronize()
        for t in (gp, g1, g2, gs):
            assert bool((t == sent).all()), what
    assert call(s.b._h, None, cb, None, None, gp, None, None, None, 0) == 0           # NULL positions after a solve: the batch's own
    torch.cuda.synchronize()
    assert np.array_equal(_raw(gp.cpu().numpy()), _raw(_vjp(s.b, s.pos, np.ones(nc), want=("positions",))["positions"]))
    posb = _positions_b(s)
    assert call(unsolved._h, _t(posb), cb, rb, wb, gp, g1, g2, gs, 1) == 0            # explicit positions need no solve
    torch.cuda.synchronize()
    assert np.array_equal(_raw(gp.cpu().numpy()), _raw(_vjp(s.b, posb, np.ones(nc), want=("positions",))["positions"]))
    for bad in (dict(want=()), dict(want=("grad",))):
        with pytest.raises(ValueError):
            s.b.evaluate_vjp(cost_bar=cb, **bad)
    with pytest.raises(ValueError):
        s.b.evaluate_vjp(cost_bar=cb.float())


# --------------------------------------------------------------------------------------------------- 10. Refiner.objective
def _leaf(x, flows=True):
    return _dev(x, flows).requires_grad_(True)


def test_refiner_objective_adds_the_explicit_part(lfr_lib):
    ma = synthetic.generate(seed=41, n_images=12, n_tracks=120)
    banned = ("000005.png",)
    r = Refiner(_dev(ma.disp1), _dev(ma.disp2), _dev(ma.sim, flows=False), banned=banned, **_meta(ma))
    rows = _kept_rows(ma.pair_img1, ma.pair_img2, ma.pair_off, list(ma.image_names), banned)
    gone = np.ones(ma.n_matches, bool)
    gone[rows] = False
    assert gone.any()
    idx = torch.as_tensor(rows, device=DEV)

    def to_rows(t):
        full = torch.zeros((ma.n_matches,) + tuple(t.shape[1:]), dtype=t.dtype, device=DEV)
        full[idx] = t
        return full

    d1, d2, sm = _leaf(ma.disp1), _leaf(ma.disp2), _leaf(ma.sim, flows=False)
    with pytest.raises(RuntimeError):
        r.objective(torch.zeros((r.n_nodes, 2), dtype=torch.float64, device=DEV), d1, d2, sm)      # before the first forward
    pos = r(d1, d2, sm)
    nc = len(r._batch.component_info()["component"])
    # the explicit part alone: detached positions
    out = r.objective(pos.detach(), d1, d2, sm)
    assert sorted(out) == ["cost"] and out["cost"].dtype == torch.float64 and out["cost"].shape == (nc,)
    assert torch.equal(out["cost"].detach(), r.evaluate()["cost"])
    out["cost"].sum().backward()
    ex = r._batch.evaluate_vjp(pos.detach(), cost_bar=torch.ones(nc, dtype=torch.float64, device=DEV))
    explicit = {"d1": to_rows(ex["disp1"]).float(), "d2": to_rows(ex["disp2"]).float(), "sm": to_rows(ex["sim"]).float()}
    for t, k in ((d1, "d1"), (d2, "d2"), (sm, "sm")):
        assert t.grad.dtype == torch.float32 and torch.equal(t.grad, explicit[k].reshape(t.shape)) and bool(t.grad.any()), k
        assert not bool(t.grad[torch.as_tensor(gone)].any()), k
        t.grad = None
    # with the positions attached autograd adds J^T dF/dx from lfr_batch_backward, in float32
    r.objective(pos, d1, d2, sm)["cost"].sum().backward()
    # dL/dx of sum F is dF/dx.  Autograd hands lfr_batch_backward the vjp's own position gradient: bitwise with that one.  The
    # evaluate's "grad" is the same vector from other roundings (2^-53 relative per term); the backward is linear in it and its
    # outputs are float32, so the two sums agree to a few float32 roundings of the largest entry: 1e-5 of it
    via_vjp = r._batch.backward(ex["positions"], f64=False)
    via_eval = r._batch.backward(r.evaluate()["grad"], f64=False)
    for t, k, a, e in ((d1, "d1", via_vjp[0], via_eval[0]), (d2, "d2", via_vjp[1], via_eval[1]), (sm, "sm", via_vjp[2], via_eval[2])):
        assert torch.equal(t.grad, explicit[k].reshape(t.shape) + to_rows(a).reshape(t.shape)), k
        want = explicit[k].reshape(t.shape) + to_rows(e).reshape(t.shape)
        assert float((t.grad - want).abs().max()) <= 1e-5 * float(want.abs().max()) and bool(to_rows(e).any()), k
        t.grad = None
    # residuals and weights back-propagate a random bar to the Batch call's values
    out = r.objective(pos.detach(), d1, d2, sm, residuals=True, weights=True)
    assert out["residuals"].shape == (ma.n_matches, 2, 2) and out["weights"].shape == (ma.n_matches, 2) and out["weights"].dtype == torch.float64
    assert bool((out["weights"][torch.as_tensor(gone)] == -1).all())
    rng = np.random.default_rng(5)
    rbar, wbar = _t(rng.standard_normal((ma.n_matches, 2, 2))), _t(rng.standard_normal((ma.n_matches, 2)))
    ((out["residuals"] * rbar).sum() + (out["weights"] * wbar).sum()).backward()
    ex = r._batch.evaluate_vjp(pos.detach(), residuals_bar=rbar[idx].contiguous(), weights_bar=wbar[idx].contiguous())
    assert torch.equal(d1.grad, to_rows(ex["disp1"]).float()) and torch.equal(d2.grad, to_rows(ex["disp2"]).float()) and bool(d1.grad.any())
    assert not bool(sm.grad.any())
    # other tensors than the latest forward's; a backward after a newer forward
    with pytest.raises(ValueError):
        r.objective(pos.detach(), _leaf(ma.disp1), d2, sm)
    with pytest.raises(ValueError):
        r.objective(pos.detach(), d1, d2, None)
    stale = r.objective(pos.detach(), d1, d2, sm)["cost"].sum()
    r(d1, d2, sm)
    with pytest.raises(RuntimeError) as e:
        stale.backward()
    assert "stale" in str(e.value)
    r.close()
