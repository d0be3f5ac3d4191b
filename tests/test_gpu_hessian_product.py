"""lfr_batch_hessian_product (include/lfr.h) against tests/hessian_product_ref.py: H v and v . H v of every launch class on its row and
edge limits, exact and Gauss-Newton, one vector and four, at two position sets - (a) the solve's own, (b) evaluate_ref.positions_b -
and the call's contract: Tukey saturation, the free set, no row limit, the algebra of a symmetric operator, the round trip with
lfr_batch_jvp, repeatability and isolation bit for bit, lfr_batch_set_inputs, shards, arguments, Refiner.hessian_product.

Tolerances: products and curvature within 8 x the fp64 constants measured by tests/test_hessian_product_ref.py, in the units of
tests/hessian_product_ref.py; the round trip within 8 x the relative residual that file measures on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import backward_ref as BR
import class_limit_cases as CL
import cost_ref as CR
import evaluate_ref as ER
import hessian_product_ref as HR
import jvp_ref as JR
import match_covariance_ref as MR
import test_gpu_class_limits as TCL
from test_gpu_backward import _nodes
from test_gpu_evaluate import _components, _raw, _small, _twice
from test_gpu_jvp import _jvp, _tangents
from test_gpu_set_inputs import _build, _dev, _flows18, _meta
from lfr_amd import capi, synthetic
from lfr_amd.autograd import Refiner

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LD = CR.LD
MODES = pytest.mark.parametrize("gn", [False, True], ids=["exact", "gauss_newton"])
_cache = {}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device=DEV)


def _hp(b, v, pos=None, **kw):
    kw.setdefault("curvature", True)
    out = b.hessian_product(_t(v), None if pos is None else _t(pos), **kw)
    torch.cuda.synchronize()
    return {k: (x.cpu().numpy() if isinstance(x, torch.Tensor) else x) for k, x in out.items()}


def _same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_raw(x), _raw(y))


def _reference(key, comps, pos, vs, variant, gn, fs):
    """{component: [Hvp per vector]}, computed once per key"""
    if key not in _cache:
        _cache[key] = {c: [HR.product(ed, pos[var_nodes], v[var_nodes], variant, gn, fs) for v in vs] for c, (var_nodes, ed) in comps.items()}
    return _cache[key]


def _check(out, info, comps, ref, n_nodes, which, what):
    """products [K, n, 2] and curvature [K, nc] of the vectors `which` (indices into the reference's) within the tolerance"""
    worst = {"products": 0.0, "curvature": 0.0}
    is_var = np.zeros(n_nodes, bool)
    prod, curv = out["products"].reshape(len(which), n_nodes, 2), out["curvature"].reshape(len(which), -1)
    assert curv.shape[1] == len(info["component"])
    for i, c in enumerate(info["component"].tolist()):
        var_nodes, ed = comps[c]
        is_var[var_nodes] = True
        for k, kv in enumerate(which):
            r = ref[c][kv]
            err, tol = np.abs(prod[k][var_nodes].astype(LD) - r.hv), HR.GPU_FACTOR * HR.GAMMA_HVP_CPU * r.hv_unit
            ratio = float((err[tol > 0] / tol[tol > 0]).max(initial=0.0))
            assert np.isfinite(prod[k][var_nodes]).all() and (err <= tol).all(), "%s, component %d, vector %d: product off by %.3g tolerances" % (what, c, kv, ratio)
            worst["products"] = max(worst["products"], ratio)
            e, t = abs(LD(curv[k, i]) - r.curvature), HR.GPU_FACTOR * HR.GAMMA_CURV_CPU * r.curv_unit
            assert e <= t, "%s, component %d, vector %d: curvature %.17g, reference %.17g, %.3g tolerances" % (what, c, kv, curv[k, i], float(r.curvature), float(e / t))
            worst["curvature"] = max(worst["curvature"], float(e / t) if t > 0 else 0.0)
    assert not prod[:, ~is_var].any(), what                                          # constants, unsolved nodes, other shards: exactly 0
    print("%s: largest error in its tolerance: products %.4f, curvature %.4f" % (what, worst["products"], worst["curvature"]))
    return worst


def _positions(s, which):
    return s.pos if which == "a" else ER.positions_b(_components(s.ma, s.g, s.p), s.g.n_nodes)


# ------------------------------------------------------------------------------------------ 1. every launch class at its limits
@MODES
@pytest.mark.parametrize("which", ["a", "b"])
def test_every_class_at_its_limits(lfr_lib, which, gn):
    s = TCL.all_solved()
    pos, vs = _positions(s, which), HR.vectors(s.g.n_nodes)
    comps = _components(s.ma, s.g, s.p, s.info)
    ref = _reference(("cl", which, gn), comps, pos, vs, "ceres1", gn, False)
    four = _hp(s.b, vs, pos, gauss_newton=gn, want_stats=True)
    assert four["products"].shape == (4, s.g.n_nodes, 2) and four["curvature"].shape == (4, len(CL.NAMES))
    assert four["stats"] == dict(four["stats"], n_components=len(CL.NAMES), n_nonfinite=0, n_bound_coordinates=0) and four["stats"]["kernel_ms"] > 0
    _check(four, s.info, comps, ref, s.g.n_nodes, [0, 1, 2, 3], "class limits/%s/(%s)/K=4" % ("gn" if gn else "exact", which))
    one = _hp(s.b, vs[0], pos, gauss_newton=gn)
    assert one["products"].shape == (s.g.n_nodes, 2) and one["curvature"].shape == (len(CL.NAMES),)
    _check(one, s.info, comps, ref, s.g.n_nodes, [0], "class limits/%s/(%s)/K=1" % ("gn" if gn else "exact", which))
    if which == "b":
        assert (np.abs(pos) > 1.0).any() and (np.abs(pos) == 0.5).any()             # nothing is clamped; the kink is met


@MODES
def test_every_class_twice_in_shared_waves(lfr_lib, gn):
    mt, g, p, b, comps, names, posb = _twice()
    if "twice_solved" not in _cache:
        b.solve()
        _cache["twice_solved"] = b.download().copy()
    info, vs = b.component_info(), HR.vectors(g.n_nodes)
    for which, pos in (("a", _cache["twice_solved"]), ("b", posb)):
        ref = _reference(("twice", which, gn), comps, pos, vs, "ceres1", gn, False)
        for sel in ([0, 1, 2, 3], [0]):
            out = _hp(b, vs[sel], pos, gauss_newton=gn)
            _check(out, info, comps, ref, g.n_nodes, sel, "twice/%s/(%s)/K=%d" % ("gn" if gn else "exact", which, len(sel)))


# --------------------------------------------------------------------------------------------- 2. losses at work and bounds
@pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
def test_saturated_tukey_edges_contribute_nothing(lfr_lib, variant):
    for cap in (0, 12):
        ma, g, p, b, st, pos = _small(CR.TUKEY_GRAPH, variant, cap)
        info = b.component_info()
        comps = _components(ma, g, p, info)
        evals = ER.at_positions(comps, pos, variant)
        assert any((ev.rho1[comps[c][1].kind == CR.KIND_INTER] == 0).any() for c, ev in evals.items())
        vs = HR.vectors(g.n_nodes, 2)
        for gn in (False, True):
            ref = {c: [HR.product(ed, pos[vn], v[vn], variant, gn) for v in vs] for c, (vn, ed) in comps.items()}
            _check(_hp(b, vs, pos, gauss_newton=gn), info, comps, ref, g.n_nodes, [0, 1], "tukey/%s/cap %d/%s" % (variant, cap, "gn" if gn else "exact"))
            # the same components with their saturated edges taken out: the reference does not move by a bit
            for c, (vn, ed) in comps.items():
                sat = (ed.kind == CR.KIND_INTER) & (evals[c].rho1 == 0)
                if sat.any():
                    k = ~sat
                    cut = CR.Edges(ed.nv, ed.src[k], ed.dst[k], ed.w[k], ed.kind[k], ed.flow[k], ed.eids[k])
                    assert np.array_equal(HR.product(cut, pos[vn], vs[0][vn], variant, gn).hv, ref[c][0].hv)


def test_free_set_makes_identity_rows_and_columns(lfr_lib):
    ma, g, p, b, st, pos = _small(CR.BOUNDS_GRAPH)
    info = b.component_info()
    comps = _components(ma, g, p, info)
    vs = HR.vectors(g.n_nodes, 2)
    is_var = np.zeros(g.n_nodes, bool)
    for vn, _ in comps.values():
        is_var[vn] = True
    at_bound = (np.abs(pos) >= 1.0) & is_var[:, None]
    assert at_bound.sum() >= 10
    for gn in (False, True):
        free = {c: [HR.product(ed, pos[vn], v[vn], "ceres1", gn, True) for v in vs] for c, (vn, ed) in comps.items()}
        whole = {c: [HR.product(ed, pos[vn], v[vn], "ceres1", gn, False) for v in vs] for c, (vn, ed) in comps.items()}
        out = _hp(b, vs, pos, gauss_newton=gn, free_set=True, want_stats=True)
        _check(out, info, comps, free, g.n_nodes, [0, 1], "bounds/free set/%s" % ("gn" if gn else "exact"))
        assert out["stats"]["n_bound_coordinates"] == int(at_bound.sum()) == sum(r[0].n_bound for r in free.values())
        assert np.array_equal(_raw(out["products"][:, at_bound]), _raw(vs[:, at_bound]))          # (H v)_i = v_i, the very bits
        moved = vs.copy()
        moved[:, at_bound] += 3.0                                                                  # v_i enters no other row
        again = _hp(b, moved, pos, gauss_newton=gn, free_set=True)
        assert np.array_equal(_raw(again["products"][:, ~at_bound]), _raw(out["products"][:, ~at_bound]))
        plain = _hp(b, vs, pos, gauss_newton=gn, want_stats=True)
        _check(plain, info, comps, whole, g.n_nodes, [0, 1], "bounds/whole set/%s" % ("gn" if gn else "exact"))
        assert plain["stats"]["n_bound_coordinates"] == 0 and not _same(plain["products"], out["products"])


# ------------------------------------------------------------------------------------------------------------ 3. no row limit
def _ring_6146():
    if "ring" not in _cache:
        ma = TCL._ring(3074)
        g = capi.Graph.from_arrays(ma)
        p = capi.Problem(g)
        b = capi.Batch(p, 0)
        st = b.solve()
        info = b.component_info()
        assert info["n_var_nodes"].tolist() == [3073] and st["n_failed"] == 0
        _cache["ring"] = (ma, g, p, b, b.download().copy(), info)
    return _cache["ring"]


@MODES
def test_a_ring_of_6146_rows(lfr_lib, gn):
    """two rows more than the dense factorization of the backward serves: that answers LFR_ERR_UNSUPPORTED, the product is served"""
    ma, g, p, b, pos, info = _ring_6146()
    with pytest.raises(capi.LfrError) as e:
        b.backward(torch.zeros((g.n_nodes, 2), dtype=torch.float64, device=DEV))
    assert e.value.code == -5
    comps = _components(ma, g, p, info)
    vs = HR.vectors(g.n_nodes, 2)
    ref = {c: [HR.product(ed, pos[vn], v[vn], "ceres1", gn) for v in vs] for c, (vn, ed) in comps.items()}
    _check(_hp(b, vs, pos, gauss_newton=gn), info, comps, ref, g.n_nodes, [0, 1], "ring of 6146 rows/%s" % ("gn" if gn else "exact"))


@MODES
def test_a_tree_class_component(lfr_lib, gn):
    ma, g, p, b, st, pos = _small(dict(n_images=1344, n_tracks=MR.CAPSIZED_SMALLEST, seed=7, track_degree=4, chain_links=1, eps_out=0.0005, ratio_sims=True))
    info = b.component_info()
    assert (2 * info["n_var_nodes"]).max() > CL.MAX_BLOCK_ROWS
    comps = _components(ma, g, p, info)
    vs = HR.vectors(g.n_nodes, 2)
    ref = {c: [HR.product(ed, pos[vn], v[vn], "ceres1", gn) for v in vs] for c, (vn, ed) in comps.items()}
    _check(_hp(b, vs, pos, gauss_newton=gn), info, comps, ref, g.n_nodes, [0, 1], "tree class/%s" % ("gn" if gn else "exact"))


# ------------------------------------------------------------------------------------------------ 4. algebra on the GPU alone
def test_symmetry_curvature_definiteness_and_zero(lfr_lib):
    s = TCL.all_solved()
    comps = _components(s.ma, s.g, s.p, s.info)
    posb = _positions(s, "b")
    vs = HR.vectors(s.g.n_nodes)
    for pos, which in ((s.pos, "a"), (posb, "b")):
        for gn in (False, True):
            ref = _reference(("cl", which, gn), comps, pos, vs, "ceres1", gn, False)
            out = _hp(s.b, vs, pos, gauss_newton=gn)
            for i, c in enumerate(s.info["component"].tolist()):
                vn, _ = comps[c]
                u, v, hu, hv = vs[0][vn], vs[1][vn], out["products"][0][vn], out["products"][1][vn]
                unit = HR.GPU_FACTOR * HR.GAMMA_HVP_CPU * ((np.abs(u) * ref[c][1].hv_unit).sum() + (np.abs(v) * ref[c][0].hv_unit).sum())
                unit += CR.U * 4 * len(vn) * (np.abs(u * hv).sum() + np.abs(v * hu).sum())       # (the two dot products taken here, in fp64)
                assert abs(LD((u * hv).sum()) - LD((v * hu).sum())) <= unit, (which, gn, c)
                for k in range(4):
                    vk, hk = vs[k][vn], out["products"][k][vn]
                    dot = (vk.astype(LD) * hk.astype(LD)).sum()
                    assert abs(LD(out["curvature"][k, i]) - dot) <= CR.U * (2 * len(vn) + 1) * np.abs(vk * hk).sum(), (which, gn, c, k)
                    if gn:
                        assert out["curvature"][k, i] >= -HR.GPU_FACTOR * HR.GAMMA_CURV_CPU * float(ref[c][k].curv_unit), (which, c, k)
            zero = _hp(s.b, np.zeros((2, s.g.n_nodes, 2)), pos, gauss_newton=gn)
            assert not zero["products"].any() and not zero["curvature"].any()


# --------------------------------------------------------------------------------------------- 5. round trip with lfr_batch_jvp
@MODES
def test_round_trip_with_the_jvp(lfr_lib, gn):
    """H xdot = b: xdot from lfr_batch_jvp (float64 tangents), b = jvp_ref.rhs on the free set, H through the product with the free
    set at the batch's positions.  |H xdot - b|_2 <= 8 x ROUND_TRIP_REL_CPU |b|_2 per component with status 0"""
    s = TCL.all_solved()
    ts = _tangents(s.ma, 41)
    xdot = _jvp(s.b, ts, gn)
    status = s.b.jvp_status()
    assert (status == capi.JVP_OK).all()
    out = _hp(s.b, xdot, None, gauss_newton=gn, free_set=True, curvature=False)
    comps = BR.graph_components(s.ma, *s.p.labels(), *_nodes(s.g, s.ma))
    worst = 0.0
    for c in s.info["component"].tolist():
        vn, cp = comps[c]
        x = s.pos[vn].reshape(-1)
        m, odd = cp.eids >> 1, (cp.eids & 1) == 1
        want = np.where(cp.free(x), JR.rhs(cp, x, np.where(odd[:, None], ts[0][m], ts[1][m]), ts[2][m]), 0.0)
        rel = float(np.linalg.norm(out["products"][vn].reshape(-1) - want) / np.linalg.norm(want))
        worst = max(worst, rel)
        assert rel <= HR.GPU_FACTOR * HR.ROUND_TRIP_REL_CPU, "component %d: relative residual %.3e, bound %.3e" % (c, rel, HR.GPU_FACTOR * HR.ROUND_TRIP_REL_CPU)
    print("round trip %s: largest relative residual %.3e (bound %.3e)" % ("gn" if gn else "exact", worst, HR.GPU_FACTOR * HR.ROUND_TRIP_REL_CPU))


# ------------------------------------------------------------------------------------------------------------------ 6. bitwise
def test_repeatable_and_the_same_for_every_assembly(lfr_lib):
    h, d = TCL.all_solved(False), TCL.all_solved(True)
    posb, vs = _positions(h, "b"), HR.vectors(h.g.n_nodes)
    order = [int(np.nonzero(d.info["component"] == c)[0][0]) for c in h.info["component"]]
    ma, _ = CL.all_shapes()
    _, _, fused, _ = _build(ma, "fused")
    fused.solve()
    _, _, twice, _ = _build(ma, "fused")
    twice.solve()
    twice.solve()                                      # the second solve materialised the records
    for gn in (False, True):
        first = _hp(h.b, vs, posb, gauss_newton=gn)
        second = _hp(h.b, vs, posb, gauss_newton=gn)
        assert _same(first["products"], second["products"]) and _same(first["curvature"], second["curvature"])
        dev = _hp(d.b, vs, posb, gauss_newton=gn)
        assert _same(first["products"], dev["products"]) and _same(first["curvature"], dev["curvature"][:, order])
        f = _hp(fused, vs, posb, gauss_newton=gn)      # (the first of these calls materialises the records)
        t = _hp(twice, vs, posb, gauss_newton=gn)
        assert _same(f["products"], t["products"]) and _same(f["curvature"], t["curvature"])
        assert _same(f["products"], dev["products"]) and _same(f["curvature"], dev["curvature"])
        # vector k alone, among random others, among NaNs
        for k in range(4):
            alone = _hp(h.b, vs[k], posb, gauss_newton=gn)
            assert _same(alone["products"], first["products"][k]) and _same(alone["curvature"], first["curvature"][k]), (gn, k)
            for fill in (HR.vectors(h.g.n_nodes, 4, seed=9300 + k), np.full(vs.shape, np.nan)):
                mixed = fill.copy()
                slot = (k + 1) % 4
                mixed[slot] = vs[k]
                among = _hp(h.b, mixed, posb, gauss_newton=gn)
                assert _same(among["products"][slot], first["products"][k]) and _same(among["curvature"][slot], first["curvature"][k]), (gn, k)


def test_a_nan_fails_its_component_alone(lfr_lib):
    mt, g, p, b, comps, names, pos = _twice()
    info, vs = b.component_info(), HR.vectors(g.n_nodes)
    for gn in (False, True):
        out = _hp(b, vs, pos, gauss_newton=gn, want_stats=True)
        assert out["stats"]["n_nonfinite"] == 0 and out["stats"]["n_components"] == len(info["component"])
        for victim in (names[1]["k7_first_reread"], names[0]["k5"], names[1]["k14"], names[0]["ring46"], names[1]["k98"]):
            rows = info["component"] != victim
            nodes = np.ones(g.n_nodes, bool)
            nodes[comps[victim][0]] = False
            # a vector entry
            bad_v = vs.copy()
            bad_v[2, comps[victim][0][1], 0] = np.nan
            bad = _hp(b, bad_v, pos, gauss_newton=gn, want_stats=True)
            assert bad["stats"]["n_nonfinite"] == 1 and not np.isfinite(bad["curvature"][2, ~rows]).any()
            assert np.array_equal(_raw(bad["products"][:, nodes]), _raw(out["products"][:, nodes]))
            assert np.array_equal(_raw(bad["curvature"][:, rows]), _raw(out["curvature"][:, rows]))
            for k in (0, 1, 3):                                                      # the victim's other vectors too
                assert np.array_equal(_raw(bad["products"][k]), _raw(out["products"][k]))
            # a flow
            eid = int(comps[victim][1].eids[3])
            d1, d2 = _flows18(mt.disp1).copy(), _flows18(mt.disp2).copy()
            (d1 if eid & 1 else d2)[eid >> 1, 8] = np.nan
            b.set_inputs(_dev(d1), _dev(d2))
            bad = _hp(b, vs, pos, gauss_newton=gn, want_stats=True)
            b.set_inputs(_dev(mt.disp1), _dev(mt.disp2))
            assert bad["stats"]["n_nonfinite"] == 1 and not np.isfinite(bad["products"][:, ~nodes]).all()
            assert np.array_equal(_raw(bad["products"][:, nodes]), _raw(out["products"][:, nodes]))
            assert np.array_equal(_raw(bad["curvature"][:, rows]), _raw(out["curvature"][:, rows]))
        again = _hp(b, vs, pos, gauss_newton=gn)
        assert _same(again["products"], out["products"]) and _same(again["curvature"], out["curvature"])


# -------------------------------------------------------------------------------------------------------------------- 7. state
def test_new_flows_at_the_held_positions_and_explicit_positions_before_a_solve(lfr_lib):
    ma, _ = CL.all_shapes()
    mb = CL.second_inputs()
    g, p, b, _ = _build(ma, "host")
    vs = HR.vectors(g.n_nodes, 2)
    with pytest.raises(capi.LfrError) as e:
        b.hessian_product(_t(vs))                                                    # NULL positions before the first solve
    assert e.value.code == -1
    comps = _components(ma, g, p)
    info = b.component_info()
    posb = ER.positions_b(comps, g.n_nodes)
    ref = {c: [HR.product(ed, posb[vn], v[vn]) for v in vs] for c, (vn, ed) in comps.items()}
    _check(_hp(b, vs, posb), info, comps, ref, g.n_nodes, [0, 1], "explicit positions before the first solve")
    b.solve()
    x0 = b.download().copy()
    b.set_inputs(_dev(mb.disp1), _dev(mb.disp2), _dev(mb.sim, flows=False))
    compsb = _components(mb, g, p, info)
    ref = {c: [HR.product(ed, x0[vn], v[vn]) for v in vs] for c, (vn, ed) in compsb.items()}
    _check(_hp(b, vs, None), info, compsb, ref, g.n_nodes, [0, 1], "new flows at the held positions")
    # set_inputs waits for the product: on two streams, without a host synchronisation in between
    want = _hp(b, vs, None)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    got = b.hessian_product(_t(vs), None, curvature=True, stream=s1.cuda_stream)
    b.set_inputs(_dev(ma.disp1), _dev(ma.disp2), _dev(ma.sim, flows=False), stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert _same(got["products"].cpu().numpy(), want["products"]) and _same(got["curvature"].cpu().numpy(), want["curvature"])


def test_shards(lfr_lib):
    s = TCL.all_solved()
    posb, vs = _positions(s, "b"), HR.vectors(s.g.n_nodes, 2)
    whole = _hp(s.b, vs, posb)
    seen = np.zeros(s.g.n_nodes, bool)
    for rank in range(2):
        b = capi.Batch(s.p, 0, rank, 2)
        info = b.component_info()
        comps = _components(s.ma, s.g, s.p, info)
        ref = {c: [HR.product(ed, posb[vn], v[vn]) for v in vs] for c, (vn, ed) in comps.items()}
        o = _hp(b, vs, posb)
        _check(o, info, comps, ref, s.g.n_nodes, [0, 1], "shard %d of 2" % rank)
        mine = np.zeros(s.g.n_nodes, bool)
        for vn, _ in comps.values():
            mine[vn] = True
        assert not (seen & mine).any() and np.array_equal(_raw(o["products"][:, mine]), _raw(whole["products"][:, mine]))
        seen |= mine
    assert seen.sum() == sum(len(vn) for vn, _ in _components(s.ma, s.g, s.p, s.info).values())
    # a batch over one rank's connected components is served: everything is per node
    mc = synthetic.generate(seed=32, n_images=48, n_tracks=3000, eps_out=0.002)
    g2 = capi.Graph.from_arrays(mc)
    p2 = capi.Problem(g2, device_graph_stage=0, shard=(0, 2))
    assert p2.cc_sharded
    b2 = capi.Batch(p2, 0)
    b2.solve()
    v2 = HR.vectors(g2.n_nodes, 1)
    o = _hp(b2, v2, None, gauss_newton=True, want_stats=True)
    info2 = b2.component_info()
    assert o["stats"]["n_nonfinite"] == 0 and o["stats"]["n_components"] == len(info2["component"]) == o["curvature"].shape[1]
    assert o["products"].any() and np.isfinite(o["products"]).all() and (o["curvature"] > 0).all()


# ---------------------------------------------------------------------------------------------------------------- 8. arguments
def test_argument_errors_touch_no_output(lfr_lib):
    s = TCL.all_solved()
    L = capi.lib()
    n, nc = s.g.n_nodes, len(s.info["component"])
    v = _t(HR.vectors(n))
    prod = torch.full((4, n, 2), 7.0, dtype=torch.float64, device=DEV)
    curv = torch.full((4, nc), 7.0, dtype=torch.float64, device=DEV)
    pv, pp, pc = C.c_void_p(v.data_ptr()), C.c_void_p(prod.data_ptr()), C.c_void_p(curv.data_ptr())
    call = lambda vec, k, p_, c_, flags: L.lfr_batch_hessian_product(s.b._h, None, vec, k, p_, c_, flags, None, None)
    for args in ((pv, 1, None, None, 0), (None, 1, pp, pc, 0), (pv, 0, pp, pc, 0), (pv, 5, pp, pc, 0), (pv, -1, pp, pc, 0), (pv, 1, pp, pc, 1),
                 (pv, 1, pp, pc, 8), (pv, 1, pp, pc, 2 | 4 | 16)):
        assert call(*args) == -1, args[1:]
        torch.cuda.synchronize()
        assert bool((prod == 7.0).all()) and bool((curv == 7.0).all()), args[1:]
    assert L.lfr_batch_hessian_product(None, None, pv, 1, pp, pc, 0, None, None) == -1
    assert call(pv, 4, pp, pc, 2 | 4) == 0
    torch.cuda.synchronize()
    want = _hp(s.b, v.cpu().numpy(), None, gauss_newton=True, free_set=True)
    assert _same(prod.cpu().numpy(), want["products"]) and _same(curv.cpu().numpy(), want["curvature"])
    only = _hp(s.b, v.cpu().numpy(), None, gauss_newton=True, free_set=True, products=False)      # either output alone: the same bits
    assert sorted(only) == ["curvature"] and _same(only["curvature"], want["curvature"])
    with pytest.raises(capi.LfrError) as e:
        s.b.hessian_product(v, products=False, curvature=False)
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------------------------- 9. Python
def test_refiner_hessian_product_and_argument_checks(lfr_lib):
    ma = synthetic.generate(seed=41, n_images=12, n_tracks=120)
    r = Refiner(_dev(ma.disp1), _dev(ma.disp2), _dev(ma.sim, flows=False), banned=("000005.png",), **_meta(ma))
    x = r(_dev(ma.disp1), _dev(ma.disp2))
    n = r.n_nodes
    vs = _t(HR.vectors(n, 3)).requires_grad_(True)
    for kw in (dict(), dict(gauss_newton=True, free_set=True, curvature=True)):
        out = r.hessian_product(vs, **kw)
        inner = r._batch.hessian_product(vs.detach(), **kw)
        at = r.hessian_product(vs, x, **kw)
        torch.cuda.synchronize()
        assert sorted(out) == sorted(inner) and out["products"].shape == (3, n, 2) and bool(out["products"].any())
        for k in out:
            assert torch.equal(out[k], inner[k]) and torch.equal(out[k], at[k]) and not out[k].requires_grad
    one = r.hessian_product(vs[0].detach().contiguous(), curvature=True)
    assert one["products"].shape == (n, 2) and one["curvature"].dim() == 1
    b = r._batch
    good = vs.detach()
    for bad in (good.float(), good.cpu(), good[:, :-1], good.transpose(1, 2), good[:, ::2], torch.zeros((5, n, 2), dtype=torch.float64, device=DEV),
                torch.zeros((0, n, 2), dtype=torch.float64, device=DEV), good.cpu().numpy()):
        with pytest.raises(ValueError):
            b.hessian_product(bad)
    for bad in (x.detach().float(), x.detach().cpu(), x.detach()[:-1], x.detach().reshape(-1)):
        with pytest.raises(ValueError):
            b.hessian_product(good, bad)
    r.close()
