"""lfr_batch_hessian_solve (include/lfr.h) against tests/hessian_solve_ref.py and the dense matrices of backward_ref / backward_gn_ref:
every launch class on its row and edge limits, Gauss-Newton and exact, one right-hand side and four, and the call's contract -
negative curvature, Tukey saturation, the free set, damping, no row limit, the round trips with lfr_batch_hessian_product and
lfr_batch_jvp, repeatability and isolation bit for bit, lfr_batch_set_inputs, shards, arguments, status 1, the Python layers.

Tolerances.  With t = GPU_FACTOR x TRUE_RESIDUAL_OVER_TOL_CPU x rel_tolerance (tests/hessian_solve_ref.py), per component at status 0:
the true residual |b - A y|_2 of the GPU's y under the longdouble product is <= t |b|_2, and, derived from it for a positive definite
A, |y - y*|_2 <= kappa_2(A) t |y*|_2 with y* and kappa_2 from the dense matrix."""
import ctypes as C

import numpy as np
import pytest
import torch

import backward_ref as BR
import class_limit_cases as CL
import cost_ref as CR
import evaluate_ref as ER
import hessian_product_ref as HR
import hessian_solve_ref as SR
import jvp_ref as JR
import match_covariance_ref as MR
import test_gpu_class_limits as TCL
from test_gpu_backward import _nodes
from test_gpu_evaluate import _components, _raw, _small, _twice
from test_gpu_hessian_product import _hp, _positions, _ring_6146, _same, _t
from test_gpu_jvp import _jvp, _tangents
from test_gpu_set_inputs import _build, _dev, _flows18, _meta
from test_hessian_product_ref import _component, _dense
from lfr_amd import capi, synthetic
from lfr_amd.autograd import Refiner

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LD = CR.LD
TOL = 1e-10
T_RES = SR.GPU_FACTOR * SR.TRUE_RESIDUAL_OVER_TOL_CPU * TOL
MODES = pytest.mark.parametrize("gn", [False, True], ids=["exact", "gauss_newton"])
KEYS = ("solutions", "status", "iterations", "residual")


def _hs(b, rhs, pos=None, **kw):
    out = b.hessian_solve(_t(rhs), None if pos is None else _t(pos), **kw)
    torch.cuda.synchronize()
    return {k: (x.cpu().numpy() if isinstance(x, torch.Tensor) else x) for k, x in out.items()}


def _all_same(x, y, keys=KEYS):
    return all(_same(x[k], y[k]) for k in keys)


def _check(out, info, comps, pos, bs, n_nodes, variant, gn, what, fs=False, damping=0.0, max_iterations=None, dense=True, whole=True):
    """every (right-hand side, component) of one converged solve within the tolerances of the module's text.  dense=False (the tree
    class, whose dense reference matrices take minutes to build): the true residual under the longdouble product is checked all the same"""
    K = len(bs)
    sol = out["solutions"].reshape(K, n_nodes, 2)
    status, its, res = (out[k].reshape(K, -1) for k in ("status", "iterations", "residual"))
    assert status.shape[1] == len(info["component"])
    is_var = np.zeros(n_nodes, bool)
    worst = worst_y = 0.0
    for i, c in enumerate(info["component"].tolist()):
        vn, ed = comps[c]
        is_var[vn] = True
        cap = max_iterations or 8 * ed.nv
        H = None
        for k in range(K):
            assert status[k, i] == capi.HSOLVE_OK, "%s, component %d, rhs %d: status %d after %d steps" % (what, c, k, status[k, i], its[k, i])
            assert 0 <= res[k, i] <= TOL and 0 < its[k, i] <= cap, (what, c, k, res[k, i], its[k, i])
            y = sol[k][vn]
            r, bn = SR.true_residual(ed, pos[vn], bs[k][vn], y, variant, gn, fs, damping)
            worst = max(worst, float(r / (T_RES * bn)))
            assert r <= T_RES * bn, "%s, component %d, rhs %d: true residual %.3g tolerances" % (what, c, k, float(r / (T_RES * bn)))
            if dense:
                # A is positive definite in every case that asks for this check (Gauss-Newton; the exact Hessian at the solve's own
                # positions; the exact Hessian damped beyond -lambda_min): asserted, not assumed
                if H is None:
                    H = _dense(_component(ed, variant), pos[vn], gn, fs) + damping * np.eye(2 * ed.nv)
                    if fs:
                        bound = (np.abs(pos[vn]) >= 1).reshape(-1)
                        H[bound, bound] = 1.0
                    ev = np.linalg.eigvalsh(H)
                    assert ev[0] > 0, "%s, component %d: smallest eigenvalue %.3g" % (what, c, ev[0])
                y_star = np.linalg.solve(H, bs[k][vn].reshape(-1))
                ratio = float(np.linalg.norm(y.reshape(-1) - y_star) / (float(ev[-1] / ev[0]) * T_RES * np.linalg.norm(y_star)))
                worst_y = max(worst_y, ratio)
                assert ratio <= 1.0, "%s, component %d, rhs %d: |y - y*| is %.3g of kappa_2(A) t |y*|" % (what, c, k, ratio)
    assert not whole or not sol[:, ~is_var].any(), what              # constants, unsolved nodes, other shards: exactly 0
    print("%s: largest true residual %.4f of its tolerance, largest |y - y*| %.4g of its bound, iterations %d..%d" % (what, worst, worst_y, its.min(), its.max()))


# ------------------------------------------------------------------------------------------ 1. every launch class at its limits
@pytest.mark.parametrize("which,gn", [("a", True), ("b", True), ("a", False)], ids=["gn-a", "gn-b", "exact-a"])
def test_every_class_at_its_limits(lfr_lib, which, gn):
    s = TCL.all_solved()
    pos, bs = _positions(s, which), SR.rhs(s.g.n_nodes)
    comps = _components(s.ma, s.g, s.p, s.info)
    four = _hs(s.b, bs, pos, gauss_newton=gn, rel_tolerance=TOL, want_stats=True)
    assert four["solutions"].shape == (4, s.g.n_nodes, 2) and four["status"].shape == (4, len(CL.NAMES))
    st = four["stats"]
    assert st == dict(st, n_components=len(CL.NAMES), n_converged=4 * len(CL.NAMES), n_max_iterations=0, n_negative_curvature=0, n_nonfinite=0,
                      n_bound_coordinates=0, sum_iterations=int(four["iterations"].sum()), max_iterations_used=int(four["iterations"].max())) and st["kernel_ms"] > 0
    _check(four, s.info, comps, pos, bs, s.g.n_nodes, "ceres1", gn, "class limits/%s/(%s)/K=4" % ("gn" if gn else "exact", which))
    one = _hs(s.b, bs[0], pos, gauss_newton=gn, rel_tolerance=TOL)
    assert one["solutions"].shape == (s.g.n_nodes, 2) and one["status"].shape == (len(CL.NAMES),)
    _check(one, s.info, comps, pos, bs[:1], s.g.n_nodes, "ceres1", gn, "class limits/%s/(%s)/K=1" % ("gn" if gn else "exact", which))
    # iterations against the float64 restatement's
    spread = 0
    for i, c in enumerate(s.info["component"].tolist()):
        vn, ed = comps[c]
        ref = SR.solve(ed, pos[vn], bs[0][vn], "ceres1", gn, rel_tolerance=TOL, dtype=np.float64)
        assert ref.status == SR.OK
        spread = max(spread, abs(int(one["iterations"][i]) - ref.iterations))
    print("iterations: largest |GPU - float64 restatement| %d" % spread)
    if SR.ITERATION_SPREAD_GPU is not None:
        assert spread <= SR.ITERATION_SPREAD_GPU


# ----------------------------------------------------------------------------------- 2. the same components twice in shared waves
@MODES
def test_every_class_twice_in_shared_waves(lfr_lib, gn):
    mt, g, p, b, comps, names, posb = _twice()
    b.solve()
    pos = b.download().copy()
    info, bs = b.component_info(), SR.rhs(g.n_nodes, 2)
    out = _hs(b, bs, pos, gauss_newton=gn, rel_tolerance=TOL)
    _check(out, info, comps, pos, bs, g.n_nodes, "ceres1", gn, "twice/%s" % ("gn" if gn else "exact"))


# ------------------------------------------------------------------------------------------------- 3. exact mode at positions_b
def test_negative_curvature_at_positions_b(lfr_lib):
    s = TCL.all_solved()
    posb, bs = _positions(s, "b"), SR.rhs(s.g.n_nodes, 2)
    comps = _components(s.ma, s.g, s.p, s.info)
    out = _hs(s.b, bs, posb, rel_tolerance=TOL, want_stats=True)
    assert (out["status"] == capi.HSOLVE_NEGATIVE_CURVATURE).all() and out["stats"]["n_negative_curvature"] == out["status"].size
    # y against the float64 restatement's iterate, in the form of item 1's bound: |y - y_ref|_2 <= kappa_2(A) t |y_ref|_2 with kappa_2
    # the 2-norm condition number (largest over smallest |eigenvalue|) of the dense exact matrix, which is indefinite here.  Both run
    # the same recurrence for the same number of steps, so they differ by roundings only; the comparison needs equal step counts,
    # which may differ by SR.ITERATION_SPREAD_GPU where p . A p lands within rounding of 0 - most pairs must compare.
    n_pairs = n_compared = n_first = 0
    worst = 0.0
    for i, c in enumerate(s.info["component"].tolist()):
        vn, ed = comps[c]
        ev = np.abs(np.linalg.eigvalsh(_dense(_component(ed, "ceres1"), posb[vn], False, False)))
        assert ev.min() > 0
        for k in range(2):
            ref = SR.solve(ed, posb[vn], bs[k][vn], rel_tolerance=TOL, dtype=np.float64)
            assert ref.status == SR.NEGATIVE_CURVATURE
            y, its = out["solutions"][k][vn], int(out["iterations"][k, i])
            n_pairs += 1
            assert abs(its - ref.iterations) <= SR.ITERATION_SPREAD_GPU, (c, k, its, ref.iterations)
            if its == 0:
                assert not y.any(), (c, k)                    # the first direction failed: zeros
                n_first += 1
            if its == ref.iterations:
                n_compared += 1
                if its:
                    ratio = float(np.linalg.norm(y - ref.y) / (float(ev.max() / ev.min()) * T_RES * np.linalg.norm(ref.y)))
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, "component %d, rhs %d: |y - y_ref| is %.3g of its bound after %d steps" % (c, k, ratio, its)
    print("negative curvature: %d pairs, %d at the restatement's step (%d of them at the first direction), largest |y - y_ref| %.4g of its bound"
          % (n_pairs, n_compared, n_first, worst))
    assert 2 * n_compared > n_pairs
    _check(_hs(s.b, bs, posb, gauss_newton=True, rel_tolerance=TOL), s.info, comps, posb, bs, s.g.n_nodes, "ceres1", True, "positions b/gn")


# ---------------------------------------------------------------------------------- 4. Tukey saturation, the free set, damping
@pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
def test_tukey_saturation_and_damping(lfr_lib, variant):
    ma, g, p, b, st, pos = _small(CR.TUKEY_GRAPH, variant)
    info = b.component_info()
    comps = _components(ma, g, p, info)
    evals = ER.at_positions(comps, pos, variant)
    assert any((ev.rho1[comps[c][1].kind == CR.KIND_INTER] == 0).any() for c, ev in evals.items())
    bs = SR.rhs(g.n_nodes, 1)
    _check(_hs(b, bs, pos, gauss_newton=True, rel_tolerance=TOL), info, comps, pos, bs, g.n_nodes, variant, True, "tukey/%s/gn" % variant)
    # exact: three components meet negative curvature; damping above -lambda_min of the dense matrix makes them converge
    out = _hs(b, bs, pos, rel_tolerance=TOL)
    neg = np.nonzero(out["status"][0] == capi.HSOLVE_NEGATIVE_CURVATURE)[0]
    assert len(neg) == 3 and ((out["status"][0] == capi.HSOLVE_OK) | (out["status"][0] == capi.HSOLVE_NEGATIVE_CURVATURE)).all()
    lam = min(np.linalg.eigvalsh(_dense(_component(comps[c][1], variant), pos[comps[c][0]], False, False))[0] for c in info["component"][neg].tolist())
    assert lam < 0
    damping = float(-lam) * 1.5
    damped = _hs(b, bs, pos, rel_tolerance=TOL, damping=damping)
    sub = {k: (v[:, neg] if k != "solutions" else v) for k, v in damped.items()}
    _check(sub, {"component": info["component"][neg]}, comps, pos, bs, g.n_nodes, variant, False, "tukey/%s/damped" % variant, damping=damping, whole=False)
    assert (damped["status"][0, neg] == capi.HSOLVE_OK).all()


def test_free_set_makes_identity_rows_and_columns(lfr_lib):
    ma, g, p, b, st, pos = _small(CR.BOUNDS_GRAPH)
    info = b.component_info()
    comps = _components(ma, g, p, info)
    bs = SR.rhs(g.n_nodes, 2)
    is_var = np.zeros(g.n_nodes, bool)
    for vn, _ in comps.values():
        is_var[vn] = True
    at_bound = (np.abs(pos) >= 1.0) & is_var[:, None]
    assert at_bound.sum() >= 10
    for gn in (True, False):
        out = _hs(b, bs, pos, gauss_newton=gn, free_set=True, rel_tolerance=TOL, want_stats=True)
        _check(out, info, comps, pos, bs, g.n_nodes, "ceres1", gn, "bounds/free set/%s" % ("gn" if gn else "exact"), fs=True)
        assert out["stats"]["n_bound_coordinates"] == int(at_bound.sum())
        assert np.array_equal(_raw(out["solutions"][:, at_bound]), _raw(bs[:, at_bound]))             # y_i = b_i, the very bits
        moved = bs.copy()
        moved[:, at_bound] += 3.0                                                                      # b_i moves no other row
        again = _hs(b, moved, pos, gauss_newton=gn, free_set=True, rel_tolerance=TOL)
        assert np.array_equal(_raw(again["solutions"][:, ~at_bound]), _raw(out["solutions"][:, ~at_bound]))
        assert _all_same(again, out, KEYS[1:])
        plain = _hs(b, bs, pos, gauss_newton=gn, rel_tolerance=TOL, want_stats=True)
        assert plain["stats"]["n_bound_coordinates"] == 0 and not _same(plain["solutions"], out["solutions"])


# ------------------------------------------------------------------------------------------------------------ 5. no row limit
def test_a_ring_of_6146_rows(lfr_lib):
    ma, g, p, b, pos, info = _ring_6146()
    comps = _components(ma, g, p, info)
    bs = SR.rhs(g.n_nodes, 1)
    out = _hs(b, bs, pos, gauss_newton=True, rel_tolerance=TOL, damping=SR.RING_DAMPING, max_iterations=4 * 6146)
    _check(out, info, comps, pos, bs, g.n_nodes, "ceres1", True, "ring of 6146 rows", damping=SR.RING_DAMPING, max_iterations=4 * 6146)


def test_a_tree_class_component(lfr_lib):
    ma, g, p, b, st, pos = _small(dict(n_images=1344, n_tracks=MR.CAPSIZED_SMALLEST, seed=7, track_degree=4, chain_links=1, eps_out=0.0005, ratio_sims=True))
    info = b.component_info()
    assert (2 * info["n_var_nodes"]).max() > CL.MAX_BLOCK_ROWS
    comps = _components(ma, g, p, info)
    bs = SR.rhs(g.n_nodes, 2)
    _check(_hs(b, bs, pos, gauss_newton=True, rel_tolerance=TOL), info, comps, pos, bs, g.n_nodes, "ceres1", True, "tree class/gn", dense=False)


# -------------------------------------------------------------------------------------------------------------- 6. round trips
@MODES
def test_round_trips_with_the_product_and_the_jvp(lfr_lib, gn):
    s = TCL.all_solved()
    comps = _components(s.ma, s.g, s.p, s.info)
    v = HR.vectors(s.g.n_nodes, 1)
    hv = _hp(s.b, v, s.pos, gauss_newton=gn, curvature=False)["products"]
    out = _hs(s.b, hv, s.pos, gauss_newton=gn, rel_tolerance=TOL)
    assert (out["status"] == capi.HSOLVE_OK).all()
    worst = 0.0
    for c in s.info["component"].tolist():
        vn, ed = comps[c]
        ev = np.linalg.eigvalsh(_dense(_component(ed, "ceres1"), s.pos[vn], gn, False))
        assert ev[0] > 0
        # b = fl(H v): v solves a system whose right-hand side is off by the product's rounding, which kappa T_RES dominates
        ratio = float(np.linalg.norm(out["solutions"][0][vn] - v[0][vn]) / (float(ev[-1] / ev[0]) * T_RES * np.linalg.norm(v[0][vn])))
        worst = max(worst, ratio)
        assert ratio <= 1.0, "component %d: |y - v| is %.3g of kappa_2(A) t |v|" % (c, ratio)
    print("round trip with the product/%s: largest |y - v| %.4g of its bound" % ("gn" if gn else "exact", worst))
    # b = jvp_ref.rhs on the free set at the batch's positions: y agrees with lfr_batch_jvp's xdot
    ts = _tangents(s.ma, 41)
    xdot = _jvp(s.b, ts, gn)
    assert (s.b.jvp_status() == capi.JVP_OK).all()
    bcomps = BR.graph_components(s.ma, *s.p.labels(), *_nodes(s.g, s.ma))
    b = np.zeros((s.g.n_nodes, 2))
    for c in s.info["component"].tolist():
        vn, cp = bcomps[c]
        x = s.pos[vn].reshape(-1)
        m, odd = cp.eids >> 1, (cp.eids & 1) == 1
        b[vn] = np.where(cp.free(x), JR.rhs(cp, x, np.where(odd[:, None], ts[0][m], ts[1][m]), ts[2][m]), 0.0).reshape(-1, 2)
    out = _hs(s.b, b, None, gauss_newton=gn, free_set=True, rel_tolerance=TOL)
    assert (out["status"] == capi.HSOLVE_OK).all()
    worst = 0.0
    for c in s.info["component"].tolist():
        vn, ed = comps[c]
        H = _dense(_component(ed, "ceres1"), s.pos[vn], gn, True)
        ev = np.linalg.eigvalsh(H)
        free = (np.abs(s.pos[vn]) < 1)
        assert ev[0] > 0
        ratio = float(np.linalg.norm((out["solutions"][vn] - xdot[vn])[free]) / (float(ev[-1] / ev[0]) * T_RES * np.linalg.norm(xdot[vn])))
        worst = max(worst, ratio)
        assert ratio <= 1.0, "component %d: |y - xdot| is %.3g of kappa_2(A) t |xdot|" % (c, ratio)
    print("round trip with the jvp/%s: largest |y - xdot| %.4g of its bound" % ("gn" if gn else "exact", worst))


# ------------------------------------------------------------------------------------------------------------------ 7. bitwise
def test_repeatable_and_the_same_for_every_assembly(lfr_lib):
    h, d = TCL.all_solved(False), TCL.all_solved(True)
    pos, bs = h.pos, SR.rhs(h.g.n_nodes)
    order = [int(np.nonzero(d.info["component"] == c)[0][0]) for c in h.info["component"]]
    ma, _ = CL.all_shapes()
    _, _, fused, _ = _build(ma, "fused")
    fused.solve()
    for gn in (False, True):
        first = _hs(h.b, bs, pos, gauss_newton=gn)
        assert _all_same(first, _hs(h.b, bs, pos, gauss_newton=gn))
        dev = _hs(d.b, bs, pos, gauss_newton=gn)
        assert _same(first["solutions"], dev["solutions"]) and all(_same(first[k], dev[k][:, order]) for k in KEYS[1:])
        f = _hs(fused, bs, pos, gauss_newton=gn)
        assert _all_same(f, dev)
        for k in range(4):                                   # right-hand side k alone, among random others, among NaNs
            alone = _hs(h.b, bs[k], pos, gauss_newton=gn)
            assert all(_same(alone[key], first[key][k]) for key in KEYS), (gn, k)
            for fill in (SR.rhs(h.g.n_nodes, 4, seed=9500 + k), np.full(bs.shape, np.nan)):
                mixed = fill.copy()
                slot = (k + 1) % 4
                mixed[slot] = bs[k]
                among = _hs(h.b, mixed, pos, gauss_newton=gn)
                assert all(_same(among[key][slot], first[key][k]) for key in KEYS), (gn, k)


def test_a_nan_fails_its_component_alone(lfr_lib):
    mt, g, p, b, comps, names, posb = _twice()
    b.solve()
    pos = b.download().copy()
    info, bs = b.component_info(), SR.rhs(g.n_nodes)
    out = _hs(b, bs, pos, gauss_newton=True, want_stats=True)
    assert out["stats"]["n_nonfinite"] == 0
    for victim in (names[1]["k7_first_reread"], names[0]["k5"], names[1]["k14"], names[0]["ring46"], names[1]["k98"]):
        rows = info["component"] != victim
        nodes = np.ones(g.n_nodes, bool)
        nodes[comps[victim][0]] = False
        bad_b = bs.copy()
        bad_b[2, comps[victim][0][1], 0] = np.nan
        bad = _hs(b, bad_b, pos, gauss_newton=True, want_stats=True)
        assert bad["stats"]["n_nonfinite"] == 1 and (bad["status"][2, ~rows] == capi.HSOLVE_NONFINITE).all()
        assert np.array_equal(_raw(bad["solutions"][:, nodes]), _raw(out["solutions"][:, nodes]))
        for key in KEYS[1:]:
            assert np.array_equal(_raw(bad[key][:, rows]), _raw(out[key][:, rows]))
        for k in (0, 1, 3):                                  # the victim's other right-hand sides too
            assert all(np.array_equal(_raw(bad[key][k]), _raw(out[key][k])) for key in KEYS)
        eid = int(comps[victim][1].eids[3])                  # a flow
        d1, d2 = _flows18(mt.disp1).copy(), _flows18(mt.disp2).copy()
        (d1 if eid & 1 else d2)[eid >> 1, 8] = np.nan
        b.set_inputs(_dev(d1), _dev(d2))
        bad = _hs(b, bs, pos, gauss_newton=True, want_stats=True)
        b.set_inputs(_dev(mt.disp1), _dev(mt.disp2))
        assert bad["stats"]["n_nonfinite"] == 4 and (bad["status"][:, ~rows] == capi.HSOLVE_NONFINITE).all()
        assert np.array_equal(_raw(bad["solutions"][:, nodes]), _raw(out["solutions"][:, nodes]))
        for key in KEYS[1:]:
            assert np.array_equal(_raw(bad[key][:, rows]), _raw(out[key][:, rows]))
    assert _all_same(_hs(b, bs, pos, gauss_newton=True), out)


# -------------------------------------------------------------------------------------------------------------------- 8. state
def test_state_streams_and_shards(lfr_lib):
    ma, _ = CL.all_shapes()
    mb = CL.second_inputs()
    g, p, b, _ = _build(ma, "host")
    bs = SR.rhs(g.n_nodes, 2)
    with pytest.raises(capi.LfrError) as e:
        b.hessian_solve(_t(bs), gauss_newton=True)                                   # NULL positions before the first solve
    assert e.value.code == -1
    b.solve()
    x0 = b.download().copy()
    info = b.component_info()
    comps = _components(ma, g, p, info)
    _check(_hs(b, bs, x0, gauss_newton=True), info, comps, x0, bs, g.n_nodes, "ceres1", True, "explicit positions")
    b.set_inputs(_dev(mb.disp1), _dev(mb.disp2), _dev(mb.sim, flows=False))
    compsb = _components(mb, g, p, info)
    _check(_hs(b, bs, None, gauss_newton=True), info, compsb, x0, bs, g.n_nodes, "ceres1", True, "new flows at the held positions")
    # set_inputs waits for the solve: on two streams, without a host synchronisation in between
    want = _hs(b, bs, None, gauss_newton=True)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    got = b.hessian_solve(_t(bs), None, gauss_newton=True, stream=s1.cuda_stream)
    b.set_inputs(_dev(ma.disp1), _dev(ma.disp2), _dev(ma.sim, flows=False), stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert all(_same(got[k].cpu().numpy(), want[k]) for k in KEYS)
    # two solves of one batch on two streams share the pass's workspace: the second waits for the first, both return a lone call's bits
    other = SR.rhs(g.n_nodes, 2, seed=9600)
    want_other = _hs(b, other, None, gauss_newton=True)
    want = _hs(b, bs, None, gauss_newton=True)
    torch.cuda.synchronize()
    t1, t2 = _t(bs), _t(other)
    torch.cuda.synchronize()
    got1 = b.hessian_solve(t1, None, gauss_newton=True, stream=s1.cuda_stream)
    got2 = b.hessian_solve(t2, None, gauss_newton=True, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert all(_same(got1[k].cpu().numpy(), want[k]) for k in KEYS) and all(_same(got2[k].cpu().numpy(), want_other[k]) for k in KEYS)
    # shards
    s = TCL.all_solved()
    whole = _hs(s.b, bs, s.pos, gauss_newton=True)
    for rank in range(2):
        sb = capi.Batch(s.p, 0, rank, 2)
        sinfo = sb.component_info()
        scomps = _components(s.ma, s.g, s.p, sinfo)
        o = _hs(sb, bs, s.pos, gauss_newton=True)
        mine = np.zeros(s.g.n_nodes, bool)
        for vn, _ in scomps.values():
            mine[vn] = True
        assert (o["status"] == capi.HSOLVE_OK).all() and np.array_equal(_raw(o["solutions"][:, mine]), _raw(whole["solutions"][:, mine]))
        assert not o["solutions"][:, ~mine].any()
    mc = synthetic.generate(seed=32, n_images=48, n_tracks=3000, eps_out=0.002)
    g2 = capi.Graph.from_arrays(mc)
    p2 = capi.Problem(g2, device_graph_stage=0, shard=(0, 2))
    assert p2.cc_sharded
    b2 = capi.Batch(p2, 0)
    b2.solve()
    o = _hs(b2, SR.rhs(g2.n_nodes, 1), None, gauss_newton=True, want_stats=True)
    assert o["stats"]["n_converged"] == o["stats"]["n_components"] == o["status"].shape[1] and np.isfinite(o["solutions"]).all() and o["solutions"].any()


# ---------------------------------------------------------------------------------------------------------------- 9. arguments
def test_argument_errors_touch_no_output(lfr_lib):
    s = TCL.all_solved()
    L = capi.lib()
    n, nc = s.g.n_nodes, len(s.info["component"])
    rhs = _t(SR.rhs(n))
    sol = torch.full((4, n, 2), 7.0, dtype=torch.float64, device=DEV)
    res = torch.full((4, nc), 7.0, dtype=torch.float64, device=DEV)
    sta = torch.full((4, nc), 7, dtype=torch.int32, device=DEV)
    its = torch.full((4, nc), 7, dtype=torch.int32, device=DEV)
    pr, ps = C.c_void_p(rhs.data_ptr()), C.c_void_p(sol.data_ptr())
    info = (C.c_void_p(sta.data_ptr()), C.c_void_p(its.data_ptr()), C.c_void_p(res.data_ptr()))
    call = lambda r, k, damping, tol, mi, y, flags: L.lfr_batch_hessian_solve(s.b._h, None, r, k, damping, tol, mi, y, *info, flags, None, None)
    nan, inf = float("nan"), float("inf")
    for args in ((None, 1, 0.0, TOL, 10, ps, 2), (pr, 1, 0.0, TOL, 10, None, 2), (pr, 0, 0.0, TOL, 10, ps, 2), (pr, 5, 0.0, TOL, 10, ps, 2),
                 (pr, 1, 0.0, TOL, 10, ps, 1), (pr, 1, 0.0, TOL, 10, ps, 8), (pr, 1, -1.0, TOL, 10, ps, 2), (pr, 1, nan, TOL, 10, ps, 2),
                 (pr, 1, inf, TOL, 10, ps, 2), (pr, 1, 0.0, -1e-3, 10, ps, 2), (pr, 1, 0.0, nan, 10, ps, 2), (pr, 1, 0.0, TOL, 0, ps, 2)):
        assert call(*args) == -1, args[1:]
        torch.cuda.synchronize()
        assert bool((sol == 7.0).all()) and bool((res == 7.0).all()) and bool((sta == 7).all()) and bool((its == 7).all()), args[1:]
    untouched = lambda: bool((sol == 7.0).all()) and bool((res == 7.0).all()) and bool((sta == 7).all()) and bool((its == 7).all())
    assert L.lfr_batch_hessian_solve(None, None, pr, 1, 0.0, TOL, 10, ps, *info, 2, None, None) == -1              # no batch
    torch.cuda.synchronize()
    assert untouched()
    ma, _ = CL.all_shapes()
    _, _, unsolved, _ = _build(ma, "host")                                           # the same graph, never solved
    assert L.lfr_batch_hessian_solve(unsolved._h, None, pr, 1, 0.0, TOL, 10, ps, *info, 2, None, None) == -1      # NULL positions before the first solve
    torch.cuda.synchronize()
    assert untouched()
    assert call(pr, 4, 0.0, TOL, 1000, ps, 2 | 4) == 0
    torch.cuda.synchronize()
    want = _hs(s.b, rhs.cpu().numpy(), None, gauss_newton=True, free_set=True, rel_tolerance=TOL, max_iterations=1000)
    assert _same(sol.cpu().numpy(), want["solutions"]) and _same(sta.cpu().numpy(), want["status"]) and _same(res.cpu().numpy(), want["residual"])
    bare = _hs(s.b, rhs.cpu().numpy(), None, gauss_newton=True, free_set=True, rel_tolerance=TOL, max_iterations=1000, want_info=False)
    assert sorted(bare) == ["solutions"] and _same(bare["solutions"], want["solutions"])


# ---------------------------------------------------------------------------------------------------------------- 10. status 1
def test_one_iteration_is_status_1(lfr_lib):
    s = TCL.all_solved()
    out = _hs(s.b, SR.rhs(s.g.n_nodes, 2), s.pos, gauss_newton=True, rel_tolerance=TOL, max_iterations=1, want_stats=True)
    big = 2 * s.info["n_var_nodes"] > 2
    assert (out["status"][:, big] == capi.HSOLVE_MAX_ITERATIONS).all() and (out["iterations"][:, big] == 1).all() and (out["residual"][:, big] > TOL).all()
    assert (out["iterations"] == 1).all() and out["stats"]["max_iterations_used"] == 1 and out["stats"]["n_max_iterations"] >= 2 * big.sum()


# ------------------------------------------------------------------------------------------------------------------ 11. Python
def test_refiner_hessian_solve_and_argument_checks(lfr_lib):
    ma = synthetic.generate(seed=41, n_images=12, n_tracks=120)
    r = Refiner(_dev(ma.disp1), _dev(ma.disp2), _dev(ma.sim, flows=False), banned=("000005.png",), **_meta(ma))
    x = r(_dev(ma.disp1), _dev(ma.disp2))
    n = r.n_nodes
    bs = _t(SR.rhs(n, 3)).requires_grad_(True)
    for kw in (dict(gauss_newton=True), dict(gauss_newton=True, free_set=True, damping=0.5, want_stats=True)):
        out = r.hessian_solve(bs, **kw)
        inner = r._batch.hessian_solve(bs.detach(), **kw)
        at = r.hessian_solve(bs, x, **kw)
        torch.cuda.synchronize()
        assert sorted(out) == sorted(inner) and out["solutions"].shape == (3, n, 2) and bool(out["solutions"].any())
        assert out["status"].dtype == torch.int32 and out["status"].shape == out["iterations"].shape == out["residual"].shape and out["status"].dim() == 2
        for k in KEYS:
            assert torch.equal(out[k], inner[k]) and torch.equal(out[k], at[k]) and not out[k].requires_grad
        assert bool((out["status"] == capi.HSOLVE_OK).all())
    one = r.hessian_solve(bs[0].detach().contiguous(), gauss_newton=True)
    assert one["solutions"].shape == (n, 2) and one["status"].dim() == 1
    b = r._batch
    nvar = int(b.component_info()["n_var_nodes"].max())
    capped = b.hessian_solve(bs.detach(), gauss_newton=True, rel_tolerance=0.0)      # max_iterations=None: 4 x the largest component's rows
    assert int(capped["iterations"].max()) <= 8 * nvar
    good = bs.detach()
    for bad in (good.float(), good.cpu(), good[:, :-1], good.transpose(1, 2), good[:, ::2], torch.zeros((5, n, 2), dtype=torch.float64, device=DEV),
                torch.zeros((0, n, 2), dtype=torch.float64, device=DEV), good.cpu().numpy()):
        with pytest.raises(ValueError):
            b.hessian_solve(bad)
    for bad in (x.detach().float(), x.detach().cpu(), x.detach()[:-1], x.detach().reshape(-1)):
        with pytest.raises(ValueError):
            b.hessian_solve(good, bad)
    for kw in (dict(damping=-1.0), dict(damping=float("nan")), dict(rel_tolerance=-1.0), dict(rel_tolerance=float("nan")), dict(max_iterations=0)):
        with pytest.raises(ValueError):
            b.hessian_solve(good, **kw)
    r.close()
