"""The Gauss-Newton fallback of the backward and the jvp (LFR_BACKWARD_FALLBACK_GAUSS_NEWTON, LFR_JVP_FALLBACK_GAUSS_NEWTON,
include/lfr.h): exact where the exact Hessian factors, J^T J for the components where it does not, the outcome per component in the
status array - against the composition of the CPU references (tests/hessian_fallback_ref.py) with the GPU's own positions x^, and
bit for bit against the two pure modes on the same solve.

Inputs: the hard cases of tests/lm_decision_cases.py, one per kernel path - packed_24_32 (one wave per component), block_m (matrix in
LDS), tree and global (matrix in the HBM workspace; HBM_CASES below) - the class limits of tests/test_gpu_class_limits.py (nothing
indefinite), the 48-image synthetic graph of the other backward tests, and three path-shaped tracks whose end nodes are leaves.

Tolerance: the project's own for these passes, |got - ref| <= 1e-8 |ref| + 1e-14 per component; on the lm_decision_cases inputs the
relative term is max(1e-8, 64 eps kappa_2) with kappa_2 of the matrix the reference used (test_gpu_backward_gn's rule).  The adjoint
identity: test_gpu_jvp's, 1e-8 (|ubar_c| |xdot_c| + |g_c| |thetadot_c|) per component.  No component is left out of a comparison."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import backward_ref as BR
import hessian_fallback_ref as FR
import lm_decision_cases as LC
from test_gpu_backward import _nodes, _setup, _ubar
from test_gpu_backward_gn import _leaf_tensors, _raw_backward
from test_gpu_class_limits import all_solved
from test_gpu_jvp import _by_component, _dev, _leaf_match, _match_nodes, _meta, _raw_jvp, _tangents
from test_gpu_lm_decisions import solved
from lfr_amd import capi, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EPS = np.finfo(np.float64).eps
LFR_ERR_ARG = -1
# The two inputs above 192 rows, with the references at the oracle's positions: in `tree` the exact Hessian of ALL 12 components is
# indefinite and J^T J positive definite (12 x status 3, none of status 0); in `global` all 6 are positive definite (6 x status 0).
# `tree` is the case that has something to fall back from, but neither input alone shows both outcomes, so the HBM-matrix kernel runs
# on both: `tree` must fall back at least once, `global` must stay exact at least once, everything else is checked on either.
HBM_CASES = ("tree", "global")
CASES = ["packed_24_32", "block_m"] + list(HBM_CASES)
MUST_SHOW = {"packed_24_32": (0, 3), "block_m": (0, 3), "tree": (3,), "global": (0,)}      # statuses an input must yield at least once
_cache = {}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _backward(b, gp, f64=True, **mode):
    """([grad_disp1, grad_disp2, grad_sim] as numpy, stats, per-component status) of one backward call"""
    out = b.backward(gp, f64=f64, want_stats=True, **mode)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out[:3]], out[3], b.backward_status().copy()


def _jvp(b, ts, **mode):
    f64 = next(t for t in ts if t is not None).dtype == np.float64
    out, st = b.jvp(*_dev(ts), f64=f64, want_stats=True, **mode)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st, b.jvp_status().copy()


def _rows_of(cp, outs):
    """one component's part of the three outputs: its match rows of grad_disp1/2 (the direction of each record) and its grad_sim"""
    m, odd = cp.eids >> 1, (cp.eids & 1) == 1
    return np.concatenate([np.where(odd[:, None], outs[0][m], outs[1][m]).ravel(), outs[2][np.unique(m)]])


def _case(name):
    """a hard case solved once, its components, and per component the reference composition of the backward and of the jvp at the
    GPU's positions: computed once, shared, left unchanged"""
    if name not in _cache:
        ma, _, _ = LC.reference(name)
        g, p, b, _, pos = solved(name)
        comps = BR.graph_components(ma, *p.labels(), *_nodes(g, ma))
        info = b.component_info()
        assert sorted(comps) == sorted(info["component"].tolist()) and (info["termination"] != capi.TERM_FAILURE).all()
        gp, ts = _ubar(g.n_nodes, 5), _tangents(ma, 6)
        ub = gp.cpu().numpy()
        back, items = {}, []
        for c in sorted(comps):
            var_nodes, cp = comps[c]
            x = pos[var_nodes].reshape(-1)
            gf, gw, rs, kappa = FR.backward(cp, x, ub[var_nodes].reshape(-1))
            ref_s = np.zeros(len(ma.sim))
            np.add.at(ref_s, cp.eids >> 1, gw)
            back[c] = (np.concatenate([gf.ravel(), ref_s[np.unique(cp.eids >> 1)]]), rs, kappa)
            m, odd = cp.eids >> 1, (cp.eids & 1) == 1
            items.append((cp, x, np.where(odd[:, None], ts[0][m], ts[1][m]), ts[2][m]))
        fwd = dict(zip(sorted(comps), FR.jvp_many(items)))
        _cache[name] = dict(ma=ma, g=g, p=p, b=b, pos=pos, comps=comps, info=info, gp=gp, ts=ts, back=back, fwd=fwd)
    return _cache[name]


def _histogram(status):
    return {s: int((status == s).sum()) for s in (0, 1, 2, 3)}


def _check_stats(st, status):
    h = _histogram(status)
    assert st["n_differentiated"] == h[0] + h[3] and st["n_indefinite"] == h[2] and st["n_not_usable"] == h[1]
    assert h[0] + h[1] + h[2] + h[3] == len(status)
    return h


# ---------------------------------------------------------------------------------------------- 1. mode and values, every class
@pytest.mark.parametrize("name", CASES)
def test_backward_mode_and_values(lfr_lib, name):
    k = _case(name)
    outs, st, status = _backward(k["b"], k["gp"], gn_fallback=True)
    stat = _by_component(k["info"], status)
    worst = 0.0
    for c, (var_nodes, cp) in k["comps"].items():
        ref, rs, kappa = k["back"][c]
        got = _rows_of(cp, outs)
        assert stat[c] == rs, "component %d: status %d, the reference composition %d" % (c, stat[c], rs)
        if rs == FR.INDEFINITE:
            assert not got.any(), c
            continue
        rel = max(1e-8, 64.0 * EPS * kappa)
        ratio = np.linalg.norm(got - ref) / (rel * np.linalg.norm(ref) + 1e-14)
        worst = max(worst, ratio)
        assert ratio <= 1.0, "component %d (status %d): error / bound %.3f (kappa_2 %.3e)" % (c, rs, ratio, kappa)
    h = _check_stats(st, status)
    print("%s backward: statuses %s, worst error / bound %.4f" % (name, h, worst))
    assert all(h[s] >= 1 for s in MUST_SHOW[name]) and h[1] == 0
    assert h[0] + h[2] + h[3] == len(k["comps"])


# ------------------------------------------------------------------------------------------------------------------- 2. bits
@pytest.mark.parametrize("name", CASES)
def test_backward_bits(lfr_lib, name):
    k = _case(name)
    b, gp = k["b"], k["gp"]
    fb, _, status = _backward(b, gp, gn_fallback=True)
    exact, _, exact_status = _backward(b, gp)
    gn, _, _ = _backward(b, gp, gauss_newton=True)
    stat, rows = _by_component(k["info"], status), _by_component(k["info"], 2 * k["info"]["n_var_nodes"])
    n = {0: 0, "3 bitwise": 0, "3 packed": 0}
    for c, (_, cp) in k["comps"].items():
        mine = _rows_of(cp, fb)
        if stat[c] == capi.BACKWARD_OK:
            assert _same(mine, _rows_of(cp, exact)), c
            n[0] += 1
        elif stat[c] == capi.BACKWARD_FALLBACK and rows[c] > 32:
            assert _same(mine, _rows_of(cp, gn)), c
            n["3 bitwise"] += 1
        elif stat[c] == capi.BACKWARD_FALLBACK:          # one wave per component here, an explicit inverse in the Gauss-Newton mode
            want = _rows_of(cp, gn)
            rel = max(1e-8, 64.0 * EPS * k["back"][c][2])
            assert mine.any() and np.linalg.norm(mine - want) <= rel * np.linalg.norm(want) + 1e-14, c
            n["3 packed"] += 1
        else:
            assert stat[c] == capi.BACKWARD_INDEFINITE and not mine.any(), c
    assert np.array_equal(status == capi.BACKWARD_OK, exact_status == capi.BACKWARD_OK)      # the fallback starts where the exact mode gives up
    print("%s: %s" % (name, n))
    assert n[0] >= (0 in MUST_SHOW[name]) and n["3 packed" if name == "packed_24_32" else "3 bitwise"] >= (3 in MUST_SHOW[name])
    again, _, again_status = _backward(b, gp, gn_fallback=True)
    assert all(_same(x, y) for x, y in zip(fb, again)) and np.array_equal(status, again_status)
    f32, _, _ = _backward(b, gp, f64=False, gn_fallback=True)
    assert all(z.dtype == np.float32 and _same(z, x.astype(np.float32)) for x, z in zip(fb, f32))
    bd = capi.Batch(capi.Problem(k["g"], device_graph_stage=0), 0)
    bd.solve()
    assert _same(bd.download(), k["pos"])
    dev, _, dev_status = _backward(bd, gp, gn_fallback=True)
    assert all(_same(x, y) for x, y in zip(fb, dev)) and np.array_equal(status, dev_status)
    xd, _, js = _jvp(b, k["ts"], gn_fallback=True)
    xdd, _, jsd = _jvp(bd, k["ts"], gn_fallback=True)
    assert _same(xd, xdd) and np.array_equal(js, jsd)


# ------------------------------------------------------------------------------------------------ 3. both factorizations fail
@pytest.fixture(scope="module")
def small():
    return synthetic.generate(seed=11, n_images=48, n_tracks=400, eps_out=0.01)


@pytest.fixture(scope="module")
def small_run(lfr_lib, small):
    """the unmodified input solved once: graph, problem, batch, dL/dx, tangents, fallback outputs of both passes, positions, components"""
    g, p, b = _setup(small)
    gp, ts = _ubar(g.n_nodes, 7), _tangents(small, 8)
    comps = BR.graph_components(small, *p.labels(), *_nodes(g, small))
    return dict(g=g, p=p, b=b, gp=gp, ts=ts, back=_backward(b, gp, gn_fallback=True), fwd=_jvp(b, ts, gn_fallback=True),
                pos=b.download().copy(), comps=comps)


def _others_unchanged(r, b, back, xdot, touched):
    """every untouched component whose positions are the same bits in both solves has the same bits in the outputs of both passes"""
    x, n = b.download(), 0
    for c, (var_nodes, cp) in r["comps"].items():
        if c in touched or not _same(x[var_nodes], r["pos"][var_nodes]):
            continue
        assert _same(_rows_of(cp, back), _rows_of(cp, r["back"][0])) and _same(xdot[var_nodes], r["fwd"][0][var_nodes]), c
        n += 1
    assert n >= 0.9 * (len(r["comps"]) - len(touched)) and n >= 1


def _both_fail(ma, r, zero_matches, c_zero, c_fail):
    """similarity 0 on `zero_matches` (each the only match of a leaf of the components c_zero), a non-finite flow in c_fail: the
    fallback backward and jvp of that input against the run `r` of the unmodified one"""
    comps = r["comps"]
    mb = copy.deepcopy(ma)
    for m in zero_matches:
        mb.sim[m] = 0.0                                          # unties the leaf: its rows of H and of J^T J are zero
    if c_fail is not None:
        e = int(comps[c_fail][1].eids[0])
        (mb.disp1 if e & 1 else mb.disp2)[e >> 1, 4, 0] = np.inf     # FAILURE component
    g, p, b = _setup(mb)
    assert (p.labels()[2] == r["p"].labels()[2]).all()           # (the weights do not move the component structure here)
    info = b.component_info()
    back, st, status = _backward(b, r["gp"], gn_fallback=True)
    xdot, jst, js = _jvp(b, r["ts"], gn_fallback=True)
    assert np.array_equal(status, js)
    stat, term = _by_component(info, status), _by_component(info, info["termination"])
    assert all(stat[c] == capi.BACKWARD_INDEFINITE == 2 for c in c_zero)
    touched = set(c_zero)
    if c_fail is not None:
        assert term[c_fail] == capi.TERM_FAILURE and stat[c_fail] == capi.BACKWARD_NOT_USABLE == 1
        touched.add(c_fail)
    for c in touched:
        assert _rows_of(comps[c][1], r["back"][0]).any() and r["fwd"][0][comps[c][0]].any()      # (they had a result before)
        assert not _rows_of(comps[c][1], back).any() and not xdot[comps[c][0]].any()
    h = _check_stats(st, status)
    _check_stats(jst, js)
    assert h[2] >= len(c_zero) >= 1 and st["n_indefinite"] >= 1 and h[1] == (c_fail is not None)
    _others_unchanged(r, b, back, xdot, touched)
    return _by_component(info, 2 * info["n_var_nodes"])


def test_both_factorizations_fail_in_a_packed_class_and_a_failed_component(small, small_run):
    comps = small_run["comps"]
    c_lo, m_lo = _leaf_match(comps)                              # test_gpu_jvp's construction
    assert len(m_lo) == 1
    c_fail = next(c for c in sorted(comps)[40:] if c != c_lo)
    rows = _both_fail(small, small_run, [m_lo], [c_lo], c_fail)
    assert rows[c_lo] <= 32


def test_both_factorizations_fail_in_the_workgroup_classes(lfr_lib):
    """`small` has no leaf above 32 rows.  A track matched along a path has two: tracks of 40 and 110 nodes (78 rows: matrix in LDS,
    218 rows: matrix in HBM) beside three complete tracks."""
    import class_limit_cases as CL
    ma = CL.tracks(31, [(40, 39, 0), (110, 109, 0), 6, 12, 30])
    g, p, b = _setup(ma)
    gp, ts = _ubar(g.n_nodes, 7), _tangents(ma, 8)
    comps = BR.graph_components(ma, *p.labels(), *_nodes(g, ma))
    r = dict(g=g, p=p, b=b, gp=gp, ts=ts, back=_backward(b, gp, gn_fallback=True), fwd=_jvp(b, ts, gn_fallback=True),
             pos=b.download().copy(), comps=comps)
    leaves = [_leaf_match({c: v}) for c, v in comps.items() if len(v[1].src) == 2 * v[1].nv]      # the paths: a match per variable node
    assert len(leaves) == 2 and all(len(m) == 1 for _, m in leaves)
    rows = _both_fail(ma, r, [m for _, m in leaves], [c for c, _ in leaves], None)
    assert sorted(rows[c] for c, _ in leaves) == [78, 218]


# ------------------------------------------------------------------------------------------------ 4. nothing to fall back from
def test_class_limits_fallback_is_the_exact_mode(lfr_lib):
    s = all_solved()
    gp = _ubar(s.g.n_nodes, 21)
    ts = _tangents(s.ma, 22)
    exact, est, estatus = _backward(s.b, gp)
    fb, st, status = _backward(s.b, gp, gn_fallback=True)
    assert (estatus == capi.BACKWARD_OK).all() and est["n_indefinite"] == 0
    assert all(x.any() and _same(x, y) for x, y in zip(exact, fb))
    assert (status == capi.BACKWARD_OK).all() and st["n_differentiated"] == len(status)
    xe, _, jse = _jvp(s.b, ts)
    xf, jst, jsf = _jvp(s.b, ts, gn_fallback=True)
    assert xe.any() and _same(xe, xf) and (jsf == capi.JVP_OK).all() and np.array_equal(jse, jsf)
    assert jst["n_differentiated"] == len(jsf) and jst["n_indefinite"] == 0


# -------------------------------------------------------------------------------------------------------------------- 5. jvp
@pytest.mark.parametrize("name", CASES)
def test_jvp_mode_values_bits_and_adjoint_identity(lfr_lib, name):
    k = _case(name)
    b, ts, ma, g, p = k["b"], k["ts"], k["ma"], k["g"], k["p"]
    xdot, st, js = _jvp(b, ts, gn_fallback=True)
    back, _, status = _backward(b, k["gp"], gn_fallback=True)
    assert np.array_equal(js, status)                            # the two passes decide from the same matrix with the same code
    stat, rows = _by_component(k["info"], js), _by_component(k["info"], 2 * k["info"]["n_var_nodes"])
    exact, _, _ = _jvp(b, ts)
    gn, _, _ = _jvp(b, ts, gauss_newton=True)
    worst = 0.0
    for c, (var_nodes, cp) in k["comps"].items():
        ref, rs = k["fwd"][c]
        got = xdot[var_nodes].reshape(-1)
        assert stat[c] == rs == k["back"][c][1], "component %d: status %d, the reference composition %d" % (c, stat[c], rs)
        if rs == FR.INDEFINITE:
            assert not got.any(), c
            continue
        rel = max(1e-8, 64.0 * EPS * k["back"][c][2])
        ratio = np.linalg.norm(got - ref) / (rel * np.linalg.norm(ref) + 1e-14)
        worst = max(worst, ratio)
        assert ratio <= 1.0, "component %d (status %d): error / bound %.3f" % (c, rs, ratio)
        assert not got[np.abs(k["pos"][var_nodes].reshape(-1)) >= 1.0].any()
        if rs == FR.OK:
            assert _same(got, exact[var_nodes].reshape(-1)), c
        elif rows[c] > 32:
            assert _same(got, gn[var_nodes].reshape(-1)), c
        else:
            want = gn[var_nodes].reshape(-1)
            assert got.any() and np.linalg.norm(got - want) <= rel * np.linalg.norm(want) + 1e-14, c
    h = _check_stats(st, js)
    assert all(h[s] >= 1 for s in MUST_SHOW[name])
    # repeatable; float32 tangents are the float64 tangents of the same values
    again, _, js2 = _jvp(b, ts, gn_fallback=True)
    assert _same(xdot, again) and np.array_equal(js, js2)
    t32 = [t.astype(np.float32) for t in ts]
    x32, _, js32 = _jvp(b, t32, gn_fallback=True)
    x64, _, _ = _jvp(b, [t.astype(np.float64) for t in t32], gn_fallback=True)
    assert x32.any() and _same(x32, x64) and np.array_equal(js, js32)
    # the adjoint identity per differentiated component (test_gpu_jvp._check_adjoint, statuses 0 and 3)
    track, root, comp = p.labels()
    n1, n2 = _match_nodes(ma, g)
    ok = np.zeros(int(comp.max()) + 2, bool)
    ok[k["info"]["component"][(js == capi.JVP_OK) | (js == capi.JVP_FALLBACK)]] = True
    K = len(ok)
    u = k["gp"].cpu().numpy() * (~root[:, None] & (np.abs(k["pos"]) < 1.0))
    lhs = np.bincount(comp, (u * xdot).sum(1), K)
    nu = np.sqrt(np.bincount(comp, (u * u).sum(1), K))
    nx = np.sqrt(np.bincount(comp, (xdot * xdot).sum(1), K))
    kept = ((track[n1] == track[n2]) | (comp[n1] == comp[n2])) & ~(root[n1] & root[n2])
    cm = comp[n1]
    g1, g2, gs = back
    per_match = (g1 * ts[0]).sum(1) + (g2 * ts[1]).sum(1) + gs * ts[2]
    assert not per_match[~kept].any()
    rhs = np.bincount(cm[kept], per_match[kept], K)
    ng = np.sqrt(np.bincount(cm[kept], ((g1 * g1).sum(1) + (g2 * g2).sum(1) + gs * gs)[kept], K))
    nt = np.sqrt(np.bincount(cm[kept], ((ts[0] ** 2).sum(1) + (ts[1] ** 2).sum(1) + ts[2] ** 2)[kept], K))
    bound = 1e-8 * (nu * nx + ng * nt)
    assert (nx[ok] > 0).all()
    ratio = np.abs(lhs - rhs)[ok] / bound[ok]
    print("%s jvp: statuses %s, worst error / bound %.4f, adjoint identity over %d components, worst |lhs - rhs| / bound %.4f"
          % (name, h, worst, ok.sum(), ratio.max()))
    assert (ratio <= 1.0).all()
    assert not xdot[~ok[comp]].any()


# -------------------------------------------------------------------------------------------------------------------- 6. flags
def test_flags_and_epochs(lfr_lib, small):
    g = capi.Graph.from_arrays(small)
    b = capi.Batch(capi.Problem(g, device_graph_stage=0), 0)
    gp = _ubar(g.n_nodes, 13)
    d = _dev(_tangents(small, 11, np.float32))
    for call in (lambda: b.backward(gp, gn_fallback=True), lambda: b.jvp(*d, gn_fallback=True)):
        with pytest.raises(capi.LfrError) as e:
            call()                                               # before the first solve
        assert e.value.code == LFR_ERR_ARG
    b.solve()
    assert capi.BACKWARD_FALLBACK_GAUSS_NEWTON == capi.JVP_FALLBACK_GAUSS_NEWTON == 32
    out = torch.full((g.n_nodes, 2), 7.0, dtype=torch.float64, device=DEV)
    for extra in (0, capi.BACKWARD_F64):
        rc, outs = _raw_backward(b, gp, 32 | capi.BACKWARD_GAUSS_NEWTON | extra)
        assert rc == LFR_ERR_ARG and not any(t.any() for t in outs)
        assert _raw_jvp(b, d, 32 | capi.JVP_GAUSS_NEWTON, out) == LFR_ERR_ARG and (out == 7.0).all()
    want, _, status = _backward(b, gp, gn_fallback=True)
    rc, outs = _raw_backward(b, gp, 32 | capi.BACKWARD_F64)
    assert rc == 0 and all(_same(x.cpu().numpy(), y) for x, y in zip(outs, want))
    g1 = torch.zeros((len(small.sim), 18), dtype=torch.float32, device=DEV)
    g2, gs = torch.zeros_like(g1), torch.zeros((len(small.sim),), dtype=torch.float32, device=DEV)
    rc = capi.lib().lfr_batch_backward(b._h, C.c_void_p(gp.data_ptr()), C.c_void_p(g1.data_ptr()), C.c_void_p(g2.data_ptr()),
                                       C.c_void_p(gs.data_ptr()), 32, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and all(_same(x.cpu().numpy(), y.astype(np.float32)) for x, y in zip((g1, g2, gs), want))
    xdot, _, js = _jvp(b, [t.cpu().numpy() for t in d], gn_fallback=True)
    assert _raw_jvp(b, d, 32, out) == 0 and _same(out.cpu().numpy(), xdot)
    d64 = [t.double() for t in d]
    assert _raw_jvp(b, d64, 32 | capi.JVP_F64, out) == 0 and _same(out.cpu().numpy(), xdot)
    assert np.array_equal(js, status) and (status == capi.BACKWARD_FALLBACK).any()      # (the mode does something on this input)
    with pytest.raises(ValueError):
        b.backward(gp, gn_fallback=True, gauss_newton=True)
    with pytest.raises(ValueError):
        b.jvp(*d, gn_fallback=True, gauss_newton=True)
    # between set_inputs and the next solve the positions do not belong to the records
    f1 = torch.as_tensor(np.asarray(small.disp1, np.float32).reshape(-1, 18), device=DEV)
    f2 = torch.as_tensor(np.asarray(small.disp2, np.float32).reshape(-1, 18), device=DEV)
    b.set_inputs(f1, f2, None)
    for call in (lambda: b.backward(gp, f64=True, gn_fallback=True), lambda: b.jvp(*d, gn_fallback=True)):
        with pytest.raises(capi.LfrError) as e:
            call()
        assert e.value.code == LFR_ERR_ARG
    b.solve()
    again, _, _ = _backward(b, gp, gn_fallback=True)
    assert all(_same(x, y) for x, y in zip(want, again))


# ----------------------------------------------------------------------------------------------------------------- 7. autograd
def test_refine_and_refiner_autograd_and_forward_ad(lfr_lib, small):
    import torch.autograd.forward_ad as fwAD
    from lfr_amd.autograd import Refiner, refine
    ma, meta = small, _meta(small)
    d1, d2, sim = _leaf_tensors(ma)
    for hessian in ("newton", "exact_or_newton"):
        with pytest.raises(ValueError):
            refine(d1, d2, sim, hessian=hessian, **meta)
        with pytest.raises(ValueError):
            Refiner(d1, d2, sim, hessian=hessian, **meta)
    g, p, b = _setup(ma)
    w = _ubar(g.n_nodes, 11)
    want, _, status = _backward(b, w, gn_fallback=True)
    exact, _, _ = _backward(b, w)
    assert (status == capi.BACKWARD_FALLBACK).any() and any(not _same(x, y) for x, y in zip(want, exact))
    t = _dev(_tangents(ma, 14, np.float32))
    xdot = b.jvp(*t, gn_fallback=True).cpu().numpy()
    pos, ni, nf = refine(d1, d2, sim, hessian="exact_or_gauss_newton", **meta)
    assert _same(pos.detach().cpu().numpy(), b.download())
    (pos * w).sum().backward()
    for x, r in ((d1.grad, want[0]), (d2.grad, want[1]), (sim.grad, want[2])):
        assert r.any() and _same(x.cpu().numpy(), r.astype(np.float32))
    r = Refiner(d1.detach(), d2.detach(), sim.detach(), hessian="exact_or_gauss_newton", **meta)
    e1, e2, es = _leaf_tensors(ma)
    pos = r(e1, e2, es)
    assert _same(pos.detach().cpu().numpy(), b.download())
    (pos * w).sum().backward()
    for x, y in ((e1.grad, want[0]), (e2.grad, want[1]), (es.grad, want[2])):
        assert _same(x.cpu().numpy(), y.astype(np.float32))
    assert _same(r.jvp(*t).cpu().numpy(), xdot)
    with fwAD.dual_level():
        duals = [fwAD.make_dual(x.detach(), tt) for x, tt in zip((d1, d2, sim), t)]
        assert _same(fwAD.unpack_dual(r(*duals)).tangent.cpu().numpy(), xdot)
        assert _same(fwAD.unpack_dual(refine(*duals, hessian="exact_or_gauss_newton", **meta)[0]).tangent.cpu().numpy(), xdot)
    r.close()
