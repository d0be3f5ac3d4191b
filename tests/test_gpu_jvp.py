"""Forward-mode sensitivity of the refined positions (lfr_batch_jvp, include/lfr.h) against the CPU reference of tests/jvp_ref.py with
the GPU's own positions x^, and against lfr_batch_backward through the adjoint identity ubar . (J thetadot) = (J^T ubar) . thetadot,
which needs no reference and runs in every kernel class and both Hessian modes.

Tolerances: against the reference the project's own for the backward, |got - ref| <= 1e-8 |ref| + 1e-14 per component
(test_gpu_backward); the adjoint identity the sum of the two passes' reference tolerances, 1e-8 (|ubar_c| |xdot_c| + |g_c| |thetadot_c|).
The 95 % of test_standins_match_reference carries over: the reference's H and its Cholesky are Component.backward's, so the
components it leaves indefinite are the same ones at the same x^."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import backward_ref as BR
import jvp_ref as JR
from test_gpu_backward import _nodes, _setup, _ubar
from lfr_amd import capi, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LFR_ERR_ARG, LFR_ERR_UNSUPPORTED = -1, -5
MODES = pytest.mark.parametrize("gn", [False, True], ids=["exact", "gauss_newton"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _tangents(ma, seed, dtype=np.float64):
    """random (tan_disp1, tan_disp2, tan_sim) in the match layout, as numpy"""
    rng = np.random.default_rng(seed)
    m = len(ma.sim)
    return [rng.standard_normal((m, 18)).astype(dtype), rng.standard_normal((m, 18)).astype(dtype), rng.standard_normal(m).astype(dtype)]


def _dev(ts):
    return [None if t is None else torch.as_tensor(t, device=DEV) for t in ts]


def _jvp(b, ts, gn=False, **kw):
    f64 = next(t for t in ts if t is not None).dtype == np.float64
    out = b.jvp(*_dev(ts), f64=f64, gauss_newton=gn, **kw)
    torch.cuda.synchronize()
    return (out[0].cpu().numpy(), out[1]) if kw.get("want_stats") else out.cpu().numpy()


def _by_component(info, arr):
    return dict(zip(info["component"].tolist(), arr.tolist()))


# ------------------------------------------------------------------------------------------------------ 1. the reference
def _check_against_reference(ma, g, p, b, ts, which, gn, variant="ceres1"):
    """`variant`: the Tukey variant the batch `b` was created with (the reference's components take it)"""
    xdot, st = _jvp(b, ts, gn, want_stats=True)
    x = b.download()
    info = b.component_info()
    term, stat = _by_component(info, info["termination"]), _by_component(info, b.jvp_status())
    comps = BR.graph_components(ma, *p.labels(), *_nodes(g, ma), variant, which=set(which))
    n_checked, worst = 0, 0.0
    usable = [c for c in which if c in comps and term[c] != capi.TERM_FAILURE]
    items = []
    for c in usable:
        var_nodes, cp = comps[c]
        m, odd = cp.eids >> 1, (cp.eids & 1) == 1
        items.append((cp, x[var_nodes].reshape(-1), np.where(odd[:, None], ts[0][m], ts[1][m]), ts[2][m]))
    reference = dict(zip(usable, JR.jvp_many(items, gauss_newton=gn)))      # (one torch program for all of them)
    for c in which:
        if c not in comps:
            continue
        var_nodes, cp = comps[c]
        got = xdot[var_nodes].reshape(-1)
        if term[c] == capi.TERM_FAILURE:
            assert stat[c] == capi.JVP_NOT_USABLE and not got.any()
            continue
        ref, rs = reference[c]
        if rs == 2:
            assert stat[c] == capi.JVP_INDEFINITE and not got.any(), "component %d" % c
            continue
        assert stat[c] == capi.JVP_OK, "component %d" % c
        bound = 1e-8 * np.linalg.norm(ref) + 1e-14
        worst = max(worst, np.linalg.norm(got - ref) / bound)
        assert np.linalg.norm(got - ref) <= bound, "component %d: error / bound %.3f" % (c, np.linalg.norm(got - ref) / bound)
        assert not got[np.abs(x[var_nodes].reshape(-1)) >= 1.0].any()
        n_checked += 1
    return n_checked, st, xdot, worst


@MODES
@pytest.mark.parametrize("name", ["config1", "config3"])
def test_standins_match_reference(lfr_lib, name, gn):
    ma = synthetic.config1_standin() if name == "config1" else synthetic.config3_standin()
    g, p, b = _setup(ma)
    comps = b.component_info()["component"].tolist()
    n, st, _, worst = _check_against_reference(ma, g, p, b, _tangents(ma, 1), comps, gn)
    print("%s %s: %d of %d components compared, worst error / bound %.4f, stats %s" % (name, "gn" if gn else "exact", n, len(comps), worst, st))
    assert n >= 0.95 * len(comps)
    assert st["n_differentiated"] + st["n_not_usable"] + st["n_indefinite"] == len(comps) and st["n_differentiated"] >= n


@pytest.fixture(scope="module")
def config5_run(lfr_lib):
    ma = synthetic.config5()
    g, p, b = _setup(ma)
    info = b.component_info()
    rows = 2 * info["n_var_nodes"]
    which = np.random.default_rng(5).choice(info["component"], size=min(300, len(rows)), replace=False).tolist()
    which += info["component"][np.argsort(rows)[-5:]].tolist()
    return ma, g, p, b, which, rows


@pytest.fixture(scope="module")
def capsized_run(lfr_lib):
    ma = synthetic.capsized_sparse(n_tracks=2500, seed=7)
    g, p, b = _setup(ma)
    info = b.component_info()
    rows = 2 * info["n_var_nodes"]
    return ma, g, p, b, info["component"][rows > 192].tolist(), rows


@MODES
def test_config5_workgroup_classes_match_reference(config5_run, gn):
    ma, g, p, b, which, rows = config5_run
    n, st, _, worst = _check_against_reference(ma, g, p, b, _tangents(ma, 2), which, gn)
    print("config 5 %s: %d components compared, worst error / bound %.4f, jvp %.3f ms" % ("gn" if gn else "exact", n, worst, st["kernel_ms"]))
    assert n >= 250 and rows.max() > 88


@MODES
def test_cap_sized_sparse_matches_reference(capsized_run, gn):
    ma, g, p, b, big, rows = capsized_run
    assert len(big) >= 3 and rows.max() >= 2000
    n, st, _, worst = _check_against_reference(ma, g, p, b, _tangents(ma, 3), big, gn)
    status = b.jvp_status()[rows > 192]
    print("cap-sized %s: %d components above 192 rows, %d compared, worst error / bound %.4f, jvp %.3f ms"
          % ("gn" if gn else "exact", len(big), n, worst, st["kernel_ms"]))
    assert n >= 1 and n == (status == capi.JVP_OK).sum()


# ------------------------------------------------------------------------------------------------- 2. the adjoint identity
def _match_nodes(ma, g):
    ni, nf = _nodes(g, ma)
    key = ni.astype(np.int64) << 32 | nf.astype(np.int64)
    order = np.argsort(key)
    pi = np.repeat(np.arange(len(ma.pair_img1)), np.diff(ma.pair_off))
    k1 = ma.pair_img1[pi].astype(np.int64) << 32 | ma.feat1.astype(np.int64)
    k2 = ma.pair_img2[pi].astype(np.int64) << 32 | ma.feat2.astype(np.int64)
    return order[np.searchsorted(key[order], k1)], order[np.searchsorted(key[order], k2)]


def _check_adjoint(ma, g, p, b, gn, seed):
    """per component with status 0 in both passes: |ubar_c . xdot_c - <g_c, thetadot_c>| <= 1e-8 (|ubar_c| |xdot_c| + |g_c| |thetadot_c|),
    ubar_c over the component's free coordinates, thetadot_c over its kept edges with a variable end -> (components, worst ratio)"""
    ts = _tangents(ma, seed)
    ub = _ubar(g.n_nodes, seed + 100)
    xdot = _jvp(b, ts, gn)
    js = b.jvp_status().copy()
    g1, g2, gs = [t.cpu().numpy() for t in b.backward(ub, f64=True, gauss_newton=gn)]
    assert np.array_equal(js, b.backward_status())
    track, root, comp = p.labels()
    x = b.download()
    n1, n2 = _match_nodes(ma, g)
    info = b.component_info()
    ok = np.zeros(int(comp.max()) + 2, bool)
    ok[info["component"][js == capi.JVP_OK]] = True
    K = len(ok)
    u = ub.cpu().numpy() * (~root[:, None] & (np.abs(x) < 1.0))
    lhs = np.bincount(comp, (u * xdot).sum(1), K)
    nu = np.sqrt(np.bincount(comp, (u * u).sum(1), K))
    nx = np.sqrt(np.bincount(comp, (xdot * xdot).sum(1), K))
    kept = ((track[n1] == track[n2]) | (comp[n1] == comp[n2])) & ~(root[n1] & root[n2])
    cm = comp[n1]
    per_match = (g1 * ts[0]).sum(1) + (g2 * ts[1]).sum(1) + gs * ts[2]
    assert not per_match[~kept].any()
    rhs = np.bincount(cm[kept], per_match[kept], K)
    ng = np.sqrt(np.bincount(cm[kept], ((g1 * g1).sum(1) + (g2 * g2).sum(1) + gs * gs)[kept], K))
    nt = np.sqrt(np.bincount(cm[kept], ((ts[0] ** 2).sum(1) + (ts[1] ** 2).sum(1) + ts[2] ** 2)[kept], K))
    bound = 1e-8 * (nu * nx + ng * nt)
    err = np.abs(lhs - rhs)
    live = ok & (nx > 0)
    assert live.sum() >= 0.9 * ok.sum()
    ratio = err[live] / bound[live]
    bad = np.nonzero(live)[0][ratio > 1.0]
    assert len(bad) == 0, "components %s: |lhs - rhs| / bound up to %.3f" % (bad[:5].tolist(), ratio.max())
    assert not xdot[~ok[comp]].any()
    return int(live.sum()), float(ratio.max()), js


@pytest.fixture(scope="module")
def small():
    return synthetic.generate(seed=11, n_images=48, n_tracks=400, eps_out=0.01)


@pytest.fixture(scope="module")
def small_run(lfr_lib, small):
    g, p, b = _setup(small)
    return g, p, b


@MODES
@pytest.mark.parametrize("name", ["small", "config5", "capsized"])
def test_adjoint_identity_with_the_backward(request, name, gn):
    if name == "small":
        ma, (g, p, b) = request.getfixturevalue("small"), request.getfixturevalue("small_run")
    else:
        ma, g, p, b = request.getfixturevalue(name + "_run")[:4]
    n, worst, js = _check_adjoint(ma, g, p, b, gn, 4)
    info = b.component_info()
    rows = 2 * info["n_var_nodes"][js == capi.JVP_OK] if gn else 2 * info["n_var_nodes"]      # (exact mode: the largest may be indefinite)
    print("%s %s: %d components, worst |lhs - rhs| / bound %.4f, rows %d..%d" % (name, "gn" if gn else "exact", n, worst, rows.min(), rows.max()))
    if name == "small":
        assert rows.min() <= 8 and n >= 50
    elif name == "config5":
        assert rows.max() > 130 and (rows <= 32).any()
    else:
        assert rows.max() > 192


# --------------------------------------------------------------------------------------------------------------- 3. zeros
def _leaf_match(comps):
    """(component, its match) of a variable node with one match: similarity 0 on it unties the node (test_gpu_backward_gn)"""
    for c in sorted(comps):
        var_nodes, cp = comps[c]
        d = np.bincount(np.concatenate([cp.src[cp.src >= 0], cp.dst[cp.dst >= 0]]), minlength=cp.nv)
        if len(var_nodes) >= 2 and (d == 2).any():
            l = int(np.nonzero(d == 2)[0][0])
            return c, np.unique(cp.eids[(cp.src == l) | (cp.dst == l)] >> 1)
    raise AssertionError("no leaf")


@MODES
def test_zeros_where_the_contract_says_zero(small, small_run, gn):
    g0, p0, b0 = small_run
    comps = BR.graph_components(small, *p0.labels(), *_nodes(g0, small))
    ref = _jvp(b0, _tangents(small, 5), gn)
    ma = copy.deepcopy(small)
    ids = sorted(comps)
    for c in ids[10:30]:                                         # large flows push these components' nodes to the bound
        m = comps[c][1].eids >> 1
        ma.disp1[m] *= 40.0
        ma.disp2[m] *= 40.0
    c_fail = ids[40]
    e = int(comps[c_fail][1].eids[0])
    (ma.disp1 if e & 1 else ma.disp2)[e >> 1, 4, 0] = np.nan     # FAILURE component
    c_sing, m_leaf = _leaf_match({c: comps[c] for c in ids[50:]})
    ma.sim[m_leaf] = 0.0                                         # Gauss-Newton: singular; exact: indefinite
    g, p, b = _setup(ma)
    track, root, comp = p.labels()
    assert (comp == p0.labels()[2]).all()
    x = b.download()
    xdot, st = _jvp(b, _tangents(small, 5), gn, want_stats=True)
    info = b.component_info()
    stat, term = _by_component(info, b.jvp_status()), _by_component(info, info["termination"])
    bound = np.abs(x) >= 1.0
    assert bound.sum() >= 3 and st["n_bound_coordinates"] >= 3 and root.any()
    assert not xdot[bound].any() and not xdot[root].any()
    solved = np.isin(comp, info["component"])
    assert not xdot[~solved].any()
    assert term[c_fail] == capi.TERM_FAILURE and stat[c_fail] == capi.JVP_NOT_USABLE and st["n_not_usable"] == 1
    assert ref[comps[c_fail][0]].any() and not xdot[comps[c_fail][0]].any()
    assert stat[c_sing] == capi.JVP_INDEFINITE and st["n_indefinite"] >= 1
    assert (ref[comps[c_sing][0]].any() or not gn) and not xdot[comps[c_sing][0]].any()      # (exact mode: it may have been indefinite before)
    for c, s in stat.items():
        if s != capi.JVP_OK and c in comps:
            assert not xdot[comps[c][0]].any()
    # a component with a coordinate at the bound still gets the tangent of its free coordinates
    with_bound = [c for c in ids[10:30] if stat[c] == capi.JVP_OK and bound[comps[c][0]].any() and not bound[comps[c][0]].all()]
    print("%s: %d coordinates at a bound, %d components with bound and free coordinates differentiated" % ("gn" if gn else "exact", bound.sum(), len(with_bound)))
    assert (with_bound or not gn) and all(xdot[comps[c][0]].any() for c in with_bound)      # (exact mode: such a component may be indefinite)
    # the untouched components keep their bits
    same = [c for c in ids[60:] if c != c_sing and _same(x[comps[c][0]], b0.download()[comps[c][0]])]
    assert len(same) >= 0.9 * len(ids[60:]) and all(_same(xdot[comps[c][0]], ref[comps[c][0]]) for c in same)


# ------------------------------------------------------------------------------------------------- 4. a tangent that is not finite
@MODES
def test_nonfinite_tangent_stays_in_its_component(small, small_run, gn):
    g, p, b = small_run
    comps = BR.graph_components(small, *p.labels(), *_nodes(g, small))
    info = b.component_info()
    ts = _tangents(small, 6)
    ref = _jvp(b, ts, gn)
    status = b.jvp_status().copy()
    stat, rows = _by_component(info, status), _by_component(info, 2 * info["n_var_nodes"])
    # components of the 8-row class sit eight to a wave in the batch order: take one from the middle of that class
    small_ones = [c for c in info["component"].tolist() if c in comps and rows[c] <= 8 and stat[c] == capi.JVP_OK]
    assert len(small_ones) >= 16
    c_bad = small_ones[len(small_ones) // 2 + 3]
    for which, val in ((0, np.nan), (2, np.inf)):
        t = [a.copy() for a in ts]
        e = int(comps[c_bad][1].eids[0])
        if which == 0:
            (t[0] if e & 1 else t[1])[e >> 1, 7] = val
        else:
            t[2][e >> 1] = val
        got = _jvp(b, t, gn)
        assert np.array_equal(b.jvp_status(), status)            # the status stays 0
        mine = np.zeros(len(got), bool)
        mine[comps[c_bad][0]] = True
        assert not np.isfinite(got[mine]).all()
        assert _same(got[~mine], ref[~mine])                     # nobody else changes by a bit


# ----------------------------------------------------------------------------------------------------------- 5. linearity
@MODES
def test_linearity(small, small_run, gn):
    g, p, b = small_run
    t1, t2 = _tangents(small, 7), _tangents(small, 8)
    a, c = 0.75, -2.5
    lhs = _jvp(b, [a * x + c * y for x, y in zip(t1, t2)], gn)
    j1, j2 = _jvp(b, t1, gn), _jvp(b, t2, gn)
    comp = p.labels()[2]
    K = int(comp.max()) + 1
    err = np.sqrt(np.bincount(comp, ((lhs - (a * j1 + c * j2)) ** 2).sum(1), K))
    scale = abs(a) * np.sqrt(np.bincount(comp, (j1 ** 2).sum(1), K)) + abs(c) * np.sqrt(np.bincount(comp, (j2 ** 2).sum(1), K))
    live = scale > 0
    print("linearity %s: worst error / scale %.3e over %d components" % ("gn" if gn else "exact", (err[live] / scale[live]).max(), live.sum()))
    assert live.sum() >= 50 and (err[live] <= 1e-12 * scale[live]).all()


# -------------------------------------------------------------------------------------------------------- 6. input arguments
@MODES
def test_input_forms(small, small_run, gn):
    g, p, b = small_run
    t1, t2, ts = _tangents(small, 9, np.float32)
    z18, z1 = np.zeros_like(t1), np.zeros_like(ts)
    full = _jvp(b, [t1, t2, ts], gn)
    assert full.any()
    assert _same(_jvp(b, [t1, t2, None], gn), _jvp(b, [t1, t2, z1], gn))
    assert _same(_jvp(b, [None, None, ts], gn), _jvp(b, [z18, z18, ts], gn))
    assert _same(full, _jvp(b, [t1.astype(np.float64), t2.astype(np.float64), ts.astype(np.float64)], gn))
    assert _same(full, b.jvp(*[t.reshape(-1, 9, 2) if t.dim() == 2 else t for t in _dev([t1, t2, ts])], gauss_newton=gn).cpu().numpy())
    d = _dev([t1, t2, ts])
    for kw in (dict(tan_disp1=d[0].double(), tan_disp2=d[1]), dict(tan_sim=d[2].cpu()), dict(tan_disp1=d[0][:-1], tan_disp2=d[1][:-1]),
               dict(tan_sim=ts)):
        with pytest.raises(ValueError):
            b.jvp(**kw)


# ------------------------------------------------------------------------------------------------ 7. repeatability and assembly
@MODES
def test_calls_repeat_assemblies_agree_shards_sum_and_nothing_else_moves(small, small_run, gn):
    g, p, b = small_run
    ts = _tangents(small, 10)
    gp = _ubar(g.n_nodes, 12)
    x0, info0 = b.download().copy(), b.component_info()
    back0 = [t.cpu().numpy() for t in b.backward(gp, f64=True, gauss_newton=gn)]
    a = _jvp(b, ts, gn)
    assert a.any() and _same(a, _jvp(b, ts, gn))                  # bitwise repeatable
    assert _same(b.download(), x0)
    info1 = b.component_info()
    assert all(np.array_equal(info0[k], info1[k]) for k in info0)
    for x, y in zip(back0, [t.cpu().numpy() for t in b.backward(gp, f64=True, gauss_newton=gn)]):
        assert _same(x, y)
    _, _, bd = _setup(small, device_assembly=True)
    assert _same(a, _jvp(bd, ts, gn))
    acc = np.zeros_like(a)
    for r in range(2):
        bs = capi.Batch(p, 0, r, 2)
        bs.solve()
        part = _jvp(bs, ts, gn)
        assert part.any()
        acc += part
    assert np.abs(a - acc).max() == 0.0


# ----------------------------------------------------------------------------------------------------------------- 8. errors
def _raw_jvp(b, d, flags, out):
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = capi.lib().lfr_batch_jvp(b._h, ptr(d[0]), ptr(d[1]), ptr(d[2]), C.c_void_p(out.data_ptr()), flags, None, None)
    torch.cuda.synchronize()
    return rc


def test_errors(lfr_lib, small):
    g = capi.Graph.from_arrays(small)
    p = capi.Problem(g, device_graph_stage=0)
    b = capi.Batch(p, 0)
    d = _dev(_tangents(small, 11, np.float32))
    out = torch.full((g.n_nodes, 2), 7.0, dtype=torch.float64, device=DEV)
    with pytest.raises(capi.LfrError) as e:
        b.jvp(*d)                                                # before the first solve
    assert e.value.code == LFR_ERR_ARG
    with pytest.raises(capi.LfrError) as e:
        b.jvp_status()
    assert e.value.code == LFR_ERR_ARG
    b.solve()
    ok = b.jvp(*d).cpu().numpy()
    assert _raw_jvp(b, [None, None, None], 0, out) == LFR_ERR_ARG
    assert _raw_jvp(b, [d[0], None, d[2]], 0, out) == LFR_ERR_ARG and _raw_jvp(b, [None, d[1], None], 0, out) == LFR_ERR_ARG
    for flags in (4, 8, 4 | capi.JVP_F64, 16 | capi.JVP_GAUSS_NEWTON):
        assert _raw_jvp(b, d, flags, out) == LFR_ERR_ARG, flags
    assert (out == 7.0).all()                                    # a refused call writes nothing
    assert _raw_jvp(b, d, 0, out) == 0 and _same(out.cpu().numpy(), ok)
    f1 = torch.as_tensor(np.asarray(small.disp1, np.float32).reshape(-1, 18), device=DEV)
    f2 = torch.as_tensor(np.asarray(small.disp2, np.float32).reshape(-1, 18), device=DEV)
    b.set_inputs(f1, f2, None)
    with pytest.raises(capi.LfrError) as e:
        b.jvp(*d)                                                # between set_inputs and the next solve
    assert e.value.code == LFR_ERR_ARG and "inputs changed since the latest solve" in str(e.value)
    b.solve()
    assert _same(b.jvp(*d).cpu().numpy(), ok)
    # a batch over one rank's connected components numbers its matches by itself: refused
    mc = synthetic.generate(seed=32, n_images=48, n_tracks=3000, eps_out=0.002)
    g2 = capi.Graph.from_arrays(mc)
    p2 = capi.Problem(g2, device_graph_stage=0, shard=(0, 2))
    assert p2.cc_sharded
    b2 = capi.Batch(p2, 0)
    b2.solve()
    with pytest.raises(capi.LfrError) as e:
        b2.jvp(*_dev(_tangents(mc, 1, np.float32)))
    assert e.value.code == LFR_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------- 9. set_inputs ordering
@MODES
def test_set_inputs_on_another_stream_waits_for_the_jvp(lfr_lib, small, gn):
    g, p, b = _setup(small, device_assembly=True)
    d = _dev(_tangents(small, 13, np.float32))
    want = b.jvp(*d, gauss_newton=gn)
    torch.cuda.synchronize()
    f1 = torch.as_tensor(np.asarray(small.disp1, np.float32).reshape(-1, 18) * np.float32(3.0), device=DEV)
    f2 = torch.as_tensor(np.asarray(small.disp2, np.float32).reshape(-1, 18) * np.float32(3.0), device=DEV)
    sim = torch.zeros(len(small.sim), dtype=torch.float32, device=DEV)
    other = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    got = b.jvp(*d, gauss_newton=gn)                             # on torch's current stream, not waited for
    b.set_inputs(f1, f2, sim, stream=other.cuda_stream)          # rewrites every record on another stream
    torch.cuda.synchronize()
    assert _same(got.cpu().numpy(), want.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ 10. torch
def _meta(ma):
    return dict(image_names=ma.image_names, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off, feat1=ma.feat1,
                feat2=ma.feat2, image_facts=ma.facts)


@pytest.mark.parametrize("hessian", ["exact", "gauss_newton"])
def test_refiner_jvp_and_forward_ad_with_a_banned_image(lfr_lib, small, hessian):
    import torch.autograd.forward_ad as fwAD
    from lfr_amd.autograd import Refiner, refine
    ma, gn, banned = small, hessian == "gauss_newton", ("000005.png",)
    assert banned[0] in ma.image_names
    f1 = torch.as_tensor(np.asarray(ma.disp1, np.float32).reshape(-1, 18), device=DEV)
    f2 = torch.as_tensor(np.asarray(ma.disp2, np.float32).reshape(-1, 18), device=DEV)
    sim = torch.as_tensor(np.asarray(ma.sim, np.float32), device=DEV)
    t1, t2, ts = _dev(_tangents(ma, 14, np.float32))
    r = Refiner(f1, f2, sim, banned=banned, hessian=hessian, **_meta(ma))
    assert r._idx is not None and len(r._idx) < r.n_rows          # the caller's rows are not the graph's
    with pytest.raises(RuntimeError):
        r.jvp(t1, t2, ts)                                        # before the first forward
    a = [f1.clone().requires_grad_(True), f2.clone().requires_grad_(True), sim.clone().requires_grad_(True)]
    pos = r(*a)
    xdot = r.jvp(t1, t2, ts)
    assert not xdot.requires_grad and tuple(xdot.shape) == (r.n_nodes, 2) and xdot.any()
    # the batch's own jvp on the graph's rows
    want = r._batch.jvp(t1[r._idx].contiguous(), t2[r._idx].contiguous(), ts[r._idx].contiguous(), gauss_newton=gn)
    assert _same(xdot.cpu().numpy(), want.cpu().numpy())
    assert _same(r.jvp(t1, t2).cpu().numpy(), r._batch.jvp(t1[r._idx].contiguous(), t2[r._idx].contiguous(), gauss_newton=gn).cpu().numpy())
    with pytest.raises(ValueError):
        r.jvp(None, None, None)
    # reverse mode on the same forward: sum(grad * tangent) = w . xdot within the adjoint identity's tolerance
    w = _ubar(r.n_nodes, 15)
    (pos * w).sum().backward()
    rev = sum(float((x.grad.double() * t.double()).sum()) for x, t in zip(a, (t1, t2, ts)))
    scale = float(w.norm() * xdot.norm()) + float(torch.cat([x.grad.double().reshape(-1) for x in a]).norm()
                                                   * torch.cat([t.double().reshape(-1) for t in (t1, t2, ts)]).norm())
    # forward mode through Refiner.__call__ and through refine()
    with fwAD.dual_level():
        duals = [fwAD.make_dual(x, t) for x, t in zip((f1, f2, sim), (t1, t2, ts))]
        p_r, tan_r = fwAD.unpack_dual(r(*duals))
        assert _same(tan_r.cpu().numpy(), xdot.cpu().numpy()) and _same(p_r.cpu().numpy(), pos.detach().cpu().numpy())
        fwd = float(fwAD.unpack_dual((r(*duals) * w).sum()).tangent)
        out = refine(*duals, banned=banned, hessian=hessian, **_meta(ma))
        p_f, tan_f = fwAD.unpack_dual(out[0])
        assert _same(p_f.cpu().numpy(), p_r.cpu().numpy()) and _same(tan_f.cpu().numpy(), xdot.cpu().numpy())
    print("%s: forward %.12e reverse %.12e, |difference| / bound %.4f" % (hessian, fwd, rev, abs(fwd - rev) / (1e-8 * scale)))
    assert abs(fwd - rev) <= 1e-8 * scale
    # a stale forward raises: the dual output of an older step cannot be produced after the next forward
    ctx_epoch = r._epoch
    r(f1, f2, sim)
    assert r._epoch == ctx_epoch + 1
    from lfr_amd.autograd import _RefinerStep

    class _Ctx:
        refiner, epoch = r, ctx_epoch
    with pytest.raises(RuntimeError, match="stale"):
        _RefinerStep.jvp(_Ctx, t1, t2, ts, None)
    r.close()
    with pytest.raises(RuntimeError):
        r.jvp(t1, t2, ts)
