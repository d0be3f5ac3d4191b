"""The Gauss-Newton mode of the implicit-gradient backward (LFR_BACKWARD_GAUSS_NEWTON, include/lfr.h) against the CPU reference of
tests/backward_gn_ref.py, with the GPU's own positions x^: every launch class at its limits, coordinates at the bound, the components
whose exact Hessian is indefinite (what the mode is for), neighbours, repeatability, flags and epochs, autograd.

Tolerance: the project's own for the backward, |got - ref| <= 1e-8 |ref| + 1e-14 per component (test_gpu_backward).  On the hard
inputs of tests/lm_decision_cases.py only, the relative term is max(1e-8, 64 eps kappa_2(H_GN)) with kappa_2 from the reference: the
packed classes form an explicit inverse without pivoting, whose error grows with the condition number."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import backward_gn_ref as GN
import backward_ref as BR
import lm_decision_cases as LC
from test_gpu_backward import _nodes, _setup, _ubar
from test_gpu_class_limits import all_solved
from test_gpu_lm_decisions import solved
from lfr_amd import capi, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EPS = np.finfo(np.float64).eps
LFR_ERR_ARG = -1
_reference = {}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _gn(b, gp, f64=True, want_stats=False):
    out = b.backward(gp, f64=f64, want_stats=want_stats, gauss_newton=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out[:3]] + list(out[3:])


def _component_reference(variant, c, cp, x, ub):
    """(grad_flow, grad_sim, status, kappa_2) of the reference, computed once per (component, positions, dL/dx)"""
    key = (variant, c, x.tobytes(), ub.tobytes())
    if key not in _reference:
        gf, gw, rs = cp.backward(x, ub)
        _reference[key] = (gf, gw, rs, cp.kappa2(x) if rs == 0 else np.inf)
    return _reference[key]


def _check_against_reference(ma, g, p, b, gp, which, variant="ceres1", hard=False):
    """test_gpu_backward._check_against_reference for the Gauss-Newton mode -> (components compared, stats, outputs, worst error /
    bound, {component: status})"""
    g1, g2, gs, st = _gn(b, gp, want_stats=True)
    x = b.download()
    track, root, comp = p.labels()
    ni, nf = _nodes(g, ma)
    info = b.component_info()
    term = dict(zip(info["component"].tolist(), info["termination"].tolist()))
    stat = dict(zip(info["component"].tolist(), b.backward_status().tolist()))
    comps = GN.graph_components(ma, track, root, comp, ni, nf, variant, which=set(which))
    ub = gp.cpu().numpy()
    n_checked, worst = 0, 0.0
    for c in which:
        if c not in comps:
            continue
        var_nodes, cp = comps[c]
        e = cp.eids
        m, odd = e >> 1, (e & 1) == 1
        got_f = np.where(odd[:, None], g1[m], g2[m])
        got_s = gs[np.unique(m)]
        if term[c] == capi.TERM_FAILURE:
            assert stat[c] == capi.BACKWARD_NOT_USABLE and not got_f.any() and not got_s.any()
            continue
        gf, gw, rs, kappa = _component_reference(variant, c, cp, x[var_nodes].reshape(-1).copy(), ub[var_nodes].reshape(-1).copy())
        if rs == 2:
            assert stat[c] == capi.BACKWARD_INDEFINITE and not got_f.any() and not got_s.any(), "component %d" % c
            continue
        assert stat[c] == capi.BACKWARD_OK, "component %d" % c
        ref_s = np.zeros(len(ma.sim))
        np.add.at(ref_s, m, gw)
        ref = np.concatenate([gf.ravel(), ref_s[np.unique(m)]])
        got = np.concatenate([got_f.ravel(), got_s])
        rel = max(1e-8, 64.0 * EPS * kappa) if hard else 1e-8
        ratio = np.linalg.norm(got - ref) / (rel * np.linalg.norm(ref) + 1e-14)
        worst = max(worst, ratio)
        assert ratio <= 1.0, "component %d: error / bound %.3f (kappa_2 %.3e)" % (c, ratio, kappa)
        n_checked += 1
    return n_checked, st, (g1, g2, gs), worst, stat


# ------------------------------------------------------------------------------------------- 1. every launch class at its limits
@pytest.mark.parametrize("device_assembly", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
def test_every_launch_class_at_its_limits(lfr_lib, variant, device_assembly):
    s = all_solved(device_assembly, variant)
    gp = _ubar(s.g.n_nodes, 21)
    comps = s.info["component"].tolist()
    n, st, _, worst, _ = _check_against_reference(s.ma, s.g, s.p, s.b, gp, comps, variant)
    print("class limits %s/%s: %d components, worst error / bound %.4f" % (variant, "device" if device_assembly else "host", n, worst))
    assert n == len(comps) == len(s.feats)                       # every component compared: none failed, none singular
    assert (s.b.backward_status() == capi.BACKWARD_OK).all()
    assert st["n_differentiated"] == n and st["n_not_usable"] == 0 and st["n_indefinite"] == 0


# ---------------------------------------------------------------------------------------------------------------------- 2. bounds
@pytest.mark.parametrize("name", ["packed_24_32", "block_m"])
def test_components_at_the_bound(lfr_lib, name):
    ma, ref, sensitive = LC.reference(name)
    g, p, b, _, pos = solved(name)
    at_bound = LC.bound_mask(pos)
    track, root, comp = p.labels()
    which = np.setdiff1d(np.unique(comp[at_bound.any(axis=1)]), sensitive).tolist()
    n, st, _, worst, stat = _check_against_reference(ma, g, p, b, _ubar(g.n_nodes, 3), which, hard=True)
    print("%s: %d components with a coordinate at the bound, %d compared, worst error / bound %.4f, %d coordinates at a bound"
          % (name, len(which), n, worst, st["n_bound_coordinates"]))
    assert n == len(which) >= 5 and all(stat[c] == capi.BACKWARD_OK for c in which)
    assert st["n_bound_coordinates"] == int(at_bound.sum()) >= 1
    # the gradient only flows through free coordinates: a dL/dx on roots and bound coordinates gives zeros
    gp = torch.zeros((g.n_nodes, 2), dtype=torch.float64, device=DEV)
    fixed = torch.as_tensor(root[:, None] | (np.abs(pos) >= 1.0), device=DEV)
    gp[fixed] = 1.0
    assert root.any() and at_bound.any()
    assert not any(t.any() for t in _gn(b, gp))


# ----------------------------------------------------------------------------------------------------- 3. what the mode is for
def test_indefinite_components_get_a_gradient(lfr_lib):
    ma, ref, sensitive = LC.reference("packed_24_32")
    g, p, b, _, pos = solved("packed_24_32")
    gp = _ubar(g.n_nodes, 5)
    b.backward(gp, f64=True)
    exact = dict(zip(b.component_info()["component"].tolist(), b.backward_status().tolist()))
    indefinite = [c for c, s in exact.items() if s == capi.BACKWARD_INDEFINITE]
    assert len(indefinite) >= 1
    n, st, (g1, g2, gs), worst, stat = _check_against_reference(ma, g, p, b, gp, indefinite, hard=True)
    print("packed_24_32: %d components indefinite in the exact mode, %d of them differentiated and compared in Gauss-Newton mode, "
          "worst error / bound %.4f" % (len(indefinite), n, worst))
    assert n >= 1 and all(stat[c] == capi.BACKWARD_OK for c in indefinite)
    assert st["n_indefinite"] == 0 and not (b.backward_status() == capi.BACKWARD_INDEFINITE).any()
    track, root, comp = p.labels()
    ni, nf = _nodes(g, ma)
    for c, (_, cp) in BR.graph_components(ma, track, root, comp, ni, nf, which=set(indefinite)).items():
        m, odd = cp.eids >> 1, (cp.eids & 1) == 1
        assert np.where(odd[:, None], g1[m], g2[m]).any() and gs[m].any(), c


# -------------------------------------------------------------------------------------------------------------- 4. neighbours
@pytest.fixture(scope="module")
def small():
    return synthetic.generate(seed=11, n_images=48, n_tracks=400, eps_out=0.01)


@pytest.fixture(scope="module")
def small_run(lfr_lib, small):
    """the unmodified input solved once: (graph, problem, batch, dL/dx, Gauss-Newton outputs, positions, components)"""
    g, p, b = _setup(small)
    gp = _ubar(g.n_nodes, 7)
    out = _gn(b, gp)
    comps = BR.graph_components(small, *p.labels(), *_nodes(g, small))
    return g, p, b, gp, out, b.download().copy(), comps


def _others_unchanged(small_run, b, out, c_bad):
    """every component but c_bad whose positions are the same bits in both solves has the same bits in all three outputs"""
    _, _, _, _, ref, x0, comps = small_run
    x = b.download()
    n = 0
    for c, (var_nodes, cp) in comps.items():
        if c == c_bad or not _same(x[var_nodes], x0[var_nodes]):
            continue
        m = np.unique(cp.eids >> 1)
        for got, want in zip(out, ref):
            assert _same(got[m], want[m]), c
        n += 1
    assert n >= 0.9 * (len(comps) - 1)
    return n


def test_failed_component_and_its_neighbours(small, small_run):
    g0, p0, b0, gp, ref, _, comps = small_run
    c_bad = sorted(comps)[40]
    e = int(comps[c_bad][1].eids[0])
    ma = copy.deepcopy(small)
    (ma.disp1 if e & 1 else ma.disp2)[e >> 1, 4, 0] = np.inf
    g, p, b = _setup(ma)
    g1, g2, gs, st = _gn(b, gp, want_stats=True)
    info = b.component_info()
    failed = info["termination"] == capi.TERM_FAILURE
    assert failed.sum() == 1 and info["component"][failed].tolist() == [c_bad] and st["n_not_usable"] == 1
    assert (b.backward_status()[failed] == capi.BACKWARD_NOT_USABLE).all()
    m = comps[c_bad][1].eids >> 1
    assert ref[0][m].any() or ref[1][m].any()
    assert not g1[m].any() and not g2[m].any() and not gs[m].any()
    _others_unchanged(small_run, b, (g1, g2, gs), c_bad)


def test_singular_component_and_its_neighbours(small, small_run):
    g0, p0, b0, gp, ref, _, comps = small_run
    comp = p0.labels()[2]
    leaf = None
    for c in sorted(comps):                                      # a variable node with one match: similarity 0 on it unties the node
        var_nodes, cp = comps[c]
        d = np.bincount(np.concatenate([cp.src[cp.src >= 0], cp.dst[cp.dst >= 0]]), minlength=cp.nv)
        if len(var_nodes) >= 2 and (d == 2).any():               # one match = two directed edges
            l = int(np.nonzero(d == 2)[0][0])
            leaf = (c, np.unique(cp.eids[(cp.src == l) | (cp.dst == l)] >> 1))
            break
    assert leaf is not None and len(leaf[1]) == 1
    ma = copy.deepcopy(small)
    ma.sim[leaf[1]] = 0.0                                        # every match that touches the node
    g, p, b = _setup(ma)
    assert (p.labels()[2] == comp).all()                         # (the weight does not move the component structure here)
    g1, g2, gs, st = _gn(b, gp, want_stats=True)
    info = b.component_info()
    sing = b.backward_status() == capi.BACKWARD_INDEFINITE
    assert st["n_indefinite"] == 1 and info["component"][sing].tolist() == [leaf[0]]
    m = comps[leaf[0]][1].eids >> 1
    assert ref[0][m].any() or ref[1][m].any()
    assert not g1[m].any() and not g2[m].any() and not gs[m].any()
    _others_unchanged(small_run, b, (g1, g2, gs), leaf[0])


# ------------------------------------------------------------------------------------------- 5. repeatability and assembly
def test_calls_repeat_f32_rounds_f64_assemblies_agree_shards_sum(small, small_run):
    g, p, b, gp, a, _, _ = small_run
    c = _gn(b, gp)
    f = _gn(b, gp, f64=False)
    for x, y, z in zip(a, c, f):
        assert x.any() and _same(x, y)                           # bitwise repeatable
        assert z.dtype == np.float32 and _same(z, x.astype(np.float32))
    _, _, bd = _setup(small, device_assembly=True)
    for x, y in zip(a, _gn(bd, gp)):
        assert _same(x, y)
    for world in (2, 4):
        acc = [np.zeros_like(x) for x in a]
        for r in range(world):
            bs = capi.Batch(p, 0, r, world)
            bs.solve()
            for s, t in zip(acc, _gn(bs, gp)):
                s += t
        for x, y in zip(a, acc):
            assert np.abs(x - y).max() == 0.0, world


# ------------------------------------------------------------------------------------------------------- 6. flags and epochs
def _raw_backward(b, gp, flags):
    n, m = b.problem.graph.n_nodes, b.problem.graph.n_edges // 2
    g1 = torch.zeros((m, 18), dtype=torch.float64, device=DEV)
    g2 = torch.zeros_like(g1)
    gs = torch.zeros((m,), dtype=torch.float64, device=DEV)
    rc = capi.lib().lfr_batch_backward(b._h, C.c_void_p(gp.data_ptr()), C.c_void_p(g1.data_ptr()), C.c_void_p(g2.data_ptr()),
                                       C.c_void_p(gs.data_ptr()), flags, None, None)
    torch.cuda.synchronize()
    return rc, (g1, g2, gs)


def test_flags_and_epochs(lfr_lib, small):
    g, p, b = _setup(small, device_assembly=True)
    gp = _ubar(g.n_nodes, 13)
    x0 = b.download().copy()
    exact_alone = [t.cpu().numpy() for t in b.backward(gp, f64=True)]
    status_alone = b.backward_status().copy()
    for flags in (4, 8, 4 | capi.BACKWARD_F64, 8 | capi.BACKWARD_GAUSS_NEWTON):
        rc, out = _raw_backward(b, gp, flags)
        assert rc == LFR_ERR_ARG and not any(t.any() for t in out), flags
    rc, out = _raw_backward(b, gp, capi.BACKWARD_F64 | capi.BACKWARD_GAUSS_NEWTON)
    gn = _gn(b, gp)
    assert rc == 0 and all(_same(x.cpu().numpy(), y) for x, y in zip(out, gn))
    assert any(not _same(x, y) for x, y in zip(gn, exact_alone))                 # (the mode does something)
    # an exact-mode call after a Gauss-Newton call is an exact-mode call alone
    for x, y in zip([t.cpu().numpy() for t in b.backward(gp, f64=True)], exact_alone):
        assert _same(x, y)
    assert np.array_equal(b.backward_status(), status_alone)
    assert _same(b.download(), x0)
    # between set_inputs and the next solve the positions do not belong to the records
    d1 = torch.as_tensor(np.asarray(small.disp1, np.float32).reshape(-1, 18), device=DEV)
    d2 = torch.as_tensor(np.asarray(small.disp2, np.float32).reshape(-1, 18), device=DEV)
    b.set_inputs(d1, d2, None)
    with pytest.raises(capi.LfrError) as e:
        b.backward(gp, f64=True, gauss_newton=True)
    assert e.value.code == LFR_ERR_ARG
    b.solve()
    assert _same(b.download(), x0)
    for x, y in zip(_gn(b, gp), gn):
        assert _same(x, y)


# ----------------------------------------------------------------------------------------------------------------- 7. autograd
def _leaf_tensors(ma, scale=1.0):
    d1 = torch.as_tensor(np.asarray(ma.disp1, np.float32).reshape(-1, 18) * np.float32(scale), device=DEV).requires_grad_(True)
    d2 = torch.as_tensor(np.asarray(ma.disp2, np.float32).reshape(-1, 18) * np.float32(scale), device=DEV).requires_grad_(True)
    sim = torch.as_tensor(np.asarray(ma.sim, np.float32), device=DEV).requires_grad_(True)
    return d1, d2, sim


def test_refine_and_refiner_autograd(lfr_lib):
    from lfr_amd.autograd import Refiner, refine
    ma = synthetic.config3_standin()
    meta = dict(image_names=ma.image_names, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off, feat1=ma.feat1,
                feat2=ma.feat2, image_facts=ma.facts)
    d1, d2, sim = _leaf_tensors(ma)
    with pytest.raises(ValueError):
        refine(d1, d2, sim, hessian="newton", **meta)
    with pytest.raises(ValueError):
        Refiner(d1, d2, sim, hessian="newton", **meta)
    pos, ni, nf = refine(d1, d2, sim, hessian="gauss_newton", **meta)
    g, p, b = _setup(ma)
    assert _same(pos.detach().cpu().numpy(), b.download())
    w = _ubar(g.n_nodes, 11)
    (pos * w).sum().backward()
    want = _gn(b, w)
    exact = [t.cpu().numpy() for t in b.backward(w, f64=True)]
    assert any(not _same(x, y) for x, y in zip(want, exact))
    for t, r in ((d1.grad, want[0]), (d2.grad, want[1]), (sim.grad, want[2])):
        assert r.any() and _same(t.cpu().numpy(), r.astype(np.float32))
    # Refiner: two steps, the second with changed flows
    r = Refiner(d1.detach(), d2.detach(), sim.detach(), hessian="gauss_newton", **meta)
    for step, scale in enumerate((1.0, 0.97)):
        e1, e2, es = _leaf_tensors(ma, scale)
        pos = r(e1, e2, es)
        (pos * w).sum().backward()
        mb = copy.deepcopy(ma)
        mb.disp1 = e1.detach().cpu().numpy().reshape(np.asarray(ma.disp1).shape)
        mb.disp2 = e2.detach().cpu().numpy().reshape(np.asarray(ma.disp2).shape)
        gb, pb, bb = _setup(mb)
        assert _same(pos.detach().cpu().numpy(), bb.download()), step
        want = _gn(bb, w)
        for t, x in ((e1.grad, want[0]), (e2.grad, want[1]), (es.grad, want[2])):
            assert x.any() and _same(t.cpu().numpy(), x.astype(np.float32)), step
    r.close()
