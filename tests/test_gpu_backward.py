"""Implicit-gradient backward through the batched LM solve (lfr_batch_backward, include/lfr.h) against the CPU reference of
tests/backward_ref.py, with the GPU's own positions x^."""
import copy

import numpy as np
import pytest
import torch

import backward_ref as BR
from lfr_amd import capi, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _setup(ma, variant="ceres1", device_assembly=False, shard=(0, 1)):
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g, device_graph_stage=0) if device_assembly else capi.Problem(g)
    b = capi.Batch(p, 0, shard[0], shard[1], tukey_variant=variant)
    b.solve()
    return g, p, b


def _nodes(g, ma):
    """node -> (image index of `ma`, feature): the graph numbers images in order of first appearance"""
    ni, nf = g.nodes()
    idx = {n: i for i, n in enumerate(ma.image_names)}
    return np.array([idx[n] for n in g.image_names()], np.int32)[ni], nf


def _ubar(n, seed=0):
    return torch.as_tensor(np.random.default_rng(seed).standard_normal((n, 2)), device=DEV)


def _gpu_f64(b, gp):
    g1, g2, gs, st = b.backward(gp, f64=True, want_stats=True)
    torch.cuda.synchronize()
    return g1.cpu().numpy(), g2.cpu().numpy(), gs.cpu().numpy(), st


def _check_against_reference(ma, g, p, b, gp, which, variant="ceres1"):
    g1, g2, gs, st = _gpu_f64(b, gp)
    x = b.download()
    track, root, comp = p.labels()
    ni, nf = _nodes(g, ma)
    info = b.component_info()
    status = b.backward_status()
    term = dict(zip(info["component"].tolist(), info["termination"].tolist()))
    stat = dict(zip(info["component"].tolist(), status.tolist()))
    comps = BR.graph_components(ma, track, root, comp, ni, nf, variant, which=set(which))
    ub = gp.cpu().numpy()
    n_checked = 0
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
        gf, gw, rs = cp.backward(x[var_nodes].reshape(-1), ub[var_nodes].reshape(-1))
        if rs == 2:
            assert stat[c] == capi.BACKWARD_INDEFINITE and not got_f.any() and not got_s.any()
            continue
        assert stat[c] == capi.BACKWARD_OK
        ref_s = np.zeros(len(ma.sim))
        np.add.at(ref_s, m, gw)
        ref = np.concatenate([gf.ravel(), ref_s[np.unique(m)]])
        got = np.concatenate([got_f.ravel(), got_s])
        assert np.linalg.norm(got - ref) <= 1e-8 * np.linalg.norm(ref) + 1e-14, "component %d" % c
        n_checked += 1
    return n_checked, st, (g1, g2, gs)


@pytest.mark.parametrize("name", ["config1", "config3"])
def test_standins_match_reference(lfr_lib, name):
    ma = synthetic.config1_standin() if name == "config1" else synthetic.config3_standin()
    g, p, b = _setup(ma)
    gp = _ubar(g.n_nodes)
    info = b.component_info()
    n, st, _ = _check_against_reference(ma, g, p, b, gp, info["component"].tolist())
    assert n >= 0.95 * len(info["component"])
    assert st["n_differentiated"] + st["n_not_usable"] + st["n_indefinite"] == len(info["component"])


def test_config5_workgroup_classes_match_reference(lfr_lib):
    ma = synthetic.config5()
    g, p, b = _setup(ma)
    gp = _ubar(g.n_nodes, 1)
    info = b.component_info()
    rows = 2 * info["n_var_nodes"]
    rng = np.random.default_rng(5)
    which = rng.choice(info["component"], size=min(300, len(rows)), replace=False).tolist()
    which += info["component"][np.argsort(rows)[-5:]].tolist()
    n, st, _ = _check_against_reference(ma, g, p, b, gp, which)
    assert n >= 250 and rows.max() > 88
    print("config 5: %d components, %d indefinite, %d coordinates at a bound, backward %.3f ms"
          % (len(rows), st["n_indefinite"], st["n_bound_coordinates"], st["kernel_ms"]))


def test_cap_sized_sparse_matches_reference(lfr_lib):
    ma = synthetic.capsized_sparse(n_tracks=2500, seed=7)
    g, p, b = _setup(ma)
    gp = _ubar(g.n_nodes, 2)
    info = b.component_info()
    rows = 2 * info["n_var_nodes"]
    big = info["component"][rows > 192]
    assert len(big) >= 3 and rows.max() >= 2000
    n, st, _ = _check_against_reference(ma, g, p, b, gp, big.tolist())      # (indefinite ones: zero on both sides)
    status = b.backward_status()[rows > 192]
    print("cap-sized: %d components above 192 rows, %d differentiated, %d indefinite; backward %.3f ms"
          % (len(big), (status == capi.BACKWARD_OK).sum(), (status == capi.BACKWARD_INDEFINITE).sum(), st["kernel_ms"]))
    assert n >= 1 and n == (status == capi.BACKWARD_OK).sum()


def test_config4_sample_matches_reference(lfr_lib):
    ma = synthetic.config4()
    g, p, b = _setup(ma, device_assembly=True)
    gp = _ubar(g.n_nodes, 3)
    info = b.component_info()
    which = np.random.default_rng(4).choice(info["component"], size=1200, replace=False).tolist()
    n, st, _ = _check_against_reference(ma, g, p, b, gp, which)
    assert n >= 1000
    assert st["n_indefinite"] == 0 and st["n_not_usable"] == 0


@pytest.fixture(scope="module")
def small():
    ma = synthetic.generate(seed=11, n_images=48, n_tracks=400, eps_out=0.01)
    return ma


def test_f32_is_f64_rounded_and_calls_repeat(lfr_lib, small):
    g, p, b = _setup(small)
    gp = _ubar(g.n_nodes)
    a = [t.cpu().numpy() for t in b.backward(gp, f64=True)]
    c = [t.cpu().numpy() for t in b.backward(gp, f64=True)]
    f = [t.cpu().numpy() for t in b.backward(gp)]
    for x, y, z in zip(a, c, f):
        assert (x == y).all()                               # bitwise repeatable
        assert z.dtype == np.float32 and (z == x.astype(np.float32)).all()


def test_zeros_where_the_contract_says_zero(lfr_lib, small):
    g, p, b = _setup(small)
    track, root, comp = p.labels()
    ni, nf = _nodes(g, small)
    x = b.download()
    g1, g2, gs = [t.cpu().numpy() for t in b.backward(_ubar(g.n_nodes), f64=True)]
    comps = BR.graph_components(small, track, root, comp, ni, nf)
    kept = np.zeros(2 * len(small.sim), bool)
    for _, (_, cp) in comps.items():
        kept[cp.eids] = True
    m = np.arange(len(small.sim))
    assert not g2[~kept[2 * m]].any() and not g1[~kept[2 * m + 1]].any()        # dropped / cross-component edges
    assert not gs[~(kept[2 * m] | kept[2 * m + 1])].any()
    # the gradient only flows through free coordinates: a dL/dx on roots and bound coordinates changes nothing
    gp = torch.zeros((g.n_nodes, 2), dtype=torch.float64, device=DEV)
    fixed = torch.as_tensor(root[:, None] | (np.abs(x) >= 1.0), device=DEV)
    gp[fixed] = 1.0
    assert root.any()
    assert not any(t.any() for t in b.backward(gp, f64=True))


def test_zero_similarity_and_failed_component(lfr_lib, small):
    g0, p0, b0 = _setup(small)
    gp = _ubar(g0.n_nodes, 7)
    ref1, ref2, refs = [t.cpu().numpy() for t in b0.backward(gp, f64=True)]
    live = np.nonzero(np.abs(ref2).sum(1) > 0)[0]
    # a non-finite flow fails its component (LFR_TERM_FAILURE): zero gradient there, every other component bitwise unchanged
    ma = copy.deepcopy(small)
    ma.disp2[int(live[40]), 4, 0] = np.inf
    g, p, b = _setup(ma)
    g1, g2, gs = [t.cpu().numpy() for t in b.backward(gp, f64=True)]
    info = b.component_info()
    failed = info["termination"] == capi.TERM_FAILURE
    assert failed.sum() == 1 and (b.backward_status()[failed] == capi.BACKWARD_NOT_USABLE).all()
    ni, nf = _nodes(g, ma)
    e = BR.graph_components(ma, *p.labels(), ni, nf)[int(info["component"][failed][0])][1].eids
    assert not g1[e >> 1].any() and not g2[e >> 1].any() and not gs[e >> 1].any()
    other = np.ones(len(ma.sim), bool)
    other[e >> 1] = False
    assert (g1[other] == ref1[other]).all() and (g2[other] == ref2[other]).all() and (gs[other] == refs[other]).all()
    # similarity 0: the edge leaves the cost - no flow gradient, but a similarity gradient
    ma = copy.deepcopy(small)
    m0 = int(live[5])
    ma.sim[m0] = 0.0
    g, p, b = _setup(ma)
    g1, g2, gs = [t.cpu().numpy() for t in b.backward(_ubar(g.n_nodes, 7), f64=True)]
    assert not g1[m0].any() and not g2[m0].any() and gs[m0] != 0.0


def test_device_and_host_assembly_agree_and_shards_sum(lfr_lib, small):
    g, p, b = _setup(small)
    gp = _ubar(g.n_nodes, 9)
    ref = [t.cpu().numpy() for t in b.backward(gp, f64=True)]
    _, _, bd = _setup(small, device_assembly=True)
    got = [t.cpu().numpy() for t in bd.backward(gp, f64=True)]
    for x, y in zip(ref, got):
        assert (x == y).all()
    for world in (2, 4):
        acc = [np.zeros_like(x) for x in ref]
        for r in range(world):
            bs = capi.Batch(p, 0, r, world)
            bs.solve()
            for a, t in zip(acc, bs.backward(gp, f64=True)):
                a += t.cpu().numpy()
        for x, y in zip(ref, acc):
            assert np.abs(x - y).max() == 0.0, world


def test_backward_leaves_the_solve_alone(lfr_lib, small):
    g, p, b = _setup(small, device_assembly=True)
    x1 = b.download().copy()
    b.backward(_ubar(g.n_nodes))
    b.solve()
    assert (b.download() == x1).all()
    with pytest.raises(capi.LfrError):
        b2 = capi.Batch(p, 0)
        b2.backward(_ubar(g.n_nodes))


def test_refine_autograd(lfr_lib):
    from lfr_amd.autograd import refine
    ma = synthetic.config3_standin()
    d1 = torch.as_tensor(np.asarray(ma.disp1, np.float32).reshape(-1, 18), device=DEV).requires_grad_(True)
    d2 = torch.as_tensor(np.asarray(ma.disp2, np.float32).reshape(-1, 18), device=DEV).requires_grad_(True)
    sim = torch.as_tensor(np.asarray(ma.sim, np.float32), device=DEV).requires_grad_(True)
    pos, ni, nf = refine(d1, d2, sim, image_names=ma.image_names, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2,
                         pair_off=ma.pair_off, feat1=ma.feat1, feat2=ma.feat2, image_facts=ma.facts)
    g, p, b = _setup(ma)
    assert (pos.detach().cpu().numpy() == b.download()).all()
    w = _ubar(g.n_nodes, 11)
    (pos * w).sum().backward()
    n, _, (r1, r2, rs) = _check_against_reference(ma, g, p, b, w, b.component_info()["component"].tolist())
    assert n > 100
    for t, r in ((d1.grad, r1), (d2.grad, r2), (sim.grad, rs)):
        assert (t.cpu().numpy() == r.astype(np.float32)).all()
