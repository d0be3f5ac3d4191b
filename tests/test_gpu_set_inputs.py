"""lfr_batch_set_inputs (include/lfr.h): new flows and similarities into a live batch, and lfr_amd.autograd.Refiner on top of it.

The reference throughout is a FRESH batch built from the new values on the same assembly path: structure is a function of the matches
and the similarities alone, so the two batches hold the same records in the same order and the deterministic solve must agree bit for
bit.  The one exception is the project's own: a component above 192 rows that a team could not serve at its size (team_fallbacks) is
solved "to rounding" - those components, and only when a fallback happened, are compared at the position tolerance 6.25e-6."""
import dataclasses

import numpy as np
import pytest
import torch

from lfr_amd import capi, synthetic
from lfr_amd.autograd import Refiner, refine

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
POS_TOL = 6.25e-6                 # 1e-4 px, the project's position tolerance (tests/test_gpu_sparse.py)
SIGMA_NOISE = 0.02                # synthetic.generate's flow noise: the size of the perturbations here
KINDS = ["host", "fused", "device_flows", "shard", "device_shard"]


# ------------------------------------------------------------------------------------------------------------------ inputs
@pytest.fixture(scope="module")
def small():
    return synthetic.generate(seed=11, n_images=48, n_tracks=400, eps_out=0.01)


@pytest.fixture(scope="module")
def allclasses():
    """Tracks of 2..97 nodes, every pair inside a track matched, no wrong matches: a track of L nodes is a component of 2 (L - 1) rows
    and L (L - 1) records, which walks through every class that holds records (parameters picked on the CPU)."""
    return synthetic.generate(seed=20, n_images=100, n_tracks=80, len_dist="uniform", len_lo=2, len_hi=97, eps_out=0.0)


@pytest.fixture(scope="module")
def capsized():
    return synthetic.capsized_sparse(n_tracks=2500, seed=7)


def _flows18(x):
    return np.ascontiguousarray(x, np.float32).reshape(-1, 18)


def _perturbed(ma, seed, rows=None):
    """(disp1', disp2'): the flows plus seeded noise of the generator's own size, kept inside the generator's range; rows: only those."""
    rng = np.random.default_rng(seed)
    lo, hi = min(ma.disp1.min(), ma.disp2.min()), max(ma.disp1.max(), ma.disp2.max())
    out = []
    for d in (ma.disp1, ma.disp2):
        n = np.clip(d + rng.normal(0.0, SIGMA_NOISE, size=d.shape).astype(np.float32), lo, hi).astype(np.float32)
        if rows is not None:
            keep = np.ones(len(d), bool)
            keep[rows] = False
            n[keep] = d[keep]
        assert np.isfinite(n).all()
        out.append(n)
    return out


def _dev(x, flows=True):
    a = _flows18(x) if flows else np.ascontiguousarray(x, np.float32)
    return torch.as_tensor(a).to(DEV)


def _build(ma, kind):
    """(graph, problem, batch, keep-alive) of one of the batch kinds, unsolved"""
    keep = None
    if kind == "device_flows":
        keep = (_dev(ma.disp1), _dev(ma.disp2))
        torch.cuda.synchronize()
        g = capi.Graph.from_device_flows(ma, keep[0].data_ptr(), keep[1].data_ptr(), device=0)
    else:
        g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g) if kind in ("host", "shard") else capi.Problem(g, device_graph_stage=0)     # (device_shard: assembled on the GPU)
    b = capi.Batch(p, 0, 1, 2) if kind in ("shard", "device_shard") else capi.Batch(p, 0)     # shard 1 of 2
    return g, p, b, keep


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _assert_same_solve(a, b, p, what=""):
    """positions, iterations, termination and final cost of the two batches' latest solves: bitwise"""
    xa, xb = a.download(), b.download()
    ia, ib = a.component_info(), b.component_info()
    for k in ("component", "n_var_nodes", "n_edges"):
        assert np.array_equal(ia[k], ib[k]), "%s: the two batches differ in structure (%s)" % (what, k)
    loose = np.zeros(len(ia["component"]), bool)
    if a.team_fallbacks() or b.team_fallbacks():          # (see the module docstring)
        loose = 2 * ia["n_var_nodes"] > 192
    if loose.any():
        nodes = np.isin(p.labels()[2], ia["component"][loose])
        d = np.abs(xa[nodes] - xb[nodes]).max()
        print("%s: team fallbacks: %d components above 192 rows compared at %.3g, max difference %.3g" % (what, loose.sum(), POS_TOL, d))
        assert d <= POS_TOL, what
        xa = xa.copy()
        xa[nodes] = xb[nodes]
    tight = ~loose
    assert np.array_equal(_bits(xa), _bits(xb)), "%s: positions differ, max %.3g" % (what, np.abs(xa - xb).max())
    assert np.array_equal(ia["iterations"][tight], ib["iterations"][tight]), what
    assert np.array_equal(ia["termination"][tight], ib["termination"][tight]), what
    assert np.array_equal(_bits(ia["final_cost"][tight]), _bits(ib["final_cost"][tight])), what


# class limits of lfr_internal.hpp (KernelClass, kBlockRowsS / kBlockRowsM / kBlockMaxRows) and classify() of lfr_graph.cpp
def _kernel_class(rows, edges):
    for name, r, e in (("G8", 8, 24), ("G16", 16, 96), ("G64_2", 24, 192), ("G64_4", 32, 320)):
        if rows <= r and edges <= e:
            return name
    for name, r in (("BLOCK", 88), ("BLOCK_M", 130), ("BLOCK_L", 192)):
        if rows <= r:
            return name
    return "GLOBAL"


def _classes(info):
    return {_kernel_class(int(2 * v), int(e)) for v, e in zip(info["n_var_nodes"], info["n_edges"])}


# ------------------------------------------------------------------------------------- 1. equals a fresh build, bit for bit
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("graph", ["small", "allclasses", "capsized"])
def test_equals_fresh_build(lfr_lib, request, graph, kind):
    ma = request.getfixturevalue(graph)
    d1, d2 = _perturbed(ma, 101)
    t1, t2 = _dev(d1), _dev(d2)
    gb, pb, b, keep_b = _build(dataclasses.replace(ma, disp1=d1, disp2=d2), kind)
    b.solve()
    info = b.component_info()
    if graph == "capsized":
        # components above 192 rows exist only as pieces of the size cap's cut; the cut reads matches and similarities, never the flows,
        # so the two batches still share one structure (_assert_same_solve checks it component by component)
        assert (2 * info["n_var_nodes"] > 192).sum() >= 3
    else:
        assert pb.stats()["n_cut_components"] == 0
    if graph == "allclasses" and "shard" not in kind:
        assert _classes(info) == {"G8", "G16", "G64_2", "G64_4", "BLOCK", "BLOCK_M", "BLOCK_L"}
    # set_inputs before the first solve, after one solve and after two (a fused batch writes its packed records in the first case
    # from set_inputs itself with nothing solved, in the second from set_inputs, in the third from its second solve)
    for n_before in ((0, 1, 2) if kind == "fused" else (1,)):
        ga, pa, a, keep_a = _build(ma, kind)
        for _ in range(n_before):
            a.solve(want_stats=False)
        a.set_inputs(t1, t2)
        a.solve()
        _assert_same_solve(a, b, pb, "%s/%s after %d solve(s)" % (graph, kind, n_before))
        assert a.spin_timeouts() == 0
        a.close()
    if graph == "small":
        # flow arrays that start 4 bytes into a float buffer: a 72-byte row is then not 8-byte aligned and the kernel's scalar loads run
        views = []
        for t in (t1, t2):
            buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
            v = buf[1:].view(t.shape)
            v.copy_(t)
            assert v.is_contiguous() and v.data_ptr() % 8 == 4
            views.append(v)
        ga, pa, a, keep_a = _build(ma, kind)
        a.solve(want_stats=False)
        a.set_inputs(*views)
        a.solve()
        _assert_same_solve(a, b, pb, "%s/%s misaligned flows" % (graph, kind))
        ts = _dev(ma.sim, flows=False)
        a.set_inputs(_dev(ma.disp1), _dev(ma.disp2))
        a.set_inputs(views[0], views[1], ts)              # (the full form's scalar variant)
        a.solve()
        _assert_same_solve(a, b, pb, "%s/%s misaligned flows with sim" % (graph, kind))
        a.close()


# --------------------------------------------------------------------------------------------------------- 2. similarities
@pytest.mark.parametrize("kind", ["host", "fused", "device_flows"])
def test_similarities_and_partial_forms(lfr_lib, small, kind):
    ma = small
    half = (0.5 * ma.sim).astype(np.float32)               # exact: order, ties and the graph stage's sums scale with it
    d1, d2 = _perturbed(ma, 102)
    t1, t2, ts = _dev(d1), _dev(d2), _dev(half, flows=False)
    # sim alone against a fresh build from 0.5 * sim
    g0, p0, ref, k0 = _build(dataclasses.replace(ma, sim=half), kind)
    assert p0.stats()["n_cut_components"] == 0
    ref.solve()
    ga, pa, a, ka = _build(ma, kind)
    a.solve(want_stats=False)
    a.set_inputs(sim=ts)
    a.solve()
    _assert_same_solve(a, ref, p0, "sim only/" + kind)
    # flows-only then sim-only == both at once == a fresh build from both
    g1, p1, both, k1 = _build(dataclasses.replace(ma, sim=half, disp1=d1, disp2=d2), kind)
    both.solve()
    a.set_inputs(t1, t2)               # (the similarities are 0.5 * sim already: this form must leave them alone)
    a.solve()
    _assert_same_solve(a, both, p1, "flows only after sim only/" + kind)
    gc, pc, c, kc = _build(ma, kind)
    c.set_inputs(t1, t2, ts)
    c.solve()
    _assert_same_solve(c, both, p1, "combined/" + kind)
    gd, pd, d, kd = _build(ma, kind)
    d.solve(want_stats=False)
    d.set_inputs(sim=ts)
    d.set_inputs(disp1=t1, disp2=t2)
    d.solve()
    _assert_same_solve(d, both, p1, "sim only then flows only/" + kind)


# ---------------------------------------------------------------------------------------------- 3. round trip and isolation
def _match_nodes(g, ma):
    """graph node of either end of every match"""
    ni, nf = g.nodes()
    idx = {n: i for i, n in enumerate(ma.image_names)}
    img_of = np.array([idx[n] for n in g.image_names()], np.int64)
    key = img_of[ni] * (1 << 32) + nf.astype(np.int64)
    order = np.argsort(key)
    per_pair = np.diff(ma.pair_off)
    k1 = np.repeat(ma.pair_img1.astype(np.int64), per_pair) * (1 << 32) + ma.feat1.astype(np.int64)
    k2 = np.repeat(ma.pair_img2.astype(np.int64), per_pair) * (1 << 32) + ma.feat2.astype(np.int64)
    return order[np.searchsorted(key[order], k1)], order[np.searchsorted(key[order], k2)]


@pytest.mark.parametrize("kind", ["host", "fused"])
def test_round_trip_and_isolation(lfr_lib, small, kind):
    ma = small
    g, p, b, keep = _build(ma, kind)
    b.solve()
    x0 = b.download().copy()
    o1, o2 = _dev(ma.disp1), _dev(ma.disp2)
    d1, d2 = _perturbed(ma, 103)
    b.set_inputs(_dev(d1), _dev(d2))
    b.solve()
    x1 = b.download().copy()
    assert not np.array_equal(x0, x1)
    b.set_inputs(o1, o2)
    b.solve()
    assert np.array_equal(_bits(b.download()), _bits(x0))

    # one component of the 8-row class that is neither first nor last of its wavefront (8 components per wave, in batch order)
    info = b.component_info()
    cls = np.array([_kernel_class(int(2 * v), int(e)) for v, e in zip(info["n_var_nodes"], info["n_edges"])])
    g8 = np.nonzero(cls == "G8")[0]
    # component_info is in batch order and the 8-row class opens the batch (KC_G8 = 0), contiguous; the packed kernel deals its class's
    # components to waves eight at a time from the class's first one, so rows 0..7 share a wavefront.  Asserted, so that a change of
    # that layout shows here instead of silently losing the "same wavefront" case (all other components are compared anyway).
    assert len(g8) >= 16 and g8[0] == 0 and np.array_equal(g8, np.arange(len(g8)))
    victim = int(info["component"][3])
    comp = p.labels()[2]
    n1, n2 = _match_nodes(g, ma)
    rows = np.nonzero((comp[n1] == victim) & (comp[n2] == victim))[0]
    assert len(rows) >= 1
    e1, e2 = _perturbed(ma, 104, rows=rows)
    b.set_inputs(_dev(e1), _dev(e2))
    b.solve()
    x2 = b.download()
    inside = comp == victim
    assert np.array_equal(_bits(x2[~inside]), _bits(x0[~inside]))
    assert not np.array_equal(x2[inside], x0[inside])


# ------------------------------------------------------------------------------------------ 4. consumers see the new records
@pytest.mark.parametrize("first", ["backward_first", "set_inputs_first"])
@pytest.mark.parametrize("graph,kind", [("small", "host"), ("small", "device_flows"), ("small", "fused"), ("allclasses", "host"),
                                        ("small", "shard")])
def test_backward_and_covariance_see_new_records(lfr_lib, request, graph, kind, first):
    ma = request.getfixturevalue(graph)
    d1, d2 = _perturbed(ma, 105)
    gb, pb, b, kb = _build(dataclasses.replace(ma, disp1=d1, disp2=d2), kind)
    b.solve()
    gp = torch.as_tensor(np.random.default_rng(7).standard_normal((gb.n_nodes, 2)), device=DEV)
    want = [t.cpu().numpy() for t in b.backward(gp, f64=True)] + [b.covariance(f64=True).cpu().numpy()]
    ga, pa, a, ka = _build(ma, kind)
    a.solve()
    if first == "backward_first":      # the record -> edge map comes from the backward ...
        a.backward(gp, f64=True)
        a.covariance(f64=True)
    a.set_inputs(_dev(d1), _dev(d2))   # ... or from set_inputs
    a.solve()
    _assert_same_solve(a, b, pb, "%s/%s" % (graph, kind))
    got = [t.cpu().numpy() for t in a.backward(gp, f64=True)] + [a.covariance(f64=True).cpu().numpy()]
    assert np.array_equal(a.backward_status(), b.backward_status())
    assert np.array_equal(a.covariance_status(), b.covariance_status())
    for name, x, y in zip(("grad_disp1", "grad_disp2", "grad_sim", "covariance"), got, want):
        assert np.array_equal(_bits(x), _bits(y)), name
    assert any(np.any(w != 0) for w in want[:3]) and np.any(want[3] != 0)


# ----------------------------------------------------------------------------------------------- 5. epoch rule and arguments
def test_epoch_rule_and_arguments(lfr_lib, small):
    ma = small
    g, p, b, keep = _build(ma, "host")
    t1, t2, ts = _dev(ma.disp1), _dev(ma.disp2), _dev(ma.sim, flows=False)
    gp = torch.zeros((g.n_nodes, 2), dtype=torch.float64, device=DEV)
    b.solve()
    b.backward(gp)
    b.covariance()
    b.set_inputs(t1, t2, ts)
    x = b.download()                                       # positions keep their meaning between set_inputs and the next solve
    for call in (lambda: b.backward(gp), lambda: b.covariance()):
        with pytest.raises(capi.LfrError) as e:
            call()
        assert e.value.code == -1                          # LFR_ERR_ARG
        assert "inputs changed since the latest solve" in str(e.value)
    b.solve()
    assert np.array_equal(_bits(b.download()), _bits(x))   # (the same values went in)
    b.backward(gp)
    b.covariance()
    # refused on the host, before any launch
    with pytest.raises(capi.LfrError) as e:
        b.set_inputs()
    assert e.value.code == -1
    for kw in ({"disp1": t1}, {"disp2": t2}, {"disp1": t1, "sim": ts}):
        with pytest.raises(capi.LfrError) as e:
            b.set_inputs(**kw)
        assert e.value.code == -1
    assert capi.lib().lfr_batch_set_inputs(None, None, None, None, None) == -1
    b.backward(gp)                                         # a refused call changes nothing: the epoch still matches
    m = ma.n_matches
    bad = [dict(disp1=t1.double(), disp2=t2), dict(disp1=t1, disp2=t2.half()), dict(sim=ts.double()),
           dict(disp1=t1.cpu(), disp2=t2), dict(sim=ts.cpu()), dict(disp1=t1[:-1], disp2=t2[:-1]), dict(sim=ts[:-1]),
           dict(disp1=t1.reshape(m, 2, 9), disp2=t2), dict(disp1=t1.t().contiguous().t(), disp2=t2), dict(sim=ma.sim)]
    for kw in bad:
        with pytest.raises(ValueError):
            b.set_inputs(**kw)
    b.set_inputs(t1.reshape(m, 9, 2), t2.reshape(m, 9, 2))       # the producer's own shape
    b.solve()
    assert np.array_equal(_bits(b.download()), _bits(x))

    # a batch over one rank's connected components numbers its matches by itself: refused
    mc = synthetic.generate(seed=32, n_images=48, n_tracks=3000, eps_out=0.002)      # (many connected components: dealt out by component)
    g2 = capi.Graph.from_arrays(mc)
    p2 = capi.Problem(g2, device_graph_stage=0, shard=(0, 2))
    assert p2.cc_sharded
    b2 = capi.Batch(p2, 0)
    with pytest.raises(capi.LfrError) as e:
        b2.set_inputs(_dev(mc.disp1), _dev(mc.disp2))
    assert e.value.code == -5                              # LFR_ERR_UNSUPPORTED

    # a batch that needs the record -> edge map from the graph, and the graph is gone: refused by set_inputs and by the backward
    L = capi.lib()
    g3, p3, b3, _ = _build(ma, "host")
    b3.solve()
    out = [torch.zeros((m, 18), device=DEV), torch.zeros((m, 18), device=DEV), torch.zeros((m,), device=DEV)]
    g3.close()
    assert L.lfr_batch_set_inputs(b3._h, t1.data_ptr(), t2.data_ptr(), None, None) == -1
    assert "graph has been freed" in L.lfr_last_error().decode()
    assert L.lfr_batch_backward(b3._h, gp.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), 0, None, None) == -1
    assert "graph has been freed" in L.lfr_last_error().decode()
    b3.close()
    p3.close()


# ------------------------------------------------------------------------------------------------------------- 6. Refiner
def _meta(ma):
    return dict(image_names=ma.image_names, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off, feat1=ma.feat1,
                feat2=ma.feat2, image_facts=ma.facts)


def _leaf(x, flows=True):
    return _dev(x, flows).requires_grad_(True)


@pytest.mark.parametrize("banned", [(), ("000005.png",)])
def test_refiner_matches_refine(lfr_lib, small, banned):
    ma = small
    sim = _dev(ma.sim, flows=False)
    r = Refiner(_dev(ma.disp1), _dev(ma.disp2), sim, banned=banned, **_meta(ma))
    w = None
    for step in range(3):
        d1, d2 = (ma.disp1, ma.disp2) if step == 0 else _perturbed(ma, 200 + step)
        a = [_leaf(d1), _leaf(d2), _leaf(ma.sim, flows=False)]
        c = [_leaf(d1), _leaf(d2), _leaf(ma.sim, flows=False)]
        pos = r(*a)
        ref, node_image, node_feature = refine(*c, banned=banned, **_meta(ma))
        if w is None:
            w = torch.as_tensor(np.random.default_rng(9).standard_normal(tuple(ref.shape)), device=DEV)
            assert np.array_equal(node_image, r.node_image) and np.array_equal(node_feature, r.node_feature) and r.n_nodes == ref.shape[0]
        (pos * w).sum().backward()
        (ref * w).sum().backward()
        assert np.array_equal(_bits(pos.detach().cpu().numpy()), _bits(ref.detach().cpu().numpy())), "step %d" % step
        for x, y, name in zip(a, c, ("disp1", "disp2", "sim")):
            gx, gy = x.grad.cpu().numpy(), y.grad.cpu().numpy()
            assert np.array_equal(gx.view(np.uint32), gy.view(np.uint32)), "step %d: %s.grad" % (step, name)
            assert np.any(gy != 0)
    cov = r.covariance(f64=True)
    assert cov.shape == (r.n_nodes, 3) and bool((cov != 0).any())
    r.close()


def test_refiner_stale_backward_and_stream_order(lfr_lib, small):
    ma = small
    flows = [(ma.disp1, ma.disp2)] + [_perturbed(ma, 300 + k) for k in range(2)]
    sim = _dev(ma.sim, flows=False)
    want = [refine(_dev(f[0]), _dev(f[1]), sim, **_meta(ma))[0].cpu().numpy() for f in flows]
    r = Refiner(_dev(ma.disp1), _dev(ma.disp2), sim, **_meta(ma))
    # the caller's buffers are overwritten in stream order right behind every forward, and nothing synchronises in between
    src = [(_dev(f[0]), _dev(f[1])) for f in flows]
    buf1, buf2 = torch.empty_like(src[0][0]), torch.empty_like(src[0][1])
    torch.cuda.synchronize()
    got = []
    for s1, s2 in src:
        buf1.copy_(s1)
        buf2.copy_(s2)
        got.append(r(buf1, buf2))
        buf1.fill_(float("nan"))
        buf2.fill_(float("nan"))
    for k, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y)), "forward %d" % k
    # the batch holds only its latest solve
    a1 = [_leaf(flows[1][0]), _leaf(flows[1][1])]
    a2 = [_leaf(flows[2][0]), _leaf(flows[2][1])]
    p1 = r(*a1)
    p2 = r(*a2)
    with pytest.raises(RuntimeError, match="stale"):
        p1.sum().backward()
    assert a1[0].grad is None
    p2.sum().backward(retain_graph=True)
    g_first = a2[0].grad.clone()
    p2.sum().backward()                                    # a second backward of the latest forward is fine
    assert torch.equal(a2[0].grad, 2 * g_first) and bool((g_first != 0).any())
    r.close()
