"""lfr_graph_from_device_arrays (csrc/lfr_graphbuild.hip): the match graph numbered on the GPU from device arrays is the graph
lfr_graph_from_arrays_device_flows builds on the host from the same values - nodes, images, labels from both graph stages, positions,
the solution file, the backward after set_inputs - bit for bit; it is resident after the call, survives an eviction, and refine()
takes the device road when feat1 / feat2 / sim are device tensors."""
import ctypes

import numpy as np
import pytest
import torch

import numbering_ref as R
from lfr_amd import capi, synthetic
from lfr_amd.synthetic import MatchArrays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LFR_ERR_ARG = -1


class DeviceCase:
    """The per-match arrays of a case as device tensors (kept alive here), and the two graphs built from them."""

    def __init__(self, case, sim=None, disp1=None, disp2=None, facts=None):
        M = len(case["feat1"])
        rng = np.random.Generator(np.random.PCG64(M + 17))
        names = case["image_names"]
        self.banned = tuple(case.get("banned", ()))
        sim = rng.uniform(0.8, 1.0, M).astype(np.float32) if sim is None else np.ascontiguousarray(sim, np.float32)
        disp1 = rng.normal(0, 0.05, (M, 18)).astype(np.float32) if disp1 is None else np.ascontiguousarray(disp1, np.float32).reshape(M, 18)
        disp2 = rng.normal(0, 0.05, (M, 18)).astype(np.float32) if disp2 is None else np.ascontiguousarray(disp2, np.float32).reshape(M, 18)
        facts = (1.0 + 0.25 * np.arange(len(names))).astype(np.float32) if facts is None else np.ascontiguousarray(facts, np.float32)
        self.ma = MatchArrays(image_names=list(names), facts=facts, pair_img1=case["pair_img1"], pair_img2=case["pair_img2"],
                              pair_off=case["pair_off"], feat1=np.ascontiguousarray(case["feat1"], np.uint32),
                              feat2=np.ascontiguousarray(case["feat2"], np.uint32), sim=sim, disp1=disp1, disp2=disp2)
        # (one spare element: an empty tensor has no address, and these stand for arrays the producer owns)
        pad = lambda a: np.concatenate([a.reshape(-1), np.zeros(1, a.dtype)])
        self.f1 = torch.from_numpy(pad(self.ma.feat1).view(np.int32)).to(DEV)
        self.f2 = torch.from_numpy(pad(self.ma.feat2).view(np.int32)).to(DEV)
        self.sim = torch.from_numpy(pad(sim)).to(DEV)
        self.d1 = torch.from_numpy(pad(disp1)).to(DEV)
        self.d2 = torch.from_numpy(pad(disp2)).to(DEV)
        torch.cuda.synchronize()

    def host_numbered(self, banned=None):
        return capi.Graph.from_device_flows(self.ma, self.d1.data_ptr(), self.d2.data_ptr(), 0, self.banned if banned is None else banned)

    def device_numbered(self, banned=None):
        host_only = MatchArrays(image_names=self.ma.image_names, facts=self.ma.facts, pair_img1=self.ma.pair_img1, pair_img2=self.ma.pair_img2,
                                pair_off=self.ma.pair_off, feat1=None, feat2=None, sim=None, disp1=None, disp2=None)
        return capi.Graph.from_device_arrays(host_only, self.f1.data_ptr(), self.f2.data_ptr(), self.sim.data_ptr(), self.d1.data_ptr(),
                                             self.d2.data_ptr(), 0, self.banned if banned is None else banned)


def same_graph(want, got, labels=True):
    assert got.n_nodes == want.n_nodes and got.n_edges == want.n_edges and got.n_images == want.n_images
    assert got.image_names() == want.image_names() and got.image_facts() == want.image_facts()
    for a, b in zip(got.nodes(), want.nodes()):
        assert (a == b).all()
    if labels and want.n_nodes:
        # the endpoints: on the device (device graph stage) and in the host mirror (host graph stage)
        for kw in (dict(device_graph_stage=0), dict(device_assembly=True)):
            lw, lg = capi.Problem(want, **kw).labels(), capi.Problem(got, **kw).labels()
            for a, b in zip(lg, lw):
                assert (a == b).all(), kw


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_hand_made_order_cases(lfr_lib, name):
    case = R.HAND_CASES[name]
    c = DeviceCase(case)
    want, got = c.host_numbered(), c.device_numbered()
    same_graph(want, got)
    seen, n1, n2, node_image, node_feat, rows = R.expected_graph(case)      # and both are what the rule says
    assert got.image_names() == seen and got.n_edges == 2 * len(rows)
    gi, gf = got.nodes()
    assert (gi == node_image).all() and (gf == node_feat).all()


@pytest.mark.parametrize("n_matches", [255, 256, 257, 4097])
def test_tile_boundaries_with_long_runs(lfr_lib, n_matches):
    for banned in ((), ("img001.png",)):
        c = DeviceCase(R.random_case(31 * n_matches, n_matches, banned=banned))
        same_graph(c.host_numbered(), c.device_numbered())


def test_run_that_crosses_workgroups(lfr_lib):
    c = DeviceCase(R.hub_case(1500))
    want, got = c.host_numbered(), c.device_numbered()
    same_graph(want, got)
    # (b, 5) and (c, 6), the hub (a, 0), and its 1500 partners (b, 0..1499) of which (b, 5) is there already
    assert got.n_nodes == 2 + 1 + 1499
    seen, n1, n2, node_image, node_feat, rows = R.expected_graph(R.hub_case(1500))
    assert np.bincount(np.concatenate([n1, n2])).max() == 1501 and len(node_image) == got.n_nodes


def test_large_input_path_of_the_sort(lfr_lib):
    """140 000 matches = 280 000 entries: above the 256 K entries from which the sort takes its one-sweep driver."""
    ma = synthetic.generate(seed=8, n_images=64, n_tracks=10000, eps_out=0.001)
    M = 140000
    assert ma.n_matches > M
    P = int(np.searchsorted(ma.pair_off, M, "left"))           # the first P pairs, the last one cut at M
    off = np.concatenate([ma.pair_off[:P], [M]]).astype(np.int64)
    case = dict(image_names=ma.image_names, pair_img1=ma.pair_img1[:P], pair_img2=ma.pair_img2[:P], pair_off=off, feat1=ma.feat1[:M], feat2=ma.feat2[:M])
    c = DeviceCase(case, sim=ma.sim[:M], disp1=ma.disp1[:M], disp2=ma.disp2[:M], facts=ma.facts)
    want, got = c.host_numbered(), c.device_numbered()
    assert got.n_edges == 2 * M
    same_graph(want, got)


# ---- downstream identity ----
@pytest.fixture(scope="module")
def scene():
    ma = synthetic.generate(seed=41, n_images=24, n_tracks=300, eps_out=0.003)
    case = dict(image_names=ma.image_names, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off, feat1=ma.feat1, feat2=ma.feat2)
    return ma, DeviceCase(case, sim=ma.sim, disp1=ma.disp1, disp2=ma.disp2, facts=ma.facts)


def _solve(g, tmp_path, tag, new_inputs):
    p = capi.Problem(g, device_graph_stage=0)
    b = capi.Batch(p, 0)
    b.solve()
    pos = b.download().copy()
    path = str(tmp_path / ("solution_%s.pb" % tag))
    n_out = g.write_solution(pos, path)
    b.set_inputs(*new_inputs)                            # (the record -> edge map comes from the graph's host arrays)
    b.solve()
    pos2 = b.download().copy()
    w = torch.as_tensor(np.random.Generator(np.random.PCG64(3)).normal(size=(g.n_nodes, 2)), device=DEV)
    grads = [t.cpu().numpy() for t in b.backward(w)]
    return p.labels(), pos, (n_out, open(path, "rb").read()), pos2, grads


@pytest.mark.parametrize("with_ban", [False, True])
def test_downstream_results_are_identical(lfr_lib, scene, tmp_path, with_ban):
    ma, c = scene
    banned = (ma.image_names[3],) if with_ban else ()
    want, got = c.host_numbered(banned), c.device_numbered(banned)
    same_graph(want, got)                                # (labels of lfr_problem_build_hip and lfr_problem_build_labels included)
    m = got.n_edges // 2
    assert (m < ma.n_matches) == with_ban and m > 1000
    rng = np.random.Generator(np.random.PCG64(9))
    new_inputs = [torch.as_tensor(rng.normal(0, 0.05, (m, 18)).astype(np.float32), device=DEV) for _ in range(2)]
    new_inputs.append(torch.as_tensor(rng.uniform(0.8, 1.0, m).astype(np.float32), device=DEV))
    rw, rg = _solve(want, tmp_path, "host", new_inputs), _solve(got, tmp_path, "device", new_inputs)
    for a, b in zip(rg[0], rw[0]):
        assert (a == b).all()
    assert (rg[1] == rw[1]).all() and np.abs(rg[1]).max() > 0
    assert rg[2] == rw[2] and len(rg[2][1]) > 0          # write_solution: same count, same bytes
    assert (rg[3] == rw[3]).all() and not (rg[3] == rg[1]).all()
    for a, b in zip(rg[4], rw[4]):
        assert (a == b).all()
    assert any(np.abs(a).max() > 0 for a in rg[4])


def test_wide_similarity_range_takes_the_host_stage(lfr_lib, scene):
    """Similarities that span more than 2^10: the device graph stage hands back to the host stage (sims_sum_exactly, computed by
    finish() from the mirrored similarities)."""
    ma, _ = scene
    sim = np.asarray(ma.sim, np.float32).copy()
    sim[::7] *= np.float32(2.0 ** -12)
    case = dict(image_names=ma.image_names, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off, feat1=ma.feat1, feat2=ma.feat2)
    c = DeviceCase(case, sim=sim, disp1=ma.disp1, disp2=ma.disp2, facts=ma.facts)
    same_graph(c.host_numbered(), c.device_numbered())


def test_resident_after_the_call_and_after_eviction(lfr_lib, scene):
    ma, c = scene
    want, _ = capi.Problem(c.host_numbered(), device_graph_stage=0).solve_hip(0)
    got = c.device_numbered()
    p = capi.Problem(got, device_graph_stage=0)
    b = capi.Batch(p, 0)
    b.solve()
    assert (b.download() == want).all()
    labels = p.labels()
    got.evict_device()                                   # the next use rebuilds the device copy from the host mirror
    p2 = capi.Problem(got, device_graph_stage=0)
    b2 = capi.Batch(p2, 0)
    b2.solve()
    assert (b2.download() == want).all()
    for a, b_ in zip(p2.labels(), labels):
        assert (a == b_).all()
    b.solve()                                            # (the first batch kept its own reference to the first copy)
    assert (b.download() == want).all()


# ---- refine() ----
@pytest.mark.parametrize("with_ban", [False, True])
def test_refine_with_device_tensors(lfr_lib, scene, with_ban):
    from lfr_amd.autograd import refine
    ma, c = scene
    banned = (ma.image_names[5],) if with_ban else ()
    meta = dict(image_names=ma.image_names, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off, image_facts=ma.facts, banned=banned)
    out = []
    for on_device in (False, True):
        d1 = torch.as_tensor(np.asarray(ma.disp1, np.float32).reshape(-1, 18), device=DEV).requires_grad_(True)
        d2 = torch.as_tensor(np.asarray(ma.disp2, np.float32).reshape(-1, 18), device=DEV).requires_grad_(True)
        sim = torch.as_tensor(np.asarray(ma.sim, np.float32), device=DEV).requires_grad_(True)
        if on_device:      # int64 indices, as a matcher's argmax gives them
            f1, f2 = (torch.as_tensor(np.asarray(f, np.int64), device=DEV) for f in (ma.feat1, ma.feat2))
        else:
            f1, f2 = ma.feat1, ma.feat2
        pos, ni, nf = refine(d1, d2, sim, feat1=f1, feat2=f2, **meta)
        w = torch.as_tensor(np.random.Generator(np.random.PCG64(12)).normal(size=tuple(pos.shape)), device=DEV)
        (pos * w).sum().backward()
        out.append([pos.detach().cpu().numpy(), ni, nf] + [t.grad.cpu().numpy() for t in (d1, d2, sim)])
    for a, b in zip(*out):
        assert a.shape == b.shape and (a == b).all()
    assert all(np.abs(a).max() > 0 for a in out[1][3:])
    with pytest.raises(ValueError):                      # the device arrays are checked against pair_off before the GPU reads them
        refine(d1, d2, sim, feat1=f1[:-1], feat2=f2, **meta)


# ---- errors ----
def test_bad_arguments_are_rejected_on_the_host(lfr_lib):
    c = DeviceCase(R.HAND_CASES["same_node_several_pairs"])
    ma = c.ma
    L = capi.lib()
    ptrs = [c.f1.data_ptr(), c.f2.data_ptr(), c.sim.data_ptr(), c.d1.data_ptr(), c.d2.data_ptr()]

    def call(p1=ma.pair_img1, ptrs=ptrs, device=0):
        h = ctypes.c_void_p(0xdead)
        facts, p1 = np.ascontiguousarray(ma.facts, np.float32), np.ascontiguousarray(p1, np.int32)
        rc = L.lfr_graph_from_device_arrays(len(ma.image_names), capi._cstrs(ma.image_names), capi._ptr(facts), len(p1), capi._ptr(p1),
                                            capi._ptr(ma.pair_img2), capi._ptr(ma.pair_off), *[ctypes.c_void_p(p) for p in ptrs], device,
                                            capi._cstrs([]), 0, ctypes.byref(h))
        return rc, h.value, L.lfr_last_error().decode()

    bad = ma.pair_img1.copy()
    bad[2] = len(ma.image_names)
    rc, h, msg = call(p1=bad)
    assert rc == LFR_ERR_ARG and not h and "image index out of range" in msg
    for k in range(5):
        rc, h, msg = call(ptrs=ptrs[:k] + [None] + ptrs[k + 1:])
        assert rc == LFR_ERR_ARG and not h and "NULL" in msg, k
    rc, h, msg = call(device=-1)
    assert rc == LFR_ERR_ARG and not h and msg
    rc, h, msg = call()
    assert rc == 0 and h
    L.lfr_graph_free(ctypes.c_void_p(h))
    with pytest.raises(capi.LfrError):
        capi.Problem(c.device_numbered())                # host assembly needs host flows, as for from_device_flows
    with pytest.raises(capi.LfrError):
        capi.Problem(c.host_numbered())
