"""lfr_batch_covariance_matches (include/lfr.h) on the GPU: the cross block C_12 and D = Cov(x_node2 - x_node1) per match against the
longdouble reference of tests/match_covariance_ref.py at the GPU's own positions x^, and the call's contract - node output, root ends,
internal consistency, sentinels, failed and singular components, repeatability, assemblies, shards, arguments, Refiner.

Bounds (constants from the error analysis of tests/test_gpu_covariance.py, not from the GPU's output): every entry of a compared
component's cross blocks is held to covariance_ref.component_bound - the inversion's entry-wise bound plus the parity of the
device-assembled A - and every entry of D, a sum of four such entries, to 4 x that bound.  Above 400 rows the columns of 48 sampled
nodes (first, last and the ends of drawn matches) stand for the component, with both maxima of the bound over those columns only,
which does not widen it.  Internal consistency: D is two sums and one difference of fp64 numbers, so it agrees with the longdouble
combination of the call's own `cov` and `cross` to 4 ulp of the largest term."""
import copy

import numpy as np
import pytest
import torch

import backward_ref as BR
import class_limit_cases as CL
import covariance_ref as CR
import match_covariance_ref as MR
import test_gpu_class_limits as TCL
from test_gpu_set_inputs import _dev, _meta
from lfr_amd import capi, synthetic
from lfr_amd.autograd import Refiner, _kept_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = ("cov", "cross", "relative")
SMALL = dict(seed=11, n_images=48, n_tracks=400, eps_out=0.01)
MARK = np.array(MR.NOT_IN_PROGRAM)
_cache = {}


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _cm(b, **kw):
    out = b.covariance_matches(**kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _same(x, y, what="", keys=KEYS):
    for k in keys:
        assert x[k].dtype == y[k].dtype and np.array_equal(_raw(x[k]), _raw(y[k])), (what, k)


def _setup(ma, variant="ceres1", device_assembly=False, shard=(0, 1)):
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g, device_graph_stage=0) if device_assembly else capi.Problem(g)
    b = capi.Batch(p, 0, shard[0], shard[1], tukey_variant=variant)
    b.solve()
    return g, p, b


def _nodes(g, ma):
    ni, nf = g.nodes()
    idx = {n: i for i, n in enumerate(ma.image_names)}
    return np.array([idx[n] for n in g.image_names()], np.int32)[ni], nf


def _graph_components(ma, g, p, which=None, variant="ceres1"):
    track, root, comp = p.labels()
    ni, nf = _nodes(g, ma)
    return BR.graph_components(ma, track, root, comp, ni, nf, variant, which=None if which is None else set(which))


def _in_program(comps, n_matches):
    """bool[n_matches]: the match's direction node1 -> node2 is a residual block of one of `comps`"""
    out = np.zeros(n_matches, bool)
    for _, cp in comps.values():
        out[[m for m, _, _ in MR.program_matches(cp)]] = True
    return out


def _check_against_reference(ma, g, p, b, which, out=None, variant="ceres1"):
    """cross and relative of the components `which` against the longdouble reference at the batch's x^ -> (components compared,
    matches compared, worst error / bound)"""
    out = _cm(b, want_stats=True) if out is None else out
    x = b.download()
    info = b.component_info()
    status = dict(zip(info["component"].tolist(), b.covariance_status().tolist()))
    term = dict(zip(info["component"].tolist(), info["termination"].tolist()))
    comps = _graph_components(ma, g, p, which, variant)
    rng = np.random.default_rng(17)
    n_comp = n_match = 0
    worst = 0.0
    for c in which:
        var_nodes, cp = comps[c]
        ms = [m for m, _, _ in MR.program_matches(cp)]
        A = None if term[c] == capi.TERM_FAILURE else CR.normal_matrix(CR.problem_of(cp), x[var_nodes].reshape(-1))
        if A is None or not CR.is_positive_definite(A):
            assert status[c] == (capi.COVARIANCE_NOT_USABLE if A is None else capi.COVARIANCE_SINGULAR), "component %d" % c
            assert not out["cov"][var_nodes].any() and not out["cross"][ms].any() and not out["relative"][ms].any(), "component %d" % c
            continue
        assert status[c] == capi.COVARIANCE_OK, "component %d" % c
        n = A.shape[0]
        inv, cols = MR.inverse_columns(A, None if n <= 400 else MR.sample_nodes(cp, rng))
        ref = MR.match_reference(cp, inv, cols)
        assert len(ref) == len(ms) if n <= 400 else len(ref) >= 8, "component %d" % c
        bound = CR.component_bound(A, inv, cols)
        for m, (cross, rel) in ref.items():
            e_cross = float(np.max(np.abs(out["cross"][m].astype(CR.LD) - cross)))
            e_rel = float(np.max(np.abs(out["relative"][m].astype(CR.LD) - rel)))
            worst = max(worst, e_cross / bound, e_rel / (4 * bound))
            assert e_cross <= bound, "component %d (%d rows), match %d: cross off by %.3e > bound %.3e" % (c, n, m, e_cross, bound)
            assert e_rel <= 4 * bound, "component %d (%d rows), match %d: relative off by %.3e > 4 x bound %.3e" % (c, n, m, e_rel, bound)
            assert MR.is_psd(out["relative"][m], 4 * bound), (c, m)
        n_comp += 1
        n_match += len(ref)
    return n_comp, n_match, worst


# ---------------------------------------------------------------------------------------------------------- 1., 2. known answers
def _ulps(got, want):
    return np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.maximum(np.abs(want), 2.0 ** -1000))


def test_triangle(lfr_lib):
    ma = MR.triangle()
    g, p, b = _setup(ma)
    out = _cm(b, want_stats=True)
    _, root, _ = p.labels()
    ni, _ = _nodes(g, ma)
    assert root.tolist() == (ni == 0).tolist() and out["stats"]["n_computed"] == 1
    assert not out["cov"][root].any()
    for k in np.nonzero(~root)[0]:
        assert out["cov"][k, 1] == 0.0 and (_ulps(out["cov"][k, [0, 2]], 0.375) <= 4).all()
    for m, (cross_d, rel_d) in MR.TRIANGLE_WANT.items():
        cross, rel = out["cross"][m], out["relative"][m]
        assert cross[0, 1] == 0.0 and cross[1, 0] == 0.0 and rel[1] == 0.0, m
        if cross_d == 0.0:
            assert not cross.any(), m
        else:
            assert (_ulps(np.diag(cross), cross_d) <= 4).all(), (m, cross)
        assert (_ulps(rel[[0, 2]], rel_d) <= 4).all(), (m, rel)


@pytest.mark.parametrize("w", [0.25, 0.7, 1.0, 3.0])
def test_two_node_analytic(lfr_lib, w):
    """One root, one variable node, one match with zero flows: A = 2 w I, so relative = C = I / (2 w) to 4 ulp and cross = 0."""
    ma = synthetic.MatchArrays(image_names=["a", "b"], facts=np.ones(2, np.float32), pair_img1=np.array([0], np.int32),
                               pair_img2=np.array([1], np.int32), pair_off=np.array([0, 1], np.int64), feat1=np.array([0], np.uint32),
                               feat2=np.array([0], np.uint32), sim=np.array([w], np.float32), disp1=np.zeros((1, 9, 2), np.float32),
                               disp2=np.zeros((1, 9, 2), np.float32))
    g, p, b = _setup(ma)
    out = _cm(b)
    want = 1.0 / (2.0 * float(np.float32(w)))
    rel = out["relative"][0]
    assert not out["cross"].any() and rel[1] == 0.0 and (_ulps(rel[[0, 2]], want) <= 4).all(), (rel, want)
    assert np.array_equal(_raw(rel), _raw(out["cov"][~p.labels()[1]][0]))


# ------------------------------------------------------------------------------------------ 3. every kernel class at its limits
def class_limit_outputs(device_assembly):
    key = ("cl", device_assembly)
    if key not in _cache:
        s = TCL.all_solved(device_assembly)
        _cache[key] = (s, _cm(s.b, want_stats=True))
    return _cache[key]


@pytest.mark.parametrize("device_assembly", [False, True], ids=["host", "device"])
def test_every_class_at_its_limits(lfr_lib, device_assembly):
    s, out = class_limit_outputs(device_assembly)
    which = s.info["component"].tolist()
    assert sorted(which) == sorted(s.comp.values()) and len(which) == len(CL.NAMES)
    n_comp, n_match, worst = _check_against_reference(s.ma, s.g, s.p, s.b, which, out)
    print("class limits/%s: %d of %d components, %d matches compared, worst error / bound %.4f, %s"
          % (device_assembly, n_comp, len(which), n_match, worst, out["stats"]))
    # every named shape is positive definite at x^ (tests/test_match_covariance_ref.py: at the oracle's positions), so all are compared
    assert n_comp == len(CL.NAMES) >= 0.95 * len(which) and out["stats"]["n_computed"] == len(which)
    if device_assembly:
        _same(out, class_limit_outputs(False)[1], "device against host assembly")


# ------------------------------------------------------------------------------------------------------ 4. workgroup classes
# capsized_sparse(seed=7): 21 tracks is the smallest count with a component above 192 rows (tests/test_match_covariance_ref.py), 23
# tracks give components of the two larger LDS classes, 60 tracks one above 400 rows, where the reference samples its columns
@pytest.mark.parametrize("n_tracks", [MR.CAPSIZED_SMALLEST, 23, 60])
def test_workgroup_classes(lfr_lib, n_tracks):
    ma = synthetic.capsized_sparse(n_tracks=n_tracks, seed=7)
    g, p, b = _setup(ma)
    info = b.component_info()
    rows = 2 * info["n_var_nodes"]
    assert rows.max() > {MR.CAPSIZED_SMALLEST: 192, 23: 130, 60: 400}[n_tracks]
    which = [int(info["component"][np.argmax(rows)])]
    for lo, hi in ((32, 88), (88, 130), (130, 192)):                    # one per LDS class, where the graph has one
        sel = np.nonzero((rows > lo) & (rows <= hi))[0]
        if len(sel):
            which.append(int(info["component"][sel[np.argmax(rows[sel])]]))
    n_comp, n_match, worst = _check_against_reference(ma, g, p, b, which)
    print("cap-sized, %d tracks: components of %s rows, %d matches compared, worst error / bound %.4f"
          % (n_tracks, [int(rows[info["component"] == c][0]) for c in which], n_match, worst))
    assert n_comp == len(which)


# ------------------------------------------------------------------------------ 5. node output; solve and backward stay as they are
def test_node_output_is_the_covariance_call_and_nothing_else_moves(lfr_lib):
    s, out = class_limit_outputs(False)
    b = s.b
    gp = torch.as_tensor(np.random.default_rng(0).standard_normal((s.g.n_nodes, 2)), device=DEV)
    x0 = b.download().copy()
    cov0 = b.covariance(f64=True).cpu().numpy()
    bwd0 = [t.cpu().numpy() for t in b.backward(gp, f64=True, gauss_newton=True)]
    again = _cm(b)
    _same(again, out, "second call")
    assert np.array_equal(_raw(again["cov"]), _raw(cov0)) and cov0.any()
    assert np.array_equal(_raw(b.covariance(f64=True).cpu().numpy()), _raw(cov0))
    assert np.array_equal(_raw(_cm(b, f64=False)["cov"]), _raw(b.covariance().cpu().numpy()))
    assert np.array_equal(_raw(b.download()), _raw(x0))
    for u, v in zip(bwd0, [t.cpu().numpy() for t in b.backward(gp, f64=True, gauss_newton=True)]):
        assert np.array_equal(_raw(u), _raw(v))
    only = _cm(b, want=("relative",))                                   # any subset of the outputs: the same bits
    assert sorted(only) == ["relative"] and np.array_equal(_raw(only["relative"]), _raw(out["relative"]))
    only = _cm(b, want=("cov",))
    assert np.array_equal(_raw(only["cov"]), _raw(cov0))


# -------------------------------------------------------------------------------------- 6., 7. root ends, internal consistency
def _ends(g, ma, p):
    """(node1, node2) per match of the graph, from the arrays"""
    ni, nf = _nodes(g, ma)
    key = ni.astype(np.int64) << 32 | nf.astype(np.int64)
    order = np.argsort(key)
    pi = np.repeat(np.arange(len(ma.pair_img1)), np.diff(ma.pair_off))
    k1 = ma.pair_img1[pi].astype(np.int64) << 32 | ma.feat1.astype(np.int64)
    k2 = ma.pair_img2[pi].astype(np.int64) << 32 | ma.feat2.astype(np.int64)
    return order[np.searchsorted(key[order], k1)], order[np.searchsorted(key[order], k2)]


@pytest.mark.parametrize("name", ["class limits", "small"])
def test_root_ends_and_internal_consistency(lfr_lib, name):
    if name == "small":
        ma = synthetic.generate(**SMALL)
        g, p, b = _setup(ma)
        out = _cm(b)
    else:
        s, out = class_limit_outputs(False)
        ma, g, p, b = s.ma, s.g, s.p, s.b
    n1, n2 = _ends(g, ma, p)
    _, root, _ = p.labels()
    inprog = ~(out["relative"] == MARK).all(1)
    ok = inprog & (out["relative"][:, 0] > 0)                            # (not a status 1 / 2 component)
    one = ok & (root[n1] != root[n2])
    both = ok & ~root[n1] & ~root[n2]
    assert one.sum() >= 30 and both.sum() >= 300 and not (inprog & root[n1] & root[n2]).any()
    other = np.where(root[n1], n2, n1)
    assert np.array_equal(_raw(out["relative"][one]), _raw(out["cov"][other[one]])) and not out["cross"][one].any()
    worst = 0.0
    for m in np.nonzero(both)[0]:
        want, largest = MR.relative_from_blocks(out["cov"][n1[m]], out["cov"][n2[m]], out["cross"][m])
        tol = 4 * np.spacing(largest)
        err = float(np.abs(out["relative"][m].astype(CR.LD) - want).max())
        worst = max(worst, err / tol)
        assert err <= tol, (m, err, tol)
        r = out["relative"][m]
        assert r[0] >= 0 and r[2] >= 0 and r[0] * r[2] - r[1] * r[1] >= -tol * max(r[0], r[2]), (m, r)
    print("%s: %d root matches, %d matches with two variable ends, worst |relative - blocks| %.3f of 4 ulp" % (name, one.sum(), both.sum(), worst))


# ---------------------------------------------------------------------------------------------------------------- 8. sentinels
def test_sentinels(lfr_lib):
    ma = synthetic.generate(**SMALL)
    g, p, b = _setup(ma)
    out = _cm(b)
    comps = _graph_components(ma, g, p)
    inprog = _in_program(comps, ma.n_matches)
    assert 1 <= (~inprog).sum() < ma.n_matches                           # (matches the program drops: wrong matches between two roots)
    marked = (out["relative"] == MARK).all(1)
    assert np.array_equal(marked, ~inprog) and not out["cross"][~inprog].any()
    assert (out["relative"][inprog][:, [0, 2]] > 0).all()
    w = b.evaluate(cost=False, grad=False, residuals=False)["weights"].cpu().numpy()
    assert marked.sum() == (w[:, 0] == -1).sum() and np.array_equal(marked, w[:, 0] == -1)


# ------------------------------------------------------------------------------------------------ 9. failures and isolation
def _cut_loose(ma, cp, labels):
    """`ma` with similarity 0 on every tie of one variable node of component cp: the first node without a tie to a constant node for
    which the host graph stage still gives `labels`"""
    at_const = set(cp.src[cp.dst < 0].tolist()) | set(cp.dst[cp.src < 0].tolist())
    for l in range(cp.nv):
        if l in at_const:
            continue
        mb = copy.deepcopy(ma)
        mb.sim[np.unique(cp.eids[(cp.src == l) | (cp.dst == l)] >> 1)] = 0.0
        if all(np.array_equal(u, v) for u, v in zip(capi.Problem(capi.Graph.from_arrays(mb)).labels(), labels)):
            return mb
    raise AssertionError("no node can be cut loose without moving the graph stage")


def test_failed_and_singular_components_and_their_wave_neighbours(lfr_lib):
    ma, feats = CL.all_twice()
    base = TCL.Solved(ma, feats[0])
    ref = _cm(base.b)
    comps = _graph_components(ma, base.g, base.p)
    comp = base.p.labels()[2]
    n1, n2 = _ends(base.g, ma, base.p)
    # one component FAILS (a non-finite flow); one of a workgroup class and one of a packed class are singular (similarity 0 on every
    # tie of one node - the shapes have no leaf - chosen so that tracks, roots and components stay: _cut_loose)
    c_bad, c_sing, c_sing2 = base.comp["k6"], base.comp["ring18"], base.comp["s11_first_reread"]
    e = int(comps[c_bad][1].eids[0])
    mb = copy.deepcopy(ma)
    (mb.disp1 if e & 1 else mb.disp2)[e >> 1, 4, 0] = np.inf
    for c in (c_sing, c_sing2):
        mb = _cut_loose(mb, comps[c][1], base.p.labels())
    s = TCL.Solved(mb, feats[0])
    assert (s.p.labels()[2] == comp).all()                              # (the weights do not move the component structure here)
    out = _cm(s.b, want_stats=True)
    status = dict(zip(s.info["component"].tolist(), s.b.covariance_status().tolist()))
    assert status[c_bad] == capi.COVARIANCE_NOT_USABLE and status[c_sing] == status[c_sing2] == capi.COVARIANCE_SINGULAR
    assert out["stats"]["n_not_usable"] == 1 and out["stats"]["n_singular"] == 2
    hit = np.isin(comp[n1], [c_bad, c_sing, c_sing2]) & (comp[n1] == comp[n2])
    inprog = ~(ref["relative"] == MARK).all(1)
    assert (inprog & hit).sum() >= 40
    assert not out["relative"][hit & inprog].any() and not out["cross"][hit].any() and not out["cov"][np.isin(comp, [c_bad, c_sing, c_sing2])].any()
    assert np.array_equal(_raw(out["relative"][~hit]), _raw(ref["relative"][~hit])) and np.array_equal(_raw(out["cross"][~hit]), _raw(ref["cross"][~hit]))
    keep = ~np.isin(comp, [c_bad, c_sing, c_sing2])
    assert np.array_equal(_raw(out["cov"][keep]), _raw(ref["cov"][keep]))


# ------------------------------------------------------------------------------------------ 10. repeatability and assemblies
def test_repeat_assemblies_f32_and_shards(lfr_lib):
    ma = synthetic.generate(**SMALL)
    g, p, b = _setup(ma)
    a = _cm(b)
    _same(_cm(b), a, "second call")
    f = _cm(b, f64=False)
    for k in KEYS:
        assert f[k].dtype == np.float32 and np.array_equal(_raw(f[k]), _raw(a[k].astype(np.float32))), k
    gd, pd, bd = _setup(ma, device_assembly=True)                       # device-assembled: the first call gathers (fused) ...
    _same(_cm(bd), a, "device-assembled, fused gather")
    bd.solve()                                                           # ... the second solve wrote the records
    _same(_cm(bd), a, "device-assembled, records")
    inprog = ~(a["relative"] == MARK).all(1)
    seen = np.zeros(ma.n_matches, bool)
    acc = {k: np.zeros_like(a[k]) for k in ("cov", "cross")}
    rel = np.tile(MARK, (ma.n_matches, 1))
    for r in range(2):
        bs = capi.Batch(p, 0, r, 2)
        bs.solve()
        o = _cm(bs)
        mine = ~(o["relative"] == MARK).all(1)
        assert not (seen & mine).any()
        seen |= mine
        rel[mine] = o["relative"][mine]
        for k in acc:
            acc[k] += o[k]
    assert np.array_equal(seen, inprog)
    assert np.array_equal(_raw(rel), _raw(a["relative"])) and all(np.array_equal(_raw(acc[k] + 0.0), _raw(a[k] + 0.0)) for k in acc)


# ---------------------------------------------------------------------------------------------------------------- 11. arguments
def test_arguments(lfr_lib):
    s, out = class_limit_outputs(False)
    L = capi.lib()
    rel = torch.zeros((s.g.n_edges // 2, 3), dtype=torch.float64, device=DEV)
    assert L.lfr_batch_covariance_matches(s.b._h, None, None, None, 1, None, None) == -1
    assert L.lfr_batch_covariance_matches(s.b._h, None, None, rel.data_ptr(), 2, None, None) == -1
    assert L.lfr_batch_covariance_matches(None, None, None, rel.data_ptr(), 1, None, None) == -1
    assert L.lfr_batch_covariance_matches(s.b._h, None, None, rel.data_ptr(), 1, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_raw(rel.cpu().numpy()), _raw(out["relative"]))
    with pytest.raises(ValueError):
        s.b.covariance_matches(want=())
    ma = synthetic.generate(seed=41, n_images=12, n_tracks=120)
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g)
    b = capi.Batch(p, 0)
    with pytest.raises(capi.LfrError) as e:                             # before the first solve
        b.covariance_matches()
    assert e.value.code == -1
    b.solve()
    b.covariance_matches()
    b.set_inputs(_dev(ma.disp1), _dev(ma.disp2))
    with pytest.raises(capi.LfrError) as e:                             # new inputs, no solve yet
        b.covariance_matches()
    assert e.value.code == -1
    b.solve()
    assert _cm(b)["relative"].any()
    # a batch over one rank's connected components numbers its matches by itself
    mc = synthetic.generate(seed=32, n_images=48, n_tracks=3000, eps_out=0.002)
    g2 = capi.Graph.from_arrays(mc)
    p2 = capi.Problem(g2, device_graph_stage=0, shard=(0, 2))
    assert p2.cc_sharded
    b2 = capi.Batch(p2, 0)
    b2.solve()
    for want in (KEYS, ("cross",), ("cov", "relative")):
        with pytest.raises(capi.LfrError) as e:
            b2.covariance_matches(want=want)
        assert e.value.code == -5
    o = _cm(b2, want=("cov",))
    assert o["cov"].any() and np.array_equal(_raw(o["cov"]), _raw(b2.covariance(f64=True).cpu().numpy()))


# ------------------------------------------------------------------------------------------------------------------ 12. Refiner
def test_refiner_match_covariance_scatters_to_the_callers_rows(lfr_lib):
    ma = synthetic.generate(seed=41, n_images=12, n_tracks=120)
    banned = ("000005.png",)
    r = Refiner(_dev(ma.disp1), _dev(ma.disp2), _dev(ma.sim, flows=False), banned=banned, **_meta(ma))
    with pytest.raises(RuntimeError):
        r.match_covariance()
    r(_dev(ma.disp1), _dev(ma.disp2))
    out = r.match_covariance()
    inner = r._batch.covariance_matches(want=("cross", "relative"))
    torch.cuda.synchronize()
    rows = _kept_rows(ma.pair_img1, ma.pair_img2, ma.pair_off, list(ma.image_names), banned)
    gone = np.ones(ma.n_matches, bool)
    gone[rows] = False
    assert gone.any() and out["cross"].shape == (ma.n_matches, 2, 2) and out["relative"].shape == (ma.n_matches, 3)
    assert not bool(out["cross"][gone].any()) and bool((out["relative"][gone] == torch.as_tensor(MARK, device=DEV)).all())
    for k in ("cross", "relative"):
        assert torch.equal(out[k][~torch.as_tensor(gone)], inner[k]) and not out[k].requires_grad and out[k].dtype == torch.float64
    assert bool((out["relative"][:, 0] > 0).any()) and r.match_covariance(f64=False)["relative"].dtype == torch.float32
    r.close()
