"""Per-keypoint covariance of the refined positions (lfr_batch_covariance, include/lfr.h) on the GPU: the packed classes' in-register
inversion through lfr_debug_invert_spd against the longdouble inverse, and the whole call against the CPU reference of
tests/covariance_ref.py at the GPU's own positions x^.

Bounds (constants from the error analysis, not from the GPU's output): the probe is held entry-wise to
max(16 |inv_numpy - inv_ld|, 4 n u kappa_inf(A) |inv_ld|); end to end a component gets that plus 2 kappa_2(A) 1e-12 max|C_ref| for
the difference between the device-assembled and the oracle-assembled A.  The longdouble inverse comes from
linsolve_ref.solve_ld on identity columns up to 48 rows (every packed class); above, an elimination in longdouble per column is out of
reach, and the columns come from longdouble iterative refinement (covariance_ref.inverse_refined, pinned to solve_ld's inverse by
tests/test_covariance_ref.py): all columns up to 400 rows, above that a sample of 48 nodes (first, last and 46 drawn) with both
maxima of the bound taken over those columns only, which does not widen it.  Every node of every component is still checked for
status, zeros and positivity."""
import copy
import dataclasses

import numpy as np
import pytest
import torch

import backward_ref as BR
import covariance_ref as CR
import linsolve_ref as LS
from lfr_amd import capi, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KINDS = ("normal", "disconnected", "graded2", "graded6", "graded12", "cond1e4", "cond1e10", "identity", "diagonal")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. unit probe
# ---------------------------------------------------------------------------------------------------------------------------
def _matrix(rng, n, kind):
    if kind == "normal":
        return LS.normal_matrix(rng, n)
    if kind == "disconnected":
        return LS.normal_matrix(rng, n, disconnected=True)
    if kind.startswith("graded"):
        return LS.graded(rng, n, 10.0 ** int(kind[6:]))
    if kind.startswith("cond"):
        return LS.spd_with_cond(rng, n, float(kind[4:]))
    if kind == "identity":
        return np.eye(n)
    return np.diag(10.0 ** rng.uniform(-3, 3, n))


def _invert(solver, slots):
    """slots: a matrix or None (an empty group) per system, in wave order -> (list of inverse or None, status)."""
    n_rows = np.array([0 if s is None else s.shape[0] for s in slots], np.int32)
    A = np.concatenate([np.zeros(0)] + [LS.to_tri(s) for s in slots if s is not None])
    C, status = capi.invert_spd_hip(solver, n_rows, A)
    out, k = [], 0
    for n in n_rows:
        t = n * (n + 1) // 2
        out.append(C[k:k + t] if n else None)
        k += t
    return out, status


def _place(systems, G, neighbour=None):
    slots, pos = [], []
    for i, s in enumerate(systems):
        w = [None] * G
        w[i % G] = s
        if neighbour is not None:
            w[(i + 1) % G] = neighbour
        pos.append(len(slots) + i % G)
        slots += w
    return slots, pos


@pytest.fixture(scope="module")
def probe(lfr_lib):
    res = {}
    for si, solver in enumerate(LS.PACKED):
        rng = np.random.default_rng(5100 + si)
        G, lim = LS.GROUPS[solver], capi.SOLVER_MAX_ROWS[solver]
        systems = [(n, kind, _matrix(rng, n, kind)) for n in range(2, lim + 1, 2) for kind in KINDS]
        slots, pos = _place([s for _, _, s in systems], G)
        c, st = _invert(solver, slots)
        r = dict(systems=systems, alone=[c[p] for p in pos], alone_status=[int(st[p]) for p in pos], beside=None)
        if G > 1:
            slots, pos = _place([s for _, _, s in systems], G, _matrix(rng, lim, "normal"))
            c, st = _invert(solver, slots)
            r.update(beside=[c[p] for p in pos], beside_status=[int(st[p]) for p in pos])
        res[solver] = r
    return res


@pytest.mark.parametrize("solver", LS.PACKED)
def test_probe_inverse_error(probe, solver):
    r = probe[solver]
    assert r["alone_status"] == [0] * len(r["systems"])
    worst = 0.0
    for (n, kind, A), c in zip(r["systems"], r["alone"]):
        ref = CR.inverse_ld(A)
        got = np.tril(LS.from_tri(c, n))                     # row i as lane i holds it
        err = float(np.max(np.abs(got.astype(LS.LD) - np.tril(ref))))
        bound = CR.inverse_bound(A, ref)
        worst = max(worst, err / bound)
        assert err <= bound, "%s n=%d %s: error %.3e > bound %.3e" % (solver, n, kind, err, bound)
    print("%s: worst error / bound = %.4f over %d matrices" % (solver, worst, len(r["systems"])))


@pytest.mark.parametrize("solver", LS.PACKED)
def test_probe_covers_every_instantiation(probe, solver):
    got = {CR.cov_cl(solver, n) for n, _, _ in probe[solver]["systems"]}
    want = {"g8": {2, 4, 6, 8}, "g16": {10, 12, 14, 16}, "g64_2": {18, 20, 22, 24}, "g64_4": {20, 26, 28, 30, 32}}[solver]
    assert got == want


@pytest.mark.parametrize("solver", [s for s in LS.PACKED if LS.GROUPS[s] > 1])
def test_probe_independent_of_neighbours(probe, solver):
    r = probe[solver]
    assert r["beside_status"] == [0] * len(r["systems"])
    for (n, kind, _), a, b in zip(r["systems"], r["alone"], r["beside"]):
        assert np.array_equal(a, b), "%s n=%d %s" % (solver, n, kind)


@pytest.mark.parametrize("solver", LS.PACKED)
def test_probe_reports_non_positive_pivots(lfr_lib, solver):
    rng = np.random.default_rng(5200 + LS.PACKED.index(solver))
    G, lim = LS.GROUPS[solver], capi.SOLVER_MAX_ROWS[solver]
    good = [LS.normal_matrix(rng, n) for n in range(2, lim + 1, 2)]
    base, st = _invert(solver, good + [None] * (-len(good) % G))
    assert not st.any()
    for zero in (False, True):
        for at in (0, -1):
            slots = list(good) + [None] * (-len(good) % G)
            bad_at = list(range(0, len(good), max(G, 2)))   # one bad system per wave (every other wave where G == 1)
            for i in bad_at:
                n = good[i].shape[0]
                slots[i] = LS.not_pd(rng, n, at % n, zero=zero)
            c, st = _invert(solver, slots)
            for i in range(len(good)):
                if i in bad_at:
                    assert st[i] == capi.COVARIANCE_SINGULAR and not c[i].any()
                else:
                    assert st[i] == 0 and np.array_equal(c[i], base[i])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. end to end against the oracle's matrix
# ---------------------------------------------------------------------------------------------------------------------------
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


def _cov64(b):
    c, st = b.covariance(f64=True, want_stats=True)
    torch.cuda.synchronize()
    return c.cpu().numpy(), st


def _check_against_reference(ma, g, p, b, which, variant="ceres1"):
    cov, st = _cov64(b)
    x = b.download()
    track, root, comp = p.labels()
    ni, nf = _nodes(g, ma)
    info = b.component_info()
    status = dict(zip(info["component"].tolist(), b.covariance_status().tolist()))
    term = dict(zip(info["component"].tolist(), info["termination"].tolist()))
    comps = BR.graph_components(ma, track, root, comp, ni, nf, variant, which=set(which))
    rng = np.random.default_rng(17)
    n_compared, worst = 0, 0.0
    for c in which:
        var_nodes, cp = comps[c]
        got = cov[var_nodes]
        if term[c] == capi.TERM_FAILURE:
            assert status[c] == capi.COVARIANCE_NOT_USABLE and not got.any()
            continue
        A = CR.normal_matrix(CR.problem_of(cp), x[var_nodes].reshape(-1))
        if not CR.is_positive_definite(A):
            assert status[c] == capi.COVARIANCE_SINGULAR and not got.any(), "component %d" % c
            continue
        assert status[c] == capi.COVARIANCE_OK, "component %d" % c
        assert (got[:, 0] > 0).all() and (got[:, 2] > 0).all() and (got[:, 0] * got[:, 2] - got[:, 1] ** 2 >= 0).all()
        n = A.shape[0]
        if n <= 48:                                            # every packed class: solve_ld on identity columns
            sel, cols = np.arange(n // 2), None
            inv = CR.inverse_ld(A)
            blocks = CR.node_blocks(inv, range(n))
        elif n <= 400:                                         # all columns by longdouble iterative refinement
            sel, cols = np.arange(n // 2), None
            inv = CR.inverse_refined(A, range(n))
            blocks = CR.node_blocks(inv, range(n))
        else:
            sel = np.unique(np.concatenate([[0, n // 2 - 1], rng.choice(n // 2, 46, replace=False)]))
            cols = np.stack([2 * sel, 2 * sel + 1], 1).reshape(-1).tolist()
            inv = CR.inverse_refined(A, cols)
            blocks = CR.node_blocks(inv, cols)
        err = float(np.max(np.abs(got[sel].astype(LS.LD) - blocks)))
        bound = CR.component_bound(A, inv, cols)
        worst = max(worst, err / bound)
        assert err <= bound, "component %d (%d rows): error %.3e > bound %.3e" % (c, n, err, bound)
        n_compared += 1
    return n_compared, st, worst


def _all_nodes_accounted(p, b, cov):
    """roots and nodes outside computed components are 0; the status counts add up"""
    track, root, comp = p.labels()
    assert not cov[root].any()
    info = b.component_info()
    ok = info["component"][b.covariance_status() == capi.COVARIANCE_OK]
    outside = ~np.isin(comp, ok)
    assert not cov[outside].any()
    assert (cov[~outside & ~root][:, [0, 2]] > 0).all()


SMALL = dict(seed=11, n_images=48, n_tracks=400, eps_out=0.01)


@pytest.mark.parametrize("name", ["config1", "config3", "small"])
def test_all_components_match_reference(lfr_lib, name):
    ma = {"config1": synthetic.config1_standin, "config3": synthetic.config3_standin,
          "small": lambda: synthetic.generate(**SMALL)}[name]()
    g, p, b = _setup(ma)
    comps = b.component_info()["component"].tolist()
    n, st, worst = _check_against_reference(ma, g, p, b, comps)
    print("%s: %d of %d components compared, worst error / bound %.4f, %s" % (name, n, len(comps), worst, st))
    assert n >= 0.95 * len(comps)
    assert st["n_computed"] + st["n_not_usable"] + st["n_singular"] == len(comps)
    _all_nodes_accounted(p, b, _cov64(b)[0])


def test_config4_sample_matches_reference(lfr_lib):
    ma = synthetic.config4()
    g, p, b = _setup(ma, device_assembly=True)
    info = b.component_info()
    which = np.random.default_rng(4).choice(info["component"], size=1200, replace=False).tolist()
    n, st, worst = _check_against_reference(ma, g, p, b, which)
    print("config 4: %d of 1200 compared, worst error / bound %.4f, %s" % (n, worst, st))
    assert n >= 0.95 * 1200
    assert st["n_computed"] + st["n_not_usable"] + st["n_singular"] == len(info["component"])


def test_config5_sample_matches_reference(lfr_lib):
    ma = synthetic.config5()
    g, p, b = _setup(ma)
    info = b.component_info()
    rows = 2 * info["n_var_nodes"]
    which = np.random.default_rng(5).choice(info["component"], size=min(300, len(rows)), replace=False).tolist()
    which += [c for c in info["component"][np.argsort(rows)[-5:]].tolist() if c not in which]
    n, st, worst = _check_against_reference(ma, g, p, b, which)
    print("config 5: %d of %d compared, largest %d rows, worst error / bound %.4f, %s" % (n, len(which), rows.max(), worst, st))
    assert n >= 0.95 * len(which) and rows.max() > 88
    assert st["n_computed"] + st["n_not_usable"] + st["n_singular"] == len(rows)


def test_cap_sized_sparse_matches_reference(lfr_lib):
    ma = synthetic.capsized_sparse(n_tracks=2500, seed=7)
    g, p, b = _setup(ma)
    info = b.component_info()
    rows = 2 * info["n_var_nodes"]
    big = info["component"][rows > 192].tolist()
    assert len(big) >= 3 and rows.max() >= 2000
    n, st, worst = _check_against_reference(ma, g, p, b, big)
    print("cap-sized: %d of %d components above 192 rows compared, worst error / bound %.4f, %s" % (n, len(big), worst, st))
    assert n >= 0.95 * len(big)
    assert st["n_computed"] + st["n_not_usable"] + st["n_singular"] == len(rows)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. analytic case
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.25, 0.7, 1.0, 3.0])
def test_two_node_analytic(lfr_lib, w):
    """One root, one variable node, one match with zero flows: A = 2 w I, C = I / (2 w) to 4 ulp."""
    ma = synthetic.MatchArrays(image_names=["a", "b"], facts=np.ones(2, np.float32), pair_img1=np.array([0], np.int32),
                               pair_img2=np.array([1], np.int32), pair_off=np.array([0, 1], np.int64), feat1=np.array([0], np.uint32),
                               feat2=np.array([0], np.uint32), sim=np.array([w], np.float32), disp1=np.zeros((1, 9, 2), np.float32),
                               disp2=np.zeros((1, 9, 2), np.float32))
    g, p, b = _setup(ma)
    cov, st = _cov64(b)
    _, root, _ = p.labels()
    assert root.sum() == 1 and st["n_computed"] == 1
    want = 1.0 / (2.0 * float(np.float32(w)))
    assert not cov[root].any()
    c = cov[~root][0]
    assert c[1] == 0.0 and abs(c[0] - want) <= 4 * np.spacing(want) and abs(c[2] - want) <= 4 * np.spacing(want), (c, want)


# ---------------------------------------------------------------------------------------------------------------------------
# 4.-8. the interface's promises
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return synthetic.generate(**SMALL)


def test_f32_rounds_f64_calls_repeat_assemblies_agree_shards_sum(lfr_lib, small):
    g, p, b = _setup(small)
    a = b.covariance(f64=True).cpu().numpy()
    assert (b.covariance(f64=True).cpu().numpy() == a).all()
    f = b.covariance().cpu().numpy()
    assert f.dtype == np.float32 and (f == a.astype(np.float32)).all()
    _, pd, bd = _setup(small, device_assembly=True)
    assert (bd.covariance(f64=True).cpu().numpy() == a).all()
    _all_nodes_accounted(p, b, a)
    for world in (2, 4):
        acc = np.zeros_like(a)
        for r in range(world):
            bs = capi.Batch(p, 0, r, world)
            bs.solve()
            acc += bs.covariance(f64=True).cpu().numpy()
        assert (acc == a).all(), world


def test_failed_and_singular_components(lfr_lib, small):
    g0, p0, b0 = _setup(small)
    ref = b0.covariance(f64=True).cpu().numpy()
    ni, nf = _nodes(g0, small)
    track, root, comp = p0.labels()
    comps = BR.graph_components(small, track, root, comp, ni, nf)
    # a non-finite flow fails its component: zeros there, status not usable, every other node bitwise unchanged
    c_bad = sorted(comps)[40]
    ma = copy.deepcopy(small)
    e = int(comps[c_bad][1].eids[0])
    (ma.disp1 if e & 1 else ma.disp2)[e >> 1, 4, 0] = np.inf
    g, p, b = _setup(ma)
    cov, st = _cov64(b)
    info = b.component_info()
    failed = info["termination"] == capi.TERM_FAILURE
    assert failed.sum() == 1 and st["n_not_usable"] == 1 and (b.covariance_status()[failed] == capi.COVARIANCE_NOT_USABLE).all()
    nodes = p.labels()[2] == info["component"][failed][0]
    assert not cov[nodes].any() and (cov[~nodes] == ref[~nodes]).all()
    # similarity 0 on the only match of a leaf node: that component singular, the rest bitwise unchanged
    deg = np.zeros(g0.n_nodes, int)
    leaf = None
    for c in sorted(comps):
        var_nodes, cp = comps[c]
        d = np.bincount(np.concatenate([cp.src[cp.src >= 0], cp.dst[cp.dst >= 0]]), minlength=cp.nv)
        if len(var_nodes) >= 2 and (d == 2).any():             # one match = two directed edges
            l = int(np.nonzero(d == 2)[0][0])
            leaf = (c, int(cp.eids[(cp.src == l) | (cp.dst == l)][0]) >> 1)
            break
    assert leaf is not None
    ma = copy.deepcopy(small)
    ma.sim[leaf[1]] = 0.0
    g, p, b = _setup(ma)
    cov, st = _cov64(b)
    assert (p.labels()[2] == comp).all()                       # (the weight does not move the component structure here)
    info = b.component_info()
    sing = b.covariance_status() == capi.COVARIANCE_SINGULAR
    assert st["n_singular"] == 1 and info["component"][sing].tolist() == [leaf[0]]
    nodes = comp == leaf[0]
    assert not cov[nodes].any() and (cov[~nodes] == ref[~nodes]).all()


def test_covariance_leaves_solve_and_backward_alone(lfr_lib, small):
    g, p, b = _setup(small, device_assembly=True)
    with pytest.raises(capi.LfrError):
        capi.Batch(p, 0).covariance()
    gp = torch.as_tensor(np.random.default_rng(0).standard_normal((g.n_nodes, 2)), device=DEV)
    x1 = b.download().copy()
    before = [t.cpu().numpy() for t in b.backward(gp, f64=True)]
    b.covariance(f64=True)
    assert (b.download() == x1).all()
    after = [t.cpu().numpy() for t in b.backward(gp, f64=True)]
    for u, v in zip(before, after):
        assert (u == v).all()
    b.covariance()
    b.solve()
    assert (b.download() == x1).all()


def test_refine_returns_the_covariance(lfr_lib):
    from lfr_amd.autograd import refine
    ma = synthetic.config3_standin()
    d1 = torch.as_tensor(np.asarray(ma.disp1, np.float32).reshape(-1, 18), device=DEV).requires_grad_(True)
    d2 = torch.as_tensor(np.asarray(ma.disp2, np.float32).reshape(-1, 18), device=DEV)
    sim = torch.as_tensor(np.asarray(ma.sim, np.float32), device=DEV)
    kw = dict(image_names=ma.image_names, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off, feat1=ma.feat1,
              feat2=ma.feat2, image_facts=ma.facts)
    assert len(refine(d1, d2, sim, **kw)) == 3
    pos, ni, nf, cov = refine(d1, d2, sim, return_covariance=True, **kw)
    g, p, b = _setup(ma, device_assembly=True)
    assert cov.dtype == torch.float64 and not cov.requires_grad and tuple(cov.shape) == (g.n_nodes, 3)
    assert (cov.cpu().numpy() == b.covariance(f64=True).cpu().numpy()).all()
    pos.sum().backward()
    assert d1.grad is not None


def test_keypoint_covariances_on_a_solve(lfr_lib, small):
    g, p, b = _setup(small)
    cov = b.covariance(f64=True).cpu().numpy()
    ni, nf = g.nodes()
    facts = g.image_facts()
    nfeat = int(nf.max()) + 2
    for im, name in list(enumerate(g.image_names()))[:6]:
        out = g.keypoint_covariances(cov, name, nfeat)
        assert (out == CR.keypoint_covariances(cov, ni, nf, im, facts[im], nfeat)).all() and out.any()


# ---------------------------------------------------------------------------------------------------------------------------
# 9. covariance and backward share one batch: independent of each other, of their order and of lfr_batch_set_inputs in between
# ---------------------------------------------------------------------------------------------------------------------------
# the "allclasses" graph of tests/test_gpu_set_inputs.py: tracks of 2..97 nodes, so every packed class and every LDS class holds components
ALLCLASSES = dict(seed=20, n_images=100, n_tracks=80, len_dist="uniform", len_lo=2, len_hi=97, eps_out=0.0)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("kind", ["host", "fused"])
def test_passes_crossed_on_one_batch_equal_each_alone(lfr_lib, kind):
    """solve, covariance, backward, set_inputs, solve, backward, covariance on ONE batch; each of the four pass results must equal, bit
    for bit, the same pass run alone on a fresh batch built from the same inputs (host-assembled, and device-assembled with the fused gather)."""
    ma = synthetic.generate(**ALLCLASSES)
    rng = np.random.default_rng(106)
    lo, hi = min(ma.disp1.min(), ma.disp2.min()), max(ma.disp1.max(), ma.disp2.max())
    d1, d2 = (np.clip(d + rng.normal(0.0, 0.02, size=d.shape).astype(np.float32), lo, hi).astype(np.float32) for d in (ma.disp1, ma.disp2))
    mb = dataclasses.replace(ma, disp1=d1, disp2=d2)
    alive = []

    def fresh(m):
        g = capi.Graph.from_arrays(m)
        p = capi.Problem(g, device_graph_stage=0) if kind == "fused" else capi.Problem(g)
        b = capi.Batch(p, 0)
        b.solve()
        alive.append((g, p, b))
        return g, b

    def cov(b):
        return [b.covariance(f64=True).cpu().numpy(), b.covariance_status()]

    def bwd(b):
        return [t.cpu().numpy() for t in b.backward(gp, f64=True)] + [b.backward_status()]

    def same(got, want, what):
        for k, (x, y) in enumerate(zip(got[:-1], want[:-1])):
            assert np.array_equal(_bits(x), _bits(y)), "%s/%s: result %d differs, max %.3g" % (kind, what, k, np.abs(x - y).max())
        assert any(np.any(y != 0) for y in want[:-1]), what
        assert np.array_equal(got[-1], want[-1]), "%s/%s: status" % (kind, what)

    g, b = fresh(ma)
    gp = torch.as_tensor(np.random.default_rng(8).standard_normal((g.n_nodes, 2)), device=DEV)
    rows = 2 * b.component_info()["n_var_nodes"]
    assert (rows <= 32).any() and ((rows > 32) & (rows <= 88)).any() and ((rows > 88) & (rows <= 130)).any() and (rows > 130).any()
    want = {}
    for tag, m in (("first", ma), ("second", mb)):             # every pass alone on a batch of its own
        (_, bc), (_, bb) = fresh(m), fresh(m)
        want[tag] = (bc.download().copy(), cov(bc), bwd(bb))
        assert np.array_equal(_bits(bb.download()), _bits(want[tag][0]))
    assert not np.array_equal(want["first"][0], want["second"][0])

    assert np.array_equal(_bits(b.download()), _bits(want["first"][0]))
    same(cov(b), want["first"][1], "covariance, first solve")
    same(bwd(b), want["first"][2], "backward after covariance, first solve")
    b.set_inputs(torch.as_tensor(d1.reshape(-1, 18)).to(DEV), torch.as_tensor(d2.reshape(-1, 18)).to(DEV))
    for call in (lambda: b.backward(gp, f64=True), lambda: b.covariance(f64=True)):
        with pytest.raises(capi.LfrError) as e:
            call()
        assert e.value.code == -1                              # LFR_ERR_ARG
    b.solve()
    assert np.array_equal(_bits(b.download()), _bits(want["second"][0]))
    same(bwd(b), want["second"][2], "backward, second solve")
    same(cov(b), want["second"][1], "covariance after backward, second solve")
    assert b.spin_timeouts() == 0
