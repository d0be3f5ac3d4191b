"""lfr_batch_jvp in every launch class at its exact row and edge limits: the 33 shapes of tests/class_limit_cases.py (a last resident
slot that is full, the first re-read edge, rows that fit a class whose edges do not, the first and the last row count of every LDS
footprint, the two-root component, the smallest elimination-tree components, duplicated matches) against tests/jvp_ref.py with the
GPU's own positions, in every mode, Tukey variant and assembly; alone, among the others and in a batch that holds each twice; through
the adjoint identity with the backward per shape; with coordinates at the bound per class; at the 6144-row limit of the dense
factorization; and after lfr_batch_set_inputs.

What the random stand-ins of tests/test_gpu_jvp.py can miss is the jvp's own code: the record loop of jvp_gn_packed_kernel with its
two spare right-hand-side slots, the one wave of the exact mode that walks all records of a packed component, the owner-computes
right-hand side of the workgroup classes, the LDS carving by the largest component of the class that is in the batch.  A record
dropped, doubled or mis-addressed changes a component's right-hand side by the order of 1 / E of its norm (E <= 9506 edges), far
above the tolerance, so dense random tangents on all three inputs detect it.

Tolerances: against the reference the project's own for this pass, |got - ref|_2 <= 1e-8 |ref|_2 + 1e-14 per component
(test_gpu_jvp, test_gpu_backward); on the hard inputs with coordinates at the bound and at 6144 rows the relative term is
max(1e-8, 64 eps kappa_2) with kappa_2 of the matrix the reference factors (test_gpu_backward_gn's `hard` rule); the adjoint identity
1e-8 (|ubar_c| |xdot_c| + |g_c| |thetadot_c|) (test_gpu_jvp).  The solved batches are those of test_gpu_class_limits (its cache)."""
import numpy as np
import pytest
import torch

import backward_gn_ref as GN
import backward_ref as BR
import banded_ref as BD
import class_limit_cases as CL
import hessian_fallback_ref as FR
import jvp_ref as JR
import lm_decision_cases as LC
from test_gpu_backward import _nodes
from test_gpu_class_limits import N, Solved, _ring, all_solved, alone_solved, oracle
from test_gpu_jvp import _bits, _by_component, _check_adjoint, _check_against_reference, _jvp, _match_nodes, _raw_jvp, _tangents
from test_gpu_lm_decisions import solved
from test_gpu_parity import TOL_UNITS
from test_gpu_set_inputs import _build, _dev as _inputs
from lfr_amd import capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EPS = np.finfo(np.float64).eps
LFR_ERR_UNSUPPORTED = -5
EXACT, GAUSS_NEWTON, FALLBACK = "exact", "gauss_newton", "exact_or_gauss_newton"
MODE_KW = {EXACT: {}, GAUSS_NEWTON: dict(gauss_newton=True), FALLBACK: dict(gn_fallback=True)}
THREE_MODES = pytest.mark.parametrize("mode", [EXACT, GAUSS_NEWTON, FALLBACK])
TWO_MODES = pytest.mark.parametrize("mode", [EXACT, GAUSS_NEWTON])
ASSEMBLIES = pytest.mark.parametrize("device_assembly", [False, "labels", True], ids=["host", "host_labels", "device"])
VARIANTS = pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
TANGENT_SEED = 7500    # shape k of CL.NAMES draws its tangents from seed TANGENT_SEED + k
_cache = {}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _close(got, ref):
    """the reference tolerance of this pass"""
    return np.linalg.norm(got - ref) <= 1e-8 * np.linalg.norm(ref) + 1e-14


def _call(b, ts, mode, **kw):
    """test_gpu_jvp._jvp in one of the three modes"""
    return _jvp(b, ts, mode == GAUSS_NEWTON, **(dict(gn_fallback=True) if mode == FALLBACK else {}), **kw)


def _run(b, ts, mode):
    """(xdot, stats, per-component status) of one jvp call in `mode`"""
    xdot, st = _call(b, ts, mode, want_stats=True)
    return xdot, st, b.jvp_status().copy()


def _assert_all_differentiated(st, status, n):
    assert len(status) == n and (status == capi.JVP_OK).all()
    assert st["n_differentiated"] == n and st["n_not_usable"] == 0 and st["n_indefinite"] == 0


# --------------------------------------------------------- 1. the reference on ALL: every mode, Tukey variant and assembly
@ASSEMBLIES
@VARIANTS
@THREE_MODES
def test_jvp_matches_the_reference_on_every_shape(lfr_lib, mode, variant, device_assembly):
    """float64 random tangents on all three inputs against jvp_many at the GPU's own positions, no component left out (the reference
    alone has status 0 on every shape: tests/test_jvp_class_limit_ref.py).  The fallback mode is compared with the exact reference
    and is the exact mode's bits: nothing is indefinite here"""
    s = all_solved(device_assembly, variant)
    assert (oracle(variant)["comp"] == s.p.labels()[2]).all()
    ts = _tangents(s.ma, 31)
    comps = s.info["component"].tolist()
    n, st, xdot, worst = _check_against_reference(s.ma, s.g, s.p, s.b, ts, comps, mode == GAUSS_NEWTON, variant)
    status = s.b.jvp_status().copy()
    if mode == FALLBACK:                                          # (the comparison above ran the exact mode)
        _assert_all_differentiated(st, status, N)
        exact, exact_status = xdot, status
        xdot, st, status = _run(s.b, ts, FALLBACK)
        assert _same(xdot, exact) and np.array_equal(status, exact_status)
    print("class limits jvp %s/%s/%s: %d components compared, worst error / bound %.3e" % (mode, variant, device_assembly, n, worst))
    assert n == len(comps) == N                                   # every component compared: none failed, none indefinite
    _assert_all_differentiated(st, status, N)
    assert st["n_bound_coordinates"] == 0 and (np.abs(s.pos) < 1.0).all()
    root = s.p.labels()[1]
    assert root.sum() == N + 1 and not xdot[root].any()          # roots read exact zeros
    for name in CL.NAMES:
        assert xdot[s.nodes[name]].any(), name
    # float32 tangents are the float64 tangents of the same values
    t32 = [t.astype(np.float32) for t in ts]
    x32 = _call(s.b, t32, mode)
    x64 = _call(s.b, [t.astype(np.float64) for t in t32], mode)
    assert x32.dtype == np.float64 and x32.any() and _same(x32, x64) and not _same(x32, xdot)
    assert s.b.spin_timeouts() == 0


# ------------------------------------------------------------------------------------------------------- 2. neighbours in a wave
def _twice():
    """the batch that holds every shape twice, solved once: (first copy, second copy) as two views of it"""
    if "twice" not in _cache:
        mt, feats2 = CL.all_twice()
        first = Solved(mt, feats2[0])
        assert first.st["n_components"] == 2 * N and first.st["n_failed"] == 0
        _cache["twice"] = (first, first.view(feats2[1]))
    return _cache["twice"]


def _shape_tangents(ma, feats_list):
    """(tan_disp1, tan_disp2, tan_sim) of a batch of shapes: every shape draws its tangents from a stream of its own and they sit on
    that shape's match rows, so a shape has the same tangents, bit for bit, in every batch that holds it (class_limit_cases does the
    same for its flows: the rows of a shape are in the same order in every batch, asserted on the flows here)"""
    m = len(ma.sim)
    ts = [np.zeros((m, 18)), np.zeros((m, 18)), np.zeros(m)]
    filled = np.zeros(m, bool)
    for feats in feats_list:
        for name, fs in feats.items():
            rows = np.nonzero(np.isin(ma.feat1, fs))[0]
            own = CL.alone(name)
            assert np.isin(ma.feat2[rows], fs).all() and not filled[rows].any()
            assert np.array_equal(ma.disp1[rows], own.disp1) and np.array_equal(ma.sim[rows], own.sim), name
            rng = np.random.default_rng(TANGENT_SEED + CL.NAMES.index(name))
            for t in ts:
                t[rows] = rng.standard_normal((len(rows),) + t.shape[1:])
            filled[rows] = True
    assert filled.all()
    return ts


@TWO_MODES
def test_a_shape_does_not_depend_on_its_neighbours(lfr_lib, mode):
    """xdot of every shape in ALL, alone in its batch (where rows_max of its class is its own rows: the LDS carving has no slack) and
    in both copies of the doubled batch, from the same tangents: the same bits in the packed and LDS classes, whose positions are the
    same bits; the two 194-row shapes, whose positions differ at rounding level between team shapes, to the reference tolerance"""
    a = all_solved()
    ts = _shape_tangents(a.ma, [a.feats])
    xa, st, status = _run(a.b, ts, mode)
    _assert_all_differentiated(st, status, N)
    assert _same(xa, _run(a.b, ts, mode)[0])                     # a second call on the same batch is bitwise the first
    t0, t1 = _twice()
    xt, st, status = _run(t0.b, _shape_tangents(t0.ma, [t0.feats, t1.feats]), mode)
    _assert_all_differentiated(st, status, 2 * N)
    worst = 0.0
    for name in CL.NAMES:
        x = xa[a.nodes[name]]
        assert x.any(), name
        o = alone_solved(name)
        to = _shape_tangents(o.ma, [o.feats])
        xo, st, status = _run(o.b, to, mode)
        _assert_all_differentiated(st, status, 1)
        assert _same(xo, _run(o.b, to, mode)[0]), name
        for what, y in (("alone", xo[o.nodes[name]]), ("twice, first copy", xt[t0.nodes[name]]), ("twice, second copy", xt[t1.nodes[name]])):
            assert x.shape == y.shape, (name, what)
            if name in CL.TREE:
                worst = max(worst, np.linalg.norm(y - x) / (1e-8 * np.linalg.norm(x) + 1e-14))
                assert _close(y, x), (name, what)
                continue
            assert _same(x, y), "%s, %s: tangents differ by %.3g" % (name, what, np.abs(x - y).max())
    print("neighbours %s: %d shapes bitwise, the two 194-row shapes worst difference / bound %.3e" % (mode, N - len(CL.TREE), worst))


# ----------------------------------------------------------------------------------------------- 3. the adjoint identity per shape
class _FallbackMode:
    """A batch whose jvp and backward run in the fallback mode: test_gpu_jvp._check_adjoint names two modes, this is the third."""

    def __init__(self, b):
        self._b = b

    def __getattr__(self, k):
        return getattr(self._b, k)

    def jvp(self, *a, gauss_newton=False, **kw):
        return self._b.jvp(*a, gn_fallback=True, **kw)

    def backward(self, *a, gauss_newton=False, **kw):
        return self._b.backward(*a, gn_fallback=True, **kw)


@THREE_MODES
def test_adjoint_identity_with_the_backward_on_every_shape(lfr_lib, mode):
    """ubar . (J thetadot) = (J^T ubar) . thetadot against the backward of the same mode, per component: all 33 live and inside the
    bound, the statuses the backward's (both asserted by _check_adjoint for the components it counts)"""
    s = all_solved()
    b = _FallbackMode(s.b) if mode == FALLBACK else s.b
    n, worst, js = _check_adjoint(s.ma, s.g, s.p, b, mode == GAUSS_NEWTON, 36)
    print("class limits adjoint identity %s: %d components, worst |lhs - rhs| / bound %.3e" % (mode, n, worst))
    assert n == N == len(js) and (js == capi.JVP_OK).all() and worst <= 1.0
    assert np.array_equal(js, s.b.jvp_status()) and np.array_equal(js, s.b.backward_status())


# -------------------------------------------------------------------------------------------- 4. bound coordinates per class
@TWO_MODES
@pytest.mark.parametrize("name", ["packed_24_32", "block_m"])
def test_components_at_the_bound(lfr_lib, name, mode):
    """the graphs of test_gpu_backward_gn.test_components_at_the_bound, its rounding-sensitive components set aside: the components
    with a coordinate at the bound against the reference under the `hard` rule, exact zeros on the bound coordinates, their exact
    count over the whole batch, and a tangent on matches between fixed ends"""
    gn = mode == GAUSS_NEWTON
    ma, ref, sensitive = LC.reference(name)
    g, p, b, _, pos = solved(name)
    assert np.array_equal(_bits(b.download()), _bits(pos))
    at_bound = LC.bound_mask(pos)
    track, root, comp = p.labels()
    which = np.setdiff1d(np.unique(comp[at_bound.any(axis=1)]), sensitive).tolist()
    ts = _tangents(ma, 33)
    xdot, st, status = _run(b, ts, mode)
    info = b.component_info()
    stat, term = _by_component(info, status), _by_component(info, info["termination"])
    comps = BR.graph_components(ma, track, root, comp, *_nodes(g, ma), which=set(which))
    assert sorted(comps) == which
    items = []
    for c in which:
        var_nodes, cp = comps[c]
        m, odd = cp.eids >> 1, (cp.eids & 1) == 1
        items.append((cp, pos[var_nodes].reshape(-1), np.where(odd[:, None], ts[0][m], ts[1][m]), ts[2][m]))
    n, n_indefinite, worst = 0, 0, 0.0
    for c, (want, rs) in zip(which, JR.jvp_many(items, gauss_newton=gn)):
        var_nodes, cp = comps[c]
        x, got = pos[var_nodes].reshape(-1), xdot[var_nodes].reshape(-1)
        assert term[c] != capi.TERM_FAILURE and (np.abs(x) >= 1.0).any()
        if rs == 2:                                               # indefinite on both sides: a zero tangent
            assert stat[c] == capi.JVP_INDEFINITE and not got.any(), "component %d" % c
            n_indefinite += 1
            continue
        assert stat[c] == capi.JVP_OK, "component %d" % c
        kappa = GN.Component.of(cp).kappa2(x) if gn else FR.kappa2(cp, x, FR.OK)
        rel = max(1e-8, 64.0 * EPS * kappa)
        ratio = np.linalg.norm(got - want) / (rel * np.linalg.norm(want) + 1e-14)
        worst = max(worst, ratio)
        assert ratio <= 1.0, "component %d: error / bound %.3f (kappa_2 %.3e)" % (c, ratio, kappa)
        assert got.any() and not got[np.abs(x) >= 1.0].any()
        n += 1
    print("%s %s: %d components with a coordinate at the bound, %d compared, %d indefinite on both sides, worst error / bound %.3e, "
          "%d coordinates at a bound" % (name, mode, len(which), n, n_indefinite, worst, st["n_bound_coordinates"]))
    assert n + n_indefinite == len(which) >= 5 and n >= 1
    assert n_indefinite == 0 or not gn                            # Gauss-Newton mode: every selected component is compared
    assert st["n_bound_coordinates"] == int(at_bound.sum()) >= 1
    fixed = root[:, None] | (np.abs(pos) >= 1.0)
    assert root.any() and not xdot[fixed].any()
    # a tangent on the matches whose two ends are both fixed (a root, or a node with a coordinate at the bound) and on nothing else
    n1, n2 = _match_nodes(ma, g)
    held = root | at_bound.any(axis=1)
    kept = ((track[n1] == track[n2]) | (comp[n1] == comp[n2])) & ~(root[n1] & root[n2])
    sel = held[n1] & held[n2] & kept
    assert sel.sum() >= 1
    only = [np.where(sel.reshape((-1,) + (1,) * (t.ndim - 1)), t, 0.0) for t in ts]
    xf, _, status_f = _run(b, only, mode)
    assert np.array_equal(status_f, status) and not xf[fixed].any()
    assert xf.any() or not gn                                     # (the free coordinate of such a node does move; exact mode: it may be indefinite)
    assert not xf[~np.isin(comp, comp[n1[sel]])].any()            # and nobody else's


# ------------------------------------------------------------------------------------------------------ 5. the 6144-row limit
def _ring_solved(n):
    if ("ring", n) not in _cache:
        ma = _ring(n)
        g = capi.Graph.from_arrays(ma)
        p = capi.Problem(g)
        b = capi.Batch(p, 0)
        st = b.solve()
        info = b.component_info()
        assert info["n_var_nodes"].tolist() == [n - 1] and info["n_edges"].tolist() == [2 * n]
        assert st["n_failed"] == 0 and info["termination"][0] != capi.TERM_FAILURE
        _cache[("ring", n)] = (ma, g, p, b, b.download().copy())
    return _cache[("ring", n)]


@TWO_MODES
def test_jvp_at_6144_rows(lfr_lib, mode):
    """one ring of 3073 nodes: 6144 rows, the largest system the pass serves (pass_begin's limit, kBwdMaxRows), against
    banded_ref.jvp - jvp_ref's right-hand side and a longdouble banded Cholesky, pinned to jvp_ref.jvp by tests/test_banded_ref.py -
    under the `hard` rule with kappa_2 of the matrix it factors"""
    gn = mode == GAUSS_NEWTON
    ma, g, p, b, x = _ring_solved(3073)
    ts = _tangents(ma, 34)
    xdot, st, status = _run(b, ts, mode)
    assert status.tolist() == [capi.JVP_OK] and st["n_differentiated"] == 1
    track, root, comp = p.labels()
    (var_nodes, cp), = BR.graph_components(ma, track, root, comp, *_nodes(g, ma)).values()
    assert len(var_nodes) == 3072
    xc = x[var_nodes].reshape(-1)
    m, odd = cp.eids >> 1, (cp.eids & 1) == 1
    ref, rs = BD.jvp(cp, xc, np.where(odd[:, None], ts[0][m], ts[1][m]), ts[2][m], gauss_newton=gn)
    assert rs == 0 and ref.any()
    kappa = BD.Inverse(BD.reduced_hessian(cp, xc, gn)).kappa2
    rel = max(1e-8, 64.0 * EPS * kappa)
    got = xdot[var_nodes].reshape(-1)
    print("6144 rows: jvp %s relative error %.3e (bound %.3e), kappa_2 %.3e"
          % (mode, np.linalg.norm(got - ref) / np.linalg.norm(ref), rel, kappa))
    assert np.linalg.norm(got - ref) <= rel * np.linalg.norm(ref) + 1e-14
    assert st["n_bound_coordinates"] == int((np.abs(xc) >= 1.0).sum()) and not got[np.abs(xc) >= 1.0].any()
    assert root.sum() == 1 and not xdot[root].any()
    assert b.spin_timeouts() == 0


def test_jvp_refuses_6146_rows(lfr_lib):
    """one ring of 3074 nodes: 6146 rows, two more than the dense factorization serves.  The solve is served; the jvp answers
    LFR_ERR_UNSUPPORTED in every mode, names the rows and leaves its output untouched; the batch goes on solving"""
    ma, g, p, b, x = _ring_solved(3074)
    assert x.any() and np.isfinite(x).all()
    d = [torch.as_tensor(t, device=DEV) for t in _tangents(ma, 35)]
    out = torch.full((g.n_nodes, 2), 7.0, dtype=torch.float64, device=DEV)
    for flags in (capi.JVP_F64, capi.JVP_F64 | capi.JVP_GAUSS_NEWTON, capi.JVP_F64 | capi.JVP_FALLBACK_GAUSS_NEWTON):
        assert _raw_jvp(b, d, flags, out) == LFR_ERR_UNSUPPORTED, flags
        message = capi.lib().lfr_last_error().decode("utf-8", "replace")
        assert "6146 rows" in message and "6144" in message, message
        assert (out == 7.0).all()                                # a refused call writes nothing
    for kw in MODE_KW.values():
        with pytest.raises(capi.LfrError) as e:
            b.jvp(*d, f64=True, **kw)
        assert e.value.code == LFR_ERR_UNSUPPORTED
        assert "6146 rows" in str(e.value) and "6144" in str(e.value)
    b.solve()                                                     # (to the position tolerance: the team that serves it may differ from solve to solve)
    assert np.abs(b.download() - x).max() <= TOL_UNITS
    assert b.spin_timeouts() == 0


# ------------------------------------------------------------------------------------------------------------------ 6. set_inputs
@pytest.mark.parametrize("kind", ["host", "fused"])
def test_set_inputs_equals_a_fresh_build(lfr_lib, kind):
    """new flows and similarities (class_limit_cases.second_inputs: the structure of ALL) into the live batch: the jvp after the next
    solve is that of a batch built from the new inputs, bit for bit, in both modes - and not the one before"""
    ma, _ = CL.all_shapes()
    mb = CL.second_inputs()
    gb, pb, b, _ = _build(mb, kind)
    b.solve()
    ga, pa, a, _ = _build(ma, kind)
    a.solve()
    ts = _tangents(ma, 37)
    before = {mode: _run(a, ts, mode)[0] for mode in (EXACT, GAUSS_NEWTON)}
    a.set_inputs(_inputs(mb.disp1), _inputs(mb.disp2), _inputs(mb.sim, flows=False))
    a.solve()
    assert np.array_equal(_bits(a.download()), _bits(b.download())) and a.team_fallbacks() == 0 and b.team_fallbacks() == 0
    for mode in (EXACT, GAUSS_NEWTON):
        got, gst, gs = _run(a, ts, mode)
        want, wst, ws = _run(b, ts, mode)
        _assert_all_differentiated(wst, ws, N)
        assert np.array_equal(gs, ws) and gst["n_differentiated"] == N, mode
        assert want.any() and _same(got, want) and not _same(got, before[mode]), mode
    assert a.spin_timeouts() == 0
