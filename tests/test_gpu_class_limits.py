"""Every launch class at its exact row and edge limits: the shapes of tests/class_limit_cases.py (tests/test_class_limit_cases.py
establishes on the CPU that each sits where its table says) through solve, device assembly, backward, covariance and
lfr_batch_set_inputs, and the capacity limits include/lfr.h documents.

A component full to its last edge slot, one edge past the resident slots, rows that fit a class whose edges do not, the first and the
last row count of every LDS footprint and the smallest elimination-tree component are where an off-by-one of classify(), of
classify_dev(), of a slot loop or of an LDS size shows; the neighbours tests place every shape alone, among the others and in a
batch that holds each twice, so that a full last slot leaking into the next group of its wave changes some bit."""
import numpy as np
import pytest

import class_limit_cases as CL
import lfr_oracle as O
from test_gpu_backward import _check_against_reference as backward_check, _ubar      # (imports torch: before the library is loaded)
from test_gpu_covariance import _check_against_reference as covariance_check
from test_gpu_set_inputs import _assert_same_solve, _bits, _build, _dev
from lfr_amd import capi, synthetic
from test_gpu_parity import TOL_UNITS

pytestmark = pytest.mark.gpu
N = len(CL.NAMES)
LFR_ERR_UNSUPPORTED = -5
_cache = {}


def _shape_nodes(g, feats):
    """{name: graph nodes of the shape ordered by (image, feature)}: the same nodes in the same order in every batch that holds it"""
    ni, nf = g.nodes()
    img = np.array([int(n[:6]) for n in g.image_names()])[ni]
    out = {}
    for name, fs in feats.items():
        sel = np.nonzero(np.isin(nf, fs))[0]
        out[name] = sel[np.lexsort((nf[sel], img[sel]))]
    return out


class Solved:
    """a graph of shapes, host- or device-assembled, solved once: positions, info and stats of that first solve"""

    def __init__(self, ma, feats, device_assembly=False, variant="ceres1"):
        """device_assembly: False - graph stage and assembly on the host; "labels" - the host's labels, the batch assembled on the GPU
        (classify_dev against classify and nothing else); True - graph stage and assembly on the GPU"""
        self.ma, self.feats = ma, feats
        self.g = capi.Graph.from_arrays(ma)
        self.p = (capi.Problem(self.g, device_assembly=True) if device_assembly == "labels" else
                  capi.Problem(self.g, device_graph_stage=0) if device_assembly else capi.Problem(self.g))
        self.b = capi.Batch(self.p, 0, tukey_variant=variant)
        self.st = self.b.solve()
        self.pos = self.b.download().copy()
        self.info = self.b.component_info()
        self._index(feats)

    def _index(self, feats):
        self.feats = feats
        self.nodes = _shape_nodes(self.g, feats)
        self.comp = CL.components_of(feats, self.g.nodes()[1], self.p.labels()[2])
        self.row = {name: int(np.nonzero(self.info["component"] == c)[0][0]) for name, c in self.comp.items()}      # row of component_info

    def view(self, feats):
        """the same solved batch, its shapes looked up through other features (the second copy of a batch that holds every shape twice)"""
        v = Solved.__new__(Solved)
        v.__dict__.update(self.__dict__)
        v._index(feats)
        return v


def all_solved(device_assembly=False, variant="ceres1"):
    key = ("all", device_assembly, variant)
    if key not in _cache:
        ma, feats = CL.all_shapes()
        _cache[key] = Solved(ma, feats, device_assembly, variant)
    return _cache[key]


def alone_solved(name):
    if ("alone", name) not in _cache:
        _cache[("alone", name)] = Solved(CL.alone(name), {name: [0, 1] if name == CL.TWO_ROOTS else [0]})
    return _cache[("alone", name)]


def oracle(variant="ceres1"):
    if ("oracle", variant) not in _cache:
        ref = O.run(CL.all_shapes()[0], n_threads=4, tukey_variant=variant)
        assert ref["rc"] == 0
        _cache[("oracle", variant)] = ref
    return _cache[("oracle", variant)]


# ------------------------------------------------------------------------------------------------------ solve against the oracle
def test_every_shape_matches_the_oracle(lfr_lib):
    s, ref = all_solved(), oracle()
    assert (ref["comp"] == s.p.labels()[2]).all()
    assert s.st["n_failed"] == 0 and s.st["n_components"] == len(s.info["component"]) == N
    for name in CL.NAMES:
        c, r = s.comp[name], s.row[name]
        sh = CL.SHAPES[name]
        assert (2 * s.info["n_var_nodes"][r], s.info["n_edges"][r]) == (sh["rows"], sh["edges"]), name
        err = np.abs(s.pos[s.nodes[name]] - ref["positions"][s.nodes[name]]).max()
        oi = ref["infos"][c]
        print("%-18s %3d rows %5d edges %-12s max |dx| %.3e, iterations %d (oracle %d)"
              % (name, sh["rows"], sh["edges"], sh["cls"], err, s.info["iterations"][r], oi["iterations"]))
        assert err <= TOL_UNITS, name
        assert s.info["termination"][r] == oi["termination"] == capi.TERM_CONVERGENCE, name
        assert s.info["iterations"][r] == oi["iterations"], name
    oc = ref["infos"][s.info["component"]]
    ne = s.info["n_edges"].astype(np.int64)
    assert s.st["ref_jacobian_passes_edges"] == int((oc["n_jac_evals"] * ne).sum())
    assert s.st["ref_cost_passes_edges"] == int((oc["n_cost_evals"] * ne).sum())
    assert s.b.spin_timeouts() == 0


@pytest.mark.parametrize("name", CL.NAMES)
def test_shape_runs_in_the_launch_of_its_class(lfr_lib, name):
    """alone in its batch, the component's edges are counted in the slot of its class and in no other (lfr_batch_timing)"""
    s = alone_solved(name)
    sh = CL.SHAPES[name]
    assert s.st["n_components"] == 1 and s.st["n_failed"] == 0
    assert (2 * s.info["n_var_nodes"][0], s.info["n_edges"][0]) == (sh["rows"], sh["edges"])
    _, _, class_edges = s.b.timing()
    want = np.zeros(capi.NUM_KERNEL_CLASSES, np.int64)
    want[CL.CLASS_SLOT[sh["cls"]]] = sh["edges"]
    assert class_edges.tolist() == want.tolist()
    ts = s.b.tree_stats()
    if name in CL.TREE:
        assert ts["columns"][0] >= (sh["rows"] + 15) // 16 and ts["tiles"][0] >= ts["columns"][0] and ts["levels"][0] >= 1
        dense = ts["tiles"][0] == ts["columns"][0] * (ts["columns"][0] + 1) // 2
        assert dense != CL.THIN_PLAN[name]                        # (a complete track fills every tile, a ring few)
    else:
        assert not any(v.any() for v in ts.values())
    assert s.b.spin_timeouts() == 0


# ------------------------------------------------------------------------------------------- device assembly == host assembly
@pytest.mark.parametrize("how", ["labels", True], ids=["host_labels", "device_graph_stage"])
def test_device_assembly_classifies_and_solves_as_the_host_assembly(lfr_lib, how):
    """the batch assembled on the GPU - from the host's labels (only classify_dev and the device assembly differ from the host path)
    and from the device graph stage's (the pipeline the benchmark runs) - against the host-assembled one"""
    h, d = all_solved(), all_solved(device_assembly=how)
    assert (oracle()["comp"] == d.p.labels()[2]).all()
    for k in ("component", "n_var_nodes", "n_edges", "iterations", "termination"):
        assert np.array_equal(h.info[k], d.info[k]), k           # the same components in the same batch order: classify_dev == classify
    assert np.array_equal(_bits(h.info["final_cost"]), _bits(d.info["final_cost"]))
    assert np.array_equal(_bits(h.pos), _bits(d.pos))
    for k in ("n_components", "n_edges", "ref_jacobian_passes_edges", "ref_cost_passes_edges", "exec_passes_edges"):
        assert h.st[k] == d.st[k], k


# ------------------------------------------------------------------------------------------------------- neighbours in a wave
def test_a_shape_does_not_depend_on_its_neighbours(lfr_lib):
    """ALL, every ALONE[name] and a batch that holds ALL twice: positions, iterations and final cost of every packed and LDS-class
    component are the same bits in all of them; the two 194-row components agree to the position tolerance (include/lfr.h promises
    rounding-level equality across team shapes for the elimination-tree kernel)"""
    a = all_solved()
    mt, feats2 = CL.all_twice()
    twice0 = Solved(mt, feats2[0])
    twice1 = twice0.view(feats2[1])                               # the second copy: the same solved batch seen through its own features
    assert twice0.st["n_components"] == 2 * N and twice0.st["n_failed"] == 0
    assert not set(twice0.comp.values()) & set(twice1.comp.values())
    for name in CL.NAMES:
        x, r = a.pos[a.nodes[name]], a.row[name]
        for what, other in (("alone", alone_solved(name)), ("twice, first copy", twice0), ("twice, second copy", twice1)):
            y, q = other.pos[other.nodes[name]], other.row[name]
            assert x.shape == y.shape and x.any(), (name, what)
            assert a.info["termination"][r] == other.info["termination"][q], (name, what)
            if name in CL.TREE:
                assert np.abs(x - y).max() <= TOL_UNITS, (name, what)
                continue
            assert np.array_equal(_bits(x), _bits(y)), "%s, %s: positions differ by %.3g" % (name, what, np.abs(x - y).max())
            assert a.info["iterations"][r] == other.info["iterations"][q], (name, what)
            assert np.array_equal(_bits(a.info["final_cost"][r]), _bits(other.info["final_cost"][q])), (name, what)


def test_second_solve_is_bitwise_the_first(lfr_lib):
    for s in (all_solved(), all_solved(device_assembly="labels"), all_solved(device_assembly=True)):
        s.b.solve()
        assert np.array_equal(_bits(s.b.download()), _bits(s.pos))
        info = s.b.component_info()
        assert np.array_equal(info["iterations"], s.info["iterations"]) and np.array_equal(_bits(info["final_cost"]), _bits(s.info["final_cost"]))
        assert s.b.spin_timeouts() == 0


# -------------------------------------------------------------------------------------------------- backward and covariance
@pytest.mark.parametrize("device_assembly", [False, "labels", True], ids=["host", "host_labels", "device"])
@pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
def test_backward_matches_the_reference_on_every_shape(lfr_lib, variant, device_assembly):
    s = all_solved(device_assembly, variant)
    gp = _ubar(s.g.n_nodes, 21)
    comps = s.info["component"].tolist()
    n, st, (g1, g2, gs) = backward_check(s.ma, s.g, s.p, s.b, gp, comps, variant)
    assert n == len(comps) == N                                   # every component compared: none failed, none indefinite
    assert (s.b.backward_status() == capi.BACKWARD_OK).all()
    assert st["n_differentiated"] == N and st["n_not_usable"] == 0 and st["n_indefinite"] == 0
    for x, f in zip((g1, g2, gs), s.b.backward(gp)):
        f = f.cpu().numpy()
        assert f.dtype == np.float32 and np.array_equal(f, x.astype(np.float32))


@pytest.mark.parametrize("device_assembly", [False, "labels", True], ids=["host", "host_labels", "device"])
@pytest.mark.parametrize("variant", ["ceres1", "ceres2"])
def test_covariance_matches_the_reference_on_every_shape(lfr_lib, variant, device_assembly):
    s = all_solved(device_assembly, variant)
    comps = s.info["component"].tolist()
    n, st, worst = covariance_check(s.ma, s.g, s.p, s.b, comps, variant)
    print("covariance %s/%s: worst error / bound %.4f" % (variant, device_assembly, worst))
    assert n == len(comps) == N
    assert (s.b.covariance_status() == capi.COVARIANCE_OK).all()
    assert st["n_computed"] == N and st["n_not_usable"] == 0 and st["n_singular"] == 0
    c64, c32 = s.b.covariance(f64=True).cpu().numpy(), s.b.covariance().cpu().numpy()
    assert c32.dtype == np.float32 and np.array_equal(c32, c64.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ set_inputs
@pytest.mark.parametrize("kind", ["host", "fused"])
def test_set_inputs_equals_a_fresh_build(lfr_lib, kind):
    """new flows and similarities (class_limit_cases.second_inputs: the structure of ALL) into the live batch: the solve, the backward
    and the covariance after it are those of a batch built from the new inputs, bit for bit"""
    import torch
    ma, _ = CL.all_shapes()
    mb = CL.second_inputs()
    gb, pb, b, _ = _build(mb, kind)
    b.solve()
    ga, pa, a, _ = _build(ma, kind)
    a.solve()
    x0 = a.download().copy()
    a.set_inputs(_dev(mb.disp1), _dev(mb.disp2), _dev(mb.sim, flows=False))
    a.solve()
    assert len(a.component_info()["component"]) == N
    _assert_same_solve(a, b, pb, "class limits/" + kind)
    assert not np.array_equal(a.download(), x0)
    assert a.team_fallbacks() == 0 and b.team_fallbacks() == 0    # (so _assert_same_solve compared every component bit for bit)
    gp = torch.as_tensor(np.random.default_rng(22).standard_normal((ga.n_nodes, 2)), device=torch.device("cuda", 0))
    got = [t.cpu().numpy() for t in a.backward(gp, f64=True)] + [a.covariance(f64=True).cpu().numpy()]
    want = [t.cpu().numpy() for t in b.backward(gp, f64=True)] + [b.covariance(f64=True).cpu().numpy()]
    assert np.array_equal(a.backward_status(), b.backward_status()) and (b.backward_status() == capi.BACKWARD_OK).all()
    assert np.array_equal(a.covariance_status(), b.covariance_status()) and (b.covariance_status() == capi.COVARIANCE_OK).all()
    for what, x, y in zip(("grad_disp1", "grad_disp2", "grad_sim", "covariance"), got, want):
        assert np.array_equal(_bits(x), _bits(y)) and y.any(), what
    assert a.spin_timeouts() == 0


# ------------------------------------------------------------------------------------------- the documented capacity limits
def _ring(n):
    return synthetic.generate(seed=31, n_images=n, n_tracks=1, len_dist="uniform", len_lo=n, len_hi=n, track_degree=2)


def _small_batch_still_solves():
    s = Solved(CL.alone("k5_full"), {"k5_full": [0]})
    assert np.array_equal(_bits(s.pos), _bits(alone_solved("k5_full").pos)) and s.st["n_failed"] == 0 and s.pos.any()


def test_backward_and_covariance_at_6144_rows(lfr_lib):
    """one ring of 3073 nodes: 6144 rows, the largest system backward and covariance serve (kBwdMaxRows: the matrix in the HBM
    workspace, the LDS full of vectors).  Against backward_ref and covariance_ref at the tolerances of test_gpu_backward and
    test_gpu_covariance (its rule above 400 rows: 48 sampled nodes); the references' linear algebra is tests/banded_ref.py's banded
    Cholesky, pinned to the dense forms by tests/test_banded_ref.py, because those take minutes at this size"""
    import backward_ref as BR
    import banded_ref as BD
    import covariance_ref as CR
    import linsolve_ref as LS
    from test_gpu_backward import _nodes
    ma = _ring(3073)
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g)
    b = capi.Batch(p, 0)
    st = b.solve()
    info = b.component_info()
    assert info["n_var_nodes"].tolist() == [3072] and info["n_edges"].tolist() == [2 * 3073]
    assert st["n_failed"] == 0 and info["termination"][0] != capi.TERM_FAILURE
    x = b.download().copy()
    gp = _ubar(g.n_nodes, 23)
    g1, g2, gs, bst = b.backward(gp, f64=True, want_stats=True)
    g1, g2, gs = g1.cpu().numpy(), g2.cpu().numpy(), gs.cpu().numpy()
    cov, cst = b.covariance(f64=True, want_stats=True)
    cov = cov.cpu().numpy()
    assert b.backward_status().tolist() == [capi.BACKWARD_OK] and bst["n_differentiated"] == 1
    assert b.covariance_status().tolist() == [capi.COVARIANCE_OK] and cst["n_computed"] == 1
    track, root, comp = p.labels()
    (var_nodes, cp), = BR.graph_components(ma, track, root, comp, *_nodes(g, ma)).values()
    assert len(var_nodes) == 3072
    xc = x[var_nodes].reshape(-1)
    # backward: test_gpu_backward._check_against_reference's comparison
    gf, gw, rs = BD.backward(cp, xc, gp.cpu().numpy()[var_nodes].reshape(-1))
    assert rs == 0
    m, odd = cp.eids >> 1, (cp.eids & 1) == 1
    ref_s = np.zeros(len(ma.sim))
    np.add.at(ref_s, m, gw)
    ref = np.concatenate([gf.ravel(), ref_s[np.unique(m)]])
    got = np.concatenate([np.where(odd[:, None], g1[m], g2[m]).ravel(), gs[np.unique(m)]])
    berr = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    # covariance: test_gpu_covariance._check_against_reference's comparison above 400 rows
    c = cov[var_nodes]
    assert (c[:, 0] > 0).all() and (c[:, 2] > 0).all() and (c[:, 0] * c[:, 2] - c[:, 1] ** 2 >= 0).all() and not cov[root].any()
    inv = BD.Inverse(BD.normal_matrix(CR.problem_of(cp), xc))
    n = 2 * len(var_nodes)
    sel = np.unique(np.concatenate([[0, n // 2 - 1], np.random.default_rng(17).choice(n // 2, 46, replace=False)]))
    cols = np.stack([2 * sel, 2 * sel + 1], 1).reshape(-1).tolist()
    X = inv.columns(cols)
    cerr = float(np.max(np.abs(c[sel].astype(LS.LD) - CR.node_blocks(X, cols))))
    bound = inv.bound(X, cols)
    print("6144 rows: backward relative error %.3e, covariance error %.3e (bound %.3e), kappa_2 %.3e" % (berr, cerr, bound, inv.kappa2))
    assert np.linalg.norm(got - ref) <= 1e-8 * np.linalg.norm(ref) + 1e-14
    assert cerr <= bound
    assert b.spin_timeouts() == 0


def test_backward_and_covariance_refuse_6146_rows(lfr_lib):
    """one ring of 3074 nodes: 6146 rows, two more than the dense factorization's vectors fit in LDS (kBwdMaxRows).  The solve is
    served; backward and covariance answer LFR_ERR_UNSUPPORTED and name the rows; the batch goes on solving"""
    import torch
    ma = _ring(3074)
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g)
    b = capi.Batch(p, 0)
    st = b.solve()
    info = b.component_info()
    assert info["n_var_nodes"].tolist() == [3073] and info["n_edges"].tolist() == [2 * 3074]
    assert st["n_failed"] == 0 and info["termination"][0] != capi.TERM_FAILURE
    x = b.download().copy()
    assert x.any() and np.isfinite(x).all()
    gp = torch.zeros((g.n_nodes, 2), dtype=torch.float64, device=torch.device("cuda", 0))
    for call in (lambda: b.backward(gp, f64=True), lambda: b.covariance(f64=True)):
        with pytest.raises(capi.LfrError) as e:
            call()
        assert e.value.code == LFR_ERR_UNSUPPORTED
        assert "6146 rows" in str(e.value) and "6144" in str(e.value)
    b.solve()                                                     # (to the position tolerance: the team that serves it may differ from solve to solve)
    assert np.abs(b.download() - x).max() <= TOL_UNITS
    assert b.spin_timeouts() == 0


@pytest.mark.parametrize("assembly", ["host", "device"])
def test_component_of_32768_nodes_is_refused(lfr_lib, assembly):
    """one ring of 32768 nodes, one more than a component's local indices hold (15 bits): the host assembly refuses in
    lfr_problem_build, the device assembly in lfr_batch_create; nothing is solved at this size, and the device stays usable"""
    ma = CL.tracks(32, [(32768, 32768, 0)])                       # (32768 images, so the size cap does not cut it)
    g = capi.Graph.from_arrays(ma)
    assert g.n_nodes == 32768
    with pytest.raises(capi.LfrError) as e:
        if assembly == "host":
            capi.Problem(g)
        else:
            p = capi.Problem(g, device_assembly=True)             # labels only: the batch is assembled on the GPU
            assert np.bincount(p.labels()[2]).tolist() == [32768]
            capi.Batch(p, 0)
    assert e.value.code == LFR_ERR_UNSUPPORTED
    assert "exceeds the 32767-node batch limit" in str(e.value)
    _small_batch_still_solves()
