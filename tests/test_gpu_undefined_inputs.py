"""Inputs the reference does not define: similarities that are 0, negative, +inf or NaN (cosine similarities of
two-view-refinement/feature_matchers.py:36-63 are unconstrained in sign; solve.cc:111,120 hand them to ScaledLoss), flow entries that are
not finite, all-zero flow grids (SKIP_REFINEMENT, compute_match_graph.py:150-152).

The library's contract (include/lfr.h, "Undefined inputs"): a component whose evaluation is not finite never produces a valid LM step,
terminates LFR_TERM_FAILURE after ten invalid steps and keeps ZERO displacements (Ceres: non-finite residuals / jacobians fail the
evaluation, IsSolutionUsable() is false, solve.cc:609-612 left the positions at 0); every other component - also those packed into the
same wave - is solved as if the bad edge were not in the file.  The HIP path must agree with the C oracle on terminations and positions.
A NaN similarity additionally makes the order-dependent graph stage (solve.cc:489-582 sorts by similarity) undefined in the reference
itself: it is only tested where the order cannot matter (two images: every track is one match)."""
import copy

import numpy as np
import pytest

import lfr_oracle as O
from lfr_amd import capi, synthetic

pytestmark = pytest.mark.gpu
TOL_UNITS = 6.25e-6


def run_both(ma, device_stage):
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g, device_graph_stage=0) if device_stage else capi.Problem(g)
    b = capi.Batch(p, 0)
    st = b.solve()
    pos = b.download().copy()
    info = b.component_info()
    ref = O.run(ma, n_threads=4)
    assert ref["rc"] == 0
    return p, st, pos, info, ref


def check_against_oracle(p, st, pos, info, ref):
    assert (ref["comp"] == p.labels()[2]).all()
    assert not np.isnan(pos).any()
    oi = ref["infos"][info["component"]]
    assert (oi["termination"] == info["termination"]).all()
    assert np.abs(pos - ref["positions"]).max() <= TOL_UNITS


@pytest.mark.parametrize("device_stage", [False, True])
@pytest.mark.parametrize("what", ["sim_zero", "sim_negative", "sim_inf", "flow_pinf", "flow_ninf", "flow_nan"])
def test_one_bad_edge_fails_its_component_only(lfr_lib, what, device_stage):
    """Short tracks: 8-row and 16-row packed classes, eight / four components to a wave.  One match of one track is poisoned."""
    ma0 = synthetic.generate(seed=91, n_images=16, n_tracks=600)
    p0, st0, pos0, info0, ref0 = run_both(ma0, device_stage)
    assert st0["n_failed"] == 0
    ma = copy.deepcopy(ma0)
    m = 37
    if what == "sim_zero": ma.sim[m] = 0.0
    elif what == "sim_negative": ma.sim[m] = -0.5
    elif what == "sim_inf": ma.sim[m] = np.inf
    elif what == "flow_pinf": ma.disp2[m, 4, 0] = np.inf
    elif what == "flow_ninf": ma.disp1[m, 0, 1] = -np.inf
    else: ma.disp2[m, 8, 1] = np.nan
    p, st, pos, info, ref = run_both(ma, device_stage)
    check_against_oracle(p, st, pos, info, ref)
    comp = p.labels()[2]
    n1 = int(ma.feat1[m])      # (node ids are not feature ids: find the component through the oracle's node table instead)
    changed = np.abs(pos - pos0).max(axis=1) > 0
    if what == "sim_zero":
        # a zero weight is a legal input: the edge drops out of the cost, its component is solved without it
        assert st["n_failed"] == 0
        assert len(set(comp[changed])) <= 1
    else:
        assert st["n_failed"] == 1
        bad = info["component"][info["termination"] == 2]
        assert bad.size == 1
        nodes_bad = comp == bad[0]
        assert (pos[nodes_bad] == 0).all()                       # a failed component keeps zero displacements
        assert (pos[~nodes_bad] == pos0[~nodes_bad]).all()       # everything else is BITWISE what it was without the bad edge
        assert changed[nodes_bad].any()


@pytest.mark.parametrize("what", ["sim_negative", "flow_nan"])
def test_bad_edge_in_a_workgroup_component(lfr_lib, what):
    """The same for the workgroup-per-component kernels (long tracks: LDS-matrix classes, fused sweep with fixed-point sums - a NaN term
    sends the component down the scratch sweep first): the poisoned component fails with zeros, the others are bitwise untouched."""
    ma0 = synthetic.generate(seed=93, n_images=96, n_tracks=40, len_dist="uniform", len_lo=20, len_hi=70)
    p0, st0, pos0, info0, ref0 = run_both(ma0, False)
    assert st0["n_failed"] == 0
    ma = copy.deepcopy(ma0)
    m = 1234
    if what == "sim_negative": ma.sim[m] = -0.25
    else: ma.disp1[m, 3, 0] = np.nan
    p, st, pos, info, ref = run_both(ma, False)
    check_against_oracle(p, st, pos, info, ref)
    assert st["n_failed"] == 1
    comp = p.labels()[2]
    bad = info["component"][info["termination"] == 2]
    nodes_bad = comp == bad[0]
    assert (pos[nodes_bad] == 0).all() and (pos[~nodes_bad] == pos0[~nodes_bad]).all()


def test_nan_similarity_two_images(lfr_lib):
    """Two images: every track is a single match.  Even here the reference's graph stage is order-dependent on a NaN (which end of a
    two-node track becomes its root is a tie broken by the similarity order, solve.cc:552-582), so the oracle is not the yardstick:
    the poisoned component fails with zeros, nothing non-finite comes out, and every component whose root did not move is BITWISE what
    it was without the NaN - including the seven that share the poisoned component's wave."""
    ma0 = synthetic.generate(seed=92, n_images=2, n_tracks=500)
    g0 = capi.Graph.from_arrays(ma0)
    p0 = capi.Problem(g0)
    pos0, st0 = p0.solve_hip(0)
    ma = copy.deepcopy(ma0)
    ma.sim[11] = np.nan
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g)
    b = capi.Batch(p, 0)
    st = b.solve()
    pos = b.download()
    info = b.component_info()
    assert np.isfinite(pos).all() and np.abs(pos).max() <= 1.0
    assert st["n_failed"] == 1 and st0["n_failed"] == 0
    (_, root0, comp0), (_, root, comp) = p0.labels(), p.labels()
    assert (comp == comp0).all()
    bad = info["component"][info["termination"] == 2]
    assert bad.size == 1 and (pos[comp == bad[0]] == 0).all()
    same_root = np.ones(len(comp), bool)
    for c in np.unique(comp[root != root0]):
        same_root &= comp != c
    same_root &= comp != bad[0]
    assert same_root.sum() >= 0.9 * len(comp)
    assert (pos[same_root] == pos0[same_root]).all()


def test_all_zero_flow_grids_at_config2_size(lfr_lib):
    """SKIP_REFINEMENT (compute_match_graph.py:150-152) writes all-zero grids: x = 0 is the minimiser with zero cost and gradient, every
    component converges at iteration 0 and no displacement leaves zero - at config-2 size (100 k tracks), through the device pipeline."""
    ma = synthetic.config2()
    ma.disp1[:] = 0.0
    ma.disp2[:] = 0.0
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g, device_graph_stage=0)
    b = capi.Batch(p, 0)
    st = b.solve()
    pos = b.download()
    assert st["n_failed"] == 0 and st["n_converged"] == st["n_components"] > 90000
    assert (pos == 0).all()
    info = b.component_info()
    assert (info["iterations"] == 0).all()
    # the oracle on a sample of the same graph (the full size takes the C oracle a while): same outcome
    ms = synthetic.generate(seed=7, n_images=64, n_tracks=2000)
    ms.disp1[:] = 0.0
    ms.disp2[:] = 0.0
    _, st2, pos2, info2, ref2 = run_both(ms, True)
    assert (pos2 == 0).all() and (ref2["positions"] == 0).all()
    assert (ref2["infos"][info2["component"]]["iterations"] == info2["iterations"]).all()


# the first evaluation of a solve in the packed classes takes eval_edge's origin shortcut, which reads 10 of the 18 flow values (the
# centre of the grid and its four neighbours); the other 8, the corners, only the general form reads.  include/lfr.h, "Undefined
# inputs": a non-finite corner is seen one evaluation later - the first step is taken, the re-evaluation fails the component: the same
# termination and zeros, one iteration more than the oracle (Ceres).
READ_AT_ORIGIN = (2, 3, 6, 7, 8, 9, 10, 11, 14, 15)
_wave = {}


def _check_flow_position(k, st, info, ref, r, st8, info8):
    """iterations and evaluation counts of a batch whose component in row r holds a non-finite flow value at position k, as
    include/lfr.h states them; st8, info8: the same batch with the value at position 8, which every evaluation reads"""
    oi = ref["infos"][info["component"]]
    ne = info["n_edges"].astype(np.int64)
    others = np.arange(len(ne)) != r
    assert (info["iterations"][others] == oi["iterations"][others]).all()
    if k in READ_AT_ORIGIN:
        assert info["iterations"][r] == oi["iterations"][r]
        assert st["ref_jacobian_passes_edges"] == int((oi["n_jac_evals"] * ne).sum())
        assert st["ref_cost_passes_edges"] == int((oi["n_cost_evals"] * ne).sum())
        for f in ("component", "iterations", "termination", "n_var_nodes", "n_edges"):
            assert np.array_equal(info[f], info8[f]), f
        for f in ("n_converged", "n_failed", "sum_iterations", "ref_jacobian_passes_edges", "ref_cost_passes_edges"):
            assert st[f] == st8[f], f
    else:
        assert info["iterations"][r] == oi["iterations"][r] + 1          # the first step is taken, the re-evaluation fails the component
        assert st["ref_jacobian_passes_edges"] > int((oi["n_jac_evals"] * ne).sum())
        for f in ("component", "termination", "n_var_nodes", "n_edges"):
            assert np.array_equal(info[f], info8[f]), f
        for f in ("n_converged", "n_failed"):
            assert st[f] == st8[f], f


def _k5_wave(k=None, value=None):
    """Eight 8-row components (the `k5` shape of tests/class_limit_cases.py from eight seeds): one wave of the packed kernel.  With k:
    flow value k of the first match of the fourth one (its edge node1 -> node2) set to `value`.  -> (MatchArrays, that match, batch
    stats, positions, info, oracle result, component of the fourth), computed once per (k, value)"""
    import class_limit_cases as CL
    key = (k, None if value is None else str(value))
    if key not in _wave:
        ma, first = CL.merge([CL.part("k5", CL.SEED + 50 * i) for i in range(8)])
        m = int(np.nonzero(ma.feat1 == first[3])[0][0])
        if k is not None:
            ma.disp2.reshape(-1, 18)[m, k] = value
        p, st, pos, info, ref = run_both(ma, False)
        victim = int(ref["comp"][np.nonzero(ref["node_feat"] == first[3])[0][0]])
        _wave[key] = (ma, m, p, st, pos, info, ref, victim)
    return _wave[key]


@pytest.mark.parametrize("value", [np.inf, np.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("k", range(18))
def test_non_finite_flow_at_every_grid_position(lfr_lib, k, value):
    """include/lfr.h: a flow entry that is not finite fails its component with zero displacements, wherever it sits in the grid.
    Against the oracle: termination and zero positions at all 18 positions; iterations and the batch's evaluation counts equal to the
    oracle's at the ten positions the first evaluation reads and equal among them, one iteration more at the eight corners (the
    contract's text); the seven components that share the wave bitwise what they are without the poison."""
    _, _, p0, st0, pos0, info0, ref0, victim = _k5_wave()
    assert st0["n_failed"] == 0 and st0["n_components"] == 8 and (info0["n_var_nodes"] == 4).all() and (info0["n_edges"] == 20).all()
    ma, m, p, st, pos, info, ref, v = _k5_wave(k, value)
    assert v == victim and not np.isfinite(ma.disp2.reshape(-1, 18)[m, k])
    check_against_oracle(p, st, pos, info, ref)
    comp = p.labels()[2]
    r = int(np.nonzero(info["component"] == victim)[0][0])
    oi = ref["infos"][info["component"]]
    print("flow[%d] = %s: iterations %d (oracle %d), jacobian passes x edges %d (oracle %d), cost passes x edges %d (oracle %d)"
          % (k, value, info["iterations"][r], oi["iterations"][r], st["ref_jacobian_passes_edges"], int((oi["n_jac_evals"] * info["n_edges"]).sum()),
             st["ref_cost_passes_edges"], int((oi["n_cost_evals"] * info["n_edges"]).sum())))
    assert st["n_failed"] == 1 and info["termination"][r] == oi["termination"][r] == capi.TERM_FAILURE
    assert (pos[comp == victim] == 0).all() and (ref["positions"][comp == victim] == 0).all()
    _, _, _, st8, pos8, info8, _, _ = _k5_wave(8, value)
    _check_flow_position(k, st, info, ref, r, st8, info8)
    # the seven neighbours in the wave: bitwise what they were
    assert (pos[comp != victim] == pos0[comp != victim]).all() and pos0[comp != victim].any()
    others = np.arange(8) != r
    for f in ("iterations", "termination"):
        assert np.array_equal(info[f][others], info0[f][others]), f
    assert np.array_equal(info["final_cost"][others].view(np.uint64), info0["final_cost"][others].view(np.uint64))


G16_WAVE = ("k7_first_reread", "k9_full", "k6", "k7_resident_full")      # four components of the 16-row class: one wave
_wave16 = {}


def _g16_wave(victim=None, k=None, value=None):
    """The four shapes of G16_WAVE (tests/class_limit_cases.py).  With victim: flow value k of its LAST match's edge node2 -> node1 set
    to `value` - the packed classes hold their records in edge order, so that is the component's last record, edge 49 of 50 or 95 of 96:
    slot 3 or 5 of the 16-lane group, beyond the three resident slots, re-read from memory by every sweep."""
    import class_limit_cases as CL
    key = (victim, k, None if value is None else str(value))
    if key not in _wave16:
        ma, first = CL.merge([CL.part(n) for n in G16_WAVE])
        feat = first[G16_WAVE.index(victim or G16_WAVE[0])]
        m = int(np.nonzero(ma.feat1 == feat)[0][-1])
        if victim is not None:
            ma.disp1.reshape(-1, 18)[m, k] = value
        p, st, pos, info, ref = run_both(ma, False)
        c = int(ref["comp"][np.nonzero(ref["node_feat"] == feat)[0][0]])
        _wave16[key] = (ma, m, p, st, pos, info, ref, c)
    return _wave16[key]


@pytest.mark.parametrize("value", [np.inf, np.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("k", range(18))
@pytest.mark.parametrize("victim", G16_WAVE[:2])
def test_non_finite_flow_in_a_reread_record(lfr_lib, victim, k, value):
    """the same for a record the packed kernel does not keep in registers but re-reads in every sweep: the oracle's termination and
    zeros at all 18 positions, iterations and evaluation counts as include/lfr.h states them, the three neighbours of the wave bitwise
    unchanged."""
    import class_limit_cases as CL
    _, _, p0, st0, pos0, info0, ref0, _ = _g16_wave()
    assert st0["n_failed"] == 0 and st0["n_components"] == 4
    assert sorted(zip((2 * info0["n_var_nodes"]).tolist(), info0["n_edges"].tolist())) == sorted((CL.SHAPES[n]["rows"], CL.SHAPES[n]["edges"]) for n in G16_WAVE)
    ma, m, p, st, pos, info, ref, c = _g16_wave(victim, k, value)
    check_against_oracle(p, st, pos, info, ref)
    comp = p.labels()[2]
    r = int(np.nonzero(info["component"] == c)[0][0])
    E = CL.SHAPES[victim]["edges"]
    assert info["n_edges"][r] == E and (E - 1) // 16 >= 3          # the last record lies beyond the resident slots
    # (it is the last record: no later match of the graph belongs to the component)
    oi = ref["infos"][info["component"]]
    ne = info["n_edges"].astype(np.int64)
    print("%s flow[%d] = %s: iterations %d (oracle %d), jacobian passes x edges %d (oracle %d), cost passes x edges %d (oracle %d)"
          % (victim, k, value, info["iterations"][r], oi["iterations"][r], st["ref_jacobian_passes_edges"], int((oi["n_jac_evals"] * ne).sum()),
             st["ref_cost_passes_edges"], int((oi["n_cost_evals"] * ne).sum())))
    assert st["n_failed"] == 1 and info["termination"][r] == oi["termination"][r] == capi.TERM_FAILURE
    assert (pos[comp == c] == 0).all() and (ref["positions"][comp == c] == 0).all()
    _, _, _, st8, _, info8, _, _ = _g16_wave(victim, 8, value)
    _check_flow_position(k, st, info, ref, r, st8, info8)
    assert (pos[comp != c] == pos0[comp != c]).all() and pos0[comp != c].any()
    others = np.arange(4) != r
    for f in ("iterations", "termination"):
        assert np.array_equal(info[f][others], info0[f][others]), f
    assert np.array_equal(info["final_cost"][others].view(np.uint64), info0["final_cost"][others].view(np.uint64))
