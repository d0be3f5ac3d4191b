"""The packed kernel on the smallest batches that run the code around its arithmetic: the assembly's block addresses (diagonal
block of a variable source, cross block stored below or transposed above the diagonal, nothing for a fixed end point) and the step's
sums read from every lane of a group, rows beyond the system included - which rely on those rows staying zero for a whole solve.

Batches (tracks are complete: n nodes, n (n - 1) directed edges, 2 (n - 1) rows; one root per track is fixed):
  mixed_rows    three tracks each of 2, 3 and 5 nodes - the 8-row class at 2, 4 and 8 rows with 1, 1 and 3 slot passes; the batch is
                ordered by edges, so the first wave holds five-, three- and two-node groups side by side and the second one group and seven
                empty ones (`have` false); three tracks of 9 and two of 6 nodes - the 16-row class at 16 and 10 rows, 5 and 2 slot passes,
                again a mixed wave and a wave with one group; three tracks of 10 and one of 17 nodes - both 32-row classes, two groups of
                one wave and a wave with an empty half
  partial_wave  three tracks of 3 nodes and one of 6: one wave per class, five of eight and three of four groups empty
  hard          tests/test_gpu_packed_rounds.py's HARD recipe (steep, noisy flows far from the origin): components that reject a step
                and components whose line search contracts, in the 8- and 16-row classes
  non_finite    mixed_rows with +inf at a corner of one flow grid of a five-node track.  The first evaluation (at the origin) does not
                read the corners, so the component's cost turns non-finite at its first trial point, next to finite groups in its wave: what
                a multiplication by a 0 / 1 lane factor in place of a select would turn into NaN for the lanes it should leave out.
                No finite input reaches a non-finite cost (a residual is at most ~1e39, its square far inside fp64), and every
                non-finite one ends its component as include/lfr.h, "Undefined inputs", says: LFR_TERM_FAILURE and zero displacements,
                in the oracle too, which sees the corner one evaluation earlier - hence one iteration less.  The oracle's run itself
                returns 0 and converges on every other component.

Every batch is compared entry by entry with the C oracle: positions at tests/test_gpu_parity.py's tolerance (the one
tests/test_gpu_class_limits.py uses against the same oracle), termination codes and iteration counts.  The oracle's side is checked
without a GPU by the first test."""
import numpy as np
import pytest

import lfr_oracle as O
from class_limit_cases import tracks
from lfr_amd import capi, synthetic
from test_gpu_packed_rounds import HARD
from test_gpu_parity import TOL_UNITS

MIXED = [2, 3, 5] * 3 + [9, 6, 9, 6, 9] + [10, 10, 10, 17]
# (variable nodes, directed edges) of the components, sorted
MIXED_SHAPES = sorted([(n - 1, n * (n - 1)) for n in MIXED])
VICTIM_TRACK, VICTIM_CORNER = 2, 0          # the first five-node track of MIXED; flow value 0 is a corner of the 3 x 3 grid


def _mixed(poison=False):
    ma = tracks(9100, MIXED)
    if poison:
        m = int(np.nonzero(ma.feat1 == VICTIM_TRACK)[0][0])          # (the feature index of a node is its track's number)
        ma.disp2.reshape(-1, 18)[m, VICTIM_CORNER] = np.inf
    return ma


CASES = {
    "mixed_rows": lambda: (_mixed(), MIXED_SHAPES),
    "partial_wave": lambda: (tracks(9101, [3, 3, 3, 6]), [(2, 6)] * 3 + [(5, 30)]),
    "hard": lambda: (synthetic.generate(**HARD), None),
    "non_finite": lambda: (_mixed(poison=True), MIXED_SHAPES),
}
_inputs, _solved = {}, {}


def inputs(name):
    """(MatchArrays, expected shapes, oracle result, component that fails or None): computed once, shared, left unchanged"""
    if name not in _inputs:
        ma, shapes = CASES[name]()
        ref = O.run(ma, n_threads=2)
        victim = None
        if name == "non_finite":
            victim = int(ref["comp"][np.nonzero(ref["node_feat"] == VICTIM_TRACK)[0][0]])
        _inputs[name] = (ma, shapes, ref, victim)
    return _inputs[name]


def solved(name):
    if name not in _solved:
        ma = inputs(name)[0]
        p = capi.Problem(capi.Graph.from_arrays(ma))
        b = capi.Batch(p, 0)
        st = b.solve()
        _solved[name] = (p, b, st, b.download().copy(), b.component_info())
    return _solved[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_terminates_every_component(name):
    """no GPU: the oracle alone runs through, converges on every component but the poisoned one and takes the decisions a case is for"""
    ma, shapes, ref, victim = inputs(name)
    assert ref["rc"] == 0
    oi = ref["infos"][ref["comp_nvar"] > 0]
    ok = np.ones(len(ref["infos"]), bool)
    if victim is not None:
        ok[victim] = False
        assert ref["infos"][victim]["termination"] == capi.TERM_FAILURE and (ref["positions"][ref["comp"] == victim] == 0).all()
    assert (ref["infos"][ok & (ref["comp_nvar"] > 0)]["termination"] == capi.TERM_CONVERGENCE).all()
    if shapes is not None:
        assert int((ref["comp_nvar"] > 0).sum()) == len(shapes)
    if name == "hard":
        assert (oi["n_successful"] < oi["iterations"] - 1).any()          # a rejected step
        assert (oi["n_ls_evals"] > oi["iterations"]).any()                # a line-search contraction


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_batch_matches_the_oracle_entry_by_entry(lfr_lib, name):
    ma, shapes, ref, victim = inputs(name)
    p, b, st, pos, info = solved(name)
    assert (ref["comp"] == p.labels()[2]).all()
    if shapes is not None:
        assert sorted(zip(info["n_var_nodes"].tolist(), info["n_edges"].tolist())) == shapes
    oi = ref["infos"][info["component"]]
    err = np.abs(pos - ref["positions"])
    print("%s: %d components, max |dx| %.3e, iterations %s" % (name, st["n_components"], err.max(), sorted(set(info["iterations"].tolist()))))
    assert not np.isnan(pos).any()
    assert (err <= TOL_UNITS).all(), "max |dx| = %.3e units on %d entries" % (err.max(), (err > TOL_UNITS).sum())
    assert np.array_equal(info["termination"], oi["termination"])
    want = oi["iterations"].copy()
    if victim is not None:
        r = int(np.nonzero(info["component"] == victim)[0][0])
        want[r] += 1                     # include/lfr.h: a non-finite corner is seen one evaluation later than the oracle sees it
        assert info["termination"][r] == capi.TERM_FAILURE and (pos[p.labels()[2] == victim] == 0).all()
    assert np.array_equal(info["iterations"], want)
    assert st["n_failed"] == (0 if victim is None else 1) and st["n_components"] == len(info["component"])
    assert b.spin_timeouts() == 0


@pytest.mark.gpu
def test_poisoned_component_leaves_its_wave_alone(lfr_lib):
    """the groups that share a wave with the non-finite component - and every other component of the batch - are bitwise what they
    are without it"""
    _, _, ref, victim = inputs("non_finite")
    p0, _, _, pos0, info0 = solved("mixed_rows")
    p, _, _, pos, info = solved("non_finite")
    comp = p.labels()[2]
    assert np.array_equal(comp, p0.labels()[2]) and np.array_equal(info["component"], info0["component"])
    keep = comp != victim
    assert np.array_equal(pos[keep].view(np.uint64), pos0[keep].view(np.uint64)) and pos0[keep].any() and pos0[~keep].any()
    others = info["component"] != victim
    for f in ("iterations", "termination"):
        assert np.array_equal(info[f][others], info0[f][others]), f
    assert np.array_equal(info["final_cost"][others].view(np.uint64), info0["final_cost"][others].view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_second_solve_is_bitwise_the_first(lfr_lib, name):
    """a solve leaves nothing behind that the next one reads: the same bits and iteration counts again"""
    _, b, _, pos, info = solved(name)
    b.solve()
    assert np.array_equal(b.download().view(np.uint64), pos.view(np.uint64))
    assert np.array_equal(b.component_info()["iterations"], info["iterations"])
