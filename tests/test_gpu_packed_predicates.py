"""Lane predicates of the packed kernel on the smallest waves at which a wrong one shows: which lanes hold a row (`is_row`, the pivot
tests `row == K` of the elimination, which the kernel evaluates per LM step from an opaque copy of the lane's row), which edge slots of
a lane are present (`sl + S k < E`), which lane of a pair owns which cross entry (`q`, and the row / column selected for the two cross
atomics), and the group-uniform LM flags while other groups of the wave are idle or on another path.  Positions against the C oracle at
test_gpu_parity's tolerance, termination codes and iteration counts exactly, and a second solve bit for bit.

Every case holds at most four components of the 16-row class and at most eight of the 8-row class, so the components of a class share
one wave (a wave64 hosts 4 groups of 16 lanes or 8 groups of 8); every case pins its components' (variable nodes, directed edges).
classify() sends a component of <= 8 rows and <= 24 edges to the 8-row class whatever its neighbours are, so "2 rows next to 16 rows"
and "2 edges next to 96 edges" cannot share a wave: the 2-row / 2-edge pair sits next to the full 8-row component in the 8-row wave,
the 16-row / 96-edge component next to the 10-row / 18-edge one in the 16-row wave, in one batch.

  partial_slot_16   E = 18 (the second slot row holds lanes 0 and 1 only) next to E = 32 (two full slot rows), 10 rows each
  partial_slot_8    E = 10 (second slot row: lanes 0, 1) next to E = 20, in the 8-row class
  limits            16 rows / 96 edges (all six slots, three of them re-read) with 10 rows / 18 edges and 16 rows / 72 edges in the
                    16-row wave; 2 rows / 2 edges (a single match) with 8 rows / 24 edges (the class full) and 4 rows / 4 edges in
                    the 8-row wave
  pair_bit          paths of 2..5 nodes (edges to a fixed root at the path's end: of such a pair of lanes one assembles a source block and
                    the other does not; a path of n nodes puts its n - 1 pairs at lanes 0-1, 2-3, ...: even and odd matches of the
                    slot row) and two 3-node tracks joined by a wrong match (Tukey next to Cauchy edges), one 8-row wave
  cost_only_wave    four rings under steep, noisy flows (lm_decision_cases' HARD_SIGMAS) in ONE 16-row wave, each on the plain path of
                    the oracle (every step accepted at full length): in two of them every cost-only prediction holds, in the other
                    two one prediction fails and the point is evaluated again in full (test_mixed_cost_only_round)
  rejecting_wave    one ring that rejects steps and contracts in the line search (10 iterations, 61 line-search samples) with three
                    rings that stop after 5-6 iterations, in ONE 16-row wave: the three sit idle in lockstep for most of the solve

The rings were picked by solving candidates alone (seeds 9300-9329, 6-9 nodes): the oracle's counters say which path a ring takes,
the executed sweeps of a one-component batch how many predictions failed.
"""
import numpy as np
import pytest

import lfr_oracle as O
from class_limit_cases import merge, tracks
from lm_decision_cases import HARD_SIGMAS
from lfr_amd import capi

pytestmark = pytest.mark.gpu
TOL_UNITS = 6.25e-6          # tests/test_gpu_parity.py


def ring(n, seed):
    """one ring of n nodes (2 (n - 1) rows, 2 n directed edges: the 16-row class from 6 nodes on) under the hard sigmas; a stream of
    its own, so the ring has the same flows alone and merged with others"""
    return tracks(seed, [(n, n, 0)], **HARD_SIGMAS)


# (nodes, seed): predictions of the cost-only round that all hold / of which at least one fails, both on the oracle's plain path
HOLD = [(7, 9307), (9, 9303)]
FAIL = [(8, 9326), (6, 9305)]
REJECTING, IDLE = (9, 9302), [(6, 9314), (7, 9309), (8, 9306)]

# name: (MatchArrays, expected (variable nodes, directed edges) of its components, sorted)
CASES = {
    "partial_slot_16": lambda: (tracks(9101, [(6, 9, 0), (6, 15, 1)]), [(5, 18), (5, 32)]),
    "partial_slot_8": lambda: (tracks(9102, [(4, 5, 0), 5]), [(3, 10), (4, 20)]),
    "limits": lambda: (tracks(9103, [(9, 36, 12), (6, 9, 0), 9, 2, (5, 10, 2), (3, 2, 0)]),
                       [(1, 2), (2, 4), (4, 24), (5, 18), (8, 72), (8, 96)]),
    # (the track stage splits the joined six nodes - two per image - and cuts one match: 3 variable nodes, 12 edges)
    "pair_bit": lambda: (tracks(9104, [2, (3, 2, 0), (4, 3, 0), (5, 4, 0), 3, 3], wrong=[(4, 0, 5, 2)], n_images=6),
                         [(1, 2), (2, 4), (3, 6), (3, 12), (4, 8)]),
    "cost_only_wave": lambda: (merge([ring(*r) for r in HOLD + FAIL])[0], [(n - 1, 2 * n) for n, _ in HOLD + FAIL]),
    "rejecting_wave": lambda: (merge([ring(*r) for r in [REJECTING] + IDLE])[0], [(n - 1, 2 * n) for n, _ in [REJECTING] + IDLE]),
}
_solved = {}


def solve(ma):
    """(batch, stats, positions, oracle result) of one solve"""
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g)
    b = capi.Batch(p, 0)
    st = b.solve()
    pos = b.download()
    ref = O.run(ma, n_threads=2)
    assert ref["rc"] == 0 and (ref["comp"] == p.labels()[2]).all()
    return b, st, pos, ref


def solved(name):
    """(batch, stats, positions of the first solve, oracle result, shapes), once per case"""
    if name not in _solved:
        ma, shapes = CASES[name]()
        _solved[name] = solve(ma) + (shapes,)
    return _solved[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_predicates_match_the_oracle(lfr_lib, name):
    b, st, pos, ref, shapes = solved(name)
    info = b.component_info()
    assert sorted(zip(info["n_var_nodes"].tolist(), info["n_edges"].tolist())) == sorted(shapes)
    # one wave per class: at most four components above 8 rows or 24 edges (none above the 16-row class), at most eight below
    small = (2 * info["n_var_nodes"] <= 8) & (info["n_edges"] <= 24)
    assert (2 * info["n_var_nodes"] <= 16).all() and (info["n_edges"] <= 96).all()
    assert small.sum() <= 8 and (~small).sum() <= 4
    assert st["n_failed"] == 0 and st["n_components"] == len(info["component"]) > 0
    err = np.abs(pos - ref["positions"]).max()
    oi = ref["infos"][info["component"]]
    print("%s: %d components, max |dx| %.3e, iterations %s" % (name, st["n_components"], err, sorted(set(info["iterations"].tolist()))))
    assert err <= TOL_UNITS
    assert (oi["termination"] == info["termination"]).all()
    assert (oi["iterations"] == info["iterations"]).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_second_solve_is_bitwise_the_first(lfr_lib, name):
    b, _, pos, _, _ = solved(name)
    b.solve()
    assert np.array_equal(b.download(), pos)


def _alone(n, seed):
    """(edges, sweeps the kernel executed, the oracle's counters) of a ring solved alone: a one-component batch's `exec_passes_edges` is
    that component's edges x its executed sweeps"""
    _, st, _, ref = solve(ring(n, seed))
    o = ref["infos"][ref["comp_nvar"] > 0]
    assert len(o) == 1 and o[0]["termination"] == 0 and st["exec_passes_edges"] % (2 * n) == 0
    return 2 * n, st["exec_passes_edges"] // (2 * n), o[0]


def test_mixed_cost_only_round(lfr_lib):
    """A group whose cost-only prediction fails repeats the point in full; the kernel counts that extra sweep in its executed passes and
    in no other counter.  On the oracle's plain path (every step accepted at the full length: n_successful = iterations - 1, one
    line-search sample per iteration, so no re-evaluation after a rejection and no candidate sweep) a component executes the first sweep
    and one sweep per iteration, plus one per failed prediction.  Alone, the HOLD rings execute exactly 1 + iterations sweeps and the FAIL
    rings more; together in one wave the four execute what they execute alone, with the oracle's iterations: the failed groups repeat
    their point while the others go on or sit idle, and a wrong group-uniform flag in either direction changes the sum.
    (That a prediction was MADE and held in a HOLD ring is not visible in any counter: a held prediction and none cost one sweep both.)"""
    want = 0
    for kind, rings in (("hold", HOLD), ("fail", FAIL)):
        for n, seed in rings:
            E, sweeps, o = _alone(n, seed)
            assert o["n_successful"] == o["iterations"] - 1 and o["n_ls_evals"] == o["iterations"]          # the plain path
            surplus = sweeps - 1 - int(o["iterations"])
            print("ring %d / %d alone: %d iterations, %d sweeps executed, %d repeated (%s)" % (n, seed, o["iterations"], sweeps, surplus, kind))
            assert surplus == 0 if kind == "hold" else surplus >= 1
            want += E * sweeps
    b, st, _, ref, _ = solved("cost_only_wave")
    info = b.component_info()
    oc = ref["infos"][info["component"]]
    assert (oc["n_successful"] == oc["iterations"] - 1).all() and (oc["n_ls_evals"] == oc["iterations"]).all()
    plain = int(((1 + oc["iterations"].astype(np.int64)) * info["n_edges"]).sum())
    print("cost_only_wave: executed passes x edges %d, alone %d, without a repeated point %d" % (st["exec_passes_edges"], want, plain))
    assert st["exec_passes_edges"] == want > plain


def test_rejecting_group_beside_idle_groups(lfr_lib):
    """the oracle must reject a step and contract a step in exactly one ring of the wave, long after the other three have stopped; the
    kernel's evaluation counts follow the oracle's as in tests/test_gpu_packed_rounds.py"""
    b, st, _, ref, _ = solved("rejecting_wave")
    info = b.component_info()
    oc = ref["infos"][info["component"]]
    assert (oc["termination"] == 0).all()
    hard = (oc["n_successful"] < oc["iterations"] - 1) & (oc["n_ls_evals"] > oc["iterations"])
    assert hard.sum() == 1 and info["n_var_nodes"][hard][0] == REJECTING[0] - 1
    assert (oc["n_ls_evals"][~hard] == oc["iterations"][~hard]).all() and oc["iterations"][~hard].max() < oc["iterations"][hard][0]
    ne = info["n_edges"].astype(np.int64)
    want_jac, want_cost = int((oc["n_jac_evals"] * ne).sum()), int((oc["n_cost_evals"] * ne).sum())
    print("rejecting_wave: jacobian passes x edges %d (oracle %d), cost passes x edges %d (oracle %d)"
          % (st["ref_jacobian_passes_edges"], want_jac, st["ref_cost_passes_edges"], want_cost))
    assert st["ref_jacobian_passes_edges"] == pytest.approx(want_jac, rel=1e-3)
    assert st["ref_cost_passes_edges"] == pytest.approx(want_cost, rel=1e-3)
