"""The packed kernel's rounds on the smallest batches that reach every path of its prologue, sweeps and post-sweep code: positions and
per-component iterations / termination against the C oracle at test_gpu_parity's tolerance, and two solves of one batch bit for bit.

Shapes (rows = 2 x variable nodes, one root per track is fixed; edges are directed, two per match):
  pairs        2 nodes, 2 edges: 2 rows, every lane of the 8-lane group but two holds absent slots only
  k5           5 nodes, 20 edges: the 8-row class, its last slot (lanes 16..23) partly filled
  k5_dup       5 nodes, 24 edges (two matches given twice): the 8-row class full
  k9           9 nodes, 72 edges: the 16-row class with slots beyond the three resident ones, re-read by every sweep
  k13 / k17    13 nodes, 156 edges / 17 nodes, 272 edges: the 24-row and the 32-row class
  mixed        two tracks joined by a wrong match: inter-track (Tukey) next to intra-track (Cauchy) edges in one wave
  hard         steep, noisy flows far from the origin: components that reject a step or contract it in the line search (see HARD)
The component counts (3 pairs, 5 + 1 of the 8-row class, 3 of the 16-row class) are no multiple of 8 or 4: waves with missing groups.
"""
import numpy as np
import pytest

import lfr_oracle as O
from class_limit_cases import tracks
from lfr_amd import capi, synthetic

pytestmark = pytest.mark.gpu
TOL_UNITS = 6.25e-6          # tests/test_gpu_parity.py

# (on the CPU the oracle converges on all 60 components of this batch, rejects a step in 2 and contracts a step in 4)
HARD = dict(seed=200, n_images=12, n_tracks=60, len_dist="uniform", len_lo=3, len_hi=6, sigma_p=0.7, sigma_noise=0.3, sigma_A=0.8)


# name: (MatchArrays, expected (variable nodes, directed edges) of its components, sorted)
CASES = {
    "pairs": lambda: (tracks(91, [2, 2, 2]), [(1, 2)] * 3),
    "k5": lambda: (tracks(92, [5] * 5), [(4, 20)] * 5),
    "k5_dup": lambda: (tracks(93, [5], dups=[(0, 2)]), [(4, 24)]),
    "k9": lambda: (tracks(94, [9] * 3), [(8, 72)] * 3),
    "k13": lambda: (tracks(95, [13]), [(12, 156)]),
    "k17": lambda: (tracks(96, [17]), [(16, 272)]),
    "mixed": lambda: (tracks(97, [3, 3, 6, 2, 2], wrong=[(0, 0, 1, 2)]), [(1, 2), (1, 2), (3, 12), (5, 30)]),      # (the track stage splits the joined six nodes into three tracks)
    "all_classes": lambda: (tracks(98, [2, 5, 9, 13, 17, 2, 5, 9, 2, 3, 3], dups=[(1, 2)], wrong=[(9, 0, 10, 1)]), None),
    "hard": lambda: (synthetic.generate(**HARD), None),
}
_solved = {}


def solved(name):
    """(batch, positions of the first solve, oracle result), once per case"""
    if name not in _solved:
        ma, shapes = CASES[name]()
        g = capi.Graph.from_arrays(ma)
        p = capi.Problem(g)
        b = capi.Batch(p, 0)
        st = b.solve()
        pos = b.download()
        ref = O.run(ma, n_threads=2)
        assert ref["rc"] == 0 and (ref["comp"] == p.labels()[2]).all()
        _solved[name] = (b, st, pos, ref, shapes)
    return _solved[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_rounds_match_the_oracle(lfr_lib, name):
    b, st, pos, ref, shapes = solved(name)
    info = b.component_info()
    if shapes is not None:
        assert sorted(zip(info["n_var_nodes"].tolist(), info["n_edges"].tolist())) == sorted(shapes)
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


def test_hard_case_leaves_the_plain_path(lfr_lib):
    """the 'hard' batch is there for the rejected steps and line-search contractions: the oracle must have taken some, and the kernel
    must have taken the same ones - its Ceres-equivalent evaluation counts (from the per-component counters of the rounds: line-search
    samples, candidate evaluations, successful steps) against the oracle's, as tests/test_gpu_parity.py compares them"""
    b, st, _, ref, _ = solved("hard")
    oi = ref["infos"]
    assert (oi["termination"] == 0).all()
    assert (oi["n_successful"] < oi["iterations"] - 1).any()          # a rejected step (the last iteration of a solve is never "successful")
    assert (oi["n_ls_evals"] > oi["iterations"]).any()                # a contraction: more line-search samples than iterations
    info = b.component_info()
    oc = oi[info["component"]]
    ne = info["n_edges"].astype(np.int64)
    want_jac, want_cost = int((oc["n_jac_evals"] * ne).sum()), int((oc["n_cost_evals"] * ne).sum())
    print("hard: jacobian passes x edges %d (oracle %d), cost passes x edges %d (oracle %d)"
          % (st["ref_jacobian_passes_edges"], want_jac, st["ref_cost_passes_edges"], want_cost))
    assert st["ref_jacobian_passes_edges"] == pytest.approx(want_jac, rel=1e-3)
    assert st["ref_cost_passes_edges"] == pytest.approx(want_cost, rel=1e-3)
    # the oracle counts two jacobian passes per plain iteration; what the contractions and rejections add must be more than the
    # tolerance of the comparison above, or that comparison would not see them
    plain_jac = 2 * int((oc["iterations"].astype(np.int64) * ne).sum())
    assert want_jac > plain_jac * (1 + 2e-3)
