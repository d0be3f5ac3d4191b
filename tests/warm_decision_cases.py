"""Inputs AND starts on which tests/warm_ref.py - the reference of lfr_batch_solve_from - takes the trust-region decisions that the
warm-start tests' easy starts never reach: rejected LM steps, line searches that contract (once, and three times or more),
coordinates projected onto the bound during a warm trajectory.  The counterpart of tests/lm_decision_cases.py for the WARM
instantiations of the solve kernels.  Not a test: tests/test_warm_decision_cases.py checks on the CPU that every case still reaches
what it is here for, tests/test_gpu_warm_decisions.py runs the kernels on them.

The match graphs are lm_decision_cases' rings (sparse tracks under steep, noisy flows), one case per launch class of the workgroup
kernels and one for the 24- and 32-row packed classes, plus

  packed_8_16    rings of 3..9 nodes: 4..16 rows and 6..18 directed edges, the G8 (up to 5 nodes) and G16 (6..9 nodes) classes.  A ring
                 never has the 49..96 edges at 16 rows or fewer that make the G16_streamed class, so the set is {G8, G16}.
  global         lm_decision_cases' complete tracks above 192 rows (the barrier schedule of the plan), cut to GLOBAL_TRACKS tracks:
                 warm_ref takes 26 s on three, and the reference runs it twice (`solve_both_orders`).

The start of a case is rng(START_SEED[case]).normal(0, START_SIGMA) per coordinate, with a handful of coordinates put beyond the box
on either side (`start_of`), so that the projection of the start happens on a hard trajectory as well.  The seed is chosen per case
on the CPU so that warm_ref terminates CONVERGENCE on every component; the warm solution is another local minimum than the cold one
(they differ by more than a unit), so a warm kernel cannot pass by reproducing the cold answer.

REQUIRED[case] = minimum counts of components (of coordinates for `at_bound`) in warm_ref's result, with lm_decision_cases' meanings:
  rejected     n_successful < iterations - 1
  contracted   n_ls_evals > iterations
  long_search  n_ls_evals - iterations >= 3
  at_bound     variable coordinates with |x| == 1.0 exactly
The counts must hold among the components outside the rounding-sensitive set (`reference`), which may hold at most
MAX_SENSITIVE_FRACTION of a case.  What warm_ref reaches at these seeds (each minimum is about half of it, and at least 1):

  case          start seed  components  rejected  contracted  long_search  at_bound
  packed_8_16        1          80          4         23          19          25
  packed_24_32       1          80          7         49          41          61
  block_s            1          40          6         35          29          68
  block_m            6          40          5         38          36         142
  block_l            2          40          2         40          37         214
  tree              12          12          2         12          12          77
  global             1           3          0          0           0           0
No component of any case is rounding-sensitive at these seeds.

Cells not reached: see UNREACHED below, with the search that was tried.
"""
import numpy as np

import lfr_ref as R
import lm_decision_cases as LC
import warm_ref as W

START_SIGMA = 0.3
MAX_SENSITIVE_FRACTION = LC.MAX_SENSITIVE_FRACTION          # 0.05, the project's cap: a condition on the inputs
GLOBAL_TRACKS = 3
DECISIONS = ("rejected", "contracted", "long_search", "at_bound")

CASES = {name: LC.CASES[name] for name in ("packed_24_32", "block_s", "block_m", "block_l", "tree")}
CASES["packed_8_16"] = LC._rings(204, 80, 3, 9)
CASES["global"] = dict(LC.CASES["global"], n_tracks=GLOBAL_TRACKS)
CLASSES = dict({name: LC.CLASSES[name] for name in CASES if name in LC.CLASSES}, packed_8_16={"G8", "G16"})
THIN_PLAN = LC.THIN_PLAN
# Seeds 1..13 were run on block_m and block_l, 1..50 on tree; every one of them converges on every component.  Seed 1 rejects a step
# in 1 / 0 / 0 components of block_m / block_l / tree; taken: the seed with the most rejected steps (block_l: the first of two with 2).
# tree: seeds 6, 11, 25 and 37 reject a step in one component, 12 in two, the other 45 in none.
START_SEED = dict(dict.fromkeys(CASES, 1), block_m=6, block_l=2, tree=12)
REQUIRED = {
    "packed_8_16": dict(rejected=2, contracted=11, long_search=9, at_bound=12),
    "packed_24_32": dict(rejected=3, contracted=24, long_search=20, at_bound=30),
    "block_s": dict(rejected=3, contracted=17, long_search=14, at_bound=34),
    "block_m": dict(rejected=2, contracted=19, long_search=18, at_bound=71),
    "block_l": dict(rejected=1, contracted=20, long_search=18, at_bound=107),
    "tree": dict(rejected=1, contracted=6, long_search=6, at_bound=38),
    "global": dict(),
}
# Cells no start reached.  `global`: start seeds 1..5 on the three tracks: every LM step accepted at full length, no coordinate at
# the bound - complete tracks are as over-determined from a start of sigma 0.3 as from the origin (lm_decision_cases.UNREACHED: 600
# inputs from the origin, none reaches a decision).  The case is here for the warm kernel on the plan's barrier schedule.
UNREACHED = {"global": DECISIONS}


def generate(name):
    from lfr_amd import synthetic
    return synthetic.generate(**CASES[name])


def start_of(n_nodes, seed):
    """N(0, START_SIGMA) per coordinate; every 37th node's x at 1.5 and every 41st node's y at -1.5: beyond the box on either side
    (tests/test_gpu_warm_start.py's _bounds_start, sparser and finite)"""
    s = np.random.default_rng(seed).normal(0.0, START_SIGMA, size=(n_nodes, 2))
    s[0::37, 0] = 1.5
    s[5::41, 1] = -1.5
    return s


def labels(ma):
    """lfr_ref's graph stage as warm_ref.components runs it, in the form of the oracle's result (what LC.plan_words reads): image_names,
    node_image, node_feat, track, is_root, comp per node, comp_nvar per component; `key` = lfr_ref.MatchGraph's node keys"""
    g = R.MatchGraph(ma.to_pairs())
    track, n_tracks = R.build_tracks(g)
    is_root = np.array(R.select_roots(g, track, n_tracks), bool)
    comp = np.array(R.split_components(g, track, n_tracks, len(g.images_set))[0], np.int64)
    names = list(dict.fromkeys(k[0] for k in g.node_key))
    index = {n: i for i, n in enumerate(names)}
    nvar = np.bincount(comp[~is_root], minlength=comp.max() + 1)
    nvar[np.bincount(comp) == 1] = 0                                            # (a component of one node is not solved)
    return dict(key=g.node_key, image_names=names, node_image=np.array([index[k[0]] for k in g.node_key], np.int64),
                node_feat=np.array([k[1] for k in g.node_key], np.int64), track=np.array(track, np.int64), is_root=is_root, comp=comp,
                comp_nvar=nvar)


def solve_both_orders(ma, start):
    """warm_ref from `start` ([n_nodes, 2] in the node order of `ma`'s graph) on `ma` and on LC.permuted(ma) - the same problem summed
    in another order, the start carried over node by node through the node keys -> (comps, positions, infos, sensitive): the result
    on `ma` and the ids of the components whose iterations, termination or n_ls_evals differ between the two runs.  Asserts that the
    two runs did solve the same problem: the same nodes, roots and components."""
    comps, n = W.components(ma)
    pos, infos = W.solve_graph(comps, n, start)
    mb = LC.permuted(ma)
    la, lb = labels(ma), labels(mb)
    (key_a, root_a, comp_a), (key_b, root_b, comp_b) = ((l["key"], l["is_root"], l["comp"]) for l in (la, lb))
    assert len(key_a) == len(key_b) == n and len(set(key_a)) == n
    index_b = {k: i for i, k in enumerate(key_b)}
    to_b = np.array([index_b[k] for k in key_a], np.int64)      # node of run a -> the same node in run b
    assert sorted(to_b.tolist()) == list(range(n))
    assert (root_a == root_b[to_b]).all()
    comps_b, n_b = W.components(mb)
    assert n_b == n
    start_b = np.empty((n, 2))
    start_b[to_b] = np.asarray(start, np.float64)
    _, infos_b = W.solve_graph(comps_b, n, start_b)
    sensitive = []
    for c in sorted(comps):
        var_nodes = comps[c][0]
        cb = int(comp_b[to_b[var_nodes[0]]])
        assert (comp_b[to_b[comp_a == c]] == cb).all() and (comp_b == cb).sum() == (comp_a == c).sum()
        assert sorted(to_b[var_nodes].tolist()) == sorted(comps_b[cb][0].tolist())
        if any(infos[c][k] != infos_b[cb][k] for k in ("iterations", "termination", "n_ls_evals")):
            sensitive.append(c)
    return comps, pos, infos, np.array(sensitive, np.int64)


_reference = {}


def reference(name, zero_start=False):
    """(MatchArrays, start, comps, ref_pos, ref_infos, sensitive) of a case - warm_ref.components' {component: (variable nodes,
    Problem)}, warm_ref's positions [n_nodes, 2] and {component: info} from the case's start (zero_start: from the origin, what
    tests/test_gpu_warm_decisions.py's mixed waves need), the ids of the rounding-sensitive components: computed once per process,
    shared, left unchanged"""
    if (name, zero_start) not in _reference:
        ma = generate(name)
        n = len(labels(ma)["key"])
        start = np.zeros((n, 2)) if zero_start else start_of(n, START_SEED[name])
        _reference[name, zero_start] = (ma, start) + solve_both_orders(ma, start)
    return _reference[name, zero_start]


def decision_counts(comps, ref_pos, ref_infos, leave_out=()):
    """warm_ref's decisions over the components outside `leave_out`"""
    out = dict.fromkeys(DECISIONS, 0)
    for c in comps:
        if c in set(np.asarray(leave_out).tolist()):
            continue
        i = ref_infos[c]
        out["rejected"] += i["n_successful"] < i["iterations"] - 1
        out["contracted"] += i["n_ls_evals"] > i["iterations"]
        out["long_search"] += i["n_ls_evals"] - i["iterations"] >= 3
        out["at_bound"] += int(LC.bound_mask(ref_pos[comps[c][0]]).sum())
    return {k: int(v) for k, v in out.items()}
