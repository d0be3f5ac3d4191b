"""Inputs on which the oracle takes the trust-region decisions the plain inputs never reach: rejected LM steps, line searches that
contract (once, and three times or more), coordinates projected onto the bound.  Not a test: tests/test_lm_decision_cases.py checks on
the CPU that every case still reaches what it is here for, tests/test_gpu_lm_decisions.py runs the kernels on them.

Complete tracks are so over-determined that the full LM step is always accepted; every case but `global` is therefore made of SPARSE
tracks (`track_degree=2`: a ring, every node matched to its two neighbours) under steep, noisy flows.  One case per launch class of
the workgroup kernels, one for the 24- and 32-row packed classes:

  packed_24_32   tracks of 10..17 nodes: 18..32 rows, the G64_2 and G64_4 classes (a 9-node ring has 16 rows and 18 edges: the 16-row
                 class, which tests/test_gpu_packed_rounds.py's `hard` batch already covers)
  block_s/m/l    tracks of 18..45 / 46..66 / 67..97 nodes: 34..88 / 90..130 / 132..192 rows, one LDS footprint each
  tree           rings above 192 rows: the elimination-tree kernel on plans that run on dependency counters ("thin" plans)
  global         complete tracks above 192 rows.  There is ONE kernel above 192 rows (solve_tree_component; KC_GLOBAL names the class of
                 the components whose matrices live in the HBM workspace); what a dense component changes is the plan's schedule: too
                 many tiles per column for the counters, so the factorization keeps a barrier per level (lfr_treeplan.cpp, blob[28] =
                 0).  The LM control code is the same as `tree`'s; the case is here for that second schedule.

Every component is one track (no wrong matches), and n_images is at least the longest track, so nothing is cut.

REQUIRED[case] = minimum counts of components (of coordinates for `at_bound`) in the oracle's result:
  rejected     n_successful < iterations - 1
  contracted   n_ls_evals > iterations
  long_search  n_ls_evals - iterations >= 3: `previous` samples and the cubic / quartic interpolants, not only the first quadratic
  at_bound     variable coordinates with |x| == 1.0 exactly
  backward     components with a coordinate at the bound AND a positive-definite reduced Hessian at the oracle's positions (what
               the backward pass can be checked on)
The counts must also hold among the components outside the rounding-sensitive set (see `permuted`), which may hold at most
MAX_SENSITIVE_FRACTION of a case.

Cells not reached: every decision in `global` (UNREACHED below, with the search that was tried).  Every other cell is reached,
`rejected` in `tree` included (one component of twelve).
"""
import numpy as np

from lfr_amd import synthetic

HARD_SIGMAS = dict(sigma_p=0.7, sigma_noise=0.3, sigma_A=0.8)          # tests/test_gpu_packed_rounds.py's HARD
MAX_SENSITIVE_FRACTION = 0.05
MAX_BLOCK_ROWS = 192


def _rings(seed, n_tracks, lo, hi, **kw):
    return dict(seed=seed, n_images=hi, n_tracks=n_tracks, len_dist="uniform", len_lo=lo, len_hi=hi, track_degree=2, **HARD_SIGMAS, **kw)


CASES = {
    "packed_24_32": _rings(204, 80, 10, 17),
    "block_s": _rings(204, 40, 18, 45),
    "block_m": _rings(203, 40, 46, 66),
    "block_l": _rings(202, 40, 67, 97),
    "tree": _rings(202, 12, 98, 160),
    "global": dict(seed=0, n_images=120, n_tracks=6, len_dist="uniform", len_lo=100, len_hi=120, **HARD_SIGMAS),
}
# the classes (kernel_class below) a case's components must lie in; every one of them must occur
CLASSES = {"packed_24_32": {"G64_2", "G64_4"}, "block_s": {"BLOCK_S"}, "block_m": {"BLOCK_M"}, "block_l": {"BLOCK_L"},
           "tree": {"GLOBAL"}, "global": {"GLOBAL"}}
# cases above 192 rows: whether every component's elimination-tree plan runs on dependency counters (word 28 of the plan)
THIN_PLAN = {"tree": True, "global": False}
# Minimum counts.  What the oracle reaches at these seeds (no component is rounding-sensitive in any case):
#   case           components  rejected  contracted  long_search  at_bound
#   packed_24_32       80         10         44          36          52
#   block_s            40          4         28          23          64
#   block_m            40          4         34          30         114
#   block_l            40          2         40          35         151
#   tree               12          1         12          12          60
#   global              6          0          0           0           0
REQUIRED = {
    "packed_24_32": dict(rejected=5, contracted=20, long_search=10, at_bound=20, backward=5),
    "block_s": dict(rejected=2, contracted=15, long_search=10, at_bound=20),
    "block_m": dict(rejected=2, contracted=15, long_search=10, at_bound=20, backward=5),
    "block_l": dict(rejected=1, contracted=15, long_search=10, at_bound=20),
    "tree": dict(rejected=1, contracted=6, long_search=6, at_bound=20),
    "global": dict(),
}
# Cells no input reached.  `global`: 200 seeds (0..199) of six complete tracks of 100..120 nodes at each of the three levels
# (sigma_noise, sigma_A) = (0.3, 0.8), (0.6, 1.5), (1.0, 3.0) with sigma_p = 0.7: 600 oracle runs, 3600 components, not one rejected
# step, contraction or coordinate at the bound.  Ring lattices of 100..120 nodes were tried as well: up to degree 8 they reach
# decisions but their plans are thin (that is the `tree` case), from degree 32 on the plans keep the barrier schedule and every
# decision is gone again (degree 16: some of each, no decision).
UNREACHED = {"global": ("rejected", "contracted", "long_search", "at_bound")}


def kernel_class(rows, edges):
    """The launch class of a component of `rows` = 2 x variable nodes and `edges` directed edges (lfr_graph.cpp's classify)."""
    r, e = int(rows), int(edges)
    return ("G8" if r <= 8 and e <= 24 else "G16" if r <= 16 and e <= 48 else "G16_streamed" if r <= 16 and e <= 96 else
            "G64_2" if r <= 24 and e <= 192 else "G64_4" if r <= 32 and e <= 320 else "BLOCK_S" if r <= 88 else
            "BLOCK_M" if r <= 130 else "BLOCK_L" if r <= MAX_BLOCK_ROWS else "GLOBAL")


def generate(name):
    return synthetic.generate(**CASES[name])


def permuted(ma):
    """The same match graph with the matches of every image pair in reversed order and the pairs in reversed order: the same problem,
    summed in another order by the oracle.  A component whose iterations, termination or n_ls_evals differ between the oracle's two
    runs sits on a rounding-level decision: the GPU test leaves its trajectory out (never its positions or termination)."""
    P = len(ma.pair_img1)
    off = np.asarray(ma.pair_off, np.int64)
    idx = np.concatenate([np.arange(off[p + 1] - 1, off[p] - 1, -1) for p in range(P - 1, -1, -1)]) if P else np.zeros(0, np.int64)
    counts = np.diff(off)[::-1]
    return synthetic.MatchArrays(list(ma.image_names), ma.facts.copy(), ma.pair_img1[::-1].copy(), ma.pair_img2[::-1].copy(),
                                 np.r_[0, np.cumsum(counts)].astype(np.int64), ma.feat1[idx], ma.feat2[idx], ma.sim[idx],
                                 ma.disp1[idx], ma.disp2[idx])


def node_keys(ma, ref):
    """(image index of `ma`) << 32 | feature of the oracle's nodes: a name for a node that does not depend on the input's order"""
    idx = {n: i for i, n in enumerate(ma.image_names)}
    img = np.array([idx[n] for n in ref["image_names"]], np.int64)[ref["node_image"]]
    return img << 32 | ref["node_feat"].astype(np.int64)


def sensitive_components(ma, ref, ref_perm):
    """Component ids (of `ref`) whose trajectory differs between the oracle's runs on `ma` and on permuted(ma).  Asserts that the
    two runs did solve the same problem: the same nodes, roots and components."""
    ka, kb = node_keys(ma, ref), node_keys(ma, ref_perm)
    oa, ob = np.argsort(ka), np.argsort(kb)
    assert (ka[oa] == kb[ob]).all()
    to_b = np.empty(len(ka), np.int64)
    to_b[oa] = ob                                              # node of run a -> the same node in run b
    assert (ref["is_root"] == ref_perm["is_root"][to_b]).all()
    comp_b = ref_perm["comp"][to_b]
    first = {}
    for n, c in enumerate(ref["comp"]):
        first.setdefault(int(c), n)
    out = []
    for c, n in sorted(first.items()):
        cb = int(comp_b[n])
        assert (comp_b[ref["comp"] == c] == cb).all()
        if ref["comp_nvar"][c] == 0:
            continue
        a, b = ref["infos"][c], ref_perm["infos"][cb]
        if any(a[k] != b[k] for k in ("iterations", "termination", "n_ls_evals")):
            out.append(c)
    return np.array(out, np.int64)


_reference = {}


def reference(name):
    """(MatchArrays, oracle result, ids of the rounding-sensitive components) of a case: computed once, shared, left unchanged"""
    if name not in _reference:
        import lfr_oracle as O
        ma = generate(name)
        ref = O.run(ma, n_threads=4)
        assert ref["rc"] == 0
        ref_perm = O.run(permuted(ma), n_threads=4)
        assert ref_perm["rc"] == 0
        _reference[name] = (ma, ref, sensitive_components(ma, ref, ref_perm))
    return _reference[name]


def bound_mask(positions):
    return np.abs(positions) == 1.0


def decision_counts(ref, leave_out=()):
    """The oracle's decisions over the solved components outside `leave_out`."""
    solved = ref["comp_nvar"] > 0
    solved[np.asarray(leave_out, np.int64)] = False
    oi = ref["infos"][solved]
    it = oi["iterations"]
    keep_node = solved[ref["comp"]]
    return {"rejected": int((oi["n_successful"] < it - 1).sum()),
            "contracted": int((oi["n_ls_evals"] > it).sum()),
            "long_search": int((oi["n_ls_evals"] - it >= 3).sum()),
            "at_bound": int(bound_mask(ref["positions"][keep_node]).sum())}


def components_at_bound(ref):
    """ids of the components with at least one coordinate at the bound"""
    return np.unique(ref["comp"][bound_mask(ref["positions"]).any(axis=1)])


def plan_words(ma, ref, c):
    """(n_var, records) of component c as lfr_debug_tree_plan takes them: words src | (dst | kind << 15) << 16 over the component's
    own numbering (variable nodes first, in node order, the roots behind them), by source node."""
    key = node_keys(ma, ref)
    order = np.argsort(key)
    pi = np.repeat(np.arange(len(ma.pair_img1)), np.diff(ma.pair_off))
    k1 = ma.pair_img1[pi].astype(np.int64) << 32 | ma.feat1.astype(np.int64)
    k2 = ma.pair_img2[pi].astype(np.int64) << 32 | ma.feat2.astype(np.int64)
    n1, n2 = order[np.searchsorted(key[order], k1)], order[np.searchsorted(key[order], k2)]
    m = (ref["comp"][n1] == c) & (ref["comp"][n2] == c)
    src, dst = np.stack([n1[m], n2[m]], 1).reshape(-1), np.stack([n2[m], n1[m]], 1).reshape(-1)
    nodes = np.nonzero(ref["comp"] == c)[0]
    var = nodes[~ref["is_root"][nodes]]
    local = {int(n): i for i, n in enumerate(np.r_[var, nodes[ref["is_root"][nodes]]])}
    s = np.array([local[int(n)] for n in src], np.uint32)
    d = np.array([local[int(n)] for n in dst], np.uint32)
    kind = (ref["track"][src] != ref["track"][dst]).astype(np.uint32)
    w = s | ((d | (kind << 15)) << 16)
    return len(var), w[np.argsort(s, kind="stable")]
