"""The systems tests/test_gpu_tree_solve.py gives the elimination-tree kernel's LM step solve (lfr_debug_solve_tree), built on the CPU:
structures from the generators of tests/test_tree_plan.py and tests/test_gpu_sparse.py, their plans, matrices with the plans' block
sparsity, and what the plans' words say about the kernel paths they reach.  tests/test_linsolve_ref.py checks all of it without a GPU
(coverage of the paths, and that the float64 CPU emulator meets the bounds the GPU test asserts).  Test infrastructure."""
import numpy as np

import linsolve_ref as R
from lfr_amd import capi, synthetic
from tree_plan_emul import Plan, dense_reference, NONE

RELS = (1e-22, 1e-12, 1e-6, 1e-2, 1.0, 1e8, 1e32, 1e64)     # dd / a_ii, the ladder of tests/test_gpu_linear_solve.py
KWAVES = 8                                                  # waves of the elimination-tree kernel's workgroup (LFR_THREADS_G / 64)


# ---- structures ----
def component_words(ma, rank=0):
    """(n_var, words) of the component with the rank-th most variable nodes of a match graph, through the product's host graph stage:
    variable nodes first (graph order), the track roots (constants) behind them, records by source."""
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g)
    track, root, comp = p.labels()
    img, feat = g.nodes()
    at = {name: i for i, name in enumerate(ma.image_names)}
    img = np.array([at[name] for name in g.image_names()], np.int64)[img]          # (the graph numbers the images in its own order)
    key = img << 32 | feat.astype(np.int64)
    order = np.argsort(key)
    pair = np.repeat(np.arange(len(ma.pair_img1)), np.diff(ma.pair_off))

    def node_of(images, feats):
        k = images.astype(np.int64) << 32 | feats.astype(np.int64)
        i = np.minimum(np.searchsorted(key[order], k), len(key) - 1)
        return order[i], key[order][i] == k                        # (a match the graph did not keep has no nodes)
    (n1, ok1), (n2, ok2) = node_of(ma.pair_img1[pair], ma.feat1), node_of(ma.pair_img2[pair], ma.feat2)
    ids, counts = np.unique(comp[(comp >= 0) & ~root], return_counts=True)
    c = ids[np.argsort(-counts, kind="stable")[rank]]
    nodes = np.nonzero(comp == c)[0]
    nodes = np.r_[nodes[~root[nodes]], nodes[root[nodes]]]
    n_var = int((~root[nodes]).sum())
    local = np.full(len(comp), -1, np.int64)
    local[nodes] = np.arange(len(nodes))
    m = ok1 & ok2 & (comp[n1] == c) & (comp[n2] == c)
    a, b = local[n1[m]], local[n2[m]]
    kind = (track[n1[m]] != track[n2[m]]).astype(np.uint32)
    from test_tree_plan import _words, _by_source
    return n_var, _by_source(_words(a, b, kind))


def structures():
    """name -> (n_var, words).  Fixed seeds: tests/test_linsolve_ref.py asserts what their plans reach."""
    import test_tree_plan as T
    from test_gpu_sparse import _explicit
    out = {}
    out["chain"] = T._chain_of_tracks(200, 5, np.random.default_rng(3))
    out["chain_small"] = T._chain_of_tracks(9, 5, np.random.default_rng(4))                        # fewer columns than waves
    out["random_tree"] = T._random_tree_of_tracks_with_cycles(np.random.default_rng(5))
    out["dense_track"] = T._long_dense_track_with_short_tracks(np.random.default_rng(9))
    out["dense_track_88"] = T._long_dense_track_with_short_tracks(np.random.default_rng(10), L=88)
    out["dense_meta"] = T._dense_meta_graph(np.random.default_rng(11))
    out["dense_meta_40"] = T._dense_meta_graph(np.random.default_rng(12), T=40)
    out["constants"] = T._tracks_linked_only_through_a_constant(np.random.default_rng(13))
    star = [(0, i) for i in range(1, 171)]
    comb = [(200 + i, 201 + i) for i in range(119)] + [(200 + i, 400 + i) for i in range(120)]
    chords = [(700 + i, 701 + i) for i in range(149)] + [(700 + i, 700 + i + 37) for i in range(0, 110, 11)]
    ma = _explicit(900, star + comb + chords, seed=5)
    for rank, name in enumerate(("comb", "star", "chords")):                                       # 240, 170 and 149 variable nodes
        out[name] = component_words(ma, rank)
    out["capsized"] = component_words(synthetic.capsized_sparse(n_tracks=2500, seed=7), 0)
    return out


FAMILY = {"chain": "chain", "chain_small": "chain", "random_tree": "random tree", "dense_track": "dense track", "dense_track_88": "dense track",
          "dense_meta": "dense meta graph", "dense_meta_40": "dense meta graph", "constants": "constants", "comb": "star / comb / chords",
          "star": "star / comb / chords", "chords": "star / comb / chords", "capsized": "cap-sized"}


def plans(structs):
    return {name: Plan(capi.tree_plan(n_var, w)[0]) for name, (n_var, w) in structs.items()}


def coverage(pl):
    """What a plan's words say about the kernel paths it reaches."""
    ns = np.diff(pl.colptr) - 1
    extra = ns - pl.ncarry
    thin = int(pl.blob[28]) != 0
    return dict(thin=thin, ncarry=set(pl.ncarry.tolist()), max_extra=int(extra.max()), n_p1=pl.n_p1,
                x_cnt=set(pl.x_tasks[:, 2].tolist()) if len(pl.x_tasks) else set(), nreal=set(pl.nreal.tolist()),
                max_ne=int(np.diff(pl.col_upd_ptr).max()), n_levels=pl.n_levels, NB=pl.NB, n_pad=pl.n_pad)


# ---- values ----
def jtj(plan, n_var, words, rng):
    """J^T J and J^T r from random 2x2 Jacobian blocks per record (tree_plan_emul.dense_reference), in the plan's padded matrix order."""
    E = len(words)
    J1 = -np.eye(2)[None] - 0.3 * rng.standard_normal((E, 2, 2))
    sq = rng.uniform(0.5, 1.0, E)
    r = rng.standard_normal((E, 2))
    A, g, _ = dense_reference(plan, words, n_var, J1, sq, r)
    return A, g


def system(plan, n_var, words, kind, serial, rng):
    """(A, damp, g) of one SPD test system in padded matrix order; padding rows are zero in all three."""
    real = R.real_rows(plan)
    rel = RELS[serial % len(RELS)]
    A, _ = jtj(plan, n_var, words, rng)
    # nodes that only meet other variable nodes leave J^T J without an anchor: the LM diagonal is what makes such a system definite
    if kind.startswith("graded"):
        span = 10.0 ** int(kind[6:])
        s = np.ones(plan.n_pad)
        sv = np.logspace(-0.5 * np.log10(span), 0.5 * np.log10(span), int(real.sum()))
        rng.shuffle(sv)
        s[real] = sv
        A = s[:, None] * A * s[None, :]
        A = 0.5 * (A + A.T)
        rel = 1e-6
    elif kind == "identity":
        A, rel = np.diag(real.astype(np.float64)), 0.0
    elif kind == "diagonal":
        A = np.diag(np.where(real, 10.0 ** rng.uniform(-3, 3, plan.n_pad), 0.0))
    damp = np.where(real, np.sqrt(rel * np.maximum(np.diag(A), 1e-300)), 0.0)
    g = np.where(real, rng.normal(0, 1, plan.n_pad) * 10.0 ** rng.uniform(-2, 2), 0.0)
    return A, damp, g


KINDS = ("jtj",) * len(RELS) + ("graded2", "graded6", "graded12", "identity", "diagonal")
KINDS_CAPSIZED = ("jtj", "jtj", "jtj", "graded6", "diagonal")          # (serial 0, 1, 2: rel 1e-22, 1e-12, 1e-6)


def corpus(structs, pls):
    """[(structure, kind, (A, damp, g))] over every structure, seeds fixed."""
    out = []
    for si, (name, (n_var, w)) in enumerate(structs.items()):
        rng = np.random.default_rng(5100 + si)
        for serial, kind in enumerate(KINDS_CAPSIZED if name == "capsized" else KINDS):
            out.append((name, kind, system(pls[name], n_var, w, kind, serial, rng)))
    return out


# ---- systems that are not positive definite ----
def _ldl(M, real):
    """L, d of the real rows' L D L^T without pivoting, in matrix order - an elimination order of the plan (a column's rows are its
    ancestors, which lie behind it) - scattered back to padded indices."""
    idx = np.nonzero(real)[0]
    W = M[np.ix_(idx, idx)].copy()
    n = len(idx)
    L = np.eye(n)
    d = np.zeros(n)
    for k in range(n):
        d[k] = W[k, k]
        L[k + 1:, k] = W[k + 1:, k] / d[k]
        W[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], W[k, k + 1:])
    return idx, L, d


def bad_pivot_cases(structs, pls):
    """[(structure, where, row, (A, damp, g))]: an SPD system of the structure whose pivot at one matrix row is made negative or
    zero by lowering that row's diagonal entry (pivots of rows that do not depend on it stay as they are).
      first_level / root / half_filled: a row of a level-0 column, of the last level's column, of a block with padding rows;
      through_tile (plans with tiles their columns do not carry): row k of a block K = rowsof[t] of such a tile t = (K, J).  The
      diagonal is lowered by d_k + c / 2, c = sum_{j in J} l_kj^2 d_j the share of pivot k that arrives through tile t: the pivot is
      -c / 2 when the tile task / the finishing of t and its extra-row substitution did their work, and +c / 2 without them."""
    out = []
    for si, name in enumerate(("random_tree", "dense_track", "dense_meta_40", "dense_track_88", "comb", "chain")):
        n_var, w = structs[name]
        pl = pls[name]
        rng = np.random.default_rng(5300 + si)
        A, damp, g = system(pl, n_var, w, "jtj", 3, rng)
        real = R.real_rows(pl)
        M = R.damped(A, damp, "tree")
        idx, L, d = _ldl(M, real)
        assert (d > 0).all()
        at = {int(r): i for i, r in enumerate(idx)}
        lvl = np.zeros(pl.NB, np.int64)
        for l in range(pl.n_levels):
            lvl[pl.level_cols[pl.level_ptr[l]:pl.level_ptr[l + 1]]] = l
        first = int(pl.level_cols[0])
        root = int(pl.level_cols[-1])
        half = [J for J in range(pl.NB) if pl.nreal[J] < 8]
        picks = [("first_level", 16 * first, None), ("root", 16 * root + 2 * int(pl.nreal[root]) - 1, None)]
        if half:
            J = half[len(half) // 2]
            picks.append(("half_filled", 16 * J + 2 * int(pl.nreal[J]) - 1, None))
        share = lambda k, J: float(np.sum(L[k, [at[c] for c in range(16 * J, 16 * J + 16) if c in at]] ** 2 * d[[at[c] for c in range(16 * J, 16 * J + 16) if c in at]]))
        for J in range(pl.NB):
            ns = int(pl.colptr[J + 1] - pl.colptr[J] - 1)
            if ns > pl.ncarry[J]:
                K = int(pl.rowsof[pl.colptr[J] + ns])              # the last tile of the column: never carried
                rows = [r for r in range(16 * K, 16 * K + 2 * int(pl.nreal[K])) if share(at[r], J) > 1e-3 * d[at[r]]]
                if rows:
                    picks.append(("through_tile", rows[0], J))
                    break
        for where, row, J in picks:
            k = at[row]
            B = A.copy()
            if where == "first_level" and si % 2:                 # a zero pivot: row and column zero
                B[row, :] = 0.0
                B[:, row] = 0.0
                dm = damp.copy()
                dm[row] = 0.0
                out.append((name, where + "_zero", row, (B, dm, g)))
                continue
            drop = 2.0 * d[k]
            if J is not None:
                c = share(k, J)
                drop = d[k] + 0.5 * c
            B[row, row] -= drop
            out.append((name, where, row, (B, damp, g)))
    return out


# ---- the criteria (those of the workgroup solvers in tests/test_gpu_linear_solve.py, n = n_pad) ----
def reference(plan, sysm):
    """(M, g, y_ref, forward bound) over the real rows of one system: M as the kernel forms it, y_ref in longdouble."""
    A, damp, g = sysm
    real = R.real_rows(plan)
    M = R.damped(A, damp, "tree")[np.ix_(real, real)]
    gr = g[real]
    y_ref = R.solve_ref(M, gr)
    n = plan.n_pad
    y_lap = np.linalg.solve(M, gr)
    lap = float(np.max(np.abs(y_lap.astype(R.LD) - y_ref)))
    bound = max(16.0 * lap, 4.0 * n * R.U * float(np.linalg.cond(M, np.inf)) * float(np.max(np.abs(y_ref))))
    return M, gr, y_ref, bound


def errors(plan, ref, y):
    """(forward error / its bound, backward error / (8 n_pad u)) of a solution y[n_pad] against reference(plan, system)."""
    M, gr, y_ref, bound = ref
    yr = np.asarray(y, np.float64)[R.real_rows(plan)]
    fe = R.forward_error(yr, y_ref)
    be = R.backward_error(M, yr, gr)
    return (fe / bound if bound > 0 else (0.0 if fe == 0 else np.inf)), be / (8 * plan.n_pad * R.U)


def assert_coverage(pls):
    """The kernel paths the structures must reach, from the plans' words."""
    cov = {name: coverage(pl) for name, pl in pls.items()}
    thin = [c for c in cov.values() if c["thin"]]
    thick = [c for c in cov.values() if not c["thin"]]
    assert thin and thick                                                        # both schedules (blob[28])
    assert set().union(*(c["ncarry"] for c in thin)) == {0, 1, 2, 3} == set().union(*(c["ncarry"] for c in thick))
    assert any(1 <= c["max_extra"] <= 6 and c["n_p1"] > 0 for c in thin)         # tiles finished behind the elimination (finish_extra)
    assert any(c["n_p1"] > 0 for c in thick)                                     # tile tasks of the barrier schedule
    assert {1, 4} <= set().union(*(c["x_cnt"] for c in thick))                   # extra-row tasks of one tile and of four
    for cs in (thin, thick):
        nreal = set().union(*(c["nreal"] for c in cs))
        assert 1 in nreal and any(1 < r < 8 for r in nreal) and 8 in nreal       # half-filled blocks, a one-node block
        assert any(c["max_ne"] > 2 for c in cs)                                  # update entries beyond the two in the descriptor
    assert any(c["n_levels"] == 1 for c in cov.values()) and any(c["n_levels"] >= 6 for c in thin) and any(c["n_levels"] >= 6 for c in thick)
    assert any(c["NB"] < KWAVES for c in cov.values()) and any(c["NB"] >= KWAVES for c in thin) and any(c["NB"] >= KWAVES for c in thick)
    assert cov["capsized"]["thin"] and cov["capsized"]["n_pad"] >= 2000          # a real cap-sized component
    return cov
