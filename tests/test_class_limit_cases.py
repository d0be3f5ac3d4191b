"""The shapes of tests/class_limit_cases.py are what their table says, established on the CPU: rows and edges of every component (the
oracle's own counts and the host assembly's), the launch class they give, convergence of the oracle on every one, and no component on
a rounding-level decision.  Without this a change of the builder or of the graph stage could move a shape off its limit and
tests/test_gpu_class_limits.py would go on passing beside the limits instead of on them."""
import numpy as np
import pytest

import class_limit_cases as CL
import lfr_oracle as O
import lm_decision_cases as LC


@pytest.fixture(scope="module")
def all_ref():
    ma, feats = CL.all_shapes()
    ref = O.run(ma, n_threads=4)
    assert ref["rc"] == 0
    return ma, feats, ref, CL.components_of(feats, ref["node_feat"], ref["comp"])


def test_pair_order_is_ring_then_chords():
    for n in (2, 3, 4, 5, 11, 15, 98):
        pairs = CL.pair_order(n)
        assert pairs[:n - 1] == [(i, i + 1) for i in range(n - 1)]          # a path: every prefix from n - 1 on is connected
        if n >= 3:
            assert pairs[n - 1] == (0, n - 1)
        assert sorted(pairs) == [(i, j) for i in range(n) for j in range(i + 1, n)]


def test_table_holds_every_limit():
    """the table itself: both sides of every row / edge limit of classify(), and of every resident / re-read slot boundary"""
    got = {(s["rows"], s["edges"]) for s in CL.SHAPES.values()}
    for rows, edges in ((8, 24), (8, 26), (16, 96), (16, 98), (24, 192), (24, 194), (32, 320), (32, 322),       # edge limits
                        (12, 48), (12, 50), (20, 64), (20, 66), (28, 128), (28, 130)):                          # resident slots
        assert (rows, edges) in got
    rows = {s["rows"] for s in CL.SHAPES.values()}
    assert {8, 10, 16, 18, 24, 26, 32, 34, 88, 90, 130, 132, 192, 194} <= rows
    for s in CL.SHAPES.values():
        assert LC.kernel_class(s["rows"], s["edges"]) == s["cls"]
    assert len(CL.SHAPES) == 18 + 14 + 1


def test_shapes_have_their_rows_edges_and_class(lfr_lib, all_ref):
    from lfr_amd import capi
    ma, feats, ref, comps = all_ref
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g)
    assert (p.labels()[2] == ref["comp"]).all()
    ids, edges = p.shard_components(0, 1)
    host_edges = dict(zip(ids.tolist(), edges.tolist()))
    assert sorted(host_edges) == sorted(comps.values()) == np.nonzero(ref["comp_nvar"] > 0)[0].tolist()
    n_nodes = np.bincount(ref["comp"])
    for name, c in comps.items():
        s = CL.SHAPES[name]
        rows, e = 2 * int(ref["comp_nvar"][c]), int(ref["comp_nedges"][c])
        assert (rows, e, host_edges[c]) == (s["rows"], s["edges"], s["edges"]), name
        assert LC.kernel_class(rows, e) == s["cls"], name
        assert n_nodes[c] == s["n_nodes"], name
        assert n_nodes[c] - ref["comp_nvar"][c] == (2 if name == CL.TWO_ROOTS else 1), name          # roots
    assert p.stats()["n_cut_components"] == 0


def test_oracle_converges_and_no_shape_is_rounding_sensitive(all_ref):
    ma, feats, ref, comps = all_ref
    assert (ref["infos"]["termination"] == 0).all() and (ref["infos"]["iterations"] >= 1).all()
    ref_perm = O.run(LC.permuted(ma), n_threads=4)
    assert ref_perm["rc"] == 0
    assert len(LC.sensitive_components(ma, ref, ref_perm)) == 0          # (a sensitive shape gets another seed: class_limit_cases.SEED_OVERRIDE)


def _shape_positions(ref, feats):
    """{name: positions of the shape's nodes ordered by (image, feature)} of an oracle result"""
    img = np.array([int(n[:6]) for n in ref["image_names"]])[ref["node_image"]]
    out = {}
    for name, fs in feats.items():
        sel = np.nonzero(np.isin(ref["node_feat"], fs))[0]
        out[name] = ref["positions"][sel[np.lexsort((ref["node_feat"][sel], img[sel]))]]
    return out


def test_a_shape_is_the_same_problem_alone_and_in_company(all_ref):
    """ALONE[name] and both copies of the doubled batch hold the component of ALL, bit for bit: the oracle, deterministic and serial
    inside a component, returns identical positions"""
    ma, feats, ref, comps = all_ref
    want = _shape_positions(ref, feats)
    mt, feats2 = CL.all_twice()
    rt = O.run(mt, n_threads=4)
    assert rt["rc"] == 0 and rt["n_components"] == 2 * len(CL.NAMES)
    for f in feats2:
        got = _shape_positions(rt, f)
        for name in CL.NAMES:
            assert np.array_equal(got[name], want[name]), name
    for name in CL.NAMES:
        ra = O.run(CL.alone(name), n_threads=1)
        assert ra["rc"] == 0 and ra["n_components"] == 1, name
        assert 2 * ra["comp_nvar"][0] == CL.SHAPES[name]["rows"] and ra["comp_nedges"][0] == CL.SHAPES[name]["edges"], name
        got = _shape_positions(ra, {name: [0, 1] if name == CL.TWO_ROOTS else [0]})
        assert np.array_equal(got[name], want[name]) and want[name].any(), name


def test_second_inputs_keep_the_structure(all_ref):
    ma, feats, ref, comps = all_ref
    mb = CL.second_inputs()
    rb = O.run(mb, n_threads=4)
    assert rb["rc"] == 0
    for k in ("track", "comp", "is_root", "comp_nvar", "comp_nedges"):
        assert np.array_equal(ref[k], rb[k]), k
    assert (rb["infos"]["termination"] == 0).all()
    assert not np.array_equal(ma.disp1, mb.disp1) and not np.array_equal(ref["positions"], rb["positions"])


@pytest.mark.parametrize("name", CL.TREE)
def test_smallest_tree_components_take_both_schedules(lfr_lib, all_ref, name):
    """194 rows: the ring's plan is thin (it runs on dependency counters), the complete track's is not"""
    from lfr_amd import capi
    ma, feats, ref, comps = all_ref
    n_var, words = LC.plan_words(ma, ref, comps[name])
    assert n_var == 97 and len(words) == CL.SHAPES[name]["edges"]
    blob, _ = capi.tree_plan(n_var, words)
    assert bool(blob[28]) == CL.THIN_PLAN[name]
