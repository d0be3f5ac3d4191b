"""The CPU reference of the covariance between matched keypoints (tests/match_covariance_ref.py) pinned by a known answer and by its
own algebra, and the exported ABI of the feature.  No GPU."""
import os
import re

import numpy as np
import pytest

import backward_ref as BR
import class_limit_cases as CL
import covariance_ref as CR
import lfr_oracle as O
import match_covariance_ref as MR
from lfr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _components(ma, ref):
    idx = {n: i for i, n in enumerate(ma.image_names)}
    ni = np.array([idx[n] for n in ref["image_names"]], np.int32)[ref["node_image"]]
    return BR.graph_components(ma, ref["track"], ref["is_root"], ref["comp"], ni, ref["node_feat"]), ni


def test_triangle_known_answer():
    ma = MR.triangle()
    ref = O.run(ma)
    assert ref["rc"] == 0 and ref["n_components"] == 1
    comps, ni = _components(ma, ref)
    assert ref["is_root"].tolist() == (ni == 0).tolist() and ref["is_root"].sum() == 1          # a is the root
    assert not ref["positions"].any()                                                             # zero flows: x^ = 0
    (var_nodes, cp), = comps.values()
    assert ni[var_nodes].tolist() == [1, 2]
    A = CR.normal_matrix(CR.problem_of(cp), ref["positions"][var_nodes].reshape(-1))
    A_exact = np.kron(np.array([[3.0, -1.0], [-1.0, 3.0]]), np.eye(2))
    assert np.abs(A - A_exact).max() <= 4 * np.spacing(3.0)         # (sqrt(0.5)^2 rounds)
    inv, cols = MR.inverse_columns(A_exact)
    blocks = CR.node_blocks(inv, range(4))
    tol = 4 * 2.0 ** -64
    assert np.abs(blocks - np.array([[0.375, 0.0, 0.375]] * 2, CR.LD)).max() <= tol
    got = MR.match_reference(cp, inv, cols)
    assert sorted(got) == [0, 1, 2]
    for m, (cross_d, rel_d) in MR.TRIANGLE_WANT.items():
        cross, rel = got[m]
        assert np.abs(cross - cross_d * np.eye(2)).max() <= tol, m
        assert np.abs(rel - np.array([rel_d, 0.0, rel_d])).max() <= tol, m


@pytest.fixture(scope="module")
def shapes():
    ma, _ = CL.batch(["k6", CL.TWO_ROOTS, "s11_first_reread", "ring18"])
    ref = O.run(ma, n_threads=4)
    assert ref["rc"] == 0
    comps, _ = _components(ma, ref)
    assert len(comps) == 4
    out = []
    for c, (var_nodes, cp) in sorted(comps.items()):
        A = CR.normal_matrix(CR.problem_of(cp), ref["positions"][var_nodes].reshape(-1))
        assert CR.is_positive_definite(A)
        out.append((cp, A))
    return out


def test_relative_is_positive_semidefinite_and_the_combination_of_its_blocks(shapes):
    n_root = n_both = 0
    for cp, A in shapes:
        inv, cols = MR.inverse_columns(A)
        blocks = CR.node_blocks(inv, range(A.shape[0]))
        got = MR.match_reference(cp, inv, cols)
        assert sorted(got) == sorted(m for m, _, _ in MR.program_matches(cp))
        for m, s, d in MR.program_matches(cp):
            cross, rel = got[m]
            assert MR.is_psd(rel), (m, rel)
            if s >= 0 and d >= 0:
                want, largest = MR.relative_from_blocks(blocks[s], blocks[d], cross)
                assert np.abs(want - rel).max() <= 4 * 2.0 ** -63 * largest
                # strongly correlated through the root: the difference is far smaller than the sum of the two node blocks
                assert rel[0] < blocks[s][0] + blocks[d][0] and cross[0, 0] > 0
                n_both += 1
            else:
                assert not cross.any() and np.array_equal(rel, blocks[max(s, d)])
                n_root += 1
    assert n_root >= 4 and n_both >= 40


def test_two_constant_ends_are_no_residual_block(shapes):
    cp, _ = [s for s in shapes if s[0].nv == 4 and len(s[0].src) == 14][0]                 # the two-root shape: 6 nodes, 7 matches
    assert len(MR.program_matches(cp)) == 7 - int(((cp.src < 0) & (cp.dst < 0)).sum() // 2)


def test_sampled_columns_give_the_same_matches(shapes):
    cp, A = shapes[-1]                                           # ring18: 34 rows
    full = MR.match_reference(cp, *MR.inverse_columns(A))
    nodes = MR.sample_nodes(cp, np.random.default_rng(1), n_matches=5)
    assert len(nodes) <= 12 and 0 in nodes and cp.nv - 1 in nodes
    part = MR.match_reference(cp, *MR.inverse_columns(A, nodes))
    assert 0 < len(part) < len(full)
    kinf = float(np.linalg.cond(A, np.inf))
    for m, (cross, rel) in part.items():
        for got, want in ((cross, full[m][0]), (rel, full[m][1])):
            assert np.abs(got - want).max() <= 32 * A.shape[0] * kinf * 2.0 ** -64 * float(np.abs(full[m][1]).max() + np.abs(want).max())


def test_every_class_limit_shape_is_positive_definite_at_the_oracles_positions():
    """tests/test_gpu_match_covariance.py compares every named shape: none may fall out as singular (part(name, seed) would replace it)"""
    ma, feats = CL.all_shapes()
    ref = O.run(ma, n_threads=4)
    assert ref["rc"] == 0
    comps, _ = _components(ma, ref)
    cmap = CL.components_of(feats, ref["node_feat"], ref["comp"])
    for name, c in cmap.items():
        var_nodes, cp = comps[c]
        A = CR.normal_matrix(CR.problem_of(cp), ref["positions"][var_nodes].reshape(-1))
        assert A.shape[0] == CL.SHAPES[name]["rows"] and CR.is_positive_definite(A), name


def test_smallest_cap_sized_workload_with_a_component_above_192_rows(lfr_lib):
    from lfr_amd import synthetic

    def largest(n_tracks):
        p = capi.Problem(capi.Graph.from_arrays(synthetic.capsized_sparse(n_tracks=n_tracks, seed=7)))
        _, root, comp = p.labels()
        return 2 * int(np.bincount(comp[~root.astype(bool)]).max())

    assert largest(MR.CAPSIZED_SMALLEST) > 192
    assert all(largest(n) <= 192 for n in range(2, MR.CAPSIZED_SMALLEST))
    assert largest(60) > 400


def test_abi_and_bindings_list_the_match_covariance(lfr_lib):
    assert "lfr_batch_covariance_matches" in capi.EXPORTS and hasattr(lfr_lib, "lfr_batch_covariance_matches")
    assert hasattr(capi.Batch, "covariance_matches")
    from lfr_amd.autograd import Refiner
    assert hasattr(Refiner, "match_covariance")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfr.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+lfr_batch_covariance_matches\s*\(\s*lfr_batch\s*\*\s*b\s*,\s*void\s*\*\s*cov_device\s*,\s*void\s*\*\s*cross_device\s*,"
                     r"\s*void\s*\*\s*rel_device\s*,\s*int\s+flags\s*,\s*void\s*\*\s*hip_stream\s*,\s*lfr_covariance_stats\s*\*\s*stats\s*\)\s*;", text)
