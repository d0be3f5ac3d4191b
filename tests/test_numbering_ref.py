"""The sort / head-flag / two-prefix-sum numbering of lfr_graph_from_device_arrays (numbering_ref.number_by_sort, the numpy
restatement of csrc/lfr_graphbuild.hip) against a dictionary-based first-appearance numbering: hand-made order cases and random
graphs with long runs.  No GPU."""
import numpy as np
import pytest

import numbering_ref as R


def both(case):
    seen, i1, i2, rows = R.kept_pairs(case["image_names"], case["pair_img1"], case["pair_img2"], case["pair_off"], case["banned"])
    f1, f2 = case["feat1"][rows], case["feat2"][rows]
    return seen, rows, R.number_by_sort(i1, f1, i2, f2), R.number_by_dict(i1, f1, i2, f2)


def assert_same(got, want):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all()


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_hand_made_cases(name):
    seen, rows, got, want = both(R.HAND_CASES[name])
    assert_same(got, want)
    n1, n2, node_image, node_feat = got
    assert len(n1) == len(rows)
    if len(node_image):
        assert node_image.min() >= 0 and node_image.max() < len(seen)
        # first appearance: node ids come up in order, and every image id is first met in order too
        ends = np.stack([n1, n2], 1).ravel()
        first = np.unique(ends, return_index=True)[1]
        assert (np.argsort(first) == np.arange(len(first))).all()


def test_hand_made_cases_say_what_they_claim():
    c = R.HAND_CASES
    seen, n1, n2, node_image, node_feat, rows = R.expected_graph(c["node2_then_node1"])
    assert n2[0] == n1[1]                                   # (b, 5): node2 of match 0, node1 of match 1
    seen, n1, n2, node_image, node_feat, rows = R.expected_graph(c["same_feature_two_images"])
    assert len(set(node_image[node_feat == 3])) == 3        # feature 3 is a node of its own in three images
    seen, n1, n2, node_image, node_feat, rows = R.expected_graph(c["duplicate_matches"])
    assert len(node_image) == 2 and len(n1) == 5
    seen, *_ = R.expected_graph(c["empty_pair"])
    assert seen == ["d.jpg", "a.jpg", "b.jpg", "c.jpg"]     # the empty first pair brings its images
    seen, n1, n2, node_image, node_feat, rows = R.expected_graph(c["feature_0_and_top"])
    assert set(node_feat) == {0, 0xFFFFFFFF} and len(node_feat) == 6
    seen, n1, n2, node_image, node_feat, rows = R.expected_graph(c["image_only_in_banned_pairs"])
    assert seen == ["a.jpg", "c.jpg"] and list(rows) == [1, 3, 4]      # d.jpg only met b.jpg: gone, the ids shift
    seen, n1, n2, node_image, node_feat, rows = R.expected_graph(c["banned_start_middle_end"])
    assert list(rows) == [1, 2, 4]
    seen, n1, n2, node_image, node_feat, rows = R.expected_graph(c["all_pairs_banned"])
    assert seen == [] and len(rows) == 0 and len(node_image) == 0


@pytest.mark.parametrize("n_matches", [0, 1, 2, 255, 256, 257, 4097])
def test_random_graphs_with_long_runs(n_matches):
    for seed in range(3):
        case = R.random_case(1000 * seed + n_matches, n_matches, banned=("img002.png",) if seed == 2 else ())
        seen, rows, got, want = both(case)
        assert_same(got, want)


def test_hub_node_and_wide_features():
    seen, rows, got, want = both(R.hub_case(1500))
    assert_same(got, want)
    assert np.bincount(np.concatenate([got[0], got[1]])).max() == 1501
    case = R.random_case(77, 5000, n_images=40, n_features=2 ** 32)
    seen, rows, got, want = both(case)
    assert_same(got, want)
