"""The node numbering of lfr_graph_from_device_arrays (csrc/lfr_graphbuild.hip) restated in numpy, pass by pass, and a dictionary
reference for it: the algorithm is pinned where no GPU is needed (test_numbering_ref.py), and the hand-made order cases are shared
with the GPU tests (test_gpu_graph_from_device.py).

The graph's rule (solve.cc:444-451, 474-475): pairs that touch a banned image are skipped; images are interned in order of first
appearance over the kept pairs (an empty pair brings its images too); nodes = distinct (image, feature) in order of first appearance,
match by match, node1 before node2.
"""
import numpy as np


def kept_pairs(image_names, pair_img1, pair_img2, pair_off, banned=()):
    """The host part: (seen image names, per graph match: interned image of node1, of node2, caller row)."""
    ban = set(banned)
    seen, index = [], {}

    def intern(i):
        name = image_names[i]
        if name not in index:
            index[name] = len(seen)
            seen.append(name)
        return index[name]

    i1, i2, rows = [], [], []
    for p in range(len(pair_img1)):
        a, b = int(pair_img1[p]), int(pair_img2[p])
        if image_names[a] in ban or image_names[b] in ban:
            continue
        ia, ib = intern(a), intern(b)
        lo, hi = int(pair_off[p]), int(pair_off[p + 1])
        i1 += [ia] * (hi - lo)
        i2 += [ib] * (hi - lo)
        rows += range(lo, hi)
    return seen, np.array(i1, np.int64), np.array(i2, np.int64), np.array(rows, np.int64)


def _exclusive_sum(flags):
    out = np.zeros(len(flags) + 1, np.int64)
    np.cumsum(flags, out=out[1:])
    return out


def number_by_sort(img1, feat1, img2, feat2):
    """(n1, n2, node_image, node_feat) through the device plan: expand -> stable sort by key -> head flags -> two prefix sums ->
    heads -> scatter.  img*: interned image per match; feat*: uint32 feature per match."""
    M = len(feat1)
    E = 2 * M
    if M == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.uint32)
    # 1. expand: entries 2g (node1) and 2g + 1 (node2)
    keys = np.empty(E, np.uint64)
    keys[0::2] = (np.asarray(img1, np.uint64) << np.uint64(32)) | np.asarray(feat1, np.uint64)
    keys[1::2] = (np.asarray(img2, np.uint64) << np.uint64(32)) | np.asarray(feat2, np.uint64)
    pos = np.arange(E, dtype=np.int64)
    # 2. stable sort by key
    order = np.argsort(keys, kind="stable")
    skeys, spos = keys[order], pos[order]
    # 3. head flags and their prefix sums
    run_flag = np.zeros(E + 1, np.int64)
    run_flag[0] = 1
    run_flag[1:E] = skeys[1:] != skeys[:-1]
    pos_flag = np.zeros(E, np.int64)
    pos_flag[spos] = run_flag[:E]
    run_index = _exclusive_sum(run_flag)[:E + 1]       # run_index[E] = N
    pos_rank = _exclusive_sum(pos_flag)[:E]
    N = int(run_index[E])
    # 4. heads, then scatter
    heads = np.nonzero(run_flag[:E])[0]
    run_node = np.full(N, -1, np.int64)
    ids = pos_rank[spos[heads]]
    run_node[run_index[heads]] = ids
    node_image = np.full(N, -1, np.int32)
    node_feat = np.zeros(N, np.uint32)
    node_image[ids] = (skeys[heads] >> np.uint64(32)).astype(np.int32)
    node_feat[ids] = (skeys[heads] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    entry_id = run_node[run_index[:E] + run_flag[:E] - 1]
    ends = np.empty(E, np.uint32)
    ends[spos] = entry_id
    return ends[0::2].copy(), ends[1::2].copy(), node_image, node_feat


def number_by_dict(img1, feat1, img2, feat2):
    """The same four arrays the way the host builds them: one dictionary insert per endpoint, in order."""
    ids, node_image, node_feat = {}, [], []

    def node(im, f):
        k = (int(im), int(f))
        if k not in ids:
            ids[k] = len(node_image)
            node_image.append(k[0])
            node_feat.append(k[1])
        return ids[k]

    n1, n2 = [], []
    for m in range(len(feat1)):
        n1.append(node(img1[m], feat1[m]))      # node1 before node2
        n2.append(node(img2[m], feat2[m]))
    return np.array(n1, np.uint32), np.array(n2, np.uint32), np.array(node_image, np.int32), np.array(node_feat, np.uint32)


def _case(names, pairs, banned=()):
    """pairs: [(image1, image2, [(feat1, feat2), ...]), ...] by image index."""
    p1 = np.array([p[0] for p in pairs], np.int32)
    p2 = np.array([p[1] for p in pairs], np.int32)
    off = np.zeros(len(pairs) + 1, np.int64)
    off[1:] = np.cumsum([len(p[2]) for p in pairs])
    f1 = np.array([m[0] for p in pairs for m in p[2]], np.uint32)
    f2 = np.array([m[1] for p in pairs for m in p[2]], np.uint32)
    return dict(image_names=list(names), pair_img1=p1, pair_img2=p2, pair_off=off, feat1=f1, feat2=f2, banned=tuple(banned))


_ABCD = ["a.jpg", "b.jpg", "c.jpg", "d.jpg"]
_TOP = 0xFFFFFFFF
HAND_CASES = {
    "node2_then_node1": _case(_ABCD, [(0, 1, [(1, 5)]), (1, 2, [(5, 7), (6, 7)]), (2, 0, [(7, 1)])]),
    "same_feature_two_images": _case(_ABCD, [(0, 1, [(3, 3), (4, 3)]), (1, 2, [(3, 3)]), (2, 0, [(3, 4)])]),
    "same_node_several_pairs": _case(_ABCD, [(0, 1, [(1, 2)]), (0, 2, [(1, 9), (8, 9)]), (1, 2, [(2, 9)]), (0, 3, [(1, 1)])]),
    "duplicate_matches": _case(_ABCD, [(0, 1, [(1, 2), (1, 2), (1, 2)]), (1, 0, [(2, 1), (2, 1)])]),
    "empty_pair": _case(_ABCD, [(3, 0, []), (0, 1, [(1, 2)]), (1, 2, []), (2, 0, [(5, 1)]), (2, 3, [])]),
    "feature_0_and_top": _case(_ABCD, [(0, 1, [(0, _TOP), (_TOP, 0)]), (1, 2, [(_TOP, _TOP), (0, 0)]), (2, 0, [(_TOP, 0)])]),
    "image_only_in_banned_pairs": _case(_ABCD, [(1, 3, [(1, 1)]), (0, 2, [(1, 2)]), (3, 1, [(4, 4)]), (2, 0, [(2, 1), (3, 3)])], banned=["b.jpg"]),
    "banned_start_middle_end": _case(_ABCD, [(3, 0, [(9, 9)]), (0, 1, [(1, 2), (3, 4)]), (1, 3, [(2, 2)]), (1, 2, [(2, 5)]), (2, 3, [(5, 6), (7, 8)])],
                                     banned=["d.jpg"]),
    "all_pairs_banned": _case(_ABCD, [(0, 1, [(1, 2)]), (1, 2, [(2, 3)]), (0, 2, [(1, 3)])], banned=["a.jpg", "c.jpg"]),
    "no_pairs": _case(_ABCD, []),
    "no_matches": _case(_ABCD, [(0, 1, []), (1, 2, [])]),
    "one_match": _case(_ABCD, [(0, 1, [(7, 7)])]),
    "two_matches": _case(_ABCD, [(0, 1, [(7, 7)]), (1, 0, [(7, 7)])]),
}


def random_case(seed, n_matches, n_images=6, n_features=5, n_pairs=None, banned=()):
    """Few features: long runs of equal keys.  Pairs of random length (some empty) over random ordered image pairs."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_pairs = n_pairs or max(1, min(n_matches, 2 * n_images))
    cuts = np.sort(rng.integers(0, n_matches + 1, size=n_pairs - 1))
    off = np.concatenate([[0], cuts, [n_matches]]).astype(np.int64)
    p1 = rng.integers(0, n_images, size=n_pairs).astype(np.int32)
    p2 = ((p1 + rng.integers(1, n_images, size=n_pairs)) % n_images).astype(np.int32)
    f1 = rng.integers(0, n_features, size=n_matches).astype(np.uint32)
    f2 = rng.integers(0, n_features, size=n_matches).astype(np.uint32)
    return dict(image_names=["img%03d.png" % i for i in range(n_images)], pair_img1=p1, pair_img2=p2, pair_off=off, feat1=f1, feat2=f2,
                banned=tuple(banned))


def hub_case(degree):
    """One node of degree `degree`: feature 0 of image 0 matched to `degree` features of image 1 (a run that crosses workgroups)."""
    return _case(_ABCD, [(1, 2, [(5, 6)]), (0, 1, [(0, k) for k in range(degree)]), (2, 0, [(6, 0)])])


def expected_graph(case):
    """What the graph must hold for a case: (seen image names, n1, n2, node_image, node_feat, rows), by the dictionary rule."""
    seen, i1, i2, rows = kept_pairs(case["image_names"], case["pair_img1"], case["pair_img2"], case["pair_off"], case["banned"])
    n1, n2, node_image, node_feat = number_by_dict(i1, case["feat1"][rows], i2, case["feat2"][rows])
    return seen, n1, n2, node_image, node_feat, rows
