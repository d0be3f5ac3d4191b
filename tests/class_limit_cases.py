"""Components that sit exactly ON the row and edge limits of the nine launch classes (classify() of lfr_graph.cpp, classify_dev() of
lfr_assemble.hip), one component per named shape.  Not a test: tests/test_class_limit_cases.py checks on the CPU that every shape has
the rows, the edges and the class listed here and that the oracle converges on it away from any rounding-level decision;
tests/test_gpu_class_limits.py runs the kernels on them.

A shape is one track of n nodes with m distinct matches and d duplicated ones: rows = 2 (n - 1) (one root is fixed), directed edges =
2 (m + d).  The m matches are the first m pairs of `pair_order(n)`: the ring (0,1), (1,2) ... (n-2,n-1), (0,n-1) first - its first
n - 1 pairs are a path, so any m >= n - 1 is connected - then the chords by ring distance 2, 3, ...; m = n (n - 1) / 2 is the
complete track, m = n the ring.  The d duplicates repeat the first d matches (the reference keeps duplicates, solve.cc:476-478).
Sigmas are the defaults of `tracks()`: easy problems whose trajectories do not hang on a rounding.

Edge slots of the packed classes (<NV, LPR, EPL> and the limits are the rows of kPackedClass in lfr_internal.hpp, the one statement
of them: S = NV * LPR lanes per group, edge e of a component sits in lane e % S, slot e / S; in the forward solve_group_body the first
RES slots stay in registers, the others are re-read from memory by every sweep):
  8-row class   <8, 1, 3>   S =  8, 3 slots, RES 3: 24 edges, all resident
  16-row class  <16, 1, 6>  S = 16, 6 slots, RES 3: 96 edges, 48 resident - the pair 12/48 and 12/50 of the table
  24-row class  <32, 1, 6>  S = 32, 6 slots, RES 2 (LFR_RES4): 192 edges, 2 x 32 = 64 resident.  A complete track of 10 nodes (the
                smallest above 16 rows) has 90 edges already, so the pair at 64 / 66 edges is sparse: 11 nodes (20 rows),
                m = 32 and m = 33 of the 55 pairs
  32-row class  <32, 2, 5>  S = 64, 5 slots, RES 2: 320 edges, 2 x 64 = 128 resident.  Above 24 rows: 15 nodes (28 rows), m = 64 and
                m = 65 of the 105 pairs give 128 / 130 edges
Every shape of a batch is generated from a random stream of its own (seed + its index in SHAPES), so a shape has the same flows and
similarities, bit for bit, alone, among the others and in a batch that holds every shape twice."""
import dataclasses

import numpy as np

from lfr_amd import synthetic

MAX_BLOCK_ROWS = 192


def pair_order(n, m=None):
    """The first m (None: all n (n - 1) / 2) node pairs (i < j) of a track: ring first, then chords by ring distance, then by first node."""
    total = n * (n - 1) // 2
    m = total if m is None else m
    out = [(i, i + 1) for i in range(n - 1)]
    if n >= 3:
        out.append((0, n - 1))
    for dist in range(2, n // 2 + 1):
        if len(out) >= m:
            break
        for i in range(n if 2 * dist != n else n // 2):
            a, b = i, (i + dist) % n
            out.append((min(a, b), max(a, b)))
    assert len(out) >= m and (len(out) != total or len(set(out)) == total)
    return out[:m]


def _arrays(n_images, i1, i2, f1, f2, sim, disp1, disp2):
    """MatchArrays of matches sorted by image pair.  An image without a match gets an empty pair (0, image) behind the others: the
    size cap of the graph stage is the number of images SEEN, and a pair without matches counts (solve.cc:448-451)."""
    M = len(sim)
    key = i1.astype(np.int64) * n_images + i2
    starts = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0]
    seen = np.zeros(n_images, bool)
    seen[i1] = True
    seen[i2] = True
    unseen = np.nonzero(~seen)[0]
    p1, p2 = np.r_[i1[starts], np.zeros(len(unseen), np.int64)], np.r_[i2[starts], unseen]
    return synthetic.MatchArrays(["%06d.png" % i for i in range(n_images)], np.ones(n_images, np.float32), p1.astype(np.int32),
                                 p2.astype(np.int32), np.r_[starts, [M] * (1 + len(unseen))].astype(np.int64),
                                 np.asarray(f1).astype(np.uint32), np.asarray(f2).astype(np.uint32), sim, disp1, disp2)


def tracks(seed, lengths, dups=(), wrong=(), sigma_p=0.15, sigma_noise=0.02, sigma_A=0.05, n_images=0):
    """MatchArrays of tracks: track t has lengths[t] nodes, node i of every track in image i.  lengths[t] = n: the complete track;
    lengths[t] = (n, m, d): the first m pairs of pair_order(n), the first d of them twice.  dups: (track, n) gives the first n matches
    of the track twice; wrong: (track a, node i, track b, node j), i != j - a match the track stage cannot merge
    (the joined component must not exceed the graph stage's size cap, the number of images: the longest track, or n_images if that
    is more - the images beyond the longest track are seen through pairs without matches)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sizes = [n if np.isscalar(n) else n[0] for n in lengths]
    n_images = max(max(sizes), n_images)
    off = np.r_[0, np.cumsum(sizes)]
    img = np.concatenate([np.arange(n) for n in sizes])
    feat = np.concatenate([np.full(n, t) for t, n in enumerate(sizes)])      # feature index inside an image = track number
    pos = np.clip(rng.normal(0.0, sigma_p, size=(off[-1], 2)), -0.45, 0.45)
    a, b, bad = [], [], []
    for t, n in enumerate(lengths):
        if np.isscalar(n):
            iu, ju = np.triu_indices(n, k=1)
        else:
            n, m, d = n
            assert n - 1 <= m <= n * (n - 1) // 2 and 0 <= d <= m
            pairs = pair_order(n, m)
            pairs += pairs[:d]
            iu, ju = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        a += list(off[t] + iu); b += list(off[t] + ju); bad += [False] * iu.size
        for (td, nd) in dups:
            if td == t:
                a += list(off[t] + iu[:nd]); b += list(off[t] + ju[:nd]); bad += [False] * nd
    for (ta, i, tb, j) in wrong:
        assert i < j
        a.append(off[ta] + i); b.append(off[tb] + j); bad.append(True)
    a, b, bad = np.array(a), np.array(b), np.array(bad)
    M = a.size
    grid = synthetic.GRID.astype(np.float32)

    def flow(src, dst):
        base = np.where(bad[:, None], rng.normal(0.0, 0.3, size=(M, 2)), pos[dst] - pos[src]).astype(np.float32)
        A = rng.standard_normal(size=(M, 2, 2), dtype=np.float32) * np.float32(sigma_A)
        out = rng.standard_normal(size=(M, 9, 2), dtype=np.float32) * np.float32(sigma_noise) + base[:, None, :]
        out += A[:, None, :, 0] * grid[None, :, 0, None]
        out += A[:, None, :, 1] * grid[None, :, 1, None]
        return out

    disp2, disp1 = flow(a, b), flow(b, a)
    sim = rng.uniform(0.8, 1.0, size=M).astype(np.float32)
    i1, i2 = img[a], img[b]
    o = np.lexsort((np.arange(M), i2, i1))
    a, b, i1, i2, sim, disp1, disp2 = a[o], b[o], i1[o], i2[o], sim[o], disp1[o], disp2[o]
    return _arrays(n_images, i1, i2, feat[a], feat[b], sim, disp1, disp2)


def merge(parts):
    """One MatchArrays of several made by tracks(): the features (= track numbers) of part k renumbered behind those of the parts
    before it, images by index, the matches of an image pair in the order of the parts.  Returns (MatchArrays, first feature per part)."""
    n_images = max(len(p.image_names) for p in parts)
    i1 = np.concatenate([np.repeat(p.pair_img1, np.diff(p.pair_off)) for p in parts]).astype(np.int64)
    i2 = np.concatenate([np.repeat(p.pair_img2, np.diff(p.pair_off)) for p in parts]).astype(np.int64)
    n_feat = [int(max(p.feat1.max(), p.feat2.max())) + 1 for p in parts]
    first = np.r_[0, np.cumsum(n_feat)][:-1]
    f1 = np.concatenate([p.feat1.astype(np.int64) + f for p, f in zip(parts, first)])
    f2 = np.concatenate([p.feat2.astype(np.int64) + f for p, f in zip(parts, first)])
    sim, d1, d2 = (np.concatenate([getattr(p, k) for p in parts]) for k in ("sim", "disp1", "disp2"))
    M = len(sim)
    o = np.lexsort((np.arange(M), i2, i1))
    return _arrays(n_images, i1[o], i2[o], f1[o], f2[o], sim[o], d1[o], d2[o]), first.tolist()


def _complete(n, d=0):
    return (n, n * (n - 1) // 2, d)


# name: (track as (n, m, d), rows, directed edges, class by lm_decision_cases.kernel_class's names)
_PACKED = [
    ("k5", _complete(5), 8, 20, "G8"),
    ("k5_full", _complete(5, 2), 8, 24, "G8"),
    ("k5_edges_over", _complete(5, 3), 8, 26, "G16"),                   # the rows fit the 8-row class, the edges do not
    ("k6", _complete(6), 10, 30, "G16"),
    ("k7_resident_full", _complete(7, 3), 12, 48, "G16"),               # last resident slot full
    ("k7_first_reread", _complete(7, 4), 12, 50, "G16_streamed"),       # first re-read edge
    ("k9_full", _complete(9, 12), 16, 96, "G16_streamed"),
    ("k9_edges_over", _complete(9, 13), 16, 98, "G64_2"),
    ("k10", _complete(10), 18, 90, "G64_2"),
    ("s11_resident_full", (11, 32, 0), 20, 64, "G64_2"),                # 24-row class: two resident slots of 32 lanes full
    ("s11_first_reread", (11, 33, 0), 20, 66, "G64_2"),
    ("k13_full", _complete(13, 18), 24, 192, "G64_2"),
    ("k13_edges_over", _complete(13, 19), 24, 194, "G64_4"),
    ("k14", _complete(14), 26, 182, "G64_4"),
    ("s15_resident_full", (15, 64, 0), 28, 128, "G64_4"),               # 32-row class: two resident slots of 64 lanes full
    ("s15_first_reread", (15, 65, 0), 28, 130, "G64_4"),
    ("k17_full", _complete(17, 24), 32, 320, "G64_4"),
    ("k17_edges_over", _complete(17, 25), 32, 322, "BLOCK_S"),
]
_WORKGROUP = [(18, 34, "BLOCK_S"), (45, 88, "BLOCK_S"), (46, 90, "BLOCK_M"), (66, 130, "BLOCK_M"), (67, 132, "BLOCK_L"),
              (97, 192, "BLOCK_L"), (98, 194, "GLOBAL")]
# two tracks of three nodes (images 0..2 each, so they cannot merge) joined by a wrong match: 6 nodes, 2 roots, 4 variable nodes = 8
# rows exactly with n_nodes = n_var + 2; 3 + 3 + 1 matches
TWO_ROOTS = "two_roots_8"
TWO_ROOTS_TRACKS = dict(lengths=[3, 3], wrong=[(0, 0, 1, 2)], n_images=6)          # (six images: the size cap holds the six nodes)

SHAPES = {name: dict(track=t, rows=r, edges=e, cls=c, n_nodes=t[0]) for name, t, r, e, c in _PACKED}
for _n, _r, _c in _WORKGROUP:
    SHAPES["ring%d" % _n] = dict(track=(_n, _n, 0), rows=_r, edges=2 * _n, cls=_c, n_nodes=_n)
    SHAPES["k%d" % _n] = dict(track=_complete(_n), rows=_r, edges=_n * (_n - 1), cls=_c, n_nodes=_n)
SHAPES[TWO_ROOTS] = dict(track=None, rows=8, edges=14, cls="G8", n_nodes=6)
NAMES = list(SHAPES)
TREE = ["ring98", "k98"]                      # the two smallest components of the elimination-tree kernel
THIN_PLAN = {"ring98": True, "k98": False}    # whether the plan runs on dependency counters (lm_decision_cases.THIN_PLAN)
# class name -> slot of lfr_batch_timing's class_edges (KernelClass of lfr_internal.hpp; slot 2 is the retired KC_G32)
CLASS_SLOT = {"G8": 0, "G16": 1, "G16_streamed": 1, "G64_2": 3, "G64_4": 4, "BLOCK_S": 5, "BLOCK_M": 6, "BLOCK_L": 7, "GLOBAL": 8}

SEED = 7100            # shape k of SHAPES is drawn from seed SEED + k
SEED_SECOND = 7300     # another draw of the same structure: the new inputs of the set_inputs test
# a shape found rounding-sensitive at its seed (tests/test_class_limit_cases.py) gets another one here; none is left out
SEED_OVERRIDE = {}


def part(name, seed=SEED):
    s = SEED_OVERRIDE.get((name, seed), seed + NAMES.index(name))
    if name == TWO_ROOTS:
        return tracks(s, **TWO_ROOTS_TRACKS)
    return tracks(s, [SHAPES[name]["track"]])


_parts = {}


def _part(name, seed):
    if (name, seed) not in _parts:
        _parts[(name, seed)] = part(name, seed)
    return _parts[(name, seed)]


def batch(names, seed=SEED):
    """(MatchArrays, {position in `names`: features of that shape's nodes}) of the named shapes in one graph."""
    parts = [_part(n, seed) for n in names]
    ma, first = merge(parts)
    n_feat = [2 if n == TWO_ROOTS else 1 for n in names]
    return ma, [list(range(f, f + k)) for f, k in zip(first, n_feat)]


def all_shapes(seed=SEED):
    """ALL: every shape in one graph -> (MatchArrays, {name: features})."""
    ma, feats = batch(NAMES, seed)
    return ma, dict(zip(NAMES, feats))


def alone(name, seed=SEED):
    """ALONE[name]: one graph per shape (its feature(s): 0, and 1 for the two-track shape)."""
    return batch([name], seed)[0]


def all_twice(seed=SEED):
    """Every shape twice in one graph: other wave neighbours and group positions -> (MatchArrays, [{name: features}] * 2)."""
    ma, feats = batch(NAMES + NAMES, seed)
    return ma, [dict(zip(NAMES, feats[:len(NAMES)])), dict(zip(NAMES, feats[len(NAMES):]))]


def second_inputs():
    """ALL with the flows of another seed and HALF the similarities of the first: scaling every similarity by 0.5 is exact and keeps
    their order, ties and the graph stage's sums, so tracks, roots and components - the structure lfr_batch_set_inputs holds fixed -
    are those of ALL (the CPU test asserts it), which independent similarities of another seed would not promise."""
    ma, _ = all_shapes()
    mb, _ = all_shapes(SEED_SECOND)
    for k in ("pair_img1", "pair_img2", "pair_off", "feat1", "feat2"):
        assert np.array_equal(getattr(ma, k), getattr(mb, k))
    return dataclasses.replace(mb, sim=(0.5 * ma.sim).astype(np.float32))


def components_of(feats, node_feat, comp):
    """{name: component id} from {name: features}: the component that holds the nodes of the shape's features (asserted to be one)."""
    out = {}
    for name, fs in feats.items():
        c = np.unique(comp[np.isin(node_feat, fs)])
        assert len(c) == 1, (name, c)
        out[name] = int(c[0])
    assert len(set(out.values())) == len(out)
    return out
