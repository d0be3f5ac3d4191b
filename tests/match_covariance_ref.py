"""CPU reference of the covariance between matched keypoints (lfr_batch_covariance_matches, include/lfr.h): per match of a component's
program the cross block C_12 = Cov(x_node1, x_node2) and D = Cov(x_node2 - x_node1) = C_11 + C_22 - C_12 - C_12^T, from columns of the
longdouble inverse of tests/covariance_ref.py (inverse_ld up to 48 rows, inverse_refined above).  Test infrastructure."""
import numpy as np

import covariance_ref as CR
from lfr_amd import synthetic

LD = CR.LD
NOT_IN_PROGRAM = (-1.0, 0.0, -1.0)          # `relative` of a match that is no residual block
CAPSIZED_SMALLEST = 21                      # smallest n_tracks of synthetic.capsized_sparse(seed=7) with a component above 192 rows


def triangle():
    """Three images a, b, c with one feature each, zero flows, similarities (a,b) = 1, (a,c) = 1, (b,c) = 0.5: one track whose root is
    a (the largest similarity sum).  Every residual is 0 at x = 0, rho' = 1, so with a fixed A = [[3, -1], [-1, 3]] (x) I:
    C_bb = C_cc = 3/8 I, cross(b,c) = 1/8 I, rel(b,c) = 1/2 I, rel(a,b) = rel(a,c) = 3/8 I, cross of both root matches 0."""
    return synthetic.MatchArrays(image_names=["a", "b", "c"], facts=np.ones(3, np.float32), pair_img1=np.array([0, 0, 1], np.int32),
                                 pair_img2=np.array([1, 2, 2], np.int32), pair_off=np.array([0, 1, 2, 3], np.int64),
                                 feat1=np.zeros(3, np.uint32), feat2=np.zeros(3, np.uint32), sim=np.array([1.0, 1.0, 0.5], np.float32),
                                 disp1=np.zeros((3, 9, 2), np.float32), disp2=np.zeros((3, 9, 2), np.float32))


TRIANGLE_WANT = {      # match (row of the arrays above): (cross diagonal, relative diagonal); every off-diagonal entry is 0
    0: (0.0, 3.0 / 8.0), 1: (0.0, 3.0 / 8.0), 2: (1.0 / 8.0, 1.0 / 2.0)}


def program_matches(cp):
    """[(match, local node1, local node2)] of a backward_ref.Component with graph edge ids: the matches whose direction node1 -> node2
    is a residual block (-1 = a constant end).  An edge between two constant nodes is no residual block."""
    return [(int(e) >> 1, int(s), int(d)) for e, s, d in zip(cp.eids, cp.src, cp.dst) if not (e & 1) and (s >= 0 or d >= 0)]


def sample_nodes(cp, rng, n_matches=23):
    """At most 48 local nodes for the components whose full inverse is out of reach: the first and the last node and the variable ends
    of `n_matches` drawn matches (so that some matches have both their ends' columns)."""
    both = [(s, d) for _, s, d in program_matches(cp) if s >= 0 and d >= 0]
    pick = rng.choice(len(both), size=min(n_matches, len(both)), replace=False)
    nodes = {0, cp.nv - 1}
    for k in pick:
        nodes.update(both[k])
    return sorted(nodes)


def inverse_columns(A, nodes=None):
    """(columns of A^-1 in longdouble, cols): every column (nodes = None; inverse_ld up to 48 rows, inverse_refined above), or the two
    columns of each local node in `nodes` by inverse_refined.  cols = None for "all", as covariance_ref.component_bound takes it."""
    n = A.shape[0]
    if nodes is None:
        return (CR.inverse_ld(A) if n <= 48 else CR.inverse_refined(A, range(n))), None
    cols = [2 * l + p for l in nodes for p in (0, 1)]
    return CR.inverse_refined(A, cols), cols


def match_reference(cp, inv, cols=None):
    """{match: (cross [2, 2], relative [3])} in longdouble for the program's matches whose variable ends all have their columns in
    `inv` (cols as inverse_columns returns them)."""
    n = inv.shape[0]
    pos = {c: k for k, c in enumerate(range(n) if cols is None else cols)}

    def block(i, j):                       # C(2i+p, 2j+q) from the columns of node j
        return np.array([[inv[2 * i + p, pos[2 * j + q]] for q in (0, 1)] for p in (0, 1)], LD)

    out = {}
    for m, s, d in program_matches(cp):
        if any(v >= 0 and 2 * v not in pos for v in (s, d)):
            continue
        if s >= 0 and d >= 0:
            c12 = block(s, d)
            rel = block(s, s) + block(d, d) - c12 - c12.T
        else:
            c12 = np.zeros((2, 2), LD)
            rel = block(max(s, d), max(s, d))
        out[m] = (c12, np.array([rel[0, 0], rel[0, 1], rel[1, 1]], LD))
    return out


def relative_from_blocks(cov1, cov2, cross):
    """D = C_11 + C_22 - C_12 - C_12^T in longdouble from two node rows (C(di,di), C(di,dj), C(dj,dj)) and a cross block [2, 2], and
    the largest term that enters it: (relative [3], largest)."""
    a, b, c = (np.asarray(v, LD) for v in (cov1, cov2, cross))
    rel = np.array([a[0] + b[0] - 2 * c[0, 0], a[1] + b[1] - c[0, 1] - c[1, 0], a[2] + b[2] - 2 * c[1, 1]], LD)
    return rel, float(max(np.abs(a).max(), np.abs(b).max(), np.abs(c).max()))


def is_psd(rel, tol=0.0):
    r = np.asarray(rel, np.float64)
    return bool(r[0] >= -tol and r[2] >= -tol and r[0] * r[2] - r[1] * r[1] >= -tol * max(abs(r[0]), abs(r[2]), 1e-300))
