"""Extended-precision restatement of the objective a solve reports as `final_cost` (include/lfr.h, lfr_batch_component_info; cost.cc and
solve.cc of the reference): numpy np.longdouble (64-bit significand on x86), written from the formulas, calling neither the oracle, nor
the library, nor backward_ref's arithmetic.  Not a test: tests/test_cost_ref.py pins it to the two fp64 evaluators the project has
and measures GAMMA_CPU_MEASURED, tests/test_gpu_final_cost.py holds every kernel's final_cost against it at the kernel's own positions.

  F_c(x) = sum_e 1/2 w_e rho_kind(e)(|r_e|^2),   r_e = x_dst - x_src - f(x_src; phi_e)
over the kept directed edges of component c with at least one variable end (an edge between two constant nodes is not in the reduced
program, solve.cc:131-143 / Ceres: the oracle and the kernels leave it out of the cost); f the biquadratic interpolant of the 3 x 3
flow grid phi_e, its argument clamped to [-0.5, 0.5] per coordinate (cost.cc:13-48); rho Cauchy(0.25) on intra-track edges,
rho(s) = b log(1 + s / b), b = 0.25^2, and Tukey(0.0625) on inter-track edges, rho(s) = k (1 - (1 - min(s, a^2) / a^2)^3) with
k = a^2 / 6 ("ceres1", Ceres <= 1.14) or a^2 / 3 ("ceres2", Ceres >= 2.0).  Flows and similarities are the float32 values of the
input, positions the float64 values handed in, all converted exactly.

The unit of every tolerance.  A first-order forward-error scale of evaluating F_c in fp64, whatever the summation order:
  S_c = sum_e |w_e| (1/2 rho_e + rho'_e |r_e| (|x_dst|_1 + |x_src|_1 + sum_k |b_k phi_k|_1))
(rho' = d rho / d s, b_k the nine basis weights: a relative rounding in each operand of r_e moves the term by at most that), plus
E_c cost_c for the summation of E_c terms.  tol_c = gamma 2^-53 (S_c + E_c cost_c).

What S_c leaves out.  Ceres' CauchyLoss - hence the oracle and the kernels - forms 1 + s / b and takes its logarithm.  The sum lies in
[1, 2) for s < b, where round-to-nearest errs by up to 2^-53; that moves the logarithm by up to 2^-53 / (1 + s / b), rho by up to
b 2^-53 and the term by up to 1/2 |w_e| b 2^-53, however small the residual is.  S_c is proportional to |r_e| and does not cover
this on clean tracks of two or three nodes: on tests/test_gpu_parity.py's seed-78 graph the ORACLE's own final_cost is up to 6.5
units of 2^-53 (S_c + E_c cost_c) from F_c.  `Cost.arg_rounding` is that worst case, the sum over the intra-track edges of
1/2 |w_e| b 2^-53.  tests/test_gpu_final_cost.py holds the kernels to tol_c only on inputs where arg_rounding <= tol_c for every
component (it asserts so, and tests/test_cost_ref.py asserts the same of those inputs without a GPU): the check is restricted to
such inputs, the tolerance is not widened for the others.
"""
import dataclasses

import numpy as np

import backward_ref as BR          # graph_components only: which edges, which ends are constant, which kind (no arithmetic)

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble is no wider than float64 on this platform"
U = LD(2.0) ** -53
CAUCHY_B = LD(0.25) * LD(0.25)
TUKEY_A2 = LD(0.0625) * LD(0.0625)
KIND_INTRA, KIND_INTER = 0, 1

# The largest |fp64 evaluator - longdouble| / (2^-53 (S_c + E_c cost_c)) over every component of tests/test_cost_ref.py's inputs
# (class_limit_cases.all_shapes(), every case of lm_decision_cases.CASES, test_oracle_kat's `outliers` and `bounds` in both Tukey
# variants), the evaluators being backward_ref.Component.cost (torch fp64, log1p) and the C oracle's final_cost (log(1 + s / b) in
# the order of the residual blocks), both at the oracle's positions.  Measured 0.2810, by the C oracle on a 4-row component of
# test_oracle_kat's `outliers` (the same in both variants: its edges are intra-track; the largest of torch is 0.157, on that case
# too; class_limit_cases gives 0.196, the lm_decision_cases 0.087 at most); rounded up to two digits.  test_cost_ref.py prints
# the measurement and fails if it exceeds this constant or falls below half of it.
GAMMA_CPU_MEASURED = 0.29
# The kernels contract to FMA, sum in wave and block trees and use their own logarithm and rsqrt-based corrector:
# a few ulp per term, hence the factor; any defect this is for (a cost of another iterate) is many orders of magnitude above it.
GAMMA_GPU = 8 * GAMMA_CPU_MEASURED

# The two graphs tests/test_gpu_final_cost.py makes for itself (synthetic.generate): tests/test_gpu_parity.py's graph with wrong matches
# (seed 78) cut to 300 tracks, at the flow noise of that file's `noisy` case - at the default noise its clean two-node tracks are
# outside the tolerance's validity, see "What S_c leaves out" - and its `active_bounds` graph cut to 300 tracks.
TUKEY_GRAPH = dict(seed=78, n_images=300, n_tracks=300, eps_out=0.006, sigma_noise=0.25)
BOUNDS_GRAPH = dict(seed=74, n_images=30, n_tracks=300, sigma_p=0.7, sigma_noise=0.15)


@dataclasses.dataclass
class Edges:
    """the reduced program of one component: E edges, src / dst = index of a variable node or -1 (constant node at 0)"""
    nv: int
    src: np.ndarray
    dst: np.ndarray
    w: np.ndarray            # [E] longdouble
    kind: np.ndarray         # [E] KIND_INTRA / KIND_INTER
    flow: np.ndarray         # [E, 9, 2] longdouble: grid point 3 i + j (row i, column j), component
    eids: np.ndarray         # [E] directed edge ids of the graph (2 m: node1 -> node2, 2 m + 1: node2 -> node1)

    def __len__(self):
        return len(self.src)

    def without(self, e):
        k = np.arange(len(self)) != e
        return Edges(self.nv, self.src[k], self.dst[k], self.w[k], self.kind[k], self.flow[k], self.eids[k])


@dataclasses.dataclass
class Cost:
    cost: LD                 # F_c in longdouble
    scale: LD                # S_c
    n_edges: int             # E_c
    terms: np.ndarray        # [E] 1/2 w rho, longdouble
    arg_rounding: float      # worst case of rounding 1 + s / b in fp64 over the intra-track edges (see the module's text)

    @property
    def cost64(self):
        return float(self.cost)

    def tol(self, gamma=None):
        """gamma 2^-53 (S_c + E_c cost_c), gamma = GAMMA_GPU unless given"""
        return float((GAMMA_GPU if gamma is None else gamma) * U * (self.scale + self.n_edges * abs(self.cost)))


def components(ma, track, is_root, comp, node_image, node_feature, which=None):
    """{component id: (variable nodes, Edges)} from the labels of a graph stage, as backward_ref.graph_components derives them
    (node_image: index into ma.image_names)"""
    out = {}
    for c, (var_nodes, cp) in BR.graph_components(ma, np.asarray(track), np.asarray(is_root, bool), np.asarray(comp), np.asarray(node_image),
                                                  np.asarray(node_feature), which=which).items():
        keep = (cp.src >= 0) | (cp.dst >= 0)
        flow = cp.flow.numpy()[keep]
        assert np.array_equal(flow, flow.astype(np.float32))                       # the float32 values the kernels read
        out[c] = (var_nodes, Edges(cp.nv, cp.src[keep], cp.dst[keep], cp.sim.numpy()[keep].astype(LD), cp.kind.numpy()[keep],
                                   flow.astype(LD).reshape(-1, 9, 2), cp.eids[keep]))
    return out


def oracle_components(ma, ref, which=None):
    """the same from a result of lfr_oracle.run (its nodes carry indices into the images it has seen)"""
    idx = {n: i for i, n in enumerate(ma.image_names)}
    img = np.array([idx[n] for n in ref["image_names"]], np.int64)[ref["node_image"]]
    return components(ma, ref["track"], ref["is_root"], ref["comp"], img, ref["node_feat"], which)


def _basis(t):
    t = np.clip(t, LD(-0.5), LD(0.5))
    return np.stack([2 * t * (t - LD(0.5)), -4 * (t - LD(0.5)) * (t + LD(0.5)), 2 * t * (t + LD(0.5))], -1)


def evaluate(ed, x, variant="ceres1"):
    """F_c and S_c of the component at x ([nv, 2] or flat, float64 or longdouble)"""
    assert variant in ("ceres1", "ceres2")
    x = np.asarray(x).astype(LD).reshape(-1, 2)
    assert len(x) == ed.nv
    xe = np.concatenate([x, np.zeros((1, 2), LD)])                                 # index -1: the constant node
    xs, xd = xe[ed.src], xe[ed.dst]
    b = (_basis(xs[:, 0])[:, :, None] * _basis(xs[:, 1])[:, None, :]).reshape(-1, 9)
    bf = b[:, :, None] * ed.flow
    r = xd - xs - bf.sum(1)
    s = (r * r).sum(1)
    k = TUKEY_A2 / (6 if variant == "ceres1" else 3)
    v = 1 - np.minimum(s, TUKEY_A2) / TUKEY_A2
    intra = ed.kind == KIND_INTRA
    rho = np.where(intra, CAUCHY_B * np.log1p(s / CAUCHY_B), k * (1 - v * v * v))
    drho = np.where(intra, 1 / (1 + s / CAUCHY_B), 3 * k / TUKEY_A2 * v * v)
    terms = LD(0.5) * ed.w * rho
    mag = np.abs(xd).sum(1) + np.abs(xs).sum(1) + np.abs(bf).sum((1, 2))
    scale = (np.abs(ed.w) * (LD(0.5) * rho + drho * np.sqrt(s) * mag)).sum()
    return Cost(terms.sum(dtype=LD), scale, len(ed), terms, float(np.abs(ed.w)[intra].sum() * CAUCHY_B / 2 * U))


def at_positions(comps, positions, variant="ceres1"):
    """{component id: Cost} of {id: (variable nodes, Edges)} at positions [n_nodes, 2] of the whole graph"""
    return {c: evaluate(ed, positions[var_nodes], variant) for c, (var_nodes, ed) in comps.items()}
