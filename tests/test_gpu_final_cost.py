"""The final_cost every solve kernel reports (lfr_batch_component_info) against the objective of tests/cost_ref.py evaluated, in
extended precision, at the positions the same solve wrote; and lfr_solve_stats against the per-component records.

The positions are pinned to the oracle at 6.25e-6 units elsewhere; the last step of a solve - the one after a rejected step, after a
contracted line search, the one the function or parameter tolerance discards - is often smaller than that.  A kernel that stored the
iterate before its last accepted step, reported the cost of a candidate it rejected, or (the elimination-tree kernel swaps pointers on
acceptance) the cost of one buffer next to the positions of the other, passes those tests.  F_c at the returned positions does not
depend on the trajectory and is known to gamma 2^-53 (S_c + E_c cost_c) (tests/cost_ref.py; tests/test_cost_ref.py shows that the
costs of the neighbouring iterates lie 1e7 .. 1e12 such tolerances away).

Inputs: the shapes of tests/class_limit_cases.py (every launch class at its row and edge limits), the cases of
tests/lm_decision_cases.py (rejected steps, contracted searches, the bound; packed 24 / 32, three LDS footprints, both schedules of the
elimination-tree kernel), the `hard` batch of tests/test_gpu_packed_rounds.py (8- and 16-row classes), cuts of tests/test_gpu_parity.py's
graph with wrong matches (both Tukey variants) and of its bounds graph, the NaN victims of tests/test_gpu_undefined_inputs.py.  Every
input lies where the tolerance is valid (cost_ref, "What S_c leaves out"): Checked asserts it, tests/test_cost_ref.py does so without a
GPU.  No component of any input ends NO_CONVERGENCE (the oracle converges on every one; 100 iterations are never reached), so that
termination has no case here."""
import copy

import numpy as np
import pytest

import cost_ref as CR                # (imports torch: before the library is loaded)
import class_limit_cases as CL
import lm_decision_cases as LC
import test_gpu_class_limits as TCL
import test_gpu_lm_decisions as TLM
import test_gpu_packed_rounds as TPR
import test_gpu_undefined_inputs as TUI
from test_gpu_backward import _nodes
from lfr_amd import capi, synthetic

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Checked:
    """one solved batch against cost_ref: per row of component_info the reported cost, F_c at the downloaded positions, F_c(0), and -
    where an oracle result is given - the oracle's record and F_c at the oracle's positions"""

    def __init__(self, ma, g, p, b, pos, variant="ceres1", ref=None, info=None):
        self.info = b.component_info() if info is None else info
        self.comps = CR.components(ma, *p.labels(), *_nodes(g, ma))
        self.ref = ref
        comp = self.info["component"]
        assert sorted(comp.tolist()) == sorted(self.comps)
        self.k = [CR.evaluate(self.comps[c][1], pos[self.comps[c][0]], variant) for c in comp]
        self.k0 = [CR.evaluate(self.comps[c][1], np.zeros((self.comps[c][1].nv, 2)), variant) for c in comp]
        self.ko = None if ref is None else [CR.evaluate(self.comps[c][1], ref["positions"][self.comps[c][0]], variant) for c in comp]
        self.cost = self.info["final_cost"]
        self.err = np.array([abs(float(CR.LD(v) - k.cost)) / k.tol() for v, k in zip(self.cost, self.k)])      # in units of tol_c

    def assert_self_consistent(self, what):
        for i, c in enumerate(self.info["component"]):
            assert self.info["n_var_nodes"][i] == self.comps[c][1].nv and self.info["n_edges"][i] == len(self.comps[c][1]), (what, c)
            assert self.k[i].arg_rounding <= self.k[i].tol(), (what, c)           # the tolerance is valid on this input (cost_ref's text)
            assert np.isfinite(self.cost[i]) and self.err[i] <= 1.0, \
                "%s, component %d: final_cost %.17g, F_c at its positions %.17g, %.3g tol_c" % (what, c, self.cost[i], self.k[i].cost64, self.err[i])
            assert self.cost[i] <= self.k0[i].cost64 + self.k[i].tol(), (what, c)              # LM only accepts decreases, from the origin

    def against_oracle(self):
        """(rows whose iterations and termination equal the oracle's, those of them whose final_cost is NOT the oracle's within
        tol_c(own positions) + tol_c(oracle's) + |F_c(own) - F_c(oracle's)|)"""
        oi = self.ref["infos"][self.info["component"]]
        same = np.nonzero((oi["iterations"] == self.info["iterations"]) & (oi["termination"] == self.info["termination"]))[0]
        bad = [i for i in same if abs(self.cost[i] - oi["final_cost"][i]) >
               self.k[i].tol() + self.ko[i].tol() + abs(float(self.k[i].cost - self.ko[i].cost))]
        return same, bad


def class_limits(device_assembly):
    key = ("cl", device_assembly)
    if key not in _cache:
        s = TCL.all_solved(device_assembly)
        _cache[key] = (s, Checked(s.ma, s.g, s.p, s.b, s.pos, ref=TCL.oracle(), info=s.info))
    return _cache[key]


def lm_case(name):
    if ("lm", name) not in _cache:
        if name == "hard":
            b, st, pos, ref, _ = TPR.solved("hard")
            ma, (p, g) = TPR.CASES["hard"]()[0], (b.problem, b.problem.graph)
        else:
            ma, ref, _ = LC.reference(name)
            g, p, b, st, pos = TLM.solved(name)
        _cache[("lm", name)] = (b, st, ref, Checked(ma, g, p, b, pos, ref=ref))
    return _cache[("lm", name)]


# ------------------------------------------------------------------------------------- 1. every launch class at its limits
@pytest.mark.parametrize("device_assembly", [False, True], ids=["host", "device"])
def test_final_cost_is_the_cost_at_the_positions_on_every_class_limit(lfr_lib, device_assembly):
    s, ch = class_limits(device_assembly)
    assert len(ch.info["component"]) == len(CL.NAMES) and s.st["n_failed"] == 0
    for name in CL.NAMES:
        r, sh = s.row[name], CL.SHAPES[name]
        print("%-18s %-12s %3d rows %5d edges  final_cost %.17g  error %.4f tol_c" % (name, sh["cls"], sh["rows"], sh["edges"], ch.cost[r], ch.err[r]))
        assert (2 * ch.info["n_var_nodes"][r], ch.info["n_edges"][r]) == (sh["rows"], sh["edges"])
    ch.assert_self_consistent("class limits")
    assert s.b.spin_timeouts() == 0


# --------------------------------------------------------------------------------------- 2. where the decisions are hard
@pytest.mark.parametrize("name", sorted(LC.CASES) + ["hard"])
def test_final_cost_is_the_cost_at_the_positions_after_hard_decisions(lfr_lib, name):
    """EVERY component, the rounding-sensitive ones included: the check does not depend on the trajectory.  Reported apart: the
    components that rejected a step (n_successful < iterations - 1 in the oracle) or contracted a line search"""
    b, st, ref, ch = lm_case(name)
    oi = ref["infos"][ch.info["component"]]
    assert (oi["termination"] == capi.TERM_CONVERGENCE).all() and st["n_failed"] == 0 and st["n_no_convergence"] == 0
    rejected = oi["n_successful"] < oi["iterations"] - 1
    contracted = oi["n_ls_evals"] > oi["iterations"]
    classes = sorted({LC.kernel_class(2 * v, e) for v, e in zip(ch.info["n_var_nodes"], ch.info["n_edges"])})
    print("%s (%s): %d components, largest error %.4f tol_c; %d rejected a step: %.4f tol_c; %d contracted a search: %.4f tol_c"
          % (name, " ".join(classes), len(ch.err), ch.err.max(), rejected.sum(), ch.err[rejected].max(initial=0.0), contracted.sum(),
             ch.err[contracted].max(initial=0.0)))
    if name == "hard":
        assert classes == ["G16", "G8"] and rejected.sum() >= 1 and contracted.sum() >= 1
    else:
        assert set(classes) == LC.CLASSES[name]
        assert rejected.sum() >= LC.REQUIRED[name].get("rejected", 0) and contracted.sum() >= LC.REQUIRED[name].get("contracted", 0)
    ch.assert_self_consistent(name)
    assert b.spin_timeouts() == 0


# ------------------------------------------------------------------------------ 3. the oracle's cost where the trajectory is its
def test_final_cost_is_the_oracles_where_the_trajectory_coincides(lfr_lib):
    n = n_same = 0
    for what, ch in [("class limits/host", class_limits(False)[1]), ("class limits/device", class_limits(True)[1])] + \
                    [(name, lm_case(name)[3]) for name in sorted(LC.CASES) + ["hard"]]:
        same, bad = ch.against_oracle()
        oi = ch.ref["infos"][ch.info["component"]]
        print("%s: %d of %d components on the oracle's trajectory, largest |final_cost - oracle's| %.3e" %
              (what, len(same), len(ch.cost), np.abs(ch.cost - oi["final_cost"])[same].max(initial=0.0)))
        assert not bad, (what, [(int(ch.info["component"][i]), ch.cost[i], oi["final_cost"][i]) for i in bad])
        n += len(ch.cost)
        n_same += len(same)
    print("%d of %d components (%.1f %%) qualify" % (n_same, n, 100.0 * n_same / n))
    assert n_same >= (1.0 - LC.MAX_SENSITIVE_FRACTION) * n


# ------------------------------------------------------------------------------------------------- 4. Tukey variants, bounds
def _small(kw, variant):
    ma = synthetic.generate(**kw)
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g)
    b = capi.Batch(p, 0, tukey_variant=variant)
    st = b.solve()
    pos = b.download().copy()
    return b, st, pos, Checked(ma, g, p, b, pos, variant)


def test_final_cost_in_both_tukey_variants(lfr_lib):
    """cost_ref.TUKEY_GRAPH: tests/test_gpu_parity.py's graph with wrong matches (seed 78) cut to 300 tracks, four components with
    inter-track edges, at a flow noise of 0.25 (at the default 0.02 the rounding of 1 + s / b, which S_c leaves out, puts the oracle's
    own final_cost up to 6.5 units from F_c on its clean two-node tracks - tests/cost_ref.py)"""
    kw = CR.TUKEY_GRAPH
    (b1, st1, _, c1), (b2, st2, _, c2) = _small(kw, "ceres1"), _small(kw, "ceres2")
    assert np.array_equal(c1.info["component"], c2.info["component"]) and st1["n_failed"] == st2["n_failed"] == 0
    inter = np.array([(c1.comps[c][1].kind == CR.KIND_INTER).any() for c in c1.info["component"]])
    print("ceres1: largest error %.4f tol_c, ceres2: %.4f tol_c; %d components with inter-track edges, final_cost differs on %d of them"
          % (c1.err.max(), c2.err.max(), inter.sum(), (c1.cost != c2.cost)[inter].sum()))
    c1.assert_self_consistent("ceres1")
    c2.assert_self_consistent("ceres2")
    assert inter.sum() >= 1 and (c1.cost != c2.cost)[inter].any()
    assert np.array_equal(_bits(c1.cost[~inter]), _bits(c2.cost[~inter]))          # (no inter-track edge: the variant changes nothing)


def test_final_cost_with_coordinates_at_the_bound(lfr_lib):
    """cost_ref.BOUNDS_GRAPH: tests/test_gpu_parity.py's `active_bounds` cut to 300 tracks"""
    b, st, pos, ch = _small(CR.BOUNDS_GRAPH, "ceres1")
    at_bound = LC.bound_mask(pos)
    print("bounds: %d coordinates at the bound, largest error %.4f tol_c" % (at_bound.sum(), ch.err.max()))
    assert at_bound.sum() >= 10 and st["n_failed"] == 0
    ch.assert_self_consistent("bounds")


# ------------------------------------------------------------------------------------------------- 5. stats are the records
def _seq_sum(v):
    s = 0.0
    for x in v:                      # (in batch order, one add per component: collect_stats of lfr_batch.hip)
        s += float(x)
    return s


def _assert_stats_are_the_records(st, info, what):
    assert _bits(st["sum_final_cost"]) == _bits(_seq_sum(info["final_cost"])), (what, st["sum_final_cost"], _seq_sum(info["final_cost"]))
    term = info["termination"]
    assert st["n_components"] == len(term), what
    assert st["n_converged"] == int((term == capi.TERM_CONVERGENCE).sum()), what
    assert st["n_no_convergence"] == int((term == capi.TERM_NO_CONVERGENCE).sum()), what
    assert st["n_failed"] == int((term == capi.TERM_FAILURE).sum()), what
    assert st["sum_iterations"] == int(info["iterations"].astype(np.int64).sum()), what
    assert st["n_edges"] == int(info["n_edges"].astype(np.int64).sum()), what


def test_stats_are_the_sums_of_the_records(lfr_lib):
    """sum_final_cost is accumulated in batch order, one add per component (lfr_batch.hip, collect_stats): bit for bit the sequential
    sum of component_info's final_cost"""
    for device_assembly in (False, True):
        s, ch = class_limits(device_assembly)
        _assert_stats_are_the_records(s.st, s.info, "class limits")
        assert s.st["sum_final_cost"] > 0
    for name in sorted(LC.CASES) + ["hard"]:
        b, st, _, ch = lm_case(name)
        _assert_stats_are_the_records(st, ch.info, name)


def test_shards_and_the_multi_device_entry_add_up(lfr_lib):
    s, _ = class_limits(False)
    whole = dict(zip(s.info["component"].tolist(), s.info["final_cost"]))
    bound = len(whole) * U * float(np.abs(s.info["final_cost"]).sum())
    total, seen = 0.0, []
    for r in range(3):
        b = capi.Batch(s.p, 0, shard_rank=r, shard_world=3)
        st = b.solve()
        info = b.component_info()
        _assert_stats_are_the_records(st, info, "shard %d" % r)
        assert np.array_equal(_bits(info["final_cost"]), _bits([whole[c] for c in info["component"].tolist()])), r
        total += st["sum_final_cost"]
        seen += info["component"].tolist()
    assert sorted(seen) == sorted(whole)
    assert abs(total - s.st["sum_final_cost"]) <= bound
    pos, stm = capi.solve_hip_multi(s.p, [0, 0])
    print("sum_final_cost: batch %.17g, three shards %.17g, lfr_solve_hip_multi %.17g (bound %.3e)" % (s.st["sum_final_cost"], total, stm["sum_final_cost"], bound))
    assert abs(stm["sum_final_cost"] - s.st["sum_final_cost"]) <= bound
    for k in ("n_components", "n_edges", "n_converged", "n_no_convergence", "n_failed", "sum_iterations"):
        assert stm[k] == s.st[k], k
    tree = np.isin(np.arange(len(pos)), np.concatenate([s.nodes[n] for n in CL.TREE]))
    assert np.array_equal(_bits(pos[~tree]), _bits(s.pos[~tree])) and np.abs(pos - s.pos).max() <= TCL.TOL_UNITS


# ------------------------------------------------------------------------------------------------------------ 6. FAILURE
def _assert_failure_contract(ma, p, st, info, ref, info0, victim, what):
    """include/lfr.h: a FAILURE component reports the cost of the last iterate it accepted (the start when it accepted none), not
    of the zeros it returns - NaN when that evaluation was not finite, as the oracle's; it is a term of sum_final_cost"""
    r = int(np.nonzero(info["component"] == victim)[0][0])
    oi = ref["infos"][victim]
    print("%s: FAILURE component %d: final_cost %r (oracle %r), iterations %d (oracle %d), sum_final_cost %r"
          % (what, victim, info["final_cost"][r], oi["final_cost"], info["iterations"][r], oi["iterations"], st["sum_final_cost"]))
    assert info["termination"][r] == oi["termination"] == capi.TERM_FAILURE
    assert np.isnan(info["final_cost"][r]) == np.isnan(oi["final_cost"]) and np.isfinite(info["final_cost"][r]) == np.isfinite(oi["final_cost"])
    others = np.arange(len(info["component"])) != r
    assert np.array_equal(info["component"], info0["component"])
    assert np.array_equal(_bits(info["final_cost"][others]), _bits(info0["final_cost"][others]))
    assert np.isfinite(info["final_cost"][others]).all()
    # the failed component is a term of the sum like any other: a NaN cost makes the sum NaN
    assert np.isnan(st["sum_final_cost"]) == np.isnan(info["final_cost"][r])
    if not np.isnan(st["sum_final_cost"]):
        assert _bits(st["sum_final_cost"]) == _bits(_seq_sum(info["final_cost"]))
    assert st["n_failed"] == 1 and st["n_converged"] == int(others.sum())
    return info["final_cost"][r]


def test_failure_reports_the_same_cost_in_every_kernel_family(lfr_lib):
    """a NaN flow value every evaluation reads: one component of the packed kernel (the fourth 8-row component of a wave) and one of
    the workgroup kernel fail; both families and the oracle agree on what final_cost then is (NaN), the neighbours keep their bits.
    Not pinned here: a FAILURE whose cost is finite (ten invalid steps after an accepted one).  That include/lfr.h promises the cost
    of the last accepted iterate for it comes from reading the kernels (the packed phase machine and LmControl::invalid_step leave
    `cost` alone), not from a test: no input of the existing modules fails that way."""
    _, _, p0, st0, _, info0, _, victim = TUI._k5_wave()
    ma, m, p, st, pos, info, ref, v = TUI._k5_wave(8, np.nan)
    assert v == victim and st0["n_failed"] == 0
    packed = _assert_failure_contract(ma, p, st, info, ref, info0, victim, "packed")
    ma0 = synthetic.generate(seed=93, n_images=96, n_tracks=40, len_dist="uniform", len_lo=20, len_hi=70)
    _, st0, _, info0, _ = TUI.run_both(ma0, False)
    ma = copy.deepcopy(ma0)
    ma.disp1[1234, 3, 0] = np.nan
    p, st, pos, info, ref = TUI.run_both(ma, False)
    bad = info["component"][info["termination"] == capi.TERM_FAILURE]
    assert st0["n_failed"] == 0 and bad.size == 1
    r = int(np.nonzero(info["component"] == bad[0])[0][0])
    assert 2 * info["n_var_nodes"][r] > 32                                              # a workgroup class
    block = _assert_failure_contract(ma, p, st, info, ref, info0, int(bad[0]), "workgroup")
    assert np.isnan(packed) == np.isnan(block)
