"""tests/hessian_product_ref.py pinned without a GPU: its products against the dense matrices of backward_ref.Component.hessian and
backward_gn_ref times the vector, with and without the free set; the measurements behind GAMMA_HVP_CPU / GAMMA_CURV_CPU (the float64
restatement and the dense fp64 product against longdouble, the method of tests/test_evaluate_ref.py); the round trip with the jvp's
linear system behind ROUND_TRIP_REL_CPU; hand-made facts (symmetry, saturated edges, zero vectors, bound rows)."""
import dataclasses

import numpy as np

import backward_gn_ref as GN
import backward_ref as BR
import cost_ref as CR
import evaluate_ref as ER
import hessian_product_ref as HR
import jvp_ref as JR
from test_evaluate_ref import _tukey_at_work, inputs

LD = CR.LD
MODES = [(gn, fs) for gn in (False, True) for fs in (False, True)]


def _component(ed, variant):
    return BR.Component(ed.nv, list(zip(ed.src.tolist(), ed.dst.tolist(), ed.w.astype(np.float64), ed.kind.tolist(),
                                        ed.flow.astype(np.float64).reshape(-1, 18))), variant)


def _dense(cp, x, gn, fs):
    x = np.asarray(x, np.float64).reshape(-1)
    H = GN.Component.of(cp).hessian(x) if gn else cp.hessian(x)
    if fs:
        fr = cp.free(x)
        H[~fr, :] = 0.0
        H[:, ~fr] = 0.0
        H[~fr, ~fr] = 1.0
    return H


def _ratio(err, unit):
    err, unit = np.asarray(err, LD).reshape(-1), np.asarray(unit, LD).reshape(-1)
    assert (err[unit == 0] == 0).all()                       # (zero vector entries, saturated Tukey edges, bound rows: exact)
    return float((err[unit > 0] / unit[unit > 0]).max(initial=0.0))


# ------------------------------------------------------------------------------ 1. the dense matrices and the measured constants
def test_products_agree_with_the_dense_matrices_and_the_gammas_are_as_recorded():
    worst = {"hvp": 0.0, "hvp_dense": 0.0, "curv": 0.0, "curv_dense": 0.0}
    n = n_bound = 0
    for label, variant, comps, sets in inputs():
        w_in = dict.fromkeys(worst, 0.0)
        vs = HR.vectors(len(sets["a"]), 2)
        for which, pos in sets.items():
            for c, (var_nodes, ed) in comps.items():
                x, cp = pos[var_nodes], _component(ed, variant)
                for gn, fs in MODES:
                    if fs and not (np.abs(x) >= 1).any():
                        continue                                 # (the free set is the whole set: the case above)
                    H = _dense(cp, x, gn, fs)
                    for v in vs[:, var_nodes]:
                        ref = HR.product(ed, x, v, variant, gn, fs)
                        r64 = HR.product(ed, x, v, variant, gn, fs, dtype=np.float64)
                        hd = (H @ v.reshape(-1)).reshape(-1, 2)
                        assert ref.n_bound == (int((np.abs(x) >= 1).sum()) if fs else 0)
                        n_bound += ref.n_bound
                        for key, err, unit in (("hvp", np.abs(r64.hv.astype(LD) - ref.hv), ref.hv_unit),
                                               ("hvp_dense", np.abs(hd.astype(LD) - ref.hv), ref.hv_unit),
                                               ("curv", abs(LD(r64.curvature) - ref.curvature), ref.curv_unit),
                                               ("curv_dense", abs(LD(float(v.reshape(-1) @ hd.reshape(-1))) - ref.curvature), ref.curv_unit)):
                            w_in[key] = max(w_in[key], _ratio(err, unit))
                        n += 1
        print("%-14s %-6s largest error / unit: product %.4f (numpy) %.4f (dense), curvature %.4f (numpy) %.4f (dense)"
              % (label, variant, w_in["hvp"], w_in["hvp_dense"], w_in["curv"], w_in["curv_dense"]))
        for key in worst:
            worst[key] = max(worst[key], w_in[key])
    measured = {"GAMMA_HVP_CPU": max(worst["hvp"], worst["hvp_dense"]), "GAMMA_CURV_CPU": max(worst["curv"], worst["curv_dense"])}
    for name, m in measured.items():
        print("%s: measured %.4f over %d products (%d bound coordinates met), recorded %.4g, on the GPU %d x"
              % (name, m, n, n_bound, getattr(HR, name), HR.GPU_FACTOR))
    assert n_bound >= 10
    for name, m in measured.items():
        assert 0.5 * getattr(HR, name) <= m <= getattr(HR, name), (name, m)          # (the constants stay measurements)
    assert HR.GPU_FACTOR == ER.GPU_FACTOR == 8


# --------------------------------------------------------------------------------------------------------------- 2. round trip
def test_round_trip_with_the_jvps_linear_system():
    """xdot solves (reduced H) xdot = b with b = jvp_ref.rhs masked to the free set (numpy, float64): product(xdot, free set) in float64
    gives b back.  The largest |H xdot - b|_2 / |b|_2 per component is ROUND_TRIP_REL_CPU; the GPU test gives the kernels 8 x that."""
    label, variant, comps, sets = inputs()[0]
    assert label == "class_limits"
    pos = sets["a"]
    rng = np.random.default_rng(9210)
    worst = {False: 0.0, True: 0.0}
    for c, (var_nodes, ed) in comps.items():
        cp, x = _component(ed, variant), pos[var_nodes].reshape(-1)
        b = JR.rhs(cp, x, rng.standard_normal((len(ed), 18)), rng.standard_normal(len(ed)))
        for gn in (False, True):
            xdot, status = JR._solve(_dense(cp, x, gn, False), b.copy(), cp.free(x))
            assert status == 0
            got = HR.product(ed, x, xdot, variant, gn, True, dtype=np.float64).hv.reshape(-1)
            want = np.where(cp.free(x), b, 0.0)
            worst[gn] = max(worst[gn], float(np.linalg.norm(got - want) / np.linalg.norm(want)))
    print("round trip: largest relative residual %.3e (exact), %.3e (Gauss-Newton), recorded %.3g" % (worst[False], worst[True], HR.ROUND_TRIP_REL_CPU))
    m = max(worst.values())
    assert 0.5 * HR.ROUND_TRIP_REL_CPU <= m <= HR.ROUND_TRIP_REL_CPU


# ------------------------------------------------------------------------------------------------------------ 3. hand-made facts
def test_symmetry_zero_vector_saturated_edges_and_bound_rows():
    ed, x = _tukey_at_work(600)
    rng = np.random.default_rng(9220)
    u, v = rng.standard_normal((2, 2)), rng.standard_normal((2, 2))
    for gn in (False, True):
        hu, hv = HR.product(ed, x, u, gauss_newton=gn), HR.product(ed, x, v, gauss_newton=gn)
        assert abs((u * hv.hv).sum() - (v * hu.hv).sum()) <= (np.abs(u) * hv.hv_unit).sum() + (np.abs(v) * hu.hv_unit).sum()
        z = HR.product(ed, x, np.zeros((2, 2)), gauss_newton=gn)
        assert not z.hv.any() and z.curvature == 0 and not z.hv_unit.any() and z.curv_unit == 0
        if gn:
            assert hv.curvature > 0
    # a saturated Tukey edge contributes exactly nothing, to the products and to the units
    far = CR.Edges(1, np.array([0]), np.array([-1]), np.array([1.0], LD), np.array([CR.KIND_INTER]), np.zeros((1, 9, 2), LD), np.array([0]))
    for gn in (False, True):
        p = HR.product(far, [[0.3, 0.0]], [[1.0, -2.0]], gauss_newton=gn)
        assert not p.hv.any() and not p.hv_unit.any()
    # a bound coordinate: its row is the identity's and its entry reaches no other row
    ed = dataclasses.replace(ed, kind=np.full(len(ed), CR.KIND_INTRA))            # (Cauchy: the far node's edges stay at work)
    xb = np.array(x, np.float64)
    xb[0, 1] = 1.0
    a = HR.product(ed, xb, v, free_set=True)
    v2 = v.copy()
    v2[0, 1] = 7.0
    b = HR.product(ed, xb, v2, free_set=True)
    assert a.n_bound == 1 and a.hv[0, 1] == v[0, 1] and b.hv[0, 1] == 7.0 and a.hv_unit[0, 1] == 0
    keep = np.ones((2, 2), bool)
    keep[0, 1] = False
    assert np.array_equal(a.hv[keep], b.hv[keep]) and HR.product(ed, xb, v).n_bound == 0
    assert not np.array_equal(HR.product(ed, xb, v).hv[keep], a.hv[keep])
