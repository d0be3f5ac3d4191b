"""The jvp's CPU reference (tests/jvp_ref.py) on the class-limit shapes of tests/class_limit_cases.py, at the oracle's positions: status 0
and a non-zero tangent for all 33 shapes in both Hessian modes and both Tukey variants.  tests/test_gpu_jvp_class_limits.py demands
that EVERY shape is compared with this reference; here the reference alone is shown to stay inside that condition (no shape whose
Hessian it finds indefinite) before any kernel runs."""
import numpy as np
import pytest

import backward_ref as BR
import class_limit_cases as CL
import jvp_ref as JR
import lfr_oracle as O


@pytest.fixture(scope="module", params=["ceres1", "ceres2"])
def shapes(request):
    """{name: (component of backward_ref, the oracle's positions of its variable nodes)} of ALL under one Tukey variant"""
    ma, feats = CL.all_shapes()
    ref = O.run(ma, n_threads=4, tukey_variant=request.param)
    assert ref["rc"] == 0 and (ref["infos"]["termination"][ref["comp_nvar"] > 0] == 0).all()
    idx = {name: i for i, name in enumerate(ma.image_names)}
    ni = np.array([idx[name] for name in ref["image_names"]], np.int32)[ref["node_image"]]
    comps = BR.graph_components(ma, ref["track"], ref["is_root"], ref["comp"], ni, ref["node_feat"], request.param)
    by_name = CL.components_of(feats, ref["node_feat"], ref["comp"])
    assert sorted(by_name.values()) == sorted(comps)
    return ma, {name: (comps[c][1], ref["positions"][comps[c][0]].reshape(-1)) for name, c in by_name.items()}


@pytest.mark.parametrize("gn", [False, True], ids=["exact", "gauss_newton"])
def test_reference_differentiates_every_shape(shapes, gn):
    ma, by_name = shapes
    rng = np.random.default_rng(41)
    t1, t2, ts = rng.standard_normal((len(ma.sim), 18)), rng.standard_normal((len(ma.sim), 18)), rng.standard_normal(len(ma.sim))
    items = []
    for name in CL.NAMES:
        cp, x = by_name[name]
        assert (2 * cp.nv, len(cp.src)) == (CL.SHAPES[name]["rows"], CL.SHAPES[name]["edges"]), name
        m, odd = cp.eids >> 1, (cp.eids & 1) == 1
        items.append((cp, x, np.where(odd[:, None], t1[m], t2[m]), ts[m]))
    out = JR.jvp_many(items, gauss_newton=gn)
    assert len(out) == len(CL.NAMES) == 33
    for name, (xdot, status) in zip(CL.NAMES, out):
        assert status == 0, name
        assert np.isfinite(xdot).all() and xdot.any(), name
        assert (np.abs(by_name[name][1]) < 1.0).all(), name          # (no coordinate at the bound: every row is a row of H)
