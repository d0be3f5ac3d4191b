"""HIP-event times of lfr_batch_hessian_product, warm, median of 20 repetitions in one process, on config 4, the long-track workload
(config 5) and the cap-sized sparse workload: one vector and four, exact and Gauss-Newton, each beside the same run's
lfr_batch_evaluate with the gradient as its only output.  Writes profiles/hessian_product_bench.json (or the path given) and prints
it.  (bench.py stays the measure of the forward.)

The two expectations DESIGN.md 5.12 states are recorded as ratios, not enforced: one vector against the evaluate's gradient sweep,
four vectors against four calls with one."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-feature-refinement_amd"))

import numpy as np
import torch

from lfr_amd import capi, synthetic


def measure(name, ma, reps, device_assembly):
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g, device_graph_stage=0) if device_assembly else capi.Problem(g)
    b = capi.Batch(p, 0)
    vs = torch.as_tensor(np.random.default_rng(0).standard_normal((4, g.n_nodes, 2)), device="cuda:0")
    b.solve()
    b.solve()                                      # warm: records materialised
    cases = {"%s_k%d" % ("gauss_newton" if gn else "exact", k): (gn, k) for gn in (False, True) for k in (1, 4)}
    b.evaluate(cost=False, residuals=False, weights=False, want_stats=True)
    for gn, k in cases.values():
        b.hessian_product(vs[:k], gauss_newton=gn, curvature=True, want_stats=True)
    ev, hp = [], {c: [] for c in cases}
    for _ in range(reps):
        ev.append(b.evaluate(cost=False, residuals=False, weights=False, want_stats=True)["stats"]["kernel_ms"])
        for c, (gn, k) in cases.items():
            hp[c].append(b.hessian_product(vs[:k], gauss_newton=gn, curvature=True, want_stats=True)["stats"]["kernel_ms"])
    info = b.component_info()
    e = float(np.median(ev))
    out = {"workload": name, "components": int(len(info["component"])), "edges": int(info["n_edges"].sum()),
           "max_rows": int(2 * info["n_var_nodes"].max()), "reps": reps, "evaluate_gradient_ms_median": e, "evaluate_gradient_ms_min": float(np.min(ev))}
    for c in cases:
        out[c + "_ms_median"], out[c + "_ms_min"] = float(np.median(hp[c])), float(np.min(hp[c]))
    for mode in ("exact", "gauss_newton"):
        out[mode + "_k1_over_evaluate_gradient"] = out[mode + "_k1_ms_median"] / e
        out[mode + "_k4_over_four_k1"] = out[mode + "_k4_ms_median"] / (4.0 * out[mode + "_k1_ms_median"])
    return out


def main():
    reps = int(os.environ.get("LFR_BENCH_REPS", "20"))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hessian_product_bench.json")
    out = [measure("config4", synthetic.config4(), reps, True),
           measure("config5", synthetic.config5(), reps, False),
           measure("capsized_sparse", synthetic.capsized_sparse(), reps, False)]
    text = json.dumps({"device": torch.cuda.get_device_name(0), "results": out}, indent=1)
    with open(path, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
