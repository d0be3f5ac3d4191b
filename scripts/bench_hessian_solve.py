"""HIP-event times of lfr_batch_hessian_solve, warm, median of 20 repetitions in one process, on config 4, the long-track workload
(config 5) and the cap-sized sparse workload: Gauss-Newton, one right-hand side and four, rel_tolerance 1e-10, with the iterations
taken (sum, max).  Beside each: the same run's lfr_batch_hessian_product with one vector and, where the backward serves the workload,
the Gauss-Newton lfr_batch_backward.  Writes profiles/hessian_solve_bench.json (or the path given) and prints it.  (bench.py stays the
measure of the forward.)

Recorded as a ratio, not enforced: the time per iteration of the component that iterates longest (solve time / max iterations, an
upper bound on it: the packed launch runs in front of the workgroup launch on the same stream) against one product call, products
only."""
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
    rng = np.random.default_rng(0)
    bs = torch.as_tensor(rng.standard_normal((4, g.n_nodes, 2)), device="cuda:0")
    b.solve()
    b.solve()                                      # warm: records materialised
    info = b.component_info()
    out = {"workload": name, "components": int(len(info["component"])), "edges": int(info["n_edges"].sum()),
           "max_rows": int(2 * info["n_var_nodes"].max()), "reps": reps, "rel_tolerance": 1e-10}
    kw = dict(gauss_newton=True, rel_tolerance=1e-10, want_stats=True)
    hp, hs, stats = [], {1: [], 4: []}, {}
    for rep in range(reps + 1):                    # (the first round warms)
        t = b.hessian_product(bs[0], gauss_newton=True, want_stats=True)["stats"]["kernel_ms"]
        if rep:
            hp.append(t)
        for k in (1, 4):
            st = b.hessian_solve(bs[:k], **kw)["stats"]
            stats[k] = st
            if rep:
                hs[k].append(st["kernel_ms"])
    out["hessian_product_k1_ms_median"] = float(np.median(hp))
    for k in (1, 4):
        st = stats[k]
        out["solve_k%d_ms_median" % k], out["solve_k%d_ms_min" % k] = float(np.median(hs[k])), float(np.min(hs[k]))
        out["solve_k%d_iterations_sum" % k], out["solve_k%d_iterations_max" % k] = int(st["sum_iterations"]), int(st["max_iterations_used"])
        out["solve_k%d_status" % k] = {n: int(st[n]) for n in ("n_converged", "n_max_iterations", "n_negative_curvature", "n_nonfinite")}
    out["solve_k1_ms_per_iteration_of_the_longest_over_product_k1"] = (out["solve_k1_ms_median"] / max(1, out["solve_k1_iterations_max"])
                                                                        / out["hessian_product_k1_ms_median"])
    grad = torch.as_tensor(rng.standard_normal((g.n_nodes, 2)), device="cuda:0")
    try:
        bw = [b.backward(grad, gauss_newton=True, want_stats=True)[-1]["kernel_ms"] for _ in range(reps + 1)][1:]      # (the first call warms)
        out["backward_gauss_newton_ms_median"] = float(np.median(bw))
    except capi.LfrError as e:                      # the backward refuses the workload (a component above its row limit)
        out["backward_gauss_newton_ms_median"] = None
        out["backward_not_served"] = str(e)[:160]
    return out


def main():
    reps = int(os.environ.get("LFR_BENCH_REPS", "20"))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hessian_solve_bench.json")
    out = [measure("config4", synthetic.config4(), reps, True),
           measure("config5", synthetic.config5(), reps, False),
           measure("capsized_sparse", synthetic.capsized_sparse(), reps, False)]
    text = json.dumps({"device": torch.cuda.get_device_name(0), "results": out}, indent=1)
    with open(path, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
