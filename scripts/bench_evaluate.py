"""HIP-event times of lfr_batch_evaluate - all four outputs (float64) and cost only - beside the SAME run's lfr_solve_stats.kernel_ms of
the same batch, warm, median of 20 repetitions in one process, on config 4 and the long-track workload (config 5), and the bytes the
call has to move held against 8 TB/s of HBM.  Writes profiles/evaluate_bench.json (or the path given) and prints it.  (bench.py stays
the measure of the forward.)

The expectation: the evaluate makes one sweep over the records where the solve makes at least two plus its factorizations, so it
should come in below the solve on both workloads.  The script reports whether it did; it does not fail when it did not."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-feature-refinement_amd"))

import numpy as np
import torch

from lfr_amd import capi, synthetic

HBM_BYTES_PER_S = 8e12


def measure(name, ma, reps, device_assembly):
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g, device_graph_stage=0) if device_assembly else capi.Problem(g)
    b = capi.Batch(p, 0)
    b.solve()
    b.solve()                                      # warm: records materialised
    b.evaluate(want_stats=True)                    # the record -> edge map, the pass state
    fwd, full, cost = [], [], []
    for _ in range(reps):
        fwd.append(b.solve()["kernel_ms"])
        full.append(b.evaluate(want_stats=True)["stats"]["kernel_ms"])
        cost.append(b.evaluate(grad=False, residuals=False, weights=False, want_stats=True)["stats"]["kernel_ms"])
    st = b.evaluate(want_stats=True)["stats"]
    info = b.component_info()
    n_edges, n_var = int(info["n_edges"].astype(np.int64).sum()), int(info["n_var_nodes"].astype(np.int64).sum())
    wg_edges = int(info["n_edges"][2 * info["n_var_nodes"] > 32].astype(np.int64).sum())     # (rows above 32: read twice when the gradient is asked for)
    n, m = g.n_nodes, g.n_edges // 2
    # records, positions of the variable nodes and the cost; with every output: the record -> edge map, the gradient (cleared, then
    # stored), residuals and weights in float64 (cleared / set to -1, then stored), the second read of the workgroup classes' records
    bytes_cost = 80 * n_edges + 16 * n_var + 8 * len(info["component"])
    bytes_full = bytes_cost + 4 * n_edges + 80 * wg_edges + 16 * n + 16 * n_var + 2 * 8 * (4 * m + 2 * m)
    f, e, c = float(np.median(fwd)), float(np.median(full)), float(np.median(cost))
    return {"workload": name, "components": int(len(info["component"])), "max_rows": int(2 * info["n_var_nodes"].max()), "edges": n_edges,
            "reps": reps, "solve_ms_median": f, "evaluate_ms_median": e, "evaluate_cost_only_ms_median": c,
            "solve_ms_min": float(np.min(fwd)), "evaluate_ms_min": float(np.min(full)), "evaluate_cost_only_ms_min": float(np.min(cost)),
            "evaluate_over_solve": e / f, "cost_only_over_solve": c / f,
            "bytes_all_outputs": bytes_full, "bytes_cost_only": bytes_cost,
            "hbm_floor_ms_all_outputs": 1e3 * bytes_full / HBM_BYTES_PER_S, "hbm_floor_ms_cost_only": 1e3 * bytes_cost / HBM_BYTES_PER_S,
            "n_nonfinite": st["n_nonfinite"], "sum_cost": st["sum_cost"]}


def main():
    reps = int(os.environ.get("LFR_BENCH_REPS", "20"))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "evaluate_bench.json")
    out = [measure("config4", synthetic.config4(), reps, True),
           measure("long_tracks_config5", synthetic.config5(), reps, False)]
    res = {"device": torch.cuda.get_device_name(0), "results": out,
           "evaluate_below_solve": {r["workload"]: bool(r["evaluate_ms_median"] < r["solve_ms_median"]) for r in out}}
    text = json.dumps(res, indent=1)
    with open(path, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
