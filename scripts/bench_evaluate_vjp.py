"""HIP-event times of lfr_batch_evaluate_vjp - all three bars in, all four gradients out (float64), and the cost bar alone into the
position gradient - beside the SAME run's lfr_batch_evaluate (all outputs, float64), lfr_batch_set_inputs (flows and similarities) and
Gauss-Newton lfr_batch_backward on the same batch: warm, the median of 20 repetitions, on config 4, the long-track workload (config 5)
and the cap-sized sparse workload, a fresh child process per workload.  Also the bytes the full call has to move held against 8 TB/s
of HBM.  Writes profiles/evaluate_vjp_bench.json (or LFR_BENCH_OUT) and prints it as one JSON line.

Nothing is gated: nobody had measured this kernel before.  (bench.py stays the measure of the forward.)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-feature-refinement_amd"))

WORKLOADS = {"config4": True, "config5": False, "capsized_sparse": False}       # name: device assembly
CHILD_TIMEOUT_S = 420
HBM_BYTES_PER_S = 8e12


def measure(name, reps):
    import numpy as np
    import torch

    from lfr_amd import capi, synthetic
    ma = getattr(synthetic, name)()
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g, device_graph_stage=0) if WORKLOADS[name] else capi.Problem(g)
    b = capi.Batch(p, 0)
    dev = torch.device("cuda", 0)
    n, m = g.n_nodes, g.n_edges // 2
    rng = np.random.default_rng(0)
    gp = torch.as_tensor(rng.standard_normal((n, 2)), device=dev)
    d1, d2 = (torch.as_tensor(np.ascontiguousarray(x, np.float32).reshape(-1, 18)).to(dev) for x in (ma.disp1, ma.disp2))
    sim = torch.as_tensor(np.ascontiguousarray(ma.sim, np.float32)).to(dev)
    b.solve()
    b.solve()                                      # warm: records materialised
    info = b.component_info()
    cbar = torch.as_tensor(rng.standard_normal(len(info["component"])), device=dev)
    rbar, wbar = torch.as_tensor(rng.standard_normal((m, 2, 2)), device=dev), torch.as_tensor(rng.standard_normal((m, 2)), device=dev)
    full_kw = dict(cost_bar=cbar, residuals_bar=rbar, weights_bar=wbar, want_stats=True)
    st = b.evaluate_vjp(**full_kw)["stats"]        # the record -> edge map, the pass states
    b.evaluate(want_stats=True)
    b.backward(gp, want_stats=True, gauss_newton=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = {k: [] for k in ("solve", "evaluate", "evaluate_vjp", "evaluate_vjp_cost_bar_to_positions", "set_inputs", "backward_gn")}
    for _ in range(reps):
        e0.record()
        b.set_inputs(d1, d2, sim)                  # (the values the batch holds: the solve below is the same solve)
        e1.record()
        e1.synchronize()
        t["set_inputs"].append(e0.elapsed_time(e1))
        t["solve"].append(b.solve()["kernel_ms"])
        t["evaluate"].append(b.evaluate(want_stats=True)["stats"]["kernel_ms"])
        t["evaluate_vjp"].append(b.evaluate_vjp(**full_kw)["stats"]["kernel_ms"])
        t["evaluate_vjp_cost_bar_to_positions"].append(b.evaluate_vjp(cost_bar=cbar, want=("positions",), want_stats=True)["stats"]["kernel_ms"])
        t["backward_gn"].append(b.backward(gp, want_stats=True, gauss_newton=True)[3]["kernel_ms"])
    n_edges, n_var = int(info["n_edges"].astype(np.int64).sum()), int(info["n_var_nodes"].astype(np.int64).sum())
    wg_edges = int(info["n_edges"][2 * info["n_var_nodes"] > 32].astype(np.int64).sum())     # (rows above 32: records and bars read twice)
    # the full float64 call: records, edge map and the two per-match bars (twice in the workgroup classes), positions and cost bar in;
    # the three per-match gradients cleared and the records' rows stored, the similarity scratch cleared, stored, read and combined,
    # the position gradient cleared and stored
    bytes_full = ((80 + 4 + 16 + 8) * (n_edges + wg_edges) + 16 * n_var + 8 * len(info["component"])
                  + 2 * 18 * 8 * m + 18 * 8 * n_edges + 16 * m + 8 * n_edges + 16 * m + 8 * m + 16 * n + 16 * n_var)
    out = {"workload": name, "components": int(len(info["component"])), "max_rows": int(2 * info["n_var_nodes"].max()), "edges": n_edges,
           "matches": m, "reps": reps}
    for k, v in t.items():
        out[k + "_ms_median"], out[k + "_ms_min"] = float(np.median(v)), float(np.min(v))
    out.update({"evaluate_vjp_over_evaluate": out["evaluate_vjp_ms_median"] / out["evaluate_ms_median"],
                "evaluate_vjp_over_backward_gn": out["evaluate_vjp_ms_median"] / out["backward_gn_ms_median"],
                "bytes_all_bars_all_outputs": bytes_full, "hbm_floor_ms_all_bars_all_outputs": 1e3 * bytes_full / HBM_BYTES_PER_S,
                "n_nonfinite": int(st["n_nonfinite"])})
    return out


def main():
    reps = int(os.environ.get("LFR_BENCH_REPS", "20"))
    if len(sys.argv) == 3 and sys.argv[1] == "--workload":
        print("RESULT " + json.dumps(measure(sys.argv[2], reps)), flush=True)
        return 0
    results = []
    for name in WORKLOADS:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", name], capture_output=True, text=True,
                                 timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            sys.stderr.write("%s: no result after %d s\n" % (name, CHILD_TIMEOUT_S))
            return 2                                # (nothing further is started on the device)
        lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
        if out.returncode != 0 or not lines:
            sys.stderr.write(out.stdout + out.stderr)
            return 2                                # (nothing further is started on the device)
        results.append(json.loads(lines[-1][len("RESULT "):]))
    doc = {"reps": reps, "timer": "HIP events around each call (the stats' kernel_ms; lfr_batch_set_inputs: a pair of events on its stream), "
                                  "median of warm repetitions", "results": results}
    path = os.environ.get("LFR_BENCH_OUT", os.path.join(ROOT, "profiles", "evaluate_vjp_bench.json"))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
