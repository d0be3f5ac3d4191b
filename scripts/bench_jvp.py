"""HIP-event times of the forward solve, the backward (lfr_batch_backward) and the forward-mode sensitivity (lfr_batch_jvp) in both
Hessian modes on the same batch in the same process: the median of 20 warm repetitions on config 4, config 5 and the cap-sized sparse
workload, a fresh child process per workload.  Writes profiles/jvp_bench.json and prints it as one JSON line.

No gate: nobody had measured this pass.  The figure to read is jvp beside the same run's backward in the same mode.  (bench.py stays
the measure of the forward.)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-feature-refinement_amd"))

WORKLOADS = {"config4": True, "config5": False, "capsized_sparse": False}       # name: device assembly
CHILD_TIMEOUT_S = 420
MODES = {"exact": False, "gn": True}


def measure(name, reps):
    import numpy as np
    import torch

    from lfr_amd import capi, synthetic
    ma = getattr(synthetic, name)()
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g, device_graph_stage=0) if WORKLOADS[name] else capi.Problem(g)
    b = capi.Batch(p, 0)
    rng = np.random.default_rng(0)
    m = g.n_edges // 2
    gp = torch.as_tensor(rng.standard_normal((g.n_nodes, 2)), device="cuda:0")
    tan = [torch.as_tensor(rng.standard_normal(s).astype(np.float32), device="cuda:0") for s in ((m, 18), (m, 18), (m,))]
    b.solve()
    b.solve()                                      # warm: records materialised, the passes' workspaces set up below
    st = {k: (b.backward(gp, want_stats=True, gauss_newton=gn)[3], b.jvp(*tan, want_stats=True, gauss_newton=gn)[1]) for k, gn in MODES.items()}
    fwd, bwd, jvp = [], {k: [] for k in MODES}, {k: [] for k in MODES}
    for _ in range(reps):
        fwd.append(b.solve()["kernel_ms"])
        for k, gn in MODES.items():
            bwd[k].append(b.backward(gp, want_stats=True, gauss_newton=gn)[3]["kernel_ms"])
            jvp[k].append(b.jvp(*tan, want_stats=True, gauss_newton=gn)[1]["kernel_ms"])
    info = b.component_info()
    rows = 2 * info["n_var_nodes"]
    out = {"workload": name, "components": int(len(rows)), "components_up_to_32_rows": int((rows <= 32).sum()), "max_rows": int(rows.max()),
           "forward_ms_median": float(np.median(fwd)), "forward_ms_min": float(np.min(fwd))}
    for k in MODES:
        out["backward_%s_ms_median" % k] = float(np.median(bwd[k]))
        out["jvp_%s_ms_median" % k] = float(np.median(jvp[k]))
        out["backward_%s_ms_min" % k] = float(np.min(bwd[k]))
        out["jvp_%s_ms_min" % k] = float(np.min(jvp[k]))
        out["jvp_over_backward_%s" % k] = out["jvp_%s_ms_median" % k] / out["backward_%s_ms_median" % k]
        out["status2_%s" % k] = int(st[k][1]["n_indefinite"])
        assert st[k][0]["n_indefinite"] == st[k][1]["n_indefinite"] and st[k][0]["n_differentiated"] == st[k][1]["n_differentiated"]
    out["n_not_usable"] = int(st["gn"][1]["n_not_usable"])
    out["n_bound_coordinates"] = int(st["gn"][1]["n_bound_coordinates"])
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
    doc = {"reps": reps, "timer": "HIP events around the pass (lfr_jvp_stats.kernel_ms / lfr_backward_stats.kernel_ms / lfr_solve_stats), "
                                  "median of warm repetitions", "results": results}
    path = os.environ.get("LFR_BENCH_OUT", os.path.join(ROOT, "profiles", "jvp_bench.json"))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
