"""HIP-event times of the forward solve, the exact backward and the Gauss-Newton backward (lfr_batch_backward with
LFR_BACKWARD_GAUSS_NEWTON) on the same batch in the same process: the median of 20 warm repetitions on config 4, config 5 and the
cap-sized sparse workload, a fresh child process per workload.  Writes profiles/backward_gn_bench.json and prints it as one JSON line.

Gate: on config 4 the Gauss-Newton backward must be faster than the exact backward (exit status 1 otherwise); config 5 and the
cap-sized workload are recorded, not gated.  (bench.py stays the measure of the forward.)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-feature-refinement_amd"))

WORKLOADS = {"config4": True, "config5": False, "capsized_sparse": False}       # name: device assembly
CHILD_TIMEOUT_S = 420


def measure(name, reps):
    import numpy as np
    import torch

    from lfr_amd import capi, synthetic
    ma = getattr(synthetic, name)()
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g, device_graph_stage=0) if WORKLOADS[name] else capi.Problem(g)
    b = capi.Batch(p, 0)
    gp = torch.as_tensor(np.random.default_rng(0).standard_normal((g.n_nodes, 2)), device="cuda:0")
    b.solve()
    b.solve()                                      # warm: records materialised, backward workspace set up below
    st = {False: b.backward(gp, want_stats=True)[3], True: b.backward(gp, want_stats=True, gauss_newton=True)[3]}
    fwd, bwd = [], {False: [], True: []}
    for _ in range(reps):
        fwd.append(b.solve()["kernel_ms"])
        for gn in (False, True):
            bwd[gn].append(b.backward(gp, want_stats=True, gauss_newton=gn)[3]["kernel_ms"])
    info = b.component_info()
    rows = 2 * info["n_var_nodes"]
    exact, gauss = float(np.median(bwd[False])), float(np.median(bwd[True]))
    return {"workload": name, "components": int(len(rows)), "components_up_to_32_rows": int((rows <= 32).sum()), "max_rows": int(rows.max()),
            "forward_ms_median": float(np.median(fwd)), "backward_exact_ms_median": exact, "backward_gn_ms_median": gauss,
            "forward_ms_min": float(np.min(fwd)), "backward_exact_ms_min": float(np.min(bwd[False])),
            "backward_gn_ms_min": float(np.min(bwd[True])), "gn_over_exact": gauss / exact,
            "status2_exact": int(st[False]["n_indefinite"]), "status2_gn": int(st[True]["n_indefinite"]),
            "n_not_usable": int(st[True]["n_not_usable"]), "n_bound_coordinates": int(st[True]["n_bound_coordinates"])}


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
    c4 = results[0]
    doc = {"reps": reps, "timer": "HIP events around the pass (lfr_backward_stats.kernel_ms / lfr_solve_stats), median of warm repetitions",
           "gate": {"workload": "config4", "rule": "backward_gn_ms_median < backward_exact_ms_median", "gn_over_exact": c4["gn_over_exact"],
                    "met": bool(c4["backward_gn_ms_median"] < c4["backward_exact_ms_median"])},
           "results": results}
    path = os.environ.get("LFR_BENCH_OUT", os.path.join(ROOT, "profiles", "backward_gn_bench.json"))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if doc["gate"]["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
