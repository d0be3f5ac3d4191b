"""HIP-event times of the forward solve, lfr_batch_covariance, the Gauss-Newton backward and lfr_batch_covariance_matches (all three
outputs, float32) on the same batch in the same process: the median of 20 warm repetitions on config 4, config 5 and the cap-sized
sparse workload, a fresh child process per workload.  Writes profiles/match_covariance_bench.json and prints it as one JSON line.

Gate: on config 4 the new call must take no longer than the Gauss-Newton backward - the same sweep, inversion and record re-read, and
about five times the bytes written - beyond the run's own spread (the larger of the two calls' max - min over the repetitions); exit
status 1 otherwise.  lfr_batch_covariance is recorded beside it: against the same script run on the parent commit it shows that the
existing kernels kept their time.  Config 5 and the cap-sized workload (the workgroup classes) are recorded, not gated."""
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
    new = hasattr(b, "covariance_matches")          # (the parent commit: the three existing passes only)
    b.solve()
    b.solve()                                      # warm: records materialised, the passes' workspaces set up below
    calls = {"forward": lambda: b.solve()["kernel_ms"],
             "covariance": lambda: b.covariance(want_stats=True)[1]["kernel_ms"],
             "backward_gn": lambda: b.backward(gp, want_stats=True, gauss_newton=True)[3]["kernel_ms"]}
    if new:
        calls["covariance_matches"] = lambda: b.covariance_matches(f64=False, want_stats=True)["stats"]["kernel_ms"]
    for f in calls.values():
        f()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            ms[k].append(f())
    info = b.component_info()
    rows = 2 * info["n_var_nodes"]
    out = {"workload": name, "components": int(len(rows)), "components_up_to_32_rows": int((rows <= 32).sum()), "max_rows": int(rows.max()),
           "matches": int(g.n_edges // 2)}
    for k, v in ms.items():
        out[k + "_ms_median"] = float(np.median(v))
        out[k + "_ms_min"] = float(np.min(v))
        out[k + "_ms_max"] = float(np.max(v))
    if new:
        st = b.covariance_matches(f64=False, want_stats=True)["stats"]
        out.update(n_computed=int(st["n_computed"]), n_not_usable=int(st["n_not_usable"]), n_singular=int(st["n_singular"]),
                   matches_over_backward_gn=out["covariance_matches_ms_median"] / out["backward_gn_ms_median"])
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
    c4 = results[0]
    doc = {"reps": reps, "timer": "HIP events around the pass (kernel_ms of the call's stats), median of warm repetitions", "results": results}
    if "covariance_matches_ms_median" in c4:
        spread = max(c4[k + "_ms_max"] - c4[k + "_ms_min"] for k in ("covariance_matches", "backward_gn"))
        doc["gate"] = {"workload": "config4", "rule": "covariance_matches_ms_median <= backward_gn_ms_median + spread", "spread_ms": spread,
                       "matches_over_backward_gn": c4["matches_over_backward_gn"],
                       "met": bool(c4["covariance_matches_ms_median"] <= c4["backward_gn_ms_median"] + spread)}
    path = os.environ.get("LFR_BENCH_OUT", os.path.join(ROOT, "profiles", "match_covariance_bench.json"))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if doc.get("gate", {"met": True})["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
