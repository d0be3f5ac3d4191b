"""HIP-event times of the backward and the jvp in their three Hessian modes - exact, Gauss-Newton, and exact with the Gauss-Newton
fallback (LFR_BACKWARD_FALLBACK_GAUSS_NEWTON / LFR_JVP_FALLBACK_GAUSS_NEWTON) - on the same batch in the same process: config 4,
config 5 and the cap-sized sparse workload, a fresh child process per workload, the modes interleaved inside every repetition.
A run is the median of 20 warm repetitions; every workload is measured in RUNS such runs, so that the spread of the exact mode's own
medians from run to run stands next to the difference between the modes.  Per mode also the status histogram
(lfr_batch_backward_status / lfr_batch_jvp_status).  Writes profiles/backward_fallback_bench.json and prints it as one JSON line.

Expectation (checked, exit status 1 otherwise): config 4 has no indefinite component, so the fallback mode runs the exact mode's
work there and must cost what the exact mode costs - |median(fallback) - median(exact)| within the spread (max - min) of the exact
mode's medians, for the backward and for the jvp.  Config 5 and the cap-sized workload factor their indefinite components twice and
sweep them: recorded, not gated.  (bench.py stays the measure of the forward.)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-feature-refinement_amd"))

WORKLOADS = {"config4": True, "config5": False, "capsized_sparse": False}       # name: device assembly
MODES = {"exact": {}, "gauss_newton": {"gauss_newton": True}, "fallback": {"gn_fallback": True}}
RUNS = 5
CHILD_TIMEOUT_S = 420


def measure(name, reps):
    import numpy as np
    import torch

    from lfr_amd import capi, synthetic
    ma = getattr(synthetic, name)()
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g, device_graph_stage=0) if WORKLOADS[name] else capi.Problem(g)
    b = capi.Batch(p, 0)
    rng = np.random.default_rng(0)
    gp = torch.as_tensor(rng.standard_normal((g.n_nodes, 2)), device="cuda:0")
    m = len(ma.sim)
    ts = [torch.as_tensor(rng.standard_normal(s).astype(np.float32), device="cuda:0") for s in ((m, 18), (m, 18), (m,))]
    b.solve()
    b.solve()                                      # warm: records materialised, the passes' workspaces set up below
    calls = {"backward": lambda kw: b.backward(gp, want_stats=True, **kw)[3], "jvp": lambda kw: b.jvp(*ts, want_stats=True, **kw)[1]}
    status = {"backward": b.backward_status, "jvp": b.jvp_status}
    out = {"workload": name}
    info = b.component_info()
    rows = 2 * info["n_var_nodes"]
    out.update(components=int(len(rows)), components_up_to_32_rows=int((rows <= 32).sum()), max_rows=int(rows.max()))
    for what, call in calls.items():
        hist = {}
        for mode, kw in MODES.items():             # warm every mode once; its status histogram
            call(kw)
            s = status[what]()
            hist[mode] = {str(v): int((s == v).sum()) for v in (0, 1, 2, 3)}
        medians = {mode: [] for mode in MODES}
        for _ in range(RUNS):
            ms = {mode: [] for mode in MODES}
            for _ in range(reps):
                for mode, kw in MODES.items():
                    ms[mode].append(call(kw)["kernel_ms"])
            for mode in MODES:
                medians[mode].append(float(np.median(ms[mode])))
        res = {"status_histogram": hist, "run_medians_ms": medians}
        for mode in MODES:
            res[mode + "_ms_median"] = float(np.median(medians[mode]))
        res["exact_run_to_run_spread_ms"] = float(max(medians["exact"]) - min(medians["exact"]))
        res["fallback_minus_exact_ms"] = res["fallback_ms_median"] - res["exact_ms_median"]
        res["fallback_over_exact"] = res["fallback_ms_median"] / res["exact_ms_median"]
        out[what] = res
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
    check = {"workload": "config4", "rule": "|fallback_ms_median - exact_ms_median| <= exact_run_to_run_spread_ms, no status 3"}
    for what in ("backward", "jvp"):
        r = c4[what]
        check[what] = {"fallback_minus_exact_ms": r["fallback_minus_exact_ms"], "exact_run_to_run_spread_ms": r["exact_run_to_run_spread_ms"],
                       "met": bool(abs(r["fallback_minus_exact_ms"]) <= r["exact_run_to_run_spread_ms"]
                                   and r["status_histogram"]["fallback"]["3"] == 0)}
    check["met"] = check["backward"]["met"] and check["jvp"]["met"]
    doc = {"reps": reps, "runs": RUNS,
           "timer": "HIP events around the pass (lfr_backward_stats.kernel_ms / lfr_jvp_stats.kernel_ms); a run = the median of `reps` "
                    "warm repetitions with the three modes interleaved, *_ms_median = the median of the runs' medians",
           "expectation": check, "results": results}
    path = os.environ.get("LFR_BENCH_OUT", os.path.join(ROOT, "profiles", "backward_fallback_bench.json"))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if check["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
