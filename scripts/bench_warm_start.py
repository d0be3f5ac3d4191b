#!/usr/bin/env python3
"""Cold against warm solve after a small flow change -> profiles/warm_start_bench.json (recorded, not gated).

Per workload (config 4, config 5, the cap-sized sparse graph), each in a fresh child process: a cold solve, then set_inputs with the
flows perturbed by N(0, 0.002) at a fixed seed; on those inputs lfr_batch_solve and lfr_batch_solve_from(NULL) alternate 20 times, the
start restored to the first solution before each warm call.  Medians of kernel_ms, sum_iterations, exec_passes_edges and of the
per-class times of lfr_batch_timing.

    python scripts/bench_warm_start.py [--repeats 20] [--out profiles/warm_start_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-feature-refinement_amd"))
SEED = 20260
SIGMA = 0.002


def workload(name):
    from lfr_amd import synthetic
    if name == "config4":
        return synthetic.config4()
    if name == "config5":
        return synthetic.config5()
    return synthetic.capsized_sparse(n_tracks=12000)          # bench.py's --sparse-tracks default


def child(name, repeats):
    import numpy as np
    import torch
    from lfr_amd import capi
    dev = torch.device("cuda", 0)
    ma = workload(name)
    g = capi.Graph.from_arrays(ma)
    p = capi.Problem(g, device_graph_stage=0)
    b = capi.Batch(p, 0)
    first_stats = b.solve()
    first = torch.empty((g.n_nodes, 2), dtype=torch.float64, device=dev)
    b.positions_to(first)
    gen = torch.Generator(device=dev).manual_seed(SEED)

    def perturbed(x):
        t = torch.as_tensor(np.ascontiguousarray(x, np.float32).reshape(-1, 18)).to(dev)
        return t + SIGMA * torch.randn(t.shape, generator=gen, device=dev, dtype=torch.float32)

    b.set_inputs(perturbed(ma.disp1), perturbed(ma.disp2))
    torch.cuda.synchronize()
    rows = {"cold": [], "warm": []}
    for _ in range(repeats):
        st = b.solve()
        rows["cold"].append((st["kernel_ms"], st["sum_iterations"], st["exec_passes_edges"], b.timing()[1].tolist()))
        st = b.solve_from(first)             # (an explicit copy of the first solution: the start is the same before every warm call)
        rows["warm"].append((st["kernel_ms"], st["sum_iterations"], st["exec_passes_edges"], b.timing()[1].tolist()))
    out = {"workload": name, "n_components": first_stats["n_components"], "n_edges": first_stats["n_edges"],
           "first_solve_iterations": first_stats["sum_iterations"], "repeats": repeats, "sigma": SIGMA, "seed": SEED,
           "spin_timeouts": int(b.spin_timeouts()), "team_fallbacks": int(b.team_fallbacks())}
    for k, r in rows.items():
        out[k] = {"kernel_ms": float(np.median([x[0] for x in r])), "sum_iterations": int(np.median([x[1] for x in r])),
                  "exec_passes_edges": int(np.median([x[2] for x in r])),
                  "class_ms": np.median(np.array([x[3] for x in r]), axis=0).tolist()}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warm_start_bench.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--workloads", default="config4,config5,capsized")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.repeats)
        return
    results = []
    for name in a.workloads.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(a.repeats)],
                           capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("workload %s failed (exit %d)" % (name, r.returncode))
        results.append(json.loads(line[0][7:]))
        print("%-9s cold %.3f ms / %d iterations, warm %.3f ms / %d iterations" % (
            name, results[-1]["cold"]["kernel_ms"], results[-1]["cold"]["sum_iterations"],
            results[-1]["warm"]["kernel_ms"], results[-1]["warm"]["sum_iterations"]), flush=True)
    json.dump({"workloads": results}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
