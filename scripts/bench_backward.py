"""HIP-event times of the forward solve and the implicit-gradient backward (lfr_batch_backward), warm, over 20 repetitions, on config 4,
config 5 and the cap-sized sparse workload.  Prints one JSON line.  (bench.py stays the measure of the forward.)"""
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
    gp = torch.as_tensor(np.random.default_rng(0).standard_normal((g.n_nodes, 2)), device="cuda:0")
    b.solve()
    b.solve()                                      # warm: records materialised, backward workspace set up below
    _, _, _, st = b.backward(gp, want_stats=True)
    fwd, bwd = [], []
    for _ in range(reps):
        fwd.append(b.solve()["kernel_ms"])
        bwd.append(b.backward(gp, want_stats=True)[3]["kernel_ms"])
    info = b.component_info()
    return {"workload": name, "components": int(len(info["component"])), "max_rows": int(2 * info["n_var_nodes"].max()),
            "forward_ms_median": float(np.median(fwd)), "backward_ms_median": float(np.median(bwd)),
            "forward_ms_min": float(np.min(fwd)), "backward_ms_min": float(np.min(bwd)),
            "n_indefinite": st["n_indefinite"], "n_not_usable": st["n_not_usable"], "n_bound_coordinates": st["n_bound_coordinates"]}


def main():
    reps = int(os.environ.get("LFR_BENCH_REPS", "20"))
    out = [measure("config4", synthetic.config4(), reps, True),
           measure("config5", synthetic.config5(), reps, False),
           measure("capsized_sparse", synthetic.capsized_sparse(), reps, False)]
    print(json.dumps({"reps": reps, "results": out}))


if __name__ == "__main__":
    main()
