"""HIP-event times of the forward solve, the implicit-gradient backward and the per-keypoint covariance (lfr_batch_covariance), warm,
median of 20 repetitions in one process, on config 4, config 5 and the cap-sized sparse workload, plus the covariance's status
counts.  Writes profiles/covariance_bench.json (or the path given) and prints it.  (bench.py stays the measure of the forward.)

The gate of the packed layout: on config 4 the covariance must take less time than the backward on the same batch in this run."""
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
    b.solve()                                      # warm: records materialised, workspaces set up below
    b.backward(gp, want_stats=True)
    _, st = b.covariance(want_stats=True)
    fwd, bwd, cov = [], [], []
    for _ in range(reps):
        fwd.append(b.solve()["kernel_ms"])
        bwd.append(b.backward(gp, want_stats=True)[3]["kernel_ms"])
        cov.append(b.covariance(want_stats=True)[1]["kernel_ms"])
    info = b.component_info()
    f, w, c = float(np.median(fwd)), float(np.median(bwd)), float(np.median(cov))
    return {"workload": name, "components": int(len(info["component"])), "max_rows": int(2 * info["n_var_nodes"].max()), "reps": reps,
            "forward_ms_median": f, "backward_ms_median": w, "covariance_ms_median": c,
            "forward_ms_min": float(np.min(fwd)), "backward_ms_min": float(np.min(bwd)), "covariance_ms_min": float(np.min(cov)),
            "covariance_over_backward": c / w, "covariance_over_forward": c / f,
            "n_computed": st["n_computed"], "n_not_usable": st["n_not_usable"], "n_singular": st["n_singular"]}


def main():
    reps = int(os.environ.get("LFR_BENCH_REPS", "20"))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "covariance_bench.json")
    out = [measure("config4", synthetic.config4(), reps, True),
           measure("config5", synthetic.config5(), reps, False),
           measure("capsized_sparse", synthetic.capsized_sparse(), reps, False)]
    res = {"device": torch.cuda.get_device_name(0), "results": out,
           "gate_config4_covariance_faster_than_backward": bool(out[0]["covariance_ms_median"] < out[0]["backward_ms_median"])}
    text = json.dumps(res, indent=1)
    with open(path, "w") as fh:
        fh.write(text + "\n")
    print(text)
    if not res["gate_config4_covariance_faster_than_backward"]:
        sys.exit("config 4: the covariance (%.3f ms) is not faster than the backward (%.3f ms)"
                 % (out[0]["covariance_ms_median"], out[0]["backward_ms_median"]))


if __name__ == "__main__":
    main()
