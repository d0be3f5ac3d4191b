"""A training step's forward on a live batch (lfr_batch_set_inputs, lfr_amd.autograd.Refiner) against the same step through refine(),
which builds graph, problem and batch anew: on config 4 and on the long-track workload (config 5), warm, medians over LFR_BENCH_REPS
(default 20) steps.  Per workload:
  (a) lfr_batch_set_inputs alone, by device events on the stream, with the bytes it has to move and their share of the HBM peak;
  (b) Refiner forward (set_inputs + solve + positions), host clock around the call and a device synchronise;
  (c) refine() with the same values, measured the same way - (b) and (c) alternate inside one loop.
Prints one JSON line and writes it to profiles/set_inputs_bench.json (or to the path given as the first argument)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-feature-refinement_amd"))

import numpy as np
import torch

from lfr_amd import capi, synthetic
from lfr_amd.autograd import Refiner, refine

HBM_PEAK = 8.0e12           # bytes / s (MI355X)
DEV = torch.device("cuda", 0)


def measure(name, ma, reps, warmup=3):
    meta = dict(image_names=ma.image_names, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off, feat1=ma.feat1,
                feat2=ma.feat2, image_facts=ma.facts)
    rng = np.random.default_rng(0)
    sim = torch.as_tensor(ma.sim).to(DEV)
    # two sets of flows, alternating, so that every step really changes the records: the generator's own, and those plus noise of
    # the generator's size
    flows = []
    for k in range(2):
        flows.append(tuple(torch.as_tensor((d + rng.normal(0.0, 0.02 * k, size=d.shape)).astype(np.float32).reshape(-1, 18)).to(DEV)
                           for d in (ma.disp1, ma.disp2)))
    r = Refiner(flows[0][0], flows[0][1], sim, **meta)
    b = r._batch
    b.solve()
    n_rec = int(b.component_info()["n_edges"].sum())
    # per record: its edge id, one 72-byte flow row, the similarity and the record's last word in; 80 bytes out
    bytes_all = n_rec * (4 + 72 + 4 + 4 + 80)
    bytes_sim = n_rec * (4 + 4 + 4)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    solve_ms, set_all, set_flows, set_sim, fwd_refiner, fwd_refine = [], [], [], [], [], []
    for it in range(warmup + reps):
        d1, d2 = flows[it & 1]
        for kw, acc in (({"disp1": d1, "disp2": d2, "sim": sim}, set_all), ({"disp1": d1, "disp2": d2}, set_flows), ({"sim": sim}, set_sim)):
            e0.record()
            b.set_inputs(**kw)
            e1.record()
            e1.synchronize()
            if it >= warmup:
                acc.append(e0.elapsed_time(e1))
        st = b.solve()
        if it >= warmup:
            solve_ms.append(st["kernel_ms"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pos = r(d1, d2)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ref = refine(d1, d2, sim, **meta)[0]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if it >= warmup:
            fwd_refiner.append(1e3 * (t1 - t0))
            fwd_refine.append(1e3 * (t2 - t1))
        if it == 0:
            assert torch.equal(pos, ref), "Refiner and refine() disagree"
        del ref
    med = lambda v: float(np.median(v))
    out = {"workload": name, "matches": int(ma.n_matches), "records": n_rec,
           "set_inputs_ms_median": med(set_all), "set_inputs_ms_min": float(np.min(set_all)),
           "set_inputs_bytes": bytes_all, "set_inputs_share_of_hbm_peak": bytes_all / (1e-3 * med(set_all)) / HBM_PEAK,
           "set_inputs_flows_only_ms_median": med(set_flows),
           "set_inputs_sim_only_ms_median": med(set_sim), "set_inputs_sim_only_bytes": bytes_sim,
           "solve_kernel_ms_median": med(solve_ms),
           "refiner_forward_wall_ms_median": med(fwd_refiner), "refine_forward_wall_ms_median": med(fwd_refine),
           "refine_over_refiner": med(fwd_refine) / med(fwd_refiner)}
    r.close()
    return out


def main():
    reps = int(os.environ.get("LFR_BENCH_REPS", "20"))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "set_inputs_bench.json")
    out = {"reps": reps, "results": [measure("config4", synthetic.config4(), reps), measure("config5", synthetic.config5(), reps)]}
    line = json.dumps(out)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
