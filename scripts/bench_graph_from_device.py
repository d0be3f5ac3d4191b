"""The match graph built on the GPU (lfr_graph_from_device_arrays, Graph.from_device_arrays) against the host numbering over the same
arrays (lfr_graph_from_arrays_device_flows, Graph.from_device_flows), and a refine() forward through each of the two roads: on
config 4 and on the long-track workload (config 5), one process per workload and kind of measurement, warm, medians over
LFR_BENCH_REPS (default 20) repetitions; a host clock around the call and a device synchronise, the roads alternating inside one loop.
The host road is timed twice: the bare call with the similarities already on the host, and with their copy from the device in front
(what refine() paid).  The new call's spans (host pair table, host mirror and finish() by the host clock; expand, sort, head flags +
prefix sums, heads + scatter by device events) come from a process of their own under LFR_GRAPHBUILD_SPANS=1 - the switch adds a
stream wait, so the call's own time is taken without it.
Gate: on config 4 the new call is faster than from_device_flows in the same process.
Prints one JSON line and writes it to profiles/graph_from_device_bench.json (or to the path given as the first argument)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-feature-refinement_amd"))


def measure(name, reps, warmup=3):
    os.environ["LFR_GRAPHBUILD_SPANS"] = "0"      # (the library reads it once, at its first such call: the spans have a process of their own)
    import numpy as np
    import torch

    from lfr_amd import capi, synthetic
    from lfr_amd.autograd import refine
    from lfr_amd.synthetic import MatchArrays

    dev = torch.device("cuda", 0)
    ma = getattr(synthetic, name)()
    M = int(ma.n_matches)
    d1 = torch.as_tensor(np.asarray(ma.disp1, np.float32).reshape(-1, 18)).to(dev)
    d2 = torch.as_tensor(np.asarray(ma.disp2, np.float32).reshape(-1, 18)).to(dev)
    sim = torch.as_tensor(np.asarray(ma.sim, np.float32)).to(dev)
    f1 = torch.as_tensor(np.ascontiguousarray(ma.feat1, np.uint32).view(np.int32)).to(dev)
    f2 = torch.as_tensor(np.ascontiguousarray(ma.feat2, np.uint32).view(np.int32)).to(dev)
    host_only = MatchArrays(image_names=ma.image_names, facts=ma.facts, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off,
                            feat1=None, feat2=None, sim=None, disp1=None, disp2=None)
    meta = dict(image_names=ma.image_names, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off, image_facts=ma.facts)
    torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def from_flows():        # what refine() paid before: the similarities to the host, then the host numbering
        m = MatchArrays(image_names=ma.image_names, facts=ma.facts, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off,
                        feat1=ma.feat1, feat2=ma.feat2, sim=sim.cpu().numpy(), disp1=None, disp2=None)
        return capi.Graph.from_device_flows(m, d1.data_ptr(), d2.data_ptr(), 0)

    sim_host = sim.cpu().numpy()
    m_bare = MatchArrays(image_names=ma.image_names, facts=ma.facts, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off,
                         feat1=ma.feat1, feat2=ma.feat2, sim=sim_host, disp1=None, disp2=None)

    def from_flows_bare():   # the host numbering alone: the similarities are on the host already
        return capi.Graph.from_device_flows(m_bare, d1.data_ptr(), d2.data_ptr(), 0)

    def from_arrays():
        return capi.Graph.from_device_arrays(host_only, f1.data_ptr(), f2.data_ptr(), sim.data_ptr(), d1.data_ptr(), d2.data_ptr(), 0)

    t_bare, t_flows, t_arrays, t_ref_host, t_ref_dev = [], [], [], [], []
    n_nodes = 0
    for it in range(warmup + reps):
        e, gc = timed(from_flows_bare)
        a, ga = timed(from_flows)
        b, gb = timed(from_arrays)
        if it == 0:
            assert ga.n_nodes == gb.n_nodes and all((x == y).all() for x, y in zip(ga.nodes(), gb.nodes())), "the two graphs differ"
            n_nodes = int(gb.n_nodes)
        gc.close()
        ga.close()
        gb.close()
        c, ph = timed(lambda: refine(d1, d2, sim, feat1=ma.feat1, feat2=ma.feat2, **meta)[0])
        d, pd = timed(lambda: refine(d1, d2, sim, feat1=f1, feat2=f2, **meta)[0])
        if it == 0:
            assert torch.equal(ph, pd), "refine() differs between the two roads"
        del ph, pd
        if it >= warmup:
            t_bare.append(e), t_flows.append(a), t_arrays.append(b), t_ref_host.append(c), t_ref_dev.append(d)
    med = lambda v: float(np.median(v))
    return {"workload": name, "matches": M, "pairs": int(len(ma.pair_img1)), "nodes": n_nodes,
            "from_device_flows_ms_median": med(t_bare), "from_device_flows_ms_min": float(np.min(t_bare)),
            "sim_to_host_plus_from_device_flows_ms_median": med(t_flows), "sim_to_host_plus_from_device_flows_ms_min": float(np.min(t_flows)),
            "from_device_arrays_ms_median": med(t_arrays), "from_device_arrays_ms_min": float(np.min(t_arrays)),
            "flows_over_arrays": med(t_bare) / med(t_arrays),
            "refine_forward_host_numbering_ms_median": med(t_ref_host), "refine_forward_device_numbering_ms_median": med(t_ref_dev),
            "refine_host_over_device": med(t_ref_host) / med(t_ref_dev)}


def measure_spans(name, reps, warmup=3):
    os.environ["LFR_GRAPHBUILD_SPANS"] = "1"
    import numpy as np
    import torch

    from lfr_amd import capi, synthetic
    from lfr_amd.synthetic import MatchArrays

    dev = torch.device("cuda", 0)
    ma = getattr(synthetic, name)()
    t = [torch.as_tensor(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev) for a in (ma.feat1, ma.feat2)]
    t.append(torch.as_tensor(np.asarray(ma.sim, np.float32)).to(dev))
    t += [torch.as_tensor(np.asarray(d, np.float32).reshape(-1, 18)).to(dev) for d in (ma.disp1, ma.disp2)]
    host_only = MatchArrays(image_names=ma.image_names, facts=ma.facts, pair_img1=ma.pair_img1, pair_img2=ma.pair_img2, pair_off=ma.pair_off,
                            feat1=None, feat2=None, sim=None, disp1=None, disp2=None)
    torch.cuda.synchronize()
    rows = []
    for it in range(warmup + reps):
        capi.Graph.from_device_arrays(host_only, *[x.data_ptr() for x in t], 0).close()
        if it >= warmup:
            rows.append(capi.Graph.build_spans())
    return {k + "_ms_median": float(np.median([r[k] for r in rows])) for k in rows[0]}


def main():
    reps = int(os.environ.get("LFR_BENCH_REPS", "20"))
    if len(sys.argv) > 2 and sys.argv[1] in ("--workload", "--spans"):      # a child: one workload, one JSON line
        fn = measure if sys.argv[1] == "--workload" else measure_spans
        print("RESULT " + json.dumps(fn(sys.argv[2], reps)), flush=True)
        return
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "graph_from_device_bench.json")
    results = []
    for name in ("config4", "config5"):
        res = {}
        for mode in ("--workload", "--spans"):
            text = subprocess.run([sys.executable, os.path.abspath(__file__), mode, name], check=True, stdout=subprocess.PIPE, text=True,
                                  timeout=600).stdout        # (a child that fails or hangs ends the run: nothing else is started)
            line = [ln for ln in text.splitlines() if ln.startswith("RESULT ")][-1]
            res.update({"spans": json.loads(line[7:])} if mode == "--spans" else json.loads(line[7:]))
        results.append(res)
    out = {"reps": reps, "results": results,
           "gate_config4_new_call_faster": results[0]["from_device_arrays_ms_median"] < results[0]["from_device_flows_ms_median"]}
    line = json.dumps(out)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)
    if not out["gate_config4_new_call_faster"]:
        sys.exit("gate missed: on config 4 from_device_arrays is not faster than from_device_flows")


if __name__ == "__main__":
    main()
