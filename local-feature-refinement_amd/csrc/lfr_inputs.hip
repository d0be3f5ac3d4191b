// New flows and similarities into a live batch (lfr_batch_set_inputs, include/lfr.h), and the record -> directed-edge
// map that it shares with the backward pass.  A translation unit of its own: it rewrites EdgeRec::flow / EdgeRec::sim of the batch's
// records in place and touches nothing else the solve reads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "lfr_assemble.hpp"
#include "lfr_batch.hpp"

using lfr::CompDesc;
using lfr::EdgeRec;

namespace {

enum : int { kSetAll = 0, kSetFlows = 1, kSetSim = 2 };

// One thread per (record, 16-byte chunk) - per record in the similarity-only form: record p is directed edge eid[p] of the graph and
// takes the flow row of its match from disp2 (even ids) or disp1 (odd ids) and the match's similarity.  The last word of the record
// (local indices and kind) is structure: the full form stores it back as it found it, the other two never touch its chunk's tail.
// A flow row is 72 bytes, so 8-byte aligned when the arrays are (ALIGNED8; a caller's tensor view may start on any float).
template <int MODE, bool ALIGNED8>
__global__ __launch_bounds__(256) void k_set_inputs(uint32_t n_records, const uint32_t *eid, const float *disp1, const float *disp2,
                                                    const float *sim, uint32_t n_matches, EdgeRec *records) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (MODE == kSetSim) {
        if (t >= n_records) return;
        const uint32_t m = eid[t] >> 1;
        if (m < n_matches) records[t].sim = sim[m];
        return;
    }
    const uint64_t p = t / 5;
    const int chunk = (int)(t - 5 * p);
    if (p >= n_records) return;
    const uint32_t id = eid[p], m = id >> 1;
    if (m >= n_matches) return;                               // (cannot happen: every record maps to an edge of the graph)
    const float *fl = ((id & 1u) ? disp1 : disp2) + 18 * (size_t)m;
    uint4 *rec = reinterpret_cast<uint4 *>(records + p);
    uint4 q;
    if (chunk < 4) {
        if (ALIGNED8) {
            const uint2 a = reinterpret_cast<const uint2 *>(fl)[2 * chunk], b = reinterpret_cast<const uint2 *>(fl)[2 * chunk + 1];
            q.x = a.x; q.y = a.y; q.z = b.x; q.w = b.y;
        } else {
            q.x = __float_as_uint(fl[4 * chunk]); q.y = __float_as_uint(fl[4 * chunk + 1]);
            q.z = __float_as_uint(fl[4 * chunk + 2]); q.w = __float_as_uint(fl[4 * chunk + 3]);
        }
        rec[chunk] = q;
        return;
    }
    q.x = __float_as_uint(fl[16]); q.y = __float_as_uint(fl[17]);
    if (MODE == kSetFlows) {
        *reinterpret_cast<uint2 *>(rec + 4) = make_uint2(q.x, q.y);
    } else {
        q.z = __float_as_uint(sim[m]);
        q.w = reinterpret_cast<const uint32_t *>(rec + 4)[3];
        rec[4] = q;
    }
}

__global__ void k_record_words(uint32_t n, const EdgeRec *edges, uint32_t *words) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) words[p] = (uint32_t)edges[p].src | ((uint32_t)edges[p].dst_kind << 16);
}

template <int MODE>
void launch_set_inputs(bool aligned8, uint32_t n, const uint32_t *eid, const float *d1, const float *d2, const float *sim, uint32_t M,
                       EdgeRec *records, hipStream_t st) {
    const uint64_t threads = MODE == kSetSim ? (uint64_t)n : (uint64_t)5 * n;
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (aligned8) hipLaunchKernelGGL((k_set_inputs<MODE, true>), grid, dim3(256), 0, st, n, eid, d1, d2, sim, M, records);
    else hipLaunchKernelGGL((k_set_inputs<MODE, false>), grid, dim3(256), 0, st, n, eid, d1, d2, sim, M, records);
}

}  // namespace

// record -> directed edge of the graph for batches without edge_ref: the records of a component come in the reference's residual-block
// order (solve.cc:98-102: by source node, a node's out-edges in insertion order = ascending directed-edge id) or, in the packed
// classes, in edge-id order - either way the records of one source node ascend in edge id - and a kept edge is kept for its two end
// points' labels alone, so the k-th record from s to t is the k-th out-edge of s that ends at t.
// One map per batch: whichever of lfr_batch_backward and lfr_batch_set_inputs comes first builds it, the other finds it.
int lfr::ensure_edge_map(lfr_batch *b) {
    if (b->d_edge_ref || b->d_eid) return LFR_OK;
    if (!b->graph || !lfr::graph_alive(b->graph, b->graph_serial)) {
        lfr::set_error("the batch maps its records to the graph's edges on first use, and its graph has been freed");
        return LFR_ERR_ARG;
    }
    int rc = lfr::ensure_mirrors(b);
    if (rc != LFR_OK) return rc;
    const lfr::Graph *g = b->graph;
    const size_t ne = (size_t)b->n_edges;
    std::vector<uint32_t> words(ne), eid(ne, 0);
    hipStream_t st = b->ctx->s_main;
    if (!b->map_slab.init(b->ctx, 4 * std::max<size_t>(ne, 1) + 4096)) return LFR_ERR_NOMEM;
    struct Guard { lfr_batch *b; bool keep; ~Guard() { if (!keep) b->map_slab.reset(); } } guard{b, false};
    uint32_t *d_eid = b->map_slab.take_n<uint32_t>(ne);
    if (!d_eid) { lfr::set_error("edge-map slab exhausted"); return LFR_ERR_NOMEM; }
    if (ne) {
        // The words are structure, written once when the batch was made (creation ends with a host wait for the upload / the assembly).
        // Still, order this read behind everything that stores into the records' last chunk: a full-form k_set_inputs of another
        // stream stores the word back with the value it found.  (The map's own array serves as the staging area.)
        if (b->n_solves > 0) HIP_TRY(hipStreamWaitEvent(st, b->ev[1], 0));
        if (b->inputs_epoch > 0) HIP_TRY(hipStreamWaitEvent(st, b->ev_inputs, 0));
        hipLaunchKernelGGL(k_record_words, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, (uint32_t)ne, b->d_edges, d_eid);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(words.data(), d_eid, 4 * ne, hipMemcpyDeviceToHost, st));
        HIP_TRY(lfr::stream_wait(st));
    }
    std::vector<int64_t> out_off, out_eid;
    lfr::build_out_csr(*g, out_off, out_eid);
    std::vector<int64_t> cursor(out_off.begin(), out_off.end() - 1);
    auto dst_of = [&](int64_t e) -> uint32_t { return (e & 1) ? g->m_node1[e >> 1] : g->m_node2[e >> 1]; };
    for (const CompDesc &dsc : b->descs) {
        for (uint32_t p = dsc.edge_off; p < dsc.edge_off + dsc.n_edges; ++p) {
            const uint32_t sl = words[p] & 0xffffu, tl = (words[p] >> 16) & 0x7fffu;
            const uint32_t s = b->node_ids[dsc.node_off + sl], t = b->node_ids[dsc.node_off + tl];
            int64_t &c = cursor[s];
            while (c < out_off[s + 1] && dst_of(out_eid[c]) != t) ++c;
            if (c >= out_off[s + 1]) { lfr::set_error("record %u has no edge in the graph", p); return LFR_ERR_ARG; }
            eid[p] = (uint32_t)out_eid[c++];
        }
    }
    if (ne) {
        HIP_TRY(hipMemcpyAsync(d_eid, eid.data(), 4 * ne, hipMemcpyHostToDevice, st));
        HIP_TRY(lfr::stream_wait(st));
    }
    guard.keep = true;
    b->d_eid = d_eid;
    return LFR_OK;
}

extern "C" {

int lfr_batch_set_inputs(lfr_batch *b, const float *disp1_device, const float *disp2_device, const float *sim_device, void *hip_stream) {
    if (!b) { lfr::set_error("lfr_batch_set_inputs: no batch"); return LFR_ERR_ARG; }
    if (!disp1_device && !disp2_device && !sim_device) { lfr::set_error("lfr_batch_set_inputs: nothing to set (all three inputs are NULL)"); return LFR_ERR_ARG; }
    if (!disp1_device != !disp2_device) { lfr::set_error("lfr_batch_set_inputs: disp1 and disp2 go together (both or neither)"); return LFR_ERR_ARG; }
    if (b->cc_sharded) {
        lfr::set_error("lfr_batch_set_inputs: a batch over one rank's connected components numbers its matches by itself (lfr_problem_build_hip_shard)");
        return LFR_ERR_UNSUPPORTED;
    }
    HIP_TRY(hipSetDevice(b->device));
    if (!b->d_edge_ref && !b->d_eid) { const int rc = lfr::ensure_edge_map(b); if (rc != LFR_OK) return rc; }
    if (!b->ev_inputs && !(b->ev_inputs = b->ctx->event_acquire(false))) return LFR_ERR_HIP;
    hipStream_t st = (hipStream_t)hip_stream;
    // everything that reads the records: the latest solve, backward, covariance, evaluate, evaluate_vjp, jvp, hessian_product and hessian_solve, whatever streams they ran on
    if (b->n_solves > 0) HIP_TRY(hipStreamWaitEvent(st, b->ev[1], 0));
    for (const lfr::PassState *pass : {b->bwd, b->cov, b->eval, b->evjp, b->jvp, b->hvp, b->hsolve})
        if (hipEvent_t e = lfr::pass_last_event(pass)) HIP_TRY(hipStreamWaitEvent(st, e, 0));
    if (b->inputs_epoch > 0 && b->inputs_stream != st) HIP_TRY(hipStreamWaitEvent(st, b->ev_inputs, 0));
    if (b->fused) {          // complete records first (words, and whichever of flows / similarity this call keeps), from the graph's arrays
        lfr::materialize_records(b, st);
        HIP_TRY(hipGetLastError());
        b->fused = false;    // from here on the solve, the backward and the covariance read d_edges
        // (dev_hold stays, as it does after the second solve of a fused batch: the launch above still reads the graph's arrays, the
        // problem holds the same reference anyway, and letting go later would need an event to ask)
    }
    const uint32_t n = (uint32_t)b->n_edges, M = (uint32_t)b->n_graph_matches;
    const uint32_t *eid = lfr::edge_map(b);
    if (n) {
        const bool aligned8 = (((uintptr_t)disp1_device | (uintptr_t)disp2_device) & 7u) == 0;
        if (!disp1_device) launch_set_inputs<kSetSim>(true, n, eid, nullptr, nullptr, sim_device, M, b->d_edges, st);
        else if (!sim_device) launch_set_inputs<kSetFlows>(aligned8, n, eid, disp1_device, disp2_device, nullptr, M, b->d_edges, st);
        else launch_set_inputs<kSetAll>(aligned8, n, eid, disp1_device, disp2_device, sim_device, M, b->d_edges, st);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(b->ev_inputs, st));
    b->inputs_stream = st;
    b->inputs_pending = true;
    ++b->inputs_epoch;
    return LFR_OK;
}

}  // extern "C"
