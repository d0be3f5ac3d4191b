// The batch behind the C ABI (include/lfr.h): creation (device- or host-assembled), the workspace of the workgroup classes, the launch
// plan of lfr_batch_solve with its diagnostic read-backs and statistics, the state that the passes behind a solve share (PassState),
// timing, downloads, warm-up / reserve and the multi-GPU entry points.  The forward kernels live in
// lfr_solve.hip and are reached through the launch functions of lfr_batch.hpp; this file holds only the small utility kernels of the
// host code (k_materialize_records, k_wg_order_keys, k_place_plans, k_positions_to_f32, k_occupy).  lfr_batch_set_inputs: lfr_inputs.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <array>
#include <chrono>
#include <memory>
#include <string>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lfr_assemble.hpp"
#include "lfr_batch.hpp"
#include "lfr_hessian_device.hpp"
#include "lfr_internal.hpp"

using lfr::CompDesc;
using lfr::CompInfoDev;
using lfr::EdgeRec;
using lfr::KernelArgs;
using lfr::PackedRanges;
using lfr::block_lds_bytes;
using lfr::ensure_mirrors;

namespace {

// A fused batch solved a SECOND time: its packed-class records are materialised once (one thread per 16-byte chunk) and every
// later solve reads them - contiguous 80-byte records cost the packed kernel 10 % less than the gather (0.49 against 0.54 ms on
// config 4), while a one-shot pipeline (one solve per batch) never pays for writing and re-reading 400 MB.
__global__ void k_materialize_records(uint32_t n_records, const uint32_t *edge_ref, const uint32_t *edge_word, const uint32_t *f_row,
                                      const float *disp1, const float *disp2, const float *sim, uint4 *records) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t p = t / 5;
    const int chunk = (int)(t - 5 * p);
    if (p >= n_records) return;
    const uint32_t eid = edge_ref[p], m = eid >> 1;
    const size_t row = f_row ? (size_t)f_row[m] : (size_t)m;
    const float *fl = ((eid & 1u) ? disp1 : disp2) + 18 * row;
    uint4 q;
    if (chunk < 4) {
        const uint2 a = reinterpret_cast<const uint2 *>(fl)[2 * chunk], b = reinterpret_cast<const uint2 *>(fl)[2 * chunk + 1];
        q.x = a.x; q.y = a.y; q.z = b.x; q.w = b.y;
    } else {
        q.x = __float_as_uint(fl[16]); q.y = __float_as_uint(fl[17]); q.z = __float_as_uint(sim[m]); q.w = edge_word[p];
    }
    records[5 * p + chunk] = q;
}

// Order in which a class hands out its components: by expected duration, longest first.  The batch order inside a class is by
// edge count, which predicts a workgroup's lifetime hardly better than a random order (list-scheduling the measured lifetimes of
// the config-5 class of 131-192 rows on 256 CUs: 6.9 ms by edges, 6.6 random, 4.9 with the lifetimes known).  Rows (the
// factorization is cubic in them) and whether the component joins several tracks (its Tukey edges cost iterations: 6.3 against
// 4.2 on average, Spearman 0.58) give 5.8 ms.  key = class, then rows x (1 + [more than one track]) descending; a component
// has one constant node (the root) per track.
__global__ void k_wg_order_keys(const CompDesc *descs, int n, int b1, int b2, int b3, uint32_t *keys, uint32_t *vals, int wg_begin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const CompDesc d = descs[i];
    const uint32_t cls = (i >= b1) + (i >= b2) + (i >= b3);                   // boundaries of the four classes, relative
    const uint32_t work = (uint32_t)d.n_var * (1u + ((uint32_t)d.n_nodes - d.n_var > 1u ? 1u : 0u));
    keys[i] = (cls << 24) | (0xffffffu - min(work, 0xffffffu));
    vals[i] = (uint32_t)(wg_begin + i);
}

// LFR_HOST_TRACE=1: host-side time stamps (us, steady clock) of the calls that make the Solver span, to stderr
static inline void host_trace(const char *what) {
    static const bool on = [] { const char *e = getenv("LFR_HOST_TRACE"); return e && e[0] == '1'; }();
    if (!on) return;
    static const auto t0 = std::chrono::steady_clock::now();
    fprintf(stderr, "lfr-host %10.1f us  %s\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), what);
}

}  // namespace

// host mirrors of a device-assembled batch (descriptors, component ids, classes, node ids): 2-6 MB, fetched once
int lfr::ensure_mirrors(lfr_batch *b) {
    if (b->mirrors_valid) return LFR_OK;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = b->ctx->s_main;
    const size_t nd = (size_t)b->n_desc, nn = (size_t)b->n_nodes;
    b->descs.resize(nd); b->desc_component.resize(nd); b->desc_class.resize(nd); b->desc_tracks.resize(nd);
    b->node_ids.resize(nn);
    std::vector<uint32_t> comp(nd), cls(nd), trk(nd);
    if (nd) {
        HIP_TRY(hipMemcpyAsync(b->descs.data(), b->d_descs, nd * sizeof(CompDesc), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(comp.data(), b->d_desc_component, 4 * nd, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(cls.data(), b->d_desc_class, 4 * nd, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(trk.data(), b->d_desc_tracks, 4 * nd, hipMemcpyDeviceToHost, st));
    }
    if (nn) HIP_TRY(hipMemcpyAsync(b->node_ids.data(), b->d_node_ids, 4 * nn, hipMemcpyDeviceToHost, st));
    HIP_TRY(lfr::stream_wait(st));
    for (size_t i = 0; i < nd; ++i) { b->desc_component[i] = comp[i]; b->desc_class[i] = (int32_t)cls[i]; b->desc_tracks[i] = (int32_t)trk[i]; }
    b->mirrors_valid = true;
    return LFR_OK;
}

void lfr::materialize_records(lfr_batch *b, hipStream_t st) {
    if (!b->packed_edges) return;
    const lfr::DevGraph &dgr = *b->dev_hold->graph;
    hipLaunchKernelGGL(k_materialize_records, dim3((unsigned)(((uint64_t)5 * b->packed_edges + 255) / 256)), dim3(256), 0, st, b->packed_edges,
                       b->d_edge_ref, b->d_edge_word, dgr.flow_row, dgr.disp1, dgr.disp2, dgr.sim, reinterpret_cast<uint4 *>(b->d_edges));
}

// =============================================================================================
// the packed launch's blocks; the state of a pass that runs after a solve (lfr_batch.hpp)
// =============================================================================================
void lfr::packed_ranges(const lfr_batch *b, int waves_per_block, PackedRanges *r, int *n_blocks) {
    int nb = 0;
    for (int i = 0; i < lfr::kPackedClasses; ++i) {
        const int cls = lfr::kPackedOrder[i], per_block = lfr::kPackedClass[cls].G() * waves_per_block;
        r->blk_begin[i] = nb;
        r->desc_begin[i] = b->class_begin[cls]; r->desc_end[i] = b->class_begin[cls + 1];
        nb += (r->desc_end[i] - r->desc_begin[i] + per_block - 1) / per_block;
    }
    r->blk_begin[lfr::kPackedClasses] = nb;
    *n_blocks = nb;
}

void lfr::pass_free(PassState *s) {
    if (!s) return;
    if (s->last_stream || s->n_calls) (void)hipStreamSynchronize(s->last_stream);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    delete s;
}

hipEvent_t lfr::pass_last_event(const PassState *s) { return s && s->n_calls ? s->ev1 : nullptr; }

namespace {
// first call of a pass on this batch: the dense triangles of the components above the LDS classes live in HBM, one status per descriptor
int pass_setup(lfr_batch *b, lfr::PassState **slot, const lfr::PassKind &kind, size_t extra_bytes) {
    int rc = ensure_mirrors(b);
    if (rc != LFR_OK) return rc;
    std::unique_ptr<lfr::PassState, void (*)(lfr::PassState *)> s(kind.make(), lfr::pass_free);      // every error path releases slab and events
    const size_t nd = std::max<size_t>(b->descs.size(), 1);
    std::vector<uint64_t> off(nd, 0);
    uint64_t hws = 0;
    for (size_t i = 0; i < b->descs.size(); ++i) {
        const int cls = b->desc_class[i], rows = 2 * b->descs[i].n_var;
        s->rows_max[cls] = std::max(s->rows_max[cls], rows);
        if (cls == lfr::KC_GLOBAL) {
            if (rows > lfrdev::kBwdMaxRows) { lfr::set_error("%s: a component of %d rows exceeds the dense factorization's %d", kind.name, rows, lfrdev::kBwdMaxRows); return LFR_ERR_UNSUPPORTED; }
            off[i] = hws; hws += lfrdev::bwd_tri(rows, 0);
        }
    }
    if (!s->slab.init(b->ctx, extra_bytes + 8 * hws + 8 * nd + 4 * nd + ((size_t)1 << 16))) return LFR_ERR_NOMEM;
    s->d_hws = s->slab.take_n<double>(std::max<uint64_t>(hws, 1));
    s->d_hws_off = s->slab.take_n<uint64_t>(nd);
    s->d_status = s->slab.take_n<int32_t>(nd);
    if (!s->d_hws || !s->d_hws_off || !s->d_status) { lfr::set_error("%s slab exhausted", kind.name); return LFR_ERR_NOMEM; }
    HIP_TRY(hipEventCreate(&s->ev0)); HIP_TRY(hipEventCreate(&s->ev1));
    hipStream_t st = b->ctx->s_main;
    HIP_TRY(hipMemcpyAsync(s->d_hws_off, off.data(), 8 * nd, hipMemcpyHostToDevice, st));
    HIP_TRY(lfr::stream_wait(st));
    if ((rc = kind.extra(b, s.get())) != LFR_OK) return rc;
    *slot = s.release();
    return LFR_OK;
}
}  // namespace

int lfr::pass_begin(lfr_batch *b, PassState **slot, const PassKind &kind, size_t extra_bytes, hipStream_t st) {
    if (b->n_solves == 0) { lfr::set_error("lfr_batch_%s: the batch has not been solved", kind.name); return LFR_ERR_ARG; }
    if (b->inputs_epoch != b->solved_epoch) { lfr::set_error("lfr_batch_%s: inputs changed since the latest solve", kind.name); return LFR_ERR_ARG; }
    HIP_TRY(hipSetDevice(b->device));
    if (!*slot) { const int rc = pass_setup(b, slot, kind, extra_bytes); if (rc != LFR_OK) return rc; }
    HIP_TRY(hipStreamWaitEvent(st, b->ev[1], 0));                               // the latest solve's positions and termination codes
    HIP_TRY(hipEventRecord((*slot)->ev0, st));
    return LFR_OK;
}

// first call of a pass that needs no solve: no workspace for matrices, no status words - a slab for the pass's own carvings
// (kind.extra makes them) and the two events
int lfr::pass_setup_unsolved(lfr_batch *b, PassState **slot, const PassKind &kind, size_t slab_bytes) {
    std::unique_ptr<lfr::PassState, void (*)(lfr::PassState *)> s(kind.make(), lfr::pass_free);      // every error path releases slab and events
    if (!s->slab.init(b->ctx, slab_bytes)) return LFR_ERR_NOMEM;
    { const int rc = kind.extra(b, s.get()); if (rc != LFR_OK) return rc; }
    HIP_TRY(hipEventCreate(&s->ev0)); HIP_TRY(hipEventCreate(&s->ev1));
    *slot = s.release();
    return LFR_OK;
}

int lfr::pass_end(PassState *s, hipStream_t st) {
    HIP_TRY(hipEventRecord(s->ev1, st));
    s->last_stream = st;
    ++s->n_calls;
    return LFR_OK;
}

// What the passes that need no solve (lfr_batch.hpp) do before their launches: wait by event for the latest solve and the latest
// lfr_batch_set_inputs, record the pass's ev0, and write the packed records of a device-assembled batch that still gathers them from
// the graph's arrays
int lfr::eval_prologue(lfr_batch *b, PassState &s, hipStream_t st) {
    // the latest solve (positions; a second solve of a fused batch wrote the records) and the latest set_inputs, whatever streams they ran on
    if (b->n_solves > 0) HIP_TRY(hipStreamWaitEvent(st, b->ev[1], 0));
    if (b->ev_inputs && (b->inputs_epoch > 0 || b->inputs_pending)) HIP_TRY(hipStreamWaitEvent(st, b->ev_inputs, 0));
    HIP_TRY(hipEventRecord(s.ev0, st));
    if (b->fused) {          // the packed records have not been written yet: write them, as lfr_batch_set_inputs does - one record-reading kernel only
        if (!b->ev_inputs && !(b->ev_inputs = b->ctx->event_acquire(false))) return LFR_ERR_HIP;
        lfr::materialize_records(b, st);
        HIP_TRY(hipGetLastError());
        b->fused = false;
        // the next solve reads these records, possibly on another stream: it waits for them as for new inputs (the values are the
        // graph's own, so the inputs epoch does not move and backward / covariance keep running)
        HIP_TRY(hipEventRecord(b->ev_inputs, st));
        b->inputs_stream = st;
        b->inputs_pending = true;
    }
    return LFR_OK;
}

int lfr::pass_wait_ms(PassState *s, hipStream_t st, double *kernel_ms) {
    HIP_TRY(lfr::stream_wait(st));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    *kernel_ms = ms;
    return LFR_OK;
}

int64_t lfr::pass_status(lfr_batch *b, PassState *s, const char *name, int32_t *status) {
    if (!b || !s || !s->n_calls) { lfr::set_error("lfr_batch_%s_status: no %s has run on this batch", name, name); return LFR_ERR_ARG; }
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipEventSynchronize(s->ev1));
    const size_t n = b->descs.size();
    if (status && n) {
        HIP_TRY(hipMemcpyAsync(status, s->d_status, 4 * n, hipMemcpyDeviceToHost, s->last_stream));
        HIP_TRY(lfr::stream_wait(s->last_stream));
    }
    return (int64_t)n;
}

int lfr::pass_histogram(lfr_batch *b, PassState *s, hipStream_t st, int64_t count[3], double *kernel_ms) {
    HIP_TRY(hipEventSynchronize(s->ev1));
    std::vector<int32_t> status(b->descs.size());
    if (!status.empty()) HIP_TRY(hipMemcpyAsync(status.data(), s->d_status, 4 * status.size(), hipMemcpyDeviceToHost, st));
    { const int rc = lfr::pass_wait_ms(s, st, kernel_ms); if (rc != LFR_OK) return rc; }
    count[0] = count[1] = count[2] = 0;
    for (int32_t v : status) ++count[(v == 0 || v == 3) ? 0 : v == 1 ? 1 : 2];      // (3: differentiated with the Gauss-Newton fallback)
    return LFR_OK;
}

namespace {

// device-assembled batch: labels (device graph stage) -> batch layout, all in HBM
int create_on_device(lfr_batch *b, const lfr::Problem &p, int shard_rank, int shard_world) {
    std::shared_ptr<lfr::DevProblem> dp = p.dev_get(b->device);
    const bool stage_flows = shard_world == 1;          // a shard gathers its rows zero-copy from pinned host memory
    if (!dp) {                                           // labels came from the host stage, or live on another GPU
        int rc = p.ensure_host_labels();
        if (rc != LFR_OK) return rc;
        rc = lfr::upload_labels(p, b->device, stage_flows, dp);
        if (rc != LFR_OK) return rc;
        p.dev_set(b->device, dp);
    }
    const lfr::DevGraph &dg = *dp->graph;
    const int64_t N = dg.N, M = dg.M, C = p.stats.n_components;
    hipStream_t st = b->ctx->s_main;
    // (the assembly's duration for the statistics is host wall clock: the assembly ends with the stage's one synchronisation anyway, and
    // a pair of timing events needed another blocking wait on an idle stream - tens of microseconds of a 1.7-ms Solver span)
    const auto t_asm0 = std::chrono::steady_clock::now();
    const size_t fixed = sizeof(double) * 2 * (size_t)std::max<int64_t>(N, 1) + sizeof(CompInfoDev) * (size_t)(C + 1) +
                         kProfWords * sizeof(unsigned long long) + ((size_t)1 << 16);
    if (!b->slab.init(b->ctx, lfr::assembly_output_bytes(N, M, C) + fixed)) return LFR_ERR_NOMEM;
    LFR_TAKE(b->slab, "batch slab", b->d_positions, double, 2 * std::max<int64_t>(N, 1));
    LFR_TAKE(b->slab, "batch slab", b->d_infos, CompInfoDev, C + 1);
    LFR_TAKE(b->slab, "batch slab", b->d_prof, unsigned long long, kProfWords);
    // Roots, constants and nodes outside every solved component stay at 0 for the life of the batch
    // (solve.cc:609-612); the kernels overwrite every variable on every solve, so no per-solve memset.
    HIP_TRY(hipMemsetAsync(b->d_positions, 0, sizeof(double) * 2 * (size_t)std::max<int64_t>(N, 1), st));
    HIP_TRY(hipMemsetAsync(b->d_prof, 0, kProfWords * sizeof(unsigned long long), st));
    lfr::DeviceAssembly dev;
    host_trace("assembly: launches begin");
    const int rc = lfr::assemble_on_device(p, *dp, shard_rank, shard_world, b->slab, dev);     // ends with the one synchronisation
    host_trace("assembly: summary is back");
    if (rc != LFR_OK) return rc;
    b->h2d_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_asm0).count();
    b->d_descs = dev.d_descs; b->d_edges = dev.d_edges; b->d_node_ids = dev.d_node_ids; b->d_node_inc = dev.d_node_inc;
    b->d_in_idx = dev.d_in_idx; b->d_ws_off = dev.d_ws_off; b->d_es_off = dev.d_es_off;
    b->d_desc_component = dev.d_desc_component; b->d_desc_class = dev.d_desc_class; b->d_desc_tracks = dev.d_desc_tracks;
    b->fused = dev.fused; b->d_edge_ref = dev.d_edge_ref; b->d_edge_word = dev.d_edge_word; b->packed_edges = dev.summary.packed_edges;
    if (dev.fused) b->dev_hold = dp;
    const lfr::AsmSummary &s = dev.summary;
    b->n_desc = (int)s.n_desc; b->n_edges = s.total_edges; b->n_nodes = s.total_nodes; b->n_tracks = s.n_tracks;
    for (int c = 0; c <= lfr::KC_COUNT; ++c) b->class_begin[c] = (int)s.class_begin[c];
    for (int c = 0; c < lfr::KC_COUNT; ++c) b->class_edges[c] = (int64_t)s.class_edges[c];
    for (int c = 0; c < lfr::KC_COUNT; ++c) b->class_max_rows[c] = (int)s.class_max_rows[c];
    b->es_doubles = s.es_doubles;                        // (the workspace itself: finish_workspace)
    return LFR_OK;
}

// host-assembled batch (lfr_problem_build): shard the problem's arrays, upload
int create_from_host(lfr_batch *b, const lfr::Problem &p, int shard_rank, int shard_world) {
    const std::vector<int32_t> shard = lfr::assign_shards(p, shard_world);
    const bool whole = shard_world == 1;
    std::vector<EdgeRec> edges_copy;
    std::vector<uint32_t> in_idx_copy;
    std::vector<lfr::NodeInc> node_inc_copy;
    std::vector<uint64_t> ws_off, es_off;
    uint64_t ws = 0;
    for (size_t i = 0; i < p.descs.size(); ++i) {
        if (shard[i] != shard_rank) continue;
        CompDesc d = p.descs[i];
        if (!whole) {
            const uint32_t eo = (uint32_t)edges_copy.size(), no = (uint32_t)b->node_ids.size();
            edges_copy.insert(edges_copy.end(), p.edges.begin() + d.edge_off, p.edges.begin() + d.edge_off + d.n_edges);
            in_idx_copy.insert(in_idx_copy.end(), p.in_idx.begin() + d.edge_off, p.in_idx.begin() + d.edge_off + d.n_edges);
            b->node_ids.insert(b->node_ids.end(), p.node_ids.begin() + d.node_off, p.node_ids.begin() + d.node_off + d.n_nodes);
            node_inc_copy.insert(node_inc_copy.end(), p.node_inc.begin() + d.node_off, p.node_inc.begin() + d.node_off + d.n_nodes);
            d.edge_off = eo; d.node_off = no;
        }
        b->descs.push_back(d); b->desc_component.push_back(p.desc_component[i]);
        b->desc_class.push_back(p.desc_class[i]); b->desc_tracks.push_back(p.desc_tracks[i]);
        const int cls = p.desc_class[i], rows = 2 * d.n_var;
        es_off.push_back(ws); ws_off.push_back(0);
        if (cls >= lfr::KC_BLOCK) {
            ws += 8 * (uint64_t)d.n_edges;                                                     // per-edge scratch
            b->class_max_rows[cls] = std::max(b->class_max_rows[cls], rows);
        }
        b->class_edges[cls] += d.n_edges;
        b->n_edges += d.n_edges; b->n_nodes += d.n_nodes; b->n_tracks += p.desc_tracks[i];
    }
    if (whole) b->node_ids = p.node_ids;
    const std::vector<EdgeRec> &edges = whole ? p.edges : edges_copy;
    const std::vector<uint32_t> &in_idx = whole ? p.in_idx : in_idx_copy;
    const std::vector<lfr::NodeInc> &node_inc = whole ? p.node_inc : node_inc_copy;
    b->es_doubles = ws;                                  // (KC_GLOBAL: the matrices' workspace is planned in finish_workspace)
    b->n_desc = (int)b->descs.size();
    {   // class ranges (descs are sorted by class)
        int c = 0;
        b->class_begin[0] = 0;
        for (int i = 0; i <= b->n_desc; ++i) {
            const int cls = i < b->n_desc ? b->desc_class[i] : lfr::KC_COUNT;
            while (c < cls) b->class_begin[++c] = i;
        }
    }
    b->mirrors_valid = true;
    hipStream_t st = b->ctx->s_main;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct EvGuard { hipEvent_t &x, &y; ~EvGuard() { if (x) (void)hipEventDestroy(x); if (y) (void)hipEventDestroy(y); } } guard{e0, e1};
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, st));
    const size_t nd = std::max<size_t>(b->descs.size(), 1), ne = std::max<size_t>(edges.size(), 1), nn = std::max<size_t>(b->node_ids.size(), 1);
    const size_t npos = 2 * (size_t)std::max<int64_t>(b->n_graph_nodes, 1);
    const size_t bytes = nd * (sizeof(CompDesc) + sizeof(CompInfoDev) + 16) + ne * (sizeof(EdgeRec) + 4) + nn * (4 + sizeof(lfr::NodeInc)) +
                         npos * sizeof(double) + kProfWords * sizeof(unsigned long long) + ((size_t)1 << 16);
    if (!b->slab.init(b->ctx, bytes)) return LFR_ERR_NOMEM;
    LFR_TAKE(b->slab, "batch slab", b->d_descs, CompDesc, nd); LFR_TAKE(b->slab, "batch slab", b->d_edges, EdgeRec, ne);
    LFR_TAKE(b->slab, "batch slab", b->d_node_ids, uint32_t, nn);
    LFR_TAKE(b->slab, "batch slab", b->d_node_inc, lfr::NodeInc, nn); LFR_TAKE(b->slab, "batch slab", b->d_in_idx, uint32_t, ne);
    LFR_TAKE(b->slab, "batch slab", b->d_positions, double, npos); LFR_TAKE(b->slab, "batch slab", b->d_infos, CompInfoDev, nd);
    LFR_TAKE(b->slab, "batch slab", b->d_ws_off, uint64_t, nd); LFR_TAKE(b->slab, "batch slab", b->d_es_off, uint64_t, nd);
    LFR_TAKE(b->slab, "batch slab", b->d_prof, unsigned long long, kProfWords);
    HIP_TRY(hipMemsetAsync(b->d_positions, 0, npos * sizeof(double), st));        // solve.cc:609-612, see create_on_device
    HIP_TRY(hipMemsetAsync(b->d_prof, 0, kProfWords * sizeof(unsigned long long), st));
    if (!b->descs.empty()) {
        HIP_TRY(hipMemcpyAsync(b->d_ws_off, ws_off.data(), ws_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->d_es_off, es_off.data(), es_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->d_descs, b->descs.data(), b->descs.size() * sizeof(CompDesc), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->d_edges, edges.data(), edges.size() * sizeof(EdgeRec), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->d_node_ids, b->node_ids.data(), b->node_ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->d_node_inc, node_inc.data(), node_inc.size() * sizeof(lfr::NodeInc), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->d_in_idx, in_idx.data(), in_idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));               // the staging vectors above die at return
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    b->h2d_ms = ms;
    return LFR_OK;
}

// plan i of the elimination-tree class: tab[3 i + 2] doubles from ws[tab[3 i]] (where one copy landed all plans) to ws[tab[3 i + 1]] (its component's workspace)
__global__ void k_place_plans(double *ws, const uint64_t *tab) {
    const uint64_t from = tab[3 * blockIdx.x], to = tab[3 * blockIdx.x + 1], n = tab[3 * blockIdx.x + 2];
    for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) ws[to + i] = ws[from + i];
}

// The workgroup kernels' workspace: per-edge scratch, then - for the components of the HBM class - the elimination-tree plans
// (lfr_treeplan.cpp) with their tiles, vectors and team areas.  The plans need the components' (source, destination, kind) lists on the host: the
// last word of every edge record, fetched with one strided copy when the batch was assembled on the device.
int finish_workspace(lfr_batch *b, const lfr::Problem &p) {
    const lfr::SolveGeometry &geo = lfr::solve_geometry();
    const int kTeamMax = geo.team_max, kTeamUnitsPerXcc = geo.team_units_per_xcc, kTeamCtlWords = geo.team_ctl_words, kTeamRedPerUnit = geo.team_red_per_unit;
    const int g0 = b->class_begin[lfr::KC_GLOBAL], g1 = b->class_begin[lfr::KC_COUNT];
    hipStream_t st = b->ctx->s_main;
    if (g1 <= g0) {
        if (b->es_doubles) {
            if (!b->ws_slab.init(b->ctx, b->es_doubles * sizeof(double))) return LFR_ERR_NOMEM;
            b->d_workspace = (double *)b->ws_slab.base;
        }
        return LFR_OK;
    }
    host_trace("finish_workspace: enters (components above the LDS classes)");
    { const int rc = ensure_mirrors(b); if (rc != LFR_OK) return rc; }
    host_trace("finish_workspace: host mirrors of the descriptors");
    const int ng = g1 - g0;
    const uint32_t e0 = b->descs[g0].edge_off;
    uint64_t ne = 0;
    for (int i = g0; i < g1; ++i) ne = std::max<uint64_t>(ne, (uint64_t)b->descs[i].edge_off + b->descs[i].n_edges - e0);
    // The record words and the plans are megabytes in ~130 allocations made by the pool's workers: handing them back to the system (munmap with
    // TLB shootdowns on every core a worker ran on) took 1.2 ms at the end of this function - a thread of its own does it while the solve starts.
    struct PlanTemps { std::vector<uint32_t> words; std::vector<lfr::TreePlan> plans; };
    struct Later { PlanTemps *p; ~Later() { PlanTemps *q = p; std::thread([q] { delete q; }).detach(); } } later{new PlanTemps()};
    std::vector<uint32_t> &words = later.p->words;
    words.resize(ne);
    if (p.host_batch && b->shard_world == 1) {
        for (uint64_t e = 0; e < ne; ++e) words[e] = (uint32_t)p.edges[e0 + e].src | ((uint32_t)p.edges[e0 + e].dst_kind << 16);
    } else if (ne) {
        // (a device-assembled whole batch kept one word per record beside the records: one linear copy.  The strided copy of the records' last
        // words - 4 bytes of every 80 - took 1.1 ms for 0.3 M records)
        if (b->d_edge_word) HIP_TRY(hipMemcpyAsync(words.data(), b->d_edge_word + e0, 4 * ne, hipMemcpyDeviceToHost, st));
        else HIP_TRY(hipMemcpy2DAsync(words.data(), 4, reinterpret_cast<const char *>(b->d_edges + e0) + 76, sizeof(EdgeRec), 4, ne, hipMemcpyDeviceToHost, st));
        HIP_TRY(lfr::stream_wait(st));
    }
    host_trace("finish_workspace: record words on the host");
    std::vector<lfr::TreePlan> &plans = later.p->plans;
    plans.resize(ng);
    {
        std::atomic<int> next{0};
        // (a plan is ~1 ms of one core for a cap-sized component and the plans are independent: as many threads as components, up to half
        // the machine - 32 threads left the 130 plans of the sparse bench workload at 6.5 ms of a 10-ms Solver span)
        const int T = std::max(1, std::min(ng, (int)std::min(128u, std::max(std::min(8u, std::max(1u, std::thread::hardware_concurrency())), std::thread::hardware_concurrency() / 2))));
        auto work = [&] {
            for (;;) {
                const int i = next.fetch_add(1);
                if (i >= ng) break;
                const CompDesc &d = b->descs[g0 + i];
                lfr::tree_plan(d.n_var, d.n_edges, words.data() + (d.edge_off - e0), plans[i]);
            }
        };
        lfr::run_on_pool(T, work);                 // (persistent workers: creating 127 threads per batch was most of the 4 ms this step took)
    }
    host_trace("finish_workspace: plans made");
    std::vector<uint64_t> off(ng);
    uint64_t ws = (b->es_doubles + 31) / 32 * 32, hdr_total = 0;
    b->tree_tiles = b->tree_dense_tiles = 0;
    b->tree_levels_max = 0; b->tree_blocks = 0; b->tree_updates = 0;
    for (int i = 0; i < ng; ++i) {
        if (plans[i].blob.empty()) { lfr::set_error("a component is too large for the elimination-tree plan's 32-bit offsets"); return LFR_ERR_UNSUPPORTED; }
        off[i] = ws;
        ws += (plans[i].doubles() + 31) / 32 * 32;
        hdr_total += plans[i].header_doubles();
        b->tree_tiles += plans[i].n_tiles;
        b->tree_dense_tiles += (int64_t)plans[i].NB * (plans[i].NB + 1) / 2;
        b->tree_levels_max = std::max(b->tree_levels_max, plans[i].n_levels);
        b->tree_blocks += plans[i].NB; b->tree_updates += (int64_t)plans[i].n_updates;
        const int64_t cs[5] = {plans[i].NB, plans[i].n_tiles, (int64_t)plans[i].n_updates, plans[i].n_levels, plans[i].n_items};
        b->tree_comp_stats.insert(b->tree_comp_stats.end(), cs, cs + 5);
    }
    b->tree_begin = g0;
    // Teams (the comment above TeamCtx): a component whose hand-out key reaches team_work[k] is solved by 2 << k workgroups.
    // LFR_TREE_TEAM="w2,w4[,w8]" sets the thresholds, "0" switches teams off.  Defaults from the cap-sized sparse workload: one
    // workgroup runs ~0.11 us per row and LM iteration, iteration counts vary 10-40 whatever the size, so everything above ~700 rows
    // can end a launch on its own.
    {
        uint32_t w[3] = {700u, 1500u, 2000u};
        if (const char *e = getenv("LFR_TREE_TEAM")) {
            unsigned v[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
            const int got = sscanf(e, "%u,%u,%u", &v[0], &v[1], &v[2]);
            if (got >= 1 && v[0] == 0u) w[0] = w[1] = w[2] = 0xffffffffu;
            else if (got >= 2) { w[0] = v[0]; w[1] = std::max(v[0], v[1]); w[2] = got >= 3 ? std::max(w[1], v[2]) : 0xffffffffu; }
        }
        int64_t wgs = 0;
        bool any = false;
        for (int i = 0; i < ng; ++i) {
            const CompDesc &d = b->descs[g0 + i];
            const uint32_t work = (uint32_t)d.n_var * (1u + ((uint32_t)d.n_nodes - d.n_var > 1u ? 1u : 0u));
            int t = 1;
            for (int k = 0; k < 3; ++k) if ((2 << k) <= kTeamMax && work >= w[k]) t = 2 << k;
            if (plans[i].blob[28] == 0u) t = 1;
            any = any || t > 1;
            wgs += t;
        }
        b->team_wgs = 0;
        if (const char *e = getenv("LFR_TEAM_PATIENCE_MS")) b->team_patience_us = (uint32_t)(std::min(60000.0, std::max(0.01, atof(e))) * 1000.0);
        if (any && b->n_desc < (1 << 28)) {
            for (int k = 0; k < 3; ++k) b->team_work[k] = w[k];
            b->team_wgs = (int)std::min<int64_t>(256, (wgs + 31) / 32 * 32);
        }
    }
    const uint64_t team_off = ws;
    if (b->team_wgs) ws += (kTeamCtlWords + 1) / 2 + 8ull * kTeamUnitsPerXcc * kTeamRedPerUnit;
    // behind everything: where the plans' words land in ONE copy before a kernel moves each to its component's workspace, + {from, to, doubles} per plan
    const uint64_t land_off = ws;
    ws += hdr_total + 3ull * (uint64_t)ng;
    if (!b->ws_slab.init(b->ctx, ws * sizeof(double))) return LFR_ERR_NOMEM;
    b->d_workspace = (double *)b->ws_slab.base;
    if (b->team_wgs) {
        b->d_team_ctl = reinterpret_cast<unsigned int *>(b->d_workspace + team_off);
        b->d_team_red = b->d_workspace + team_off + (kTeamCtlWords + 1) / 2;
        // (the reduction slots carry {value, launch << 32 | reduction} granules: tags of an earlier owner of this memory must not match)
        HIP_TRY(hipMemsetAsync(b->d_team_red, 0, 8ull * kTeamUnitsPerXcc * kTeamRedPerUnit * sizeof(double), st));
    }
    // the plans' words: staged in one pinned buffer (it must outlive the asynchronous copies: waited for below)
    host_trace("finish_workspace: workspace allocated, team area cleared");
    size_t got = 0;
    double *stage = (double *)b->ctx->pinned_acquire((hdr_total + 3ull * (uint64_t)ng) * sizeof(double), &got);
    if (!stage) return LFR_ERR_NOMEM;
    {
        // (one copy + one kernel instead of a copy per plan: 130 small copies took 1.6 ms)
        uint64_t so = 0;
        uint64_t *tab = reinterpret_cast<uint64_t *>(stage + hdr_total);
        for (int i = 0; i < ng; ++i) {
            tab[3 * i] = land_off + so; tab[3 * i + 1] = off[i]; tab[3 * i + 2] = plans[i].header_doubles();
            so += plans[i].header_doubles();
        }
        std::atomic<int> next{0};
        lfr::run_on_pool(std::min(ng, 16), [&] {                    // (megabytes of words into the pinned buffer: a few workers, not one)
            for (;;) {
                const int i = next.fetch_add(1);
                if (i >= ng) break;
                memcpy(stage + (tab[3 * i] - land_off), plans[i].blob.data(), plans[i].blob.size() * 4);
            }
        });
        if (hipMemcpyAsync(b->d_workspace + land_off, stage, (hdr_total + 3ull * (uint64_t)ng) * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) {
            b->ctx->pinned_release(stage, got); lfr::set_error("hipMemcpyAsync of the plans failed"); return LFR_ERR_HIP;
        }
        hipLaunchKernelGGL(k_place_plans, dim3((unsigned)ng), dim3(256), 0, st, b->d_workspace, reinterpret_cast<const uint64_t *>(b->d_workspace + land_off + hdr_total));
    }
    hipError_t e1 = hipMemcpyAsync(b->d_ws_off + g0, off.data(), ng * sizeof(uint64_t), hipMemcpyHostToDevice, st);
    hipError_t e2 = hipStreamSynchronize(st);
    host_trace("finish_workspace: plans uploaded");
    b->ctx->pinned_release(stage, got);
    host_trace("finish_workspace: staging buffer back");
    if (e1 != hipSuccess || e2 != hipSuccess) { lfr::set_error("upload of the elimination-tree plans failed"); return LFR_ERR_HIP; }
    if (getenv("LFR_VERBOSE"))
        fprintf(stderr, "lfr: %d component(s) above %d rows: elimination-tree plans keep %lld of %lld tiles (%.1f %%) in %lld columns, at most %d levels, workspace %.1f MB\n", ng,
                lfr::block_max_rows(), (long long)b->tree_tiles, (long long)b->tree_dense_tiles, 100.0 * b->tree_tiles / std::max<int64_t>(1, b->tree_dense_tiles),
                (long long)b->tree_blocks, b->tree_levels_max, ws * 8e-6);
    return LFR_OK;
}

}  // namespace

extern "C" {

int lfr_problem_build_hip_ex(const lfr_graph *g, int device, int64_t max_nodes_in_component, const int64_t *component_override,
                             int flags, lfr_problem **out) {
    if (!g || !out) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    const bool stage_flows = !(flags & LFR_BUILD_FLOWS_STAY_ON_HOST);
    if (!component_override) {
        lfr_problem *h = new lfr_problem();
        const int rc = lfr::graph_stage_on_device(g->g, max_nodes_in_component, device, stage_flows, h->p);
        if (rc == LFR_OK) { *out = h; return LFR_OK; }
        delete h;
        if (rc != lfr::LFR_GRAPHSTAGE_USE_HOST) { *out = nullptr; return rc; }
    }
    return lfr_problem_build_labels(g, max_nodes_in_component, component_override, out);   // host graph stage
}

// Multi-GPU, one process per GPU: the graph stage of ONE rank.  The constrained spanning forest of solve.cc:489-541 is a global greedy, but
// it decomposes exactly by connected component of the match graph (no union ever crosses one), and so does everything behind it (roots,
// components, the size cap, the solve): rank r takes the connected components k = r (mod world) in node order - found by the same
// union-find pass on every rank - and runs tracks / roots / components over their matches only.  lfr_batch_create(p, device, 0, 1) then
// assembles exactly this rank's components; positions of the other ranks' nodes stay 0.  Returns with lfr_problem_cc_sharded(p) = 0
// when one connected component dominates (real data: wrong matches link everything) - the problem then covers the whole graph and the
// caller shards its components at assembly (lfr_batch_create(p, device, rank, world)) as before.
int lfr_problem_build_hip_shard(const lfr_graph *g, int device, int64_t max_nodes_in_component, int flags, int shard_rank, int shard_world,
                                lfr_problem **out) {
    if (!g || !out || shard_world < 1 || shard_world > 64 || shard_rank < 0 || shard_rank >= shard_world) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    const bool stage_flows = !(flags & LFR_BUILD_FLOWS_STAY_ON_HOST);
    lfr_problem *h = new lfr_problem();
    const int rc = lfr::graph_stage_on_device(g->g, max_nodes_in_component, device, stage_flows, h->p, shard_rank, shard_world);
    if (rc == LFR_OK) { *out = h; return LFR_OK; }
    delete h;
    if (rc != lfr::LFR_GRAPHSTAGE_USE_HOST) { *out = nullptr; return rc; }
    return lfr_problem_build_labels(g, max_nodes_in_component, nullptr, out);      // host graph stage over the whole graph (not sharded)
}
int lfr_problem_cc_sharded(const lfr_problem *p) {
    if (!p) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    return p->p.cc_sharded ? 1 : 0;
}

int lfr_problem_build_hip(const lfr_graph *g, int device, int64_t max_nodes_in_component, const int64_t *component_override,
                          lfr_problem **out) {
    return lfr_problem_build_hip_ex(g, device, max_nodes_in_component, component_override, 0, out);
}


int lfr_hip_warmup(int device) {
    // Creating the HIP context costs a few hundred ms; a host program can call this from a side
    // thread while it parses its input (the `solve` launcher does).
    lfr::DevCtx *ctx = lfr::dev_ctx(device);
    if (!ctx) return LFR_ERR_HIP;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(nullptr));
    lfr::launch_warmup();                                                                  // loads the forward kernels' code object
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    int level = 2;                                   // LFR_WARMUP_LEVEL: 0 = context only, 1 = + toy graph, 2 = + a million matches
    if (const char *e = getenv("LFR_WARMUP_LEVEL")) level = atoi(e);
    if (level < 1) return LFR_OK;
    // HIP also resolves every kernel on its first launch (~1 ms each; the graph stage and the assembly launch
    // about forty different ones, rocPRIM's included): push a toy graph - one 18-node track (workgroup kernel)
    // and one 3-node track (packed kernel) - through the whole device pipeline once.  Best effort.
    {
        constexpr int kImg = 18;
        std::vector<std::string> names(kImg);
        std::vector<const char *> name_ptrs(kImg);
        std::vector<float> facts(kImg, 1.0f);
        for (int i = 0; i < kImg; ++i) { names[i] = "warmup" + std::to_string(i); name_ptrs[i] = names[i].c_str(); }
        std::vector<int32_t> p1, p2;
        std::vector<int64_t> off{0};
        std::vector<uint32_t> f1, f2;
        for (int a = 0; a < kImg; ++a)
            for (int b = a + 1; b < kImg; ++b) {
                p1.push_back(a); p2.push_back(b);
                f1.push_back(0); f2.push_back(0);                                  // the 18-node track
                if (b < 3) { f1.push_back(1); f2.push_back(1); }                   // the 3-node track
                off.push_back((int64_t)f1.size());
            }
        const size_t M = f1.size();
        std::vector<float> sim(M, 0.9f), flows(18 * M, 0.01f);
        lfr_graph *g = nullptr; lfr_problem *pr = nullptr; lfr_batch *bt = nullptr;
        if (lfr_graph_from_arrays(kImg, name_ptrs.data(), facts.data(), (int64_t)p1.size(), p1.data(), p2.data(), off.data(),
                                  f1.data(), f2.data(), sim.data(), flows.data(), flows.data(), nullptr, 0, &g) == LFR_OK &&
            lfr_problem_build_hip(g, device, 0, nullptr, &pr) == LFR_OK &&
            lfr_batch_create(pr, device, 0, 1, LFR_TUKEY_CERES1, &bt) == LFR_OK) {
            lfr_solve_stats st;
            (void)lfr_batch_solve(bt, nullptr, &st);
            const double *view = nullptr;
            (void)lfr_batch_positions_view(bt, &view);
        }
        lfr_batch_free(bt); lfr_problem_free(pr); lfr_graph_free(g);
    }
    // the large-input sort / scan kernels of the graph stage and of the assembly (the toy graph only reached the small-input ones)
    if (lfr::warm_graphstage_primitives(ctx) != LFR_OK || lfr::warm_assembly_primitives(ctx) != LFR_OK) return LFR_OK;     // best effort
    // The first LARGE device-to-host copy of a process takes ~7 ms longer than the next one (the toy graph's 300 bytes take another
    // path; measured with the kernel trace of the CLI: the positions' copy started 7.3 ms after the solve kernel had ended): one 8-MB
    // copy between scratch buffers here.
    {
        size_t db = 0, hb = 0;
        const size_t bytes = (size_t)8 << 20;
        void *d = ctx->dev_acquire(bytes, &db);
        void *h = ctx->pinned_acquire(bytes, &hb);
        if (d && h) {
            (void)hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->s_main);
            (void)hipStreamSynchronize(ctx->s_main);
        }
        if (d) ctx->dev_release(d, db);
        if (h) ctx->pinned_release(h, hb);
    }
    if (level < 2) return LFR_OK;
    // rocPRIM picks other kernels (one-sweep radix sort, look-back scans) once the inputs are large: a second pass with a
    // million matches (170 k four-node tracks, zero flows) resolves those as well, so that a one-shot caller's
    // "Total time" is not spent loading code.  Best effort, ~30 ms beside the caller's parse.
    {
        constexpr int kImg = 64, kLen = 4;
        constexpr int64_t kTracks = 170000;
        std::vector<std::string> names(kImg);
        std::vector<const char *> name_ptrs(kImg);
        std::vector<float> facts(kImg, 1.0f);
        for (int i = 0; i < kImg; ++i) { names[i] = "warmup" + std::to_string(i); name_ptrs[i] = names[i].c_str(); }
        // one ImagePair per (image a, image b = a + d): its matches are the tracks whose window covers both
        std::vector<int32_t> p1, p2;
        std::vector<int64_t> off{0};
        std::vector<uint32_t> f1, f2;
        for (int a = 0; a < kImg; ++a)
            for (int d = 1; d < kLen; ++d) {
                const int b = a + d;
                if (b >= kImg) continue;
                p1.push_back(a); p2.push_back(b);
                for (int64_t t = 0; t < kTracks; ++t) {              // track t sits on images s .. s + kLen - 1, s = t % (kImg - kLen + 1)
                    const int s0 = (int)(t % (kImg - kLen + 1));
                    if (a >= s0 && b < s0 + kLen) { f1.push_back((uint32_t)t); f2.push_back((uint32_t)t); }
                }
                off.push_back((int64_t)f1.size());
            }
        const size_t M = f1.size();
        std::vector<float> sim(M), flows(18 * M, 0.0f);
        for (size_t m = 0; m < M; ++m) sim[m] = 0.5f + 0.4f * (float)((m * 2654435761u) & 0xffff) / 65536.0f;
        lfr_graph *g = nullptr; lfr_problem *pr = nullptr; lfr_batch *bt = nullptr;
        if (lfr_graph_from_arrays(kImg, name_ptrs.data(), facts.data(), (int64_t)p1.size(), p1.data(), p2.data(), off.data(),
                                  f1.data(), f2.data(), sim.data(), flows.data(), flows.data(), nullptr, 0, &g) == LFR_OK &&
            lfr_problem_build_hip(g, device, 0, nullptr, &pr) == LFR_OK &&
            lfr_batch_create(pr, device, 0, 1, LFR_TUKEY_CERES1, &bt) == LFR_OK) {
            (void)lfr_batch_solve(bt, ctx->s_main, nullptr);
            const double *view = nullptr;
            (void)lfr_batch_positions_view(bt, &view);
        }
        lfr_batch_free(bt); lfr_problem_free(pr); lfr_graph_free(g);
    }
    for (int i = 0; i <= lfr::KC_COUNT; ++i) (void)ctx->side_stream(i);     // last: a few ms each, and only long-track inputs need them
    return LFR_OK;
}

int lfr_hip_reserve(int device, int64_t n_nodes, int64_t n_matches) {
    // Pre-populate the slab caches with what a pipeline run over a graph of this size will ask for, so that the
    // timed span of a one-shot caller (the `solve` launcher knows the sizes once the file is parsed... or guesses
    // them from the file size while it is still parsing) pays no hipMalloc / hipHostMalloc.
    if (n_nodes < 0 || n_matches < 0) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    lfr::DevCtx *ctx = lfr::dev_ctx(device);
    if (!ctx) return LFR_ERR_HIP;
    const int64_t N = n_nodes, M = n_matches;
    const size_t want[5] = {
        (size_t)16 * M + (size_t)4 * N + (size_t)144 * M + ((size_t)1 << 16),                              // DevGraph with staged flows
        (size_t)9 * N + 4096,                                                                             // DevProblem
        (size_t)96 * M + (size_t)112 * N + ((size_t)32 << 20),                                            // graph-stage temporaries
        (size_t)96 * M + (size_t)48 * N + (size_t)128 * (N + 1) + ((size_t)32 << 20),                     // assembly temporaries (C <= N)
        lfr::assembly_output_bytes(N, M, N) + (size_t)(16 + 32) * (size_t)(N + 1) + ((size_t)1 << 17)};   // batch slab
    void *p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t got[5] = {0, 0, 0, 0, 0};
    // (the graph-stage and assembly temporaries are never alive together: the larger of the two serves both)
    for (int i = 0; i < 5; ++i) {
        if (i == 2 && want[3] >= want[2]) continue;
        if (i == 3 && want[2] > want[3]) continue;
        p[i] = ctx->dev_acquire(want[i], &got[i]);
    }
    for (int i = 0; i < 5; ++i) if (p[i]) ctx->dev_release(p[i], got[i]);
    size_t hb = 0;
    if (void *h = ctx->pinned_acquire(sizeof(double) * 2 * (size_t)std::max<int64_t>(N, 1), &hb)) ctx->pinned_release(h, hb);
    return LFR_OK;
}

int lfr_hip_synchronize(int device) {
    lfr::DevCtx *ctx = lfr::dev_ctx(device);
    if (!ctx) return LFR_ERR_HIP;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamSynchronize(ctx->s_copy));
    HIP_TRY(hipStreamSynchronize(ctx->s_main));
    return LFR_OK;
}

int lfr_hip_trim(int device) {
    lfr::DevCtx *ctx = lfr::dev_ctx(device);
    if (!ctx) return LFR_ERR_HIP;
    ctx->trim();
    return LFR_OK;
}

void lfr_batch_free(lfr_batch *b) { delete b; }

int lfr_batch_create(const lfr_problem *ph, int device, int shard_rank, int shard_world, int tukey_variant,
                     lfr_batch **out) {
    if (!ph || !out || shard_world < 1 || shard_rank < 0 || shard_rank >= shard_world ||
        (tukey_variant != LFR_TUKEY_CERES1 && tukey_variant != LFR_TUKEY_CERES2)) {
        lfr::set_error("bad argument"); return LFR_ERR_ARG;
    }
    *out = nullptr;
    const lfr::Problem &p = ph->p;
    lfr::DevCtx *ctx = lfr::dev_ctx(device);
    if (!ctx) return LFR_ERR_HIP;
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<lfr_batch> b(new lfr_batch());            // every error path below releases what was acquired
    b->device = device; b->ctx = ctx; b->tukey_variant = tukey_variant; b->shard_world = shard_world;
    { const char *e = getenv("LFR_SERIAL_CLASSES"); b->serial = e && e[0] == '1'; }
    b->n_graph_nodes = p.g->n_nodes();
    b->graph = p.g; b->graph_serial = p.g->serial; b->n_graph_matches = p.g->n_matches();
    b->cc_sharded = p.cc_sharded;
    int rc = p.host_batch ? create_from_host(b.get(), p, shard_rank, shard_world) : create_on_device(b.get(), p, shard_rank, shard_world);
    if (rc != LFR_OK) return rc;
    if ((rc = finish_workspace(b.get(), p)) != LFR_OK) return rc;
    host_trace("lfr_batch_create: workspace done");
    if (!(b->ev_fork = ctx->event_acquire(false))) return LFR_ERR_HIP;
    if (b->class_begin[lfr::KC_COUNT] > b->class_begin[lfr::KC_BLOCK]) {       // workgroup classes run beside the packed launch
        if (!(b->side_stream = ctx->side_stream(0))) return LFR_ERR_HIP;
        for (int cls = lfr::KC_BLOCK; cls < lfr::KC_COUNT; ++cls)
            if (b->class_begin[cls + 1] > b->class_begin[cls] && !(b->wg_stream[cls] = ctx->side_stream(1 + cls))) return LFR_ERR_HIP;
        {   // hand-out order of the persistent launches
            const int wg_begin = b->class_begin[lfr::KC_BLOCK], n_wg = b->class_begin[lfr::KC_COUNT] - wg_begin;
            hipStream_t so = ctx->s_main;
            size_t tmp_bytes = 0;
            HIP_TRY(rocprim::radix_sort_pairs<LfrRadixSortConfig>(nullptr, tmp_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr,
                                                                   (uint32_t *)nullptr, (size_t)n_wg, 0u, 27u, so));
            if (!b->order_slab.init(ctx, 16 * (size_t)n_wg + tmp_bytes + 4096)) return LFR_ERR_NOMEM;
            b->d_wg_order = b->order_slab.take_n<uint32_t>(n_wg);
            uint32_t *keys = b->order_slab.take_n<uint32_t>(n_wg), *keys_sorted = b->order_slab.take_n<uint32_t>(n_wg), *vals = b->order_slab.take_n<uint32_t>(n_wg);
            void *tmp = b->order_slab.take(tmp_bytes);
            if (!b->d_wg_order || !keys || !keys_sorted || !vals || !tmp) { lfr::set_error("order slab exhausted"); return LFR_ERR_NOMEM; }
            hipLaunchKernelGGL(k_wg_order_keys, dim3((n_wg + 255) / 256), dim3(256), 0, so, b->d_descs + wg_begin, n_wg,
                               b->class_begin[lfr::KC_BLOCK_M] - wg_begin, b->class_begin[lfr::KC_BLOCK_L] - wg_begin, b->class_begin[lfr::KC_GLOBAL] - wg_begin,
                               keys, vals, wg_begin);
            HIP_TRY(hipGetLastError());
            HIP_TRY(rocprim::radix_sort_pairs<LfrRadixSortConfig>(tmp, tmp_bytes, keys, keys_sorted, vals, b->d_wg_order, (size_t)n_wg, 0u, 27u, so));
            if (!(b->ev_order = ctx->event_acquire(false))) return LFR_ERR_HIP;
            HIP_TRY(hipEventRecord(b->ev_order, so));
        }
        host_trace("lfr_batch_create: hand-out order enqueued");
        const int lds_s = (int)block_lds_bytes(std::max(b->class_max_rows[lfr::KC_BLOCK], 2));
        const int lds_m = (int)block_lds_bytes(std::max(b->class_max_rows[lfr::KC_BLOCK_M], 2));
        const int lds_l = (int)block_lds_bytes(std::max(b->class_max_rows[lfr::KC_BLOCK_L], 2));
        if ((rc = lfr::reserve_block_lds(lds_s, lds_m, lds_l)) != LFR_OK) return rc;
    }
    {   // the packed launch is reported in the slot of its largest class (by edges)
        int64_t best = -1;
        for (int cls = 0; cls < lfr::KC_BLOCK; ++cls) if (b->class_edges[cls] > best) { best = b->class_edges[cls]; b->packed_slot = cls; }
    }
    *out = b.release();
    host_trace("lfr_batch_create returns");
    return LFR_OK;
}

}  // extern "C"

namespace {

KernelArgs make_kernel_args(const lfr_batch *b) {
    KernelArgs a;
    a.descs = b->d_descs; a.edges = b->d_edges; a.node_ids = b->d_node_ids; a.positions = b->d_positions;
    a.infos = b->d_infos; a.workspace = b->d_workspace; a.ws_off = b->d_ws_off; a.es_off = b->d_es_off;
    a.node_inc = b->d_node_inc; a.in_idx = b->d_in_idx; a.tukey_variant = b->tukey_variant; a.prof = b->d_prof;
    { const char *e = getenv("LFR_SCRATCH_SWEEP"); a.scratch_sweep = (e && e[0] == '1') ? 1 : 0; }
    a.queue = lfr::queue_block(b->d_prof);
    a.wg_order = b->d_wg_order; a.wg_begin = b->class_begin[lfr::KC_BLOCK];
    a.edge_ref = b->d_edge_ref; a.edge_word = b->d_edge_word;
    a.f_row = nullptr; a.f_disp1 = a.f_disp2 = a.f_sim = nullptr;
    if (b->fused) {
        const lfr::DevGraph &dgr = *b->dev_hold->graph;
        a.f_row = dgr.flow_row; a.f_disp1 = dgr.disp1; a.f_disp2 = dgr.disp2; a.f_sim = dgr.sim;
    }
    a.team_ctl = b->d_team_ctl; a.team_red = b->d_team_red;
    a.trace = nullptr;
    a.x_start = nullptr;
    for (int k = 0; k < 3; ++k) a.team_work[k] = b->team_work[k];
    a.team_epoch = (uint32_t)(b->n_solves + 1);
    a.team_patience_us = b->team_patience_us;
    return a;
}

// one workgroup class (persistent workgroups that take their components from the class's queue) on stream cs
int launch_wg_class(lfr_batch *b, KernelArgs &a, int cls, hipStream_t cs) {
    const lfr::SolveGeometry &geo = lfr::solve_geometry();
    a.desc_begin = b->class_begin[cls]; a.desc_end = b->class_begin[cls + 1]; a.cls = cls;
    const int n = a.desc_end - a.desc_begin;
    if (n <= 0) return LFR_OK;
    if (cls == lfr::KC_GLOBAL) {
        if (const char *e = getenv("LFR_DEBUG_TREE_FIRST")) a.desc_end = std::min(a.desc_end, a.desc_begin + std::max(1, atoi(e)));   // (experiments: only the first k of the hand-out order)
        // elimination-tree kernel: one 512-thread workgroup per CU (two waves per SIMD), static LDS only
        // (at least 8 kTeamMax workgroups: whatever the placement, one of the eight XCDs then holds a complete unit)
        if (b->d_team_ctl) lfr::launch_tree(a, true, std::max(lfr::kTeamXccs * geo.team_max, std::min(b->team_wgs, b->ctx->n_cu / 32 * 32)), cs);
        else lfr::launch_tree(a, false, std::min(n, b->ctx->n_cu), cs);
    } else {
        const int rows = b->class_max_rows[cls];
        const size_t lds = block_lds_bytes(rows);
        // persistent workgroups: what the chip keeps resident for the class (by LDS, and 8 waves of 256 registers per CU)
        const int threads = cls == lfr::KC_BLOCK ? geo.threads_s : cls == lfr::KC_BLOCK_M ? geo.threads_m : geo.threads_l;
        const int by_waves = std::max(1, 512 / threads), by_lds = std::max(1, (int)((size_t)160 * 1024 / (lds + 256)));
        const int wgs = std::min(n, b->ctx->n_cu * std::min(by_waves, by_lds));
        lfr::launch_block_class(cls, a, rows, wgs, cs);
    }
    HIP_TRY(hipGetLastError());
    return LFR_OK;
}

// LFR_SERIAL_CLASSES=1: every class separately on the caller's stream (per-class timings for diagnostics)
int launch_serial(lfr_batch *b, KernelArgs &a, uint32_t &recorded, hipStream_t st) {
    const int *const comps_per_block = lfr::solve_geometry().comps_per_block;
    for (int cls = 0; cls < lfr::KC_COUNT; ++cls) {
        a.desc_begin = b->class_begin[cls]; a.desc_end = b->class_begin[cls + 1]; a.cls = cls;
        const int n = a.desc_end - a.desc_begin;
        if (n <= 0) continue;
        recorded |= 1u << cls;
        HIP_TRY(hipEventRecord(b->ev[2 + 2 * cls], st));
        {
            const int grid = (n + comps_per_block[cls] - 1) / comps_per_block[cls];
            if (cls < lfr::KC_BLOCK) lfr::launch_group_class(cls, a, b->fused, grid, st);       // (KC_G32 is retired: no component)
            else { const int rc = launch_wg_class(b, a, cls, st); if (rc != LFR_OK) return rc; }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(b->ev[3 + 2 * cls], st));
    }
    return LFR_OK;
}

// The packed classes go out as ONE launch on the caller's stream (solve_packed_kernel); the few
// workgroup-per-component problems run beside it on a side stream.
// materialised: this solve wrote the packed records in front of its launches.
int launch_plan(lfr_batch *b, KernelArgs &a, bool materialised, uint32_t &recorded, hipStream_t st) {
    // Launch plan.  A workgroup-per-component kernel needs a (nearly) empty CU for each of its
    // 512-thread workgroups; once the packed launch has flooded the chip such a workgroup only gets a
    // CU at the packed launch's tail, i.e. the two kernels would run back to back.  So when big-workgroup
    // classes exist THEY go first, on the caller's stream, and the packed launch follows from a side
    // stream (its cross-queue wait makes it the later dispatch) and fills the remaining CUs.
    // Events are barrier packets on their stream: only the launches that exist are bracketed.
    const bool have_side = b->class_begin[lfr::KC_COUNT] > b->class_begin[lfr::KC_BLOCK];
    PackedRanges r;
    int nb = 0;
    lfr::packed_ranges(b, lfr::solve_geometry().packed_waves, &r, &nb);
    // the packed launch is timed as one unit: its events sit in the slot of the largest class
    // (the only launch of the solve - no workgroup class, no records to materialise in front: the solve's own pair of events brackets
    // exactly this kernel, a second pair would be two more barrier packets per solve for the same two time stamps)
    const bool alias = !have_side && !materialised;
    auto launch_packed = [&](hipStream_t cs) -> int {
        if (!alias) HIP_TRY(hipEventRecord(b->ev[2 + 2 * b->packed_slot], cs));
        lfr::launch_packed(a, r, b->fused, nb, cs);
        HIP_TRY(hipGetLastError());
        if (!alias) HIP_TRY(hipEventRecord(b->ev[3 + 2 * b->packed_slot], cs));
        recorded |= 1u << b->packed_slot;
        if (alias) recorded |= kPackedEventsAliased;
        return LFR_OK;
    };
    auto launch_big = [&](int cls, hipStream_t cs) -> int {
        HIP_TRY(hipEventRecord(b->ev[2 + 2 * cls], cs));
        const int rc = launch_wg_class(b, a, cls, cs);
        if (rc != LFR_OK) return rc;
        HIP_TRY(hipEventRecord(b->ev[3 + 2 * cls], cs));
        recorded |= 1u << cls;
        return LFR_OK;
    };
    if (!have_side) {
        if (nb > 0) { const int rc = launch_packed(st); if (rc != LFR_OK) return rc; }
        return LFR_OK;
    }
    // Every workgroup class on its own stream (the first on the caller's).  Dispatch order = issue order: the HBM-matrix
    // class first (its components run longest), then the 130-row class, the 192-row class, the 88-row class.  A 160 KB
    // workgroup only starts on an empty CU: issued first, the largest class kept the others out until its queue drained,
    // and the one slow component among THEM (iteration counts vary 8x) then ended the solve alone (config 5: 17.0 ms
    // against 13.8 at the time).  With persistent workgroups the middle class takes the whole chip for its 1.5 ms, the
    // large class follows, and the small class fills the CUs the large one's tail leaves (measured 9.15 ms against
    // 9.4-9.5 smallest-first and 12.4 largest-first); LFR_WG_ORDER overrides for experiments.  Round 3, with the fused sweep
    // (5.1 ms): largest-first 7.9 ms; largest-first with only its share of the CUs (by rows x threads x components) and full
    // grids behind it 5.8-7.2 ms - the pending workgroups of the later launches do not take the CUs the first one frees, and
    // the packed launch starves; the order stays.
    static const std::array<int, 4> kBigOrder = [] {
        std::array<int, 4> o = {lfr::KC_GLOBAL, lfr::KC_BLOCK_M, lfr::KC_BLOCK_L, lfr::KC_BLOCK};
        if (const char *e = getenv("LFR_WG_ORDER")) {
            int v[4];
            if (sscanf(e, "%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3]) == 4) {
                unsigned seen = 0;
                for (int i = 0; i < 4; ++i) if (v[i] >= lfr::KC_BLOCK && v[i] < lfr::KC_COUNT) seen |= 1u << v[i];
                if (seen == (0xfu << lfr::KC_BLOCK)) for (int i = 0; i < 4; ++i) o[i] = v[i];
            }
        }
        return o;
    }();
    int first = -1, n_big = 0;
    for (int i = 0; i < 4; ++i) if (b->class_begin[kBigOrder[i] + 1] > b->class_begin[kBigOrder[i]]) { if (first < 0) first = kBigOrder[i]; ++n_big; }
    if (n_big > 1 || nb > 0) HIP_TRY(hipEventRecord(b->ev_fork, st));
    { const int rc = launch_big(first, st); if (rc != LFR_OK) return rc; }
    for (int i = 0; i < 4; ++i) {
        const int cls = kBigOrder[i];
        if (cls == first || b->class_begin[cls + 1] <= b->class_begin[cls]) continue;
        HIP_TRY(hipStreamWaitEvent(b->wg_stream[cls], b->ev_fork, 0));
        const int rc = launch_big(cls, b->wg_stream[cls]);
        if (rc != LFR_OK) return rc;
    }
    if (nb > 0) {
        HIP_TRY(hipStreamWaitEvent(b->side_stream, b->ev_fork, 0));
        const int rc = launch_packed(b->side_stream);
        if (rc != LFR_OK) return rc;
        HIP_TRY(hipStreamWaitEvent(st, b->ev[3 + 2 * b->packed_slot], 0));
    }
    for (int i = 0; i < 4; ++i) {
        const int cls = kBigOrder[i];
        if (cls == first || b->class_begin[cls + 1] <= b->class_begin[cls]) continue;
        HIP_TRY(hipStreamWaitEvent(st, b->ev[3 + 2 * cls], 0));
    }
    return LFR_OK;
}

// What the diagnostic builds left in the solve's buffers (-DLFR_TRACE_TREE, -DLFR_PROFILE_FACTOR, -DLFR_PROFILE_PHASES), and the bounded
// spins that ran out; the solve's stream has been waited for.
int read_diagnostics(lfr_batch *b, const KernelArgs &a) {
#ifdef LFR_TRACE_TREE
    if (const char *tf = getenv("LFR_TREE_TRACE_FILE")) {
        unsigned long long n = 0;
        HIP_TRY(hipMemcpy(&n, a.trace, 8, hipMemcpyDeviceToHost));
        n = std::min<unsigned long long>(n, (1ull << 20) - 4);
        std::vector<unsigned long long> h(n + 2);
        HIP_TRY(hipMemcpy(h.data(), a.trace, (n + 2) * 8, hipMemcpyDeviceToHost));
        if (FILE *f = fopen(tf, "wb")) { fwrite(h.data() + 2, 8, n, f); fclose(f); }
    }
#endif
#ifdef LFR_PROFILE_FACTOR
    {
        unsigned long long h[lfr::kProfFactorWords * (lfr::KC_COUNT - lfr::KC_BLOCK)];
        HIP_TRY(hipMemcpy(h, lfr::factor_profile(b->d_prof, lfr::KC_BLOCK), sizeof h, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(lfr::factor_profile(b->d_prof, lfr::KC_BLOCK), 0, sizeof h));
        for (int c = 0; c < lfr::KC_COUNT - lfr::KC_BLOCK; ++c) for (int w = 0; w < 2; ++w) {
            const unsigned long long *q = h + lfr::kProfFactorWords * c + 8 * w;
            if (q[7])
                fprintf(stderr, "lfr-fprof class %d wave %d: factorizations %llu  cycles each: diag %.0f  trailing %.0f  wait %.0f  col-update %.0f  col-finish %.0f  barrier %.0f   (wave 0: diag = loads + elimination, trailing = its stores)\n",
                        lfr::KC_BLOCK + c, w, q[7], (double)q[0] / q[7], (double)q[1] / q[7], (double)q[2] / q[7], (double)q[3] / q[7], (double)q[4] / q[7], (double)q[5] / q[7]);
        }
    }
#endif
#ifdef LFR_PROFILE_PHASES
    {
        unsigned long long h[lfr::kProfPhases * lfr::KC_COUNT];
        HIP_TRY(hipMemcpy(h, b->d_prof, sizeof h, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(b->d_prof, 0, sizeof h));
        for (int c = 0; c < lfr::KC_COUNT; ++c) {
            const unsigned long long *q = h + lfr::kProfPhases * c;
            if (q[7])
                fprintf(stderr, "lfr-prof class %d: waves %llu  per-wave cycles: [0] %.0f  [1] %.0f  [2] %.0f  [3] %.0f  [4] %.0f  [5] %.0f  [6] %.0f   (packed: prologue/elim/sweep/reduce/transitions/setup/zero; block: jac-sweeps/factor/ls-sweeps/-/bookkeeping/scaling/trisolve)\n", c,
                        q[7], (double)q[0] / q[7], (double)q[1] / q[7], (double)q[2] / q[7], (double)q[3] / q[7], (double)q[4] / q[7], (double)q[5] / q[7], (double)q[6] / q[7]);
        }
    }
#endif
    // bounded spins that ran out (wave hand-offs of the factorizations, the teams' barriers): a rejected LM step or a failed
    // component instead of a hung GPU - visible under LFR_VERBOSE, an ERROR under LFR_SPIN_TIMEOUT_FATAL=1 (the GPU tests set it)
    static const bool verbose = getenv("LFR_VERBOSE") != nullptr;
    static const bool fatal = [] { const char *e = getenv("LFR_SPIN_TIMEOUT_FATAL"); return e && e[0] == '1'; }();
    if ((verbose || fatal) && b->class_begin[lfr::KC_COUNT] > b->class_begin[lfr::KC_BLOCK]) {
        unsigned int v = 0;
        HIP_TRY(hipMemcpy(&v, a.queue + lfr::kQueueSpinTimeouts, sizeof v, hipMemcpyDeviceToHost));
        if (v && verbose) fprintf(stderr, "lfr: %u bounded spin-wait(s) of the workgroup kernels ran out during this solve (rejected LM steps / failed components)\n", v);
        if (v && fatal) { lfr::set_error("%u bounded spin-wait(s) of the workgroup kernels ran out (LFR_SPIN_TIMEOUT_FATAL=1)", v); return LFR_ERR_HIP; }
    }
    return LFR_OK;
}

// the statistics of the solve just waited for: the infos come to the host, `recorded` names the launches that were bracketed by events
int collect_stats(lfr_batch *b, uint32_t recorded, hipStream_t st, lfr_solve_stats *stats) {
    memset(stats, 0, sizeof *stats);
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, b->ev[0], b->ev[1]));
    stats->kernel_ms = ms;
    stats->h2d_ms = b->h2d_ms;
    { const int rc = ensure_mirrors(b); if (rc != LFR_OK) return rc; }
    b->infos.resize(b->descs.size());
    if (!b->descs.empty()) {
        HIP_TRY(hipMemcpyAsync(b->infos.data(), b->d_infos, b->descs.size() * sizeof(CompInfoDev), hipMemcpyDeviceToHost, st));
        HIP_TRY(lfr::stream_wait(st));
    }
    b->infos_valid = true;
    stats->n_components = (int64_t)b->descs.size();
    stats->n_edges = b->n_edges; stats->n_nodes = b->n_nodes; stats->n_tracks = b->n_tracks;
    double best_ms = -1.0;
    int64_t edges = 0, nodes = 0, refp_e = 0, refp_n = 0;
    for (int cls = 0; cls < lfr::KC_COUNT; ++cls) {
        // one accounting unit per kernel LAUNCH: the packed classes are one launch unless serial
        const bool merged = !b->serial && cls < lfr::KC_BLOCK;
        if (!merged || cls == 0) { edges = 0; nodes = 0; refp_e = 0; refp_n = 0; }
        for (int i = b->class_begin[cls]; i < b->class_begin[cls + 1]; ++i) {
            const CompInfoDev &f = b->infos[i];
            const int64_t E = b->descs[i].n_edges, N = b->descs[i].n_nodes;
            const int64_t jac = 1 + f.n_ls_evals + f.n_successful, cst = f.n_cand_evals;
            stats->ref_jacobian_passes_edges += E * jac;
            stats->ref_cost_passes_edges += E * cst;
            stats->ref_passes_nodes += N * (jac + cst);
            stats->exec_passes_edges += E * f.exec_passes;
            stats->sum_iterations += f.iterations;
            stats->sum_final_cost += f.final_cost;
            if (f.termination == LFR_TERM_CONVERGENCE) ++stats->n_converged;
            else if (f.termination == LFR_TERM_NO_CONVERGENCE) ++stats->n_no_convergence;
            else ++stats->n_failed;
            edges += E; nodes += N; refp_e += E * (jac + cst); refp_n += N * (jac + cst);
        }
        if (merged && cls != lfr::KC_BLOCK - 1) continue;
        const int slot = merged ? b->packed_slot : cls;
        ms = 0.f;
        if (recorded >> slot & 1u) {
            const bool al = merged && (recorded & kPackedEventsAliased);
            HIP_TRY(hipEventElapsedTime(&ms, al ? b->ev[0] : b->ev[2 + 2 * slot], al ? b->ev[1] : b->ev[3 + 2 * slot]));
        }
        if (edges > 0 && ms > best_ms) {
            best_ms = ms;
            stats->dominant_kernel_ms = ms; stats->dominant_kernel_edges = edges; stats->dominant_kernel_nodes = nodes;
            stats->dominant_ref_passes_edges = refp_e; stats->dominant_ref_passes_nodes = refp_n;
        }
    }
    return LFR_OK;
}

// A 32-bit control word of the batch's latest solve - of the team words, or of the queue block - read once that solve's stream has
// drained; 0 when nothing has been solved or the batch has no such block.
int64_t read_solve_word(lfr_batch *b, bool team, int word) {
    if (!b) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    const unsigned int *block = team ? b->d_team_ctl : b->d_prof ? lfr::queue_block(b->d_prof) : nullptr;
    if (b->n_solves == 0 || !block) return 0;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    unsigned int v = 0;
    HIP_TRY(hipMemcpy(&v, block + word, sizeof v, hipMemcpyDeviceToHost));
    return (int64_t)v;
}

// lfr_batch_solve (x_start == nullptr: from the origin) and lfr_batch_solve_from (x_start: the start array, b->d_positions for "in
// place") over one launch plan.  The warm kernels read records: a fused batch materialises its records first, whatever its history.
int solve_impl(lfr_batch *b, const double *x_start, hipStream_t st, lfr_solve_stats *stats) {
    KernelArgs a = make_kernel_args(b);
    a.x_start = x_start;
#ifdef LFR_TRACE_TREE
    static unsigned long long *d_trace = nullptr;
    if (!d_trace) { HIP_TRY(hipMalloc(&d_trace, ((size_t)1 << 20) * 8 + 64)); }
    HIP_TRY(hipMemsetAsync(d_trace, 0, 64, st));
    a.trace = d_trace;
#endif
    bool materialised = false;
    // a fused batch that is solved a second time (it is being re-used) or started warm (the warm packed kernel reads records only):
    // write the records once, read them from now on
    if (b->fused && (b->n_solves > 0 || x_start)) {
        lfr::materialize_records(b, st);
        HIP_TRY(hipGetLastError());
        b->fused = false;
        materialised = true;
    }
    if (b->inputs_pending) {             // records rewritten by lfr_batch_set_inputs, possibly on another stream
        if (b->inputs_stream != st) HIP_TRY(hipStreamWaitEvent(st, b->ev_inputs, 0));
        b->inputs_pending = false;
    }
    b->solved_epoch = b->inputs_epoch;
    b->ev = b->ev_ring + (b->n_solves % lfr_batch::kSlots) * lfr_batch::kEvPerSlot;
    uint32_t &recorded = b->ev_recorded[b->n_solves % lfr_batch::kSlots];
    recorded = 0;
    ++b->n_solves;
    b->last_stream = st;
    if (!b->ev[0]) for (int i = 0; i < lfr_batch::kEvPerSlot; ++i) if (!(b->ev[i] = b->ctx->event_acquire(true))) return LFR_ERR_HIP;
    HIP_TRY(hipEventRecord(b->ev[0], st));
    if (b->class_begin[lfr::KC_COUNT] > b->class_begin[lfr::KC_BLOCK]) {
        HIP_TRY(hipStreamWaitEvent(st, b->ev_order, 0));
        HIP_TRY(hipMemsetAsync(a.queue, 0, lfr::kQueueWords * sizeof(unsigned int), st));      // the classes' component queues
        if (b->d_team_ctl) HIP_TRY(hipMemsetAsync(b->d_team_ctl, 0, lfr::solve_geometry().team_ctl_words * sizeof(unsigned int), st));   // registrations, mailboxes, barrier counters of the teams
    }
    { const int rc = b->serial ? launch_serial(b, a, recorded, st) : launch_plan(b, a, materialised, recorded, st); if (rc != LFR_OK) return rc; }
    HIP_TRY(hipEventRecord(b->ev[1], st));
    b->infos_valid = false;
    host_trace("lfr_batch_solve: launched");
    if (!stats) return LFR_OK;

    HIP_TRY(lfr::stream_wait(st));
    { const int rc = read_diagnostics(b, a); if (rc != LFR_OK) return rc; }
    return collect_stats(b, recorded, st, stats);
}

}  // namespace

extern "C" {

int lfr_batch_solve(lfr_batch *b, void *hip_stream, lfr_solve_stats *stats) {
    if (!b) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    host_trace("lfr_batch_solve enters");
    HIP_TRY(hipSetDevice(b->device));
    return solve_impl(b, nullptr, (hipStream_t)hip_stream, stats);
}

int lfr_batch_solve_from(lfr_batch *b, const double *initial_positions_device, void *hip_stream, lfr_solve_stats *stats) {
    if (!b) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    host_trace("lfr_batch_solve_from enters");
    HIP_TRY(hipSetDevice(b->device));
    // NULL: the batch's own positions, started in place - a component reads its nodes in its prologue and nobody else writes them
    return solve_impl(b, initial_positions_device ? initial_positions_device : b->d_positions, (hipStream_t)hip_stream, stats);
}

// Bounded spins that ran out during the batch's latest solve (the hand-off flags of the LDS factorization, the dependency counters of
// the elimination-tree kernel): a timeout rejects an LM step instead of hanging the GPU, so it must be visible - 0 in every test.
int64_t lfr_batch_spin_timeouts(lfr_batch *b) { return read_solve_word(b, false, lfr::kQueueSpinTimeouts); }

// Components the latest solve handed to a TEAM of two or more workgroups (solve_tree_team_kernel); 0 when the batch has none above the
// thresholds (LFR_TREE_TEAM) or no elimination-tree class at all.
int64_t lfr_batch_team_runs(lfr_batch *b) { return read_solve_word(b, true, lfr::kCtlTeamRuns); }

// Components the latest solve's teams could not serve at their size and a single workgroup solved instead (SOLO mode: the comment above
// TeamCtx, Residency) - 0 whenever the launch's workgroups were resident together.
int64_t lfr_batch_team_fallbacks(lfr_batch *b) { return read_solve_word(b, true, lfr::kCtlOffSize); }

// Test infrastructure: `workgroups` 512-thread workgroups of 256 registers per lane (a whole CU each, like the elimination-tree kernel's)
// that do nothing but stay resident for `milliseconds`, on a stream of their own; returns once they have started.
namespace {
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_occupy(unsigned long long ticks, unsigned int *started) {
    extern __shared__ unsigned int occ_lds[];                 // (100 KB of dynamic LDS: no second large workgroup fits the CU either way)
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) { occ_lds[0] = 1u; atomicAdd(started, occ_lds[0]); }
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
}
int lfr_debug_occupy(int device, int workgroups, double milliseconds) {
    if (workgroups < 1 || workgroups > 4096 || !(milliseconds > 0.0) || milliseconds > 2000.0) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    lfr::DevCtx *ctx = lfr::dev_ctx(device);
    if (!ctx) return LFR_ERR_HIP;
    HIP_TRY(hipSetDevice(device));
    static hipStream_t s_occ[16] = {};
    static unsigned int *h_started[16] = {};
    if (device < 0 || device >= 16) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    if (!s_occ[device]) {
        HIP_TRY(hipStreamCreateWithFlags(&s_occ[device], hipStreamNonBlocking));
        HIP_TRY(hipHostMalloc((void **)&h_started[device], 64, hipHostMallocMapped));
    }
    HIP_TRY(hipStreamSynchronize(s_occ[device]));            // (an earlier occupation has ended)
    volatile unsigned int *seen = h_started[device];
    *seen = 0u;
    unsigned int *d_started = nullptr;
    HIP_TRY(hipHostGetDevicePointer((void **)&d_started, h_started[device], 0));
    HIP_TRY(hipFuncSetAttribute((const void *)k_occupy, hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024));
    hipLaunchKernelGGL(k_occupy, dim3((unsigned)workgroups), dim3(512), 100 * 1024, s_occ[device], (unsigned long long)(milliseconds * 1e5), d_started);
    HIP_TRY(hipGetLastError());
    // the workgroups that fit are resident once the count stops growing: at most n_cu of them at a time
    const unsigned want = (unsigned)std::min(workgroups, ctx->n_cu);
    const auto t0 = std::chrono::steady_clock::now();
    while (*seen < want && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() < std::min(milliseconds, 100.0)) std::this_thread::yield();
    return LFR_OK;
}

int lfr_batch_timing(lfr_batch *b, int solves_back, double *total_ms, double *class_ms, int64_t *class_edges) {
    if (!b || solves_back < 0 || solves_back >= lfr_batch::kSlots || solves_back >= b->n_solves) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    HIP_TRY(hipSetDevice(b->device));
    const int ring_slot = (b->n_solves - 1 - solves_back) % lfr_batch::kSlots;
    hipEvent_t *ev = b->ev_ring + ring_slot * lfr_batch::kEvPerSlot;
    const uint32_t recorded = b->ev_recorded[ring_slot];
    HIP_TRY(hipEventSynchronize(ev[1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    if (total_ms) *total_ms = ms;
    for (int cls = 0; cls < lfr::KC_COUNT; ++cls) {
        if (class_ms) {
            ms = 0.f;
            if (recorded >> cls & 1u) {
                const bool al = cls == b->packed_slot && !b->serial && (recorded & kPackedEventsAliased);
                HIP_TRY(hipEventElapsedTime(&ms, al ? ev[0] : ev[2 + 2 * cls], al ? ev[1] : ev[3 + 2 * cls]));
            }
            class_ms[cls] = ms;
        }
        if (class_edges) {      // edges of the LAUNCH timed in this slot (the packed launch carries all packed classes)
            int64_t e = 0;
            const bool packed = !b->serial && cls < lfr::KC_BLOCK;
            const int lo = packed ? (cls == b->packed_slot ? 0 : cls + 1) : cls, hi = packed ? (cls == b->packed_slot ? lfr::KC_BLOCK : cls + 1) : cls + 1;
            for (int c = lo; c < hi; ++c) e += b->class_edges[c];
            class_edges[cls] = e;
        }
    }
    return LFR_OK;
}

// The positions of the whole graph in pinned host memory, valid until the next solve / download / free of this
// batch: waits for the latest solve, one D2H at link speed, no further copy.  Nodes outside this batch's shard
// read 0.
int lfr_batch_positions_view(lfr_batch *b, const double **positions) {
    if (!b || !positions) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    HIP_TRY(hipSetDevice(b->device));
    const size_t bytes = sizeof(double) * 2 * (size_t)std::max<int64_t>(b->n_graph_nodes, 1);
    if (!b->h_positions) {
        b->h_positions = (double *)b->ctx->pinned_acquire(bytes, &b->h_positions_bytes);
        if (!b->h_positions) return LFR_ERR_NOMEM;
    }
    hipStream_t st = b->ctx->s_main;
    host_trace("positions_view enters");
    if (b->n_solves > 0) HIP_TRY(hipStreamWaitEvent(st, b->ev[1], 0));        // end of the latest solve, whatever stream it ran on
    HIP_TRY(hipMemcpyAsync(b->h_positions, b->d_positions, bytes, hipMemcpyDeviceToHost, st));
    host_trace("positions_view: copy issued");
    HIP_TRY(lfr::stream_wait(st));
    host_trace("positions_view: copy done");
    *positions = b->h_positions;
    return LFR_OK;
}

namespace { __global__ void k_positions_to_f32(int64_t n, const double *in, float *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * i + 1 < n) {            // n is even (two coordinates per node): one 16-byte load, one 8-byte store per thread
        const double2 v = reinterpret_cast<const double2 *>(in)[i];
        reinterpret_cast<float2 *>(out)[i] = make_float2((float)v.x, (float)v.y);
    }
} }

int lfr_batch_positions_view_f32(lfr_batch *b, const float **positions) {
    if (!b || !positions) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    HIP_TRY(hipSetDevice(b->device));
    const int64_t n = 2 * std::max<int64_t>(b->n_graph_nodes, 1);
    const size_t bytes = sizeof(float) * (size_t)n;
    if (!b->h_positions_f32) {
        b->h_positions_f32 = (float *)b->ctx->pinned_acquire(bytes, &b->h_positions_f32_bytes);
        if (!b->h_positions_f32) return LFR_ERR_NOMEM;
    }
    if (!b->d_positions_f32) {
        b->d_positions_f32 = (float *)b->ctx->dev_acquire(bytes, &b->d_positions_f32_bytes);
        if (!b->d_positions_f32) return LFR_ERR_NOMEM;
    }
    hipStream_t st = b->ctx->s_main;
    if (b->n_solves > 0) HIP_TRY(hipStreamWaitEvent(st, b->ev[1], 0));        // end of the latest solve, whatever stream it ran on
    hipLaunchKernelGGL(k_positions_to_f32, dim3((unsigned)((n / 2 + 255) / 256)), dim3(256), 0, st, n, b->d_positions, b->d_positions_f32);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_positions_f32, b->d_positions_f32, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(lfr::stream_wait(st));
    *positions = b->h_positions_f32;
    return LFR_OK;
}

int lfr_batch_download(lfr_batch *b, double *positions) {
    if (!b || !positions) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    const double *view = nullptr;
    int rc = lfr_batch_positions_view(b, &view);
    if (rc != LFR_OK) return rc;
    if (b->shard_world == 1) {             // whole problem: every node the batch does not solve is 0 in the view as well
        const size_t n = 2 * (size_t)b->n_graph_nodes;
        const int T = n >= ((size_t)1 << 20) ? 4 : 1;
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t) th.emplace_back([=] { memcpy(positions + n * t / T, view + n * t / T, sizeof(double) * (n * (t + 1) / T - n * t / T)); });
        memcpy(positions, view, sizeof(double) * (n / T));
        for (auto &x : th) x.join();
        return LFR_OK;
    }
    if ((rc = ensure_mirrors(b)) != LFR_OK) return rc;
    for (size_t i = 0; i < b->node_ids.size(); ++i) {      // a shard writes its own nodes only
        const size_t n = b->node_ids[i];
        positions[2 * n] = view[2 * n]; positions[2 * n + 1] = view[2 * n + 1];
    }
    return LFR_OK;
}

int64_t lfr_batch_component_info(lfr_batch *b, int64_t *component, int32_t *iterations, int32_t *termination,
                                 double *final_cost, int32_t *n_var_nodes, int32_t *n_edges) {
    if (!b) return LFR_ERR_ARG;
    if (ensure_mirrors(b) != LFR_OK) return LFR_ERR_HIP;
    if (!b->infos_valid) {
        if (hipSetDevice(b->device) != hipSuccess) return LFR_ERR_HIP;
        b->infos.resize(b->descs.size());
        hipStream_t st = b->ctx->s_main;
        if (b->n_solves > 0 && hipStreamWaitEvent(st, b->ev[1], 0) != hipSuccess) return LFR_ERR_HIP;
        if (!b->descs.empty() &&
            (hipMemcpyAsync(b->infos.data(), b->d_infos, b->descs.size() * sizeof(CompInfoDev), hipMemcpyDeviceToHost, st) != hipSuccess ||
             hipStreamSynchronize(st) != hipSuccess))
            return LFR_ERR_HIP;
        b->infos_valid = true;
    }
    for (size_t i = 0; i < b->descs.size(); ++i) {
        if (component) component[i] = b->desc_component[i];
        if (iterations) iterations[i] = b->infos[i].iterations;
        if (termination) termination[i] = b->infos[i].termination;
        if (final_cost) final_cost[i] = b->infos[i].final_cost;
        if (n_var_nodes) n_var_nodes[i] = b->descs[i].n_var;
        if (n_edges) n_edges[i] = (int32_t)b->descs[i].n_edges;
    }
    return (int64_t)b->descs.size();
}

// Per component (the order of lfr_batch_component_info): what the elimination-tree plan of a component above 192 rows holds - 16-row
// columns, 16x16 tiles of the factor, 16x16x16 left-looking updates per factorization, levels of the elimination tree, sweep items; zeros
// for the components of the other kernel classes.  Lets a checker count the flops and bytes a solve executed (bench.py's roofline).
int64_t lfr_batch_tree_stats(lfr_batch *b, int64_t *columns, int64_t *tiles, int64_t *updates, int64_t *levels, int64_t *items) {
    if (!b) return LFR_ERR_ARG;
    if (ensure_mirrors(b) != LFR_OK) return LFR_ERR_HIP;
    const size_t n = b->descs.size();
    for (size_t i = 0; i < n; ++i) {
        const int64_t k = (int64_t)i - b->tree_begin;
        const bool in = k >= 0 && (size_t)(5 * k + 4) < b->tree_comp_stats.size();
        const int64_t *cs = in ? &b->tree_comp_stats[5 * k] : nullptr;
        if (columns) columns[i] = in ? cs[0] : 0;
        if (tiles) tiles[i] = in ? cs[1] : 0;
        if (updates) updates[i] = in ? cs[2] : 0;
        if (levels) levels[i] = in ? cs[3] : 0;
        if (items) items[i] = in ? cs[4] : 0;
    }
    return (int64_t)n;
}

int lfr_solve_hip(const lfr_problem *p, int device, int tukey_variant, double *positions, lfr_solve_stats *stats) {
    if (!p || !positions) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    lfr_batch *b = nullptr;
    const auto tc0 = std::chrono::steady_clock::now();
    int rc = lfr_batch_create(p, device, 0, 1, tukey_variant, &b);
    if (rc != LFR_OK) return rc;
    std::unique_ptr<lfr_batch> guard(b);
    const auto tc1 = std::chrono::steady_clock::now();
    rc = lfr_batch_solve(b, b->ctx->s_main, stats);         // (no statistics asked for: nothing but the positions leaves the device)
    if (rc != LFR_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    rc = lfr_batch_download(b, positions);
    const auto t1 = std::chrono::steady_clock::now();
    if (stats) stats->d2h_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (getenv("LFR_VERBOSE") || getenv("LFR_TIMING"))
        fprintf(stderr, "lfr: lfr_solve_hip wall: batch creation %.3f ms, solve (+ statistics) %.3f ms, download %.3f ms\n",
                std::chrono::duration<double, std::milli>(tc1 - tc0).count(), std::chrono::duration<double, std::milli>(t0 - tc1).count(),
                std::chrono::duration<double, std::milli>(t1 - t0).count());
    return rc;
}

int lfr_solve_hip_multi(const lfr_problem *p, const int *devices, int n_devices, int tukey_variant, double *positions,
                        lfr_solve_stats *stats) {
    if (!p || !devices || n_devices < 1 || !positions) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    if (n_devices == 1) return lfr_solve_hip(p, devices[0], tukey_variant, positions, stats);
    // one host thread per device (components are independent: no exchange between shards)
    std::vector<int> rcs(n_devices, LFR_OK);
    std::vector<lfr_solve_stats> sts(n_devices);
    std::vector<std::string> errs(n_devices);
    const size_t n = (size_t)p->p.g->n_nodes();
    memset(positions, 0, sizeof(double) * 2 * n);
    // labels-only problems: the labels of the other GPUs come from the GPU that ran the graph stage (peer copies in upload_labels);
    // without such a GPU the host copies are fetched once, before the threads fork
    {
        bool on_a_device = false;
        { std::lock_guard<std::mutex> lk(p->p.label_mu); for (auto &d : p->p.devs) on_a_device = on_a_device || (d && d->track); }
        if (!p->p.host_batch && !on_a_device) { const int rc = p->p.ensure_host_labels(); if (rc != LFR_OK) return rc; }
    }
    auto work = [&](int k) {
        lfr_batch *bt = nullptr;
        rcs[k] = lfr_batch_create(p, devices[k], k, n_devices, tukey_variant, &bt);
        std::unique_ptr<lfr_batch> guard(bt);
        if (rcs[k] == LFR_OK) rcs[k] = lfr_batch_solve(bt, bt->ctx->s_main, &sts[k]);
        if (rcs[k] == LFR_OK) rcs[k] = lfr_batch_download(bt, positions);       // disjoint node sets per shard
        if (rcs[k] != LFR_OK) errs[k] = lfr_last_error();
    };
    std::vector<std::thread> th;
    for (int k = 1; k < n_devices; ++k) th.emplace_back(work, k);
    work(0);
    for (auto &t : th) t.join();
    for (int k = 0; k < n_devices; ++k) if (rcs[k] != LFR_OK) { lfr::set_error("device %d: %s", devices[k], errs[k].c_str()); return rcs[k]; }
    if (stats) {
        *stats = sts[0];
        for (int k = 1; k < n_devices; ++k) {
            const lfr_solve_stats &s = sts[k];
            stats->n_components += s.n_components; stats->n_edges += s.n_edges; stats->n_nodes += s.n_nodes; stats->n_tracks += s.n_tracks;
            stats->n_converged += s.n_converged; stats->n_no_convergence += s.n_no_convergence; stats->n_failed += s.n_failed;
            stats->sum_iterations += s.sum_iterations; stats->ref_jacobian_passes_edges += s.ref_jacobian_passes_edges;
            stats->ref_cost_passes_edges += s.ref_cost_passes_edges; stats->exec_passes_edges += s.exec_passes_edges;
            stats->ref_passes_nodes += s.ref_passes_nodes; stats->sum_final_cost += s.sum_final_cost;
            stats->kernel_ms = std::max(stats->kernel_ms, s.kernel_ms); stats->h2d_ms = std::max(stats->h2d_ms, s.h2d_ms);
        }
    }
    return LFR_OK;
}

// solve.cc:487-641 over several GPUs from one process, the GRAPH STAGE INCLUDED (lfr_solve_hip_multi shards the solve of
// a problem whose tracks / roots / components one GPU computed): device k builds the problem of the connected components of the match
// graph dealt to shard k (lfr_problem_build_hip_shard), assembles, solves and downloads it; when the graph cannot be dealt out (one giant
// connected component) every device holds the whole problem and takes its share of the components, as lfr_solve_hip_multi does.
int lfr_solve_graph_hip_multi(const lfr_graph *g, const int *devices, int n_devices, int64_t max_nodes_in_component, int tukey_variant,
                              double *positions, lfr_problem_stats *problem_stats, lfr_solve_stats *stats) {
    if (!g || !devices || n_devices < 1 || n_devices > 64 || !positions) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    const size_t n = (size_t)g->g.n_nodes();
    memset(positions, 0, sizeof(double) * 2 * n);
    std::vector<int> rcs(n_devices, LFR_OK);
    std::vector<lfr_solve_stats> sts(n_devices);
    std::vector<lfr_problem_stats> pst(n_devices);
    std::vector<int> sharded(n_devices, 0);
    std::vector<std::string> errs(n_devices);
    // entries of the device list that name the same GPU take turns at the graph stage and the assembly (one context, one pair of
    // streams: the stages are written for one caller per device); their solves overlap
    static std::mutex dev_mu[64];
    auto work = [&](int k) {
        lfr_problem *pr = nullptr;
        lfr_batch *bt = nullptr;
        {
            std::lock_guard<std::mutex> turn(dev_mu[devices[k] & 63]);
            rcs[k] = n_devices == 1 ? lfr_problem_build_hip_ex(g, devices[k], max_nodes_in_component, nullptr, 0, &pr)
                                    : lfr_problem_build_hip_shard(g, devices[k], max_nodes_in_component, LFR_BUILD_FLOWS_STAY_ON_HOST, k, n_devices, &pr);
            if (rcs[k] == LFR_OK) {
                sharded[k] = pr->p.cc_sharded ? 1 : 0;
                pst[k] = pr->p.stats;
                rcs[k] = sharded[k] || n_devices == 1 ? lfr_batch_create(pr, devices[k], 0, 1, tukey_variant, &bt)
                                                      : lfr_batch_create(pr, devices[k], k, n_devices, tukey_variant, &bt);
            }
        }
        std::unique_ptr<lfr_batch> guard(bt);
        if (rcs[k] == LFR_OK) rcs[k] = lfr_batch_solve(bt, bt->ctx->s_main, &sts[k]);
        if (rcs[k] == LFR_OK) {
            // disjoint node sets per shard.  A connected-component shard is a WHOLE problem of its own (every other node reads 0 in its
            // view): only its nonzero entries may be written, the other shards' nodes live in the same array
            if (sharded[k] && n_devices > 1) {
                const double *view = nullptr;
                rcs[k] = lfr_batch_positions_view(bt, &view);
                if (rcs[k] == LFR_OK) for (size_t i = 0; i < 2 * n; ++i) if (view[i] != 0.0) positions[i] = view[i];
            } else rcs[k] = lfr_batch_download(bt, positions);
        }
        if (rcs[k] != LFR_OK) errs[k] = lfr_last_error();
        guard.reset();
        if (pr) lfr_problem_free(pr);
    };
    std::vector<std::thread> th;
    for (int k = 1; k < n_devices; ++k) th.emplace_back(work, k);
    work(0);
    for (auto &t : th) t.join();
    for (int k = 0; k < n_devices; ++k) if (rcs[k] != LFR_OK) { lfr::set_error("device %d: %s", devices[k], errs[k].c_str()); return rcs[k]; }
    if (problem_stats) {
        lfr_problem_stats a = pst[0];
        for (int k = 1; k < n_devices; ++k) {
            const lfr_problem_stats &b = pst[k];
            if (sharded[0] && sharded[k]) {                 // per-shard counts add up; a whole-graph problem (no shard) is the same on every device
                a.n_tracks += b.n_tracks; a.n_components += b.n_components; a.n_cut_components += b.n_cut_components;
                a.n_solved_components += b.n_solved_components; a.n_solved_tracks += b.n_solved_tracks;
                a.n_solved_edges += b.n_solved_edges; a.n_solved_nodes += b.n_solved_nodes;
                a.max_track_size = std::max(a.max_track_size, b.max_track_size);
                a.max_component_size = std::max(a.max_component_size, b.max_component_size);
                a.kruskal_rounds = std::max(a.kruskal_rounds, b.kruskal_rounds); a.tie_resorts = std::max(a.tie_resorts, b.tie_resorts);
            }
            a.tracks_ms = std::max(a.tracks_ms, b.tracks_ms); a.roots_ms = std::max(a.roots_ms, b.roots_ms);
            a.graph_cut_ms = std::max(a.graph_cut_ms, b.graph_cut_ms); a.assemble_ms = std::max(a.assemble_ms, b.assemble_ms);
        }
        // a shard keeps the node numbering of the whole graph: the nodes of the OTHER shards are isolated in it, each a track and a
        // component of its own - counted once per foreign shard in the sums above
        int n_sh = 0;
        for (int k = 0; k < n_devices; ++k) n_sh += sharded[k];
        if (sharded[0] && n_sh > 1) { a.n_tracks -= (int64_t)(n_sh - 1) * (int64_t)n; a.n_components -= (int64_t)(n_sh - 1) * (int64_t)n; }
        *problem_stats = a;
    }
    if (stats) {
        *stats = sts[0];
        for (int k = 1; k < n_devices; ++k) {
            const lfr_solve_stats &s2 = sts[k];
            stats->n_components += s2.n_components; stats->n_edges += s2.n_edges; stats->n_nodes += s2.n_nodes; stats->n_tracks += s2.n_tracks;
            stats->n_converged += s2.n_converged; stats->n_no_convergence += s2.n_no_convergence; stats->n_failed += s2.n_failed;
            stats->sum_iterations += s2.sum_iterations; stats->ref_jacobian_passes_edges += s2.ref_jacobian_passes_edges;
            stats->ref_cost_passes_edges += s2.ref_cost_passes_edges; stats->exec_passes_edges += s2.exec_passes_edges;
            stats->ref_passes_nodes += s2.ref_passes_nodes; stats->sum_final_cost += s2.sum_final_cost;
            stats->kernel_ms = std::max(stats->kernel_ms, s2.kernel_ms); stats->h2d_ms = std::max(stats->h2d_ms, s2.h2d_ms);
        }
    }
    return LFR_OK;
}

}  // extern "C"
