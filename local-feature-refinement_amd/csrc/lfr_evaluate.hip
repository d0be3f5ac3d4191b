// Objective, gradient, residuals and loss weights at given positions (lfr_batch_evaluate, include/lfr.h).
// A translation unit of its own: it reads the batch layout (lfr_batch.hpp), the packed record loader, the group reductions and the
// logarithm of lfr_device.hpp, and changes nothing the solve, the backward or the covariance read.
//
// Per component F_c = sum_e 1/2 w_e rho(|r_e|^2) at the caller's positions (or the batch's own), dF/dx per variable coordinate, and
// per record the raw residual and rho' in the graph's match layout:
//   packed classes (<= 32 rows)   ONE launch in the forward's layout: a wave64 hosts 64/S components, one-wave workgroups, no barriers,
//                                 sub-lane sl takes records sl + S k: every record is read once.  Positions in the group's LDS
//                                 (constants read a zero slot), the cost a fixed-order butterfly over the group's lanes, the gradient
//                                 accumulated in the group's LDS and stored by one lane per coordinate.
//   workgroup classes (above)     one workgroup per component, owner computes: the thread of a node walks the node's out-edges (cost
//                                 term, per-match outputs, source side of the gradient) and in-edges (destination side) in record
//                                 order; constant nodes walk their out-edges only, so every record is stored exactly once.  The cost
//                                 is a wave-then-block tree.  No matrix, hence no row limit.
// No fp64 value goes through a global-memory atomic; nothing depends on the order in which waves or workgroups run.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "lfr_batch.hpp"
#include "lfr_device.hpp"

using namespace lfrdev;
using lfr::CompDesc;
using lfr::EdgeRec;
using lfr::PackedRanges;

namespace {

constexpr int kEvalThreads = 256;              // workgroup classes

struct EvalArgs {
    const CompDesc *descs;
    const EdgeRec *edges;
    const uint32_t *node_ids;
    const lfr::NodeInc *node_inc;
    const uint32_t *in_idx;
    const double *positions;   // 2 per node of the whole graph: the caller's or the batch's
    const uint32_t *eid;       // per record: directed edge id of the graph (nullptr: no per-match output)
    double *cost;              // per descriptor
    double *grad;              // 2 per node of the whole graph (cleared before the launches), or nullptr
    void *res, *wts;           // n_matches x 4 / n_matches x 2, float or double (cleared / set to -1 before the launches), or nullptr
    uint32_t n_dir;            // 2 * n_matches
    int desc_begin, tukey_variant, f64;
};

// One residual block at (x1 = source, x2 = destination): raw residual, its cost term 1/2 w rho(s), rho'(s) and the two sides of
// dF/dx.  The interpolant is summed separably as in eval_edge; its first derivative is zeroed outside [-0.5, 0.5] and kept at exactly
// +-0.5 (cost.cc:38-43).  A residual that is not finite makes every output of the block not finite, in both losses (Tukey's
// comparison is written so that a NaN takes the arithmetic branch).
struct EvalEdge {
    double r0, r1, term, rho1;
    double gs0, gs1, gd0, gd1;           // d term / d x1, d term / d x2
};

__device__ __forceinline__ void eval_basis(const double x, double (&l)[3], double (&dl)[3]) {
    const double t = fmax(fmin(x, 0.5), -0.5);
    const bool in = (t == x);
    l[0] = 2. * t * (t - .5); l[1] = (-4.) * (t - .5) * (t + .5); l[2] = 2. * t * (t + .5);
    dl[0] = in ? 2. * t + 2. * (t - .5) : 0.; dl[1] = in ? (-4.) * (t - .5) + (-4.) * (t + .5) : 0.; dl[2] = in ? 2. * t + 2. * (t + .5) : 0.;
}

__device__ __forceinline__ void eval_block(const float (&flow)[18], const float simf, const int kind, const int tukey_variant,
                                           const double x1r, const double x1c, const double x2r, const double x2c, EvalEdge &o) {
    double lr[3], dlr[3], lc[3], dlc[3];
    eval_basis(x1r, lr, dlr);
    eval_basis(x1c, lc, dlc);
    double f0 = 0., f1 = 0., fr0 = 0., fr1 = 0., fc0 = 0., fc1 = 0.;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a0 = (double)flow[6 * i], a1 = (double)flow[6 * i + 1], b0 = (double)flow[6 * i + 2], b1 = (double)flow[6 * i + 3],
                     c0 = (double)flow[6 * i + 4], c1 = (double)flow[6 * i + 5];
        const double t0 = lc[0] * a0 + lc[1] * b0 + lc[2] * c0, t1 = lc[0] * a1 + lc[1] * b1 + lc[2] * c1;
        const double u0 = dlc[0] * a0 + dlc[1] * b0 + dlc[2] * c0, u1 = dlc[0] * a1 + dlc[1] * b1 + dlc[2] * c1;
        f0 += lr[i] * t0; f1 += lr[i] * t1;
        fr0 += dlr[i] * t0; fr1 += dlr[i] * t1;
        fc0 += lr[i] * u0; fc1 += lr[i] * u1;
    }
    const double r0 = x2r - x1r - f0, r1 = x2c - x1c - f1;
    const double s = r0 * r0 + r1 * r1;
    const double w = (double)simf;
    double rho0, rho1;
    if (kind == 0) {                                   // CauchyLoss(0.25)
        const double sum = 1.0 + s * kCauchyC;
        rho0 = kCauchyB * log_ge1(sum);
        rho1 = 1.0 / sum;
    } else {                                           // TukeyLoss(0.0625), Ceres 1.x (1) or 2.x (2)
        const double k0 = (tukey_variant == 1) ? kTukeyA2 / 6.0 : kTukeyA2 / 3.0, k1 = (tukey_variant == 1) ? 0.5 : 1.0;
        if (!(s > kTukeyA2)) {                         // (a NaN comes here and stays a NaN)
            const double v = 1.0 - s / kTukeyA2, v2 = v * v;
            rho0 = k0 * (1.0 - v2 * v);
            rho1 = k1 * v2;
        } else { rho0 = k0; rho1 = 0.0; }
    }
    o.r0 = r0; o.r1 = r1; o.rho1 = rho1;
    o.term = 0.5 * (w * rho0);
    const double c = w * rho1;
    o.gd0 = c * r0; o.gd1 = c * r1;
    // P = I + df/dx1 = [[1 + fr0, fc0], [fr1, 1 + fc1]]: the source side is -c P^T r
    o.gs0 = -(c * ((1.0 + fr0) * r0 + fr1 * r1));
    o.gs1 = -(c * (fc0 * r0 + (1.0 + fc1) * r1));
}

__device__ __forceinline__ void eval_store_match(const EvalArgs &a, const uint32_t id, const EvalEdge &o) {
    if (id >= a.n_dir) return;                         // (cannot happen: every record maps to an edge of the graph)
    if (a.f64) {
        if (a.res) { double *r = static_cast<double *>(a.res) + 2 * (size_t)id; r[0] = o.r0; r[1] = o.r1; }
        if (a.wts) static_cast<double *>(a.wts)[id] = o.rho1;
    } else {
        if (a.res) { float *r = static_cast<float *>(a.res) + 2 * (size_t)id; r[0] = (float)o.r0; r[1] = (float)o.r1; }
        if (a.wts) static_cast<float *>(a.wts)[id] = (float)o.rho1;
    }
}

// ---- packed classes ----
template <int NV>
struct alignas(16) EvalLds {
    double x[NV + 2];          // positions; slots 2*n_var, 2*n_var+1 stay 0 (constants)
    double g[NV + 2];          // dF/dx
};

template <int CLS, int EPL>
__device__ __forceinline__ void eval_group_body(const EvalArgs &a, const int desc_begin, const int desc_end, const int block_in_class,
                                                unsigned char *lds_raw) {
    constexpr int NV = CLS == 0 ? 8 : CLS == 1 ? 16 : 32, LPR = CLS == 3 ? 2 : 1;
    constexpr int S = NV * LPR, G = 64 / S;
    const int lane = threadIdx.x & 63;
    const int gid = lane / S, sl = lane % S;
    const int ci0 = desc_begin + block_in_class * G;
    if (ci0 >= desc_end) return;                      // wave-uniform
    const int ci = ci0 + gid;
    const bool have = ci < desc_end;
    EvalLds<NV> &L = reinterpret_cast<EvalLds<NV> *>(lds_raw)[gid];

    CompDesc d;
    d.edge_off = 0; d.n_edges = 0; d.node_off = 0; d.n_nodes = 0; d.n_var = 0;
    if (have) d = a.descs[ci];
    const int n_var = min((int)d.n_var, NV / 2), nv2 = 2 * n_var, E = min((int)d.n_edges, S * EPL);      // (the class limits: classify())
    for (int i = sl; i < NV + 2; i += S) {
        L.x[i] = (i < nv2) ? a.positions[2 * (size_t)a.node_ids[d.node_off + (i >> 1)] + (i & 1)] : 0.0;
        L.g[i] = 0.0;
    }
    wave_lds_sync();

    double cost = 0.0;
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
        const int p = sl + S * k;
        if (!(p < E)) continue;
        float flow_k[18]; float sim_k; uint32_t pk;
        load_packed_edge<false>(a, d.edge_off + p, flow_k, sim_k, pk);
        const int es = (int)(pk & 0xffffu), ed = (int)((pk >> 16) & 0x7fffu), ekind = (int)(pk >> 31);
        const int xa = 2 * min(es, n_var), xb = 2 * min(ed, n_var);      // constants read the zero slot
        EvalEdge o;
        eval_block(flow_k, sim_k, ekind, a.tukey_variant, L.x[xa], L.x[xa + 1], L.x[xb], L.x[xb + 1], o);
        cost += o.term;
        if (a.grad) {
            if (es < n_var) { atomicAdd(&L.g[xa], o.gs0); atomicAdd(&L.g[xa + 1], o.gs1); }
            if (ed < n_var) { atomicAdd(&L.g[xb], o.gd0); atomicAdd(&L.g[xb + 1], o.gd1); }
        }
        if (a.eid) eval_store_match(a, a.eid[d.edge_off + p], o);
    }
    wave_lds_sync();
    cost = group_sum<S>(cost);                       // every lane of the wave is active; the butterfly stays inside the group
    if (have && sl == 0) a.cost[ci] = cost;
    if (a.grad && sl < nv2) a.grad[2 * (size_t)a.node_ids[d.node_off + (sl >> 1)] + (sl & 1)] = L.g[sl];
}

constexpr size_t kEvalPackedLdsBytes = 8 * sizeof(EvalLds<8>);
static_assert(kEvalPackedLdsBytes >= 4 * sizeof(EvalLds<16>) && kEvalPackedLdsBytes >= 2 * sizeof(EvalLds<32>), "LDS budget");

// all packed classes in ONE launch, the blocks dealt to the classes as in solve_packed_kernel
__global__ __launch_bounds__(64) void evaluate_packed_kernel(const EvalArgs a, const PackedRanges r) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kEvalPackedLdsBytes];
    const int b = (int)blockIdx.x;
    if (b < r.blk_begin[1]) eval_group_body<3, 5>(a, r.desc_begin[0], r.desc_end[0], b - r.blk_begin[0], lds_raw);
    else if (b < r.blk_begin[2]) eval_group_body<2, 6>(a, r.desc_begin[1], r.desc_end[1], b - r.blk_begin[1], lds_raw);
    else if (b < r.blk_begin[3]) { /* retired class, never assigned */ }
    else if (b < r.blk_begin[4]) eval_group_body<1, 6>(a, r.desc_begin[3], r.desc_end[3], b - r.blk_begin[3], lds_raw);
    else eval_group_body<0, 3>(a, r.desc_begin[4], r.desc_end[4], b - r.blk_begin[4], lds_raw);
}

// ---- workgroup classes ----
template <int T>
__global__ __launch_bounds__(T) void evaluate_block_kernel(const EvalArgs a) {
    __shared__ double wave_cost[T / 64];
    const int di = a.desc_begin + blockIdx.x, tid = threadIdx.x;
    const CompDesc d = a.descs[di];
    const int nv = d.n_var, nn = d.n_nodes;
    const uint32_t ne = d.n_edges;
    const uint32_t *ids = a.node_ids + d.node_off;
    auto xof = [&](int m, int c) -> double { return m < nv ? a.positions[2 * (size_t)ids[m] + c] : 0.0; };
    double cost = 0.0;
    for (int l = tid; l < nn; l += T) {                       // variable nodes, then the constants (out-edges only)
        const lfr::NodeInc ni = a.node_inc[d.node_off + l];
        const double xr = xof(l, 0), xc = xof(l, 1);
        double g0 = 0.0, g1 = 0.0;
        for (uint32_t k = 0; k < ni.out_count; ++k) {         // l -> m
            const uint32_t p = ni.out_begin + k;
            if (p >= ne) break;                               // (cannot happen: a run lies inside its component)
            float fl[18]; float sm; uint32_t pk;
            load_packed_edge<false>(a, d.edge_off + p, fl, sm, pk);
            const int m = (int)((pk >> 16) & 0x7fffu), kind = (int)(pk >> 31);
            EvalEdge o;
            eval_block(fl, sm, kind, a.tukey_variant, xr, xc, xof(m, 0), xof(m, 1), o);
            cost += o.term;
            g0 += o.gs0; g1 += o.gs1;
            if (a.eid) eval_store_match(a, a.eid[d.edge_off + p], o);
        }
        if (!a.grad || l >= nv) continue;
        for (uint32_t k = 0; k < ni.in_count; ++k) {          // m -> l
            if (ni.in_begin + k >= ne) break;
            const uint32_t p = a.in_idx[d.edge_off + ni.in_begin + k];
            if (p >= ne) break;
            float fl[18]; float sm; uint32_t pk;
            load_packed_edge<false>(a, d.edge_off + p, fl, sm, pk);
            const int m = (int)(pk & 0xffffu), kind = (int)(pk >> 31);
            EvalEdge o;
            eval_block(fl, sm, kind, a.tukey_variant, xof(m, 0), xof(m, 1), xr, xc, o);
            g0 += o.gd0; g1 += o.gd1;
        }
        a.grad[2 * (size_t)ids[l]] = g0; a.grad[2 * (size_t)ids[l] + 1] = g1;
    }
    // the cost: a butterfly inside each wave, then the waves in order
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cost += __shfl_xor(cost, m, 64);
    if ((tid & 63) == 0) wave_cost[tid >> 6] = cost;
    __syncthreads();
    if (tid == 0) {
        double c = wave_cost[0];
#pragma unroll
        for (int w = 1; w < T / 64; ++w) c += wave_cost[w];
        a.cost[di] = c;
    }
}

// weights of the directions that are no residual block of this shard
__global__ void k_eval_fill_minus_one(size_t n, void *out, int f64) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (f64) static_cast<double *>(out)[i] = -1.0; else static_cast<float *>(out)[i] = -1.0f;
}

// the shared state of a pass (events, latest stream: lfr_batch.hpp) + a cost per descriptor for calls without cost_device.  Set up by
// this unit, not by pass_begin: the evaluate needs neither a solve nor unchanged inputs, and no workspace for matrices.
struct EvalState : lfr::PassState {
    double *d_cost = nullptr;
    std::vector<double> h_cost;
};

int eval_setup(lfr_batch *b) {
    std::unique_ptr<lfr::PassState, void (*)(lfr::PassState *)> guard(new EvalState(), lfr::pass_free);      // every error path releases slab and events
    EvalState *s = static_cast<EvalState *>(guard.get());
    const size_t nd = std::max<size_t>((size_t)b->n_desc, 1);
    if (!s->slab.init(b->ctx, 8 * nd + 4096)) return LFR_ERR_NOMEM;
    s->d_cost = s->slab.take_n<double>(nd);
    if (!s->d_cost) { lfr::set_error("evaluate slab exhausted"); return LFR_ERR_NOMEM; }
    HIP_TRY(hipEventCreate(&s->ev0)); HIP_TRY(hipEventCreate(&s->ev1));
    b->eval = guard.release();
    return LFR_OK;
}

}  // namespace

extern "C" {

int lfr_batch_evaluate(lfr_batch *b, const double *positions_device, double *cost_device, double *grad_positions_device,
                       void *residuals_device, void *weights_device, int flags, void *hip_stream, lfr_evaluate_stats *stats) {
    if (!b) { lfr::set_error("lfr_batch_evaluate: no batch"); return LFR_ERR_ARG; }
    if (flags & ~LFR_EVALUATE_F64) { lfr::set_error("lfr_batch_evaluate: unknown flag bits 0x%x", flags & ~LFR_EVALUATE_F64); return LFR_ERR_ARG; }
    if (!cost_device && !grad_positions_device && !residuals_device && !weights_device) {
        lfr::set_error("lfr_batch_evaluate: nothing to evaluate (all four outputs are NULL)"); return LFR_ERR_ARG;
    }
    if (!positions_device && b->n_solves == 0) {
        lfr::set_error("lfr_batch_evaluate: the batch has not been solved and no positions are given"); return LFR_ERR_ARG;
    }
    const bool per_match = residuals_device || weights_device;
    if (per_match && b->cc_sharded) {
        lfr::set_error("lfr_batch_evaluate: a batch over one rank's connected components numbers its matches by itself (lfr_problem_build_hip_shard): no per-match outputs");
        return LFR_ERR_UNSUPPORTED;
    }
    HIP_TRY(hipSetDevice(b->device));
    if (per_match) { const int rc = lfr::ensure_edge_map(b); if (rc != LFR_OK) return rc; }
    if (!b->eval) { const int rc = eval_setup(b); if (rc != LFR_OK) return rc; }
    EvalState &s = *static_cast<EvalState *>(b->eval);
    hipStream_t st = (hipStream_t)hip_stream;
    const int f64 = (flags & LFR_EVALUATE_F64) ? 1 : 0;
    const size_t M = (size_t)b->n_graph_matches, N = (size_t)b->n_graph_nodes, elt = f64 ? 8 : 4;
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
    if (grad_positions_device && N) HIP_TRY(hipMemsetAsync(grad_positions_device, 0, 2 * N * sizeof(double), st));
    if (residuals_device && M) HIP_TRY(hipMemsetAsync(residuals_device, 0, 4 * M * elt, st));
    if (weights_device && M) hipLaunchKernelGGL(k_eval_fill_minus_one, dim3((unsigned)((2 * M + 255) / 256)), dim3(256), 0, st, 2 * M, weights_device, f64);

    EvalArgs a;
    memset(&a, 0, sizeof(a));
    a.descs = b->d_descs; a.edges = b->d_edges; a.node_ids = b->d_node_ids; a.node_inc = b->d_node_inc; a.in_idx = b->d_in_idx;
    a.positions = positions_device ? positions_device : b->d_positions;
    a.eid = per_match ? lfr::edge_map(b) : nullptr;
    a.cost = cost_device ? cost_device : s.d_cost;
    a.grad = grad_positions_device; a.res = residuals_device; a.wts = weights_device;
    a.n_dir = (uint32_t)(2 * M); a.tukey_variant = b->tukey_variant; a.f64 = f64;
    {   // packed classes: one launch of one-wave blocks, dealt as lfr_batch_solve deals its own
        PackedRanges r;
        int nb = 0;
        lfr::packed_ranges(b, 1, &r, &nb);
        if (nb > 0) hipLaunchKernelGGL(evaluate_packed_kernel, dim3(nb), dim3(64), 0, st, a, r);
    }
    {   // workgroup classes: one workgroup per component, all classes in one launch (they are contiguous in the batch order)
        a.desc_begin = b->class_begin[lfr::KC_BLOCK];
        const int n = b->class_begin[lfr::KC_COUNT] - a.desc_begin;
        if (n > 0) hipLaunchKernelGGL((evaluate_block_kernel<kEvalThreads>), dim3(n), dim3(kEvalThreads), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    { const int rc = lfr::pass_end(&s, st); if (rc != LFR_OK) return rc; }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        s.h_cost.assign((size_t)b->n_desc, 0.0);
        if (b->n_desc) HIP_TRY(hipMemcpyAsync(s.h_cost.data(), a.cost, 8 * (size_t)b->n_desc, hipMemcpyDeviceToHost, st));
        HIP_TRY(lfr::stream_wait(st));
        for (const double c : s.h_cost) {
            if (std::isfinite(c)) stats->sum_cost += c; else ++stats->n_nonfinite;
        }
        stats->n_components = b->n_desc;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s.ev0, s.ev1));
        stats->kernel_ms = ms;
    }
    return LFR_OK;
}

}  // extern "C"
