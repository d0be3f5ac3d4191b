// Implicit-gradient backward pass through the batched LM solve (lfr_batch_backward, include/lfr.h).
// A translation unit of its own: it reads the batch layout (lfr_batch.hpp) and changes nothing the forward kernels read.  The Hessian's
// assembly and LDL^T are shared with the covariance (lfr_hessian_device.hpp).
//
// Per solved component, one workgroup:
//   1. the EXACT Hessian H of F = sum_e 1/2 w_e rho(|r_e|^2) over the free coordinates at the solve's x (owner computes: the thread of a
//      variable node sums the rows of its two coordinates over the node's out- and in-edges in record order - deterministic), the
//      caller's dL/dx as right-hand side, bound coordinates (|x| >= 1) replaced by identity rows / columns and a zero right-hand side;
//   2. LDL^T of H (right-looking; the update of column k touches only the pairs of NONZERO entries of column k, so the tree-plus-cycles
//      systems of the size cap cost what their fill costs, not n^3) and v = H^-1 ubar.  A pivot that is not positive (or not finite)
//      marks the component indefinite: its gradient stays zero;
//   3. the vector-Jacobian sweep: one thread per record writes -d/dtheta_e [v . grad F_e] into the match layout of the graph.
// The packed lower triangle of H lives in LDS for the classes of up to 192 rows (<= 148 KB) and in an HBM workspace above.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <cstring>
#include <vector>

#include "lfr_batch.hpp"
#include "lfr_hessian_device.hpp"

using namespace lfrdev;
using lfr::ensure_mirrors;

namespace {

constexpr int kBwdThreadsSmall = 64;         // packed classes (<= 32 rows): one wave per component
constexpr int kBwdThreads = 256;             // workgroup classes

template <int T, bool LDS_MATRIX>
__global__ __launch_bounds__(T) void backward_kernel(const BwdArgs a) {
    extern __shared__ double bsh[];
    const int di = a.desc_begin + blockIdx.x, tid = threadIdx.x;
    const CompDesc d = a.descs[di];
    const int nv = d.n_var, n = 2 * nv;
    if (a.infos[di].termination == LFR_TERM_FAILURE) {       // not usable: zero gradient (the outputs were cleared)
        if (tid == 0) a.status[di] = 1;
        return;
    }
    double *H = LDS_MATRIX ? bsh : a.hws + a.hws_off[di];
    double *v = LDS_MATRIX ? bsh + bwd_tri(n, 0) : bsh;           // rhs, then the solution
    double *lval = v + n;                                     // column k's nonzeros: values and rows
    int *lidx = reinterpret_cast<int *>(lval + n);
    uint8_t *fr = reinterpret_cast<uint8_t *>(lidx + n);
    __shared__ int cnt[2];
    const EdgeRec *E = a.edges + d.edge_off;
    const uint32_t *ids = a.node_ids + d.node_off;

    // 1. free coordinates, right-hand side, zero matrix
    unsigned long long n_bound = 0;
    for (int i = tid; i < n; i += T) {
        const size_t g = 2 * (size_t)ids[i >> 1] + (i & 1);
        const bool f = fabs(a.positions[g]) < kBound;
        fr[i] = f;
        v[i] = f ? a.grad_pos[g] : 0.0;
        n_bound += !f;
    }
    if (n_bound) atomicAdd(a.counters, n_bound);
    const size_t nt = bwd_tri(n, 0);
    for (size_t t = tid; t < nt; t += T) H[t] = 0.0;
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();

    // 2. assembly (owner computes, deterministic)
    auto xof = [&](int m, int c) -> double { return m < nv ? a.positions[2 * (size_t)ids[m] + c] : 0.0; };
    bwd_assemble<T, true>(a, d, nv, E, ids, H, fr, tid);
    __syncthreads();

    // 3. LDL^T over the nonzeros of each column
    const bool indefinite = bwd_ldlt<T>(H, n, lval, lidx, cnt, tid);
    if (indefinite) {                                         // zero gradient
        if (tid == 0) a.status[di] = 2;
        return;
    }
    // 4. v = L^-T D^-1 L^-1 ubar
    for (int k = 0; k < n; ++k) {
        const double vk = v[k];
        for (int i = k + 1 + tid; i < n; i += T) v[i] -= H[bwd_tri(i, k)] * vk;
        __syncthreads();
    }
    for (int i = tid; i < n; i += T) v[i] /= H[bwd_tri(i, i)];
    __syncthreads();
    for (int i = n - 1; i > 0; --i) {
        const double vi = v[i];
        for (int k = tid; k < i; k += T) v[k] -= H[bwd_tri(i, k)] * vi;
        __syncthreads();
    }

    // 5. vector-Jacobian sweep: per record, -d/dtheta [v . grad F_e] scattered to the edge's match row
    for (uint32_t p = tid; p < d.n_edges; p += T) {
        const EdgeRec e = E[p];
        const int s = e.src, m = e.dst_kind & 0x7fff, kind = e.dst_kind >> 15;
        const double vs0 = s < nv ? v[2 * s] : 0., vs1 = s < nv ? v[2 * s + 1] : 0.;
        const double vd0 = m < nv ? v[2 * m] : 0., vd1 = m < nv ? v[2 * m + 1] : 0.;
        BwdEdge o;
        bwd_eval(e, kind, a.tukey_variant, xof(s, 0), xof(s, 1), xof(m, 0), xof(m, 1), o);
        const double a0 = vd0 - (1.0 + o.fr[0]) * vs0 - o.fc[0] * vs1;      // a = J v = v_dst - P v_src
        const double a1 = vd1 - o.fr[1] * vs0 - (1.0 + o.fc[1]) * vs1;
        const double ra = o.r[0] * a0 + o.r[1] * a1;
        const uint32_t id = a.eid[d.edge_off + p];
        if ((id >> 1) >= a.n_matches) continue;               // (cannot happen: every record maps to an edge of the graph)
        const size_t row = 18 * (size_t)(id >> 1);
        void *out = (id & 1u) ? a.g_disp1 : a.g_disp2;
        a.g_sim_dir[id] = -o.rho1 * ra;
        const double q2 = 2.0 * o.w * o.rho2 * ra, q1 = o.w * o.rho1;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double A = o.lr[i] * o.lc[j], B = o.dlr[i] * o.lc[j] * vs0 + o.lr[i] * o.dlc[j] * vs1;
                const double g0 = q2 * o.r[0] * A + q1 * (A * a0 + o.r[0] * B);
                const double g1 = q2 * o.r[1] * A + q1 * (A * a1 + o.r[1] * B);
                const size_t at = row + 2 * (3 * i + j);
                if (a.f64) { static_cast<double *>(out)[at] = g0; static_cast<double *>(out)[at + 1] = g1; }
                else { static_cast<float *>(out)[at] = (float)g0; static_cast<float *>(out)[at + 1] = (float)g1; }
            }
    }
    if (tid == 0) a.status[di] = 0;
}

__global__ void k_bwd_sim(int64_t n_matches, const double *dir, void *out, int f64) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_matches) return;
    const double g = dir[2 * m] + dir[2 * m + 1];
    if (f64) static_cast<double *>(out)[m] = g; else static_cast<float *>(out)[m] = (float)g;
}

size_t bwd_lds_bytes(int rows, bool lds_matrix) {
    return (lds_matrix ? bwd_tri(rows, 0) * 8 : 0) + (size_t)rows * (8 + 8 + 4 + 1) + 16;
}

}  // namespace

struct BwdState {
    lfr::DevArena slab;
    double *d_gsim = nullptr, *d_hws = nullptr;
    uint64_t *d_hws_off = nullptr;
    int32_t *d_status = nullptr;
    unsigned long long *d_counters = nullptr;
    int rows_max[lfr::KC_COUNT] = {0};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t last_stream = nullptr;
    int64_t n_calls = 0;
};

void bwd_free(BwdState *s) {
    if (!s) return;
    if (s->last_stream || s->n_calls) (void)hipStreamSynchronize(s->last_stream);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    delete s;
}

hipEvent_t bwd_last_event(const BwdState *s) { return s && s->n_calls ? s->ev1 : nullptr; }

namespace {

int bwd_setup(lfr_batch *b) {
    int rc = ensure_mirrors(b);
    if (rc != LFR_OK) return rc;
    std::unique_ptr<BwdState> s(new BwdState());
    if ((rc = lfr::ensure_edge_map(b)) != LFR_OK) return rc;     // (records -> edges of the graph: the batch's own, shared with lfr_batch_set_inputs)
    const size_t nd = std::max<size_t>(b->descs.size(), 1);
    const size_t M = (size_t)std::max<int64_t>(b->n_graph_matches, 1);
    std::vector<uint64_t> off(nd, 0);
    uint64_t hws = 0;
    for (size_t i = 0; i < b->descs.size(); ++i) {
        const int cls = b->desc_class[i], rows = 2 * b->descs[i].n_var;
        s->rows_max[cls] = std::max(s->rows_max[cls], rows);
        if (cls == lfr::KC_GLOBAL) {
            if (rows > kBwdMaxRows) { lfr::set_error("backward: a component of %d rows exceeds the dense backward's %d", rows, kBwdMaxRows); return LFR_ERR_UNSUPPORTED; }
            off[i] = hws; hws += bwd_tri(rows, 0);
        }
    }
    const size_t bytes = 16 * M + 8 * hws + 8 * nd + 4 * nd + 64 + ((size_t)1 << 16);
    if (!s->slab.init(b->ctx, bytes)) return LFR_ERR_NOMEM;
    s->d_gsim = s->slab.take_n<double>(2 * M);
    s->d_hws = s->slab.take_n<double>(std::max<uint64_t>(hws, 1));
    s->d_hws_off = s->slab.take_n<uint64_t>(nd);
    s->d_status = s->slab.take_n<int32_t>(nd);
    s->d_counters = s->slab.take_n<unsigned long long>(8);
    if (!s->d_gsim || !s->d_hws || !s->d_hws_off || !s->d_status || !s->d_counters) { lfr::set_error("backward slab exhausted"); return LFR_ERR_NOMEM; }
    HIP_TRY(hipEventCreate(&s->ev0)); HIP_TRY(hipEventCreate(&s->ev1));
    hipStream_t st = b->ctx->s_main;
    HIP_TRY(hipMemcpyAsync(s->d_hws_off, off.data(), 8 * nd, hipMemcpyHostToDevice, st));
    b->bwd = s.release();
    HIP_TRY(lfr::stream_wait(st));
    HIP_TRY(hipFuncSetAttribute((const void *)backward_kernel<kBwdThreads, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)bwd_lds_bytes(lfr::kBlockMaxRows, true)));
    HIP_TRY(hipFuncSetAttribute((const void *)backward_kernel<kBwdThreads, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)bwd_lds_bytes(kBwdMaxRows, false)));
    return LFR_OK;
}

}  // namespace

extern "C" {

int lfr_batch_positions_to_device(lfr_batch *b, double *dst_device, void *hip_stream) {
    if (!b || !dst_device) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (b->n_solves > 0) HIP_TRY(hipStreamWaitEvent(st, b->ev[1], 0));        // end of the latest solve, whatever stream it ran on
    HIP_TRY(hipMemcpyAsync(dst_device, b->d_positions, sizeof(double) * 2 * (size_t)b->n_graph_nodes, hipMemcpyDeviceToDevice, st));
    return LFR_OK;
}

int lfr_batch_backward(lfr_batch *b, const double *grad_positions_device, void *grad_disp1_device, void *grad_disp2_device,
                       void *grad_sim_device, int flags, void *hip_stream, lfr_backward_stats *stats) {
    if (!b || !grad_positions_device || !grad_disp1_device || !grad_disp2_device || !grad_sim_device || (flags & ~LFR_BACKWARD_F64)) {
        lfr::set_error("bad argument"); return LFR_ERR_ARG;
    }
    if (b->n_solves == 0) { lfr::set_error("lfr_batch_backward: the batch has not been solved"); return LFR_ERR_ARG; }
    if (b->inputs_epoch != b->solved_epoch) { lfr::set_error("lfr_batch_backward: inputs changed since the latest solve"); return LFR_ERR_ARG; }
    HIP_TRY(hipSetDevice(b->device));
    if (!b->bwd) { const int rc = bwd_setup(b); if (rc != LFR_OK) return rc; }
    BwdState &s = *b->bwd;
    hipStream_t st = (hipStream_t)hip_stream;
    const int f64 = (flags & LFR_BACKWARD_F64) ? 1 : 0;
    const size_t M = (size_t)b->n_graph_matches, elt = f64 ? 8 : 4;
    HIP_TRY(hipStreamWaitEvent(st, b->ev[1], 0));                               // the latest solve's positions and termination codes
    HIP_TRY(hipEventRecord(s.ev0, st));
    if (b->fused) lfr::materialize_records(b, st);     // the packed records have not been written yet: write them (the next solve would write the same bytes)
    if (M) {
        HIP_TRY(hipMemsetAsync(grad_disp1_device, 0, 18 * M * elt, st));
        HIP_TRY(hipMemsetAsync(grad_disp2_device, 0, 18 * M * elt, st));
        HIP_TRY(hipMemsetAsync(s.d_gsim, 0, 16 * M, st));
    }
    HIP_TRY(hipMemsetAsync(s.d_counters, 0, 64, st));
    BwdArgs a;
    a.descs = b->d_descs; a.edges = b->d_edges; a.node_ids = b->d_node_ids; a.node_inc = b->d_node_inc; a.in_idx = b->d_in_idx;
    a.positions = b->d_positions; a.infos = b->d_infos; a.grad_pos = grad_positions_device;
    a.eid = lfr::edge_map(b);
    a.hws = s.d_hws; a.hws_off = s.d_hws_off; a.g_disp1 = grad_disp1_device; a.g_disp2 = grad_disp2_device; a.g_sim_dir = s.d_gsim;
    a.status = s.d_status; a.counters = s.d_counters; a.tukey_variant = b->tukey_variant; a.f64 = f64;
    a.n_matches = (uint32_t)M;
    // packed classes (<= 32 rows): one wave each; LDS classes: 256 threads, matrix in LDS; above 192 rows: matrix in HBM
    {
        a.desc_begin = b->class_begin[0];
        const int n = b->class_begin[lfr::KC_BLOCK] - a.desc_begin;
        a.scan_all = 1;
        if (n > 0)
            hipLaunchKernelGGL((backward_kernel<kBwdThreadsSmall, true>), dim3(n), dim3(kBwdThreadsSmall), bwd_lds_bytes(32, true), st, a);
    }
    a.scan_all = 0;
    for (int cls = lfr::KC_BLOCK; cls < lfr::KC_COUNT; ++cls) {
        a.desc_begin = b->class_begin[cls];
        const int n = b->class_begin[cls + 1] - a.desc_begin, rows = std::max(s.rows_max[cls], 2);
        if (n <= 0) continue;
        if (cls == lfr::KC_GLOBAL)
            hipLaunchKernelGGL((backward_kernel<kBwdThreads, false>), dim3(n), dim3(kBwdThreads), bwd_lds_bytes(rows, false), st, a);
        else
            hipLaunchKernelGGL((backward_kernel<kBwdThreads, true>), dim3(n), dim3(kBwdThreads), bwd_lds_bytes(rows, true), st, a);
    }
    if (M) hipLaunchKernelGGL(k_bwd_sim, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (int64_t)M, s.d_gsim, grad_sim_device, f64);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.ev1, st));
    s.last_stream = st;
    ++s.n_calls;
    if (stats) {
        HIP_TRY(hipEventSynchronize(s.ev1));
        std::vector<int32_t> status(b->descs.size());
        unsigned long long cnt[8];
        if (!status.empty()) HIP_TRY(hipMemcpyAsync(status.data(), s.d_status, 4 * status.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(cnt, s.d_counters, sizeof(cnt), hipMemcpyDeviceToHost, st));
        HIP_TRY(lfr::stream_wait(st));
        memset(stats, 0, sizeof(*stats));
        for (int32_t v : status) {
            if (v == 0) ++stats->n_differentiated;
            else if (v == 1) ++stats->n_not_usable;
            else ++stats->n_indefinite;
        }
        stats->n_bound_coordinates = (int64_t)cnt[0];
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s.ev0, s.ev1));
        stats->kernel_ms = ms;
    }
    return LFR_OK;
}

int64_t lfr_batch_backward_status(lfr_batch *b, int32_t *status) {
    if (!b || !b->bwd || !b->bwd->n_calls) { lfr::set_error("lfr_batch_backward_status: no backward has run on this batch"); return LFR_ERR_ARG; }
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipEventSynchronize(b->bwd->ev1));
    const size_t n = b->descs.size();
    if (status && n) {
        HIP_TRY(hipMemcpyAsync(status, b->bwd->d_status, 4 * n, hipMemcpyDeviceToHost, b->bwd->last_stream));
        HIP_TRY(lfr::stream_wait(b->bwd->last_stream));
    }
    return (int64_t)n;
}

}  // extern "C"
