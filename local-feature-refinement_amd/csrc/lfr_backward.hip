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
//
// Gauss-Newton mode (LFR_BACKWARD_GAUSS_NEWTON): H = J^T J of the loss-corrected Jacobian over the free coordinates - the matrix of the LM
// loop and of the covariance, positive definite wherever the exact Hessian is not - and everything else as above.  The workgroup
// classes run the same kernel with the other assembly; the packed classes (<= 32 rows) run backward_gn_packed_kernel: ONE launch in
// the covariance's layout (lfr_packed_normal_device.hpp: 64/S components per wave64, one-wave workgroups, no barriers), its sweep and
// its in-register inversion with the bound rows and columns replaced by the identity's, v = C ubar as one dot product per lane, then the
// vector-Jacobian sweep over the re-read records.
//
// Gauss-Newton fallback (LFR_BACKWARD_FALLBACK_GAUSS_NEWTON): the exact mode's launches with FB = true.  A workgroup whose exact
// Hessian is indefinite clears the triangle, assembles J^T J over the same free set and factors again (bwd_refactor_gauss_newton);
// the right-hand side is untouched.  Status 0: the exact mode's bits; 3: the Gauss-Newton matrix; 2: both failed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "lfr_batch.hpp"
#include "lfr_hessian_device.hpp"
#include "lfr_packed_normal_device.hpp"

using namespace lfrdev;
using lfr::PackedRanges;

namespace {

constexpr int kBwdThreadsSmall = 64;         // exact mode, packed classes (<= 32 rows): one wave per component (Gauss-Newton mode: backward_gn_packed_kernel)
constexpr int kBwdThreads = 256;             // workgroup classes

// The vector-Jacobian sweep of one record: -d/dtheta_e [v . grad F_e(x^; theta_e)] to the edge's match row and its directed-edge slot
// of dL/dsim.  (xs, xd), (vs, vd): x^ and v = H^-1 ubar at the record's source and destination (0 for constants); id: its directed edge.
__device__ __forceinline__ void bwd_sweep_edge(const BwdArgs &a, const EdgeRec &e, const int kind, const double xs0, const double xs1,
                                               const double xd0, const double xd1, const double vs0, const double vs1, const double vd0,
                                               const double vd1, const uint32_t id) {
    BwdEdge o;
    bwd_eval(e, kind, a.tukey_variant, xs0, xs1, xd0, xd1, o);
    const double a0 = vd0 - (1.0 + o.fr[0]) * vs0 - o.fc[0] * vs1;      // a = J v = v_dst - P v_src
    const double a1 = vd1 - o.fr[1] * vs0 - (1.0 + o.fc[1]) * vs1;
    const double ra = o.r[0] * a0 + o.r[1] * a1;
    if ((id >> 1) >= a.n_matches) return;                 // (cannot happen: every record maps to an edge of the graph)
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

// GN: H is the loss-corrected Gauss-Newton matrix (bwd_assemble<T, false, true>) instead of the exact Hessian
// FB: the exact Hessian, and where bwd_ldlt finds it indefinite the Gauss-Newton matrix in the same workgroup (status 3).  A template
// parameter, not a field of the arguments: the instantiations of the two pure modes stay the code they were
template <int T, bool LDS_MATRIX, bool GN, bool FB = false>
__global__ __launch_bounds__(T) void backward_kernel(const BwdArgs a) {
    static_assert(!(GN && FB), "the fallback starts from the exact Hessian");
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
    bwd_assemble<T, !GN, true>(a, d, nv, E, ids, H, fr, tid);
    __syncthreads();

    // 3. LDL^T over the nonzeros of each column
    bool indefinite = bwd_ldlt<T>(H, n, lval, lidx, cnt, tid);
    int status = 0;
    if constexpr (FB) {
        if (indefinite) {                                     // (block-uniform) the exact Hessian is indefinite: J^T J, same v, same fr
            indefinite = bwd_refactor_gauss_newton<T>(a, d, nv, E, ids, H, n, fr, lval, lidx, cnt, tid);
            status = 3;
        }
    }
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
        bwd_sweep_edge(a, e, kind, xof(s, 0), xof(s, 1), xof(m, 0), xof(m, 1), vs0, vs1, vd0, vd1, a.eid[d.edge_off + p]);
    }
    if (tid == 0) a.status[di] = status;
}

// ---- Gauss-Newton mode, packed classes (<= 32 rows): the covariance's layout (lfr_packed_normal_device.hpp) ----
template <int NV>
struct alignas(16) BwdGnLds {
    CovLds<NV> c;              // J^T J and x^
    double u[NV];              // ubar of the free coordinates, 0 elsewhere
    double v[NV + 2];          // v = H^-1 ubar; slots 2*n_var, 2*n_var+1 stay 0 (constants)
};

template <int KC>
__device__ __forceinline__ void bwd_gn_group_body(const BwdArgs &a, const int desc_begin, const int desc_end, const int block_in_class,
                                                  unsigned char *lds_raw) {
    constexpr int NV = PackedClass<KC>::NV, S = PackedClass<KC>::S, EPL = PackedClass<KC>::EPL, LD = NV + 1;
    PackedGroup<KC> grp;
    if (!grp.init(a.descs, desc_begin, desc_end, block_in_class)) return;
    const int gid = grp.gid, sl = grp.sl, ci = grp.ci;
    const int row = sl % NV, part = sl / NV;
    const bool have = grp.have;
    const CompDesc &d = grp.d;
    BwdGnLds<NV> &B = reinterpret_cast<BwdGnLds<NV> *>(lds_raw)[gid];
    CovLds<NV> &L = B.c;

    const bool usable = have && a.infos[ci].termination != LFR_TERM_FAILURE;
    const int n_var = usable ? grp.n_var : 0, nv2 = 2 * n_var, E = usable ? grp.E : 0;     // a group without a usable component inverts the identity
    const bool is_row = row < nv2;
    const int nv2_max = cov_wave_max(nv2);

    // the lane's coordinate: bound (|x^| >= 1) or free, its dL/dx; the group's bound rows as a mask (bit = row)
    const size_t coord = is_row ? 2 * (size_t)a.node_ids[d.node_off + (row >> 1)] + (row & 1) : 0;
    const bool bound = is_row && !(fabs(a.positions[coord]) < kBound);
    const uint32_t bmask = (uint32_t)(__builtin_amdgcn_ballot_w64(bound) >> (gid * S)) & (NV == 32 ? 0xffffffffu : (1u << NV) - 1u);
    if (sl == 0 && bmask) atomicAdd(a.counters, (unsigned long long)__popc(bmask));       // (once per coordinate: the low half of <32,2>)
    if (part == 0) B.u[row] = (is_row && !bound) ? a.grad_pos[coord] : 0.0;
    if (sl < 2) B.v[NV + sl] = 0.0;
    cov_lds_init<NV, S>(a, d, n_var, sl, L);
    wave_lds_sync();
    cov_assemble<NV, S, EPL, false>(a, d, n_var, E, sl, L);      // J^T J at x^, the covariance's sweep
    wave_lds_sync();

    // ---- inversion with the bound rows and columns the identity's, lane = row; v = C ubar ----
    const double *A = L.A;
    bool solved = false;
    cov_invert<KC>(row, nv2_max,
        [&](int c) -> double {
            double h = 0.0;
            if (is_row && c < nv2) h = (c <= row ? A[row * LD + c] : A[c * LD + row]);
            const bool fixed = !is_row || bound || ((bmask >> c) & 1u);       // padded and bound rows are identity
            return fixed ? (c == row ? 1.0 : 0.0) : h;
        },
        [&](auto &h, const bool ok) {
            constexpr int CL = sizeof(h) / sizeof(double);
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < CL; ++c) acc = fma(h[c], B.u[c], acc);
            if (part == 0) B.v[row] = is_row ? acc : 0.0;
            // cov_invert's test (the smallest pivot > 0) lets a NaN pivot pass; bwd_ldlt rejects one.  A NaN or infinite pivot leaves a
            // v that is not finite, so the group's v decides with it: status 2 means the same in every launch class
            const unsigned long long bad = __builtin_amdgcn_ballot_w64(is_row && !isfinite(acc));       // (every lane is active here)
            constexpr unsigned long long kGroup = S == 64 ? ~0ull : (1ull << S) - 1ull;
            solved = ok && !((bad >> (gid * S)) & kGroup);
        });
    if (have && sl == 0) a.status[ci] = !usable ? 1 : solved ? 0 : 2;
    wave_lds_sync();
    if (!solved) return;                              // a pivot was not positive: zero gradient (the outputs were cleared)

    // ---- vector-Jacobian sweep over the re-read records ----
    const EdgeRec *R = a.edges + d.edge_off;
    const uint32_t *eid = a.eid + d.edge_off;
#pragma unroll 1
    for (int p = sl; p < E; p += S) {
        const EdgeRec e = R[p];
        const int s = min((int)e.src, n_var), m = min((int)(e.dst_kind & 0x7fff), n_var), kind = e.dst_kind >> 15;     // constants read the zero slots
        bwd_sweep_edge(a, e, kind, L.x[2 * s], L.x[2 * s + 1], L.x[2 * m], L.x[2 * m + 1], B.v[2 * s], B.v[2 * s + 1], B.v[2 * m],
                       B.v[2 * m + 1], eid[p]);
    }
}

constexpr size_t kBwdGnLdsBytes = 4 * sizeof(BwdGnLds<16>) > 2 * sizeof(BwdGnLds<32>) ? 4 * sizeof(BwdGnLds<16>) : 2 * sizeof(BwdGnLds<32>);
static_assert(kBwdGnLdsBytes >= 8 * sizeof(BwdGnLds<8>), "LDS budget");

// all packed classes in ONE launch, the blocks dealt to the classes as in covariance_packed_kernel
__global__ __launch_bounds__(64, 2) void backward_gn_packed_kernel(const BwdArgs a, const PackedRanges r) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kBwdGnLdsBytes];
    packed_dispatch(r, [&](auto kc, int desc_begin, int desc_end, int block_in_class) LFR_INLINE_LAMBDA {
        bwd_gn_group_body<decltype(kc)::value>(a, desc_begin, desc_end, block_in_class, lds_raw);
    });
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

// the shared state of a pass behind a solve (lfr_batch.hpp) + the backward's own: dL/dsim per directed edge, {bound coordinates, ...}
struct BwdState : lfr::PassState {
    double *d_gsim = nullptr;
    unsigned long long *d_counters = nullptr;
};

int bwd_setup_extra(lfr_batch *b, lfr::PassState *ps) {
    BwdState *s = static_cast<BwdState *>(ps);
    const int rc = lfr::ensure_edge_map(b);     // (records -> edges of the graph: the batch's own, shared with lfr_batch_set_inputs)
    if (rc != LFR_OK) return rc;
    s->d_gsim = s->slab.take_n<double>(2 * (size_t)std::max<int64_t>(b->n_graph_matches, 1));
    s->d_counters = s->slab.take_n<unsigned long long>(8);
    if (!s->d_gsim || !s->d_counters) { lfr::set_error("backward slab exhausted"); return LFR_ERR_NOMEM; }
    const int lds_block = (int)bwd_lds_bytes(lfr::kBlockMaxRows, true), lds_global = (int)bwd_lds_bytes(kBwdMaxRows, false);
    HIP_TRY(hipFuncSetAttribute((const void *)backward_kernel<kBwdThreads, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_block));
    HIP_TRY(hipFuncSetAttribute((const void *)backward_kernel<kBwdThreads, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_global));
    HIP_TRY(hipFuncSetAttribute((const void *)backward_kernel<kBwdThreads, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_block));
    HIP_TRY(hipFuncSetAttribute((const void *)backward_kernel<kBwdThreads, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_global));
    HIP_TRY(hipFuncSetAttribute((const void *)backward_kernel<kBwdThreads, true, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_block));
    HIP_TRY(hipFuncSetAttribute((const void *)backward_kernel<kBwdThreads, false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_global));
    return LFR_OK;
}

const lfr::PassKind kBackward = {"backward", [] { return static_cast<lfr::PassState *>(new BwdState()); }, bwd_setup_extra};

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
    if (!b || !grad_positions_device || !grad_disp1_device || !grad_disp2_device || !grad_sim_device ||
        (flags & ~(LFR_BACKWARD_F64 | LFR_BACKWARD_GAUSS_NEWTON | LFR_BACKWARD_FALLBACK_GAUSS_NEWTON))) {
        lfr::set_error("bad argument"); return LFR_ERR_ARG;
    }
    if ((flags & LFR_BACKWARD_GAUSS_NEWTON) && (flags & LFR_BACKWARD_FALLBACK_GAUSS_NEWTON)) {
        lfr::set_error("lfr_batch_backward: LFR_BACKWARD_GAUSS_NEWTON and LFR_BACKWARD_FALLBACK_GAUSS_NEWTON exclude each other"); return LFR_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int f64 = (flags & LFR_BACKWARD_F64) ? 1 : 0;
    const bool gn = (flags & LFR_BACKWARD_GAUSS_NEWTON) != 0, fb = (flags & LFR_BACKWARD_FALLBACK_GAUSS_NEWTON) != 0;
    const size_t M = (size_t)b->n_graph_matches, elt = f64 ? 8 : 4;
    { const int rc = lfr::pass_begin(b, &b->bwd, kBackward, 16 * std::max<size_t>(M, 1) + 64, st); if (rc != LFR_OK) return rc; }
    BwdState &s = *static_cast<BwdState *>(b->bwd);
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
    // Packed classes (<= 32 rows).  Gauss-Newton mode: ONE launch of one-wave blocks, each wave hosting 64/S = 2-8 components (1 in
    // <32,2>), dealt to the classes as lfr_batch_covariance deals its own.  Exact mode (with or without the fallback): backward_kernel, one wave per component.
    if (gn) {
        a.desc_begin = b->class_begin[0]; a.scan_all = 0;
        lfr::launch_packed_pass(b, backward_gn_packed_kernel, a, st);
    } else {
        a.desc_begin = b->class_begin[0];
        const int n = b->class_begin[lfr::KC_BLOCK] - a.desc_begin;
        a.scan_all = 1;
        if (n > 0 && fb)
            hipLaunchKernelGGL((backward_kernel<kBwdThreadsSmall, true, false, true>), dim3(n), dim3(kBwdThreadsSmall), bwd_lds_bytes(32, true), st, a);
        else if (n > 0)
            hipLaunchKernelGGL((backward_kernel<kBwdThreadsSmall, true, false>), dim3(n), dim3(kBwdThreadsSmall), bwd_lds_bytes(32, true), st, a);
    }
    // Workgroup classes, every mode: one workgroup of 256 threads per component; matrix in LDS up to 192 rows, in HBM above
    a.scan_all = 0;
    for (int cls = lfr::KC_BLOCK; cls < lfr::KC_COUNT; ++cls) {
        a.desc_begin = b->class_begin[cls];
        const int n = b->class_begin[cls + 1] - a.desc_begin, rows = std::max(s.rows_max[cls], 2);
        if (n <= 0) continue;
        const bool lds_matrix = cls != lfr::KC_GLOBAL;
        const size_t lds = bwd_lds_bytes(rows, lds_matrix);
        if (fb && lds_matrix) hipLaunchKernelGGL((backward_kernel<kBwdThreads, true, false, true>), dim3(n), dim3(kBwdThreads), lds, st, a);
        else if (fb) hipLaunchKernelGGL((backward_kernel<kBwdThreads, false, false, true>), dim3(n), dim3(kBwdThreads), lds, st, a);
        else if (!lds_matrix && gn) hipLaunchKernelGGL((backward_kernel<kBwdThreads, false, true>), dim3(n), dim3(kBwdThreads), lds, st, a);
        else if (!lds_matrix) hipLaunchKernelGGL((backward_kernel<kBwdThreads, false, false>), dim3(n), dim3(kBwdThreads), lds, st, a);
        else if (gn) hipLaunchKernelGGL((backward_kernel<kBwdThreads, true, true>), dim3(n), dim3(kBwdThreads), lds, st, a);
        else hipLaunchKernelGGL((backward_kernel<kBwdThreads, true, false>), dim3(n), dim3(kBwdThreads), lds, st, a);
    }
    if (M) hipLaunchKernelGGL(k_bwd_sim, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (int64_t)M, s.d_gsim, grad_sim_device, f64);
    HIP_TRY(hipGetLastError());
    { const int rc = lfr::pass_end(&s, st); if (rc != LFR_OK) return rc; }
    if (stats) {
        unsigned long long cnt[8];
        int64_t count[3];
        memset(stats, 0, sizeof(*stats));
        HIP_TRY(hipMemcpyAsync(cnt, s.d_counters, sizeof(cnt), hipMemcpyDeviceToHost, st));       // (pass_histogram waits for st)
        { const int rc = lfr::pass_histogram(b, &s, st, count, &stats->kernel_ms); if (rc != LFR_OK) return rc; }
        stats->n_differentiated = count[0]; stats->n_not_usable = count[1]; stats->n_indefinite = count[2];
        stats->n_bound_coordinates = (int64_t)cnt[0];
    }
    return LFR_OK;
}

int64_t lfr_batch_backward_status(lfr_batch *b, int32_t *status) { return lfr::pass_status(b, b ? b->bwd : nullptr, "backward", status); }

}  // extern "C"
