// Forward-mode sensitivity of the refined positions (lfr_batch_jvp, include/lfr.h): xdot = J thetadot, J = dx^/dtheta,
// the other half of lfr_batch_backward's J^T ubar.  A translation unit of its own: it reads the batch layout (lfr_batch.hpp), shares
// the Hessian's assembly and LDL^T with the backward and the covariance (lfr_hessian_device.hpp) and the packed Gauss-Newton matrix
// and its inversion with the covariance (lfr_packed_normal_device.hpp), and changes nothing an existing kernel reads.
//
// Per solved component H xdot = b with the backward's H (exact or Gauss-Newton, bound coordinates the identity's) and
// b = -sum_e d/d eps [grad_x F_e(x^; theta_e + eps thetadot_e)] on the free coordinates (jvp_rhs_edge), 0 on bound ones:
//   jvp_kernel            backward_kernel with its first and last step exchanged for their transposes: the right-hand side is built
//                         owner-computes (the thread of a variable node sums its two rows over the node's out- and in-edges in record
//                         order, the traversal of bwd_assemble), then the assembly, the LDL^T, the two substitutions, and xdot goes to
//                         the component's nodes.  One wave per component for the classes of up to 32 rows in the exact mode.
//   jvp_gn_packed_kernel  Gauss-Newton mode, classes of up to 32 rows: ONE launch in the covariance's layout.  The sweep adds the
//                         records' terms into the group's LDS vector, the matrix is inverted in registers, xdot_row = C_row . b.
// LFR_JVP_FALLBACK_GAUSS_NEWTON: jvp_kernel with FB = true, the backward's fallback (bwd_refactor_gauss_newton) on the same matrix with
// the same code - equal statuses - and the right-hand side, built once, survives the first factorization.
// No fp64 value goes through a global-memory atomic; a component's output depends on nothing outside the component.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "lfr_batch.hpp"
#include "lfr_hessian_device.hpp"
#include "lfr_packed_normal_device.hpp"

using namespace lfrdev;
using lfr::PackedRanges;

namespace {

constexpr int kJvpThreadsSmall = 64;         // exact mode, packed classes (<= 32 rows): one wave per component
constexpr int kJvpThreads = 256;             // workgroup classes

struct JvpArgs {
    BwdArgs h;                 // what bwd_assemble / cov_assemble read (grad_pos, g_*: unused)
    JvpTangent t;              // thetadot in the match layout
    double *xdot;              // 2 per node of the whole graph (cleared before the launches)
};

// the two rows of record e (directed edge id) at its source and at its destination
__device__ __forceinline__ void jvp_record(const JvpArgs &ja, const EdgeRec &e, const uint32_t id, const double xs0, const double xs1,
                                           const double xd0, const double xd1, double (&bs)[2], double (&bd)[2]) {
    BwdEdge o;
    bwd_eval(e, e.dst_kind >> 15, ja.h.tukey_variant, xs0, xs1, xd0, xd1, o);
    double phidot[18], wdot;
    jvp_load_tangent(ja.t, id, phidot, wdot);
    jvp_rhs_edge(o, phidot, wdot, bs, bd);
}

// GN: H is the loss-corrected Gauss-Newton matrix (bwd_assemble<T, false, true>) instead of the exact Hessian
// FB: the exact Hessian, and where bwd_ldlt finds it indefinite the Gauss-Newton matrix in the same workgroup (status 3).  A template
// parameter, not a field of the arguments: the instantiations of the two pure modes stay the code they were
template <int T, bool LDS_MATRIX, bool GN, bool FB = false>
__global__ __launch_bounds__(T) void jvp_kernel(const JvpArgs ja) {
    static_assert(!(GN && FB), "the fallback starts from the exact Hessian");
    extern __shared__ double jsh[];
    const BwdArgs &a = ja.h;
    const int di = a.desc_begin + blockIdx.x, tid = threadIdx.x;
    const CompDesc d = a.descs[di];
    const int nv = d.n_var, n = 2 * nv;
    if (a.infos[di].termination == LFR_TERM_FAILURE) {       // not usable: zero tangent (the output was cleared)
        if (tid == 0) a.status[di] = 1;
        return;
    }
    double *H = LDS_MATRIX ? jsh : a.hws + a.hws_off[di];
    double *v = LDS_MATRIX ? jsh + bwd_tri(n, 0) : jsh;           // rhs, then the solution
    double *lval = v + n;                                     // column k's nonzeros: values and rows
    int *lidx = reinterpret_cast<int *>(lval + n);
    uint8_t *fr = reinterpret_cast<uint8_t *>(lidx + n);
    __shared__ int cnt[2];
    const EdgeRec *E = a.edges + d.edge_off;
    const uint32_t *eid = a.eid + d.edge_off;
    const uint32_t *ids = a.node_ids + d.node_off;

    // 1. free coordinates, zero matrix
    unsigned long long n_bound = 0;
    for (int i = tid; i < n; i += T) {
        const bool f = fabs(a.positions[2 * (size_t)ids[i >> 1] + (i & 1)]) < kBound;
        fr[i] = f;
        n_bound += !f;
    }
    if (n_bound) atomicAdd(a.counters, n_bound);
    const size_t nt = bwd_tri(n, 0);
    for (size_t t = tid; t < nt; t += T) H[t] = 0.0;
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();

    // 2. right-hand side (owner computes, deterministic: bwd_assemble's traversal), then the matrix
    auto xof = [&](int m, int c) -> double { return m < nv ? a.positions[2 * (size_t)ids[m] + c] : 0.0; };
    for (int l = tid; l < nv; l += T) {
        lfr::NodeInc ni = a.node_inc[d.node_off + l];
        if (a.scan_all) { ni.out_begin = 0; ni.out_count = d.n_edges; ni.in_count = 0; }
        const double xr = xof(l, 0), xc = xof(l, 1);
        double b0 = 0.0, b1 = 0.0, bs[2], bd[2];
        for (uint32_t k = 0; k < ni.out_count; ++k) {         // l -> m (packed classes: and m -> l)
            const uint32_t p = ni.out_begin + k;
            if (p >= d.n_edges) break;                        // (cannot happen: a run lies inside its component)
            const EdgeRec e = E[p];
            const int m = e.dst_kind & 0x7fff;
            if (a.scan_all && e.src != l) {
                if (m != l) continue;
                jvp_record(ja, e, eid[p], xof(e.src, 0), xof(e.src, 1), xr, xc, bs, bd);       // in-edge e.src -> l
                b0 += bd[0]; b1 += bd[1];
                continue;
            }
            jvp_record(ja, e, eid[p], xr, xc, xof(m, 0), xof(m, 1), bs, bd);
            b0 += bs[0]; b1 += bs[1];
        }
        for (uint32_t k = 0; k < ni.in_count; ++k) {          // m -> l
            if (ni.in_begin + k >= d.n_edges) break;
            const uint32_t p = a.in_idx[d.edge_off + ni.in_begin + k];
            if (p >= d.n_edges) break;
            const EdgeRec e = E[p];
            jvp_record(ja, e, eid[p], xof(e.src, 0), xof(e.src, 1), xr, xc, bs, bd);
            b0 += bd[0]; b1 += bd[1];
        }
        v[2 * l] = fr[2 * l] ? b0 : 0.0;
        v[2 * l + 1] = fr[2 * l + 1] ? b1 : 0.0;
    }
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
    if (indefinite) {                                         // zero tangent
        if (tid == 0) a.status[di] = 2;
        return;
    }
    // 4. v = L^-T D^-1 L^-1 b
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

    // 5. xdot to the component's nodes; a bound coordinate is an exact 0 (also beside a tangent that is not finite)
    for (int i = tid; i < n; i += T) ja.xdot[2 * (size_t)ids[i >> 1] + (i & 1)] = fr[i] ? v[i] : 0.0;
    if (tid == 0) a.status[di] = status;
}

// ---- Gauss-Newton mode, packed classes (<= 32 rows): the covariance's layout (lfr_packed_normal_device.hpp) ----
template <int NV>
struct alignas(16) JvpGnLds {
    CovLds<NV> c;              // J^T J and x^
    double b[NV + 2];          // the right-hand side; slots 2*n_var, 2*n_var+1 take the constants' rows (never read)
};

template <int KC>
__device__ __forceinline__ void jvp_gn_group_body(const JvpArgs &ja, const int desc_begin, const int desc_end, const int block_in_class,
                                                  unsigned char *lds_raw) {
    constexpr int NV = PackedClass<KC>::NV, S = PackedClass<KC>::S, EPL = PackedClass<KC>::EPL, LD = NV + 1;
    const BwdArgs &a = ja.h;
    PackedGroup<KC> grp;
    if (!grp.init(a.descs, desc_begin, desc_end, block_in_class)) return;
    const int gid = grp.gid, sl = grp.sl, ci = grp.ci;
    const int row = sl % NV, part = sl / NV;
    const bool have = grp.have;
    const CompDesc &d = grp.d;
    JvpGnLds<NV> &B = reinterpret_cast<JvpGnLds<NV> *>(lds_raw)[gid];
    CovLds<NV> &L = B.c;

    const bool usable = have && a.infos[ci].termination != LFR_TERM_FAILURE;
    const int n_var = usable ? grp.n_var : 0, nv2 = 2 * n_var, E = usable ? grp.E : 0;     // a group without a usable component inverts the identity
    const bool is_row = row < nv2;
    const int nv2_max = cov_wave_max(nv2);

    // the lane's coordinate: bound (|x^| >= 1) or free; the group's bound rows as a mask (bit = row)
    const size_t coord = is_row ? 2 * (size_t)a.node_ids[d.node_off + (row >> 1)] + (row & 1) : 0;
    const bool bound = is_row && !(fabs(a.positions[coord]) < kBound);
    const uint32_t bmask = (uint32_t)(__builtin_amdgcn_ballot_w64(bound) >> (gid * S)) & (NV == 32 ? 0xffffffffu : (1u << NV) - 1u);
    if (sl == 0 && bmask) atomicAdd(a.counters, (unsigned long long)__popc(bmask));       // (once per coordinate: the low half of <32,2>)
    for (int i = sl; i < NV + 2; i += S) B.b[i] = 0.0;
    cov_lds_init<NV, S>(a, d, n_var, sl, L);
    wave_lds_sync();
    cov_assemble<NV, S, EPL, false>(a, d, n_var, E, sl, L);      // J^T J at x^, the covariance's sweep
    wave_lds_sync();

    // ---- the right-hand side: lane sl takes records sl + S k and adds their two rows into the group's vector.  One wave issues the
    // LDS adds in program order, and one ds_add_f64 serialises its same-address lanes in a fixed order: the sum is repeatable ----
    const EdgeRec *R = a.edges + d.edge_off;
    const uint32_t *eid = a.eid + d.edge_off;
#pragma unroll 1
    for (int p = sl; p < E; p += S) {
        const EdgeRec e = R[p];
        const int s = min((int)e.src, n_var), m = min((int)(e.dst_kind & 0x7fff), n_var);      // constants: the spare slots
        double bs[2], bd[2];
        jvp_record(ja, e, eid[p], L.x[2 * s], L.x[2 * s + 1], L.x[2 * m], L.x[2 * m + 1], bs, bd);
        atomicAdd(&B.b[2 * s], bs[0]); atomicAdd(&B.b[2 * s + 1], bs[1]);
        atomicAdd(&B.b[2 * m], bd[0]); atomicAdd(&B.b[2 * m + 1], bd[1]);
    }
    wave_lds_sync();
    if (part == 0 && (bound || !is_row)) B.b[row] = 0.0;         // bound and padded rows: zero right-hand side
    wave_lds_sync();

    // ---- inversion with the bound rows and columns the identity's, lane = row; xdot_row = C_row . b ----
    const double *A = L.A;
    bool solved = false;
    double xd = 0.0;
    cov_invert<KC>(row, nv2_max,
        [&](int c) -> double {
            double h = 0.0;
            if (is_row && c < nv2) h = (c <= row ? A[row * LD + c] : A[c * LD + row]);
            const bool fixed = !is_row || bound || ((bmask >> c) & 1u);       // padded and bound rows are identity
            return fixed ? (c == row ? 1.0 : 0.0) : h;
        },
        [&](auto &h, const bool ok) {
            constexpr int CL = sizeof(h) / sizeof(double);
            double acc = 0.0, mag = 0.0;
#pragma unroll
            for (int c = 0; c < CL; ++c) { acc = fma(h[c], B.b[c], acc); mag += fabs(h[c]); }
            xd = acc;
            // cov_invert's test (the smallest pivot > 0) lets a NaN pivot pass; bwd_ldlt rejects one.  A NaN or infinite pivot leaves an
            // inverse that is not finite, so the group's rows of C decide with it (not xdot: a tangent that is not finite keeps status 0)
            const unsigned long long bad = __builtin_amdgcn_ballot_w64(is_row && !isfinite(mag));       // (every lane is active here)
            constexpr unsigned long long kGroup = ~0ull >> (64 - S);
            solved = ok && !((bad >> (gid * S)) & kGroup);
        });
    if (have && sl == 0) a.status[ci] = !usable ? 1 : solved ? 0 : 2;
    if (solved && is_row && part == 0) ja.xdot[coord] = bound ? 0.0 : xd;       // (not solved: zero tangent, the output was cleared)
}

constexpr size_t kJvpGnLdsBytes = 4 * sizeof(JvpGnLds<16>) > 2 * sizeof(JvpGnLds<32>) ? 4 * sizeof(JvpGnLds<16>) : 2 * sizeof(JvpGnLds<32>);
static_assert(kJvpGnLdsBytes >= 8 * sizeof(JvpGnLds<8>), "LDS budget");

// all packed classes in ONE launch, the blocks dealt to the classes as in covariance_packed_kernel
__global__ __launch_bounds__(64, 2) void jvp_gn_packed_kernel(const JvpArgs a, const PackedRanges r) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kJvpGnLdsBytes];
    packed_dispatch(r, [&](auto kc, int desc_begin, int desc_end, int block_in_class) LFR_INLINE_LAMBDA {
        jvp_gn_group_body<decltype(kc)::value>(a, desc_begin, desc_end, block_in_class, lds_raw);
    });
}

size_t jvp_lds_bytes(int rows, bool lds_matrix) {             // (backward_kernel's carving)
    return (lds_matrix ? bwd_tri(rows, 0) * 8 : 0) + (size_t)rows * (8 + 8 + 4 + 1) + 16;
}

// the shared state of a pass behind a solve (lfr_batch.hpp) + the jvp's own: {bound coordinates, ...}
struct JvpState : lfr::PassState {
    unsigned long long *d_counters = nullptr;
};

int jvp_setup_extra(lfr_batch *b, lfr::PassState *ps) {
    JvpState *s = static_cast<JvpState *>(ps);
    const int rc = lfr::ensure_edge_map(b);     // (records -> edges of the graph: the batch's own, shared with backward and set_inputs)
    if (rc != LFR_OK) return rc;
    s->d_counters = s->slab.take_n<unsigned long long>(8);
    if (!s->d_counters) { lfr::set_error("jvp slab exhausted"); return LFR_ERR_NOMEM; }
    const int lds_block = (int)jvp_lds_bytes(lfr::kBlockMaxRows, true), lds_global = (int)jvp_lds_bytes(kBwdMaxRows, false);
    HIP_TRY(hipFuncSetAttribute((const void *)jvp_kernel<kJvpThreads, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_block));
    HIP_TRY(hipFuncSetAttribute((const void *)jvp_kernel<kJvpThreads, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_global));
    HIP_TRY(hipFuncSetAttribute((const void *)jvp_kernel<kJvpThreads, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_block));
    HIP_TRY(hipFuncSetAttribute((const void *)jvp_kernel<kJvpThreads, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_global));
    HIP_TRY(hipFuncSetAttribute((const void *)jvp_kernel<kJvpThreads, true, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_block));
    HIP_TRY(hipFuncSetAttribute((const void *)jvp_kernel<kJvpThreads, false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_global));
    return LFR_OK;
}

const lfr::PassKind kJvp = {"jvp", [] { return static_cast<lfr::PassState *>(new JvpState()); }, jvp_setup_extra};

}  // namespace

extern "C" {

int lfr_batch_jvp(lfr_batch *b, const void *tan_disp1_device, const void *tan_disp2_device, const void *tan_sim_device,
                  double *tan_positions_device, int flags, void *hip_stream, lfr_jvp_stats *stats) {
    if (!b || !tan_positions_device) { lfr::set_error("lfr_batch_jvp: bad argument"); return LFR_ERR_ARG; }
    constexpr int kFlags = LFR_JVP_F64 | LFR_JVP_GAUSS_NEWTON | LFR_JVP_FALLBACK_GAUSS_NEWTON;
    if (flags & ~kFlags) { lfr::set_error("lfr_batch_jvp: unknown flag bits 0x%x", flags & ~kFlags); return LFR_ERR_ARG; }
    if ((flags & LFR_JVP_GAUSS_NEWTON) && (flags & LFR_JVP_FALLBACK_GAUSS_NEWTON)) {
        lfr::set_error("lfr_batch_jvp: LFR_JVP_GAUSS_NEWTON and LFR_JVP_FALLBACK_GAUSS_NEWTON exclude each other"); return LFR_ERR_ARG;
    }
    if (!tan_disp1_device && !tan_disp2_device && !tan_sim_device) { lfr::set_error("lfr_batch_jvp: no tangent (all three inputs are NULL)"); return LFR_ERR_ARG; }
    if (!tan_disp1_device != !tan_disp2_device) { lfr::set_error("lfr_batch_jvp: tan_disp1 and tan_disp2 go together (both or neither)"); return LFR_ERR_ARG; }
    if (b->cc_sharded) {
        lfr::set_error("lfr_batch_jvp: a batch over one rank's connected components numbers its matches by itself (lfr_problem_build_hip_shard)");
        return LFR_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const bool gn = (flags & LFR_JVP_GAUSS_NEWTON) != 0, fb = (flags & LFR_JVP_FALLBACK_GAUSS_NEWTON) != 0;
    { const int rc = lfr::pass_begin(b, &b->jvp, kJvp, 64, st); if (rc != LFR_OK) return rc; }
    JvpState &s = *static_cast<JvpState *>(b->jvp);
    if (b->fused) lfr::materialize_records(b, st);     // the packed records have not been written yet: write them (the next solve would write the same bytes)
    if (b->n_graph_nodes) HIP_TRY(hipMemsetAsync(tan_positions_device, 0, 2 * sizeof(double) * (size_t)b->n_graph_nodes, st));
    HIP_TRY(hipMemsetAsync(s.d_counters, 0, 64, st));
    JvpArgs ja;
    memset(&ja, 0, sizeof(ja));
    BwdArgs &a = ja.h;
    a.descs = b->d_descs; a.edges = b->d_edges; a.node_ids = b->d_node_ids; a.node_inc = b->d_node_inc; a.in_idx = b->d_in_idx;
    a.positions = b->d_positions; a.infos = b->d_infos;
    a.eid = lfr::edge_map(b);
    a.hws = s.d_hws; a.hws_off = s.d_hws_off;
    a.status = s.d_status; a.counters = s.d_counters; a.tukey_variant = b->tukey_variant;
    a.n_matches = (uint32_t)b->n_graph_matches;
    ja.t.disp1 = tan_disp1_device; ja.t.disp2 = tan_disp2_device; ja.t.sim = tan_sim_device;
    ja.t.n_matches = (uint32_t)b->n_graph_matches; ja.t.f64 = (flags & LFR_JVP_F64) ? 1 : 0;
    ja.xdot = tan_positions_device;
    // Packed classes (<= 32 rows).  Gauss-Newton mode: ONE launch of one-wave blocks, each wave hosting 64/S = 2-8 components (1 in
    // <32,2>), dealt to the classes as lfr_batch_covariance deals its own.  Exact mode (with or without the fallback): jvp_kernel, one wave per component.
    if (gn) {
        a.desc_begin = b->class_begin[0]; a.scan_all = 0;
        lfr::launch_packed_pass(b, jvp_gn_packed_kernel, ja, st);
    } else {
        a.desc_begin = b->class_begin[0];
        const int n = b->class_begin[lfr::KC_BLOCK] - a.desc_begin;
        a.scan_all = 1;
        if (n > 0 && fb)
            hipLaunchKernelGGL((jvp_kernel<kJvpThreadsSmall, true, false, true>), dim3(n), dim3(kJvpThreadsSmall), jvp_lds_bytes(32, true), st, ja);
        else if (n > 0)
            hipLaunchKernelGGL((jvp_kernel<kJvpThreadsSmall, true, false>), dim3(n), dim3(kJvpThreadsSmall), jvp_lds_bytes(32, true), st, ja);
    }
    // Workgroup classes, every mode: one workgroup of 256 threads per component; matrix in LDS up to 192 rows, in HBM above
    a.scan_all = 0;
    for (int cls = lfr::KC_BLOCK; cls < lfr::KC_COUNT; ++cls) {
        a.desc_begin = b->class_begin[cls];
        const int n = b->class_begin[cls + 1] - a.desc_begin, rows = std::max(s.rows_max[cls], 2);
        if (n <= 0) continue;
        const bool lds_matrix = cls != lfr::KC_GLOBAL;
        const size_t lds = jvp_lds_bytes(rows, lds_matrix);
        if (fb && lds_matrix) hipLaunchKernelGGL((jvp_kernel<kJvpThreads, true, false, true>), dim3(n), dim3(kJvpThreads), lds, st, ja);
        else if (fb) hipLaunchKernelGGL((jvp_kernel<kJvpThreads, false, false, true>), dim3(n), dim3(kJvpThreads), lds, st, ja);
        else if (!lds_matrix && gn) hipLaunchKernelGGL((jvp_kernel<kJvpThreads, false, true>), dim3(n), dim3(kJvpThreads), lds, st, ja);
        else if (!lds_matrix) hipLaunchKernelGGL((jvp_kernel<kJvpThreads, false, false>), dim3(n), dim3(kJvpThreads), lds, st, ja);
        else if (gn) hipLaunchKernelGGL((jvp_kernel<kJvpThreads, true, true>), dim3(n), dim3(kJvpThreads), lds, st, ja);
        else hipLaunchKernelGGL((jvp_kernel<kJvpThreads, true, false>), dim3(n), dim3(kJvpThreads), lds, st, ja);
    }
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

int64_t lfr_batch_jvp_status(lfr_batch *b, int32_t *status) { return lfr::pass_status(b, b ? b->jvp : nullptr, "jvp", status); }

}  // extern "C"
