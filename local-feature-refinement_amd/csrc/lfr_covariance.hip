// Per-keypoint covariance of the refined positions (lfr_batch_covariance, include/lfr.h).
// A translation unit of its own: it reads the batch layout (lfr_batch.hpp), the packed classes' J^T J sweep and in-register inversion
// (lfr_packed_normal_device.hpp, shared with the backward's Gauss-Newton mode; built on load_packed_edge, eval_edge and the DPP /
// swizzle broadcasts of lfr_device.hpp) and the backward's assembly and LDL^T (lfr_hessian_device.hpp), and changes nothing the solve
// or the backward read.
//
// Per solved component C = (J^T J)^-1 at the solve's x, J the loss-corrected Jacobian - the undamped, unscaled matrix of the LM loop:
//   packed classes (<= 32 rows)   ONE launch in the forward's layout: a wave64 hosts 64/S components, one-wave workgroups, no barriers.
//                                 One sweep with the forward's eval_edge and the matrix part of its LDS adds (five per edge), then an in-place Gauss-Jordan
//                                 INVERSION with one row per lane and all n columns of the row in registers; the pivot row travels as
//                                 the DPP operand of v_fmac_f64 (8- and 16-row classes) or through ds_swizzle (32-row classes).
//   workgroup classes (33..6144)  one workgroup per component: the backward's owner-computes assembly without rho'' and the second
//                                 derivatives, its zero-skipping LDL^T, then per node two forward substitutions with unit right-hand
//                                 sides and C(i,j) = sum_k W(k,i) W(k,j) / d_k, W = L^-1; nodes dealt to waves, fixed summation order.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "lfr_assemble.hpp"
#include "lfr_batch.hpp"
#include "lfr_hessian_device.hpp"
#include "lfr_packed_normal_device.hpp"

using namespace lfrdev;
using lfr::KernelArgs;
using lfr::PackedRanges;

namespace {

constexpr int kCovThreads = 256;              // workgroup classes
constexpr size_t kCovLdsMax = 160 * 1024 - 256;

// ---- packed classes (the sweep, the group's LDS and the inversion: lfr_packed_normal_device.hpp) ----
struct CovArgs {
    KernelArgs k;              // descs, edges, node_ids, positions, infos, the fused gather's arrays, tukey_variant
    void *cov;                 // 3 per node of the whole graph, float or double (cleared before the launch)
    int32_t *status;           // per descriptor
    int f64;
};

__device__ __forceinline__ void cov_store(const CovArgs &a, const uint32_t node, const double c00, const double c01, const double c11) {
    if (a.f64) { double *o = static_cast<double *>(a.cov) + 3 * (size_t)node; o[0] = c00; o[1] = c01; o[2] = c11; }
    else { float *o = static_cast<float *>(a.cov) + 3 * (size_t)node; o[0] = (float)c00; o[1] = (float)c01; o[2] = (float)c11; }
}

template <int KC, bool FUSED>
__device__ __forceinline__ void cov_group_body(const CovArgs &ca, const int desc_begin, const int desc_end, const int block_in_class,
                                               unsigned char *lds_raw) {
    constexpr int NV = PackedClass<KC>::NV, S = PackedClass<KC>::S, EPL = PackedClass<KC>::EPL, LD = NV + 1;
    const KernelArgs &a = ca.k;
    PackedGroup<KC> grp;
    if (!grp.init(a.descs, desc_begin, desc_end, block_in_class)) return;
    const int sl = grp.sl, ci = grp.ci;
    const int row = sl % NV, part = sl / NV;
    const bool have = grp.have;
    const CompDesc &d = grp.d;
    CovLds<NV> &L = reinterpret_cast<CovLds<NV> *>(lds_raw)[grp.gid];

    const bool usable = have && a.infos[ci].termination != LFR_TERM_FAILURE;
    const int n_var = usable ? grp.n_var : 0, nv2 = 2 * n_var, E = usable ? grp.E : 0;     // a group without a usable component inverts the identity
    const bool is_row = row < nv2;
    const int nv2_max = cov_wave_max(nv2);
    const uint32_t node = is_row ? a.node_ids[d.node_off + (row >> 1)] : 0u;

    cov_lds_init<NV, S>(a, d, n_var, sl, L);
    wave_lds_sync();
    cov_assemble<NV, S, EPL, FUSED>(a, d, n_var, E, sl, L);      // one sweep at x^
    wave_lds_sync();

    // ---- inversion, lane = row ----
    const double *A = L.A;
    cov_invert<KC>(row, nv2_max,
        [&](int c) -> double {
            double v = 0.0;
            if (is_row && c < nv2) v = (c <= row ? A[row * LD + c] : A[c * LD + row]);
            return (!is_row && c == row) ? 1.0 : v;                  // padded rows are identity
        },
        [&](auto &h, const bool ok) {
            constexpr int CL = sizeof(h) / sizeof(double);
            double dg = 0.0, off = 0.0;                              // C(row,row), C(row,row+1)
#pragma unroll
            for (int c = 0; c < CL; ++c) { dg = (c == row) ? h[c] : dg; off = (c == row + 1) ? h[c] : off; }
            const double dg_next = dpp_f64<kDppQuadXor1>(dg);       // the odd lane's diagonal, to the even lane of the node
            if (is_row && part == 0 && !(row & 1) && ok) cov_store(ca, node, dg, off, dg_next);
            if (have && sl == 0) ca.status[ci] = !usable ? 1 : ok ? 0 : 2;
        });
}

constexpr size_t kCovPackedLdsBytes = 4 * sizeof(CovLds<16>) > 2 * sizeof(CovLds<32>) ? 4 * sizeof(CovLds<16>) : 2 * sizeof(CovLds<32>);
static_assert(kCovPackedLdsBytes >= 8 * sizeof(CovLds<8>), "LDS budget");

// all packed classes in ONE launch, the blocks dealt to the classes as in solve_packed_kernel
template <bool FUSED>
__global__ __launch_bounds__(64, 2) void covariance_packed_kernel(const CovArgs a, const PackedRanges r) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kCovPackedLdsBytes];
    packed_dispatch(r, [&](auto kc, int desc_begin, int desc_end, int block_in_class) LFR_INLINE_LAMBDA {
        cov_group_body<decltype(kc)::value, FUSED>(a, desc_begin, desc_end, block_in_class, lds_raw);
    });
}

// lfr_debug_invert_spd: the inversion alone, systems placed as the groups of a wave
template <int KC>
__global__ __launch_bounds__(64) void debug_invert_kernel(int64_t n_sys, const int32_t *n_rows, const int64_t *tri_off, const double *A,
                                                          double *Cinv, int32_t *status) {
    constexpr int NV = PackedClass<KC>::NV, S = PackedClass<KC>::S, G = PackedClass<KC>::G;
    const int lane = threadIdx.x & 63;
    const int gid = lane / S, sl = lane % S;
    const int row = sl % NV, part = sl / NV;
    const int64_t sys = (int64_t)blockIdx.x * G + gid;
    const bool have = sys < n_sys;
    const int n = have ? n_rows[sys] : 0;
    const int64_t to = have ? tri_off[sys] : 0;
    const bool is_row = row < n;
    const int n_max = cov_wave_max(n);
    cov_invert<KC>(row, n_max,
        [&](int c) -> double {
            double v = 0.0;
            if (is_row && c < n) v = A[to + (int64_t)bwd_tri(max(row, c), min(row, c))];
            return (!is_row && c == row) ? 1.0 : v;
        },
        [&](auto &h, const bool ok) {
            constexpr int CL = sizeof(h) / sizeof(double);
#pragma unroll
            for (int c = 0; c < CL; ++c)
                if (is_row && part == 0 && c <= row) Cinv[to + (int64_t)bwd_tri(row, c)] = ok ? h[c] : 0.0;
            if (have && sl == 0) status[sys] = ok ? 0 : 2;
        });
}

// ---- workgroup classes ----
struct CovBlockArgs {
    BwdArgs b;                 // descs, edges, node_ids, node_inc, in_idx, positions, infos, hws, hws_off, status, desc_begin, tukey_variant
    void *cov;
    int f64;
    int scratch_doubles;       // dynamic LDS behind the matrix (LDS variant) or all of it (HBM variant)
};

template <int T, bool LDS_MATRIX>
__global__ __launch_bounds__(T) void covariance_block_kernel(const CovBlockArgs ca) {
    extern __shared__ double bsh[];
    const BwdArgs &a = ca.b;
    const int di = a.desc_begin + blockIdx.x, tid = threadIdx.x;
    const CompDesc d = a.descs[di];
    const int nv = d.n_var, n = 2 * nv;
    if (a.infos[di].termination == LFR_TERM_FAILURE) {       // not usable: zeros (the output was cleared)
        if (tid == 0) a.status[di] = 1;
        return;
    }
    double *H = LDS_MATRIX ? bsh : a.hws + a.hws_off[di];
    double *scratch = LDS_MATRIX ? bsh + bwd_tri(n, 0) : bsh;
    double *lval = scratch;                                   // the factorization's column buffer; afterwards the waves' vectors
    int *lidx = reinterpret_cast<int *>(lval + n);
    __shared__ int cnt[2];
    const EdgeRec *E = a.edges + d.edge_off;
    const uint32_t *ids = a.node_ids + d.node_off;

    const size_t nt = bwd_tri(n, 0);
    for (size_t t = tid; t < nt; t += T) H[t] = 0.0;
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();
    bwd_assemble<T, false>(a, d, nv, E, ids, H, nullptr, tid);
    __syncthreads();
    if (bwd_ldlt<T>(H, n, lval, lidx, cnt, tid)) {             // singular: zeros
        if (tid == 0) a.status[di] = 2;
        return;
    }
    __syncthreads();

    // diagonal blocks of C = L^-T D^-1 L^-1: node l's two columns of W = L^-1 by forward substitution (rows >= 2l only; a column of L is
    // visited only where W is not zero), the three sums accumulated as the entries of W become final - in row order, by one wave
    const int lane = tid & 63, wv = tid >> 6;
    const int ww = min(T / 64, ca.scratch_doubles / (2 * n));  // waves that have room for their two vectors (>= 1: the launch sizes the LDS)
    if (wv < ww) {
        double *w0 = scratch + (size_t)wv * 2 * n, *w1 = w0 + n;
        for (int l = wv; l < nv; l += ww) {
            const int i0 = 2 * l;
            for (int r = i0 + lane; r < n; r += 64) { w0[r] = (r == i0) ? 1.0 : 0.0; w1[r] = (r == i0 + 1) ? 1.0 : 0.0; }
            wave_lds_sync();
            double c00 = 0.0, c01 = 0.0, c11 = 0.0;
            for (int k = i0; k < n; ++k) {
                const double u = w0[k], v = w1[k];             // (wave-uniform)
                if (u == 0.0 && v == 0.0) continue;
                const double dinv = 1.0 / H[bwd_tri(k, k)];
                c00 += u * u * dinv; c01 += u * v * dinv; c11 += v * v * dinv;
                for (int r = k + 1 + lane; r < n; r += 64) {
                    const double lrk = H[bwd_tri(r, k)];
                    if (lrk != 0.0) { w0[r] -= lrk * u; w1[r] -= lrk * v; }
                }
                wave_lds_sync();
            }
            if (lane == 0) {
                if (ca.f64) { double *o = static_cast<double *>(ca.cov) + 3 * (size_t)ids[l]; o[0] = c00; o[1] = c01; o[2] = c11; }
                else { float *o = static_cast<float *>(ca.cov) + 3 * (size_t)ids[l]; o[0] = (float)c00; o[1] = (float)c01; o[2] = (float)c11; }
            }
            wave_lds_sync();
        }
    }
    if (tid == 0) a.status[di] = 0;
}

// =============================================================================================
// covariance between matched keypoints (lfr_batch_covariance_matches): the node blocks as above, and per match of the
// graph the cross block C_12 and D = C_11 + C_22 - C_12 - C_12^T.  Kernels of their own: the two above keep their code.
// Who writes match m: the record of its direction node1 -> node2 (even directed-edge id) - it exists whenever the match is in the
// program, and once.  The rows of the other matches keep what the host put there before the launches.
// =============================================================================================
struct MatchOut {
    const uint32_t *eid;       // per record: directed edge id of the graph (2m: node1 -> node2, 2m+1: node2 -> node1)
    void *cross, *rel;         // n_matches x 4 (cleared) / n_matches x 3 (set to -1, 0, -1), float or double; either may be nullptr
    uint32_t n_matches;
    int f64;
};

template <int N>
__device__ __forceinline__ void match_store(void *out, const int f64, const uint32_t m, const double (&v)[N]) {
    if (!out) return;
    if (f64) {
        double *o = static_cast<double *>(out) + N * (size_t)m;
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = v[i];
    } else {
        float *o = static_cast<float *>(out) + N * (size_t)m;
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = (float)v[i];
    }
}

// D of a match with two variable ends from the two node blocks a, b (C(di,di), C(di,dj), C(dj,dj)) and the cross block c (row-major):
// two sums of like terms and one difference per entry, all in fp64 (2 c is exact), so at most 4 ulp of the largest term
__device__ __forceinline__ void match_rel(const double (&a)[3], const double (&b)[3], const double (&c)[4], double (&d)[3]) {
    d[0] = (a[0] + b[0]) - 2.0 * c[0];
    d[1] = (a[1] + b[1]) - (c[1] + c[2]);
    d[2] = (a[2] + b[2]) - 2.0 * c[3];
}

struct CovMatchArgs {
    CovArgs c;                 // (cov may be nullptr here)
    MatchOut m;
};

// cov_group_body, and behind the inversion: every row lane puts its row of C into the group's LDS matrix (the assembled A is dead by
// then), then sub-lane sl re-reads the words of records sl + S k and the node1 -> node2 records write their match
template <int KC, bool FUSED>
__device__ __forceinline__ void cov_match_group_body(const CovMatchArgs &ma, const int desc_begin, const int desc_end, const int block_in_class,
                                                     unsigned char *lds_raw) {
    constexpr int NV = PackedClass<KC>::NV, S = PackedClass<KC>::S, EPL = PackedClass<KC>::EPL, LD = NV + 1;
    const CovArgs &ca = ma.c;
    const KernelArgs &a = ca.k;
    PackedGroup<KC> grp;
    if (!grp.init(a.descs, desc_begin, desc_end, block_in_class)) return;
    const int sl = grp.sl, ci = grp.ci;
    const int row = sl % NV, part = sl / NV;
    const bool have = grp.have;
    const CompDesc &d = grp.d;
    CovLds<NV> &L = reinterpret_cast<CovLds<NV> *>(lds_raw)[grp.gid];

    const bool usable = have && a.infos[ci].termination != LFR_TERM_FAILURE;
    const int n_var = usable ? grp.n_var : 0, nv2 = 2 * n_var, E = usable ? grp.E : 0;     // a group without a usable component inverts the identity
    const bool is_row = row < nv2;
    const int nv2_max = cov_wave_max(nv2);
    const uint32_t node = is_row ? a.node_ids[d.node_off + (row >> 1)] : 0u;

    cov_lds_init<NV, S>(a, d, n_var, sl, L);
    wave_lds_sync();
    cov_assemble<NV, S, EPL, FUSED>(a, d, n_var, E, sl, L);      // one sweep at x^
    wave_lds_sync();

    // ---- inversion, lane = row ----
    double *A = L.A;
    bool solved = false;
    cov_invert<KC>(row, nv2_max,
        [&](int c) -> double {
            double v = 0.0;
            if (is_row && c < nv2) v = (c <= row ? A[row * LD + c] : A[c * LD + row]);
            return (!is_row && c == row) ? 1.0 : v;                  // padded rows are identity
        },
        [&](auto &h, const bool ok) {
            constexpr int CL = sizeof(h) / sizeof(double);
            double dg = 0.0, off = 0.0;                              // C(row,row), C(row,row+1)
#pragma unroll
            for (int c = 0; c < CL; ++c) { dg = (c == row) ? h[c] : dg; off = (c == row + 1) ? h[c] : off; }
            const double dg_next = dpp_f64<kDppQuadXor1>(dg);       // the odd lane's diagonal, to the even lane of the node
            if (ca.cov && is_row && part == 0 && !(row & 1) && ok) cov_store(ca, node, dg, off, dg_next);
            if (have && sl == 0) ca.status[ci] = !usable ? 1 : ok ? 0 : 2;
            if (is_row && part == 0) {                               // row `row` of C over the dead A (CL <= NV < LD)
#pragma unroll
                for (int c = 0; c < CL; ++c) A[row * LD + c] = h[c];
            }
            solved = ok;
        });
    wave_lds_sync();

    // ---- the matches of the re-read records ----
    const int E_all = have ? (int)d.n_edges : 0;
    const bool good = usable && solved;                // otherwise: zeros, "no covariance", for every match of the component's program
#pragma unroll 1
    for (int p = sl; p < E_all; p += S) {
        const uint32_t rec = d.edge_off + (uint32_t)p, id = ma.m.eid[rec], m = id >> 1;
        if ((id & 1u) || m >= ma.m.n_matches) continue;
        double cr[4] = {0.0, 0.0, 0.0, 0.0}, rl[3] = {0.0, 0.0, 0.0};
        if (good) {
            const uint32_t word = FUSED ? a.edge_word[rec] : reinterpret_cast<const uint32_t *>(a.edges + rec)[19];
            const int s = (int)(word & 0xffffu), t = (int)((word >> 16) & 0x7fffu);
            const bool vs = s < n_var, vt = t < n_var;
            if (!vs && !vt) continue;                  // (cannot happen: an edge between two constants is no record)
            const int r1 = 2 * (vs ? s : t), r2 = 2 * t;
            const double b1[3] = {A[r1 * LD + r1], A[r1 * LD + r1 + 1], A[(r1 + 1) * LD + r1 + 1]};      // as cov_store takes them
            if (vs && vt) {
                const double b2[3] = {A[r2 * LD + r2], A[r2 * LD + r2 + 1], A[(r2 + 1) * LD + r2 + 1]};
                cr[0] = A[r1 * LD + r2]; cr[1] = A[r1 * LD + r2 + 1]; cr[2] = A[(r1 + 1) * LD + r2]; cr[3] = A[(r1 + 1) * LD + r2 + 1];
                match_rel(b1, b2, cr, rl);
            } else { rl[0] = b1[0]; rl[1] = b1[1]; rl[2] = b1[2]; }       // a constant end contributes zeros: the other end's block
        }
        match_store<4>(ma.m.cross, ma.m.f64, m, cr);
        match_store<3>(ma.m.rel, ma.m.f64, m, rl);
    }
}

template <bool FUSED>
__global__ __launch_bounds__(64, 2) void covariance_matches_packed_kernel(const CovMatchArgs a, const PackedRanges r) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kCovPackedLdsBytes];
    packed_dispatch(r, [&](auto kc, int desc_begin, int desc_end, int block_in_class) LFR_INLINE_LAMBDA {
        cov_match_group_body<decltype(kc)::value, FUSED>(a, desc_begin, desc_end, block_in_class, lds_raw);
    });
}

// ---- workgroup classes ----
struct CovMatchBlockArgs {
    CovBlockArgs c;            // (cov may be nullptr here; c.b.eid: the record -> directed-edge map)
    MatchOut m;
    double *diag;              // 3 per node entry of the batch (node_off + l): the node blocks in fp64, from the first pass to the second
};

// covariance_block_kernel's assembly, LDL^T and first pass (the node blocks, which also go to `diag`), then a second pass: per node l
// its two columns of W = L^-1 again, the back substitution c = L^-T D^-1 w - the node's two full columns of C in the wave's vectors -
// and a walk over the node's incident records: its out-edges l -> m with an even edge id are the matches node l owns (cross block
// C(2l+p, 2m+q) = c_p[2m+q]; a constant m: D = the node's block), and of its in-edges those from a constant node1, which has no column
// of its own.  Nodes dealt to waves, every sum in a fixed order.
template <int T, bool LDS_MATRIX>
__global__ __launch_bounds__(T) void covariance_matches_block_kernel(const CovMatchBlockArgs ma) {
    extern __shared__ double bsh[];
    const CovBlockArgs &ca = ma.c;
    const BwdArgs &a = ca.b;
    const int di = a.desc_begin + blockIdx.x, tid = threadIdx.x;
    const CompDesc d = a.descs[di];
    const int nv = d.n_var, n = 2 * nv;
    const EdgeRec *E = a.edges + d.edge_off;
    const uint32_t *ids = a.node_ids + d.node_off;
    const uint32_t *eid = a.eid + d.edge_off;
    auto no_covariance = [&](const int status) {             // zeros for every match of the component's program (the node output was cleared)
        const double z3[3] = {0.0, 0.0, 0.0};
        for (uint32_t p = tid; p < d.n_edges; p += T) {
            const uint32_t id = eid[p];
            if (!(id & 1u) && (id >> 1) < ma.m.n_matches) match_store<3>(ma.m.rel, ma.m.f64, id >> 1, z3);
        }
        if (tid == 0) a.status[di] = status;
    };
    if (a.infos[di].termination == LFR_TERM_FAILURE) { no_covariance(1); return; }      // not usable
    double *H = LDS_MATRIX ? bsh : a.hws + a.hws_off[di];
    double *scratch = LDS_MATRIX ? bsh + bwd_tri(n, 0) : bsh;
    double *lval = scratch;                                   // the factorization's column buffer; afterwards the waves' vectors
    int *lidx = reinterpret_cast<int *>(lval + n);
    __shared__ int cnt[2];

    const size_t nt = bwd_tri(n, 0);
    for (size_t t = tid; t < nt; t += T) H[t] = 0.0;
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();
    bwd_assemble<T, false>(a, d, nv, E, ids, H, nullptr, tid);
    __syncthreads();
    if (bwd_ldlt<T>(H, n, lval, lidx, cnt, tid)) { no_covariance(2); return; }         // singular
    __syncthreads();

    const int lane = tid & 63, wv = tid >> 6;
    const int ww = min(T / 64, ca.scratch_doubles / (2 * n));  // waves that have room for their two vectors (>= 1: the launch sizes the LDS)
    double *w0 = scratch + (size_t)min(wv, ww - 1) * 2 * n, *w1 = w0 + n;
    double *diag = ma.diag + 3 * (size_t)d.node_off;
    // first pass: the node blocks, as covariance_block_kernel sums them
    if (wv < ww) {
        for (int l = wv; l < nv; l += ww) {
            const int i0 = 2 * l;
            for (int r = i0 + lane; r < n; r += 64) { w0[r] = (r == i0) ? 1.0 : 0.0; w1[r] = (r == i0 + 1) ? 1.0 : 0.0; }
            wave_lds_sync();
            double c00 = 0.0, c01 = 0.0, c11 = 0.0;
            for (int k = i0; k < n; ++k) {
                const double u = w0[k], v = w1[k];             // (wave-uniform)
                if (u == 0.0 && v == 0.0) continue;
                const double dinv = 1.0 / H[bwd_tri(k, k)];
                c00 += u * u * dinv; c01 += u * v * dinv; c11 += v * v * dinv;
                for (int r = k + 1 + lane; r < n; r += 64) {
                    const double lrk = H[bwd_tri(r, k)];
                    if (lrk != 0.0) { w0[r] -= lrk * u; w1[r] -= lrk * v; }
                }
                wave_lds_sync();
            }
            if (lane == 0) {
                diag[3 * l] = c00; diag[3 * l + 1] = c01; diag[3 * l + 2] = c11;
                if (ca.cov && ca.f64) { double *o = static_cast<double *>(ca.cov) + 3 * (size_t)ids[l]; o[0] = c00; o[1] = c01; o[2] = c11; }
                else if (ca.cov) { float *o = static_cast<float *>(ca.cov) + 3 * (size_t)ids[l]; o[0] = (float)c00; o[1] = (float)c01; o[2] = (float)c11; }
            }
            wave_lds_sync();
        }
    }
    __syncthreads();                                          // every node block is in `diag`
    // second pass: full columns and the matches
    if (wv < ww) {
        for (int l = wv; l < nv; l += ww) {
            const int i0 = 2 * l;
            for (int r = lane; r < n; r += 64) { w0[r] = (r == i0) ? 1.0 : 0.0; w1[r] = (r == i0 + 1) ? 1.0 : 0.0; }
            wave_lds_sync();
            for (int k = i0; k < n; ++k) {                    // w = L^-1 e
                const double u = w0[k], v = w1[k];             // (wave-uniform)
                if (u == 0.0 && v == 0.0) continue;
                for (int r = k + 1 + lane; r < n; r += 64) {
                    const double lrk = H[bwd_tri(r, k)];
                    if (lrk != 0.0) { w0[r] -= lrk * u; w1[r] -= lrk * v; }
                }
                wave_lds_sync();
            }
            for (int r = i0 + lane; r < n; r += 64) { const double dr = H[bwd_tri(r, r)]; w0[r] /= dr; w1[r] /= dr; }
            wave_lds_sync();
            for (int i = n - 1; i > 0; --i) {                 // c = L^-T (D^-1 w): row i of L is contiguous
                const double u = w0[i], v = w1[i];             // (wave-uniform, final)
                if (u == 0.0 && v == 0.0) continue;
                const double *Li = H + bwd_tri(i, 0);
                for (int k = lane; k < i; k += 64) {
                    const double lik = Li[k];
                    if (lik != 0.0) { w0[k] -= lik * u; w1[k] -= lik * v; }
                }
                wave_lds_sync();
            }
            const lfr::NodeInc ni = a.node_inc[d.node_off + l];
            const double own[3] = {diag[3 * l], diag[3 * l + 1], diag[3 * l + 2]};
            for (uint32_t k = lane; k < ni.out_count; k += 64) {          // l -> m
                const uint32_t p = ni.out_begin + k;
                if (p >= d.n_edges) break;                    // (cannot happen: a run lies inside its component)
                const uint32_t id = eid[p], mt = id >> 1;
                if ((id & 1u) || mt >= ma.m.n_matches) continue;
                const int m = E[p].dst_kind & 0x7fff;
                double cr[4] = {0.0, 0.0, 0.0, 0.0}, rl[3] = {own[0], own[1], own[2]};
                if (m < nv) {
                    const double other[3] = {diag[3 * m], diag[3 * m + 1], diag[3 * m + 2]};
                    cr[0] = w0[2 * m]; cr[1] = w0[2 * m + 1]; cr[2] = w1[2 * m]; cr[3] = w1[2 * m + 1];
                    match_rel(own, other, cr, rl);
                }
                match_store<4>(ma.m.cross, ma.m.f64, mt, cr);
                match_store<3>(ma.m.rel, ma.m.f64, mt, rl);
            }
            for (uint32_t k = lane; k < ni.in_count; k += 64) {           // a constant node1 -> l
                if (ni.in_begin + k >= d.n_edges) break;
                const uint32_t p = a.in_idx[d.edge_off + ni.in_begin + k];
                if (p >= d.n_edges) break;
                const uint32_t id = eid[p], mt = id >> 1;
                if ((id & 1u) || mt >= ma.m.n_matches || (int)E[p].src < nv) continue;
                const double cr[4] = {0.0, 0.0, 0.0, 0.0};
                match_store<4>(ma.m.cross, ma.m.f64, mt, cr);
                match_store<3>(ma.m.rel, ma.m.f64, mt, own);
            }
            wave_lds_sync();
        }
    }
    if (tid == 0) a.status[di] = 0;
}

// the rows of `rel` that no record writes: (-1, 0, -1), "not in the program"
__global__ void k_cov_fill_rel(size_t n_matches, void *out, int f64) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * n_matches) return;
    const double v = (i % 3 == 1) ? 0.0 : -1.0;
    if (f64) static_cast<double *>(out)[i] = v; else static_cast<float *>(out)[i] = (float)v;
}

size_t cov_scratch_bytes(int rows) { return std::max<size_t>((size_t)rows * 12, (size_t)rows * 16 * (kCovThreads / 64)) + 16; }
// dynamic LDS of a launch whose largest component has `rows` rows; scratch_doubles: what lies behind the matrix
size_t cov_lds_bytes(int rows, bool lds_matrix, int &scratch_doubles) {
    const size_t mat = lds_matrix ? bwd_tri(rows, 0) * 8 : 0;
    const size_t scratch = std::min(cov_scratch_bytes(rows), kCovLdsMax - mat);
    scratch_doubles = (int)(scratch / 8);
    return mat + scratch;
}

int cov_setup_extra(lfr_batch *, lfr::PassState *) {
    int sd = 0;
    HIP_TRY(hipFuncSetAttribute((const void *)covariance_block_kernel<kCovThreads, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)cov_lds_bytes(lfr::kBlockMaxRows, true, sd)));
    HIP_TRY(hipFuncSetAttribute((const void *)covariance_block_kernel<kCovThreads, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)cov_lds_bytes(kBwdMaxRows, false, sd)));
    HIP_TRY(hipFuncSetAttribute((const void *)covariance_matches_block_kernel<kCovThreads, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)cov_lds_bytes(lfr::kBlockMaxRows, true, sd)));
    HIP_TRY(hipFuncSetAttribute((const void *)covariance_matches_block_kernel<kCovThreads, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)cov_lds_bytes(kBwdMaxRows, false, sd)));
    return LFR_OK;
}

// the shared state of a pass behind a solve (lfr_batch.hpp) + what lfr_batch_covariance_matches keeps, made on its first call: the
// fp64 node blocks of the workgroup classes between their two passes
struct CovState : lfr::PassState {
    lfr::DevArena match_slab;
    double *d_diag = nullptr;
};

const lfr::PassKind kCovariance = {"covariance", [] { return static_cast<lfr::PassState *>(new CovState()); }, cov_setup_extra};

}  // namespace

extern "C" {

int lfr_batch_covariance(lfr_batch *b, void *cov_device, int flags, void *hip_stream, lfr_covariance_stats *stats) {
    if (!b || !cov_device || (flags & ~LFR_COVARIANCE_F64)) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    hipStream_t st = (hipStream_t)hip_stream;
    const int f64 = (flags & LFR_COVARIANCE_F64) ? 1 : 0;
    { const int rc = lfr::pass_begin(b, &b->cov, kCovariance, 0, st); if (rc != LFR_OK) return rc; }
    lfr::PassState &s = *b->cov;
    if (b->n_graph_nodes) HIP_TRY(hipMemsetAsync(cov_device, 0, 3 * (size_t)b->n_graph_nodes * (f64 ? 8 : 4), st));
    {   // packed classes: one launch of one-wave blocks, dealt as lfr_batch_solve deals its own
        CovArgs a;
        memset(&a, 0, sizeof(a));
        a.k.descs = b->d_descs; a.k.edges = b->d_edges; a.k.node_ids = b->d_node_ids; a.k.positions = b->d_positions; a.k.infos = b->d_infos;
        a.k.tukey_variant = b->tukey_variant; a.k.edge_ref = b->d_edge_ref; a.k.edge_word = b->d_edge_word;
        a.cov = cov_device; a.status = s.d_status; a.f64 = f64;
        if (b->fused) {                      // the packed records have not been written yet: gather from the graph's arrays, as the solve did
            const lfr::DevGraph &dgr = *b->dev_hold->graph;
            a.k.f_row = dgr.flow_row; a.k.f_disp1 = dgr.disp1; a.k.f_disp2 = dgr.disp2; a.k.f_sim = dgr.sim;
            lfr::launch_packed_pass(b, covariance_packed_kernel<true>, a, st);
        } else {
            lfr::launch_packed_pass(b, covariance_packed_kernel<false>, a, st);
        }
    }
    CovBlockArgs c;
    memset(&c, 0, sizeof(c));
    c.b.descs = b->d_descs; c.b.edges = b->d_edges; c.b.node_ids = b->d_node_ids; c.b.node_inc = b->d_node_inc; c.b.in_idx = b->d_in_idx;
    c.b.positions = b->d_positions; c.b.infos = b->d_infos; c.b.hws = s.d_hws; c.b.hws_off = s.d_hws_off; c.b.status = s.d_status;
    c.b.tukey_variant = b->tukey_variant; c.b.scan_all = 0;
    c.cov = cov_device; c.f64 = f64;
    for (int cls = lfr::KC_BLOCK; cls < lfr::KC_COUNT; ++cls) {
        c.b.desc_begin = b->class_begin[cls];
        const int n = b->class_begin[cls + 1] - c.b.desc_begin, rows = std::max(s.rows_max[cls], 2);
        if (n <= 0) continue;
        if (cls == lfr::KC_GLOBAL) {
            const size_t lds = cov_lds_bytes(rows, false, c.scratch_doubles);
            hipLaunchKernelGGL((covariance_block_kernel<kCovThreads, false>), dim3(n), dim3(kCovThreads), lds, st, c);
        } else {
            const size_t lds = cov_lds_bytes(rows, true, c.scratch_doubles);
            hipLaunchKernelGGL((covariance_block_kernel<kCovThreads, true>), dim3(n), dim3(kCovThreads), lds, st, c);
        }
    }
    HIP_TRY(hipGetLastError());
    { const int rc = lfr::pass_end(&s, st); if (rc != LFR_OK) return rc; }
    if (stats) {
        int64_t count[3];
        memset(stats, 0, sizeof(*stats));
        { const int rc = lfr::pass_histogram(b, &s, st, count, &stats->kernel_ms); if (rc != LFR_OK) return rc; }
        stats->n_computed = count[0]; stats->n_not_usable = count[1]; stats->n_singular = count[2];
    }
    return LFR_OK;
}

int lfr_batch_covariance_matches(lfr_batch *b, void *cov_device, void *cross_device, void *rel_device, int flags, void *hip_stream,
                                 lfr_covariance_stats *stats) {
    if (!b) { lfr::set_error("lfr_batch_covariance_matches: no batch"); return LFR_ERR_ARG; }
    if (flags & ~LFR_COVARIANCE_F64) { lfr::set_error("lfr_batch_covariance_matches: unknown flag bits 0x%x", flags & ~LFR_COVARIANCE_F64); return LFR_ERR_ARG; }
    if (!cov_device && !cross_device && !rel_device) {
        lfr::set_error("lfr_batch_covariance_matches: nothing to compute (all three outputs are NULL)"); return LFR_ERR_ARG;
    }
    if (!cross_device && !rel_device) return lfr_batch_covariance(b, cov_device, flags, hip_stream, stats);      // the node output alone
    if (b->cc_sharded) {
        lfr::set_error("lfr_batch_covariance_matches: a batch over one rank's connected components numbers its matches by itself (lfr_problem_build_hip_shard): no per-match outputs");
        return LFR_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int f64 = (flags & LFR_COVARIANCE_F64) ? 1 : 0;
    const size_t M = (size_t)b->n_graph_matches, elt = f64 ? 8 : 4;
    HIP_TRY(hipSetDevice(b->device));
    if (b->n_solves > 0 && b->inputs_epoch == b->solved_epoch) {      // (otherwise pass_begin refuses the call)
        const int rc = lfr::ensure_edge_map(b);       // records -> edges of the graph: the batch's own, shared with backward, set_inputs and evaluate
        if (rc != LFR_OK) return rc;
    }
    { const int rc = lfr::pass_begin(b, &b->cov, kCovariance, 0, st); if (rc != LFR_OK) return rc; }
    CovState &s = *static_cast<CovState *>(b->cov);
    const bool any_block = b->class_begin[lfr::KC_COUNT] > b->class_begin[lfr::KC_BLOCK];
    if (any_block && !s.d_diag) {
        if (!s.match_slab.init(b->ctx, 24 * std::max<size_t>((size_t)b->n_nodes, 1) + 4096)) return LFR_ERR_NOMEM;
        s.d_diag = s.match_slab.take_n<double>(3 * (size_t)b->n_nodes);
        if (!s.d_diag) { s.match_slab.reset(); lfr::set_error("covariance: match slab exhausted"); return LFR_ERR_NOMEM; }
    }
    if (cov_device && b->n_graph_nodes) HIP_TRY(hipMemsetAsync(cov_device, 0, 3 * (size_t)b->n_graph_nodes * elt, st));
    if (cross_device && M) HIP_TRY(hipMemsetAsync(cross_device, 0, 4 * M * elt, st));
    if (rel_device && M) hipLaunchKernelGGL(k_cov_fill_rel, dim3((unsigned)((3 * M + 255) / 256)), dim3(256), 0, st, M, rel_device, f64);
    MatchOut mo;
    mo.eid = lfr::edge_map(b); mo.cross = cross_device; mo.rel = rel_device; mo.n_matches = (uint32_t)M; mo.f64 = f64;
    {   // packed classes: one launch of one-wave blocks, dealt as lfr_batch_covariance deals its own
        CovMatchArgs a;
        memset(&a, 0, sizeof(a));
        a.c.k.descs = b->d_descs; a.c.k.edges = b->d_edges; a.c.k.node_ids = b->d_node_ids; a.c.k.positions = b->d_positions; a.c.k.infos = b->d_infos;
        a.c.k.tukey_variant = b->tukey_variant; a.c.k.edge_ref = b->d_edge_ref; a.c.k.edge_word = b->d_edge_word;
        a.c.cov = cov_device; a.c.status = s.d_status; a.c.f64 = f64;
        a.m = mo;
        if (b->fused) {                      // the packed records have not been written yet: flows and words from the graph's arrays, as the solve did
            const lfr::DevGraph &dgr = *b->dev_hold->graph;
            a.c.k.f_row = dgr.flow_row; a.c.k.f_disp1 = dgr.disp1; a.c.k.f_disp2 = dgr.disp2; a.c.k.f_sim = dgr.sim;
            lfr::launch_packed_pass(b, covariance_matches_packed_kernel<true>, a, st);
        } else {
            lfr::launch_packed_pass(b, covariance_matches_packed_kernel<false>, a, st);
        }
    }
    CovMatchBlockArgs c;
    memset(&c, 0, sizeof(c));
    c.c.b.descs = b->d_descs; c.c.b.edges = b->d_edges; c.c.b.node_ids = b->d_node_ids; c.c.b.node_inc = b->d_node_inc; c.c.b.in_idx = b->d_in_idx;
    c.c.b.positions = b->d_positions; c.c.b.infos = b->d_infos; c.c.b.hws = s.d_hws; c.c.b.hws_off = s.d_hws_off; c.c.b.status = s.d_status;
    c.c.b.tukey_variant = b->tukey_variant; c.c.b.scan_all = 0; c.c.b.eid = mo.eid; c.c.b.n_matches = (uint32_t)M;
    c.c.cov = cov_device; c.c.f64 = f64;
    c.m = mo; c.diag = s.d_diag;
    for (int cls = lfr::KC_BLOCK; cls < lfr::KC_COUNT; ++cls) {
        c.c.b.desc_begin = b->class_begin[cls];
        const int n = b->class_begin[cls + 1] - c.c.b.desc_begin, rows = std::max(s.rows_max[cls], 2);
        if (n <= 0) continue;
        if (cls == lfr::KC_GLOBAL) {
            const size_t lds = cov_lds_bytes(rows, false, c.c.scratch_doubles);
            hipLaunchKernelGGL((covariance_matches_block_kernel<kCovThreads, false>), dim3(n), dim3(kCovThreads), lds, st, c);
        } else {
            const size_t lds = cov_lds_bytes(rows, true, c.c.scratch_doubles);
            hipLaunchKernelGGL((covariance_matches_block_kernel<kCovThreads, true>), dim3(n), dim3(kCovThreads), lds, st, c);
        }
    }
    HIP_TRY(hipGetLastError());
    { const int rc = lfr::pass_end(&s, st); if (rc != LFR_OK) return rc; }
    if (stats) {
        int64_t count[3];
        memset(stats, 0, sizeof(*stats));
        { const int rc = lfr::pass_histogram(b, &s, st, count, &stats->kernel_ms); if (rc != LFR_OK) return rc; }
        stats->n_computed = count[0]; stats->n_not_usable = count[1]; stats->n_singular = count[2];
    }
    return LFR_OK;
}

int64_t lfr_batch_covariance_status(lfr_batch *b, int32_t *status) { return lfr::pass_status(b, b ? b->cov : nullptr, "covariance", status); }

int lfr_debug_invert_spd(int device, int solver, int64_t n_sys, const int32_t *n_rows, const double *A, double *Cinv, int32_t *status) {
    static const int kClass[4] = {lfr::KC_G8, lfr::KC_G16, lfr::KC_G64_2, lfr::KC_G64_4};      // `solver`: the live packed classes in enum order
    if (solver < 0 || solver > 3 || n_sys < 0 || n_sys > (1 << 24) || (n_sys > 0 && (!n_rows || !A || !Cinv || !status))) {
        lfr::set_error("bad argument"); return LFR_ERR_ARG;
    }
    const lfr::PackedClassDef &pc = lfr::kPackedClass[kClass[solver]];
    std::vector<int64_t> off((size_t)n_sys);
    int64_t n_tri = 0;
    for (int64_t s = 0; s < n_sys; ++s) {
        const int n = n_rows[s];
        if (n < 0 || n > pc.max_rows || (n & 1)) { lfr::set_error("n_rows[%lld] = %d: not an even row count the solver takes", (long long)s, n); return LFR_ERR_ARG; }
        off[s] = n_tri;
        n_tri += (int64_t)n * (n + 1) / 2;
    }
    lfr::DevCtx *ctx = lfr::dev_ctx(device);
    if (!ctx) return LFR_ERR_HIP;
    if (n_sys == 0) return LFR_OK;
    HIP_TRY(hipSetDevice(device));
    lfr::DevArena ar;
    if (!ar.init(ctx, (size_t)n_sys * (4 + 8 + 4) + (size_t)n_tri * 16 + 16 * 256)) return LFR_ERR_NOMEM;
    int32_t *d_rows = ar.take_n<int32_t>(n_sys), *d_status = ar.take_n<int32_t>(n_sys);
    int64_t *d_off = ar.take_n<int64_t>(n_sys);
    double *d_A = ar.take_n<double>(std::max<int64_t>(n_tri, 1)), *d_C = ar.take_n<double>(std::max<int64_t>(n_tri, 1));
    if (!d_rows || !d_status || !d_off || !d_A || !d_C) { lfr::set_error("arena exhausted"); return LFR_ERR_NOMEM; }
    hipStream_t st = ctx->s_main;
    HIP_TRY(hipMemcpyAsync(d_rows, n_rows, 4 * (size_t)n_sys, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_off, off.data(), 8 * (size_t)n_sys, hipMemcpyHostToDevice, st));
    if (n_tri) HIP_TRY(hipMemcpyAsync(d_A, A, 8 * (size_t)n_tri, hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)((n_sys + pc.G() - 1) / pc.G()));
    switch (solver) {
        case 0: hipLaunchKernelGGL(debug_invert_kernel<lfr::KC_G8>, grid, dim3(64), 0, st, n_sys, d_rows, d_off, d_A, d_C, d_status); break;
        case 1: hipLaunchKernelGGL(debug_invert_kernel<lfr::KC_G16>, grid, dim3(64), 0, st, n_sys, d_rows, d_off, d_A, d_C, d_status); break;
        case 2: hipLaunchKernelGGL(debug_invert_kernel<lfr::KC_G64_2>, grid, dim3(64), 0, st, n_sys, d_rows, d_off, d_A, d_C, d_status); break;
        default: hipLaunchKernelGGL(debug_invert_kernel<lfr::KC_G64_4>, grid, dim3(64), 0, st, n_sys, d_rows, d_off, d_A, d_C, d_status); break;
    }
    HIP_TRY(hipGetLastError());
    if (n_tri) HIP_TRY(hipMemcpyAsync(Cinv, d_C, 8 * (size_t)n_tri, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(status, d_status, 4 * (size_t)n_sys, hipMemcpyDeviceToHost, st));
    HIP_TRY(lfr::stream_wait(st));
    return LFR_OK;
}

}  // extern "C"
