// Matrix-free linear solves with the second-order matrix of the objective (lfr_batch_hessian_solve, include/lfr.h):
// per component (H + damping I) y = b by block-Jacobi preconditioned conjugate gradients, the whole iteration inside the kernel, every
// component stopping on its own.  H is lfr_batch_hessian_product's matrix: the records go through the same hvp_edge / hvp_apply
// (lfr_hvp_device.hpp).  The blocks M, P, S of a record depend on the positions only, so they are formed ONCE per call.
//
//   packed classes (<= 32 rows)   ONE launch of one-wave workgroups, 64/S components per wave.  A lane forms the HvpEdge of its EPL
//                                 records once and keeps them in registers; lane i owns coordinate i (b, y, r, p of every right-hand
//                                 side in registers).  p and the accumulating A p live in the group's LDS as v and h do in the
//                                 product; the nodes' 2x2 diagonal blocks are summed there once and inverted by the owning lanes.
//                                 Dot products: the group's butterfly.  A finished group idles under a predicate until the wave's
//                                 last group is done: the loop's exit is wave-uniform.
//   workgroup classes (above)     one persistent workgroup of 256 per component, owner computes.  A sweep over the records writes
//                                 each record's ten block values into the pass's workspace (80 bytes per record); the thread of a
//                                 variable node then sums its two rows over the node's out- and in-edges in record order, reading
//                                 blocks instead of evaluating records.  r, p, A p of every right-hand side live in the pass's
//                                 workspace by global node id (no row limit), y in solutions_device.  Phases are separated by
//                                 __syncthreads(); the dot products are a wave butterfly, then the waves in order through LDS.
//                                 No spin-waits, nothing between workgroups.
// No fp64 value goes through a global-memory atomic; the arithmetic of one right-hand side does not depend on K or on the others.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "lfr_batch.hpp"
#include "lfr_device.hpp"
#include "lfr_hessian_device.hpp"
#include "lfr_hvp_device.hpp"
#include "lfr_packed_frame.hpp"

// every product and sum of the iteration is written out with its rounding (explicit fma where one is meant): the bits of a right-hand
// side's outputs do not depend on the instantiation (DESIGN.md §5.12 gives the reason)
#pragma clang fp contract(off)

using namespace lfrdev;
using lfr::CompDesc;
using lfr::EdgeRec;
using lfr::PackedRanges;

namespace {

constexpr int kHsThreads = 256;               // workgroup classes
constexpr int kHsMaxVectors = LFR_HVP_MAX_VECTORS;
constexpr int kHsActive = -1;                 // status of a right-hand side that still iterates

struct HsArgs {
    const CompDesc *descs;
    const EdgeRec *edges;
    const uint32_t *node_ids;
    const lfr::NodeInc *node_inc;
    const uint32_t *in_idx;
    const double *positions;   // 2 per node of the whole graph: the caller's or the batch's
    const double *rhs;         // K arrays of `stride` doubles
    double *solutions;         // K arrays of `stride` doubles (cleared before the launches)
    int32_t *status, *iterations;      // the caller's, K x n_desc, each may be nullptr
    double *residual;
    int32_t *own_status, *own_iterations;      // the pass's, K x n_desc: what the statistics read
    unsigned long long *n_bound;       // coordinates treated as bound (cleared before the launches)
    double *rec_blocks;        // workgroup classes: 10 doubles per record, record rec at 10 (rec - rec_first)
    double *vec;               // workgroup classes: per right-hand side r, p, A p, `stride` doubles each, by global node id
    double *node_inv;          // workgroup classes: the inverse of the node's diagonal block (i00, i01, i11), by global node id
    size_t stride;             // 2 * n_nodes of the whole graph
    double damping, rel_tolerance;
    uint32_t rec_first, rec_end;       // the records the workspace covers
    int n_desc, desc_begin, tukey_variant, free_set, max_iterations;
};

// the sum of a record's ten block values: finite exactly when all of them are
__device__ __forceinline__ bool hs_edge_finite(const HvpEdge &h) {
    return isfinite(h.m00 + h.m01 + h.m11 + h.p00 + h.p01 + h.p10 + h.p11 + h.s00 + h.s01 + h.s11);
}

// what a record adds to the diagonal block of its source node: P^T M P - S (symmetric)
__device__ __forceinline__ void hs_source_block(const HvpEdge &h, double &q00, double &q01, double &q11) {
    const double mp00 = fma(h.m01, h.p10, h.m00 * h.p00), mp01 = fma(h.m01, h.p11, h.m00 * h.p01);
    const double mp10 = fma(h.m11, h.p10, h.m01 * h.p00), mp11 = fma(h.m11, h.p11, h.m01 * h.p01);
    q00 = fma(h.p10, mp10, h.p00 * mp00) - h.s00;
    q01 = fma(h.p10, mp11, h.p00 * mp01) - h.s01;
    q11 = fma(h.p11, mp11, h.p01 * mp01) - h.s11;
}

// The preconditioner of one node: the inverse (i00, i01, i11) of its diagonal block of A = H + damping I, the block given without the
// damping.  A bound coordinate (b0 / b1) is the identity's in the block and takes no damping.  A block that is not finite, or has
// a00 <= 0 or det <= 0 (the exact mode can), is replaced by the identity.
__device__ __forceinline__ void hs_invert_block(double a00, double a01, double a11, const bool b0, const bool b1, const double damping,
                                                double &i00, double &i01, double &i11) {
    a00 = b0 ? 1.0 : a00 + damping;
    a11 = b1 ? 1.0 : a11 + damping;
    a01 = (b0 || b1) ? 0.0 : a01;
    const double det = fma(-a01, a01, a00 * a11);
    const bool ok = isfinite(a00) && isfinite(a01) && isfinite(a11) && isfinite(det) && a00 > 0.0 && det > 0.0;
    i00 = ok ? a11 / det : 1.0;
    i01 = ok ? -a01 / det : 0.0;
    i11 = ok ? a00 / det : 1.0;
}

// the stop of a step, the same expression in both layouts: |r|_2 <= rel_tolerance |b|_2
__device__ __forceinline__ bool hs_converged(const double rr, const double bb, const double tol) { return sqrt(rr) <= tol * sqrt(bb); }

// ---- packed classes ----
// per group: positions, the K search directions, the K products A p, the three entries of every node's diagonal block
template <int NV, int K>
struct alignas(16) HsLds {
    double x[NV];
    double p[K][NV];
    double h[K][NV];
    double blk[3][NV / 2];
};

template <int K>
constexpr size_t hs_packed_lds_bytes() { return PackedClass<lfr::KC_G8>::G * sizeof(HsLds<PackedClass<lfr::KC_G8>::NV, K>); }

template <int KC, bool EXACT, int K>
__device__ __forceinline__ void hs_group_body(const HsArgs &a, const int desc_begin, const int desc_end, const int block_in_class,
                                              unsigned char *lds_raw) {
    constexpr int NV = PackedClass<KC>::NV, S = PackedClass<KC>::S, EPL = PackedClass<KC>::EPL;
    static_assert(PackedClass<KC>::G * sizeof(HsLds<NV, K>) <= hs_packed_lds_bytes<K>(), "LDS budget");
    PackedGroup<KC> grp;
    if (!grp.init(a.descs, desc_begin, desc_end, block_in_class)) return;
    const int sl = grp.sl, ci = grp.ci, n_var = grp.n_var, nv2 = grp.nv2, E = grp.E;
    const bool have = grp.have;
    const CompDesc &d = grp.d;
    HsLds<NV, K> &L = reinterpret_cast<HsLds<NV, K> *>(lds_raw)[grp.gid];

    // lane sl owns coordinate sl of the component (NV <= S)
    const bool own = sl < nv2;
    const size_t gi = own ? 2 * (size_t)a.node_ids[d.node_off + (sl >> 1)] + (sl & 1) : 0;
    const double xi = own ? a.positions[gi] : 0.0;
    const bool bound = a.free_set && own && fabs(xi) >= 1.0;
    const bool freec = own && !bound;
    double bi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) bi[k] = own ? a.rhs[k * a.stride + gi] : 0.0;
    if (sl < NV) {
        L.x[sl] = xi;
#pragma unroll
        for (int k = 0; k < K; ++k) { L.p[k][sl] = 0.0; L.h[k][sl] = 0.0; }
    }
    if (sl < NV / 2) { L.blk[0][sl] = 0.0; L.blk[1][sl] = 0.0; L.blk[2][sl] = 0.0; }
    wave_lds_sync();

    // the lane's records, formed once: blocks in registers, (2 src | 2 dst << 8 | src variable << 16 | dst variable << 17 | present << 18)
    HvpEdge h[EPL];
    uint32_t ew[EPL];
    bool rec_bad = false;
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        const int p = sl + S * j;
        ew[j] = 0u;
        h[j].m00 = h[j].m01 = h[j].m11 = h[j].p00 = h[j].p01 = h[j].p10 = h[j].p11 = h[j].s00 = h[j].s01 = h[j].s11 = 0.0;
        if (!(p < E)) continue;
        float flow_k[18]; float sim_k; uint32_t pk;
        load_packed_edge<false>(a, d.edge_off + p, flow_k, sim_k, pk);
        const int es = (int)(pk & 0xffffu), ed = (int)((pk >> 16) & 0x7fffu), ekind = (int)(pk >> 31);
        const bool sv = es < n_var, dv = ed < n_var;                     // constants: position and vector 0, no row
        const int xa = sv ? 2 * es : 0, xb = dv ? 2 * ed : 0;
        hvp_edge<EXACT>(flow_k, sim_k, ekind, a.tukey_variant, sv ? L.x[xa] : 0.0, sv ? L.x[xa + 1] : 0.0, dv ? L.x[xb] : 0.0,
                        dv ? L.x[xb + 1] : 0.0, h[j]);
        ew[j] = (uint32_t)xa | ((uint32_t)xb << 8) | ((uint32_t)sv << 16) | ((uint32_t)dv << 17) | (1u << 18);
        rec_bad |= !hs_edge_finite(h[j]);
        if (dv) { atomicAdd(&L.blk[0][ed], h[j].m00); atomicAdd(&L.blk[1][ed], h[j].m01); atomicAdd(&L.blk[2][ed], h[j].m11); }
        if (sv) {
            double q00, q01, q11;
            hs_source_block(h[j], q00, q01, q11);
            atomicAdd(&L.blk[0][es], q00); atomicAdd(&L.blk[1][es], q01); atomicAdd(&L.blk[2][es], q11);
        }
    }
    wave_lds_sync();
    // (from here to the end every lane of the wave is active at every butterfly and exchange)
    const bool comp_bad = group_max<S>(rec_bad ? 1.0 : 0.0) != 0.0;
    const bool partner_bound = __shfl_xor((int)bound, 1, 64) != 0;
    double mine, off;                                   // z_i = mine r_i + off r_partner
    {
        const bool odd = (sl & 1) != 0;
        double i00, i01, i11;
        hs_invert_block(own ? L.blk[0][sl >> 1] : 1.0, own ? L.blk[1][sl >> 1] : 0.0, own ? L.blk[2][sl >> 1] : 1.0, odd ? partner_bound : bound,
                        odd ? bound : partner_bound, a.damping, i00, i01, i11);
        mine = odd ? i11 : i00; off = i01;
    }

    double y[K], r[K], p[K], rz[K], rr[K], bb[K];
    int st[K], it[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        y[k] = 0.0; it[k] = 0;
        r[k] = freec ? bi[k] : 0.0;
        bb[k] = group_sum<S>(hvp_mul(r[k], r[k]));
        rr[k] = bb[k];
        const double z = fma(off, __shfl_xor(r[k], 1, 64), mine * r[k]);
        rz[k] = group_sum<S>(hvp_mul(r[k], z));
        p[k] = z;
        st[k] = (comp_bad || !isfinite(bb[k])) ? LFR_HSOLVE_NONFINITE : (bb[k] == 0.0 ? LFR_HSOLVE_OK : kHsActive);
    }

    for (int iter = 0; iter < a.max_iterations; ++iter) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < K; ++k) any |= st[k] == kHsActive;
        if (!__any((int)any)) break;                    // wave-uniform: the last group of the wave is done
        if (sl < NV) {
#pragma unroll
            for (int k = 0; k < K; ++k) { L.p[k][sl] = p[k]; L.h[k][sl] = 0.0; }
        }
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            if (!(ew[j] >> 18)) continue;
            const int xa = (int)(ew[j] & 0xffu), xb = (int)((ew[j] >> 8) & 0xffu);
            const bool sv = (ew[j] >> 16) & 1u, dv = (ew[j] >> 17) & 1u;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                double hs0, hs1, hd0, hd1;
                hvp_apply<EXACT>(h[j], sv ? L.p[k][xa] : 0.0, sv ? L.p[k][xa + 1] : 0.0, dv ? L.p[k][xb] : 0.0, dv ? L.p[k][xb + 1] : 0.0, hs0, hs1,
                                 hd0, hd1);
                if (sv) { atomicAdd(&L.h[k][xa], hs0); atomicAdd(&L.h[k][xa + 1], hs1); }
                if (dv) { atomicAdd(&L.h[k][xb], hd0); atomicAdd(&L.h[k][xb + 1], hd1); }
            }
        }
        wave_lds_sync();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double ap = freec ? fma(a.damping, p[k], L.h[k][sl]) : 0.0;
            const double pap = group_sum<S>(hvp_mul(p[k], ap));
            const double alpha = rz[k] / pap;
            const double yn = fma(alpha, p[k], y[k]), rn = fma(-alpha, ap, r[k]);
            const double rrn = group_sum<S>(hvp_mul(rn, rn));
            const double zn = fma(off, __shfl_xor(rn, 1, 64), mine * rn);
            const double rzn = group_sum<S>(hvp_mul(rn, zn));
            // the verdicts are the group's: every lane of it holds the same sums.  A right-hand side that is done stays as it is
            if (st[k] == kHsActive) {
                if (!isfinite(pap)) st[k] = LFR_HSOLVE_NONFINITE;
                else if (pap <= 0.0) st[k] = LFR_HSOLVE_NEGATIVE_CURVATURE;
                else {
                    y[k] = yn; r[k] = rn; rr[k] = rrn; ++it[k];
                    if (!isfinite(rrn)) st[k] = LFR_HSOLVE_NONFINITE;
                    else if (hs_converged(rrn, bb[k], a.rel_tolerance)) st[k] = LFR_HSOLVE_OK;
                    else { p[k] = fma(rzn / rz[k], p[k], zn); rz[k] = rzn; }
                }
            }
        }
    }

#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = st[k] == kHsActive ? LFR_HSOLVE_MAX_ITERATIONS : st[k];
        if (own) a.solutions[k * a.stride + gi] = bound ? bi[k] : y[k];
        if (have && sl == 0) {
            const size_t o = (size_t)k * a.n_desc + ci;
            a.own_status[o] = s; a.own_iterations[o] = it[k];
            if (a.status) a.status[o] = s;
            if (a.iterations) a.iterations[o] = it[k];
            if (a.residual) a.residual[o] = bb[k] == 0.0 ? 0.0 : sqrt(rr[k]) / sqrt(bb[k]);
        }
    }
    if (bound) atomicAdd(a.n_bound, 1ull);             // (an integer count)
}

// all packed classes in ONE launch, the blocks dealt to the classes as in hessian_product_packed_kernel
template <bool EXACT, int K>
__global__ __launch_bounds__(64) void hessian_solve_packed_kernel(const HsArgs a, const PackedRanges r) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[hs_packed_lds_bytes<K>()];
    packed_dispatch(r, [&](auto kc, int desc_begin, int desc_end, int block_in_class) LFR_INLINE_LAMBDA {
        hs_group_body<decltype(kc)::value, EXACT, K>(a, desc_begin, desc_end, block_in_class, lds_raw);
    });
}

// ---- workgroup classes ----
// NVAL sums over the block in a fixed order: a butterfly inside each wave, then the waves in order.  Every thread gets every sum.
template <int T, int NVAL>
__device__ __forceinline__ void hs_block_sum(double (&v)[NVAL], double (*red)[T / 64], const int tid) {
#pragma unroll
    for (int i = 0; i < NVAL; ++i) {
        double c = v[i];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
        if ((tid & 63) == 0) red[i][tid >> 6] = c;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NVAL; ++i) {
        double c = red[i][0];
#pragma unroll
        for (int w = 1; w < T / 64; ++w) c += red[i][w];
        v[i] = c;
    }
    __syncthreads();                                    // (the slots are free for the next sums)
}

__device__ __forceinline__ void hs_load_blocks(const double *q, HvpEdge &h) {
    h.m00 = q[0]; h.m01 = q[1]; h.m11 = q[2]; h.p00 = q[3]; h.p01 = q[4]; h.p10 = q[5]; h.p11 = q[6]; h.s00 = q[7]; h.s01 = q[8]; h.s11 = q[9];
}

template <int T, bool EXACT, int K>
__global__ __launch_bounds__(T) void hessian_solve_block_kernel(const HsArgs a) {
    __shared__ double red[2 * K][T / 64];
    const int di = a.desc_begin + blockIdx.x, tid = threadIdx.x;
    const CompDesc d = a.descs[di];
    const int nv = d.n_var;
    const uint32_t ne = d.n_edges;
    // (cannot fire: the workspace covers the records of every workgroup class; it keeps a damaged descriptor inside it, and the
    // component reads as not finite so that no stale status is taken for its verdict)
    if (d.edge_off < a.rec_first || (uint64_t)d.edge_off + ne > (uint64_t)a.rec_end) {
        if (tid < K) {
            const size_t o = (size_t)tid * a.n_desc + di;
            a.own_status[o] = LFR_HSOLVE_NONFINITE; a.own_iterations[o] = 0;
            if (a.status) a.status[o] = LFR_HSOLVE_NONFINITE;
            if (a.iterations) a.iterations[o] = 0;
            if (a.residual) a.residual[o] = 0.0;
        }
        return;
    }
    const uint32_t *ids = a.node_ids + d.node_off;
    double *blk = a.rec_blocks + 10 * (size_t)(d.edge_off - a.rec_first);
    auto xof = [&](int m, int c) -> double { return m < nv ? a.positions[2 * (size_t)ids[m] + c] : 0.0; };
    auto word_of = [&](uint32_t p) -> uint32_t { return reinterpret_cast<const uint32_t *>(a.edges + d.edge_off + p)[19]; };
    auto vec = [&](int k, int which) -> double * { return a.vec + (size_t)(3 * k + which) * a.stride; };      // 0: r, 1: p, 2: A p
    // z = (the node's inverse block) r
    auto precond = [&](const double *inv, double r0, double r1, double &z0, double &z1) {
        z0 = fma(inv[1], r1, inv[0] * r0);
        z1 = fma(inv[1], r0, inv[2] * r1);
    };

    // the ten block values of every record, once per call
    bool bad = false;
    for (uint32_t p = tid; p < ne; p += T) {
        float fl[18]; float sm; uint32_t pk;
        load_packed_edge<false>(a, d.edge_off + p, fl, sm, pk);
        const int es = (int)(pk & 0xffffu), ed = (int)((pk >> 16) & 0x7fffu), kind = (int)(pk >> 31);
        HvpEdge h;
        hvp_edge<EXACT>(fl, sm, kind, a.tukey_variant, xof(es, 0), xof(es, 1), xof(ed, 0), xof(ed, 1), h);
        bad |= !hs_edge_finite(h);
        double *q = blk + 10 * (size_t)p;
        q[0] = h.m00; q[1] = h.m01; q[2] = h.m11; q[3] = h.p00; q[4] = h.p01; q[5] = h.p10; q[6] = h.p11; q[7] = h.s00; q[8] = h.s01; q[9] = h.s11;
    }
    const bool comp_bad = __syncthreads_or((int)bad) != 0;      // (a barrier: the blocks are the workgroup's)

    // the nodes' diagonal blocks and their inverses; r = b on the free set, y = 0, p = z
    double sums[2 * K];                                 // |b|^2, r . z
#pragma unroll
    for (int i = 0; i < 2 * K; ++i) sums[i] = 0.0;
    unsigned n_bound = 0;
    for (int l = tid; l < nv; l += T) {
        const lfr::NodeInc ni = a.node_inc[d.node_off + l];
        const size_t gl = 2 * (size_t)ids[l];
        const bool b0 = a.free_set && fabs(a.positions[gl]) >= 1.0, b1 = a.free_set && fabs(a.positions[gl + 1]) >= 1.0;
        n_bound += (unsigned)b0 + (unsigned)b1;
        double a00 = 0.0, a01 = 0.0, a11 = 0.0;
        for_out_records(ni, ne, [&](const uint32_t p) {
            HvpEdge h;
            hs_load_blocks(blk + 10 * (size_t)p, h);
            double q00, q01, q11;
            hs_source_block(h, q00, q01, q11);
            a00 += q00; a01 += q01; a11 += q11;
        });
        for_in_records(ni, a.in_idx, d.edge_off, ne, [&](const uint32_t p) {
            const double *q = blk + 10 * (size_t)p;
            a00 += q[0]; a01 += q[1]; a11 += q[2];
        });
        double inv[3];
        hs_invert_block(a00, a01, a11, b0, b1, a.damping, inv[0], inv[1], inv[2]);
        double *ginv = a.node_inv + 3 * (gl >> 1);
        ginv[0] = inv[0]; ginv[1] = inv[1]; ginv[2] = inv[2];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double raw0 = a.rhs[k * a.stride + gl], raw1 = a.rhs[k * a.stride + gl + 1];
            const double r0 = b0 ? 0.0 : raw0, r1 = b1 ? 0.0 : raw1;
            double z0, z1;
            precond(inv, r0, r1, z0, z1);
            vec(k, 0)[gl] = r0; vec(k, 0)[gl + 1] = r1;
            vec(k, 1)[gl] = z0; vec(k, 1)[gl + 1] = z1;
            a.solutions[k * a.stride + gl] = b0 ? raw0 : 0.0;
            a.solutions[k * a.stride + gl + 1] = b1 ? raw1 : 0.0;
            sums[k] += hvp_dot2(r0, r0, r1, r1);
            sums[K + k] += hvp_dot2(r0, z0, r1, z1);
        }
    }
    if (n_bound) atomicAdd(a.n_bound, (unsigned long long)n_bound);      // (an integer count)
    hs_block_sum<T, 2 * K>(sums, red, tid);             // (its barriers also publish p to the block)

    // from here every thread holds the same scalars and takes the same branches
    double bb[K], rr[K], rz[K];
    int st[K], it[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        bb[k] = rr[k] = sums[k]; rz[k] = sums[K + k]; it[k] = 0;
        st[k] = (comp_bad || !isfinite(bb[k])) ? LFR_HSOLVE_NONFINITE : (bb[k] == 0.0 ? LFR_HSOLVE_OK : kHsActive);
    }

    for (int iter = 0; iter < a.max_iterations; ++iter) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < K; ++k) any |= st[k] == kHsActive;
        if (!any) break;
        // A p, owner computes, and p . A p
        double pap[K];
#pragma unroll
        for (int k = 0; k < K; ++k) pap[k] = 0.0;
        for (int l = tid; l < nv; l += T) {
            const lfr::NodeInc ni = a.node_inc[d.node_off + l];
            const size_t gl = 2 * (size_t)ids[l];
            const bool b0 = a.free_set && fabs(a.positions[gl]) >= 1.0, b1 = a.free_set && fabs(a.positions[gl + 1]) >= 1.0;
            double pl[K][2], acc[K][2];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                pl[k][0] = vec(k, 1)[gl]; pl[k][1] = vec(k, 1)[gl + 1];
                acc[k][0] = 0.0; acc[k][1] = 0.0;
            }
            for_out_records(ni, ne, [&](const uint32_t p) {       // l -> m: the source side
                HvpEdge h;
                hs_load_blocks(blk + 10 * (size_t)p, h);
                const int m = (int)((word_of(p) >> 16) & 0x7fffu);
                const size_t gm = m < nv ? 2 * (size_t)ids[m] : 0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (st[k] != kHsActive) continue;
                    double hs0, hs1, hd0, hd1;
                    hvp_apply<EXACT>(h, pl[k][0], pl[k][1], m < nv ? vec(k, 1)[gm] : 0.0, m < nv ? vec(k, 1)[gm + 1] : 0.0, hs0, hs1, hd0, hd1);
                    acc[k][0] += hs0; acc[k][1] += hs1;
                }
            });
            for_in_records(ni, a.in_idx, d.edge_off, ne, [&](const uint32_t p) {      // m -> l: the destination side
                HvpEdge h;
                hs_load_blocks(blk + 10 * (size_t)p, h);
                const int m = (int)(word_of(p) & 0xffffu);
                const size_t gm = m < nv ? 2 * (size_t)ids[m] : 0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (st[k] != kHsActive) continue;
                    double hs0, hs1, hd0, hd1;
                    hvp_apply<EXACT>(h, m < nv ? vec(k, 1)[gm] : 0.0, m < nv ? vec(k, 1)[gm + 1] : 0.0, pl[k][0], pl[k][1], hs0, hs1, hd0, hd1);
                    acc[k][0] += hd0; acc[k][1] += hd1;
                }
            });
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (st[k] != kHsActive) continue;
                const double ap0 = b0 ? 0.0 : fma(a.damping, pl[k][0], acc[k][0]), ap1 = b1 ? 0.0 : fma(a.damping, pl[k][1], acc[k][1]);
                vec(k, 2)[gl] = ap0; vec(k, 2)[gl + 1] = ap1;
                pap[k] += hvp_dot2(pl[k][0], ap0, pl[k][1], ap1);
            }
        }
        hs_block_sum<T, K>(pap, red, tid);
        bool step[K];
        double alpha[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            step[k] = false; alpha[k] = 0.0;
            if (st[k] != kHsActive) continue;
            if (!isfinite(pap[k])) st[k] = LFR_HSOLVE_NONFINITE;
            else if (pap[k] <= 0.0) st[k] = LFR_HSOLVE_NEGATIVE_CURVATURE;
            else { step[k] = true; alpha[k] = rz[k] / pap[k]; }
        }
        // y += alpha p, r -= alpha A p, |r|^2 and r . z
#pragma unroll
        for (int i = 0; i < 2 * K; ++i) sums[i] = 0.0;
        for (int l = tid; l < nv; l += T) {
            const size_t gl = 2 * (size_t)ids[l];
            const double *ginv = a.node_inv + 3 * (gl >> 1);
            const double inv[3] = {ginv[0], ginv[1], ginv[2]};
            const bool b0 = a.free_set && fabs(a.positions[gl]) >= 1.0, b1 = a.free_set && fabs(a.positions[gl + 1]) >= 1.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (!step[k]) continue;
                const double p0 = vec(k, 1)[gl], p1 = vec(k, 1)[gl + 1];
                double *yk = a.solutions + k * a.stride + gl;
                if (!b0) yk[0] = fma(alpha[k], p0, yk[0]);            // (a bound coordinate keeps b's bits)
                if (!b1) yk[1] = fma(alpha[k], p1, yk[1]);
                const double r0 = fma(-alpha[k], vec(k, 2)[gl], vec(k, 0)[gl]), r1 = fma(-alpha[k], vec(k, 2)[gl + 1], vec(k, 0)[gl + 1]);
                vec(k, 0)[gl] = r0; vec(k, 0)[gl + 1] = r1;
                double z0, z1;
                precond(inv, r0, r1, z0, z1);
                sums[k] += hvp_dot2(r0, r0, r1, r1);
                sums[K + k] += hvp_dot2(r0, z0, r1, z1);
            }
        }
        hs_block_sum<T, 2 * K>(sums, red, tid);
        bool turn[K];
        double beta[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            turn[k] = false; beta[k] = 0.0;
            if (!step[k]) continue;
            rr[k] = sums[k]; ++it[k];
            if (!isfinite(rr[k])) st[k] = LFR_HSOLVE_NONFINITE;
            else if (hs_converged(rr[k], bb[k], a.rel_tolerance)) st[k] = LFR_HSOLVE_OK;
            else { turn[k] = true; beta[k] = sums[K + k] / rz[k]; rz[k] = sums[K + k]; }
        }
        // p = z + beta p
        for (int l = tid; l < nv; l += T) {
            const size_t gl = 2 * (size_t)ids[l];
            const double *ginv = a.node_inv + 3 * (gl >> 1);
            const double inv[3] = {ginv[0], ginv[1], ginv[2]};
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (!turn[k]) continue;
                double z0, z1;
                precond(inv, vec(k, 0)[gl], vec(k, 0)[gl + 1], z0, z1);
                vec(k, 1)[gl] = fma(beta[k], vec(k, 1)[gl], z0);
                vec(k, 1)[gl + 1] = fma(beta[k], vec(k, 1)[gl + 1], z1);
            }
        }
        __syncthreads();                                // the new p is the block's
    }

    if (tid < K) {
        int s = LFR_HSOLVE_MAX_ITERATIONS, n = 0;
        double res = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (k == tid) {
                s = st[k] == kHsActive ? LFR_HSOLVE_MAX_ITERATIONS : st[k]; n = it[k];
                res = bb[k] == 0.0 ? 0.0 : sqrt(rr[k]) / sqrt(bb[k]);
            }
        const size_t o = (size_t)tid * a.n_desc + di;
        a.own_status[o] = s; a.own_iterations[o] = n;
        if (a.status) a.status[o] = s;
        if (a.iterations) a.iterations[o] = n;
        if (a.residual) a.residual[o] = res;
    }
}

template <bool EXACT, int K>
void hs_launch(const lfr_batch *b, const HsArgs &a, hipStream_t st) {
    lfr::launch_two_layouts(b, hessian_solve_packed_kernel<EXACT, K>, hessian_solve_block_kernel<kHsThreads, EXACT, K>, kHsThreads, a, st);
}

template <bool EXACT>
void hs_launch_k(const lfr_batch *b, const HsArgs &a, int n_rhs, hipStream_t st) {
    static_assert(kHsMaxVectors == 4, "one instantiation per count of right-hand sides");
    switch (n_rhs) {
        case 1: hs_launch<EXACT, 1>(b, a, st); break;
        case 2: hs_launch<EXACT, 2>(b, a, st); break;
        case 3: hs_launch<EXACT, 3>(b, a, st); break;
        default: hs_launch<EXACT, 4>(b, a, st); break;
    }
}

// the shared state of a pass (events, latest stream: lfr_batch.hpp) + the pass's own status and iteration counts, the bound-coordinate
// count and the workspace of the workgroup classes, sized at set-up.  Set up by pass_setup_unsolved: the solve needs no LM solve.
struct HsState : lfr::PassState {
    unsigned long long *d_bound = nullptr;
    int32_t *d_own_status = nullptr, *d_own_iterations = nullptr;
    double *d_rec_blocks = nullptr, *d_vec = nullptr, *d_node_inv = nullptr;
    uint32_t rec_first = 0, rec_end = 0;
    std::vector<int32_t> h_status, h_iterations;
};

// records and nodes the workspace of the workgroup classes has to cover (0, 0 without such components)
void hs_workspace_extent(const lfr_batch *b, size_t *n_records, size_t *n_nodes) {
    const bool any = b->class_begin[lfr::KC_COUNT] > b->class_begin[lfr::KC_BLOCK];
    *n_records = any ? (size_t)b->n_edges - std::min<size_t>((size_t)b->packed_edges, (size_t)b->n_edges) : 0;
    *n_nodes = any ? (size_t)b->n_graph_nodes : 0;
}

size_t hs_slab_bytes(const lfr_batch *b) {
    size_t nrec, nn;
    hs_workspace_extent(b, &nrec, &nn);
    const size_t nd = std::max<size_t>((size_t)b->n_desc, 1);
    return 8 + 2 * 4 * kHsMaxVectors * nd + 80 * nrec + 8 * (3 * kHsMaxVectors * 2 * nn + 3 * nn) + 8 * 256 + 4096;
}

int hs_carve(lfr_batch *b, lfr::PassState *ps) {
    HsState *s = static_cast<HsState *>(ps);
    size_t nrec, nn;
    hs_workspace_extent(b, &nrec, &nn);
    const size_t nd = std::max<size_t>((size_t)b->n_desc, 1);
    s->d_bound = s->slab.take_n<unsigned long long>(1);
    s->d_own_status = s->slab.take_n<int32_t>(kHsMaxVectors * nd);
    s->d_own_iterations = s->slab.take_n<int32_t>(kHsMaxVectors * nd);
    s->d_rec_blocks = s->slab.take_n<double>(10 * nrec);
    s->d_vec = s->slab.take_n<double>(3 * kHsMaxVectors * 2 * nn);
    s->d_node_inv = s->slab.take_n<double>(3 * nn);
    if (!s->d_bound || !s->d_own_status || !s->d_own_iterations || !s->d_rec_blocks || !s->d_vec || !s->d_node_inv) {
        lfr::set_error("hessian_solve slab exhausted"); return LFR_ERR_NOMEM;
    }
    s->rec_end = (uint32_t)b->n_edges;
    s->rec_first = s->rec_end - (uint32_t)nrec;
    return LFR_OK;
}
const lfr::PassKind kHessianSolve = {"hessian_solve", [] { return static_cast<lfr::PassState *>(new HsState()); }, hs_carve};

}  // namespace

extern "C" {

int lfr_batch_hessian_solve(lfr_batch *b, const double *positions_device, const double *rhs_device, int n_rhs, double damping,
                            double rel_tolerance, int max_iterations, double *solutions_device, int32_t *status_device,
                            int32_t *iterations_device, double *residual_device, int flags, void *hip_stream,
                            lfr_hessian_solve_stats *stats) {
    // every argument error comes before an output is touched
    if (!b) { lfr::set_error("lfr_batch_hessian_solve: no batch"); return LFR_ERR_ARG; }
    constexpr int known = LFR_HSOLVE_GAUSS_NEWTON | LFR_HSOLVE_FREE_SET;
    if (flags & ~known) { lfr::set_error("lfr_batch_hessian_solve: unknown flag bits 0x%x", flags & ~known); return LFR_ERR_ARG; }
    if (!rhs_device) { lfr::set_error("lfr_batch_hessian_solve: no right-hand sides"); return LFR_ERR_ARG; }
    if (!solutions_device) { lfr::set_error("lfr_batch_hessian_solve: no solutions array"); return LFR_ERR_ARG; }
    if (n_rhs < 1 || n_rhs > LFR_HVP_MAX_VECTORS) {
        lfr::set_error("lfr_batch_hessian_solve: %d right-hand sides, need 1 to %d", n_rhs, LFR_HVP_MAX_VECTORS); return LFR_ERR_ARG;
    }
    if (!(damping >= 0.0) || !std::isfinite(damping)) { lfr::set_error("lfr_batch_hessian_solve: damping %g, need a finite value >= 0", damping); return LFR_ERR_ARG; }
    if (!(rel_tolerance >= 0.0)) { lfr::set_error("lfr_batch_hessian_solve: rel_tolerance %g, need a value >= 0", rel_tolerance); return LFR_ERR_ARG; }
    if (max_iterations < 1) { lfr::set_error("lfr_batch_hessian_solve: max_iterations %d, need at least 1", max_iterations); return LFR_ERR_ARG; }
    if (!positions_device && b->n_solves == 0) {
        lfr::set_error("lfr_batch_hessian_solve: the batch has not been solved and no positions are given"); return LFR_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(b->device));
    if (!b->hsolve) {
        const int rc = lfr::pass_setup_unsolved(b, &b->hsolve, kHessianSolve, hs_slab_bytes(b));
        if (rc != LFR_OK) return rc;
    }
    HsState &s = *static_cast<HsState *>(b->hsolve);
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t N = (size_t)b->n_graph_nodes, nd = (size_t)b->n_desc;
    // every call iterates in the pass's one workspace: a call on another stream waits for the latest one
    if (s.n_calls > 0 && s.last_stream != st) HIP_TRY(hipStreamWaitEvent(st, s.ev1, 0));
    { const int rc = lfr::eval_prologue(b, s, st); if (rc != LFR_OK) return rc; }
    // nodes that are not variable in this shard read 0
    if (N) HIP_TRY(hipMemsetAsync(solutions_device, 0, (size_t)n_rhs * 2 * N * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(s.d_bound, 0, 8, st));

    HsArgs a;
    memset(&a, 0, sizeof(a));
    a.descs = b->d_descs; a.edges = b->d_edges; a.node_ids = b->d_node_ids; a.node_inc = b->d_node_inc; a.in_idx = b->d_in_idx;
    a.positions = positions_device ? positions_device : b->d_positions;
    a.rhs = rhs_device; a.solutions = solutions_device;
    a.status = status_device; a.iterations = iterations_device; a.residual = residual_device;
    a.own_status = s.d_own_status; a.own_iterations = s.d_own_iterations; a.n_bound = s.d_bound;
    a.rec_blocks = s.d_rec_blocks; a.vec = s.d_vec; a.node_inv = s.d_node_inv;
    a.rec_first = s.rec_first; a.rec_end = s.rec_end;
    a.stride = 2 * N; a.damping = damping; a.rel_tolerance = rel_tolerance; a.max_iterations = max_iterations;
    a.n_desc = b->n_desc; a.tukey_variant = b->tukey_variant; a.free_set = (flags & LFR_HSOLVE_FREE_SET) ? 1 : 0;
    if (flags & LFR_HSOLVE_GAUSS_NEWTON) hs_launch_k<false>(b, a, n_rhs, st);
    else hs_launch_k<true>(b, a, n_rhs, st);
    HIP_TRY(hipGetLastError());
    { const int rc = lfr::pass_end(&s, st); if (rc != LFR_OK) return rc; }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        const size_t n = (size_t)n_rhs * nd;
        s.h_status.assign(n, 0); s.h_iterations.assign(n, 0);
        unsigned long long n_bound = 0;
        // (the kernels write right-hand side k at k * n_desc: the first n_rhs * n_desc entries are this call's)
        if (n) {
            HIP_TRY(hipMemcpyAsync(s.h_status.data(), s.d_own_status, 4 * n, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(s.h_iterations.data(), s.d_own_iterations, 4 * n, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipMemcpyAsync(&n_bound, s.d_bound, 8, hipMemcpyDeviceToHost, st));
        { const int rc = lfr::pass_wait_ms(&s, st, &stats->kernel_ms); if (rc != LFR_OK) return rc; }
        for (size_t i = 0; i < n; ++i) {
            switch (s.h_status[i]) {
                case LFR_HSOLVE_OK: ++stats->n_converged; break;
                case LFR_HSOLVE_MAX_ITERATIONS: ++stats->n_max_iterations; break;
                case LFR_HSOLVE_NEGATIVE_CURVATURE: ++stats->n_negative_curvature; break;
                default: ++stats->n_nonfinite; break;
            }
            stats->sum_iterations += s.h_iterations[i];
            stats->max_iterations_used = std::max<int64_t>(stats->max_iterations_used, s.h_iterations[i]);
        }
        stats->n_components = b->n_desc;
        stats->n_bound_coordinates = (int64_t)n_bound;
    }
    return LFR_OK;
}

}  // extern "C"
