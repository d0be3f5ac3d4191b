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
//
// lfr_batch_evaluate_vjp is the same sweep run backwards: the bars of the cost, the residuals and the weights in, the
// gradients with respect to the positions, the flows and the similarities out.  Two launches in the same two layouts; per record one
// 2-vector q carries everything (vjp_q), every match row is stored by exactly one record, the similarity terms of the two directions
// go through a per-direction scratch and one combine pass (k_vjp_sim).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "lfr_batch.hpp"
#include "lfr_device.hpp"
#include "lfr_packed_frame.hpp"

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
constexpr size_t kEvalPackedLdsBytes = PackedClass<lfr::KC_G8>::G * sizeof(EvalLds<PackedClass<lfr::KC_G8>::NV>);

template <int KC>
__device__ __forceinline__ void eval_group_body(const EvalArgs &a, const int desc_begin, const int desc_end, const int block_in_class,
                                                unsigned char *lds_raw) {
    constexpr int NV = PackedClass<KC>::NV, S = PackedClass<KC>::S, EPL = PackedClass<KC>::EPL;
    PackedGroup<KC> grp;
    if (!grp.init(a.descs, desc_begin, desc_end, block_in_class)) return;
    const int sl = grp.sl, ci = grp.ci, n_var = grp.n_var, nv2 = grp.nv2, E = grp.E;
    const bool have = grp.have;
    const CompDesc &d = grp.d;
    static_assert(PackedClass<KC>::G * sizeof(EvalLds<NV>) <= kEvalPackedLdsBytes, "LDS budget");
    EvalLds<NV> &L = reinterpret_cast<EvalLds<NV> *>(lds_raw)[grp.gid];

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

// all packed classes in ONE launch, the blocks dealt to the classes as in solve_packed_kernel
__global__ __launch_bounds__(64) void evaluate_packed_kernel(const EvalArgs a, const PackedRanges r) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kEvalPackedLdsBytes];
    packed_dispatch(r, [&](auto kc, int desc_begin, int desc_end, int block_in_class) LFR_INLINE_LAMBDA {
        eval_group_body<decltype(kc)::value>(a, desc_begin, desc_end, block_in_class, lds_raw);
    });
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
        for_out_records(ni, ne, [&](const uint32_t p) {       // l -> m
            float fl[18]; float sm; uint32_t pk;
            load_packed_edge<false>(a, d.edge_off + p, fl, sm, pk);
            const int m = (int)((pk >> 16) & 0x7fffu), kind = (int)(pk >> 31);
            EvalEdge o;
            eval_block(fl, sm, kind, a.tukey_variant, xr, xc, xof(m, 0), xof(m, 1), o);
            cost += o.term;
            g0 += o.gs0; g1 += o.gs1;
            if (a.eid) eval_store_match(a, a.eid[d.edge_off + p], o);
        });
        if (!a.grad || l >= nv) continue;
        for_in_records(ni, a.in_idx, d.edge_off, ne, [&](const uint32_t p) {      // m -> l
            float fl[18]; float sm; uint32_t pk;
            load_packed_edge<false>(a, d.edge_off + p, fl, sm, pk);
            const int m = (int)(pk & 0xffffu), kind = (int)(pk >> 31);
            EvalEdge o;
            eval_block(fl, sm, kind, a.tukey_variant, xof(m, 0), xof(m, 1), xr, xc, o);
            g0 += o.gd0; g1 += o.gd1;
        });
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

// =============================================================================================
// lfr_batch_evaluate_vjp: the vector-Jacobian product of the sweep above
// =============================================================================================
struct VjpArgs {
    const CompDesc *descs;
    const EdgeRec *edges;
    const uint32_t *node_ids;
    const lfr::NodeInc *node_inc;
    const uint32_t *in_idx;
    const double *positions;
    const uint32_t *eid;       // per record: directed edge id of the graph (nullptr: no per-match argument)
    const double *cbar;        // per descriptor, or nullptr (= 0)
    const void *rbar, *wbar;   // n_matches x 4 / n_matches x 2, float or double, or nullptr (= 0)
    double *grad;              // 2 per node of the whole graph (cleared before the launches), or nullptr
    void *g_disp1, *g_disp2;   // n_matches x 18, float or double (cleared before the launches), or both nullptr
    double *g_sim_dir;         // per directed edge (cleared before the launches), or nullptr
    uint32_t *bad;             // per descriptor: a q of the component is not finite (cleared before the launches)
    uint32_t n_dir;            // 2 * n_matches
    int desc_begin, tukey_variant, f64;
    int wide;                  // the flow rows are aligned for 16-byte (double) / 8-byte (float) stores
};

// eval_block's quantities that the reverse sweep needs: r, rho, rho' and P are formed exactly as there; rho'' is the backward's
// (bwd_eval): Cauchy -1 / (b (1 + s/b)^2), Tukey -6 k / a^4 (1 - s/a^2) inside and 0 where saturated.  lr, lc: the basis values of the
// clamped argument.
struct VjpEdge {
    double r0, r1, w, rho0, rho1, rho2;
    double p00, p01, p10, p11;           // P = I + df/dx1
    double lr[3], lc[3];
};

__device__ __forceinline__ void vjp_block(const float (&flow)[18], const float simf, const int kind, const int tukey_variant,
                                          const double x1r, const double x1c, const double x2r, const double x2c, VjpEdge &o) {
    double dlr[3], dlc[3];
    eval_basis(x1r, o.lr, dlr);
    eval_basis(x1c, o.lc, dlc);
    double f0 = 0., f1 = 0., fr0 = 0., fr1 = 0., fc0 = 0., fc1 = 0.;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a0 = (double)flow[6 * i], a1 = (double)flow[6 * i + 1], b0 = (double)flow[6 * i + 2], b1 = (double)flow[6 * i + 3],
                     c0 = (double)flow[6 * i + 4], c1 = (double)flow[6 * i + 5];
        const double t0 = o.lc[0] * a0 + o.lc[1] * b0 + o.lc[2] * c0, t1 = o.lc[0] * a1 + o.lc[1] * b1 + o.lc[2] * c1;
        const double u0 = dlc[0] * a0 + dlc[1] * b0 + dlc[2] * c0, u1 = dlc[0] * a1 + dlc[1] * b1 + dlc[2] * c1;
        f0 += o.lr[i] * t0; f1 += o.lr[i] * t1;
        fr0 += dlr[i] * t0; fr1 += dlr[i] * t1;
        fc0 += o.lr[i] * u0; fc1 += o.lr[i] * u1;
    }
    o.r0 = x2r - x1r - f0; o.r1 = x2c - x1c - f1;
    const double s = o.r0 * o.r0 + o.r1 * o.r1;
    o.w = (double)simf;
    if (kind == 0) {                                   // CauchyLoss(0.25)
        const double sum = 1.0 + s * kCauchyC;
        o.rho0 = kCauchyB * log_ge1(sum);
        o.rho1 = 1.0 / sum;
        o.rho2 = -kCauchyC * (o.rho1 * o.rho1);
    } else {                                           // TukeyLoss(0.0625), Ceres 1.x (1) or 2.x (2)
        const double k0 = (tukey_variant == 1) ? kTukeyA2 / 6.0 : kTukeyA2 / 3.0, k1 = (tukey_variant == 1) ? 0.5 : 1.0;
        if (!(s > kTukeyA2)) {                         // (a NaN comes here and stays a NaN)
            const double v = 1.0 - s / kTukeyA2, v2 = v * v;
            o.rho0 = k0 * (1.0 - v2 * v);
            o.rho1 = k1 * v2;
            o.rho2 = -(2.0 * k1 / kTukeyA2) * v;       // = -6 k0 / a^4 (1 - s/a^2)
        } else { o.rho0 = k0; o.rho1 = 0.0; o.rho2 = 0.0; }
    }
    o.p00 = 1.0 + fr0; o.p01 = fc0; o.p10 = fr1; o.p11 = 1.0 + fc1;
}

__device__ __forceinline__ double vjp_bar(const void *p, const size_t i, const int f64) {
    return f64 ? static_cast<const double *>(p)[i] : (double)static_cast<const float *>(p)[i];
}

// q = cbar w rho' r + rbar + wbar 2 rho'' r of directed edge `id`: the bar of the raw residual, every gradient is linear in it
__device__ __forceinline__ void vjp_q(const VjpArgs &a, const VjpEdge &o, const double cbar, const uint32_t id, double &q0, double &q1) {
    double c = cbar * (o.w * o.rho1), rb0 = 0.0, rb1 = 0.0;
    if (a.wbar) c += vjp_bar(a.wbar, id, a.f64) * (2.0 * o.rho2);
    if (a.rbar) { rb0 = vjp_bar(a.rbar, 2 * (size_t)id, a.f64); rb1 = vjp_bar(a.rbar, 2 * (size_t)id + 1, a.f64); }
    q0 = c * o.r0 + rb0; q1 = c * o.r1 + rb1;
}

// the record's per-match outputs: its direction's similarity term cbar 1/2 rho and its flow row g[6 i + 2 j + k] = -Lr_i Lc_j q_k
__device__ __forceinline__ void vjp_store_match(const VjpArgs &a, const uint32_t id, const VjpEdge &o, const double q0, const double q1,
                                                const double cbar) {
    if (a.g_sim_dir) a.g_sim_dir[id] = cbar * (0.5 * o.rho0);
    if (!a.g_disp1) return;
    double g[18];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double bij = o.lr[i] * o.lc[j];
            g[6 * i + 2 * j] = -(bij * q0); g[6 * i + 2 * j + 1] = -(bij * q1);
        }
    const size_t row = 18 * (size_t)(id >> 1);
    void *out = (id & 1u) ? a.g_disp1 : a.g_disp2;
    if (a.f64) {
        double *dst = static_cast<double *>(out) + row;
        if (a.wide) {
#pragma unroll
            for (int c = 0; c < 9; ++c) reinterpret_cast<double2 *>(dst)[c] = make_double2(g[2 * c], g[2 * c + 1]);
        } else {
#pragma unroll
            for (int c = 0; c < 18; ++c) dst[c] = g[c];
        }
    } else {
        float *dst = static_cast<float *>(out) + row;
        if (a.wide) {
#pragma unroll
            for (int c = 0; c < 9; ++c) reinterpret_cast<float2 *>(dst)[c] = make_float2((float)g[2 * c], (float)g[2 * c + 1]);
        } else {
#pragma unroll
            for (int c = 0; c < 18; ++c) dst[c] = (float)g[c];
        }
    }
}

// ---- packed classes: eval_group_body's layout, the position gradient accumulated in the group's LDS in the same order ----
template <int KC>
__device__ __forceinline__ void vjp_group_body(const VjpArgs &a, const int desc_begin, const int desc_end, const int block_in_class,
                                               unsigned char *lds_raw) {
    constexpr int NV = PackedClass<KC>::NV, S = PackedClass<KC>::S, EPL = PackedClass<KC>::EPL;
    PackedGroup<KC> grp;
    if (!grp.init(a.descs, desc_begin, desc_end, block_in_class)) return;
    const int sl = grp.sl, ci = grp.ci, n_var = grp.n_var, nv2 = grp.nv2, E = grp.E;
    const CompDesc &d = grp.d;
    static_assert(PackedClass<KC>::G * sizeof(EvalLds<NV>) <= kEvalPackedLdsBytes, "LDS budget");
    EvalLds<NV> &L = reinterpret_cast<EvalLds<NV> *>(lds_raw)[grp.gid];

    const double cbar = (grp.have && a.cbar) ? a.cbar[ci] : 0.0;                                          // one address per group
    for (int i = sl; i < NV + 2; i += S) {
        L.x[i] = (i < nv2) ? a.positions[2 * (size_t)a.node_ids[d.node_off + (i >> 1)] + (i & 1)] : 0.0;
        L.g[i] = 0.0;
    }
    wave_lds_sync();

    bool bad = false;
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
        const int p = sl + S * k;
        if (!(p < E)) continue;
        float flow_k[18]; float sim_k; uint32_t pk;
        load_packed_edge<false>(a, d.edge_off + p, flow_k, sim_k, pk);
        const int es = (int)(pk & 0xffffu), ed = (int)((pk >> 16) & 0x7fffu), ekind = (int)(pk >> 31);
        const int xa = 2 * min(es, n_var), xb = 2 * min(ed, n_var);      // constants read the zero slot
        const uint32_t id = a.eid ? a.eid[d.edge_off + p] : 0u;
        if (id >= a.n_dir && a.eid) continue;                            // (cannot happen: every record maps to an edge of the graph)
        VjpEdge o;
        vjp_block(flow_k, sim_k, ekind, a.tukey_variant, L.x[xa], L.x[xa + 1], L.x[xb], L.x[xb + 1], o);
        double q0, q1;
        vjp_q(a, o, cbar, id, q0, q1);
        bad |= !(isfinite(q0) && isfinite(q1));
        if (a.grad) {
            if (es < n_var) { atomicAdd(&L.g[xa], -(o.p00 * q0 + o.p10 * q1)); atomicAdd(&L.g[xa + 1], -(o.p01 * q0 + o.p11 * q1)); }
            if (ed < n_var) { atomicAdd(&L.g[xb], q0); atomicAdd(&L.g[xb + 1], q1); }
        }
        if (a.eid) vjp_store_match(a, id, o, q0, q1, cbar);
    }
    wave_lds_sync();
    if (bad) a.bad[ci] = 1u;                           // (a lane with a record belongs to a component; every writer stores the same word)
    if (a.grad && sl < nv2) a.grad[2 * (size_t)a.node_ids[d.node_off + (sl >> 1)] + (sl & 1)] = L.g[sl];
}

// all packed classes in ONE launch, the blocks dealt to the classes as in evaluate_packed_kernel
__global__ __launch_bounds__(64) void evaluate_vjp_packed_kernel(const VjpArgs a, const PackedRanges r) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kEvalPackedLdsBytes];
    packed_dispatch(r, [&](auto kc, int desc_begin, int desc_end, int block_in_class) LFR_INLINE_LAMBDA {
        vjp_group_body<decltype(kc)::value>(a, desc_begin, desc_end, block_in_class, lds_raw);
    });
}

// ---- workgroup classes: evaluate_block_kernel's walk.  The out-edge visit forms q, stores the record's per-match outputs and adds
// the source side; the in-edge visit of a variable node forms the same q again from that record's bars and adds the destination side
template <int T>
__global__ __launch_bounds__(T) void evaluate_vjp_block_kernel(const VjpArgs a) {
    const int di = a.desc_begin + blockIdx.x, tid = threadIdx.x;
    const CompDesc d = a.descs[di];
    const int nv = d.n_var, nn = d.n_nodes;
    const uint32_t ne = d.n_edges;
    const uint32_t *ids = a.node_ids + d.node_off;
    const double cbar = a.cbar ? a.cbar[di] : 0.0;
    auto xof = [&](int m, int c) -> double { return m < nv ? a.positions[2 * (size_t)ids[m] + c] : 0.0; };
    bool bad = false;
    for (int l = tid; l < nn; l += T) {                       // variable nodes, then the constants (out-edges only)
        const lfr::NodeInc ni = a.node_inc[d.node_off + l];
        const double xr = xof(l, 0), xc = xof(l, 1);
        double g0 = 0.0, g1 = 0.0;
        for_out_records(ni, ne, [&](const uint32_t p) {       // l -> m
            const uint32_t id = a.eid ? a.eid[d.edge_off + p] : 0u;
            if (id >= a.n_dir && a.eid) return;               // (cannot happen: every record maps to an edge of the graph)
            float fl[18]; float sm; uint32_t pk;
            load_packed_edge<false>(a, d.edge_off + p, fl, sm, pk);
            const int m = (int)((pk >> 16) & 0x7fffu), kind = (int)(pk >> 31);
            VjpEdge o;
            vjp_block(fl, sm, kind, a.tukey_variant, xr, xc, xof(m, 0), xof(m, 1), o);
            double q0, q1;
            vjp_q(a, o, cbar, id, q0, q1);
            bad |= !(isfinite(q0) && isfinite(q1));
            g0 -= o.p00 * q0 + o.p10 * q1; g1 -= o.p01 * q0 + o.p11 * q1;
            if (a.eid) vjp_store_match(a, id, o, q0, q1, cbar);
        });
        if (!a.grad || l >= nv) continue;
        for_in_records(ni, a.in_idx, d.edge_off, ne, [&](const uint32_t p) {      // m -> l
            const uint32_t id = a.eid ? a.eid[d.edge_off + p] : 0u;
            if (id >= a.n_dir && a.eid) return;
            float fl[18]; float sm; uint32_t pk;
            load_packed_edge<false>(a, d.edge_off + p, fl, sm, pk);
            const int m = (int)(pk & 0xffffu), kind = (int)(pk >> 31);
            VjpEdge o;
            vjp_block(fl, sm, kind, a.tukey_variant, xof(m, 0), xof(m, 1), xr, xc, o);
            double q0, q1;
            vjp_q(a, o, cbar, id, q0, q1);
            g0 += q0; g1 += q1;
        });
        a.grad[2 * (size_t)ids[l]] = g0; a.grad[2 * (size_t)ids[l] + 1] = g1;
    }
    if (bad) a.bad[di] = 1u;
}

// the two directions' similarity terms in a fixed order: node1 -> node2, then node2 -> node1 (k_bwd_sim's rule)
__global__ void k_vjp_sim(int64_t n_matches, const double *dir, void *out, int f64) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_matches) return;
    const double g = dir[2 * m] + dir[2 * m + 1];
    if (f64) static_cast<double *>(out)[m] = g; else static_cast<float *>(out)[m] = (float)g;
}

// weights of the directions that are no residual block of this shard
__global__ void k_eval_fill_minus_one(size_t n, void *out, int f64) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (f64) static_cast<double *>(out)[i] = -1.0; else static_cast<float *>(out)[i] = -1.0f;
}

// the shared state of a pass (events, latest stream: lfr_batch.hpp) + a cost per descriptor for calls without cost_device.  Set up by
// pass_setup_unsolved, not by pass_begin: the evaluate needs neither a solve nor unchanged inputs, and no workspace for matrices.
struct EvalState : lfr::PassState {
    double *d_cost = nullptr;
    std::vector<double> h_cost;
};

int eval_carve(lfr_batch *b, lfr::PassState *ps) {
    EvalState *s = static_cast<EvalState *>(ps);
    s->d_cost = s->slab.take_n<double>(std::max<size_t>((size_t)b->n_desc, 1));
    if (!s->d_cost) { lfr::set_error("evaluate slab exhausted"); return LFR_ERR_NOMEM; }
    return LFR_OK;
}
const lfr::PassKind kEvaluate = {"evaluate", [] { return static_cast<lfr::PassState *>(new EvalState()); }, eval_carve};

// lfr_batch_evaluate_vjp's own pass state (its events order lfr_batch_set_inputs behind it): the similarity term per directed edge
// and the non-finite mark per descriptor
struct VjpState : lfr::PassState {
    double *d_gsim = nullptr;
    uint32_t *d_bad = nullptr;
    std::vector<uint32_t> h_bad;
};

int vjp_carve(lfr_batch *b, lfr::PassState *ps) {
    VjpState *s = static_cast<VjpState *>(ps);
    s->d_gsim = s->slab.take_n<double>(2 * std::max<size_t>((size_t)b->n_graph_matches, 1));
    s->d_bad = s->slab.take_n<uint32_t>(std::max<size_t>((size_t)b->n_desc, 1));
    if (!s->d_gsim || !s->d_bad) { lfr::set_error("evaluate_vjp slab exhausted"); return LFR_ERR_NOMEM; }
    return LFR_OK;
}
const lfr::PassKind kEvaluateVjp = {"evaluate_vjp", [] { return static_cast<lfr::PassState *>(new VjpState()); }, vjp_carve};

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
    if (!b->eval) {
        const int rc = lfr::pass_setup_unsolved(b, &b->eval, kEvaluate, 8 * std::max<size_t>((size_t)b->n_desc, 1) + 4096);
        if (rc != LFR_OK) return rc;
    }
    EvalState &s = *static_cast<EvalState *>(b->eval);
    hipStream_t st = (hipStream_t)hip_stream;
    const int f64 = (flags & LFR_EVALUATE_F64) ? 1 : 0;
    const size_t M = (size_t)b->n_graph_matches, N = (size_t)b->n_graph_nodes, elt = f64 ? 8 : 4;
    { const int rc = lfr::eval_prologue(b, s, st); if (rc != LFR_OK) return rc; }
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
    lfr::launch_two_layouts(b, evaluate_packed_kernel, evaluate_block_kernel<kEvalThreads>, kEvalThreads, a, st);
    HIP_TRY(hipGetLastError());
    { const int rc = lfr::pass_end(&s, st); if (rc != LFR_OK) return rc; }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        s.h_cost.assign((size_t)b->n_desc, 0.0);
        if (b->n_desc) HIP_TRY(hipMemcpyAsync(s.h_cost.data(), a.cost, 8 * (size_t)b->n_desc, hipMemcpyDeviceToHost, st));
        { const int rc = lfr::pass_wait_ms(&s, st, &stats->kernel_ms); if (rc != LFR_OK) return rc; }
        for (const double c : s.h_cost) {
            if (std::isfinite(c)) stats->sum_cost += c; else ++stats->n_nonfinite;
        }
        stats->n_components = b->n_desc;
    }
    return LFR_OK;
}

int lfr_batch_evaluate_vjp(lfr_batch *b, const double *positions_device, const double *cost_bar_device, const void *residuals_bar_device,
                           const void *weights_bar_device, double *grad_positions_device, void *grad_disp1_device, void *grad_disp2_device,
                           void *grad_sim_device, int flags, void *hip_stream, lfr_evaluate_vjp_stats *stats) {
    // every argument error comes before an output is touched
    if (!b) { lfr::set_error("lfr_batch_evaluate_vjp: no batch"); return LFR_ERR_ARG; }
    if (flags & ~LFR_EVALUATE_F64) { lfr::set_error("lfr_batch_evaluate_vjp: unknown flag bits 0x%x", flags & ~LFR_EVALUATE_F64); return LFR_ERR_ARG; }
    if (!cost_bar_device && !residuals_bar_device && !weights_bar_device) {
        lfr::set_error("lfr_batch_evaluate_vjp: nothing to differentiate (all three bars are NULL)"); return LFR_ERR_ARG;
    }
    if (!grad_positions_device && !grad_disp1_device && !grad_disp2_device && !grad_sim_device) {
        lfr::set_error("lfr_batch_evaluate_vjp: nothing to compute (all four outputs are NULL)"); return LFR_ERR_ARG;
    }
    if (!grad_disp1_device != !grad_disp2_device) { lfr::set_error("lfr_batch_evaluate_vjp: grad_disp1 and grad_disp2 go together (both or neither)"); return LFR_ERR_ARG; }
    if (!positions_device && b->n_solves == 0) {
        lfr::set_error("lfr_batch_evaluate_vjp: the batch has not been solved and no positions are given"); return LFR_ERR_ARG;
    }
    const bool per_match = residuals_bar_device || weights_bar_device || grad_disp1_device || grad_sim_device;
    if (per_match && b->cc_sharded) {
        lfr::set_error("lfr_batch_evaluate_vjp: a batch over one rank's connected components numbers its matches by itself (lfr_problem_build_hip_shard): no per-match bars or gradients");
        return LFR_ERR_UNSUPPORTED;
    }
    HIP_TRY(hipSetDevice(b->device));
    if (per_match) { const int rc = lfr::ensure_edge_map(b); if (rc != LFR_OK) return rc; }
    if (!b->evjp) {
        const size_t nd = std::max<size_t>((size_t)b->n_desc, 1), nm = std::max<size_t>((size_t)b->n_graph_matches, 1);
        const int rc = lfr::pass_setup_unsolved(b, &b->evjp, kEvaluateVjp, 16 * nm + 4 * nd + 4096);
        if (rc != LFR_OK) return rc;
    }
    VjpState &s = *static_cast<VjpState *>(b->evjp);
    hipStream_t st = (hipStream_t)hip_stream;
    const int f64 = (flags & LFR_EVALUATE_F64) ? 1 : 0;
    const size_t M = (size_t)b->n_graph_matches, N = (size_t)b->n_graph_nodes, elt = f64 ? 8 : 4;
    { const int rc = lfr::eval_prologue(b, s, st); if (rc != LFR_OK) return rc; }
    // directions that are no residual block of this shard, and nodes that are not variable, read 0
    if (grad_positions_device && N) HIP_TRY(hipMemsetAsync(grad_positions_device, 0, 2 * N * sizeof(double), st));
    if (grad_disp1_device && M) {
        HIP_TRY(hipMemsetAsync(grad_disp1_device, 0, 18 * M * elt, st));
        HIP_TRY(hipMemsetAsync(grad_disp2_device, 0, 18 * M * elt, st));
    }
    if (grad_sim_device && M) HIP_TRY(hipMemsetAsync(s.d_gsim, 0, 16 * M, st));
    HIP_TRY(hipMemsetAsync(s.d_bad, 0, 4 * std::max<size_t>((size_t)b->n_desc, 1), st));

    VjpArgs a;
    memset(&a, 0, sizeof(a));
    a.descs = b->d_descs; a.edges = b->d_edges; a.node_ids = b->d_node_ids; a.node_inc = b->d_node_inc; a.in_idx = b->d_in_idx;
    a.positions = positions_device ? positions_device : b->d_positions;
    a.eid = per_match ? lfr::edge_map(b) : nullptr;
    a.cbar = cost_bar_device; a.rbar = residuals_bar_device; a.wbar = weights_bar_device;
    a.grad = grad_positions_device; a.g_disp1 = grad_disp1_device; a.g_disp2 = grad_disp2_device;
    a.g_sim_dir = grad_sim_device ? s.d_gsim : nullptr;
    a.bad = s.d_bad;
    a.n_dir = (uint32_t)(2 * M); a.tukey_variant = b->tukey_variant; a.f64 = f64;
    a.wide = (((uintptr_t)grad_disp1_device | (uintptr_t)grad_disp2_device) & (f64 ? 15u : 7u)) == 0;       // (a row is 144 / 72 bytes)
    lfr::launch_two_layouts(b, evaluate_vjp_packed_kernel, evaluate_vjp_block_kernel<kEvalThreads>, kEvalThreads, a, st);
    if (grad_sim_device && M) hipLaunchKernelGGL(k_vjp_sim, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (int64_t)M, s.d_gsim, grad_sim_device, f64);
    HIP_TRY(hipGetLastError());
    { const int rc = lfr::pass_end(&s, st); if (rc != LFR_OK) return rc; }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        s.h_bad.assign((size_t)b->n_desc, 0u);
        if (b->n_desc) HIP_TRY(hipMemcpyAsync(s.h_bad.data(), s.d_bad, 4 * (size_t)b->n_desc, hipMemcpyDeviceToHost, st));
        { const int rc = lfr::pass_wait_ms(&s, st, &stats->kernel_ms); if (rc != LFR_OK) return rc; }
        for (const uint32_t v : s.h_bad) stats->n_nonfinite += v != 0;
        stats->n_components = b->n_desc;
    }
    return LFR_OK;
}

}  // extern "C"
