// The exact Hessian / loss-corrected Gauss-Newton matrix of a component at the solve's x, assembled owner-computes into a packed lower
// triangle, and its zero-skipping LDL^T: the device code the backward pass (lfr_backward.hip) and the covariance of the workgroup
// classes (lfr_covariance.hip) share.
#pragma once

#include "lfr_batch.hpp"
#include "lfr_device.hpp"

namespace lfrdev {

using lfr::CompDesc;
using lfr::CompInfoDev;
using lfr::EdgeRec;


constexpr int kBwdMaxRows = 6144;            // largest system of the HBM variant: its vectors fill the LDS (lfr.h: LFR_ERR_UNSUPPORTED above)

// Derivatives of the biquadratic interpolant (cost.cc:13-48) at the source point, with the reference's zeroing of the first derivative
// outside [-0.5, 0.5] (cost.cc:38-43) carried over to the second derivatives.
struct BwdEdge {
    double lr[3], dlr[3], d2lr[3], lc[3], dlc[3], d2lc[3];
    double f[2], fr[2], fc[2], frr[2], frc[2], fcc[2];
    double r[2], w, rho1, rho2;
};

__device__ __forceinline__ void bwd_basis(double x, double (&l)[3], double (&dl)[3], double (&d2l)[3]) {
    const double t = fmax(fmin(x, 0.5), -0.5);
    const bool in = (t == x);
    l[0] = 2. * t * (t - .5); l[1] = (-4.) * (t - .5) * (t + .5); l[2] = 2. * t * (t + .5);
    dl[0] = in ? 2. * t + 2. * (t - .5) : 0.; dl[1] = in ? (-4.) * (t - .5) + (-4.) * (t + .5) : 0.; dl[2] = in ? 2. * t + 2. * (t + .5) : 0.;
    d2l[0] = in ? 4. : 0.; d2l[1] = in ? -8. : 0.; d2l[2] = in ? 4. : 0.;
}

// (flow, sim: the record's 18 flow values and its similarity, as an EdgeRec holds them or as load_packed_edge hands them over)
__device__ __forceinline__ void bwd_eval(const float (&flow)[18], const float sim, int kind, int tukey_variant, double x1r, double x1c,
                                         double x2r, double x2c, BwdEdge &o) {
    bwd_basis(x1r, o.lr, o.dlr, o.d2lr);
    bwd_basis(x1c, o.lc, o.dlc, o.d2lc);
#pragma unroll
    for (int k = 0; k < 2; ++k) { o.f[k] = o.fr[k] = o.fc[k] = o.frr[k] = o.frc[k] = o.fcc[k] = 0.; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double d = (double)flow[2 * (3 * i + j) + k];
                o.f[k] += o.lr[i] * o.lc[j] * d;
                o.fr[k] += o.dlr[i] * o.lc[j] * d;
                o.fc[k] += o.lr[i] * o.dlc[j] * d;
                o.frr[k] += o.d2lr[i] * o.lc[j] * d;
                o.frc[k] += o.dlr[i] * o.dlc[j] * d;
                o.fcc[k] += o.lr[i] * o.d2lc[j] * d;
            }
    o.r[0] = x2r - x1r - o.f[0];
    o.r[1] = x2c - x1c - o.f[1];
    const double s = o.r[0] * o.r[0] + o.r[1] * o.r[1];
    o.w = (double)sim;
    if (kind == 0) {                                   // CauchyLoss(0.25)
        const double inv = 1.0 / (1.0 + s * kCauchyC);
        o.rho1 = fmax(DBL_MIN, inv);
        o.rho2 = -kCauchyC * inv * inv;
    } else if (s <= kTukeyA2) {                        // TukeyLoss(0.0625), Ceres 1.x (1) or 2.x (2)
        const double v = 1.0 - s / kTukeyA2;
        o.rho1 = tukey_variant == 1 ? 0.5 * v * v : v * v;
        o.rho2 = tukey_variant == 1 ? -v / kTukeyA2 : -2.0 * v / kTukeyA2;
    } else {
        o.rho1 = 0.; o.rho2 = 0.;
    }
}

__device__ __forceinline__ void bwd_eval(const EdgeRec &e, int kind, int tukey_variant, double x1r, double x1c, double x2r, double x2c,
                                         BwdEdge &o) {
    bwd_eval(e.flow, e.sim, kind, tukey_variant, x1r, x1c, x2r, x2c, o);
}

// M = w (rho' I + 2 rho'' r r^T), P = I + df/dx_src: the edge's Hessian over (x_src, x_dst) is [[P^T M P - w rho' sum_k r_k d2f_k, -P^T M],
// [-M P, M]].
template <bool EXACT = true>
__device__ __forceinline__ void bwd_blocks(const BwdEdge &o, double (&M)[2][2], double (&P)[2][2]) {
    const double a = o.w * o.rho1, b = EXACT ? 2.0 * o.w * o.rho2 : 0.0;      // (not EXACT: M = w rho' I, the Gauss-Newton part)
    M[0][0] = a + b * o.r[0] * o.r[0]; M[0][1] = b * o.r[0] * o.r[1]; M[1][0] = M[0][1]; M[1][1] = a + b * o.r[1] * o.r[1];
    P[0][0] = 1.0 + o.fr[0]; P[0][1] = o.fc[0]; P[1][0] = o.fr[1]; P[1][1] = 1.0 + o.fc[1];
}

struct BwdArgs {
    const CompDesc *descs;
    const EdgeRec *edges;
    const uint32_t *node_ids;
    const lfr::NodeInc *node_inc;
    const uint32_t *in_idx;
    const double *positions;
    const CompInfoDev *infos;
    const double *grad_pos;       // dL/dx of the whole graph (2 per node)
    const uint32_t *eid;          // per record: directed edge id of the graph (2m: node1 -> node2, 2m+1: node2 -> node1)
    double *hws;                  // HBM variant: packed lower triangles
    const uint64_t *hws_off;      // per descriptor (doubles)
    void *g_disp1, *g_disp2;      // n_matches x 18, float or double
    double *g_sim_dir;            // per directed edge
    int32_t *status;              // per descriptor
    unsigned long long *counters; // [0] coordinates held at a bound
    uint32_t n_matches;
    int desc_begin, tukey_variant, f64;
    int scan_all;                 // records in edge-id order (packed classes): no out-edge runs
};

__host__ __device__ __forceinline__ size_t bwd_tri(int i, int j) { return (size_t)i * (i + 1) / 2 + j; }     // j <= i

// The matrix of a component's normal equations, lower triangle, owner computes: the thread of node l owns rows 2l, 2l+1 (columns of
// nodes <= l) and sums them over the node's out- and in-edges in record order.  EXACT: the backward's Hessian (rho'' and the
// interpolant's second derivatives included); otherwise the loss-corrected Gauss-Newton matrix J^T J = sum_e w rho' [[P^T P, -P^T],
// [-P, I]].  BOUNDS: coordinates with fr[i] == 0 become identity rows and columns (both modes of the backward); without it fr is not
// read (the covariance, lfr_covariance.hip, ignores the bounds).
template <int T, bool EXACT, bool BOUNDS = EXACT>
__device__ __forceinline__ void bwd_assemble(const BwdArgs &a, const CompDesc &d, const int nv, const EdgeRec *E, const uint32_t *ids,
                                             double *H, const uint8_t *fr, const int tid) {
    // The workgroup classes' records come by source node (out-edges contiguous, NodeInc); the packed classes' in edge-id order: a thread scans them all (at most the largest packed class's max_edges)
    auto xof = [&](int m, int c) -> double { return m < nv ? a.positions[2 * (size_t)ids[m] + c] : 0.0; };
    for (int l = tid; l < nv; l += T) {
        lfr::NodeInc ni = a.node_inc[d.node_off + l];
        if (a.scan_all) { ni.out_begin = 0; ni.out_count = d.n_edges; ni.in_count = 0; }
        const double xr = xof(l, 0), xc = xof(l, 1);
        double hd[3] = {0., 0., 0.};                          // (2l,2l) (2l+1,2l) (2l+1,2l+1)
        for (uint32_t k = 0; k < ni.out_count; ++k) {         // l -> m (packed classes: and m -> l)
            const EdgeRec e = E[ni.out_begin + k];
            const int m = e.dst_kind & 0x7fff, kind = e.dst_kind >> 15;
            if (a.scan_all && e.src != l) {
                if (m != l) continue;
                const int sm = e.src;                         // in-edge sm -> l
                BwdEdge o;
                bwd_eval(e, kind, a.tukey_variant, xof(sm, 0), xof(sm, 1), xr, xc, o);
                double M[2][2], P[2][2];
                bwd_blocks<EXACT>(o, M, P);
                hd[0] += M[0][0]; hd[1] += M[1][0]; hd[2] += M[1][1];
                if (sm < l) {
#pragma unroll
                    for (int p = 0; p < 2; ++p)
#pragma unroll
                        for (int q = 0; q < 2; ++q) H[bwd_tri(2 * l + p, 2 * sm + q)] -= M[p][0] * P[0][q] + M[p][1] * P[1][q];
                }
                continue;
            }
            BwdEdge o;
            bwd_eval(e, kind, a.tukey_variant, xr, xc, xof(m, 0), xof(m, 1), o);
            double M[2][2], P[2][2];
            bwd_blocks<EXACT>(o, M, P);
            double PM[2][2], S[2][2];                         // P^T M, P^T M P - w rho' sum_k r_k d2f_k
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int q = 0; q < 2; ++q) PM[p][q] = P[0][p] * M[0][q] + P[1][p] * M[1][q];
            const double c = o.w * o.rho1;
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int q = 0; q < 2; ++q) S[p][q] = PM[p][0] * P[0][q] + PM[p][1] * P[1][q];
            if constexpr (EXACT) {
                S[0][0] -= c * (o.r[0] * o.frr[0] + o.r[1] * o.frr[1]);
                S[1][0] -= c * (o.r[0] * o.frc[0] + o.r[1] * o.frc[1]);
                S[1][1] -= c * (o.r[0] * o.fcc[0] + o.r[1] * o.fcc[1]);
            }
            hd[0] += S[0][0]; hd[1] += S[1][0]; hd[2] += S[1][1];
            if (m < l) {                                      // src-dst block: -P^T M
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int q = 0; q < 2; ++q) H[bwd_tri(2 * l + p, 2 * m + q)] -= PM[p][q];
            }
        }
        for (uint32_t k = 0; k < ni.in_count; ++k) {          // m -> l
            const EdgeRec e = E[a.in_idx[d.edge_off + ni.in_begin + k]];
            const int m = e.src, kind = e.dst_kind >> 15;
            BwdEdge o;
            bwd_eval(e, kind, a.tukey_variant, xof(m, 0), xof(m, 1), xr, xc, o);
            double M[2][2], P[2][2];
            bwd_blocks<EXACT>(o, M, P);
            hd[0] += M[0][0]; hd[1] += M[1][0]; hd[2] += M[1][1];
            if (m < l) {                                      // dst-src block: -M P
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int q = 0; q < 2; ++q) H[bwd_tri(2 * l + p, 2 * m + q)] -= M[p][0] * P[0][q] + M[p][1] * P[1][q];
            }
        }
        H[bwd_tri(2 * l, 2 * l)] += hd[0]; H[bwd_tri(2 * l + 1, 2 * l)] += hd[1]; H[bwd_tri(2 * l + 1, 2 * l + 1)] += hd[2];
        if constexpr (BOUNDS)
            for (int p = 0; p < 2; ++p) {                     // bound coordinates: identity rows and columns
                const int i = 2 * l + p;
                for (int j = 0; j <= i; ++j)
                    if (!fr[i] || !fr[j]) H[bwd_tri(i, j)] = (i == j) ? 1.0 : 0.0;
            }
    }
}

// LDL^T of the packed lower triangle H (n rows), right-looking over the nonzeros of each column (D on the diagonal, L below it).
// lval / lidx: n entries of scratch, cnt: two counters (cnt[0] = cnt[1] = 0 on entry).  Returns true when a pivot was not positive
// (or not finite); every thread returns the same.
template <int T>
__device__ __forceinline__ bool bwd_ldlt(double *H, const int n, double *lval, int *lidx, int *cnt, const int tid) {
    bool indefinite = false;
    for (int k = 0; k < n; ++k) {
        const double dk = H[bwd_tri(k, k)];
        if (!(dk > 0.0) || !isfinite(dk)) { indefinite = true; break; }       // (uniform: every thread read the same pivot)
        const double dinv = 1.0 / dk;
        int *c = &cnt[k & 1];
        for (int i = k + 1 + tid; i < n; i += T) {
            const double x = H[bwd_tri(i, k)];
            if (x != 0.0) { const int p = atomicAdd(c, 1); lidx[p] = i; lval[p] = x; }
        }
        __syncthreads();
        const int nc = *c;
        if (tid == 0) cnt[(k + 1) & 1] = 0;
        for (int t = tid; t < nc * nc; t += T) {
            const int p = t / nc, q = t - p * nc, i = lidx[p], j = lidx[q];
            if (j <= i) H[bwd_tri(i, j)] -= lval[p] * (lval[q] * dinv);
        }
        for (int p = tid; p < nc; p += T) H[bwd_tri(lidx[p], k)] = lval[p] * dinv;
        __syncthreads();
    }
    return indefinite;
}

// The Gauss-Newton fallback of the backward and the jvp (LFR_BACKWARD_FALLBACK_GAUSS_NEWTON, LFR_JVP_FALLBACK_GAUSS_NEWTON): after
// bwd_ldlt has reported the exact Hessian indefinite, the same workgroup clears the half-factored triangle, assembles the Gauss-Newton
// matrix over the same free set fr (bound rows and columns the identity's) and factors again.  The right-hand side, fr and the
// bound-coordinate count are the caller's and are not touched.  Every thread of the block calls it (the verdict it follows is
// block-uniform) and every thread returns the same: true when J^T J met a pivot that is not positive (or not finite) too.
template <int T>
__device__ __forceinline__ bool bwd_refactor_gauss_newton(const BwdArgs &a, const CompDesc &d, const int nv, const EdgeRec *E,
                                                          const uint32_t *ids, double *H, const int n, const uint8_t *fr, double *lval,
                                                          int *lidx, int *cnt, const int tid) {
    __syncthreads();                                          // every thread has read the pivot that failed
    const size_t nt = bwd_tri(n, 0);
    for (size_t t = tid; t < nt; t += T) H[t] = 0.0;
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();
    bwd_assemble<T, false, true>(a, d, nv, E, ids, H, fr, tid);
    __syncthreads();
    return bwd_ldlt<T>(H, n, lval, lidx, cnt, tid);
}

// ---- forward-mode sensitivity (lfr_jvp.hip): the transpose of the backward's vector-Jacobian sweep ----
// The tangent of one record's inputs: the 18 flow values and the similarity of directed edge `id` in the match layout (even ids read
// tan_disp2, odd ids tan_disp1, both tan_sim); a NULL array is a zero tangent.  f64: the arrays hold doubles instead of floats.
struct JvpTangent {
    const void *disp1, *disp2, *sim;
    uint32_t n_matches;
    int f64;
};

__device__ __forceinline__ void jvp_load_tangent(const JvpTangent &t, const uint32_t id, double (&phidot)[18], double &wdot) {
    const uint32_t m = id >> 1;
    const bool in = m < t.n_matches;                          // (always: every record maps to an edge of the graph)
    const void *fl = (id & 1u) ? t.disp1 : t.disp2;
#pragma unroll
    for (int i = 0; i < 18; ++i) {
        double v = 0.0;
        if (in && fl) v = t.f64 ? static_cast<const double *>(fl)[18 * (size_t)m + i] : (double)static_cast<const float *>(fl)[18 * (size_t)m + i];
        phidot[i] = v;
    }
    wdot = 0.0;
    if (in && t.sim) wdot = t.f64 ? static_cast<const double *>(t.sim)[m] : (double)static_cast<const float *>(t.sim)[m];
}

// -d/d eps [grad_x F_e(x^; theta_e + eps thetadot_e)] of one record evaluated as `o` (bwd_eval): its two rows at the source (bs) and at
// the destination (bd).  With rdot = -sum_ij lr_i lc_j phidot_ij, sdot = 2 r . rdot and Pdot = d/d eps (I + df/dx_src):
//   d grad_dst =   wdot rho' r     + w (rho'' sdot r     + rho' rdot)
//   d grad_src = -[wdot rho' P^T r + w (rho'' sdot P^T r + rho' (Pdot^T r + P^T rdot))]
__device__ __forceinline__ void jvp_rhs_edge(const BwdEdge &o, const double (&phidot)[18], const double wdot, double (&bs)[2], double (&bd)[2]) {
    double rd[2] = {0., 0.}, pr[2] = {0., 0.}, pc[2] = {0., 0.};      // rdot, Pdot's columns
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double d = phidot[2 * (3 * i + j) + k];
                rd[k] -= o.lr[i] * o.lc[j] * d;
                pr[k] += o.dlr[i] * o.lc[j] * d;
                pc[k] += o.lr[i] * o.dlc[j] * d;
            }
    const double sdot = 2.0 * (o.r[0] * rd[0] + o.r[1] * rd[1]);
    const double c0 = wdot * o.rho1 + o.w * o.rho2 * sdot, c1 = o.w * o.rho1;      // d grad_dst = c0 r + c1 rdot
    bd[0] = -(c0 * o.r[0] + c1 * rd[0]);
    bd[1] = -(c0 * o.r[1] + c1 * rd[1]);
    const double ptr0 = (1.0 + o.fr[0]) * o.r[0] + o.fr[1] * o.r[1], ptr1 = o.fc[0] * o.r[0] + (1.0 + o.fc[1]) * o.r[1];      // P^T r
    const double q0 = pr[0] * o.r[0] + pr[1] * o.r[1] + (1.0 + o.fr[0]) * rd[0] + o.fr[1] * rd[1];      // Pdot^T r + P^T rdot
    const double q1 = pc[0] * o.r[0] + pc[1] * o.r[1] + o.fc[0] * rd[0] + (1.0 + o.fc[1]) * rd[1];
    bs[0] = c0 * ptr0 + c1 * q0;
    bs[1] = c0 * ptr1 + c1 * q1;
}
}  // namespace lfrdev
