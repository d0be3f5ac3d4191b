// The per-record arithmetic of the matrix-free passes: what lfr_hessian_product.hip (H v) and lfr_hessian_solve.hip (the conjugate
// gradients around it) both apply.  One text for both translation units, so that the product's bits do not depend on which of them
// a record went through.
#pragma once

#include "lfr_hessian_device.hpp"

namespace lfrdev {

// What one record contributes, formed once for all vectors: M (symmetric), P and, in the exact mode, the second-derivative block
// S = w rho' sum_k r_k d2f_k (symmetric)
struct HvpEdge {
    double m00, m01, m11;
    double p00, p01, p10, p11;
    double s00, s01, s11;
};

template <bool EXACT>
__device__ __forceinline__ void hvp_edge(const float (&flow)[18], const float sim, const int kind, const int tukey_variant, const double x1r,
                                         const double x1c, const double x2r, const double x2c, HvpEdge &h) {
    BwdEdge o;
    bwd_eval(flow, sim, kind, tukey_variant, x1r, x1c, x2r, x2c, o);
    double M[2][2], P[2][2];
    bwd_blocks<EXACT>(o, M, P);
    h.m00 = M[0][0]; h.m01 = M[1][0]; h.m11 = M[1][1];
    h.p00 = P[0][0]; h.p01 = P[0][1]; h.p10 = P[1][0]; h.p11 = P[1][1];
    if constexpr (EXACT) {
        const double c = o.w * o.rho1;                // bwd_assemble's own term
        h.s00 = c * (o.r[0] * o.frr[0] + o.r[1] * o.frr[1]);
        h.s01 = c * (o.r[0] * o.frc[0] + o.r[1] * o.frc[1]);
        h.s11 = c * (o.r[0] * o.fcc[0] + o.r[1] * o.fcc[1]);
    } else {
        h.s00 = h.s01 = h.s11 = 0.0;
    }
}

// One vector through one record: (vs, vd) its values at the source and the destination, (hs, hd) the record's rows there.  Every
// product and sum is written out with its rounding, so the bits of a vector's outputs do not depend on the instantiation.
template <bool EXACT>
__device__ __forceinline__ void hvp_apply(const HvpEdge &h, const double vs0, const double vs1, const double vd0, const double vd1,
                                          double &hs0, double &hs1, double &hd0, double &hd1) {
#pragma clang fp contract(off)
    const double u0 = vd0 - fma(h.p01, vs1, h.p00 * vs0), u1 = vd1 - fma(h.p11, vs1, h.p10 * vs0);      // v_dst - P v_src
    hd0 = fma(h.m01, u1, h.m00 * u0);
    hd1 = fma(h.m11, u1, h.m01 * u0);                                                                   // t = M u
    double a0 = fma(h.p10, hd1, h.p00 * hd0), a1 = fma(h.p11, hd1, h.p01 * hd0);                        // P^T t
    if constexpr (EXACT) {
        a0 += fma(h.s01, vs1, h.s00 * vs0);
        a1 += fma(h.s11, vs1, h.s01 * vs0);
    }
    hs0 = -a0; hs1 = -a1;
}

// a node's two terms of the curvature, with their roundings written out for the same reason
__device__ __forceinline__ double hvp_dot2(const double v0, const double h0, const double v1, const double h1) {
#pragma clang fp contract(off)
    return fma(v1, h1, v0 * h0);
}
__device__ __forceinline__ double hvp_mul(const double v, const double h) {
#pragma clang fp contract(off)
    return v * h;
}

}  // namespace lfrdev
