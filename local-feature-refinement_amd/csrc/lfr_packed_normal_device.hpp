// The loss-corrected Gauss-Newton matrix J^T J of the packed classes (<= 32 rows) and its inversion in registers: the device code the
// covariance (lfr_covariance.hip) and the Gauss-Newton mode of the backward pass (lfr_backward.hip) share.  A wave64 hosts 64/S
// components, one-wave workgroups, no barriers:
//   cov_assemble()   one sweep at x^ with the forward's eval_edge and the matrix part of its LDS adds (five per edge) into the group's
//                    CovLds
//   cov_invert()     in-place Gauss-Jordan INVERSION with one row per lane and all n columns of the row in registers; the pivot row
//                    travels as the DPP operand of v_fmac_f64 (8- and 16-row classes) or through ds_swizzle (32-row classes)
#pragma once

#include <type_traits>

#include "lfr_batch.hpp"
#include "lfr_device.hpp"
#include "lfr_packed_frame.hpp"

namespace lfrdev {

// ---- in-register Gauss-Jordan inversion, lane = row ----
// Step K: every lane takes pivot row K (before the step), p = its pivot; rows i != K: h_ij -= (h_iK / p) h_Kj for j != K and
// h_iK = -h_iK / p; row K: h_Kj /= p and h_KK = 1 / p.  After n steps h is the inverse.  No pivoting (SPD); padded rows are identity.
// Column K rides through the rank-1 update with the others (one wasted multiply-add) and is then overwritten.
template <int K, int BANK, int C0, int CL>
__device__ __forceinline__ void cov_fmac_cols(double nf, double (&h)[CL]) {
    constexpr int n = CL - C0;
    if constexpr (n >= 4) {
        fmac_bcast<K, BANK>(nf, h[C0], h[C0 + 1], h[C0 + 2], h[C0 + 3]);
        cov_fmac_cols<K, BANK, C0 + 4, CL>(nf, h);
    } else if constexpr (n == 3) fmac_bcast<K, BANK>(nf, h[C0], h[C0 + 1], h[C0 + 2]);
    else if constexpr (n == 2) fmac_bcast<K, BANK>(nf, h[C0], h[C0 + 1]);
    else if constexpr (n == 1) fmac_bcast<K, BANK>(nf, h[C0]);
}

template <int NV, int K, int CL>
struct CovGaussJordan {
    static __device__ __forceinline__ void run(double (&h)[CL], double &minpiv, const int row, const int n_steps) {
        const bool is_k = row == K;
        double rp, nf;
        if constexpr (NV <= 16) {
            // the group sits inside one 16-lane DPP row: row_newbcast:K inside the v_fmac_f64 (NV == 8: two groups per DPP row, the
            // update is issued per half with a bank mask).  Every asm statement of these helpers opens with s_nop 1 (lfr_device.hpp).
            const double piv = (NV == 16) ? bcast16_f64<K>(h[K]) : bcast8_f64<K>(h[K]);
            minpiv = fmin(minpiv, piv);
            rp = 1.0 / piv;
            nf = is_k ? 0.0 : -(h[K] * rp);                            // (the pivot lane's own row stays: h += 0 * h)
            if constexpr (NV == 16) cov_fmac_cols<K, 0xf, 0, CL>(nf, h);
            else { cov_fmac_cols<K, 0x3, 0, CL>(nf, h); cov_fmac_cols<K + 8, 0xc, 0, CL>(nf, h); }
        } else {
            // one burst of ds_swizzle broadcasts inside the 32-lane half (the <32,2> class holds its rows twice, once per half)
            double pr[CL];
#pragma unroll
            for (int c = 0; c < CL; ++c) pr[c] = swz_bcast<0x00, K>(h[c]);
            const double piv = pr[K];
            minpiv = fmin(minpiv, piv);
            rp = 1.0 / piv;
            nf = is_k ? 0.0 : -(h[K] * rp);
#pragma unroll
            for (int c = 0; c < CL; ++c) h[c] = fma(nf, pr[c], h[c]);
        }
        const double sc = is_k ? rp : 1.0;                             // the pivot row is scaled, the others multiply by an exact 1
#pragma unroll
        for (int c = 0; c < CL; ++c) h[c] *= sc;
        h[K] = is_k ? rp : nf;
        if constexpr (K + 1 < CL) {
            if (K + 1 < n_steps) CovGaussJordan<NV, K + 1, CL>::run(h, minpiv, row, n_steps);
        }
    }
};

// The inversion of packed class KC in the instantiation sized for the largest system of the wave (n_max, wave-uniform, at most the
// class's max_rows): build(c) = the lane's entry of column c, sink(h, ok) takes the lane's row of the inverse; ok = false: a pivot of
// the lane's group was not positive.  Every lane of the wave must be active.
template <int KC, class Build, class Sink>
__device__ __forceinline__ void cov_invert(const int row, const int n_max, Build &&build, Sink &&sink) {
    constexpr int NV = PackedClass<KC>::NV, kRows = PackedClass<KC>::max_rows;
    auto run = [&](auto cl_tag) {
        constexpr int CL = decltype(cl_tag)::value;
        double h[CL];
#pragma unroll
        for (int c = 0; c < CL; ++c) h[c] = build(c);
        double minpiv = 1.0;
        CovGaussJordan<NV, 0, CL>::run(h, minpiv, row, n_max);
        sink(h, minpiv > 0.0);
    };
#define LFR_COV_CL(n) run(std::integral_constant<int, n>{})
    if constexpr (KC == lfr::KC_G8) {
        if (n_max <= 2) LFR_COV_CL(2); else if (n_max <= 4) LFR_COV_CL(4); else if (n_max <= 6) LFR_COV_CL(6); else LFR_COV_CL(kRows);
    } else if constexpr (KC == lfr::KC_G16) {
        if (n_max <= 10) LFR_COV_CL(10); else if (n_max <= 12) LFR_COV_CL(12); else if (n_max <= 14) LFR_COV_CL(14); else LFR_COV_CL(kRows);
    } else if constexpr (KC == lfr::KC_G64_2) {
        if (n_max <= 18) LFR_COV_CL(18); else if (n_max <= 20) LFR_COV_CL(20); else if (n_max <= 22) LFR_COV_CL(22); else LFR_COV_CL(kRows);
    } else {
        static_assert(KC == lfr::KC_G64_4, "one ladder per live class");
        if (n_max <= 20) LFR_COV_CL(20); else if (n_max <= 26) LFR_COV_CL(26); else if (n_max <= 28) LFR_COV_CL(28);
        else if (n_max <= 30) LFR_COV_CL(30); else LFR_COV_CL(kRows);
    }
#undef LFR_COV_CL
}

__device__ __forceinline__ int cov_wave_max(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return __builtin_amdgcn_readfirstlane(v);
}

// ---- a group's LDS ----
template <int NV>
struct alignas(16) CovLds {
    static constexpr int LD = NV + 1;
    double A[NV * LD];         // J^T J (lower triangle)
    double x[NV + 2];          // x^; slots 2*n_var, 2*n_var+1 stay 0 (constants)
};

// Sub-lane sl of a group of S lanes clears the group's matrix and fetches x^ (component d, n_var variable nodes; n_var = 0: all zero).
// The caller syncs the wave's LDS before cov_assemble.
template <int NV, int S, class Args>
__device__ __forceinline__ void cov_lds_init(const Args &a, const lfr::CompDesc &d, const int n_var, const int sl, CovLds<NV> &L) {
    constexpr int LD = NV + 1;
    const int nv2 = 2 * n_var;
    for (int i = sl; i < NV * LD; i += S) L.A[i] = 0.0;
    for (int i = sl; i < NV + 2; i += S) L.x[i] = (i < nv2) ? a.positions[2 * (size_t)a.node_ids[d.node_off + (i >> 1)] + (i & 1)] : 0.0;
}

// One sweep at x^: the forward's evaluation and its assembly (solve_group_body).  Sub-lane sl takes records sl + S * k, k < EPL, of
// the component's E records.  (Args: lfr::KernelArgs, or any block with what load_packed_edge<FUSED> reads and tukey_variant.)
template <int NV, int S, int EPL, bool FUSED, class Args>
__device__ __forceinline__ void cov_assemble(const Args &a, const lfr::CompDesc &d, const int n_var, const int E, const int sl, CovLds<NV> &L) {
    constexpr int LD = NV + 1;
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
        if (!(sl + S * k < E)) continue;
        float flow_k[18]; float sim_k; uint32_t pk;
        load_packed_edge<FUSED>(a, d.edge_off + (sl + S * k), flow_k, sim_k, pk);
        const int es = (int)(pk & 0xffffu), ed = (int)((pk >> 16) & 0x7fffu), ekind = (int)(pk >> 31);
        const int xa = 2 * min(es, n_var), xb = 2 * min(ed, n_var);      // constants read the zero slot
        const int ra = es < n_var ? 2 * es : -1, rb = ed < n_var ? 2 * ed : -1;
        EdgeOut o;
        eval_edge<true>(flow_k, sim_k, ekind, a.tukey_variant, L.x[xa], L.x[xa + 1], L.x[xb], L.x[xb + 1], o);
        double *A = L.A;
        // lane ^ 1 holds the opposite direction of the same match (records 2m, 2m+1): its d r / d x_dst = sq' * I terms land on THIS
        // lane's source block and the two cross blocks coincide - exchanged through DPP, five LDS adds per edge
        const int q = sl & 1;
        const double p_w = dpp_f64<kDppQuadXor1>(o.sq * o.sq);
        const double c_send1 = o.sq * (q ? o.j00 : o.j01), c_send2 = o.sq * (q ? o.j11 : o.j10);
        const double c_own1 = o.sq * (q ? o.j10 : o.j00), c_own2 = o.sq * (q ? o.j01 : o.j11);
        const double c1 = c_own1 + dpp_f64<kDppQuadXor1>(c_send1);
        const double c2 = c_own2 + dpp_f64<kDppQuadXor1>(c_send2);
        if (ra >= 0) {
            atomicAdd(&A[ra * LD + ra], o.j00 * o.j00 + o.j10 * o.j10 + p_w);
            atomicAdd(&A[(ra + 1) * LD + ra], o.j01 * o.j00 + o.j11 * o.j10);
            atomicAdd(&A[(ra + 1) * LD + ra + 1], o.j01 * o.j01 + o.j11 * o.j11 + p_w);
        }
        if (ra >= 0 && rb >= 0) {
            const int r1 = rb + q, k1 = ra, r2 = rb + 1 - q, k2 = ra + 1;
            atomicAdd(&A[rb > ra ? r1 * LD + k1 : k1 * LD + r1], c1);
            atomicAdd(&A[rb > ra ? r2 * LD + k2 : k2 * LD + r2], c2);
        }
    }
}

}  // namespace lfrdev
