// The frame that the packed kernels of the analysis passes share (evaluate, evaluate_vjp, hessian_product, jvp, backward, covariance,
// covariance_matches): the traits of a packed class, the dispatcher of the one launch that hosts all of them, and the identity of a
// group of lanes inside its wave.  Everything a pass computes stays in its own unit.  The numbers come from ONE table, kPackedClass of
// lfr_internal.hpp, which classify() and classify_dev() read too.
// The forward kernel (lfr_solve.hip: solve_packed_kernel, launch_group_class, solve_geometry, the debug launch) takes every number
// from the same table through PackedClass<KC>.  It does not use packed_dispatch: its chain over the blocks' ranges is written out in
// the kernel, indexed by kPackedOrder, because the compiler emits other instructions for it through the dispatcher's lambda.
// Also here: the two guarded record walks of the workgroup layout (a node's out-edges and in-edges).
#pragma once

#include <type_traits>

#include "lfr_batch.hpp"

namespace lfrdev {

// ---- a packed class as compile-time constants, keyed by the KC_* enum ----
template <int KC>
struct PackedClass {
    static_assert(KC >= 0 && KC < lfr::kPackedClasses && !lfr::kPackedClass[KC].retired, "a live packed class");
    static constexpr int NV = lfr::kPackedClass[KC].NV, LPR = lfr::kPackedClass[KC].LPR, EPL = lfr::kPackedClass[KC].EPL;
    static constexpr int S = NV * LPR, G = 64 / S;
    static constexpr int max_rows = lfr::kPackedClass[KC].max_rows, max_edges = lfr::kPackedClass[KC].max_edges;
};

// ---- the one launch of all packed classes: block blockIdx.x belongs to class kPackedOrder[i] when it lies in
// [r.blk_begin[i], r.blk_begin[i + 1]).  f(class as std::integral_constant, desc_begin, desc_end, block_in_class): a lambda marked
// LFR_INLINE_LAMBDA, so that the group body stays part of the kernel's own code ----
#define LFR_INLINE_LAMBDA __attribute__((always_inline))
template <int I, class F>
__device__ __forceinline__ void packed_dispatch_to(const lfr::PackedRanges &r, const int b, F &&f) {
    constexpr int KC = lfr::kPackedOrder[I];
    if constexpr (!lfr::kPackedClass[KC].retired) f(std::integral_constant<int, KC>{}, r.desc_begin[I], r.desc_end[I], b - r.blk_begin[I]);
    /* else: retired class, never assigned */
}
template <class F>
__device__ __forceinline__ void packed_dispatch(const lfr::PackedRanges &r, F &&f) {
    static_assert(lfr::kPackedClasses == 5, "one branch per class");
    const int b = (int)blockIdx.x;
    if (b < r.blk_begin[1]) packed_dispatch_to<0>(r, b, f);
    else if (b < r.blk_begin[2]) packed_dispatch_to<1>(r, b, f);
    else if (b < r.blk_begin[3]) packed_dispatch_to<2>(r, b, f);
    else if (b < r.blk_begin[4]) packed_dispatch_to<3>(r, b, f);
    else packed_dispatch_to<4>(r, b, f);
}

// ---- the group identity: lane -> group gid of its wave and sub-lane sl, the group's component ci and its descriptor.  n_var and E
// are clamped to what the group's LDS and lane slots hold (>= the class limits: packed_table_ok), so every LDS index stays inside
// the group whatever the descriptor says; for every batch the library builds they are the descriptor's own. ----
template <int KC>
struct PackedGroup {
    using P = PackedClass<KC>;
    int lane, gid, sl, ci;
    bool have;                 // this group has a component (the last wave of a class may be partly empty)
    lfr::CompDesc d;           // zeroed unless `have`
    int n_var, nv2, E;         // variable nodes, matrix rows, records

    // false (wave-uniform): the wave has no component at all and the body returns at once
    __device__ __forceinline__ bool init(const lfr::CompDesc *descs, const int desc_begin, const int desc_end, const int block_in_class) {
        lane = threadIdx.x & 63;
        gid = lane / P::S; sl = lane % P::S;
        const int ci0 = desc_begin + block_in_class * P::G;
        if (ci0 >= desc_end) return false;
        ci = ci0 + gid;
        have = ci < desc_end;
        d.edge_off = 0; d.n_edges = 0; d.node_off = 0; d.n_nodes = 0; d.n_var = 0;
        if (have) d = descs[ci];
        n_var = min((int)d.n_var, P::NV / 2); nv2 = 2 * n_var;
        E = min((int)d.n_edges, P::max_edges);
        return true;
    }
};

// ---- workgroup layout: the records of local node `ni` in record order, f(p) with p the component-local record index.  The guards
// cannot fire (a run lies inside its component, in_idx holds record indices of the component); they keep a damaged incidence from
// reading outside the component's ne records. ----
template <class F>
__device__ __forceinline__ void for_out_records(const lfr::NodeInc &ni, const uint32_t ne, F &&f) {
    for (uint32_t k = 0; k < ni.out_count; ++k) {
        const uint32_t p = ni.out_begin + k;
        if (p >= ne) break;
        f(p);
    }
}
// in_idx: the batch's array; edge_off: the component's first record
template <class F>
__device__ __forceinline__ void for_in_records(const lfr::NodeInc &ni, const uint32_t *in_idx, const uint32_t edge_off, const uint32_t ne, F &&f) {
    for (uint32_t k = 0; k < ni.in_count; ++k) {
        if (ni.in_begin + k >= ne) break;
        const uint32_t p = in_idx[edge_off + ni.in_begin + k];
        if (p >= ne) break;
        f(p);
    }
}

}  // namespace lfrdev
