// Matrix-free products with the exact Hessian / the loss-corrected Gauss-Newton matrix at given positions (lfr_batch_hessian_product,
// include/lfr.h).  A translation unit of its own: it reads the batch layout (lfr_batch.hpp), the packed record
// loader and the group reductions of lfr_device.hpp and the per-edge arithmetic of the backward's assembly (lfr_hessian_device.hpp:
// bwd_eval, bwd_blocks) through hvp_edge / hvp_apply (lfr_hvp_device.hpp, shared with lfr_hessian_solve.hip), and changes nothing the solve, the backward, the jvp, the covariance or the evaluate read.
//
// Per kept directed edge e = (src -> dst) of a component and per vector v, with M, P of bwd_blocks and c = w rho':
//   t = M (v_dst - P v_src),   (H v)_dst += t,   (H v)_src += -P^T t - c (sum_k r_k d2f_k) v_src     (the last term: exact mode only)
// Two launches in lfr_batch_evaluate's two layouts, both templates on EXACT and on the vector count K: bwd_eval and the blocks are
// formed once per record for all K vectors.
//   packed classes (<= 32 rows)   ONE launch of one-wave workgroups, 64/S components per wave, sub-lane sl takes records sl + S k,
//                                 every record read once.  Positions, the K (masked) vectors and the K products in the group's LDS;
//                                 the products accumulate there as the evaluate's gradient does, lane i stores coordinate i and
//                                 hands v_i (H v)_i to the group's butterfly for the curvature.
//   workgroup classes (above)     one workgroup per component, owner computes: the thread of a variable node sums its two rows over
//                                 the node's out-edges (source side) and in-edges (destination side) in record order.  Constants own
//                                 no row and are skipped.  The curvature is a wave-then-block tree.  No matrix, hence no row limit.
// LFR_HVP_FREE_SET: a coordinate with |x| >= 1 reads as v = 0 in every edge and gets (H v)_i = v_i.
// No fp64 value goes through a global-memory atomic; the arithmetic of one vector does not depend on K or on the other vectors.

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

using namespace lfrdev;
using lfr::CompDesc;
using lfr::EdgeRec;
using lfr::PackedRanges;

namespace {

constexpr int kHvpThreads = 256;               // workgroup classes
constexpr int kHvpMaxVectors = LFR_HVP_MAX_VECTORS;

struct HvpArgs {
    const CompDesc *descs;
    const EdgeRec *edges;
    const uint32_t *node_ids;
    const lfr::NodeInc *node_inc;
    const uint32_t *in_idx;
    const double *positions;   // 2 per node of the whole graph: the caller's or the batch's
    const double *vectors;     // K arrays of `stride` doubles
    double *products;          // K arrays of `stride` doubles (cleared before the launches), or nullptr
    double *curvature;         // K x n_desc, or nullptr
    uint32_t *bad;             // per descriptor: a product entry of the component is not finite (cleared before the launches)
    unsigned long long *n_bound;      // coordinates treated as bound (cleared before the launches)
    size_t stride;             // 2 * n_nodes of the whole graph
    int n_desc, desc_begin, tukey_variant, free_set;
};

// ---- packed classes ----
// per group: positions, K masked vectors, K products, NV coordinates each (constants are selected to 0 by the reader, not by a slot:
// the four-vector instantiation stays below the 5 KiB that let 32 one-wave workgroups share a CU's LDS, as the evaluate's do)
template <int NV, int K>
struct alignas(16) HvpLds {
    double x[NV];
    double v[K][NV];
    double h[K][NV];
};

template <int K>
constexpr size_t hvp_packed_lds_bytes() { return PackedClass<lfr::KC_G8>::G * sizeof(HvpLds<PackedClass<lfr::KC_G8>::NV, K>); }

template <int KC, bool EXACT, int K>
__device__ __forceinline__ void hvp_group_body(const HvpArgs &a, const int desc_begin, const int desc_end, const int block_in_class,
                                               unsigned char *lds_raw) {
    constexpr int NV = PackedClass<KC>::NV, S = PackedClass<KC>::S, EPL = PackedClass<KC>::EPL;
    static_assert(PackedClass<KC>::G * sizeof(HvpLds<NV, K>) <= hvp_packed_lds_bytes<K>(), "LDS budget");
    PackedGroup<KC> grp;
    if (!grp.init(a.descs, desc_begin, desc_end, block_in_class)) return;
    const int sl = grp.sl, ci = grp.ci, n_var = grp.n_var, nv2 = grp.nv2, E = grp.E;
    const bool have = grp.have;
    const CompDesc &d = grp.d;
    HvpLds<NV, K> &L = reinterpret_cast<HvpLds<NV, K> *>(lds_raw)[grp.gid];

    // lane sl owns coordinate sl of the component (NV <= S): it loads it, and stores its product at the end
    const bool own = sl < nv2;
    const size_t gi = own ? 2 * (size_t)a.node_ids[d.node_off + (sl >> 1)] + (sl & 1) : 0;
    const double xi = own ? a.positions[gi] : 0.0;
    const bool bound = a.free_set && own && fabs(xi) >= 1.0;
    double vi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) vi[k] = own ? a.vectors[k * a.stride + gi] : 0.0;
    if (sl < NV) {
        L.x[sl] = xi;
#pragma unroll
        for (int k = 0; k < K; ++k) { L.v[k][sl] = bound ? 0.0 : vi[k]; L.h[k][sl] = 0.0; }
    }
    wave_lds_sync();

#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        const int p = sl + S * j;
        if (!(p < E)) continue;
        float flow_k[18]; float sim_k; uint32_t pk;
        load_packed_edge<false>(a, d.edge_off + p, flow_k, sim_k, pk);
        const int es = (int)(pk & 0xffffu), ed = (int)((pk >> 16) & 0x7fffu), ekind = (int)(pk >> 31);
        const bool sv = es < n_var, dv = ed < n_var;                     // constants: position and vector 0, no row
        const int xa = sv ? 2 * es : 0, xb = dv ? 2 * ed : 0;
        HvpEdge h;
        hvp_edge<EXACT>(flow_k, sim_k, ekind, a.tukey_variant, sv ? L.x[xa] : 0.0, sv ? L.x[xa + 1] : 0.0, dv ? L.x[xb] : 0.0,
                        dv ? L.x[xb + 1] : 0.0, h);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double hs0, hs1, hd0, hd1;
            hvp_apply<EXACT>(h, sv ? L.v[k][xa] : 0.0, sv ? L.v[k][xa + 1] : 0.0, dv ? L.v[k][xb] : 0.0, dv ? L.v[k][xb + 1] : 0.0, hs0, hs1,
                             hd0, hd1);
            if (sv) { atomicAdd(&L.h[k][xa], hs0); atomicAdd(&L.h[k][xa + 1], hs1); }
            if (dv) { atomicAdd(&L.h[k][xb], hd0); atomicAdd(&L.h[k][xb + 1], hd1); }
        }
    }
    wave_lds_sync();
    bool bad = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double hv = own ? (bound ? vi[k] : L.h[k][sl]) : 0.0;
        bad |= !isfinite(hv);
        if (own && a.products) a.products[k * a.stride + gi] = hv;
        const double c = group_sum<S>(hvp_mul(vi[k], hv));     // every lane of the wave is active; the butterfly stays inside the group
        if (have && sl == 0 && a.curvature) a.curvature[(size_t)k * a.n_desc + ci] = c;
    }
    if (bad) a.bad[ci] = 1u;                           // (an owning lane belongs to a component; every writer stores the same word)
    if (bound) atomicAdd(a.n_bound, 1ull);             // (an integer count)
}

// all packed classes in ONE launch, the blocks dealt to the classes as in evaluate_packed_kernel
template <bool EXACT, int K>
__global__ __launch_bounds__(64) void hessian_product_packed_kernel(const HvpArgs a, const PackedRanges r) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[hvp_packed_lds_bytes<K>()];
    packed_dispatch(r, [&](auto kc, int desc_begin, int desc_end, int block_in_class) LFR_INLINE_LAMBDA {
        hvp_group_body<decltype(kc)::value, EXACT, K>(a, desc_begin, desc_end, block_in_class, lds_raw);
    });
}

// ---- workgroup classes ----
template <int T, bool EXACT, int K>
__global__ __launch_bounds__(T) void hessian_product_block_kernel(const HvpArgs a) {
    __shared__ double wave_curv[K][T / 64];
    const int di = a.desc_begin + blockIdx.x, tid = threadIdx.x;
    const CompDesc d = a.descs[di];
    const int nv = d.n_var;
    const uint32_t ne = d.n_edges;
    const uint32_t *ids = a.node_ids + d.node_off;
    auto xof = [&](int m, int c) -> double { return m < nv ? a.positions[2 * (size_t)ids[m] + c] : 0.0; };
    // vector k at coordinate c of local node m whose position there is x: 0 for constants and, on the free set, at a bound
    auto vof = [&](int k, int m, int c, double x) -> double {
        if (m >= nv || (a.free_set && fabs(x) >= 1.0)) return 0.0;
        return a.vectors[k * a.stride + 2 * (size_t)ids[m] + c];
    };
    double curv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) curv[k] = 0.0;
    bool bad = false;
    unsigned n_bound = 0;
    for (int l = tid; l < nv; l += T) {                       // variable nodes only: a constant owns no row
        const lfr::NodeInc ni = a.node_inc[d.node_off + l];
        const size_t gl = 2 * (size_t)ids[l];
        const double xr = a.positions[gl], xc = a.positions[gl + 1];
        const bool b0 = a.free_set && fabs(xr) >= 1.0, b1 = a.free_set && fabs(xc) >= 1.0;
        n_bound += (unsigned)b0 + (unsigned)b1;
        double raw[K][2], vl[K][2], acc[K][2];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            raw[k][0] = a.vectors[k * a.stride + gl]; raw[k][1] = a.vectors[k * a.stride + gl + 1];
            vl[k][0] = b0 ? 0.0 : raw[k][0]; vl[k][1] = b1 ? 0.0 : raw[k][1];
            acc[k][0] = 0.0; acc[k][1] = 0.0;
        }
        for_out_records(ni, ne, [&](const uint32_t p) {       // l -> m: the source side
            float fl[18]; float sm; uint32_t pk;
            load_packed_edge<false>(a, d.edge_off + p, fl, sm, pk);
            const int m = (int)((pk >> 16) & 0x7fffu), kind = (int)(pk >> 31);
            const double yr = xof(m, 0), yc = xof(m, 1);
            HvpEdge h;
            hvp_edge<EXACT>(fl, sm, kind, a.tukey_variant, xr, xc, yr, yc, h);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                double hs0, hs1, hd0, hd1;
                hvp_apply<EXACT>(h, vl[k][0], vl[k][1], vof(k, m, 0, yr), vof(k, m, 1, yc), hs0, hs1, hd0, hd1);
                acc[k][0] += hs0; acc[k][1] += hs1;
            }
        });
        for_in_records(ni, a.in_idx, d.edge_off, ne, [&](const uint32_t p) {      // m -> l: the destination side
            float fl[18]; float sm; uint32_t pk;
            load_packed_edge<false>(a, d.edge_off + p, fl, sm, pk);
            const int m = (int)(pk & 0xffffu), kind = (int)(pk >> 31);
            const double yr = xof(m, 0), yc = xof(m, 1);
            HvpEdge h;
            hvp_edge<EXACT>(fl, sm, kind, a.tukey_variant, yr, yc, xr, xc, h);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                double hs0, hs1, hd0, hd1;
                hvp_apply<EXACT>(h, vof(k, m, 0, yr), vof(k, m, 1, yc), vl[k][0], vl[k][1], hs0, hs1, hd0, hd1);
                acc[k][0] += hd0; acc[k][1] += hd1;
            }
        });
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double h0 = b0 ? raw[k][0] : acc[k][0], h1 = b1 ? raw[k][1] : acc[k][1];
            bad |= !(isfinite(h0) && isfinite(h1));
            if (a.products) { a.products[k * a.stride + gl] = h0; a.products[k * a.stride + gl + 1] = h1; }
            curv[k] += hvp_dot2(raw[k][0], h0, raw[k][1], h1);
        }
    }
    if (bad) a.bad[di] = 1u;
    if (n_bound) atomicAdd(a.n_bound, (unsigned long long)n_bound);      // (an integer count)
    // the curvature: a butterfly inside each wave, then the waves in order
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double c = curv[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
        if ((tid & 63) == 0) wave_curv[k][tid >> 6] = c;
    }
    __syncthreads();
    if (tid < K && a.curvature) {
        double c = wave_curv[tid][0];
#pragma unroll
        for (int w = 1; w < T / 64; ++w) c += wave_curv[tid][w];
        a.curvature[(size_t)tid * a.n_desc + di] = c;
    }
}

template <bool EXACT, int K>
void hvp_launch(const lfr_batch *b, const HvpArgs &a, hipStream_t st) {
    lfr::launch_two_layouts(b, hessian_product_packed_kernel<EXACT, K>, hessian_product_block_kernel<kHvpThreads, EXACT, K>, kHvpThreads, a, st);
}

template <bool EXACT>
void hvp_launch_k(const lfr_batch *b, const HvpArgs &a, int n_vectors, hipStream_t st) {
    static_assert(kHvpMaxVectors == 4, "one instantiation per vector count");
    switch (n_vectors) {
        case 1: hvp_launch<EXACT, 1>(b, a, st); break;
        case 2: hvp_launch<EXACT, 2>(b, a, st); break;
        case 3: hvp_launch<EXACT, 3>(b, a, st); break;
        default: hvp_launch<EXACT, 4>(b, a, st); break;
    }
}

// the shared state of a pass (events, latest stream: lfr_batch.hpp) + the non-finite mark per descriptor and the bound-coordinate
// count.  Set up by pass_setup_unsolved, not by pass_begin: the product needs neither a solve nor unchanged inputs, and no workspace for matrices.
struct HvpState : lfr::PassState {
    uint32_t *d_bad = nullptr;
    unsigned long long *d_bound = nullptr;
    std::vector<uint32_t> h_bad;
};

int hvp_carve(lfr_batch *b, lfr::PassState *ps) {
    HvpState *s = static_cast<HvpState *>(ps);
    s->d_bound = s->slab.take_n<unsigned long long>(1);
    s->d_bad = s->slab.take_n<uint32_t>(std::max<size_t>((size_t)b->n_desc, 1));
    if (!s->d_bound || !s->d_bad) { lfr::set_error("hessian_product slab exhausted"); return LFR_ERR_NOMEM; }
    return LFR_OK;
}
const lfr::PassKind kHessianProduct = {"hessian_product", [] { return static_cast<lfr::PassState *>(new HvpState()); }, hvp_carve};

}  // namespace

extern "C" {

int lfr_batch_hessian_product(lfr_batch *b, const double *positions_device, const double *vectors_device, int n_vectors,
                              double *products_device, double *curvature_device, int flags, void *hip_stream,
                              lfr_hessian_product_stats *stats) {
    // every argument error comes before an output is touched
    if (!b) { lfr::set_error("lfr_batch_hessian_product: no batch"); return LFR_ERR_ARG; }
    constexpr int known = LFR_HVP_GAUSS_NEWTON | LFR_HVP_FREE_SET;
    if (flags & ~known) { lfr::set_error("lfr_batch_hessian_product: unknown flag bits 0x%x", flags & ~known); return LFR_ERR_ARG; }
    if (!products_device && !curvature_device) {
        lfr::set_error("lfr_batch_hessian_product: nothing to compute (both outputs are NULL)"); return LFR_ERR_ARG;
    }
    if (!vectors_device) { lfr::set_error("lfr_batch_hessian_product: no vectors"); return LFR_ERR_ARG; }
    if (n_vectors < 1 || n_vectors > LFR_HVP_MAX_VECTORS) {
        lfr::set_error("lfr_batch_hessian_product: %d vectors, need 1 to %d", n_vectors, LFR_HVP_MAX_VECTORS); return LFR_ERR_ARG;
    }
    if (!positions_device && b->n_solves == 0) {
        lfr::set_error("lfr_batch_hessian_product: the batch has not been solved and no positions are given"); return LFR_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(b->device));
    if (!b->hvp) {
        const int rc = lfr::pass_setup_unsolved(b, &b->hvp, kHessianProduct, 4 * std::max<size_t>((size_t)b->n_desc, 1) + 8 + 4096);
        if (rc != LFR_OK) return rc;
    }
    HvpState &s = *static_cast<HvpState *>(b->hvp);
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t N = (size_t)b->n_graph_nodes, nd = (size_t)b->n_desc;
    { const int rc = lfr::eval_prologue(b, s, st); if (rc != LFR_OK) return rc; }
    // nodes that are not variable in this shard read 0
    if (products_device && N) HIP_TRY(hipMemsetAsync(products_device, 0, (size_t)n_vectors * 2 * N * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(s.d_bad, 0, 4 * std::max<size_t>(nd, 1), st));
    HIP_TRY(hipMemsetAsync(s.d_bound, 0, 8, st));

    HvpArgs a;
    memset(&a, 0, sizeof(a));
    a.descs = b->d_descs; a.edges = b->d_edges; a.node_ids = b->d_node_ids; a.node_inc = b->d_node_inc; a.in_idx = b->d_in_idx;
    a.positions = positions_device ? positions_device : b->d_positions;
    a.vectors = vectors_device; a.products = products_device; a.curvature = curvature_device;
    a.bad = s.d_bad; a.n_bound = s.d_bound;
    a.stride = 2 * N; a.n_desc = b->n_desc; a.tukey_variant = b->tukey_variant; a.free_set = (flags & LFR_HVP_FREE_SET) ? 1 : 0;
    if (flags & LFR_HVP_GAUSS_NEWTON) hvp_launch_k<false>(b, a, n_vectors, st);
    else hvp_launch_k<true>(b, a, n_vectors, st);
    HIP_TRY(hipGetLastError());
    { const int rc = lfr::pass_end(&s, st); if (rc != LFR_OK) return rc; }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        s.h_bad.assign(nd, 0u);
        unsigned long long n_bound = 0;
        if (nd) HIP_TRY(hipMemcpyAsync(s.h_bad.data(), s.d_bad, 4 * nd, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&n_bound, s.d_bound, 8, hipMemcpyDeviceToHost, st));
        { const int rc = lfr::pass_wait_ms(&s, st, &stats->kernel_ms); if (rc != LFR_OK) return rc; }
        for (const uint32_t v : s.h_bad) stats->n_nonfinite += v != 0;
        stats->n_components = b->n_desc;
        stats->n_bound_coordinates = (int64_t)n_bound;
    }
    return LFR_OK;
}

}  // extern "C"
