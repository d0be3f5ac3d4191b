// Device-side graph stage: tracks (solve.cc:489-549), roots (solve.cc:552-582) and components
// (solve.cc:252-308) on the GPU, bit-identical to the host stage of lfr_graph.cpp; plus the device copies of
// the match graph (DevGraph) and of the labels (DevProblem) that the batch assembly continues from.
//
// The constrained maximum spanning forest is greedy over the globally sorted match list, i.e.
// order dependent — but only INSIDE a connected component of the match graph: two matches of
// different connected components never interact.  So (hard part 4):
//   1. plain connected components of the match graph, ignoring image conflicts (lock-free union-find)
//   2. ONE radix sort (rocPRIM) by (connected component, similarity descending), then the runs of equal similarities inside a
//      component put into the reference's (n1, n2) descending order in place (k_tie_fix).  Only when such a run is longer than
//      kMaxTieRun: the round-3 scheme, radix sorts by n2, by (similarity, n1) and - stable - by connected component.
//   3. (the segments of that list = the connected components)
//   4. small connected components: one thread each replays the reference's sequential union-find with the
//      image-conflict test over its own matches, in order.  Large ones (real match graphs are typically ONE
//      giant connected component: wrong matches link the tracks) run the same greedy rule in parallel ROUNDS:
//      a match whose two roots are equal or share an image can be retired at once (sets only grow, so the verdict
//      can never change); of the others, a match is accepted in this round iff no earlier pending match touches
//      either of its roots - such matches have pairwise disjoint roots and commute with everything before them,
//      so every union happens with exactly the operands it has in the sequential order (same roots, same sizes,
//      same tie rule).  Image sets are per-root bitsets (#images bits).
//   5. track ids = rank of the root nodes; roots = arg-max (score, node) per track; components =
//      connected components of the track meta-graph, numbered by their smallest track - these ARE the connected components of
//      step 1 (k_cc_min_track), a second union-find only runs after a cut (k_meta_union_cut).
// The whole chain is enqueued on ONE stream without host round trips: counts that size later steps
// (segments, tracks, components) stay on the device and bound the kernels there; every array is sized
// by its upper bound (N or M).  One 64-byte read-back at the end delivers the counts for the stdout lines
// (a second one, mid-way, tells whether large connected components exist and whether a long tie asks for the three sorts).  A component above the size cap
// needs the graph cut: the sequential priority-queue bisection stays on the host, fed with the device's tracks
// (lfr_graph.cpp: cut_components_from_pairs, the same recursive_cut as the host stage's components_from_tracks), and the labels go back to HBM.
// Integer work throughout; the only floating-point accumulation (root scores, sums of float32
// similarities in fp64) is exact for any realistic input, hence order independent.
#include <hip/hip_runtime.h>
#include <type_traits>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lfr_assemble.hpp"

namespace lfr {

namespace {

constexpr int kThreads = kPipeThreads;
constexpr int64_t kSerialSegmentEdges = 2048;     // connected components up to this many matches: one thread each
                                                   // (LFR_SERIAL_SEGMENT_EDGES overrides it: tests push everything through the rounds)
constexpr int kMaxTieRun = 64;                     // runs of equal similarities inside a connected component up to this long are ordered in place (k_tie_fix)
constexpr int kMaxRounds = 100000;                 // larger ones: parallel rounds (a path-shaped dependency chain this long: host stage)
constexpr size_t kMaxBitsetBytes = (size_t)24 << 30;
inline dim3 grid_for(int64_t n) { return pipe_grid(n); }

struct ArenaMark {                                 // temporaries: released at scope end (reuse is stream ordered)
    DevArena &a; size_t m;
    explicit ArenaMark(DevArena &ar) : a(ar), m(ar.top) {}
    ~ArenaMark() { a.top = m; }
};

template <class K, class V>
int sort_pairs(DevArena &arena, const K *kin, K *kout, const V *vin, V *vout, int64_t n, int begin_bit, int end_bit, hipStream_t st) {
    if (n <= 0) return LFR_OK;
    size_t bytes = 0;
    LFR_HIP_TRY(sort_pairs_raw(nullptr, bytes, kin, kout, vin, vout, n, begin_bit, end_bit, st));
    ArenaMark mark(arena);
    void *tmp = arena.take(bytes);
    if (!tmp) { set_error("graph stage: device arena exhausted (sort of %lld items)", (long long)n); return LFR_ERR_NOMEM; }
    LFR_HIP_TRY(sort_pairs_raw(tmp, bytes, kin, kout, vin, vout, n, begin_bit, end_bit, st));
    return LFR_OK;
}
// sums of the values of equal adjacent keys (rocPRIM reduce_by_key); *n_runs (device) = number of distinct runs
int sum_by_key(DevArena &arena, const unsigned long long *keys, unsigned long long *unique, const double *vals, double *sums, uint32_t *n_runs,
               int64_t n, hipStream_t st) {
    size_t bytes = 0;
    LFR_HIP_TRY(rocprim::reduce_by_key(nullptr, bytes, keys, vals, (size_t)n, unique, sums, n_runs, rocprim::plus<double>(), rocprim::equal_to<unsigned long long>(), st));
    void *tmp = arena.take(bytes);
    if (!tmp) { set_error("graph stage: device arena exhausted (reduce-by-key)"); return LFR_ERR_NOMEM; }
    LFR_HIP_TRY(rocprim::reduce_by_key(tmp, bytes, keys, vals, (size_t)n, unique, sums, n_runs, rocprim::plus<double>(), rocprim::equal_to<unsigned long long>(), st));
    return LFR_OK;
}

int exclusive_sum(DevArena &arena, const uint32_t *in, uint32_t *out, int64_t n, hipStream_t st) {
    if (n <= 0) return LFR_OK;
    size_t bytes = 0;
    LFR_HIP_TRY(rocprim::exclusive_scan(nullptr, bytes, in, out, std::remove_cv_t<std::remove_reference_t<decltype(*out)>>(0), (size_t)n, rocprim::plus<std::remove_cv_t<std::remove_reference_t<decltype(*out)>>>(), st));
    ArenaMark mark(arena);
    void *tmp = arena.take(bytes);
    if (!tmp) { set_error("graph stage: device arena exhausted (scan of %lld items)", (long long)n); return LFR_ERR_NOMEM; }
    LFR_HIP_TRY(rocprim::exclusive_scan(tmp, bytes, in, out, std::remove_cv_t<std::remove_reference_t<decltype(*out)>>(0), (size_t)n, rocprim::plus<std::remove_cv_t<std::remove_reference_t<decltype(*out)>>>(), st));
    return LFR_OK;
}

__device__ __forceinline__ uint32_t sim_key(float s) {       // order-preserving float -> uint32
    if (s == 0.f) s = 0.f;                                    // -0.0 == +0.0
    const uint32_t b = __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sim_from_key(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// descending order of (sim, n1, n2) == ascending order of the complemented keys; node ids are complemented inside
// their node_bits bits (N-1-n) so that the radix sorts run over 32 + 2 x node_bits key bits instead of 96
__global__ void k_match_keys(int64_t M, uint32_t n_minus_1, int node_bits, const uint32_t *n1, const uint32_t *n2, const float *sim,
                             uint64_t *k_hi, uint32_t *k_lo, uint32_t *ids) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    k_hi[m] = ((uint64_t)(~sim_key(sim[m])) << node_bits) | (uint64_t)(n_minus_1 - n1[m]);
    k_lo[m] = n_minus_1 - n2[m];
    ids[m] = (uint32_t)m;
}
// The usual case needs ONE sort: connected components are known before any order is (the union-find of step 2 does not read one), so
// the key (component | ~similarity) groups and orders the matches in seven radix passes; the thirteen passes of the three-sort
// scheme above (n2, then (sim, n1), then the component, each stable) only break ties between EQUAL similarities inside a component, and
// k_tie_fix does that in place for the short runs real similarities produce.
__global__ void k_cc_sim_keys(int64_t M, const uint32_t *n1, const float *sim, const uint32_t *cc, uint64_t *key, uint32_t *ids) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    key[m] = ((uint64_t)cc[n1[m]] << 32) | (uint64_t)(~sim_key(sim[m]));
    ids[m] = (uint32_t)m;
}
// Round 6: the usual case needs no 52-bit sort either.  Real match graphs fall into small connected components (config 4: 147 k of
// 6..136 matches) - or into one giant one, which keeps the sort above.  The matches are grouped by component with a sort over the
// component bits alone (two 10-bit passes instead of six 9-bit ones over 64-bit keys), and inside a component every match finds its
// place by COUNTING the matches that precede it in the reference's order (descending (sim, n1, n2), equal triples by match id): the
// comparison is the full one, so there are no ties to repair and no long-tie fallback.  A workgroup stages the records of the segments
// that touch its 256 positions in LDS (16 B per match: ~sim key, n1, n2, id), so a record is gathered about once.
constexpr int kRankSortMax = 1024;                   // longest segment the counting handles (LDS window: 256 + 2 x longest records, 36 KB at most)
__global__ void k_match_records(int64_t M, const uint32_t *n1, const uint32_t *n2, const float *sim, const uint32_t *cc, uint4 *rec, uint32_t *key, uint32_t *ids) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const uint32_t a = n1[m];
    rec[m] = make_uint4(~sim_key(sim[m]), a, n2[m], (uint32_t)m);
    key[m] = cc[a];
    ids[m] = (uint32_t)m;
}
__device__ __forceinline__ bool rank_precedes(const uint4 &q, const uint4 &me) {          // q comes before me in the reference's order
    return q.x < me.x || (q.x == me.x && (q.y > me.y || (q.y == me.y && (q.z > me.z || (q.z == me.z && q.w < me.w)))));
}
__global__ __launch_bounds__(kThreads) void k_rank_sort(int64_t M, const uint32_t *grouped, const uint4 *rec, const uint32_t *flags, const uint32_t *seg_id,
                                                        const uint32_t *starts, uint32_t *order, uint4 *sorted) {
    extern __shared__ uint4 s_rec[];                  // kThreads + 2 x (longest segment) records: the host knows the longest segment by now
    const int64_t b0 = (int64_t)blockIdx.x * kThreads;
    if (b0 >= M) return;
    const int64_t b1 = b0 + kThreads < M ? b0 + kThreads : M;
    const int64_t w_lo = starts[seg_id[b0] + flags[b0] - 1u], w_hi = starts[seg_id[b1 - 1] + flags[b1 - 1]];     // the segments that touch [b0, b1)
    for (int64_t j = w_lo + threadIdx.x; j < w_hi; j += kThreads) s_rec[j - w_lo] = rec[grouped[j]];
    __syncthreads();
    const int64_t i = b0 + threadIdx.x;
    if (i >= M) return;
    const uint32_t sg = seg_id[i] + flags[i] - 1u;
    const int64_t lo = starts[sg], hi = starts[sg + 1];
    const uint4 me = s_rec[i - w_lo];
    uint32_t rank = 0;
    for (int64_t j = lo; j < hi; ++j) rank += rank_precedes(s_rec[j - w_lo], me) ? 1u : 0u;
    order[lo + rank] = me.w;
    sorted[lo + rank] = me;                           // the record itself in the reference's order: k_kruskal_stream and k_scores_grouped read their matches as this stream
}
__global__ void k_gather_u64(int64_t n, const uint32_t *idx, const uint64_t *src, uint64_t *dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}
__global__ void k_iota(int64_t n, uint32_t *p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (uint32_t)i;
}

// ---- lock-free union-find (hook the larger root under the smaller): labels = smallest member ----
// The walks of a find read parent[] with WORKGROUP-scope atomic loads: they may be served from the CU's vector L1, i.e. be stale.  Sound:
// every value parent[x] ever held is an ancestor of x (or x itself) and, if not x, smaller than x, so a stale walk ends at an ancestor, and
// what decides a union is the agent-scope CAS - on a node that is no root any more it fails and hands back the current parent, from which
// uf_union continues (strictly smaller: it terminates); on a true root `a` with a stale, former root `b` < a it hooks a under a member of
// b's tree, which still joins the two trees, still points downwards, and leaves the root the smallest member.  Why not agent scope
// everywhere: in a giant connected component every find ends at the same root, and a single L2 channel serves ~2 G requests/s - the
// finds of config 5's 5.3 M matches queued on that one word (k_cc_union: 1.4 ms; the stages below and the gated halving of uf_find are the rest of that story).
__device__ __forceinline__ uint32_t uf_load(const uint32_t *parent, uint32_t x) {
    return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
constexpr int kHalveAfterHops = 3;
__device__ __forceinline__ uint32_t uf_load_near(const uint32_t *parent, uint32_t x) {
    return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
    uint32_t p = uf_load_near(parent, x);
    int hops = 0;
    while (p != x) {
        // path halving, but only on walks that turn out long: thousands of threads see the same short stale path below a hot root, and
        // their (agent-scope) halving stores of the same words queued at the L2 - config 5: 1.0-1.6 ms with them, 0.15 without
        const uint32_t gp = uf_load_near(parent, p);
        if (gp != p && ++hops > kHalveAfterHops) __hip_atomic_store(&parent[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p; p = gp;
    }
    return x;
}
__device__ __forceinline__ void uf_union(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(parent, a); b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }      // a > b: hook a under b
        const uint32_t seen = atomicCAS(&parent[a], a, b);
        if (seen == a) return;
        a = seen;                                               // a was hooked meanwhile: continue from its new parent
    }
}
// Real match graphs are ONE giant connected component: millions of unions then meet at a handful of roots.  So the unions run in
// stages (the sampling idea of Afforest, Sutton et al. 2018): every 32nd match first, then every 4th, then the rest, the parents
// flattened in between (k_uf_flatten).  The giant component forms in a stage with few threads, and from the second stage on a match
// whose ends already show the same parent is skipped without touching an atomic.  That test reads parent[] with plain loads: any
// value parent[x] ever held is an ancestor of x in the final forest (a root is hooked under another root, a halving store writes a
// grandparent, the flattening writes the root), so equal parents - however stale - prove that the ends are connected; unequal ones fall
// through to the lock-free union.  The labels (smallest member) do not depend on the schedule.  Config 5 (5.3 M matches, one giant
// component): 1.4 ms as one pass with agent-scope walks, 0.15 ms now; config 4 (147 k small components): 0.14 ms either way.
constexpr int kUnionStages = 3;
constexpr int kUnionStrides[kUnionStages] = {32, 4, 1};
__device__ __forceinline__ bool uf_connected_hint(const uint32_t *parent, uint32_t a, uint32_t b) { return parent[a] == parent[b]; }
__global__ void k_uf_flatten(int64_t n, uint32_t *parent) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x = (uint32_t)i, p = uf_load(parent, x);
    if (p == x) return;
    while (p != x) { x = p; p = uf_load(parent, x); }
    __hip_atomic_store(&parent[i], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // (a walker through i sees the old ancestor or the root)
}
// one stage: the matches 0, stride, 2 stride, ... except those an earlier stage (multiples of done_stride, 0 = none) has united already
__global__ void k_cc_union(int64_t M, int stride, int done_stride, const uint32_t *n1, const uint32_t *n2, uint32_t *parent) {
    const int64_t m = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * stride;
    if (m >= M || (done_stride && m % done_stride == 0)) return;
    const uint32_t a = n1[m], b = n2[m];
    if (done_stride && uf_connected_hint(parent, a, b)) return;
    uf_union(parent, a, b);
}
// Labels = roots, written to a SEPARATE array by a read-only walk.  (Flattening in place - parent[i] = find(i) with
// path halving - is wrong under concurrency: another thread's halving store, computed from an older read of
// parent[i], can land after the flattened value and leave an intermediate ancestor there; a giant connected
// component then appears split into two labels.)
__global__ void k_cc_labels(int64_t n, const uint32_t *parent, uint32_t *label) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x = (uint32_t)i, p = uf_load(parent, x);
    while (p != x) { x = p; p = uf_load(parent, x); }
    label[i] = x;
}
__global__ void k_cc_keys(int64_t M, const uint32_t *order, const uint32_t *n1, const uint32_t *cc, uint32_t *keys) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M) keys[i] = cc[n1[order[i]]];
}
__global__ void k_seg_flags(int64_t M, const uint32_t *keys, uint32_t *flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M) flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}
__global__ void k_seg_flags_hi(int64_t M, const uint64_t *keys, uint32_t *flags) {                // (component | ~similarity) keys
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M) flags[i] = (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32)) ? 1u : 0u;
}
// counts[] layout (device): what the host reads back at the end of the stage.  The host's pinned copy is longer and has two more uses
// between read-backs: the cut's two counters in words no kernel writes, and the counters of a batch of union-find rounds behind the block.
enum { CNT_SEG = 0, CNT_TRACKS, CNT_COMPS, CNT_MAX_TRACK, CNT_MAX_COMP, CNT_MAX_SEG, CNT_LONG_TIE, CNT_WORDS = 16,
       CNT_HOST_CUT_EDGES = 8, CNT_HOST_CUT_PAIRS = 9, CNT_HOST_ROUNDS = CNT_WORDS, CNT_HOST_WORDS = CNT_WORDS + 16 };
// Runs of equal (component, similarity) in the one-sort order: the reference's order inside a run is descending (n1, n2) (solve.cc:489,
// std::sort + reverse of (sim, n1, n2) tuples; equal triples are the same union whichever comes first - match id ascending, as the
// stable three-sort scheme leaves them).  The head of a run sorts it by insertion; a run above max_run (quantized similarities in a
// giant component) sets CNT_LONG_TIE and the host orders the list with the three sorts instead.
__global__ void k_tie_fix(int64_t M, const uint64_t *key, uint32_t *order, const uint32_t *n1, const uint32_t *n2, int max_run, uint32_t *counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const uint64_t k = key[i];
    if ((i > 0 && key[i - 1] == k) || i + 1 >= M || key[i + 1] != k) return;      // inside a run / a run of one
    int64_t j = i + 2;
    while (j < M && j - i <= max_run && key[j] == k) ++j;
    if (j - i > max_run) { counts[CNT_LONG_TIE] = 1u; return; }
    for (int64_t a = i + 1; a < j; ++a) {
        const uint32_t m = order[a], m1 = n1[m], m2 = n2[m];
        int64_t b = a;
        while (b > i) {
            const uint32_t q = order[b - 1], q1 = n1[q], q2 = n2[q];
            if (q1 > m1 || (q1 == m1 && (q2 > m2 || (q2 == m2 && q < m)))) break;  // q stays in front of m
            order[b] = q; --b;
        }
        order[b] = m;
    }
}
// seg_id[i] = exclusive count of flags; seg_id[M] = number of segments
__global__ void k_seg_starts(int64_t M, const uint32_t *flags, const uint32_t *seg_id, uint32_t *starts, uint32_t *counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M && flags[i]) starts[seg_id[i]] = (uint32_t)i;
    if (i == 0) { starts[seg_id[M]] = (uint32_t)M; counts[CNT_SEG] = seg_id[M]; }
}
// A maximum into ONE word: atomics on one address take their turns at the L2 (14 k waves, one atomic each, were 28 us of a 5-us kernel;
// looking first with an agent-scope load made it 44), so these kernels run as a few hundred workgroups that stride over the items and
// send one maximum each.
constexpr int kFewBlocks = 512;
inline dim3 grid_few(int64_t n) { const dim3 g = grid_for(n); return dim3(g.x < (unsigned)kFewBlocks ? g.x : (unsigned)kFewBlocks); }
__device__ __forceinline__ void block_atomic_max(uint32_t v, uint32_t *dst) {          // every thread of the workgroup calls it
    __shared__ uint32_t s_max[kThreads / 64];
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kThreads / 64; ++i) v = max(v, s_max[i]);
        if (v) atomicMax(dst, v);
    }
}
__global__ void k_seg_maxlen(int64_t cap, const uint32_t *starts, uint32_t *counts) {
    const int64_t n = cap < (int64_t)counts[CNT_SEG] ? cap : (int64_t)counts[CNT_SEG];
    uint32_t v = 0;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) v = max(v, starts[s + 1] - starts[s]);
    block_atomic_max(v, &counts[CNT_MAX_SEG]);
}

// ---- the reference's greedy constrained union-find, one thread per connected component ----
// parent: -1 = root (solve.cc:492); lists of member nodes replace images_in_track (every member has
// a distinct image, so |images_in_track[root]| == count[root]).
// Image sets as 128-bit signatures (one hashed bit per image, OR-ed on union): two roots whose signatures do not intersect share no
// image, so the exact test - a walk over both member lists, the bulk of this kernel's dependent loads - only runs when the signatures
// collide (config 4: ~6-node tracks in 1344 images, a few per cent of the unions).
__device__ __forceinline__ ulonglong2 image_signature(int32_t im) {
    const uint32_t h = (uint32_t)im * 0x9E3779B1u;
    const uint32_t b = h >> 25;                               // 7 bits
    ulonglong2 m;
    m.x = b < 64u ? 1ull << b : 0ull;
    m.y = b < 64u ? 0ull : 1ull << (b - 64u);
    return m;
}
// One thread replays its component's matches in order; what it waits for is memory - 2-3 waves per SIMD, every access a miss of the CU's
// L1, and each match used to be a chain of ~8 dependent loads (order -> ends -> one root -> the other -> signatures -> counts -> tail).  So
// the loads that do not depend on each other go out together: the next matches' ends two iterations ahead, the two walks to the roots hop
// for hop, everything the union reads from its two roots at once.  Three trips per match instead of eight: 0.42 -> 0.28 ms on config 4
// (an LDS copy of the segment and a records pre-pass had not paid - the chain, not the gathers, was the time; guessing the root one trip
// early does not pay either: what is left is the lockstep of 64 components of different lengths per wave).
__device__ __forceinline__ void kruskal_segment(const int64_t lo, const int64_t hi, const uint32_t *order, const uint32_t *n1,
                                                const uint32_t *n2, const int32_t *node_image, int32_t *parent, int32_t *next, int32_t *tail,
                                                int32_t *count, ulonglong2 *sig) {
    uint32_t m1 = order[lo], m2 = lo + 1 < hi ? order[lo + 1] : 0u;           // matches k and k + 1
    uint32_t a1 = n1[m1], b1 = n2[m1];
    for (int64_t k = lo; k < hi; ++k) {
        const int32_t a = (int32_t)a1, b = (int32_t)b1;
        if (k + 1 < hi) { a1 = n1[m2]; b1 = n2[m2]; }         // the ends of match k + 1, the id of match k + 2: in flight during this union
        if (k + 2 < hi) m2 = order[k + 2];
        int32_t r1 = a, r2 = b, p1 = parent[a], p2 = parent[b];
        while (p1 >= 0 || p2 >= 0) {                          // (either walk has a hop left)
            const bool h1 = p1 >= 0, h2 = p2 >= 0;
            if (h1) r1 = p1;
            if (h2) r2 = p2;
            const int32_t q1 = h1 ? parent[r1] : -1, q2 = h2 ? parent[r2] : -1;
            p1 = q1; p2 = q2;
        }
        if (r1 != a) parent[a] = r1;                          // (compression of the two starting nodes: sizes decide the unions, not the paths)
        if (r2 != b) parent[b] = r2;
        if (r1 == r2) continue;
        const ulonglong2 s1 = sig[r1], s2 = sig[r2];
        const int32_t c1 = count[r1], c2 = count[r2], t1 = tail[r1], t2 = tail[r2];
        bool conflict = false;                               // solve.cc:506-511
        if ((s1.x & s2.x) | (s1.y & s2.y)) {                 // the signatures collide: the exact test
            for (int32_t i = r1; i >= 0 && !conflict; i = next[i]) {
                const int32_t im = node_image[i];
                for (int32_t j = r2; j >= 0; j = next[j]) if (node_image[j] == im) { conflict = true; break; }
            }
        }
        if (conflict) continue;
        const bool swap = c1 < c2;                           // solve.cc:513-521 (ties: root2 under root1)
        const int32_t big = swap ? r2 : r1, small = swap ? r1 : r2;
        parent[small] = big;
        next[swap ? t2 : t1] = small; tail[big] = swap ? t1 : t2; count[big] = c1 + c2;
        sig[big] = make_ulonglong2(s1.x | s2.x, s1.y | s2.y);
    }
}
__global__ void k_kruskal(int64_t cap, int64_t serial_limit, const uint32_t *counts, const uint32_t *starts, const uint32_t *order, const uint32_t *n1,
                          const uint32_t *n2, const int32_t *node_image, int32_t *parent, int32_t *next, int32_t *tail,
                          int32_t *count, ulonglong2 *sig) {
    // (Round 6, measured and dropped: dealing the segments to the threads BY LENGTH.  In the order they come in, config 4's 147 k components
    // of 6..136 matches keep a wave busy 3.3 times the mean length; dealt by length over the whole list the factor is 1.00 and the kernel
    // ran 613 us instead of 288, dealt inside a workgroup of 256 / 512 / 1024 threads through LDS 324 / 329 / 375 us.  Neighbouring
    // threads replaying neighbouring components - one stretch of the ordered list, nodes numbered close together - is worth more than
    // equal lengths: the kernel is bound by memory transactions, not by its longest lane.  profiles/r06_ab/kruskal_by_length.txt)
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap || s >= (int64_t)counts[CNT_SEG]) return;
    const int64_t lo = starts[s], hi = starts[s + 1];
    if (hi - lo > serial_limit) return;                      // large connected component: parallel rounds (k_round_*)
    kruskal_segment(lo, hi, order, n1, n2, node_image, parent, next, tail, count, sig);
}
// The same rule fed by the stream of sorted records (round 6, counting road: k_rank_sort writes every record to its place in the
// reference's order, 16 bytes per match): no id from `order`, no gathered ends - two of the dozen scattered 32-byte sectors a match
// costs the kernel above.  Config 4: 284 -> 206 us, k_rank_sort + 4 us for the records.  Measured against it and dropped: the component's
// whole state in LDS under local node numbers (one thread per component, [slot][thread] columns, images and parents out once per
// node): 363 us - a wave's lanes diverge in every inner loop (look-up among the known ids, root walks, the image test), so every match
// costs the longest path of 64 components, where the scattered version hides its latency behind 32 waves per CU
// (profiles/r06_ab/kruskal_variants.txt).
__global__ void k_kruskal_stream(int64_t cap, int64_t serial_limit, const uint32_t *counts, const uint32_t *starts, const uint4 *sorted,
                                 const int32_t *node_image, int32_t *parent, int32_t *next, int32_t *tail, int32_t *count, ulonglong2 *sig) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap || s >= (int64_t)counts[CNT_SEG]) return;
    const int64_t lo = starts[s], hi = starts[s + 1];
    if (hi - lo > serial_limit) return;
    uint4 q = sorted[lo];
    for (int64_t k = lo; k < hi; ++k) {
        const int32_t a = (int32_t)q.y, b = (int32_t)q.z;
        if (k + 1 < hi) q = sorted[k + 1];
        int32_t r1 = a, r2 = b, p1 = parent[a], p2 = parent[b];
        while (p1 >= 0 || p2 >= 0) {
            const bool h1 = p1 >= 0, h2 = p2 >= 0;
            if (h1) r1 = p1;
            if (h2) r2 = p2;
            const int32_t q1 = h1 ? parent[r1] : -1, q2 = h2 ? parent[r2] : -1;
            p1 = q1; p2 = q2;
        }
        if (r1 != a) parent[a] = r1;
        if (r2 != b) parent[b] = r2;
        if (r1 == r2) continue;
        const ulonglong2 s1 = sig[r1], s2 = sig[r2];
        const int32_t c1 = count[r1], c2 = count[r2], t1 = tail[r1], t2 = tail[r2];
        bool conflict = false;
        if ((s1.x & s2.x) | (s1.y & s2.y)) {
            for (int32_t i = r1; i >= 0 && !conflict; i = next[i]) {
                const int32_t im = node_image[i];
                for (int32_t j = r2; j >= 0; j = next[j]) if (node_image[j] == im) { conflict = true; break; }
            }
        }
        if (conflict) continue;
        const bool swap = c1 < c2;
        const int32_t big = swap ? r2 : r1, small = swap ? r1 : r2;
        parent[small] = big;
        next[swap ? t2 : t1] = small; tail[big] = swap ? t1 : t2; count[big] = c1 + c2;
        sig[big] = make_ulonglong2(s1.x | s2.x, s1.y | s2.y);
    }
}
// parent[] is shared with k_kruskal (-1 = root).  Finds compress by halving; within the evaluation kernel no union
// happens, so a stale pointer is still an ancestor.
__device__ __forceinline__ int32_t par_load(const int32_t *parent, int32_t x) {
    return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t par_find(int32_t *parent, int32_t x) {
    for (;;) {
        const int32_t p = par_load(parent, x);
        if (p < 0) return x;
        const int32_t gp = par_load(parent, p);
        if (gp >= 0) __hip_atomic_store(&parent[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
    }
}
// append to a list with one atomic per WORKGROUP, ITEMS candidates per thread: a returning atomic on one address costs ~10 ns at the L2 whoever
// sends it, so a list of millions built wave by wave (83 k atomics for config 5's 5.3 M matches) spent 0.25-1 ms per pass on its counter.
// Every thread of the (kThreads-wide) workgroup must call it.
template <int ITEMS>
__device__ __forceinline__ void block_append(const bool (&keep)[ITEMS], uint32_t *counter, uint32_t (&at)[ITEMS]) {
    __shared__ uint32_t s_wave[kThreads / 64];
    __shared__ uint32_t s_base;
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const unsigned long long mask = __ballot(keep[j]);
        at[j] = run + (uint32_t)__popcll(mask & below);
        run += (uint32_t)__popcll(mask);
    }
    if (lane == 0) s_wave[w] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int i = 0; i < kThreads / 64; ++i) { const uint32_t c = s_wave[i]; s_wave[i] = total; total += c; }
        s_base = total ? atomicAdd(counter, total) : 0u;
    }
    __syncthreads();
    const uint32_t base = s_base + s_wave[w];
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) at[j] += base;
}
constexpr int kAppendItems = 8;
inline dim3 grid_for_items(int64_t n, int items) { return grid_for((n + items - 1) / items); }
struct Pending { uint32_t k; int32_t ra, rb; };     // position in the ordered match list, roots of n1 / n2
// a bit that many threads set: a plain (possibly stale) look saves the atomic once the bit is visible - a node of config 5 has ~70 matches
__device__ __forceinline__ void set_bit(unsigned long long *word, unsigned long long mask) {
    if (!(*word & mask)) atomicOr(word, mask);
}
// matches of large connected components -> the first pending list; bit of the own image for their nodes
__global__ void k_large_pending(int64_t k_lo, int64_t k_hi, int64_t serial_limit, const uint32_t *flags, const uint32_t *seg_id, const uint32_t *starts, const uint32_t *order,
                                const uint32_t *n1, const uint32_t *n2, const int32_t *node_image, int W, unsigned long long *bits,
                                Pending *pend, uint32_t *n_pend) {
    const int64_t k0 = k_lo + (int64_t)blockIdx.x * (kThreads * kAppendItems) + threadIdx.x;      // positions [k_lo, k_hi) of the ordered list
    bool large[kAppendItems];
    uint32_t at[kAppendItems];
#pragma unroll
    for (int j = 0; j < kAppendItems; ++j) {
        const int64_t k = k0 + (int64_t)j * kThreads;
        large[j] = false;
        if (k < k_hi) {
            const uint32_t s = seg_id[k] + flags[k] - 1u;           // segment of position k
            large[j] = (int64_t)(starts[s + 1] - starts[s]) > serial_limit;
        }
    }
    block_append(large, n_pend, at);
#pragma unroll
    for (int j = 0; j < kAppendItems; ++j) {
        if (!large[j]) continue;
        const int64_t k = k0 + (int64_t)j * kThreads;
        const uint32_t m = order[k], a = n1[m], b = n2[m];
        pend[at[j]] = Pending{(uint32_t)k, (int32_t)a, (int32_t)b};
        if (bits) {                                                  // (idempotent: every match of a node sets the same bit - look first)
            set_bit(&bits[(size_t)a * W + (node_image[a] >> 6)], 1ull << (node_image[a] & 63));
            set_bit(&bits[(size_t)b * W + (node_image[b] >> 6)], 1ull << (node_image[b] & 63));
        }
    }
}
// retire what can never be accepted (same root / shared image: monotone), bid for the roots with the rest
// (one call per wave-wide slice of the pending list: every lane of the wave calls it, `valid` says whether it holds an entry)
__device__ __forceinline__ bool round_evaluate(bool valid, Pending &q, int32_t *parent, const unsigned long long *bits, int W) {
    if (!valid) return false;
    q.ra = par_find(parent, q.ra); q.rb = par_find(parent, q.rb);
    if (q.ra == q.rb) return false;
    const unsigned long long *A = bits + (size_t)q.ra * W, *B = bits + (size_t)q.rb * W;
    unsigned long long any = 0ull;
    for (int w = 0; w < W; ++w) any |= A[w] & B[w];               // solve.cc:506-511
    return any == 0ull;
}
__device__ __forceinline__ void round_bid(const Pending q, unsigned long long round_hi, unsigned long long *minpos) {
    const unsigned long long key = round_hi | q.k;                // a later round's bid beats every stale entry
    // thousands of matches bid for the root of a grown track and all but one lose: look before bidding (the value only
    // decreases, so a bid that does not beat what is already there could not have won)
    if (key < __hip_atomic_load(&minpos[q.ra], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&minpos[q.ra], key);
    if (key < __hip_atomic_load(&minpos[q.rb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&minpos[q.rb], key);
}
constexpr int kEvalItems = 4;
__global__ void k_round_eval(const uint32_t *n_in_p, const Pending *in, int32_t *parent, const unsigned long long *bits, int W,
                             unsigned long long round_hi, unsigned long long *minpos, Pending *out, uint32_t *n_out) {
    const uint32_t i0 = blockIdx.x * (kThreads * kEvalItems) + threadIdx.x;
    const uint32_t n_in = *n_in_p;                                // (the launch is sized by an upper bound: the count of an earlier round)
    if (blockIdx.x * (kThreads * kEvalItems) >= n_in) return;     // (uniform over the workgroup)
    Pending q[kEvalItems];
    bool keep[kEvalItems];
    uint32_t at[kEvalItems];
#pragma unroll
    for (int j = 0; j < kEvalItems; ++j) {
        const uint32_t i = i0 + j * kThreads;
        const bool valid = i < n_in;
        q[j] = valid ? in[i] : Pending{0, 0, 0};
        keep[j] = round_evaluate(valid, q[j], parent, bits, W);
    }
    block_append(keep, n_out, at);
#pragma unroll
    for (int j = 0; j < kEvalItems; ++j) if (keep[j]) { out[at[j]] = q[j]; round_bid(q[j], round_hi, minpos); }
}
// counters of a batch of rounds: c[j] = matches pending before round j of the batch; the last count of the previous batch moves to the front
__global__ void k_round_counters_shift(uint32_t *c, int R) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { c[0] = c[R]; for (int j = 1; j <= R; ++j) c[j] = 0u; }
}
// a bidder that holds both of its roots is the earliest pending match touching either: accept (solve.cc:513-521)
__device__ __forceinline__ void round_accept_one(const Pending q, unsigned long long round_hi, const unsigned long long *minpos,
                                                 int32_t *parent, int32_t *count, unsigned long long *bits, int W, uint32_t *n_accepted) {
    const unsigned long long key = round_hi | q.k;
    if (minpos[q.ra] != key || minpos[q.rb] != key) return;
    int32_t big = q.ra, small = q.rb;                              // r1 = root of n1, r2 = root of n2
    if (count[q.ra] < count[q.rb]) { big = q.rb; small = q.ra; }   // ties: root2 under root1
    __hip_atomic_store(&parent[small], big, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    count[big] += count[small];
    unsigned long long *A = bits + (size_t)big * W;
    const unsigned long long *B = bits + (size_t)small * W;
    for (int w = 0; w < W; ++w) A[w] |= B[w];
    atomicAdd(n_accepted, 1u);
}
__global__ void k_round_accept(const uint32_t *n_p, const Pending *pend, unsigned long long round_hi, const unsigned long long *minpos,
                               int32_t *parent, int32_t *count, unsigned long long *bits, int W, uint32_t *n_accepted) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *n_p) return;
    round_accept_one(pend[i], round_hi, minpos, parent, count, bits, W, n_accepted);
}

// ---- size cap (solve.cc:311-364): the cut itself runs on the host, on the handful of inter-track matches it needs ----
// component (pre-cut) of every track, and the inter-track matches of components above the cap, compacted as
// (unordered track pair, similarity): key = min << 32 | max
__global__ void k_track_comp(int64_t cap, const uint32_t *counts, const uint32_t *mlabel, const uint32_t *rank, int32_t *tcomp) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < cap && t < (int64_t)counts[CNT_TRACKS]) tcomp[t] = (int32_t)rank[mlabel[t]];
}
__global__ void k_cut_edges(int64_t M, const uint32_t *n1, const uint32_t *n2, const float *sim, const int32_t *track, const int32_t *tcomp,
                            const uint32_t *csize, uint32_t max_nodes, unsigned long long *pair_key, double *pair_sim, uint32_t *n_list) {
    const int64_t m0 = (int64_t)blockIdx.x * (kThreads * kAppendItems) + threadIdx.x;
    bool keep[kAppendItems];
    uint32_t at[kAppendItems];
    int32_t ta[kAppendItems], tb[kAppendItems];
#pragma unroll
    for (int j = 0; j < kAppendItems; ++j) {
        const int64_t m = m0 + (int64_t)j * kThreads;
        keep[j] = false; ta[j] = tb[j] = 0;
        if (m < M) {
            ta[j] = track[n1[m]]; tb[j] = track[n2[m]];
            keep[j] = ta[j] != tb[j] && csize[tcomp[ta[j]]] > max_nodes;
        }
    }
    block_append(keep, n_list, at);
#pragma unroll
    for (int j = 0; j < kAppendItems; ++j) {
        if (!keep[j]) continue;
        pair_key[at[j]] = ((unsigned long long)(uint32_t)min(ta[j], tb[j]) << 32) | (uint32_t)max(ta[j], tb[j]);
        pair_sim[at[j]] = (double)sim[m0 + (int64_t)j * kThreads];
    }
}
// meta union without the cut edges (solve.cc:346-353): gc[t] = subset of track t inside its oversized component, -1 elsewhere
__global__ void k_meta_union_cut(int64_t M, const uint32_t *n1, const uint32_t *n2, const int32_t *track, const int32_t *gc, uint32_t *parent) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const int32_t ta = track[n1[m]], tb = track[n2[m]];
    if (ta == tb) return;
    if (gc[ta] >= 0 && gc[ta] != gc[tb]) return;        // both tracks are in the same oversized component: the edge was cut
    uf_union(parent, (uint32_t)ta, (uint32_t)tb);
}
__global__ void k_init_nodes(int64_t n, const int32_t *node_image, int32_t *parent, int32_t *next, int32_t *tail, int32_t *count, ulonglong2 *sig) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { parent[i] = -1; next[i] = -1; tail[i] = (int32_t)i; count[i] = 1; sig[i] = image_signature(node_image[i]); }
}
__global__ void k_root_flags(int64_t n, const int32_t *parent, uint32_t *flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = parent[i] < 0 ? 1u : 0u;
}
// rank[] = exclusive scan of the root flags over N+1 entries: rank[N] = number of tracks
__global__ void k_track_ids(int64_t n, const int32_t *parent, const uint32_t *rank, int32_t *track, uint32_t *tsize, uint32_t *counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == 0) counts[CNT_TRACKS] = rank[n];
    int32_t r = (int32_t)i;
    while (parent[r] >= 0) r = parent[r];
    track[i] = (int32_t)rank[r];                              // solve.cc:528-541
    atomicAdd(&tsize[rank[r]], 1u);
}

// ---- roots: score = sum of similarities over intra-track out-edges; arg-max (score, node) ----
__global__ void k_scores(int64_t M, const uint32_t *n1, const uint32_t *n2, const float *sim, const int32_t *track, double *score) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const uint32_t a = n1[m], b = n2[m];
    if (track[a] == track[b]) { atomicAdd(&score[a], (double)sim[m]); atomicAdd(&score[b], (double)sim[m]); }
}
// The same sums with the matches taken in the ORDERED list (grouped by connected component): the 64 matches of a wave then touch a few
// dozen nodes, each several times, and the wave adds them up in LDS first - 128 slots per wave, claimed by compare-and-swap on the node id, a
// contribution that finds its slot taken by another node goes to memory directly - and sends one fp64 atomic per node instead of two per
// match (agent-scope fp64 atomics leave the XCD: 5 M of them were 0.21 ms on config 4; 0.10 ms this way).  Exact sums: the order of the additions is free.
constexpr int kScoreSlots = 128;
__global__ void k_scores_grouped(int64_t M, const uint4 *sorted, const uint32_t *order, const uint32_t *n1, const uint32_t *n2, const float *sim, const int32_t *track, double *score) {
    __shared__ uint32_t s_key[kThreads / 64][kScoreSlots];
    __shared__ double s_val[kThreads / 64][kScoreSlots];
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
    for (int i = lane; i < kScoreSlots; i += 64) { s_key[w][i] = 0xffffffffu; s_val[w][i] = 0.0; }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t node[2] = {0u, 0u};
    double s = 0.0;
    bool live = false;
    if (i < M) {
        if (sorted) {                                                            // (counting road: the record is there, in order - no gathers)
            const uint4 q = sorted[i];
            node[0] = q.y; node[1] = q.z;
            s = (double)sim_from_key(~q.x);                                      // (-0.0 comes back as +0.0: the same sum)
        } else {
            const uint32_t m = order[i];
            node[0] = n1[m]; node[1] = n2[m];
            s = (double)sim[m];
        }
        live = track[node[0]] == track[node[1]];
    }
    // (a wave's LDS operations complete in order: the zeroing above is visible to its own lanes without a barrier, other waves use other rows)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (!live) continue;
        const uint32_t h = (node[c] * 0x9E3779B1u) >> 25;                       // 7 bits
        const uint32_t seen = atomicCAS(&s_key[w][h], 0xffffffffu, node[c]);
        if (seen == 0xffffffffu || seen == node[c]) atomicAdd(&s_val[w][h], s);
        else atomicAdd(&score[node[c]], s);
    }
    for (int k = lane; k < kScoreSlots; k += 64) {
        const uint32_t key = s_key[w][k];
        if (key != 0xffffffffu) atomicAdd(&score[key], s_val[w][k]);
    }
}
__device__ __forceinline__ unsigned long long ordered_bits(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__global__ void k_best_score(int64_t n, const int32_t *track, const double *score, unsigned long long *best) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicMax(&best[track[i]], ordered_bits(score[i]));
}
__global__ void k_best_node(int64_t n, const int32_t *track, const double *score, const unsigned long long *best, int32_t *node) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && ordered_bits(score[i]) == best[track[i]]) atomicMax(&node[track[i]], (int32_t)i);   // ties: larger node idx
}
__global__ void k_mark_roots(int64_t cap, const uint32_t *counts, const int32_t *node, uint8_t *is_root) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < cap && t < (int64_t)counts[CNT_TRACKS]) is_root[node[t]] = 1;
}

// ---- components of the track meta-graph ----
// Two tracks are in one component of the meta-graph iff their nodes are in one connected component of the MATCH graph (a track is
// connected through its accepted matches; every other match joins two tracks and is a meta edge, solve.cc:262-290), and those labels exist
// since step 1.  So no second union-find over the matches (config 5: 2.3 ms, every union at the root of the one giant component): the
// component of track t is named by the smallest track of its connected component.
__global__ void k_cc_min_track(int64_t n, const uint32_t *cc, const int32_t *track, uint32_t *min_track) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    const uint32_t c = valid ? cc[i] : 0xffffffffu;
    uint32_t t = valid ? (uint32_t)track[i] : 0xffffffffu;
    // the lanes that share the first lane's component send one minimum (a giant component: the whole wave), the others their own;
    // nobody sends what cannot lower the word (it only decreases, so a stale read errs on the side of sending)
    const uint32_t c0 = (uint32_t)__shfl((int)c, 0, 64);
    const bool same = c == c0;
    uint32_t ts = same ? t : 0xffffffffu;
    for (int o = 32; o > 0; o >>= 1) ts = min(ts, (uint32_t)__shfl_xor((int)ts, o, 64));
    if (same) { if ((threadIdx.x & 63) != 0) return; t = ts; }
    if (valid && t < min_track[c]) atomicMin(&min_track[c], t);
}
__global__ void k_track_label(int64_t n, const uint32_t *cc, const int32_t *track, const uint32_t *min_track, uint32_t *label) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) label[track[i]] = min_track[cc[i]];                // (every node of a track writes the same value)
}
__global__ void k_comp_flags(int64_t cap, const uint32_t *counts, const uint32_t *parent, uint32_t *flags) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < cap && t < (int64_t)counts[CNT_TRACKS]) flags[t] = parent[t] == (uint32_t)t ? 1u : 0u;      // representative = smallest track of the component
}
// rank[] = exclusive scan of the component flags over N+1 entries (flags beyond the tracks are 0): rank[N] = #components
__global__ void k_comp_sizes(int64_t cap, uint32_t *counts, const uint32_t *parent, const uint32_t *rank, const uint32_t *tsize, uint32_t *csize) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) counts[CNT_COMPS] = rank[cap];
    const int64_t n = cap < (int64_t)counts[CNT_TRACKS] ? cap : (int64_t)counts[CNT_TRACKS];
    uint32_t v = 0;
    for (int64_t i = t; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        atomicAdd(&csize[rank[parent[i]]], tsize[i]);
        v = max(v, tsize[i]);
    }
    block_atomic_max(v, &counts[CNT_MAX_TRACK]);
}
__global__ void k_node_comp(int64_t n, const int32_t *track, const uint32_t *parent, const uint32_t *rank, int32_t *comp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) comp[i] = (int32_t)rank[parent[track[i]]];
}
__global__ void k_max_csize(int64_t cap, uint32_t *counts, const uint32_t *csize) {
    const int64_t n = cap < (int64_t)counts[CNT_COMPS] ? cap : (int64_t)counts[CNT_COMPS];
    uint32_t v = 0;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) v = max(v, csize[c]);
    block_atomic_max(v, &counts[CNT_MAX_COMP]);
}

}  // namespace

// =================================================================================================
// device copies of the graph and of the labels
// =================================================================================================
DevGraph::~DevGraph() {
    if (ctx) {      // nothing of ours may still be reading the slab when it goes back to the cache
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->s_copy);
        (void)hipStreamSynchronize(ctx->s_main);
    }
    if (!parent) for (auto &e : ev_flows) if (e) (void)hipEventDestroy(e);      // (a shard borrows its parent's events)
}
DevProblem::~DevProblem() {
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->s_main); }
}

static int stage_flows_now(const Graph &g, DevGraph &dg) {
    // 2 x 72 B per match, in match order, on the copy stream: travels beside the graph stage
    DevCtx *ctx = dg.ctx;
    const int64_t M = dg.M;
    float *d1 = dg.slab.take_n<float>((size_t)18 * M), *d2 = dg.slab.take_n<float>((size_t)18 * M);
    if (!d1 || !d2) { set_error("device graph: slab too small for the flows"); return LFR_ERR_NOMEM; }
    for (int c = 0; c < kFlowChunks; ++c) {
        const int64_t lo = M * c / kFlowChunks, hi = M * (c + 1) / kFlowChunks;
        dg.chunk_row[c] = lo; dg.chunk_row[c + 1] = hi;
        if (hi > lo) {
            LFR_HIP_TRY(hipMemcpyAsync(d1 + 18 * lo, g.m_disp1.data() + 18 * lo, (size_t)72 * (hi - lo), hipMemcpyHostToDevice, ctx->s_copy));
            LFR_HIP_TRY(hipMemcpyAsync(d2 + 18 * lo, g.m_disp2.data() + 18 * lo, (size_t)72 * (hi - lo), hipMemcpyHostToDevice, ctx->s_copy));
        }
        if (!dg.ev_flows[c]) LFR_HIP_TRY(hipEventCreateWithFlags(&dg.ev_flows[c], hipEventDisableTiming));
        LFR_HIP_TRY(hipEventRecord(dg.ev_flows[c], ctx->s_copy));
    }
    dg.disp1 = d1; dg.disp2 = d2;
    dg.flows_staged = true; dg.flows_zero_copy = false;
    return LFR_OK;
}

static int send_endpoints(const Graph &g, DevGraph &dg) {
    const int64_t N = g.n_nodes(), M = dg.M;
    hipStream_t st = dg.ctx->s_main;
    if (M > 0) {
        LFR_HIP_TRY(hipMemcpyAsync(dg.n1, g.m_node1.data(), (size_t)4 * M, hipMemcpyHostToDevice, st));
        LFR_HIP_TRY(hipMemcpyAsync(dg.n2, g.m_node2.data(), (size_t)4 * M, hipMemcpyHostToDevice, st));
        LFR_HIP_TRY(hipMemcpyAsync(dg.sim, g.m_sim.data(), (size_t)4 * M, hipMemcpyHostToDevice, st));
    }
    if (N > 0) LFR_HIP_TRY(hipMemcpyAsync(dg.node_image, g.node_image.data(), (size_t)4 * N, hipMemcpyHostToDevice, st));
    dg.N = N;
    dg.endpoints_pending = false;
    return LFR_OK;
}

void prestage_flows(const Graph &g, int device, int64_t n_bound) {
    const int64_t M = (int64_t)(g.m_disp1.size() / 18);
    if (device < 0 || M <= 0 || M >= ((int64_t)1 << 30) || n_bound >= ((int64_t)1 << 31)) return;
    if (g.dev_disp1) return;                                     // (pageable flows are fine: the copies below are staged by the runtime, on the scanner's helper thread)
    std::lock_guard<std::mutex> lk(g.dev_mu);
    if ((int)g.devgs.size() <= device) g.devgs.resize(device + 1);
    if (g.devgs[device]) return;
    DevCtx *ctx = dev_ctx(device);
    if (!ctx || hipSetDevice(device) != hipSuccess) return;
    std::shared_ptr<DevGraph> dg(new DevGraph());
    dg->ctx = ctx; dg->N = 0; dg->N_cap = n_bound; dg->M = M;
    const size_t bytes = (size_t)16 * M + (size_t)4 * n_bound + (size_t)144 * M + ((size_t)1 << 16);
    if (!dg->slab.init(ctx, bytes)) return;
    dg->n1 = dg->slab.take_n<uint32_t>(M); dg->n2 = dg->slab.take_n<uint32_t>(M);
    dg->sim = dg->slab.take_n<float>(M); dg->node_image = dg->slab.take_n<int32_t>(n_bound);
    if (stage_flows_now(g, *dg) != LFR_OK) return;
    dg->endpoints_pending = true;
    g.devgs[device] = dg;
}

int ensure_dev_graph(const Graph &g, int device, bool stage_flows, std::shared_ptr<DevGraph> &out) {
    if (device < 0) { set_error("bad device ordinal %d", device); return LFR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(g.dev_mu);
    if ((int)g.devgs.size() <= device) g.devgs.resize(device + 1);
    if (g.devgs[device] && g.devgs[device]->endpoints_pending) {          // the scanner sent the flows ahead
        DevGraph &dg = *g.devgs[device];
        if (dg.M != g.n_matches() || g.n_nodes() > dg.N_cap) g.devgs[device].reset();     // (cannot happen; rebuild rather than trust it)
        else {
            LFR_HIP_TRY(hipSetDevice(device));
            const int rc = send_endpoints(g, dg);
            if (rc != LFR_OK) { g.devgs[device].reset(); return rc; }
        }
    }
    if (g.devgs[device]) {
        if (stage_flows && g.devgs[device]->flows_zero_copy) g.devgs[device].reset();   // a whole-problem batch after a sharded one: rebuild with staged flows
        else { out = g.devgs[device]; return LFR_OK; }
    }
    if (g.dev_disp1 && g.dev_flows_device != device) {
        set_error("the graph's flows live on device %d, the pipeline was requested on device %d", g.dev_flows_device, device);
        return LFR_ERR_ARG;
    }
    DevCtx *ctx = dev_ctx(device);
    if (!ctx) return LFR_ERR_HIP;
    LFR_HIP_TRY(hipSetDevice(device));
    const int64_t N = g.n_nodes(), M = g.n_matches();
    if (N >= ((int64_t)1 << 31) || M >= ((int64_t)1 << 30)) { set_error("graph too large for the device pipeline"); return LFR_ERR_UNSUPPORTED; }
    std::shared_ptr<DevGraph> dg(new DevGraph());
    dg->ctx = ctx; dg->N = N; dg->N_cap = N; dg->M = M;
    const bool external = g.dev_disp1 && g.dev_disp2;
    const bool host_pinned = g.m_disp1.pinned() && g.m_disp2.pinned();
    const bool stage = !external && (stage_flows || !host_pinned);      // pageable flows cannot be read zero-copy
    const size_t bytes = (size_t)16 * M + (size_t)4 * N + (stage ? (size_t)144 * M : 0) + ((size_t)1 << 16);
    if (!dg->slab.init(ctx, bytes)) return LFR_ERR_NOMEM;
    dg->n1 = dg->slab.take_n<uint32_t>(M); dg->n2 = dg->slab.take_n<uint32_t>(M);
    dg->sim = dg->slab.take_n<float>(M); dg->node_image = dg->slab.take_n<int32_t>(N);
    hipStream_t st = ctx->s_main;
    {
        const int rc = send_endpoints(g, *dg);
        if (rc != LFR_OK) return rc;
    }
    if (external) {
        dg->disp1 = g.dev_disp1; dg->disp2 = g.dev_disp2; dg->flows_external = true;
        if (!g.m_flow_row.empty()) {
            dg->flow_row = dg->slab.take_n<uint32_t>(M);
            LFR_HIP_TRY(hipMemcpyAsync(dg->flow_row, g.m_flow_row.data(), (size_t)4 * M, hipMemcpyHostToDevice, st));
        }
    } else if (stage) {
        const int rc = stage_flows_now(g, *dg);
        if (rc != LFR_OK) return rc;
    } else {
        dg->disp1 = g.m_disp1.data(); dg->disp2 = g.m_disp2.data(); dg->flows_zero_copy = true;   // pinned + portable: device visible
    }
    g.devgs[device] = dg;
    out = dg;
    return LFR_OK;
}

int upload_labels(const Problem &p, int device, bool stage_flows, std::shared_ptr<DevProblem> &out) {
    std::shared_ptr<DevGraph> dg;
    int rc = ensure_dev_graph(*p.g, device, stage_flows, dg);
    if (rc != LFR_OK) return rc;
    DevCtx *ctx = dg->ctx;
    const int64_t N = dg->N;
    std::shared_ptr<DevProblem> dp(new DevProblem());
    dp->ctx = ctx; dp->graph = dg; dp->N = N;
    if (!dp->slab.init(ctx, (size_t)9 * N + 4096)) return LFR_ERR_NOMEM;
    dp->track = dp->slab.take_n<int32_t>(N); dp->comp = dp->slab.take_n<int32_t>(N); dp->is_root = dp->slab.take_n<uint8_t>(N);
    // Labels that already live on ANOTHER GPU (the device graph stage ran there) come over the GPU-GPU link - xGMI on an 8-GPU node -
    // instead of through the host: 9 bytes per node, no D2H, no widening to the host's 64-bit labels and back.
    std::shared_ptr<DevProblem> peer;
    {
        std::lock_guard<std::mutex> lk(p.label_mu);
        for (auto &d : p.devs) if (d && d->track && d->N == N && d->ctx->device != device) { peer = d; break; }
    }
    if (peer && N > 0) {
        const int src = peer->ctx->device;
        LFR_HIP_TRY(hipMemcpyPeerAsync(dp->track, device, peer->track, src, (size_t)4 * N, ctx->s_main));
        LFR_HIP_TRY(hipMemcpyPeerAsync(dp->comp, device, peer->comp, src, (size_t)4 * N, ctx->s_main));
        LFR_HIP_TRY(hipMemcpyPeerAsync(dp->is_root, device, peer->is_root, src, (size_t)N, ctx->s_main));
        LFR_HIP_TRY(hipStreamSynchronize(ctx->s_main));
        out = dp;
        return LFR_OK;
    }
    if (N > 0) {
        if (!p.host_labels_valid) { const int rc2 = p.ensure_host_labels(); if (rc2 != LFR_OK) return rc2; }
        std::vector<int32_t> t32(N), c32(N);
        for (int64_t i = 0; i < N; ++i) { t32[i] = (int32_t)p.track[i]; c32[i] = (int32_t)p.comp[i]; }
        LFR_HIP_TRY(hipMemcpyAsync(dp->track, t32.data(), (size_t)4 * N, hipMemcpyHostToDevice, ctx->s_main));
        LFR_HIP_TRY(hipMemcpyAsync(dp->comp, c32.data(), (size_t)4 * N, hipMemcpyHostToDevice, ctx->s_main));
        LFR_HIP_TRY(hipMemcpyAsync(dp->is_root, p.is_root.data(), (size_t)N, hipMemcpyHostToDevice, ctx->s_main));
        LFR_HIP_TRY(hipStreamSynchronize(ctx->s_main));         // the staging vectors die here
    }
    out = dp;
    return LFR_OK;
}

int Problem::ensure_host_labels() const {
    std::lock_guard<std::mutex> lk(label_mu);
    if (host_labels_valid) return LFR_OK;
    std::shared_ptr<DevProblem> dev;
    for (auto &d : devs) if (d) { dev = d; break; }
    if (!dev) { set_error("internal: labels neither on the host nor on the device"); return LFR_ERR_ARG; }
    const int64_t N = dev->N;
    DevCtx *ctx = dev->ctx;
    LFR_HIP_TRY(hipSetDevice(ctx->device));
    std::vector<int32_t> t32(N), c32(N);
    track.resize(N); comp.resize(N); is_root.resize(N);
    if (N > 0) {
        LFR_HIP_TRY(hipMemcpyAsync(t32.data(), dev->track, (size_t)4 * N, hipMemcpyDeviceToHost, ctx->s_main));
        LFR_HIP_TRY(hipMemcpyAsync(c32.data(), dev->comp, (size_t)4 * N, hipMemcpyDeviceToHost, ctx->s_main));
        LFR_HIP_TRY(hipMemcpyAsync(is_root.data(), dev->is_root, (size_t)N, hipMemcpyDeviceToHost, ctx->s_main));
        LFR_HIP_TRY(hipStreamSynchronize(ctx->s_main));
    }
    for (int64_t i = 0; i < N; ++i) { track[i] = t32[i]; comp[i] = c32[i]; }
    host_labels_valid = true;
    return LFR_OK;
}

// =================================================================================================
// the stage
// =================================================================================================
int warm_graphstage_primitives(DevCtx *ctx) {
    hipStream_t st = ctx->s_main;
    LFR_HIP_TRY(hipSetDevice(ctx->device));
    const int64_t sizes[4] = {100000, 300000, 1000000, (int64_t)4 << 20};   // (merge-sort levels and radix paths differ by size)
    DevArena arena;
    if (!arena.init(ctx, (size_t)sizes[3] * 64 + ((size_t)64 << 20))) return LFR_ERR_NOMEM;
    const int64_t nmax = sizes[3];
    uint64_t *k64a = arena.take_n<uint64_t>(nmax), *k64b = arena.take_n<uint64_t>(nmax);
    uint32_t *k32a = arena.take_n<uint32_t>(nmax), *k32b = arena.take_n<uint32_t>(nmax), *v32a = arena.take_n<uint32_t>(nmax), *v32b = arena.take_n<uint32_t>(nmax);
    if (!k64a || !k64b || !k32a || !k32b || !v32a || !v32b) { set_error("warm-up arena exhausted"); return LFR_ERR_NOMEM; }
    LFR_HIP_TRY(hipMemsetAsync(k64a, 0x5a, 8 * (size_t)nmax, st));
    LFR_HIP_TRY(hipMemsetAsync(k32a, 0x3c, 4 * (size_t)nmax, st));
    LFR_HIP_TRY(hipMemsetAsync(v32a, 0, 4 * (size_t)nmax, st));
    int rc = LFR_OK;
    for (const int64_t n : sizes) {
        if ((rc = sort_pairs(arena, k32a, k32b, v32a, v32b, n, 0, 20, st)) != LFR_OK) return rc;
        if ((rc = sort_pairs(arena, k64a, k64b, v32a, v32b, n, 0, 52, st)) != LFR_OK) return rc;
        if ((rc = exclusive_sum(arena, v32a, v32b, n, st)) != LFR_OK) return rc;
    }
    LFR_HIP_TRY(stream_wait(st));
    return rc;
}

// ---- sharding by connected component (multi-GPU: every rank's graph stage, assembly and solve over its own components only) ----
__global__ void k_cc_is_root(int64_t n, const uint32_t *cc, uint32_t *flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) flag[i] = i < n && cc[i] == (uint32_t)i ? 1u : 0u;
}
// keep[m] = the connected component of match m is dealt to `rank`; per-rank match counts (one atomic per workgroup and rank present)
__global__ void k_shard_keep(int64_t M, const uint32_t *n1, const uint32_t *cc, const uint32_t *cc_index, int rank, int world, uint32_t *keep, unsigned long long *per_rank) {
    __shared__ unsigned int cnt[64];
    if (threadIdx.x < 64) cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m < M) {
        const int owner = (int)(cc_index[cc[n1[m]]] % (uint32_t)world);
        keep[m] = owner == rank ? 1u : 0u;
        atomicAdd(&cnt[owner], 1u);
    } else if (m == M) keep[m] = 0u;
    __syncthreads();
    if (threadIdx.x < world && cnt[threadIdx.x]) atomicAdd(&per_rank[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}
__global__ void k_shard_scatter(int64_t M, const uint32_t *keep, const uint32_t *pos, const uint32_t *n1, const uint32_t *n2, const float *sim,
                                const uint32_t *flow_row, uint32_t *o_n1, uint32_t *o_n2, float *o_sim, uint32_t *o_row) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M || !keep[m]) return;
    const uint32_t q = pos[m];
    o_n1[q] = n1[m]; o_n2[q] = n2[m]; o_sim[q] = sim[m];
    o_row[q] = flow_row ? flow_row[m] : (uint32_t)m;
}
// The shard of `full` for (rank, world): connected components (the same union-find kernels as the stage itself), the k-th component in
// node order to rank k mod world, a STABLE compaction of the matches (their relative order is what the batch layout of a component
// depends on: the shard's components come out bit-identical to the whole graph's).  per_rank_h[r] = matches of rank r.
static int shard_dev_graph(const std::shared_ptr<DevGraph> &full, int rank, int world, std::shared_ptr<DevGraph> &out, std::vector<unsigned long long> &per_rank_h) {
    DevCtx *ctx = full->ctx;
    hipStream_t st = ctx->s_main;
    const int64_t N = full->N, M = full->M;
    DevArena arena;
    if (!arena.init(ctx, (size_t)12 * N + (size_t)12 * M + ((size_t)8 << 20))) return LFR_ERR_NOMEM;
    uint32_t *parent = arena.take_n<uint32_t>(N), *cc = arena.take_n<uint32_t>(N), *rflag = arena.take_n<uint32_t>(N + 1), *cc_index = arena.take_n<uint32_t>(N + 1);
    uint32_t *keep = arena.take_n<uint32_t>(M + 1), *pos = arena.take_n<uint32_t>(M + 1);
    unsigned long long *per_rank = arena.take_n<unsigned long long>(64);
    if (!parent || !cc || !rflag || !cc_index || !keep || !pos || !per_rank) { set_error("shard arena exhausted"); return LFR_ERR_NOMEM; }
    LFR_HIP_TRY(hipMemsetAsync(per_rank, 0, 64 * 8, st));
    hipLaunchKernelGGL(k_iota, grid_for(N), dim3(kThreads), 0, st, N, parent);
    for (int i = 0, done = 0; i < kUnionStages; done = kUnionStrides[i], ++i) {
        if (i) hipLaunchKernelGGL(k_uf_flatten, grid_for(N), dim3(kThreads), 0, st, N, parent);
        hipLaunchKernelGGL(k_cc_union, grid_for((M + kUnionStrides[i] - 1) / kUnionStrides[i]), dim3(kThreads), 0, st, M, kUnionStrides[i], done, full->n1, full->n2, parent);
    }
    hipLaunchKernelGGL(k_cc_labels, grid_for(N), dim3(kThreads), 0, st, N, parent, cc);
    hipLaunchKernelGGL(k_cc_is_root, grid_for(N + 1), dim3(kThreads), 0, st, N, cc, rflag);
    int rc;
    if ((rc = exclusive_sum(arena, rflag, cc_index, N + 1, st)) != LFR_OK) return rc;
    hipLaunchKernelGGL(k_shard_keep, grid_for(M + 1), dim3(kThreads), 0, st, M, full->n1, cc, cc_index, rank, world, keep, per_rank);
    if ((rc = exclusive_sum(arena, keep, pos, M + 1, st)) != LFR_OK) return rc;
    per_rank_h.assign(64, 0);
    LFR_HIP_TRY(hipMemcpyAsync(per_rank_h.data(), per_rank, 64 * 8, hipMemcpyDeviceToHost, st));
    LFR_HIP_TRY(stream_wait(st));
    const int64_t Ms = (int64_t)per_rank_h[rank];
    std::shared_ptr<DevGraph> dg(new DevGraph());
    dg->ctx = ctx; dg->N = N; dg->M = Ms; dg->N_cap = N; dg->parent = full;
    if (!dg->slab.init(ctx, (size_t)16 * std::max<int64_t>(Ms, 1) + 4096)) return LFR_ERR_NOMEM;
    dg->n1 = dg->slab.take_n<uint32_t>(Ms); dg->n2 = dg->slab.take_n<uint32_t>(Ms); dg->sim = dg->slab.take_n<float>(Ms); dg->flow_row = dg->slab.take_n<uint32_t>(Ms);
    if (!dg->n1 || !dg->n2 || !dg->sim || !dg->flow_row) { set_error("shard slab exhausted"); return LFR_ERR_NOMEM; }
    dg->node_image = full->node_image;
    dg->disp1 = full->disp1; dg->disp2 = full->disp2;
    dg->flows_staged = full->flows_staged; dg->flows_zero_copy = full->flows_zero_copy; dg->flows_external = full->flows_external;
    for (int c = 0; c < 4; ++c) dg->ev_flows[c] = full->ev_flows[c];
    for (int c = 0; c < 5; ++c) dg->chunk_row[c] = full->chunk_row[c];
    hipLaunchKernelGGL(k_shard_scatter, grid_for(M), dim3(kThreads), 0, st, M, keep, pos, full->n1, full->n2, full->sim, full->flow_row,
                       dg->n1, dg->n2, dg->sim, dg->flow_row);
    LFR_HIP_TRY(hipGetLastError());
    LFR_HIP_TRY(stream_wait(st));                      // (the temporaries go back to the cache)
    out = dg;
    return LFR_OK;
}

namespace {

// =================================================================================================
// the stage: its knobs, its state, and the passes of graph_stage_on_device in the order they run
// =================================================================================================
struct StageKnobs {                                // every environment knob of the stage; read per call (the tests change them between calls)
    bool say_hand_back = false;                    // LFR_VERBOSE or LFR_TIMING set: a hand-back to the host stage says why
    int trace = 0;                                 // LFR_VERBOSE=2: lap times, 3: + every round of the parallel greedy
    int max_tie_run = kMaxTieRun;                  // LFR_MAX_TIE_RUN (tests: 0 = always the three sorts)
    bool one_sort_order = false;                   // LFR_ONE_SORT_ORDER: skip the counting road
    int64_t serial_limit = kSerialSegmentEdges;    // LFR_SERIAL_SEGMENT_EDGES
    int64_t rounds_first_block = 0;                // LFR_ROUNDS_FIRST_BLOCK (0: the default, 2 N positions)
    const char *debug_dump = nullptr;              // LFR_DEBUG_DUMP: folder for the intermediates of the stage as raw files
    static StageKnobs read() {
        StageKnobs k;
        const char *vb = getenv("LFR_VERBOSE");
        k.say_hand_back = vb || getenv("LFR_TIMING");
        k.trace = vb ? atoi(vb) >= 2 ? atoi(vb) : 0 : 0;
        if (const char *e = getenv("LFR_MAX_TIE_RUN")) k.max_tie_run = std::max(0, atoi(e));
        k.one_sort_order = getenv("LFR_ONE_SORT_ORDER") != nullptr;
        if (const char *e = getenv("LFR_SERIAL_SEGMENT_EDGES")) k.serial_limit = std::max<int64_t>(0, atoll(e));
        if (const char *e = getenv("LFR_ROUNDS_FIRST_BLOCK")) k.rounds_first_block = std::max<int64_t>(1, atoll(e));
        k.debug_dump = getenv("LFR_DEBUG_DUMP");
        return k;
    }
};

// how the matches of a connected component got into the reference's order (step 2)
enum class MatchOrder {
    counted_streamed,                              // grouped by component, ranked by counting: sorted records (srec), no ties to repair
    one_sort_tie_repair,                           // one sort over (component | ~similarity) + k_tie_fix
    three_sorts                                    // the exact order of round 3: by n2, by (similarity, n1), by component
};

struct Stage {
    // ---- the call: dimensions, stream, arena, pinned counters, events ----
    const Graph &g;
    Problem &p;
    const int device;
    const StageKnobs knobs = StageKnobs::read();
    const std::chrono::steady_clock::time_point tr0 = std::chrono::steady_clock::now();
    int64_t N, M, max_nodes = 0, seg_cap = 0;      // seg_cap: a segment has >= 1 match and >= 2 nodes
    int node_bits = 1;
    lfr_problem_stats stats{};                     // -> p.stats in publish()
    std::shared_ptr<DevGraph> dg;
    std::shared_ptr<DevProblem> dp;
    DevCtx *ctx = nullptr;
    hipStream_t st = nullptr;
    const uint32_t *n1 = nullptr, *n2 = nullptr;
    const float *sim = nullptr;
    DevArena arena;                                // temporaries of this call
    uint32_t *h_counts = nullptr;                  // pinned: CNT_HOST_WORDS words
    size_t pin_bytes = 0;
    enum { EV_FILLED, EV_TRACKS, EV_ROOTS, EV_COMPS, EV_BEGIN, EV_CUT_BEGIN, EV_CUT_END, EV_COUNT };
    hipEvent_t ev[EV_COUNT] = {};                  // (EV_BEGIN: only under LFR_VERBOSE>=2; the cut's pair: only when it runs)
    // ---- device arrays, by what they are ----
    uint32_t *counts = nullptr;                    // CNT_WORDS, first in the zero block
    size_t zero_bytes = 0, scan_words_m = 0, scan_words_n = 0;
    unsigned long long *scan_state = nullptr;      // look-back states of the three one-launch prefix sums: segments, tracks, components
    struct { uint32_t *parent = nullptr, *label = nullptr; } cc;                           // connected components of the match graph
    struct {                                       // order and segments
        uint4 *rec = nullptr, *srec = nullptr;     // counting road: the records, and the records in the reference's order
        uint64_t *khi = nullptr, *khi2 = nullptr;  // (the 64-bit keys of the sorting roads share rec's 16 M bytes)
        uint32_t *klo = nullptr, *klo2 = nullptr, *id0 = nullptr, *id1 = nullptr, *ck0 = nullptr, *ck1 = nullptr;
        uint32_t *flags = nullptr, *segid = nullptr, *starts = nullptr, *order = nullptr;
    } ord;
    struct { int32_t *par = nullptr, *next = nullptr, *tail = nullptr, *cnt = nullptr; ulonglong2 *sig = nullptr; } uf;     // constrained union-find
    struct {                                       // tracks and roots
        uint32_t *rflag = nullptr, *rrank = nullptr, *tsize = nullptr;
        double *score = nullptr; unsigned long long *best = nullptr; int32_t *bnode = nullptr;
    } trk;
    struct {                                       // component labelling (mp_parent: smallest track per connected component, starts at ~0)
        uint32_t *mp_parent = nullptr, *mp = nullptr, *cflag = nullptr, *crank = nullptr, *csize = nullptr;
        int32_t *gc = nullptr;                     // after a cut: subset of every track inside its component
    } lab;

    Stage(const Graph &g_, Problem &p_, int device_) : g(g_), p(p_), device(device_), N(g_.n_nodes()), M(g_.n_matches()) {}
    Stage(const Stage &) = delete;
    ~Stage() {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (h_counts) ctx->pinned_release(h_counts, pin_bytes);
    }
    void lap(const char *what) const {
        if (knobs.trace) fprintf(stderr, "lfr graph stage: %8.3f ms  %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count(), what);
    }
    // (every hand-back to the host graph stage says why under LFR_VERBOSE / LFR_TIMING: results are the same, the time is not - ADVICE r4)
    int use_host(const char *why) const {
        if (knobs.say_hand_back) fprintf(stderr, "lfr graph stage: handed back to the host (%s)\n", why);
        return LFR_GRAPHSTAGE_USE_HOST;
    }
    bool has_large_components() const { return (int64_t)h_counts[CNT_MAX_SEG] > knobs.serial_limit; }

    int shard_if_balanced(int shard_rank, int shard_world);
    int prepare();
    int connected_components();
    int three_sorts();
    int segments(bool states_fresh);
    int order_matches(MatchOrder &kind);
    int union_find_small(MatchOrder kind);
    int union_find_rounds();
    int tracks_and_roots(MatchOrder kind);
    int label_components(bool after_cut);
    int read_counts(const char *what);
    void trace_fill_time() const;
    void debug_dump() const;
    int cut_oversized();
    int publish();
};
constexpr char kStageArena[] = "graph stage: device arena";

int Stage::shard_if_balanced(int shard_rank, int shard_world) {
    p.cc_sharded = false;
    if (!(shard_world > 1 && shard_world <= 64 && M > 0)) return LFR_OK;
    std::shared_ptr<DevGraph> dgs;
    std::vector<unsigned long long> per_rank;
    const int rc = shard_dev_graph(dg, shard_rank, shard_world, dgs, per_rank);
    if (rc != LFR_OK) return rc;
    unsigned long long mx = 0;
    for (int r = 0; r < shard_world; ++r) mx = std::max(mx, per_rank[r]);
    // balanced enough (every rank decides the same from the same counts): the largest rank within 5/4 of the mean
    if (4ull * mx * (unsigned long long)shard_world <= 5ull * (unsigned long long)M + 4096ull * shard_world) {
        dg = dgs; M = dg->M;
        p.cc_sharded = true; p.shard_matches = M; p.shard_matches_max = (int64_t)mx;
    }
    lap(p.cc_sharded ? "sharded by connected component" : "one connected component dominates: the whole graph on every rank");
    return LFR_OK;
}

// slabs, pinned block, events, and everything that starts at zero in one block: one fill instead of a dozen memsets
int Stage::prepare() {
    dp.reset(new DevProblem());
    dp->ctx = ctx; dp->graph = dg; dp->N = N;
    if (!dp->slab.init(ctx, (size_t)9 * N + 4096)) return LFR_ERR_NOMEM;
    dp->track = dp->slab.take_n<int32_t>(N); dp->comp = dp->slab.take_n<int32_t>(N); dp->is_root = dp->slab.take_n<uint8_t>(N);
    if (!arena.init(ctx, (size_t)112 * M + (size_t)112 * N + ((size_t)32 << 20))) return LFR_ERR_NOMEM;
    h_counts = (uint32_t *)ctx->pinned_acquire(4 * CNT_HOST_WORDS, &pin_bytes);
    if (!h_counts) return LFR_ERR_NOMEM;
    for (int i = EV_FILLED; i <= EV_COMPS; ++i) LFR_HIP_TRY(hipEventCreate(&ev[i]));
    lap("slabs, pinned block, events");

    n1 = dg->n1; n2 = dg->n2; sim = dg->sim;
    while (((int64_t)1 << node_bits) < N) ++node_bits;
    seg_cap = std::min(N, M) + 1;
    if (knobs.trace) { LFR_HIP_TRY(hipEventCreate(&ev[EV_BEGIN])); LFR_HIP_TRY(hipEventRecord(ev[EV_BEGIN], st)); }
    const size_t zero_mark = arena.top;
    LFR_TAKE(arena, kStageArena, counts, uint32_t, CNT_WORDS);
    LFR_TAKE(arena, kStageArena, ord.flags, uint32_t, M + 1); LFR_TAKE(arena, kStageArena, trk.rflag, uint32_t, N + 1);
    LFR_TAKE(arena, kStageArena, trk.tsize, uint32_t, N); LFR_TAKE(arena, kStageArena, trk.score, double, N);
    LFR_TAKE(arena, kStageArena, trk.best, unsigned long long, N);
    LFR_TAKE(arena, kStageArena, lab.cflag, uint32_t, N + 1); LFR_TAKE(arena, kStageArena, lab.csize, uint32_t, N);
    // look-back states of the stage's prefix sums (exclusive_sum_one_launch: no init launch for states that start in the zero block)
    scan_words_m = scan_state_words(M + 1); scan_words_n = scan_state_words(N + 1);
    LFR_TAKE(arena, kStageArena, scan_state, unsigned long long, scan_words_m + 2 * scan_words_n);
    zero_bytes = arena.top - zero_mark;
    LFR_TAKE(arena, kStageArena, trk.bnode, int32_t, N); LFR_TAKE(arena, kStageArena, lab.mp_parent, uint32_t, N);      // (next to each other: one region of -1 / of "no track yet")
    // the stage's initial values in one launch (the memsets were 5 launches before the first kernel, 2 more before the meta-components)
    FillRegions fr;
    fr.add(arena.base + zero_mark, zero_bytes, 0);
    fr.add(dp->is_root, (size_t)N, 0);
    fr.add(trk.bnode, (size_t)(reinterpret_cast<char *>(lab.mp_parent + N) - reinterpret_cast<char *>(trk.bnode)), 0xff);
    LFR_HIP_TRY(fill_regions(fr, st));
    LFR_HIP_TRY(hipEventRecord(ev[EV_FILLED], st));
    return LFR_OK;
}

// 1. connected components of the match graph (conflicts ignored)
int Stage::connected_components() {
    LFR_TAKE(arena, kStageArena, cc.parent, uint32_t, N); LFR_TAKE(arena, kStageArena, cc.label, uint32_t, N);
    hipLaunchKernelGGL(k_iota, grid_for(N), dim3(kThreads), 0, st, N, cc.parent);
    for (int i = 0, done = 0; i < kUnionStages; done = kUnionStrides[i], ++i) {
        if (i) hipLaunchKernelGGL(k_uf_flatten, grid_for(N), dim3(kThreads), 0, st, N, cc.parent);
        hipLaunchKernelGGL(k_cc_union, grid_for((M + kUnionStrides[i] - 1) / kUnionStrides[i]), dim3(kThreads), 0, st, M, kUnionStrides[i], done, n1, n2, cc.parent);
    }
    hipLaunchKernelGGL(k_cc_labels, grid_for(N), dim3(kThreads), 0, st, N, cc.parent, cc.label);
    return LFR_OK;
}

int Stage::three_sorts() {                         // -> ord.order (= id1)
    int r;
    hipLaunchKernelGGL(k_match_keys, grid_for(M), dim3(kThreads), 0, st, M, (uint32_t)(N - 1), node_bits, n1, n2, sim, ord.khi, ord.klo, ord.id0);
    if ((r = sort_pairs(arena, ord.klo, ord.klo2, ord.id0, ord.id1, M, 0, node_bits, st)) != LFR_OK) return r;
    hipLaunchKernelGGL(k_gather_u64, grid_for(M), dim3(kThreads), 0, st, M, ord.id1, ord.khi, ord.khi2);
    if ((r = sort_pairs(arena, ord.khi2, ord.khi, ord.id1, ord.id0, M, 0, 32 + node_bits, st)) != LFR_OK) return r;
    hipLaunchKernelGGL(k_cc_keys, grid_for(M), dim3(kThreads), 0, st, M, ord.id0, n1, cc.label, ord.ck0);
    return sort_pairs(arena, ord.ck0, ord.ck1, ord.id0, ord.id1, M, 0, node_bits, st);   // stable
}

// flags -> segment ids, starts, longest segment
int Stage::segments(bool states_fresh) {
    // (the one long prefix sum of the stage: rocPRIM's larger tiles keep the look-back chain short - 20.6 us with its init launch
    // against 26.9 us for the one-launch kernel at 2.5 M flags; the short sums below are the other way round.  The one-launch sum's
    // states are good for one use: a second pass over the segments takes the library's.)
    if (M + 1 > (int64_t)1 << 20 || !states_fresh) { const int r = exclusive_sum(arena, ord.flags, ord.segid, M + 1, st); if (r != LFR_OK) return r; }
    else LFR_HIP_TRY(exclusive_sum_one_launch(ord.flags, ord.segid, M + 1, scan_state, st));
    hipLaunchKernelGGL(k_seg_starts, grid_for(std::max<int64_t>(M, 1)), dim3(kThreads), 0, st, M, ord.flags, ord.segid, ord.starts, counts);
    hipLaunchKernelGGL(k_seg_maxlen, grid_few(seg_cap), dim3(kThreads), 0, st, seg_cap, ord.starts, counts);
    return LFR_OK;
}

// 2. matches grouped by connected component, inside a component in the reference's order: descending (sim, n1, n2).
// The counting road (k_rank_sort) first: group by component, look at the longest segment (the stage's first read-back), count inside
// the segments.  A giant component (or LFR_ONE_SORT_ORDER=1) takes one sort over (component | ~similarity) + the tie repair; the
// tests' LFR_MAX_TIE_RUN=0 takes the three sorts at once (a long tie found by the repair takes them later: graph_stage_on_device).
int Stage::order_matches(MatchOrder &kind) {
    int rc;
    LFR_TAKE(arena, kStageArena, ord.rec, uint4, M);
    ord.khi = reinterpret_cast<uint64_t *>(ord.rec); ord.khi2 = ord.khi + M;
    LFR_TAKE(arena, kStageArena, ord.klo, uint32_t, M); LFR_TAKE(arena, kStageArena, ord.klo2, uint32_t, M);
    LFR_TAKE(arena, kStageArena, ord.srec, uint4, M);
    LFR_TAKE(arena, kStageArena, ord.id0, uint32_t, M); LFR_TAKE(arena, kStageArena, ord.id1, uint32_t, M);
    LFR_TAKE(arena, kStageArena, ord.ck0, uint32_t, M); LFR_TAKE(arena, kStageArena, ord.ck1, uint32_t, M);
    LFR_TAKE(arena, kStageArena, ord.segid, uint32_t, M + 1);
    LFR_TAKE(arena, kStageArena, ord.starts, uint32_t, std::min(N, M) + 2);
    ord.order = ord.id1;
    const bool try_counting = knobs.max_tie_run > 0 && !knobs.one_sort_order;
    if (try_counting) {
        hipLaunchKernelGGL(k_match_records, grid_for(M), dim3(kThreads), 0, st, M, n1, n2, sim, cc.label, ord.rec, ord.ck0, ord.id0);
        if ((rc = sort_pairs(arena, ord.ck0, ord.ck1, ord.id0, ord.id1, M, 0, node_bits, st)) != LFR_OK) return rc;
        hipLaunchKernelGGL(k_seg_flags, grid_for(M), dim3(kThreads), 0, st, M, ord.ck1, ord.flags);
        if ((rc = segments(true)) != LFR_OK) return rc;
        lap("grouped by connected component");
        if ((rc = read_counts("first read-back")) != LFR_OK) return rc;
        if ((int64_t)h_counts[CNT_MAX_SEG] <= kRankSortMax) {
            const size_t window = sizeof(uint4) * ((size_t)kThreads + 2 * (size_t)h_counts[CNT_MAX_SEG]);     // (8 KB for config 4's 136: eight workgroups per CU)
            hipLaunchKernelGGL(k_rank_sort, grid_for(M), dim3(kThreads), window, st, M, ord.id1, ord.rec, ord.flags, ord.segid, ord.starts, ord.id0, ord.srec);
            ord.order = ord.id0;
            kind = MatchOrder::counted_streamed;
            return LFR_OK;
        }
    }
    if (knobs.max_tie_run > 0) {
        hipLaunchKernelGGL(k_cc_sim_keys, grid_for(M), dim3(kThreads), 0, st, M, n1, sim, cc.label, ord.khi, ord.id0);
        if ((rc = sort_pairs(arena, ord.khi, ord.khi2, ord.id0, ord.id1, M, 0, 32 + node_bits, st)) != LFR_OK) return rc;
        hipLaunchKernelGGL(k_tie_fix, grid_for(M), dim3(kThreads), 0, st, M, ord.khi2, ord.order, n1, n2, knobs.max_tie_run, counts);
        hipLaunchKernelGGL(k_seg_flags_hi, grid_for(M), dim3(kThreads), 0, st, M, ord.khi2, ord.flags);
        kind = MatchOrder::one_sort_tie_repair;
    } else {
        if ((rc = three_sorts()) != LFR_OK) return rc;
        hipLaunchKernelGGL(k_seg_flags, grid_for(M), dim3(kThreads), 0, st, M, ord.ck1, ord.flags);
        kind = MatchOrder::three_sorts;
    }
    return segments(!try_counting);
}

// 3. greedy constrained union-find per connected component: the small ones, one thread each (from scratch: also after a re-order)
int Stage::union_find_small(MatchOrder kind) {
    if (!uf.par) {
        LFR_TAKE(arena, kStageArena, uf.par, int32_t, N); LFR_TAKE(arena, kStageArena, uf.next, int32_t, N); LFR_TAKE(arena, kStageArena, uf.tail, int32_t, N);
        LFR_TAKE(arena, kStageArena, uf.cnt, int32_t, N); LFR_TAKE(arena, kStageArena, uf.sig, ulonglong2, N);
    }
    hipLaunchKernelGGL(k_init_nodes, grid_for(N), dim3(kThreads), 0, st, N, dg->node_image, uf.par, uf.next, uf.tail, uf.cnt, uf.sig);
    if (kind == MatchOrder::counted_streamed)      // (the matches as a stream of sorted records)
        hipLaunchKernelGGL(k_kruskal_stream, grid_for(seg_cap), dim3(kThreads), 0, st, seg_cap, knobs.serial_limit, counts, ord.starts, ord.srec, dg->node_image,
                           uf.par, uf.next, uf.tail, uf.cnt, uf.sig);
    else
        hipLaunchKernelGGL(k_kruskal, grid_for(seg_cap), dim3(kThreads), 0, st, seg_cap, knobs.serial_limit, counts, ord.starts, ord.order, n1, n2,
                           dg->node_image, uf.par, uf.next, uf.tail, uf.cnt, uf.sig);
    return LFR_OK;
}

// 4. ... the large ones in parallel rounds
int Stage::union_find_rounds() {
    const int W = (int)((g.image_names.size() + 63) / 64);
    const size_t bits_bytes = (size_t)N * W * 8;
    if (bits_bytes > kMaxBitsetBytes) return use_host("image bitsets above the cap");
    // Rounds run in batches of kRoundBatch without a host round trip: every round takes its input count from the device
    // (the launches are sized by the count of the last read-back: counts only shrink), a round with nothing pending is two
    // empty launches.  Round 2 read the count back after every round: 76 synchronisations for config 5's giant component.
    constexpr int kRoundBatch = 8;
    static_assert(CNT_HOST_ROUNDS + kRoundBatch + 1 <= CNT_HOST_WORDS, "the rounds' counters fit behind the counts");
    constexpr char kRoundsArena[] = "graph stage: rounds arena";
    DevArena rounds_arena;
    if (!rounds_arena.init(ctx, bits_bytes + 2 * (size_t)M * sizeof(Pending) + 8 * (size_t)N + 65536)) return LFR_ERR_NOMEM;
    unsigned long long *bits, *minpos;
    Pending *pa, *pb;
    uint32_t *ctr, *rc_;
    LFR_TAKE(rounds_arena, kRoundsArena, bits, unsigned long long, (size_t)N * W); LFR_TAKE(rounds_arena, kRoundsArena, minpos, unsigned long long, N);
    LFR_TAKE(rounds_arena, kRoundsArena, pa, Pending, M); LFR_TAKE(rounds_arena, kRoundsArena, pb, Pending, M);
    LFR_TAKE(rounds_arena, kRoundsArena, ctr, uint32_t, 64);
    LFR_HIP_TRY(hipMemsetAsync(bits, 0, bits_bytes, st));
    LFR_HIP_TRY(hipMemsetAsync(minpos, 0xff, 8 * (size_t)N, st));
    LFR_HIP_TRY(hipMemsetAsync(ctr, 0, 4 * 64, st));
    uint32_t *h_ctr = h_counts + CNT_HOST_ROUNDS;
    // The ordered list goes through the rounds in PREFIX BLOCKS (2 N positions, then doubling): the sequential rule finishes
    // a prefix before it looks at the rest, so rounds over a block alone are exact, and a match is only carried through the
    // rounds of its own block.  With the whole list pending at once every match was re-evaluated each round until its
    // endpoints had met - 1.2e8 evaluations for config 5's 5.3 M matches (58 rounds); the tracks assemble from the first
    // few hundred thousand matches and what comes later retires in its block's first round: a twelfth of the work in a
    // simulation of this schedule, a few rounds more.
    const int64_t first_block = knobs.rounds_first_block ? knobs.rounds_first_block : std::max<int64_t>(2 * N, 1024);
    int64_t rounds = 0, launched = 0;
    // (one launch per round: grid-barrier and one-XCD forms measured slower - profiles/r03_rounds_cooperative.txt, r06_ab/rounds_tail.txt)
    LFR_TAKE(rounds_arena, kRoundsArena, rc_, uint32_t, kRoundBatch + 2);
    LFR_HIP_TRY(hipMemsetAsync(rc_, 0, 4 * (kRoundBatch + 2), st));
    for (int64_t k_lo = 0, size = first_block; k_lo < M; k_lo += size, size *= 2) {
        const int64_t k_hi = std::min(M, k_lo + size);
        LFR_HIP_TRY(hipMemsetAsync(rc_ + kRoundBatch, 0, 4, st));
        hipLaunchKernelGGL(k_large_pending, grid_for_items(k_hi - k_lo, kAppendItems), dim3(kThreads), 0, st, k_lo, k_hi, knobs.serial_limit, ord.flags, ord.segid, ord.starts,
                           ord.order, n1, n2, dg->node_image, W, bits, pa, rc_ + kRoundBatch);
        LFR_HIP_TRY(hipMemcpyAsync(h_ctr, rc_ + kRoundBatch, 4, hipMemcpyDeviceToHost, st));
        LFR_HIP_TRY(stream_wait(st));
        uint32_t bound = h_ctr[0];
        while (bound > 0) {
            if (launched + kRoundBatch > kMaxRounds) return use_host("round limit");   // a path-shaped dependency chain: sequential anyway
            hipLaunchKernelGGL(k_round_counters_shift, dim3(1), dim3(64), 0, st, rc_, kRoundBatch);
            for (int j = 0; j < kRoundBatch; ++j, ++launched) {
                const unsigned long long round_hi = (unsigned long long)(kMaxRounds - launched) << 32;
                hipLaunchKernelGGL(k_round_eval, grid_for_items(bound, kEvalItems), dim3(kThreads), 0, st, rc_ + j, pa, uf.par, bits, W, round_hi, minpos, pb, rc_ + j + 1);
                hipLaunchKernelGGL(k_round_accept, grid_for(bound), dim3(kThreads), 0, st, rc_ + j + 1, pb, round_hi, minpos, uf.par, uf.cnt, bits, W, ctr + 3);
                std::swap(pa, pb);
            }
            LFR_HIP_TRY(hipMemcpyAsync(h_ctr, rc_, 4 * (kRoundBatch + 1), hipMemcpyDeviceToHost, st));
            LFR_HIP_TRY(stream_wait(st));
            for (int j = 0; j < kRoundBatch; ++j) rounds += h_ctr[j] > 0 ? 1 : 0;
            if (knobs.trace > 2) fprintf(stderr, "lfr graph stage:   block [%lld, %lld) rounds ..%lld: pending %u -> %u\n", (long long)k_lo, (long long)k_hi, (long long)rounds, h_ctr[0], h_ctr[kRoundBatch]);
            bound = h_ctr[kRoundBatch];
        }
    }
    stats.kruskal_rounds = (double)rounds;
    return LFR_OK;                                 // (every round has been waited for: the rounds' arena goes back to the cache)
}

// 5. track ids (roots in ascending node index), sizes; then the roots
int Stage::tracks_and_roots(MatchOrder kind) {
    LFR_TAKE(arena, kStageArena, trk.rrank, uint32_t, N + 1);
    hipLaunchKernelGGL(k_root_flags, grid_for(N), dim3(kThreads), 0, st, N, uf.par, trk.rflag);
    LFR_HIP_TRY(exclusive_sum_one_launch(trk.rflag, trk.rrank, N + 1, scan_state + scan_words_m, st));
    hipLaunchKernelGGL(k_track_ids, grid_for(N), dim3(kThreads), 0, st, N, uf.par, trk.rrank, dp->track, trk.tsize, counts);
    LFR_HIP_TRY(hipEventRecord(ev[EV_TRACKS], st));
    // (small connected components only: in the ordered list of a giant one a wave's matches share no nodes - config 5: 0.40 ms grouped, 0.12 plain)
    if (has_large_components()) hipLaunchKernelGGL(k_scores, grid_for(M), dim3(kThreads), 0, st, M, n1, n2, sim, dp->track, trk.score);
    else hipLaunchKernelGGL(k_scores_grouped, grid_for(M), dim3(kThreads), 0, st, M, kind == MatchOrder::counted_streamed ? ord.srec : nullptr, ord.order, n1, n2, sim,
                            dp->track, trk.score);
    hipLaunchKernelGGL(k_best_score, grid_for(N), dim3(kThreads), 0, st, N, dp->track, trk.score, trk.best);
    hipLaunchKernelGGL(k_best_node, grid_for(N), dim3(kThreads), 0, st, N, dp->track, trk.score, trk.best, trk.bnode);
    hipLaunchKernelGGL(k_mark_roots, grid_for(N), dim3(kThreads), 0, st, N, counts, trk.bnode, dp->is_root);
    LFR_HIP_TRY(hipEventRecord(ev[EV_ROOTS], st));
    return LFR_OK;
}

// components of the track meta-graph, numbered by their smallest track (solve.cc:292-300).  The first time they ARE the connected
// components of step 1 and everything starts in the zero block; after a cut a union-find over the kept meta edges finds them
// (solve.cc:345-372), what the first pass filled is cleared and the prefix sum is the library's (the one-launch states are used up).
int Stage::label_components(bool after_cut) {
    if (!after_cut) {
        LFR_TAKE(arena, kStageArena, lab.mp, uint32_t, N); LFR_TAKE(arena, kStageArena, lab.crank, uint32_t, N + 1);
        hipLaunchKernelGGL(k_cc_min_track, grid_for(N), dim3(kThreads), 0, st, N, cc.label, dp->track, lab.mp_parent);
        hipLaunchKernelGGL(k_track_label, grid_for(N), dim3(kThreads), 0, st, N, cc.label, dp->track, lab.mp_parent, lab.mp);
    } else {
        hipLaunchKernelGGL(k_iota, grid_for(N), dim3(kThreads), 0, st, N, lab.mp_parent);
        hipLaunchKernelGGL(k_meta_union_cut, grid_for(M), dim3(kThreads), 0, st, M, n1, n2, dp->track, lab.gc, lab.mp_parent);
        hipLaunchKernelGGL(k_cc_labels, grid_for(N), dim3(kThreads), 0, st, N, lab.mp_parent, lab.mp);
        LFR_HIP_TRY(hipMemsetAsync(lab.cflag, 0, 4 * (size_t)(N + 1), st));
        LFR_HIP_TRY(hipMemsetAsync(lab.csize, 0, 4 * (size_t)N, st));
        LFR_HIP_TRY(hipMemsetAsync(counts + CNT_MAX_COMP, 0, 4, st));
    }
    hipLaunchKernelGGL(k_comp_flags, grid_for(N), dim3(kThreads), 0, st, N, counts, lab.mp, lab.cflag);
    if (after_cut) { const int rc = exclusive_sum(arena, lab.cflag, lab.crank, N + 1, st); if (rc != LFR_OK) return rc; }
    else LFR_HIP_TRY(exclusive_sum_one_launch(lab.cflag, lab.crank, N + 1, scan_state + scan_words_m + scan_words_n, st));
    hipLaunchKernelGGL(k_comp_sizes, grid_few(N), dim3(kThreads), 0, st, N, counts, lab.mp, lab.crank, trk.tsize, lab.csize);
    hipLaunchKernelGGL(k_max_csize, grid_few(N), dim3(kThreads), 0, st, N, counts, lab.csize);
    hipLaunchKernelGGL(k_node_comp, grid_for(N), dim3(kThreads), 0, st, N, dp->track, lab.mp, lab.crank, dp->comp);
    LFR_HIP_TRY(hipGetLastError());
    LFR_HIP_TRY(hipEventRecord(ev[after_cut ? EV_CUT_END : EV_COMPS], st));
    return LFR_OK;
}

int Stage::read_counts(const char *what) {         // the device's counts into the pinned block, waited for
    LFR_HIP_TRY(hipMemcpyAsync(h_counts, counts, 4 * CNT_WORDS, hipMemcpyDeviceToHost, st));
    LFR_HIP_TRY(stream_wait(st));
    lap(what);
    return LFR_OK;
}

void Stage::trace_fill_time() const {
    if (!knobs.trace) return;
    float a = 0.f;
    (void)hipEventElapsedTime(&a, ev[EV_BEGIN], ev[EV_FILLED]);
    fprintf(stderr, "lfr graph stage: device time of the memsets before the first kernel: %.3f ms (zero block %zu bytes)\n", a, zero_bytes);
}

void Stage::debug_dump() const {                   // LFR_DEBUG_DUMP: intermediates of the stage as raw files (debugging aid)
    if (!knobs.debug_dump) return;
    auto dump = [&](const char *name, const void *dptr, size_t bytes) {
        std::vector<char> h(bytes);
        (void)hipMemcpy(h.data(), dptr, bytes, hipMemcpyDeviceToHost);
        const std::string path = std::string(knobs.debug_dump) + "/" + name + ".bin";
        if (FILE *f = fopen(path.c_str(), "wb")) { fwrite(h.data(), 1, bytes, f); fclose(f); }
    };
    dump("order", ord.order, 4 * (size_t)M); dump("cc", cc.label, 4 * (size_t)N); dump("starts", ord.starts, 4 * (size_t)(std::min(N, M) + 2));
    dump("par", uf.par, 4 * (size_t)N); dump("track", dp->track, 4 * (size_t)N); dump("counts", counts, 64);
    dump("segid", ord.segid, 4 * (size_t)(M + 1)); dump("cnt", uf.cnt, 4 * (size_t)N);
}

// The size cap (solve.cc:311-343).  The deterministic bisection grows a region with a priority queue - sequential, and the meta
// graph is tiny next to the match graph - so it runs on the host (lfr_graph.cpp: cut_components_from_pairs), but only on what
// it needs: the device compacts the inter-track matches of the oversized components (a few per cent of a per cent
// of the matches), the host cuts, the subset of every affected track goes back, and the device re-labels.
int Stage::cut_oversized() {
    constexpr char kCutArena[] = "graph stage: cut arena";
    int rc;
    LFR_HIP_TRY(hipEventCreate(&ev[EV_CUT_BEGIN])); LFR_HIP_TRY(hipEventCreate(&ev[EV_CUT_END]));
    LFR_HIP_TRY(hipEventRecord(ev[EV_CUT_BEGIN], st));
    const int64_t T = h_counts[CNT_TRACKS];
    int32_t *tcomp;
    uint32_t *cut_n;
    LFR_TAKE(arena, kStageArena, tcomp, int32_t, T + 1); LFR_TAKE(arena, kStageArena, cut_n, uint32_t, 16); LFR_TAKE(arena, kStageArena, lab.gc, int32_t, T + 1);
    DevArena cut_arena;                            // (pair, similarity) of every inter-track match of an oversized component
    if (!cut_arena.init(ctx, 16 * (size_t)M + 65536)) return LFR_ERR_NOMEM;
    unsigned long long *pair_key;
    double *pair_sim;
    LFR_TAKE(cut_arena, kCutArena, pair_key, unsigned long long, M); LFR_TAKE(cut_arena, kCutArena, pair_sim, double, M);
    LFR_HIP_TRY(hipMemsetAsync(cut_n, 0, 64, st));
    hipLaunchKernelGGL(k_track_comp, grid_for(T), dim3(kThreads), 0, st, T, counts, lab.mp, lab.crank, tcomp);
    hipLaunchKernelGGL(k_cut_edges, grid_for_items(M, kAppendItems), dim3(kThreads), 0, st, M, n1, n2, sim, dp->track, tcomp, lab.csize, (uint32_t)max_nodes, pair_key, pair_sim, cut_n);
    LFR_HIP_TRY(hipMemcpyAsync(h_counts + CNT_HOST_CUT_EDGES, cut_n, 4, hipMemcpyDeviceToHost, st));
    LFR_HIP_TRY(stream_wait(st));
    const size_t n_cut_edges = h_counts[CNT_HOST_CUT_EDGES];
    // Meta edges (solve.cc:268-289,322-332): per unordered track pair the sum of the similarities -> int weight 100 * sum.
    // Sorted and summed on the device (radix sort + reduce-by-key: 0.7 M matches of config 5 took a host std::sort 60 ms);
    // sums of float32 values in fp64 are exact here, hence independent of the order of the additions.
    DevArena sum_arena;
    std::vector<unsigned long long> h_pair;
    std::vector<double> h_sum;
    std::vector<int32_t> h_tcomp((size_t)T), h_gc;
    std::vector<uint32_t> h_tsize((size_t)T);
    if (n_cut_edges) {
        if (!sum_arena.init(ctx, 64 * n_cut_edges + ((size_t)16 << 20))) return LFR_ERR_NOMEM;
        unsigned long long *key_s, *key_u;
        double *sim_s, *sim_u;
        LFR_TAKE(sum_arena, kCutArena, key_s, unsigned long long, n_cut_edges); LFR_TAKE(sum_arena, kCutArena, key_u, unsigned long long, n_cut_edges);
        LFR_TAKE(sum_arena, kCutArena, sim_s, double, n_cut_edges); LFR_TAKE(sum_arena, kCutArena, sim_u, double, n_cut_edges);
        int tbits = 1;
        while (((int64_t)1 << tbits) < T) ++tbits;
        if ((rc = sort_pairs(sum_arena, pair_key, key_s, pair_sim, sim_s, (int64_t)n_cut_edges, 0, 32 + tbits, st)) != LFR_OK) return rc;
        if ((rc = sum_by_key(sum_arena, key_s, key_u, sim_s, sim_u, cut_n + 1, (int64_t)n_cut_edges, st)) != LFR_OK) return rc;
        LFR_HIP_TRY(hipMemcpyAsync(h_counts + CNT_HOST_CUT_PAIRS, cut_n + 1, 4, hipMemcpyDeviceToHost, st));
        LFR_HIP_TRY(stream_wait(st));
        const size_t n_pairs = h_counts[CNT_HOST_CUT_PAIRS];
        h_pair.resize(n_pairs); h_sum.resize(n_pairs);
        LFR_HIP_TRY(hipMemcpyAsync(h_pair.data(), key_u, 8 * n_pairs, hipMemcpyDeviceToHost, st));
        LFR_HIP_TRY(hipMemcpyAsync(h_sum.data(), sim_u, 8 * n_pairs, hipMemcpyDeviceToHost, st));
    }
    LFR_HIP_TRY(hipMemcpyAsync(h_tcomp.data(), tcomp, 4 * (size_t)T, hipMemcpyDeviceToHost, st));
    LFR_HIP_TRY(hipMemcpyAsync(h_tsize.data(), trk.tsize, 4 * (size_t)T, hipMemcpyDeviceToHost, st));
    LFR_HIP_TRY(stream_wait(st));
    lap("cut: meta edges of the oversized components on the host");
    stats.n_cut_components = cut_components_from_pairs(h_tcomp, h_tsize, h_pair, h_sum, max_nodes, h_gc);
    lap("cut: recursive bisection");
    LFR_HIP_TRY(hipMemcpyAsync(lab.gc, h_gc.data(), 4 * (size_t)T, hipMemcpyHostToDevice, st));
    // drop the cut edges and re-label (solve.cc:345-372), the tail of the first labelling again
    if ((rc = label_components(true)) != LFR_OK) return rc;
    if ((rc = read_counts("cut: re-labelled")) != LFR_OK) return rc;      // (the staging vectors above die at scope end)
    return LFR_OK;
}

// stats and labels into the Problem: last, once every step has succeeded
int Stage::publish() {
    float ms = 0.f;
    LFR_HIP_TRY(hipEventElapsedTime(&ms, ev[EV_FILLED], ev[EV_TRACKS])); stats.tracks_ms = ms;
    LFR_HIP_TRY(hipEventElapsedTime(&ms, ev[EV_TRACKS], ev[EV_ROOTS])); stats.roots_ms = ms;
    LFR_HIP_TRY(hipEventElapsedTime(&ms, ev[EV_ROOTS], ev[EV_COMPS])); stats.graph_cut_ms = ms;
    if (ev[EV_CUT_END]) { LFR_HIP_TRY(hipEventElapsedTime(&ms, ev[EV_CUT_BEGIN], ev[EV_CUT_END])); stats.graph_cut_ms += ms; }
    stats.n_tracks = h_counts[CNT_TRACKS]; stats.max_track_size = h_counts[CNT_MAX_TRACK];
    stats.n_components = h_counts[CNT_COMPS]; stats.max_component_size = h_counts[CNT_MAX_COMP];
    dp->max_cc_matches = h_counts[CNT_MAX_SEG];
    p.stats = stats;
    std::lock_guard<std::mutex> lk(p.label_mu);
    p.track.clear(); p.comp.clear(); p.is_root.clear();
    p.host_labels_valid = false;                   // fetched from HBM on demand
    p.devs.assign((size_t)device + 1, nullptr);
    p.devs[device] = dp;
    return LFR_OK;
}

}  // namespace

int graph_stage_on_device(const Graph &g, int64_t max_nodes, int device, bool stage_flows, Problem &p, int shard_rank, int shard_world) {
    Stage s(g, p, device);
    p.g = &g;
    p.stats = lfr_problem_stats{};
    p.host_batch = false;
    { std::lock_guard<std::mutex> lk(p.label_mu); p.devs.clear(); }
    if (s.N == 0) { p.track.clear(); p.comp.clear(); p.is_root.clear(); p.host_labels_valid = true; return LFR_OK; }
    if (s.N >= ((int64_t)1 << 31) || s.M >= ((int64_t)1 << 30)) return s.use_host("2^31 nodes / 2^30 matches or more");
    if (!g.sims_sum_exactly) return s.use_host("similarity sums would round");      // atomics would round in an order-dependent way: the reference's sequential sums run on the host
    s.max_nodes = max_nodes > 0 ? max_nodes : (int64_t)g.image_names.size();
    int rc = ensure_dev_graph(g, device, stage_flows, s.dg);     // endpoints on s_main now; the flows start travelling on s_copy
    if (rc != LFR_OK) return rc;
    s.ctx = s.dg->ctx;
    LFR_HIP_TRY(hipSetDevice(device));
    s.st = s.ctx->s_main;
    s.lap("device graph ready");
    if ((rc = s.shard_if_balanced(shard_rank, shard_world)) != LFR_OK) return rc;
    if ((rc = s.prepare()) != LFR_OK) return rc;
    if ((rc = s.connected_components()) != LFR_OK) return rc;
    MatchOrder order;
    if ((rc = s.order_matches(order)) != LFR_OK) return rc;
    if ((rc = s.union_find_small(order)) != LFR_OK) return rc;
    s.lap("sorts / connected components / small-component union-find enqueued");
    // (first read-back: are there large components? - the counting road has read the counts already)
    if (order != MatchOrder::counted_streamed && (rc = s.read_counts("first read-back")) != LFR_OK) return rc;
    if (s.h_counts[CNT_LONG_TIE]) {
        // a long run of equal similarities: the exact order from the three sorts (the segments - which matches, where - are the same:
        // flags, segment ids and starts stay), the union-find of the small components again from scratch
        order = MatchOrder::three_sorts;
        if ((rc = s.three_sorts()) != LFR_OK || (rc = s.union_find_small(order)) != LFR_OK) return rc;
        s.stats.tie_resorts = 1.0;
        s.lap("three-sort order after a long tie");
    }
    s.trace_fill_time();
    if (s.has_large_components() && (rc = s.union_find_rounds()) != LFR_OK) return rc;
    if ((rc = s.tracks_and_roots(order)) != LFR_OK) return rc;
    if ((rc = s.label_components(false)) != LFR_OK) return rc;
    s.lap("tracks / roots / components enqueued");
    if ((rc = s.read_counts("final read-back")) != LFR_OK) return rc;      // the one read-back of the stage
    s.debug_dump();
    if ((int64_t)s.h_counts[CNT_MAX_COMP] > s.max_nodes && (rc = s.cut_oversized()) != LFR_OK) return rc;
    return s.publish();
}

int graph_make_resident(const Graph &g, int device) {
    std::shared_ptr<DevGraph> dg;
    return ensure_dev_graph(g, device, true, dg);
}

}  // namespace lfr

// =================================================================================================
// C ABI: device residency of the graph
// =================================================================================================
extern "C" {

int lfr_graph_to_device(const lfr_graph *g, int device) {
    if (!g) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    return lfr::graph_make_resident(g->g, device);
}

int lfr_graph_evict_device(const lfr_graph *g) {
    if (!g) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(g->g.dev_mu);
    g->g.devgs.clear();                               // problems / batches built from it keep their own reference
    return LFR_OK;
}

}  // extern "C"
