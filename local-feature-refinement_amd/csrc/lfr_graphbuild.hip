// lfr_graph_from_device_arrays: the match graph numbered ON the GPU from per-match arrays that never left it (feature indices,
// similarities, flows), bit-identical to the host numbering of lfr_graph_from_arrays_device_flows (lfr_wire.cpp: one hash-map insert
// per endpoint, serial), and installed as the graph's HBM copy (DevGraph) so that nothing is uploaded again.
//
// The host keeps what is pair level: which pairs survive the banned images, the interned image ids (order of first appearance, first
// fact wins), and where every kept pair's matches start - in the caller's rows and in the graph.  One 16-byte row per kept pair goes
// to the device; the rest is five passes over E = 2 x matches endpoint entries on the context's main stream:
//   1. expand      one thread per graph match g: its pair (binary search over the kept pairs' graph offsets), flow_row[g], sim[g], and
//                  the two entries (key = image << 32 | feature, position 2g / 2g + 1: node1 before node2, solve.cc:474-475)
//   2. sort        stable, (u64, u32), bits [0, 32 + bits(#images)): the entries are created in position order, so the head of every
//                  run of equal keys is that key's FIRST appearance
//   3. head flags  run_flag[j] = entry j heads a run; pos_flag[p] = position p is some key's first appearance.  The exclusive sum of
//                  run_flag numbers the runs (its last element is N), that of pos_flag ranks the first appearances: the node ids
//   4. heads       the head of run r writes run_node[r] = rank of its position, and the node's image and feature
//      scatter     every entry reads its run's node id and writes n1[g] or n2[g]; no thread walks a run, so a node of any degree
//                  costs the same per entry
//   5. read back   N (one 64-byte block), endpoints, similarities, rows and the node arrays: the graph's host mirror, then finish()
// No spin waits and no hand-offs between workgroups beyond the look-back of the scan driver (lfr_sort.hpp).  The passes are memory
// bound and elementwise: one entry (or one match = two entries, a 16-byte key store) per thread, grids sized from the data.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "lfr_assemble.hpp"

namespace lfr {

namespace {

constexpr int kThreads = kPipeThreads;
enum { SPAN_EXPAND = 0, SPAN_SORT, SPAN_SCANS, SPAN_SCATTER, SPAN_MIRROR, SPAN_FINISH, SPAN_PAIRS, SPAN_COUNT };
thread_local double t_spans[SPAN_COUNT] = {0, 0, 0, 0, 0, 0, 0};

// one kept, non-empty pair: its matches are graph matches [g_begin, next row's g_begin) = caller rows [row_begin, ...)
struct alignas(16) PairRow { uint32_t g_begin, row_begin; int32_t img1, img2; };
static_assert(sizeof(PairRow) == 16, "PairRow must be 16 bytes");

__global__ __launch_bounds__(kThreads) void k_gb_expand(int64_t M, int n_rows, const PairRow *__restrict__ rows, const uint32_t *__restrict__ feat1,
                                                         const uint32_t *__restrict__ feat2, const float *__restrict__ sim, uint32_t *__restrict__ flow_row,
                                                         float *__restrict__ o_sim, ulonglong2 *__restrict__ keys, uint2 *__restrict__ pos) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= M) return;
    int lo = 0, hi = n_rows - 1;                       // last row with g_begin <= g (rows[0].g_begin == 0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)rows[mid].g_begin <= g) lo = mid; else hi = mid - 1;
    }
    const PairRow r = rows[lo];
    const uint32_t row = r.row_begin + (uint32_t)(g - (int64_t)r.g_begin);
    flow_row[g] = row;
    o_sim[g] = sim[row];
    keys[g] = make_ulonglong2(((unsigned long long)(uint32_t)r.img1 << 32) | feat1[row], ((unsigned long long)(uint32_t)r.img2 << 32) | feat2[row]);
    pos[g] = make_uint2((uint32_t)(2 * g), (uint32_t)(2 * g + 1));
}

// run_flag over E + 1 entries (the last one 0: the sum's last element is the number of runs); pos_flag over E (every position is
// the value of exactly one entry, so the array is written in full)
__global__ __launch_bounds__(kThreads) void k_gb_head_flags(int64_t E, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ pos,
                                                             uint32_t *__restrict__ run_flag, uint32_t *__restrict__ pos_flag) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > E) return;
    if (j == E) { run_flag[j] = 0u; return; }
    const uint32_t head = j == 0 || keys[j] != keys[j - 1] ? 1u : 0u;
    run_flag[j] = head;
    pos_flag[pos[j]] = head;
}

__global__ __launch_bounds__(kThreads) void k_gb_heads(int64_t E, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ pos,
                                                        const uint32_t *__restrict__ run_flag, const uint32_t *__restrict__ run_index,
                                                        const uint32_t *__restrict__ pos_rank, uint32_t *__restrict__ run_node,
                                                        int32_t *__restrict__ node_image, uint32_t *__restrict__ node_feat, uint32_t *__restrict__ counts) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= E) return;
    if (j == 0) counts[0] = run_index[E];              // N
    if (!run_flag[j]) return;
    const uint32_t id = pos_rank[pos[j]];              // rank of this key's first appearance among all first appearances
    const unsigned long long key = keys[j];
    run_node[run_index[j]] = id;
    node_image[id] = (int32_t)(key >> 32);
    node_feat[id] = (uint32_t)key;
}

__global__ __launch_bounds__(kThreads) void k_gb_scatter(int64_t E, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ run_flag,
                                                          const uint32_t *__restrict__ run_index, const uint32_t *__restrict__ run_node,
                                                          uint32_t *__restrict__ n1, uint32_t *__restrict__ n2) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= E) return;
    const uint32_t id = run_node[run_index[j] + run_flag[j] - 1u];       // inclusive sum - 1 = the run of entry j
    const uint32_t p = pos[j];
    ((p & 1u) ? n2 : n1)[p >> 1] = id;
}

// `bytes`: what the driver's size query returned for this n and end_bit (the caller sized the arena with it)
int sort_entries(DevArena &arena, size_t bytes, const unsigned long long *kin, unsigned long long *kout, const uint32_t *vin, uint32_t *vout, int64_t n, int end_bit, hipStream_t st) {
    void *tmp = arena.take(bytes);
    if (!tmp) { set_error("graph build: device arena exhausted (sort of %lld entries)", (long long)n); return LFR_ERR_NOMEM; }
    LFR_HIP_TRY(sort_pairs_raw(tmp, bytes, kin, kout, vin, vout, n, 0, end_bit, st));
    return LFR_OK;
}

struct Spans {                                         // device spans between events, only under LFR_GRAPHBUILD_SPANS=1
    DevCtx *ctx;
    bool on;
    hipEvent_t ev[SPAN_SCATTER + 2] = {};
    explicit Spans(DevCtx *c) : ctx(c) {
        static const bool want = [] { const char *e = std::getenv("LFR_GRAPHBUILD_SPANS"); return e && e[0] == '1'; }();
        on = want;
        for (hipEvent_t &e : ev) if (on && !(e = ctx->event_acquire(true))) on = false;
    }
    ~Spans() { for (hipEvent_t e : ev) if (e) ctx->event_release(e, true); }
    void mark(int i, hipStream_t st) { if (on) (void)hipEventRecord(ev[i], st); }
    void collect() {                                   // (after the stream has been waited for)
        for (int i = 0; i <= SPAN_SCATTER; ++i) {
            float ms = 0.f;
            t_spans[i] = on && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess ? (double)ms : 0.0;
        }
    }
};

constexpr char kBuildArena[] = "graph build: device arena";

// the device part: g holds the images, `rows` the kept pairs; fills the per-match and per-node host arrays and g.devgs[device]
int number_on_device(Graph &g, int device, const std::vector<PairRow> &rows, int64_t M, const uint32_t *feat1, const uint32_t *feat2, const float *sim) {
    DevCtx *ctx = dev_ctx(device);
    if (!ctx) return LFR_ERR_HIP;
    LFR_HIP_TRY(hipSetDevice(device));
    hipStream_t st = ctx->s_main;
    const int64_t E = 2 * M;
    int image_bits = 1;
    while (((int64_t)1 << image_bits) < (int64_t)g.image_names.size()) ++image_bits;

    std::shared_ptr<DevGraph> dg(new DevGraph());
    dg->ctx = ctx; dg->M = M;
    if (!dg->slab.init(ctx, (size_t)16 * M + ((size_t)1 << 16))) return LFR_ERR_NOMEM;
    LFR_TAKE(dg->slab, "graph build: graph slab", dg->n1, uint32_t, M); LFR_TAKE(dg->slab, "graph build: graph slab", dg->n2, uint32_t, M);
    LFR_TAKE(dg->slab, "graph build: graph slab", dg->sim, float, M); LFR_TAKE(dg->slab, "graph build: graph slab", dg->flow_row, uint32_t, M);

    // temporaries of this call: 36 bytes per entry, the sort's own buffers (its size query: <= 12 bytes per entry and the digit
    // tables), the zero block and the pair rows
    const size_t scan_words = scan_state_words(E + 1);
    size_t sort_bytes = 0;
    LFR_HIP_TRY(sort_pairs_raw(nullptr, sort_bytes, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, E, 0, 32 + image_bits, st));
    DevArena arena;
    if (!arena.init(ctx, (size_t)44 * E + sort_bytes + 16 * scan_words + 16 * rows.size() + ((size_t)1 << 16))) return LFR_ERR_NOMEM;
    uint32_t *counts = nullptr, *pos_in = nullptr, *pos = nullptr, *run_flag = nullptr, *run_index = nullptr, *pos_flag = nullptr, *pos_rank = nullptr;
    unsigned long long *scan_state = nullptr, *keys_in = nullptr, *keys = nullptr;
    PairRow *d_rows = nullptr;
    const size_t zero_mark = arena.top;                // counts and the look-back states of the two prefix sums start at zero
    LFR_TAKE(arena, kBuildArena, counts, uint32_t, 16);
    LFR_TAKE(arena, kBuildArena, scan_state, unsigned long long, 2 * scan_words);
    const size_t zero_bytes = arena.top - zero_mark;
    LFR_TAKE(arena, kBuildArena, d_rows, PairRow, rows.size());
    LFR_TAKE(arena, kBuildArena, keys_in, unsigned long long, E); LFR_TAKE(arena, kBuildArena, keys, unsigned long long, E);
    LFR_TAKE(arena, kBuildArena, pos_in, uint32_t, E); LFR_TAKE(arena, kBuildArena, pos, uint32_t, E);
    LFR_TAKE(arena, kBuildArena, run_flag, uint32_t, E + 1); LFR_TAKE(arena, kBuildArena, run_index, uint32_t, E + 1);
    LFR_TAKE(arena, kBuildArena, pos_flag, uint32_t, E); LFR_TAKE(arena, kBuildArena, pos_rank, uint32_t, E);
    // free once the sort has read them: the unsorted keys hold the node arrays (N <= E: 2 x 4 E bytes), the unsorted positions run_node
    int32_t *t_node_image = reinterpret_cast<int32_t *>(keys_in);
    uint32_t *t_node_feat = reinterpret_cast<uint32_t *>(keys_in) + E, *run_node = pos_in;
    size_t pin_bytes = 0;
    uint32_t *h_counts = (uint32_t *)ctx->pinned_acquire(64, &pin_bytes);
    if (!h_counts) return LFR_ERR_NOMEM;
    struct PinGuard { DevCtx *c; void *p; size_t b; ~PinGuard() { c->pinned_release(p, b); } } pin_guard{ctx, h_counts, pin_bytes};
    Spans spans(ctx);
    // Every return below this line that is not the last one leaves work enqueued that reads or writes the arenas, the pinned block
    // and the graph's host arrays: the stream is waited for before any of them is let go (declared last: destroyed first).
    struct WaitOnError { hipStream_t st; bool armed; ~WaitOnError() { if (armed) (void)stream_wait(st); } } wait_on_error{st, true};

    LFR_HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), sizeof(PairRow) * rows.size(), hipMemcpyHostToDevice, st));
    FillRegions fr;
    fr.add(arena.base + zero_mark, zero_bytes, 0);
    LFR_HIP_TRY(fill_regions(fr, st));
    spans.mark(SPAN_EXPAND, st);
    hipLaunchKernelGGL(k_gb_expand, pipe_grid(M), dim3(kThreads), 0, st, M, (int)rows.size(), d_rows, feat1, feat2, sim, dg->flow_row, dg->sim,
                       reinterpret_cast<ulonglong2 *>(keys_in), reinterpret_cast<uint2 *>(pos_in));
    spans.mark(SPAN_SORT, st);
    {
        const int rc = sort_entries(arena, sort_bytes, keys_in, keys, pos_in, pos, E, 32 + image_bits, st);
        if (rc != LFR_OK) return rc;
    }
    spans.mark(SPAN_SCANS, st);
    hipLaunchKernelGGL(k_gb_head_flags, pipe_grid(E + 1), dim3(kThreads), 0, st, E, keys, pos, run_flag, pos_flag);
    LFR_HIP_TRY(exclusive_sum_one_launch(run_flag, run_index, E + 1, scan_state, st));
    LFR_HIP_TRY(exclusive_sum_one_launch(pos_flag, pos_rank, E, scan_state + scan_words, st));
    spans.mark(SPAN_SCATTER, st);
    hipLaunchKernelGGL(k_gb_heads, pipe_grid(E), dim3(kThreads), 0, st, E, keys, pos, run_flag, run_index, pos_rank, run_node, t_node_image, t_node_feat, counts);
    hipLaunchKernelGGL(k_gb_scatter, pipe_grid(E), dim3(kThreads), 0, st, E, pos, run_flag, run_index, run_node, dg->n1, dg->n2);
    LFR_HIP_TRY(hipGetLastError());
    spans.mark(SPAN_SCATTER + 1, st);

    // the host mirror: 16 bytes per match behind the 64-byte read-back of N, 8 bytes per node once N is known
    if (spans.on) LFR_HIP_TRY(stream_wait(st));        // (so that the mirror's span starts when the device is done)
    const auto t0 = std::chrono::steady_clock::now();
    g.m_node1.resize(M); g.m_node2.resize(M); g.m_sim.resize(M); g.m_flow_row.resize(M);       // (while the device works)
    LFR_HIP_TRY(hipMemcpyAsync(h_counts, counts, 64, hipMemcpyDeviceToHost, st));
    LFR_HIP_TRY(hipMemcpyAsync(g.m_node1.data(), dg->n1, (size_t)4 * M, hipMemcpyDeviceToHost, st));
    LFR_HIP_TRY(hipMemcpyAsync(g.m_node2.data(), dg->n2, (size_t)4 * M, hipMemcpyDeviceToHost, st));
    LFR_HIP_TRY(hipMemcpyAsync(g.m_sim.data(), dg->sim, (size_t)4 * M, hipMemcpyDeviceToHost, st));
    LFR_HIP_TRY(hipMemcpyAsync(g.m_flow_row.data(), dg->flow_row, (size_t)4 * M, hipMemcpyDeviceToHost, st));
    LFR_HIP_TRY(stream_wait(st));
    spans.collect();
    const int64_t N = (int64_t)h_counts[0];
    if (N < 1 || N > E) { set_error("graph build: internal error, %lld nodes for %lld matches", (long long)N, (long long)M); return LFR_ERR_HIP; }
    if (!dg->node_slab.init(ctx, (size_t)4 * N + 4096)) return LFR_ERR_NOMEM;
    LFR_TAKE(dg->node_slab, "graph build: node slab", dg->node_image, int32_t, N);
    dg->N = N; dg->N_cap = N;
    g.node_image.resize(N); g.node_feat.resize(N);
    LFR_HIP_TRY(hipMemcpyAsync(dg->node_image, t_node_image, (size_t)4 * N, hipMemcpyDeviceToDevice, st));
    LFR_HIP_TRY(hipMemcpyAsync(g.node_image.data(), t_node_image, (size_t)4 * N, hipMemcpyDeviceToHost, st));
    LFR_HIP_TRY(hipMemcpyAsync(g.node_feat.data(), t_node_feat, (size_t)4 * N, hipMemcpyDeviceToHost, st));
    LFR_HIP_TRY(stream_wait(st));                      // (the temporaries go back to the cache behind this)
    wait_on_error.armed = false;
    t_spans[SPAN_MIRROR] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

    dg->disp1 = g.dev_disp1; dg->disp2 = g.dev_disp2; dg->flows_external = true;
    std::lock_guard<std::mutex> lk(g.dev_mu);
    if ((int)g.devgs.size() <= device) g.devgs.resize(device + 1);
    g.devgs[device] = dg;
    return LFR_OK;
}

int graph_from_device_arrays(Graph &g, int32_t n_images, const char *const *image_names, const float *image_facts, int64_t n_pairs,
                             const int32_t *pair_img1, const int32_t *pair_img2, const int64_t *pair_off, const uint32_t *feat1, const uint32_t *feat2,
                             const float *sim, const void *disp1, const void *disp2, int device, const char *const *banned, int n_banned) {
    for (double &s : t_spans) s = 0.0;
    if (n_images < 0 || n_pairs < 0 || device < 0 || (n_pairs > 0 && (!pair_img1 || !pair_img2 || !pair_off)) || (n_images > 0 && (!image_names || !image_facts)) ||
        (n_banned > 0 && !banned)) {
        set_error("bad argument");
        return LFR_ERR_ARG;
    }
    const int64_t M_in = n_pairs ? pair_off[n_pairs] : 0;
    if (n_pairs && pair_off[0] < 0) { set_error("pair_off must start at a row >= 0"); return LFR_ERR_ARG; }
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int32_t a = pair_img1[p], b = pair_img2[p];
        if (a < 0 || a >= n_images || b < 0 || b >= n_images) { set_error("image index out of range"); return LFR_ERR_ARG; }
        if (pair_off[p + 1] < pair_off[p]) { set_error("pair_off must not decrease"); return LFR_ERR_ARG; }
    }
    if (M_in > 0 && (!feat1 || !feat2 || !sim || !disp1 || !disp2)) { set_error("bad argument: a per-match device array is NULL"); return LFR_ERR_ARG; }
    if (M_in >= ((int64_t)1 << 30)) { set_error("graph too large for the device pipeline"); return LFR_ERR_UNSUPPORTED; }

    const auto t_pairs = std::chrono::steady_clock::now();
    std::set<std::string> ban;
    for (int i = 0; i < n_banned; ++i) ban.insert(banned[i]);
    // per caller image: banned?, and its interned id once it has been seen (-1 before).  Interning is by NAME and idempotent, so the
    // first use of an index does exactly what the host numbering does at that pair and later uses change nothing - and the loop over
    // the pairs makes no string, set or map look-up per pair
    std::vector<int32_t> seen_as((size_t)n_images, -1);
    std::vector<uint8_t> is_banned((size_t)n_images, 0);
    if (!ban.empty()) for (int32_t i = 0; i < n_images; ++i) is_banned[i] = ban.count(image_names[i]) ? 1 : 0;
    std::vector<PairRow> rows;
    int64_t M = 0;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int32_t a = pair_img1[p], b = pair_img2[p];
        if (is_banned[a] || is_banned[b]) continue;
        if (seen_as[a] < 0) seen_as[a] = g.intern_image(image_names[a], image_facts[a]);        // image 1 before image 2
        if (seen_as[b] < 0) seen_as[b] = g.intern_image(image_names[b], image_facts[b]);
        const int32_t i1 = seen_as[a], i2 = seen_as[b];
        const int64_t n = pair_off[p + 1] - pair_off[p];
        if (n == 0) continue;                           // (an empty pair still brings its images)
        rows.push_back(PairRow{(uint32_t)M, (uint32_t)pair_off[p], i1, i2});
        M += n;
    }
    g.dev_disp1 = (const float *)disp1; g.dev_disp2 = (const float *)disp2; g.dev_flows_device = device;
    t_spans[SPAN_PAIRS] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_pairs).count();
    if (M > 0) {
        const int rc = number_on_device(g, device, rows, M, feat1, feat2, sim);
        if (rc != LFR_OK) return rc;
    }
    const auto t0 = std::chrono::steady_clock::now();
    g.finish();
    t_spans[SPAN_FINISH] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return LFR_OK;
}

}  // namespace

}  // namespace lfr

extern "C" {

int lfr_graph_from_device_arrays(int32_t n_images, const char *const *image_names, const float *image_facts,
                                 int64_t n_pairs, const int32_t *pair_img1, const int32_t *pair_img2, const int64_t *pair_off,
                                 const uint32_t *feat1_device, const uint32_t *feat2_device, const float *sim_device,
                                 const void *disp1_device, const void *disp2_device, int device,
                                 const char *const *banned, int n_banned, lfr_graph **out) {
    if (!out) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    *out = nullptr;
    lfr_graph *h = new lfr_graph();
    const int rc = lfr::graph_from_device_arrays(h->g, n_images, image_names, image_facts, n_pairs, pair_img1, pair_img2, pair_off, feat1_device,
                                                 feat2_device, sim_device, disp1_device, disp2_device, device, banned, n_banned);
    if (rc != LFR_OK) { delete h; return rc; }
    *out = h;
    return LFR_OK;
}

int lfr_debug_graph_build_spans(double *ms, int n) {
    if (!ms || n < 0) { lfr::set_error("bad argument"); return LFR_ERR_ARG; }
    for (int i = 0; i < n; ++i) ms[i] = i < lfr::SPAN_COUNT ? lfr::t_spans[i] : 0.0;
    return LFR_OK;
}

}  // extern "C"
