// What the solver's translation units share (internal): the kernel argument blocks, the layout of the control words that kernels and
// host code both touch, the batch (lfr_batch, include/lfr.h's opaque handle), the state of a pass that runs after a solve (PassState)
// and the host-side interface between the units.  No kernel bodies.
//   lfr_solve.hip        the forward kernels, their debug probes, and the launch functions declared in this header
//   lfr_batch.hip        batch creation, the launch plan of lfr_batch_solve (packed_ranges deals the packed launch), its diagnostic
//                        read-backs and statistics, the PassState functions, timing, downloads, warm-up, multi-GPU entry points
//   lfr_inputs.hip       new flows / similarities into a live batch (lfr_batch_set_inputs) and the record -> directed-edge map
// the analysis passes, each its kernels and launches; their packed kernels share one frame (lfr_packed_frame.hpp: the classes'
// traits from lfr_internal.hpp's table, the dispatcher, the group identity) and their host code the helpers at the end of this header:
//   lfr_evaluate.hip     cost, gradient, residuals and loss weights at given positions (lfr_batch_evaluate) and their vector-Jacobian
//                        product (lfr_batch_evaluate_vjp)
//   lfr_hessian_product.hip   matrix-free H v at given positions (lfr_batch_hessian_product)
//   lfr_hessian_solve.hip     matrix-free (H + damping I) y = b by preconditioned conjugate gradients (lfr_batch_hessian_solve)
//   lfr_jvp.hip          forward-mode sensitivity of the positions (lfr_batch_jvp)
//   lfr_backward.hip     implicit-gradient backward pass (lfr_batch_backward)
//   lfr_covariance.hip   per-keypoint and per-match covariance (lfr_batch_covariance, lfr_batch_covariance_matches)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "lfr_internal.hpp"

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            lfr::set_error("%s failed: %s", #expr, hipGetErrorString(_e));                    \
            return LFR_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

namespace lfr {

struct CompInfoDev {
    int32_t iterations, termination, n_successful, n_ls_evals, n_cand_evals, exec_passes;
    double final_cost;
};
static_assert(sizeof(CompInfoDev) == 32, "CompInfoDev layout");

struct KernelArgs {
    const CompDesc *descs;
    const EdgeRec *edges;
    const uint32_t *node_ids;
    double *positions;          // 2 * n_nodes of the whole graph
    CompInfoDev *infos;
    const lfr::NodeInc *node_inc;   // parallel to node_ids
    const uint32_t *in_idx;     // parallel to edges
    double *workspace;          // workgroup kernels: per-edge scratch (+ packed matrices for the HBM variant)
    const uint64_t *ws_off;     // per desc: packed-matrix offset (HBM variant)
    const uint64_t *es_off;     // per desc: per-edge scratch offset (8 doubles per edge)
    unsigned long long *prof;   // -DLFR_PROFILE_PHASES: per-class cycle counters [cls*8 + phase]
    unsigned int *queue;        // workgroup classes: next component of the class (one counter per class, zeroed per solve)
    const uint32_t *wg_order;   // workgroup classes: descriptors in the order the queue hands them out (longest expected first)
    int wg_begin;               // first descriptor of the workgroup classes (wg_order[0] belongs to it)
    int desc_begin, desc_end;
    int tukey_variant;
    int scratch_sweep;         // 1: the workgroup kernels use the scratch sweep of rounds 1-2 (LFR_SCRATCH_SWEEP=1 at batch creation; A/B and tests)
    int cls;
    // fused gather (packed classes of a device-assembled whole batch): record p is directed edge edge_ref[p] of the graph - flow row
    // (f_row ? f_row[m] : m) of f_disp2 (even ids) / f_disp1 (odd ids), similarity f_sim[m], m = id >> 1 - with local indices edge_word[p]
    const uint32_t *edge_ref, *edge_word, *f_row;
    const float *f_disp1, *f_disp2, *f_sim;
    // elimination-tree class: teams of workgroups per component (nullptr: one workgroup per component); team_work[k]: smallest
    // hand-out key (k_wg_order_keys' `work`) solved by 2 << k workgroups
    unsigned int *team_ctl;
    double *team_red;
    uint32_t team_work[3];
    uint32_t team_epoch;        // differs between launches that share the reduction slots
    uint32_t team_patience_us;  // teams that cannot form for this long with nobody at work: the launch goes on one workgroup per component (LFR_TEAM_PATIENCE_MS)
    const double *x_start;      // lfr_batch_solve_from: 2 * n_nodes start values in the layout of `positions` (may BE positions); nullptr: the origin
    unsigned long long *trace;  // -DLFR_TRACE_TREE: [0] = words used, then {s_memtime, type << 56 | wave of the team << 48 | iteration << 32 | column} pairs
};

// ---- control words: the ONE statement of where they live, for the kernels (lfr_solve.hip) and for the host code that zeroes and reads
// them.  What the team words mean: the comment above TeamCtx in lfr_solve.hip. ----
// KernelArgs::team_ctl, 32-bit words, zeroed per solve
constexpr int kTeamXccs = 8;                 // XCDs a launch registers with
constexpr int kCtlRegisteredXcc = 0;         // [0 .. kTeamXccs): workgroups registered per XCC
constexpr int kCtlRegistered = 8;            // registered in total
constexpr int kCtlAbort = 9;                 // a bounded spin ran out somewhere: every wait gives up
constexpr int kCtlTeamRuns = 10;             // components solved by a team (lfr_batch_team_runs)
constexpr int kCtlSolo = 11;                 // SOLO mode
constexpr int kCtlAtWork = 12;               // components being solved right now
constexpr int kCtlOffSize = 13;              // components solved off their team size (lfr_batch_team_fallbacks)
constexpr int kCtlMailbox = 16;              // [kCtlMailbox + kCtlUnitWords * unit + member]: mailbox of a unit's member
constexpr int kCtlUnitWords = 16;            // words per unit: mailboxes, then ...
constexpr int kCtlUnitArrival = 8;           // ... from here the arrival counters, one per leader rank
static_assert(kTeamXccs <= kCtlRegistered && kCtlOffSize < kCtlMailbox, "team control words");
// KernelArgs::queue, the queue block: 32-bit words, zeroed per solve - word cls is the next component of workgroup class cls
constexpr int kQueueWords = 16;
constexpr int kQueueSpinTimeouts = 15;       // bounded spins that ran out during the solve (lfr_batch_spin_timeouts)
static_assert(KC_COUNT <= kQueueSpinTimeouts, "queue block");
// KernelArgs::prof, the batch's slab of 64-bit words: phase counters [cls * kProfPhases + phase] (-DLFR_PROFILE_PHASES), the queue
// block, then kProfFactorWords per workgroup class (-DLFR_PROFILE_FACTOR: two waves x 8)
constexpr int kProfPhases = 8;
constexpr int kProfQueue = kProfPhases * KC_COUNT;
constexpr int kProfFactor = kProfQueue + kQueueWords / 2;
constexpr int kProfFactorWords = 16;
constexpr size_t kProfWords = kProfFactor + kProfFactorWords * (KC_COUNT - KC_BLOCK);
__host__ __device__ inline unsigned int *queue_block(unsigned long long *prof) { return reinterpret_cast<unsigned int *>(prof + kProfQueue); }
__host__ __device__ inline unsigned long long *factor_profile(unsigned long long *prof, int cls) { return prof + kProfFactor + kProfFactorWords * (cls - KC_BLOCK); }

// one launch for all packed classes: blocks [blk_begin[i], blk_begin[i+1]) belong to packed class kPackedOrder[i]
struct PackedRanges {
    int blk_begin[kPackedClasses + 1];
    int desc_begin[kPackedClasses], desc_end[kPackedClasses];
};

// ---- lfr_solve.hip: the forward kernels' launch functions.  The caller (the launch plan of lfr_batch_solve) chooses streams, events,
// grids and the order; template arguments, block sizes and dynamic LDS are chosen beside the kernels.  Errors: hipGetLastError(). ----
// Compile-time constants of the kernels (-DLFR_PACKED_WAVES, -DLFR_THREADS_*, -DLFR_TEAM_MAX) that size launches and workspaces.
struct SolveGeometry {
    int packed_waves;                    // waves per workgroup of the packed kernels
    int comps_per_block[KC_COUNT];       // components a workgroup of the class hosts
    int threads_s, threads_m, threads_l, threads_g;      // workgroup sizes of KC_BLOCK, KC_BLOCK_M, KC_BLOCK_L, KC_GLOBAL
    int team_max, team_units_per_xcc, team_ctl_words, team_red_per_unit;     // teams of the elimination-tree class (the comment above TeamCtx)
};
const SolveGeometry &solve_geometry();
size_t block_lds_bytes(int max_rows);    // dynamic LDS of a workgroup-class launch whose largest system has max_rows rows
int reserve_block_lds(int lds_s, int lds_m, int lds_l);      // hipFuncAttributeMaxDynamicSharedMemorySize of the three LDS classes
// (a.x_start set: the warm instantiations; the packed one reads records only - the caller has materialised those of a fused batch)
void launch_packed(const KernelArgs &a, const PackedRanges &r, bool fused, int n_blocks, hipStream_t cs);       // solve_packed_kernel
void launch_group_class(int cls, const KernelArgs &a, bool fused, int n_blocks, hipStream_t cs);                // one packed class (LFR_SERIAL_CLASSES=1)
void launch_block_class(int cls, const KernelArgs &a, int rows, int wgs, hipStream_t cs);                       // solve_block_kernel of an LDS class
void launch_tree(const KernelArgs &a, bool team, int grid, hipStream_t cs);                                     // solve_tree_kernel / solve_tree_team_kernel
void launch_warmup();                    // an empty kernel of lfr_solve.hip: loads the forward kernels' code object

}  // namespace lfr

// =============================================================================================
// the batch
// =============================================================================================
using lfr::kProfWords;                                  // (d_prof: the layout block above)

constexpr uint32_t kPackedEventsAliased = 1u << 31;     // ev_recorded: the packed launch is timed by the solve's own pair of events

namespace lfr {
// What a pass that runs after a solve (backward, covariance) keeps per batch, set up on its first call: workspace and offsets of the
// dense triangles of the components above the LDS classes, a status word per descriptor, the events around its latest call.
struct PassState {
    DevArena slab;
    double *d_hws = nullptr;
    uint64_t *d_hws_off = nullptr;
    int32_t *d_status = nullptr;
    int rows_max[KC_COUNT] = {0};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t last_stream = nullptr;
    int64_t n_calls = 0;
    virtual ~PassState() = default;                     // (a pass may derive its own fields: the backward does)
};
struct PassKind {                                       // what differs between the passes
    const char *name;                                   // "backward": lfr_batch_backward in the messages
    PassState *(*make)();                               // the pass's own state type
    // the pass's part of the setup, run once the shared carvings are made: its own carvings from s->slab (the extra_bytes of
    // pass_begin are there for them) and the dynamic-LDS reservation of its kernels
    int (*extra)(lfr_batch *b, PassState *s);
};
void pass_free(PassState *s);                           // waits for the latest call
hipEvent_t pass_last_event(const PassState *s);         // end of the latest call (nullptr: none has run)
// Entry of lfr_batch_<name>: the checks that do not depend on the arguments (solved at all, inputs epoch), hipSetDevice, the setup on the
// first call (*slot is installed only after every step has succeeded; slab and events are released on every error path), the wait
// for the latest solve, the record of ev0 on st.
int pass_begin(lfr_batch *b, PassState **slot, const PassKind &kind, size_t extra_bytes, hipStream_t st);
// The same for the passes that need no solve (evaluate, evaluate_vjp, hessian_product, hessian_solve), whose entry is their own: the first call's
// setup with a slab of slab_bytes for kind.extra to carve (installed in *slot as above)
int pass_setup_unsolved(lfr_batch *b, PassState **slot, const PassKind &kind, size_t slab_bytes);
int pass_end(PassState *s, hipStream_t st);             // records ev1; the call is now the pass's latest
int pass_wait_ms(PassState *s, hipStream_t st, double *kernel_ms);      // waits for st (read-backs queued on it are in): the time between the call's events
int64_t pass_status(lfr_batch *b, PassState *s, const char *name, int32_t *status);     // lfr_batch_<name>_status
int pass_histogram(lfr_batch *b, PassState *s, hipStream_t st, int64_t count[3], double *kernel_ms);     // waits for the latest call: descriptors with status 0 or 3, 1, 2 and the time between its events
// deals the blocks of the one packed launch to the packed classes, waves_per_block waves each (components per wave: solve_geometry())
void packed_ranges(const lfr_batch *b, int waves_per_block, PackedRanges *r, int *n_blocks);
}  // namespace lfr
struct lfr_batch {
    int device = 0;
    lfr::DevCtx *ctx = nullptr;
    int tukey_variant = LFR_TUKEY_CERES1;
    int64_t n_graph_nodes = 0;
    int shard_world = 1;
    // launch geometry (device-assembled batches: read back once as AsmSummary)
    int n_desc = 0;
    int class_begin[lfr::KC_COUNT + 1] = {0};
    int64_t class_edges[lfr::KC_COUNT] = {0};
    int class_max_rows[lfr::KC_COUNT] = {0};          // largest system of every workgroup class (sizes its launch's LDS)
    int64_t n_edges = 0, n_nodes = 0, n_tracks = 0;
    // device: everything lives in `slab` (+ the workgroup kernels' workspace in `ws_slab`)
    lfr::DevArena slab, ws_slab;
    lfr::CompDesc *d_descs = nullptr;
    lfr::EdgeRec *d_edges = nullptr;
    uint32_t *d_node_ids = nullptr;
    double *d_positions = nullptr;
    lfr::CompInfoDev *d_infos = nullptr;
    double *d_workspace = nullptr;
    uint64_t es_doubles = 0;                             // per-edge scratch of the workgroup classes (8 doubles per edge), the head of the workspace
    int tree_levels_max = 0;                             // KC_GLOBAL: levels of the deepest elimination tree
    int64_t tree_blocks = 0, tree_updates = 0;           // KC_GLOBAL: 16-row columns / left-looking tile updates per factorization, summed over the class
    int tree_begin = 0;                                  // first descriptor of the class; per component of the class: columns, tiles, 16x16x16 updates, levels, sweep items
    // teams of workgroups per component (solve_tree_team_kernel): control words + reduction slots at the tail of the workspace,
    // the work thresholds of teams of 2 / 4 / 8 (LFR_TREE_TEAM), the workgroups the class's components ask for together
    unsigned int *d_team_ctl = nullptr;
    double *d_team_red = nullptr;
    uint32_t team_work[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
    int team_wgs = 0;
    uint32_t team_patience_us = 50000u;                  // LFR_TEAM_PATIENCE_MS: the comment above TeamCtx (Residency)
    std::vector<int64_t> tree_comp_stats;                // 5 per component
    int64_t tree_tiles = 0, tree_dense_tiles = 0;          // KC_GLOBAL: 16x16 tiles stored / tiles of the dense lower triangles
    uint64_t *d_ws_off = nullptr, *d_es_off = nullptr;
    // fused gather: the packed kernel reads the graph's own flow arrays (kept alive through dev_hold)
    bool fused = false;                                  // the NEXT solve gathers (true until the records have been materialised)
    uint32_t packed_edges = 0;                           // records of the packed classes (the head of the edge array)
    uint32_t *d_edge_ref = nullptr, *d_edge_word = nullptr;
    std::shared_ptr<lfr::DevProblem> dev_hold;
    unsigned long long *d_prof = nullptr;
    lfr::NodeInc *d_node_inc = nullptr;
    uint32_t *d_in_idx = nullptr;
    uint32_t *d_desc_component = nullptr, *d_desc_class = nullptr, *d_desc_tracks = nullptr;   // device-assembled: behind the host mirrors
    // host mirrors (host-assembled: filled at creation; device-assembled: fetched on first use)
    bool mirrors_valid = false;
    std::vector<lfr::CompDesc> descs;
    std::vector<int64_t> desc_component;
    std::vector<int32_t> desc_class, desc_tracks;
    std::vector<uint32_t> node_ids;
    // pinned staging of the positions (downloads, zero-copy view)
    double *h_positions = nullptr;
    size_t h_positions_bytes = 0;
    float *h_positions_f32 = nullptr, *d_positions_f32 = nullptr;      // lfr_batch_positions_view_f32: converted on the device, half the copy
    size_t h_positions_f32_bytes = 0, d_positions_f32_bytes = 0;
    // events / streams
    static constexpr int kSlots = 64;                    // event ring: timings of the last 64 solves
    static constexpr int kEvPerSlot = 2 * (lfr::KC_COUNT + 1);
    hipEvent_t ev_ring[kSlots * kEvPerSlot];
    hipEvent_t *ev = ev_ring;                            // slot of the current solve
    uint32_t ev_recorded[kSlots] = {};                   // per slot: classes whose start/end events were recorded
    int64_t n_solves = 0;
    bool serial = false;                               // LFR_SERIAL_CLASSES=1: all classes on the caller's stream
    hipEvent_t ev_fork = nullptr;
    lfr::DevArena order_slab;                          // hand-out order of the workgroup classes + the sort's temporaries
    uint32_t *d_wg_order = nullptr;
    hipEvent_t ev_order = nullptr;                     // the order is sorted on the context's stream: solves wait for it
    hipStream_t side_stream = nullptr;                 // the packed launch runs beside the workgroup-per-component kernels
    hipStream_t wg_stream[lfr::KC_COUNT] = {nullptr};  // one stream per further workgroup class (all owned by the device context)
    hipStream_t last_stream = nullptr;                 // stream of the latest solve (downloads wait for it)
    int packed_slot = 0;                               // class slot that carries the packed launch's events
    double h2d_ms = 0.0;             // upload (host-assembled) or device assembly incl. waiting for the flows
    std::vector<lfr::CompInfoDev> infos;      // last downloaded
    bool infos_valid = false;
    // implicit-gradient backward (lfr_backward.hip): everything is set up on the first lfr_batch_backward
    const lfr::Graph *graph = nullptr;   // for the record -> directed-edge map of batches without edge_ref
    uint64_t graph_serial = 0;           // (lfr::graph_alive: the map is made on first use, the graph may be gone by then)
    int64_t n_graph_matches = 0;
    // record -> directed edge of the graph for batches without edge_ref (lfr::ensure_edge_map): the backward scatters through it,
    // lfr_batch_set_inputs gathers through it; whichever comes first builds it
    lfr::DevArena map_slab;
    uint32_t *d_eid = nullptr;
    // new inputs into the live batch (lfr_inputs.hip): inputs_epoch counts lfr_batch_set_inputs calls, solved_epoch is its value at
    // the latest solve - backward and covariance combine positions with records and refuse to run while the two differ
    bool cc_sharded = false;             // the problem covers one rank's connected components: its match numbering is not the graph's
    uint64_t inputs_epoch = 0, solved_epoch = 0;
    hipEvent_t ev_inputs = nullptr;      // end of the latest lfr_batch_set_inputs
    hipStream_t inputs_stream = nullptr;
    bool inputs_pending = false;         // no solve has been issued since: the next one waits for ev_inputs
    lfr::PassState *bwd = nullptr, *cov = nullptr;       // lfr_backward.hip / lfr_covariance.hip: set up on the first call
    lfr::PassState *eval = nullptr;                      // lfr_evaluate.hip: set up on the first lfr_batch_evaluate (its own entry: needs no solve)
    lfr::PassState *jvp = nullptr;                       // lfr_jvp.hip: set up on the first lfr_batch_jvp
    lfr::PassState *evjp = nullptr;                      // lfr_evaluate.hip: set up on the first lfr_batch_evaluate_vjp (needs no solve either)
    lfr::PassState *hvp = nullptr;                       // lfr_hessian_product.hip: set up on the first lfr_batch_hessian_product (needs no solve either)
    lfr::PassState *hsolve = nullptr;                    // lfr_hessian_solve.hip: set up on the first lfr_batch_hessian_solve (needs no solve either)

    lfr_batch() { for (auto &e : ev_ring) e = nullptr; }
    ~lfr_batch() {
        lfr::pass_free(bwd);
        lfr::pass_free(cov);
        lfr::pass_free(eval);
        lfr::pass_free(jvp);
        lfr::pass_free(evjp);
        lfr::pass_free(hvp);
        lfr::pass_free(hsolve);
        if (ctx) {
            (void)hipSetDevice(device);
            if (n_solves > 0) (void)hipStreamSynchronize(last_stream);      // nothing may still use the slab
            if (inputs_epoch > 0) (void)hipStreamSynchronize(inputs_stream);
            if (side_stream) (void)hipStreamSynchronize(side_stream);
            for (auto &w : wg_stream) if (w) (void)hipStreamSynchronize(w);
            (void)hipStreamSynchronize(ctx->s_main);
            if (h_positions) ctx->pinned_release(h_positions, h_positions_bytes);
            if (h_positions_f32) ctx->pinned_release(h_positions_f32, h_positions_f32_bytes);
            if (d_positions_f32) ctx->dev_release(d_positions_f32, d_positions_f32_bytes);
        }
        if (ctx) {                                      // (every stream this batch used has been waited for above: the events are idle)
            for (auto &e : ev_ring) ctx->event_release(e, true);
            ctx->event_release(ev_fork, false);
            ctx->event_release(ev_order, false);
            ctx->event_release(ev_inputs, false);
        } else {
            for (auto &e : ev_ring) if (e) (void)hipEventDestroy(e);
        }
        // slab / ws_slab return to the context's cache in their destructors
    }
};

namespace lfr {
// host mirrors of a device-assembled batch (descriptors, component ids, classes, node ids): 2-6 MB, fetched once
int ensure_mirrors(lfr_batch *b);
// writes the packed-class records of a fused batch (lfr_batch_solve does so on a batch's second solve); the caller clears b->fused
void materialize_records(lfr_batch *b, hipStream_t st);
// the batch's record -> directed-edge map (lfr_inputs.hip): nothing to do for a batch with edge_ref; otherwise built once from the graph
// (LFR_ERR_ARG when that has been freed) - a synchronising call the first time, free afterwards
int ensure_edge_map(lfr_batch *b);
inline const uint32_t *edge_map(const lfr_batch *b) { return b->d_edge_ref ? b->d_edge_ref : b->d_eid; }
// What the passes that need no solve (evaluate, evaluate_vjp, hessian_product, hessian_solve) do before their launches: wait by event for the latest
// solve and the latest lfr_batch_set_inputs, record the pass's ev0, and write the packed records of a device-assembled batch that
// still gathers them from the graph's arrays
int eval_prologue(lfr_batch *b, PassState &s, hipStream_t st);

// ---- the launches of a pass.  Errors: hipGetLastError(). ----
// packed classes: ONE launch of one-wave blocks, dealt to the classes by packed_ranges; packed(a, ranges)
template <class Packed, class Args>
void launch_packed_pass(const lfr_batch *b, Packed packed, const Args &a, hipStream_t st) {
    PackedRanges r;
    int nb = 0;
    packed_ranges(b, 1, &r, &nb);
    if (nb > 0) hipLaunchKernelGGL(packed, dim3(nb), dim3(64), 0, st, a, r);
}
// the two layouts of a pass without a matrix: the packed launch, then one workgroup per component of every workgroup class in one
// launch (they are contiguous in the batch order); block(a) with a.desc_begin its first descriptor
template <class Packed, class Block, class Args>
void launch_two_layouts(const lfr_batch *b, Packed packed, Block block, int block_threads, Args a, hipStream_t st) {
    launch_packed_pass(b, packed, a, st);
    a.desc_begin = b->class_begin[KC_BLOCK];
    const int n = b->class_begin[KC_COUNT] - a.desc_begin;
    if (n > 0) hipLaunchKernelGGL(block, dim3(n), dim3(block_threads), 0, st, a);
}
}  // namespace lfr
