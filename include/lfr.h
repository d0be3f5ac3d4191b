/* lfr.h — C ABI of liblfr_hip.so: MI355X-native multi-view keypoint-refinement solver.
 *
 * Drop-in scope: the reference's `solve` executable, multi-view-refinement/solve.cc:375-682
 * (+ cost.cc, graph.{h,cc}).  The reference has no library API for this path — its only
 * interface is the CLI + the two protobuf files (types.proto) — so the entry points below are
 * the stages of that main(), cut where a host program (the `solve` launcher, bench.py, a
 * cgo/ctypes binding) needs to hold data between them.  Each declaration cites the reference
 * lines it replaces.  Plain C types only, caller-owned output buffers, int return codes
 * (0 = ok, <0 = error, text via lfr_last_error()), no exceptions across the boundary.
 *
 * Units/axes: positions[2n] = di (row / y), positions[2n+1] = dj (col / x) of node n, in the
 * solver's unit (16 px * fact at extraction resolution; colmap_utils.py:133-136).
 *
 * Undefined inputs (the reference defines none of them; tests/test_gpu_undefined_inputs.py pins the library against the oracle):
 *   - similarity == 0 is a legal weight: the edge drops out of the cost (ScaledLoss(.., 0), solve.cc:111,120);
 *   - similarity < 0, +-inf or NaN, or a flow entry that is not finite, makes the evaluation of ITS component non-finite: no LM
 *     step of that component is ever valid, it terminates LFR_TERM_FAILURE after ten invalid steps and keeps zero displacements
 *     (Ceres: a non-finite evaluation fails, IsSolutionUsable() is false and solve.cc:609-612 left the positions at 0).  Every other
 *     component - also one packed into the same wavefront - is solved exactly as if the bad match were not there.
 *     One difference from Ceres in the packed classes (components of up to 32 rows): their first evaluation, at the origin, reads
 *     only the centre of the 3 x 3 flow grid and its four neighbours (entries 2, 3, 6..11, 14, 15 of the 18).  A non-finite value
 *     in one of the eight corner entries (0, 1, 4, 5, 12, 13, 16, 17) is seen one evaluation later: the first step is taken, the
 *     re-evaluation fails the component.  Termination and the zero displacements are the same; the component reports one iteration
 *     more than Ceres, and more evaluations.  (Seeing it at once costs the solve more than it is worth: tests/
 *     test_gpu_undefined_inputs.py pins exactly this);
 *   - a NaN similarity additionally leaves the order-dependent graph stage (tracks and roots sort by similarity, solve.cc:489-582)
 *     undefined in the reference itself; the library never emits a non-finite displacement, but which node of a tie becomes a
 *     root may differ from a given Ceres build;
 *   - all-zero flow grids (SKIP_REFINEMENT, compute_match_graph.py:150-152): every component converges at iteration 0, all zeros.
 */
#ifndef LFR_H
#define LFR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFR_VERSION 1

/* error codes */
#define LFR_OK 0
#define LFR_ERR_ARG (-1)
#define LFR_ERR_IO (-2)
#define LFR_ERR_PARSE (-3)       /* "Failed to parse proto object."  solve.cc:433-436 */
#define LFR_ERR_HIP (-4)
#define LFR_ERR_UNSUPPORTED (-5)
#define LFR_ERR_NOMEM (-6)

/* Tukey loss flavour: Ceres changed TukeyLoss by a factor 2 between 1.14 and 2.0 and the
 * reference pins no Ceres version (CMakeLists.txt:9). */
#define LFR_TUKEY_CERES1 1
#define LFR_TUKEY_CERES2 2

/* termination types (ceres::TerminationType subset that ceres::Solve can return here) */
#define LFR_TERM_CONVERGENCE 0
#define LFR_TERM_NO_CONVERGENCE 1
#define LFR_TERM_FAILURE 2

typedef struct lfr_graph lfr_graph;       /* parsed match graph: nodes + directed edges (host) */
typedef struct lfr_problem lfr_problem;   /* tracks, roots, components + device batch layout (host) */
typedef struct lfr_batch lfr_batch;       /* a problem (or one shard of it) resident in HBM */

int lfr_version(void);
const char *lfr_last_error(void);          /* thread-local, valid until the next failing call */

/* ---------------------------------------------------------------------------------------------
 * A0/A3  MatchingFile ingest + graph construction.                    solve.cc:426-481, graph.cc
 * ------------------------------------------------------------------------------------------- */

/* Parse serialized MatchingFile(s) (types.proto:3-28) in the given order, skipping image pairs
 * that touch a banned image (solve.cc:444-446).  Nodes are numbered in order of first
 * appearance, node1 before node2 (solve.cc:474-475). */
int lfr_graph_from_files(const char *const *paths, int n_paths, const char *const *banned, int n_banned,
                         lfr_graph **out);

/* Resolve `path`, or `path.part.0`, `path.part.1`, ... up to the first gap (solve.cc:416-424),
 * then behave as lfr_graph_from_files. */
int lfr_graph_from_matches_file(const char *path, const char *const *banned, int n_banned, lfr_graph **out);

/* lfr_graph_from_matches_file + lfr_graph_to_device(device) in one call, with the two overlapped: the flows (144 of the 164 bytes per
 * match) start their way to HBM as soon as the scanner has them in place, while it still numbers the nodes; endpoints, similarities and
 * node images follow before the call returns (asynchronously: the pipeline's stream waits for them, the caller does not).  The graph and
 * every result are identical to the two-call form; a device that cannot be initialised is LFR_ERR_HIP.  This is the ingest the `solve`
 * drop-in uses: the reference's "Total time" (solve.cc:487) starts after the file is in memory, ours after it is in HBM or on its way. */
int lfr_graph_from_matches_file_device(const char *path, const char *const *banned, int n_banned, int device, lfr_graph **out);

/* Same graph from flat arrays — the producer contract of compute_match_graph.py:163-187 without
 * the protobuf hop.  pair_img1/2[p]: image index of ImagePair p; matches of pair p are
 * [pair_off[p], pair_off[p+1]); disp1/disp2: n_matches x 18 float32 (grid_idx*2 + {di,dj}),
 * disp2 = flow image1->image2, disp1 = flow image2->image1 (solve.cc:477-478). */
int lfr_graph_from_arrays(int32_t n_images, const char *const *image_names, const float *image_facts,
                          int64_t n_pairs, const int32_t *pair_img1, const int32_t *pair_img2,
                          const int64_t *pair_off, const uint32_t *feat1, const uint32_t *feat2,
                          const float *sim, const float *disp1, const float *disp2,
                          const char *const *banned, int n_banned, lfr_graph **out);

/* Producer contract without the host hop for the flows (compute_match_graph.py:163-187 keeps
 * grid_displacements12/21 on the GPU): as lfr_graph_from_arrays, but disp1/disp2 are DEVICE pointers
 * (n_matches x 18 float32 on HIP device `device`, owned by the caller, alive until the batch has been
 * created).  Such a graph is solved through lfr_problem_build_labels / lfr_problem_build_hip +
 * lfr_batch_create on the same device; lfr_problem_build (host assembly) rejects it. */
int lfr_graph_from_arrays_device_flows(int32_t n_images, const char *const *image_names, const float *image_facts,
                                       int64_t n_pairs, const int32_t *pair_img1, const int32_t *pair_img2,
                                       const int64_t *pair_off, const uint32_t *feat1, const uint32_t *feat2,
                                       const float *sim, const void *disp1_device, const void *disp2_device, int device,
                                       const char *const *banned, int n_banned, lfr_graph **out);

/* Producer contract without any host hop for the per-match arrays (compute_match_graph.py:134-159 runs the matchers and the
 * two-view network on the device): as lfr_graph_from_arrays_device_flows, but feat1 / feat2 / sim are DEVICE pointers too
 * (n_matches = pair_off[n_pairs] elements each on HIP device `device`, laid out as in lfr_graph_from_arrays; feature indices use the
 * full uint32 range).  Names, facts, pair_img1/2, pair_off and banned stay on the host.  The nodes are numbered on the GPU
 *  and the graph is the one lfr_graph_from_arrays_device_flows builds from the same values, bit for bit: images in
 * order of first appearance over the kept pairs (first fact wins), pairs that touch a banned image skipped, nodes in order of first
 * appearance, match by match, node1 before node2 (solve.cc:474-475) - and so is every label, batch and result downstream.
 *   lifetime   disp1 / disp2: owned by the caller, alive until the batch has been created.  feat1 / feat2 / sim are read inside this
 *              call only; the graph keeps its own copies.
 *   order      the five arrays must be complete when the call is made (the caller synchronises); the call is synchronous and returns
 *              with the graph usable by every entry point.
 *   residency  the graph is left resident on `device`, as if lfr_graph_to_device had run: lfr_problem_build_hip and
 *              lfr_batch_create there continue from that copy and upload nothing; lfr_graph_evict_device drops it and the next use
 *              rebuilds it from the host arrays, which the call has filled from the device (16 bytes per match, 8 per node).
 *              lfr_problem_build (host assembly) rejects the graph like every graph with device flows.
 *   errors     LFR_ERR_ARG, checked on the host before any GPU work: a NULL among the five device pointers while n_matches > 0,
 *              device < 0, an image index out of range, a pair_off that starts below 0 or decreases; LFR_ERR_UNSUPPORTED:
 *              n_matches >= 2^30; LFR_ERR_HIP / LFR_ERR_NOMEM as elsewhere.  n_matches == 0, or every pair banned: an empty graph
 *              (not resident), LFR_OK. */
int lfr_graph_from_device_arrays(int32_t n_images, const char *const *image_names, const float *image_facts,
                                 int64_t n_pairs, const int32_t *pair_img1, const int32_t *pair_img2, const int64_t *pair_off,
                                 const uint32_t *feat1_device, const uint32_t *feat2_device, const float *sim_device,
                                 const void *disp1_device, const void *disp2_device, int device,
                                 const char *const *banned, int n_banned, lfr_graph **out);

/* Device residency of the graph (the GPU-side counterpart of the Graph object solve.cc:405-481 builds while it
 * parses).  lfr_graph_to_device starts copying endpoints, similarities and flows to HBM
 * asynchronously and returns; the device pipeline (lfr_problem_build_hip, lfr_batch_create) continues from that
 * copy, and creates it itself - inside the caller's "Total time" span - when it does not exist.  The copy stays
 * cached on the handle until lfr_graph_evict_device / lfr_graph_free. */
int lfr_graph_to_device(const lfr_graph *g, int device);
int lfr_graph_evict_device(const lfr_graph *g);

void lfr_graph_free(lfr_graph *g);
int64_t lfr_graph_num_nodes(const lfr_graph *g);      /* "# graph nodes"  solve.cc:484 */
int64_t lfr_graph_num_edges(const lfr_graph *g);      /* "# graph edges" = 2 x matches  solve.cc:485 */
int32_t lfr_graph_num_images(const lfr_graph *g);     /* images_set.size()  solve.cc:448,450,586 */
/* node_image[n] = index into the seen-image list; node_feature[n] = feature_idx */
int lfr_graph_get_nodes(const lfr_graph *g, int32_t *node_image, uint32_t *node_feature);
const char *lfr_graph_image_name(const lfr_graph *g, int32_t image);
float lfr_graph_image_fact(const lfr_graph *g, int32_t image);

/* Serialize a MatchingFile from flat arrays (native counterpart of compute_match_graph.py:163-205;
 * used by the generators and by callers that want to keep the file hand-off). */
int lfr_write_matching_file(const char *path, int32_t n_images, const char *const *image_names,
                            const float *image_facts, int64_t n_pairs, const int32_t *pair_img1,
                            const int32_t *pair_img2, const int64_t *pair_off, const uint32_t *feat1,
                            const uint32_t *feat2, const float *sim, const float *disp1, const float *disp2);

/* ---------------------------------------------------------------------------------------------
 * A4-A7, A9, A11  tracks, roots, components, problem assembly.          solve.cc:487-606, 79-143
 * ------------------------------------------------------------------------------------------- */
typedef struct lfr_problem_stats {
    int64_t n_tracks;              /* "# tracks"            solve.cc:534 */
    int64_t max_track_size;        /* "max track size"      solve.cc:549 */
    int64_t n_components;          /* "# components"        solve.cc:591 */
    int64_t max_component_size;    /* "max component size"  solve.cc:606 */
    int64_t n_cut_components;      /* components above the cap that went through the graph cut */
    int64_t n_solved_components;   /* components handed to the solver (>1 node, >=1 variable) */
    int64_t n_solved_tracks;       /* tracks with >=2 nodes inside solved components */
    int64_t n_solved_edges;        /* directed edges = residual blocks of the reduced programs */
    int64_t n_solved_nodes;        /* nodes (variable + constant) inside solved components */
    double tracks_ms, roots_ms, graph_cut_ms, assemble_ms;
    double kruskal_rounds;         /* device graph stage: parallel rounds spent on large connected components (0: none) */
    double tie_resorts;            /* device graph stage: 1 if a long run of equal similarities made it order the matches with the three
                                      stable sorts instead of the one sort + in-place tie fix (same order either way) */
} lfr_problem_stats;

/* max_nodes_in_component <= 0: use the number of seen images (solve.cc:586).
 * component_override: NULL, or n_nodes component ids that replace separate_meta_graph()
 * (solve.cc:586) — the side-car for exact parity with a reference run on inputs whose components
 * exceeded the cap (Graclus' cut is not reproducible). */
int lfr_problem_build(const lfr_graph *g, int64_t max_nodes_in_component, const int64_t *component_override,
                      lfr_problem **out);
/* Same graph stage (tracks, roots, components) without the host-side batch assembly: the 80-byte
 * edge records, descriptors and incidence lists are then built on the GPU by lfr_batch_create - the
 * whole problem (shard_world = 1: the flows cross PCIe once in match order) or one shard of it
 * (shard_world > 1: the device filters its components and gathers only their flow rows); no host-side
 * record array is ever materialised.  Results are bit-identical to the host-assembled batch / shard. */
int lfr_problem_build_labels(const lfr_graph *g, int64_t max_nodes_in_component, const int64_t *component_override,
                             lfr_problem **out);
/* As lfr_problem_build_labels, with the graph stage itself on HIP device `device`: radix sort of the
 * matches, connected components, the order-dependent constrained union-find (solve.cc:499-523) by one
 * GPU thread per small connected component and by exact parallel rounds over prefix blocks for large
 * ones, roots, components; components above the size cap are cut on the host from meta edges the
 * device compacts and sums, and re-labelled on the device.  Bit-identical labels.  Falls back to the
 * host stage only when component_override is given, for >= 2^31 nodes or >= 2^30 matches, when the
 * similarities span more than 2^10 in magnitude or hold inf/nan (the device sums them with atomics, exact and
 * therefore order independent only in a narrow exponent range; the host sums in the reference's order), when the
 * image bitsets of the parallel rounds would exceed 24 GB, or after 100000 rounds (a path-shaped
 * dependency chain). */
int lfr_problem_build_hip(const lfr_graph *g, int device, int64_t max_nodes_in_component,
                          const int64_t *component_override, lfr_problem **out);
/* flags: LFR_BUILD_FLOWS_STAY_ON_HOST - do not stage the flows in HBM; a sharded lfr_batch_create then gathers
 * only its shard's rows zero-copy from the graph's pinned host arrays (multi-GPU: every GPU pulls 1/world of the
 * flow bytes over its own PCIe link). */
#define LFR_BUILD_FLOWS_STAY_ON_HOST 1
int lfr_problem_build_hip_ex(const lfr_graph *g, int device, int64_t max_nodes_in_component,
                             const int64_t *component_override, int flags, lfr_problem **out);
/* Multi-GPU, one process per GPU (solve.cc:594-597: components are independent; solve.cc:489-541: the constrained spanning forest
 * never joins two connected components of the match graph, so tracks, roots and components decompose by connected component too):
 * the graph stage of rank shard_rank of shard_world over ITS connected components only - the k-th connected component in node order
 * belongs to rank k mod shard_world.  lfr_batch_create(p, device, 0, 1) then assembles this rank's components; the union over the ranks
 * is the whole problem, every component bit-identical to the unsharded run.  lfr_problem_cc_sharded(p) returns 0 when one connected
 * component dominates (or the host stage ran): the problem then covers the whole graph and the caller shards the COMPONENTS at
 * assembly, lfr_batch_create(p, device, shard_rank, shard_world), as with lfr_problem_build_hip_ex. */
int lfr_problem_build_hip_shard(const lfr_graph *g, int device, int64_t max_nodes_in_component, int flags, int shard_rank, int shard_world,
                                lfr_problem **out);
int lfr_problem_cc_sharded(const lfr_problem *p);
void lfr_problem_free(lfr_problem *p);
/* The two-way cut this library substitutes for colmap::ComputeNormalizedMinGraphCut(edges, weights, 2)
 * (solve.cc:192; COLMAP wraps Graclus there, a third-party multilevel heuristic that cannot be restated: see
 * DESIGN.md).  Exposed so that a checker can run the reference's recursion around the same primitive
 * (tests/, oracle/).  edges (edge_a[k], edge_b[k]) with integer weights; writes the distinct node ids in
 * ascending order and their side (0/1) - 2 * n_edges entries are always enough - and returns their count. */
int64_t lfr_bisect_graph(int64_t n_edges, const int32_t *edge_a, const int32_t *edge_b, const int32_t *weights,
                         int32_t *nodes, int32_t *part);
/* The whole size-cap recursion (the product's restatement of recursive_graph_cut, solve.cc:185-250, around lfr_bisect_graph): subset index
 * of every node that has an edge, nodes ascending; node_weights[id] for every id below n_node_weights.  For checkers (the oracles run their
 * own literal recursion around lfr_bisect_graph; the two must agree) and for timing the host part of the cut.  Returns the node count. */
int64_t lfr_debug_recursive_cut(int64_t n_edges, const int32_t *edge_a, const int32_t *edge_b, const int32_t *weights,
                                int64_t n_node_weights, const int64_t *node_weights, int64_t max_weight, int32_t *nodes, int32_t *subset);
/* The elimination-tree plan the solver gives a component whose normal matrix does not fit LDS (the reference hands such systems to
 * Ceres' SPARSE_NORMAL_CHOLESKY, solve.cc:147): nested dissection of the tracks, 16-row blocks, block-level symbolic factorization,
 * columns by level of the elimination tree, left-looking update lists and the sweep's (node, neighbour) items - exactly the words
 * the kernel reads, so that a checker can execute the plan on the CPU (tests/test_tree_plan.py).  words[e] as above.  Returns the
 * number of 32-bit words of the plan (copied to `blob` if cap is large enough; < 0: error); info[8] = {blocks, tiles, levels,
 * items, updates, tracks, segments, column rounds}. */
int64_t lfr_debug_tree_plan(int32_t n_var, int64_t n_edges, const uint32_t *words, uint32_t *blob, int64_t cap, int64_t *info);
int lfr_problem_get_stats(const lfr_problem *p, lfr_problem_stats *stats);
/* per node: track_idx_container, is_root, component_idx_container of solve.cc:526,570,586 */
int lfr_problem_get_labels(const lfr_problem *p, int64_t *track, uint8_t *is_root, int64_t *component);

/* Solvable components dealt to shard `shard_rank` of `shard_world`: the batch order (kernel class, then
 * edge count descending - the largest-first task order of solve.cc:599-634) dealt out and back
 * (0..W-1, W-1..0, ...), so every shard gets the same mix of classes and sizes.  Needs a host-assembled problem.
 * Fills original component ids / edge counts (either may be NULL); returns the count. */
int64_t lfr_problem_shard_components(const lfr_problem *p, int shard_rank, int shard_world, int64_t *components,
                                     int64_t *n_edges);

/* ---------------------------------------------------------------------------------------------
 * A1, A2, A8, A10  batched Levenberg-Marquardt on the GPU.    solve.cc:79-160,614-635 + cost.cc
 * ------------------------------------------------------------------------------------------- */
typedef struct lfr_solve_stats {
    int64_t n_components, n_edges, n_nodes, n_tracks;    /* of this batch/shard */
    int64_t n_converged, n_no_convergence, n_failed;
    int64_t sum_iterations;
    int64_t ref_jacobian_passes_edges;   /* sum_c E_c * (jacobian evaluations Ceres performs)  */
    int64_t ref_cost_passes_edges;       /* sum_c E_c * (cost-only evaluations Ceres performs) */
    int64_t exec_passes_edges;           /* sum_c E_c * (edge sweeps the kernels executed)     */
    int64_t ref_passes_nodes;            /* sum_c N_c * (all evaluations Ceres performs)       */
    double sum_final_cost;
    double kernel_ms;                    /* HIP-event time of the solve kernels, last solve */
    double h2d_ms, d2h_ms;
    double dominant_kernel_ms;           /* HIP-event time of the largest kernel launch */
    int64_t dominant_kernel_edges;       /* edges processed by that launch */
    int64_t dominant_kernel_nodes;
    int64_t dominant_ref_passes_edges;   /* (jacobian + cost passes) * edges for that launch */
    int64_t dominant_ref_passes_nodes;
} lfr_solve_stats;

/* Create the HIP context of `device` (a few hundred ms the first time) and run a toy graph through the
 * device pipeline once, so that every kernel is resolved before the real input arrives; safe to call
 * from a side thread while the caller parses its input. */
int lfr_hip_warmup(int device);
/* Pre-populate the per-device caches (device slabs, pinned staging) with what a pipeline run over a graph of
 * n_nodes / n_matches will ask for, so that a one-shot caller's timed span pays no allocation; lfr_hip_trim
 * returns every cached slab to the driver. */
int lfr_hip_reserve(int device, int64_t n_nodes, int64_t n_matches);
/* Wait for everything the library has in flight on its own streams of `device` (e.g. the upload started by
 * lfr_graph_to_device). */
int lfr_hip_synchronize(int device);
int lfr_hip_trim(int device);

/* Shard `shard_rank` of `shard_world` (see lfr_problem_shard_components) resident on HIP device `device`:
 * assembled there from the labels (lfr_problem_build_labels / _hip), or uploaded (lfr_problem_build).
 * Limits: <= 32767 nodes per component (16-bit local indices in the 80-byte edge record), < 2^30 matches; a component above 192 rows
 * whose factor needs 2^21 or more 16x16 tiles (4 GB: a DENSE component beyond ~16 k nodes) or that holds 2^30 or more records (the
 * plan's sweep items pack record << 2 | direction << 1 | flag into 32 bits) is refused (LFR_ERR_UNSUPPORTED). */
int lfr_batch_create(const lfr_problem *p, int device, int shard_rank, int shard_world, int tukey_variant,
                     lfr_batch **out);
void lfr_batch_free(lfr_batch *b);
/* Run every solve kernel of the batch on `hip_stream` (a hipStream_t, NULL = default stream).
 * The position array is zeroed once, when the batch is created (solve.cc:609-612); every solve rewrites every
 * variable node (a failed solve writes 0), roots and nodes outside solved components stay 0.  Asynchronous
 * unless stats != NULL, in which case the call synchronizes the stream and fills stats. */
int lfr_batch_solve(lfr_batch *b, void *hip_stream, lfr_solve_stats *stats);
/* The same solve started at given positions instead of the origin (the reference always starts at 0, solve.cc:609-612; ceres::Solve
 * itself starts from whatever the parameter blocks hold - this is that entry for callers that solve the same scenes again and again).
 *
 * The start array.  initial_positions_device: 2 * n_nodes doubles of the WHOLE graph on the batch's device, in the layout of
 * lfr_batch_positions_to_device and of lfr_batch_evaluate's positions_device.  NULL = the batch's own position array, started in
 * place: the latest solve's result, or the zeros of lfr_batch_create before the first solve (in place is safe: a component reads its
 * own nodes in its prologue and no other component writes them).  Only the coordinates of variable nodes of this shard's solved
 * components are read; roots and other constant nodes stay 0 whatever the array holds, everything else is ignored and not written.
 * An explicit array is read only by work enqueued in this call: the caller may overwrite it in stream order afterwards.
 *
 * The start point.  Per component x0 = project(initial): every coordinate clamped to [-1, 1] (Ceres' IterationZero projects onto the
 * bounds); a NaN reads as 0, +-inf clamps to +-1.  The library still never emits a non-finite displacement.
 *
 * The loop.  From x0 on it is lfr_batch_solve's, decision for decision: cost, J^T J and gradient at x0, the Jacobi scaling fixed
 * there, x_norm = |x0|, radius 1e4, the gradient test before the first iteration.  With an all-zero start (every coordinate that is
 * read +0 or -0; a -0 stays -0 as the value of x0) the results are those of lfr_batch_solve bit for bit.  That holds for the array
 * as a whole: components of up to 32 rows share a wavefront with their neighbours in the batch, and the first evaluation takes
 * lfr_batch_solve's closed form at the origin only when EVERY component of the wavefront starts there.  A component that starts at
 * zero beside one that does not is evaluated in the general form, which agrees with lfr_batch_solve to rounding only (seen: the last
 * bit of final_cost, 3e-17 in the positions).  ref_*_passes_* count what Ceres would have performed from x0.
 *
 * Results.  final_cost, iterations and termination as for lfr_batch_solve.  A component that FAILS writes x0, the PROJECTED start
 * (with a zero start the 0 of lfr_batch_solve); Ceres would leave the caller's unprojected values.
 *
 * State.  A solve in every respect: lfr_batch_timing, the wait for a pending lfr_batch_set_inputs, and lfr_batch_backward,
 * lfr_batch_covariance, lfr_batch_evaluate, the downloads and views, lfr_batch_spin_timeouts / _team_runs / _team_fallbacks serve it
 * afterwards.  A device-assembled batch whose records are not yet written writes them first (the warm kernels have no gathering
 * form).  Shards are served: the node numbering is the graph's.
 * Asynchronous unless stats != NULL. */
int lfr_batch_solve_from(lfr_batch *b, const double *initial_positions_device, void *hip_stream, lfr_solve_stats *stats);
/* HIP-event timings of one of the last 64 lfr_batch_solve / lfr_batch_solve_from calls (solves_back = 0: the latest);
 * waits for that solve to finish.  class_ms / class_edges: LFR_NUM_KERNEL_CLASSES entries, one
 * per kernel launch (packed <8,1,3>, <16,1,6>, a retired slot, <32,1,6>, <32,2,5>; workgroup per component with the matrix
 * in LDS: <= 88 rows, <= 130 rows, <= 192 rows; workgroup per component with the matrix in HBM). */
#define LFR_NUM_KERNEL_CLASSES 9
int lfr_batch_timing(lfr_batch *b, int solves_back, double *total_ms, double *class_ms, int64_t *class_edges);
/* Per component (order of lfr_batch_component_info): columns, tiles, 16x16x16 updates per factorization, levels and sweep items of the
 * elimination-tree plan a component above 192 rows is solved with (the reference: Ceres SPARSE_NORMAL_CHOLESKY, solve.cc:147); zeros
 * for the other components.  Any pointer may be NULL.  Returns the number of components (< 0: error). */
int64_t lfr_batch_tree_stats(lfr_batch *b, int64_t *columns, int64_t *tiles, int64_t *updates, int64_t *levels, int64_t *items);
/* Diagnostics: bounded spin-waits inside the workgroup kernels (wave hand-offs of the factorizations) that ran out during the
 * latest solve of the batch - each one rejected an LM step instead of hanging the GPU.  0 on a healthy run; < 0: error. */
int64_t lfr_batch_spin_timeouts(lfr_batch *b);
/* Components above 192 rows whose expected work reaches a threshold (LFR_TREE_TEAM="w2,w4": rows x [joins several tracks]; "0" = off)
 * are solved by a TEAM of 2 or 4 workgroups on one XCD (the reference: one Ceres SPARSE_NORMAL_CHOLESKY problem per pool thread,
 * solve.cc:147,617-635 - here the elimination tree's columns, the sweeps and the vector passes of ONE problem are spread over several
 * CUs).  Returns how many components the latest solve of the batch handed to a team (< 0: error). */
int64_t lfr_batch_team_runs(lfr_batch *b);
/* The teams of one launch form from workgroups that are resident on an XCD at the same time (the reference: a pool thread per problem,
 * solve.cc:617-635 - no such constraint).  When the CUs are not there - other kernels, another process, a smaller partition - and nobody
 * is at work and nothing moves for LFR_TEAM_PATIENCE_MS (default 50), the launch goes on with ONE workgroup per component: nothing
 * fails, no wait runs out (lfr_batch_spin_timeouts stays 0); the positions of such a component are those of a team of one (equal to the
 * team's to rounding, not bit for bit).  Returns how many components of the latest solve were solved that way (< 0: error). */
int64_t lfr_batch_team_fallbacks(lfr_batch *b);
/* positions: 2 * n_nodes doubles of the WHOLE graph; only this shard's nodes are written.  Waits for the
 * latest lfr_batch_solve of this batch, whatever stream it was issued on. */
int lfr_batch_download(lfr_batch *b, double *positions);
/* The same without the final host copy: *positions points at the batch's pinned staging buffer (2 * n_nodes
 * doubles, nodes outside the shard read 0), valid until the next solve / download / free of this batch. */
int lfr_batch_positions_view(lfr_batch *b, const double **positions);
/* The same in the precision the reference's SolutionFile holds (solve.cc:661-664 casts every displacement to float): converted on
 * the device, so half the bytes cross PCIe.  *positions: 2 * n_nodes floats in a pinned buffer of the batch, each the float nearest
 * to the double lfr_batch_positions_view would return; valid until the next solve / view / free of this batch. */
int lfr_batch_positions_view_f32(lfr_batch *b, const float **positions);
/* per solved component of the shard, in batch order: original component id, iterations,
 * termination, final cost (any pointer may be NULL). Returns the count.
 * final_cost is the fp64 value of F (the backward pass's, below) at the last iterate the solve accepted: the positions it wrote for
 * CONVERGENCE and NO_CONVERGENCE; for FAILURE the iterate it gave up at, not the zeros it wrote, and NaN where that evaluation was not
 * finite.  Every component, FAILURE included, is one term of lfr_solve_stats.sum_final_cost. */
int64_t lfr_batch_component_info(lfr_batch *b, int64_t *component, int32_t *iterations, int32_t *termination,
                                 double *final_cost, int32_t *n_var_nodes, int32_t *n_edges);

/* ---------------------------------------------------------------------------------------------
 * Implicit-gradient backward pass through lfr_batch_solve (no counterpart in the reference: the
 * in-process PyTorch interface, lfr_amd/autograd.py, trains the two-view network through it).
 *
 * Contract.  Take the batch after its latest lfr_batch_solve; x^ = the fp64 positions it produced.  Per solved component, with the
 * component structure of that solve held fixed:
 *   - F(x; theta) = sum_e 1/2 w_e rho_kind(e)(|r_e|^2) over the component's kept directed edges (exactly those the solve uses:
 *     intra-track edges Cauchy(0.25), inter-track edges Tukey(0.0625) in the batch's variant), r_e = x_dst - x_src - f(x_src; phi_e),
 *     phi_e the edge's 18 flow values, w_e its similarity (cost.cc:78-94, solve.cc:98-143);
 *   - usable components: termination CONVERGENCE or NO_CONVERGENCE.  FAILURE components get a zero gradient;
 *   - free coordinates: those of the variable nodes of usable components with |x^| < 1.  Coordinates at the +-1 box bound, roots and
 *     other constant nodes are constant;
 *   - H = the EXACT Hessian of F over the free coordinates at x^ (not Gauss-Newton): per edge w [J^T (rho' I + 2 rho'' r r^T) J +
 *     rho' sum_k r_k d2 r_k], the second term in the src-src block from the biquadratic's second derivatives, taken where a
 *     coordinate is in [-0.5, 0.5] and zero where cost.cc:38-43 zeroes the first derivative;
 *   - v = H^-1 ubar (ubar = the caller's dL/dx^ on the free coordinates); per kept edge
 *     (dL/dphi_e, dL/dw_e) = -d/dtheta_e [v . grad F_e(x^; theta_e)];
 *   - scattered to the MATCH layout of the graph - the input order of lfr_graph_from_arrays* with the matches of banned pairs removed:
 *     edge node1 -> node2 of match m goes to grad_disp2[m], edge node2 -> node1 to grad_disp1[m] (solve.cc:477-478), grad_sim[m] is
 *     the sum over both directions.  Every other entry is 0: dropped edges, edges with two constant ends, matches outside this shard;
 *   - a factorization of H that meets a pivot that is not positive gives that component a zero gradient and reports it indefinite.
 * The tracks, roots, components, edge kinds and the active set of the box are piecewise constant in theta: the gradient treats them
 * as fixed.  It is taken at x^, where LM stopped by its tolerances, not at an exact stationary point of F.
 * Kernels: one workgroup per component over the batch's kernel classes; H in LDS up to 192 rows, in an HBM workspace above; a dense
 * LDL^T that skips the zeros of each column.  Components above 6144 rows: LFR_ERR_UNSUPPORTED. */
typedef struct lfr_backward_stats {
    int64_t n_differentiated;      /* components whose gradient was computed (status 0 and, in fallback mode, 3) */
    int64_t n_not_usable;          /* FAILURE components (zero gradient) */
    int64_t n_indefinite;          /* components whose H met a pivot that is not positive (zero gradient) */
    int64_t n_bound_coordinates;   /* coordinates of usable components held at the +-1 bound */
    double kernel_ms;              /* HIP-event time of the backward's kernels (and its clearing of the outputs) */
} lfr_backward_stats;

#define LFR_BACKWARD_F64 1         /* outputs are double instead of float32 */
/* Gauss-Newton mode (may be combined with LFR_BACKWARD_F64; any other bit: LFR_ERR_ARG).  The contract above with one change:
 *   - H = J^T J over the free coordinates at x^, J the loss-corrected Jacobian of the component's kept directed edges (corrector
 *     sqrt(rho'), the similarity as the loss scale, the interpolant's derivative zeroed outside [-0.5, 0.5]): per edge
 *     w rho' [[P^T P, -P^T], [-P, I]], P = I + df/dx_src - no rho'' term, no second derivatives of the interpolant.  It is the matrix
 *     of the LM loop and of lfr_batch_covariance, but the bounds are honoured as in the exact mode: coordinates with |x^| >= 1, roots
 *     and constant nodes are constant (identity rows and columns, zero right-hand side);
 *   - v = H^-1 ubar, and the vector-Jacobian sweep -d/dtheta_e [v . grad F_e(x^; theta_e)] is the EXACT one above (it keeps its rho''
 *     and mixed-derivative terms): only H changes.
 * The result is the implicit gradient under the Gauss-Newton approximation of the Hessian; it equals the exact one where the
 * residuals vanish.  J^T J is positive definite for every connected component that has a root and positive weights, so components
 * whose exact Hessian is indefinite (where the robust loss is at work) get a gradient.  Status codes and lfr_backward_stats keep their
 * numbers and fields: status 2 / n_indefinite now mean SINGULAR (a pivot was not positive: a node tied in only by edges of weight 0
 * or by saturated Tukey edges), again with a zero gradient.  Outputs are bitwise repeatable from call to call, float32 is the float64
 * result rounded once, and host- and device-assembled batches give identical results, as in the exact mode.
 * Kernels: the classes of up to 32 rows run ONE launch in the covariance's packed layout (2-8 components per wave64, J^T J inverted in
 * registers, v = C ubar); the workgroup classes run the exact mode's kernel with the Gauss-Newton assembly. */
#define LFR_BACKWARD_GAUSS_NEWTON 2
/* Gauss-Newton fallback (may be combined with LFR_BACKWARD_F64; with LFR_BACKWARD_GAUSS_NEWTON in the same call: LFR_ERR_ARG, raised
 * before any output is touched).  The exact mode's contract, per usable component, with one change:
 *   - the exact Hessian over the free coordinates is assembled and factored, exactly as with flags 0.  Every pivot positive and finite:
 *     status 0, and the component's outputs - its match rows of grad_disp1/2, its terms of grad_sim - are those of the exact mode bit
 *     for bit;
 *   - otherwise the same workgroup rebuilds H as the Gauss-Newton matrix of LFR_BACKWARD_GAUSS_NEWTON over the same free set (bound
 *     rows and columns the identity's) and factors again.  Success: status 3, "differentiated with the Gauss-Newton matrix" - the
 *     outputs follow the Gauss-Newton mode's contract (v = (J^T J)^-1 ubar, the exact vector-Jacobian sweep).  A second failure (a node
 *     tied in only by edges of weight 0 or by saturated Tukey edges, a pivot that is not finite): status 2 and zeros, as today;
 *   - status 1 (FAILURE components) is unchanged.
 * lfr_backward_stats keeps its layout: n_differentiated counts status 0 AND 3, n_indefinite status 2 only; how many components fell
 * back is read from lfr_batch_backward_status.  Everything else is the exact mode's: epochs, errors, the 6144-row limit.  Outputs are
 * bitwise repeatable and identical for host- and device-assembled batches, float32 is the float64 result rounded once.  A status-3
 * component of more than 32 rows has bit for bit the outputs LFR_BACKWARD_GAUSS_NEWTON gives on the same solve (the same assembly,
 * LDL^T, substitutions and sweep on an untouched right-hand side).  In the classes of up to 32 rows the fallback runs in the exact
 * mode's one-wave-per-component kernel (LDL^T) while the Gauss-Newton mode's packed launch inverts explicitly: there the two agree
 * to rounding, |difference| <= max(1e-8, 64 eps kappa_2(J^T J)) |value| per component, not bitwise.
 * lfr_batch_jvp with LFR_JVP_FALLBACK_GAUSS_NEWTON decides from the same matrix with the same code: the statuses of the two calls on
 * one solve are equal and the adjoint identity holds between them.
 * Kernels: the exact mode's launch plan with the fallback compiled in; no extra launch, LDS or workspace. */
#define LFR_BACKWARD_FALLBACK_GAUSS_NEWTON 32

/* Stream-ordered device copy of the latest solve's positions (2 * n_nodes doubles of the whole graph; nodes outside the shard: 0). */
int lfr_batch_positions_to_device(lfr_batch *b, double *dst_device, void *hip_stream);
/* The gradient above.  grad_positions_device: 2 * n_nodes doubles (dL/dx of the whole graph); grad_disp1/2_device: n_matches x 18,
 * grad_sim_device: n_matches, float32 (double with LFR_BACKWARD_F64); whole arrays are overwritten.  flags: LFR_BACKWARD_F64 and / or
 * one of LFR_BACKWARD_GAUSS_NEWTON, LFR_BACKWARD_FALLBACK_GAUSS_NEWTON (0: the exact Hessian, float32 outputs); any other bit, or both
 * Hessian flags together: LFR_ERR_ARG before any output is touched.  Runs on `hip_stream` after the
 * latest solve; asynchronous unless stats != NULL.  LFR_ERR_ARG before the first solve, and between an lfr_batch_set_inputs and the
 * next solve.  The first call sets up its workspace and, for batches whose records do not carry their directed-edge ids, maps records to
 * edges from the graph (which must still be alive; lfr_batch_set_inputs shares the map). */
int lfr_batch_backward(lfr_batch *b, const double *grad_positions_device, void *grad_disp1_device, void *grad_disp2_device,
                       void *grad_sim_device, int flags, void *hip_stream, lfr_backward_stats *stats);
/* Per component (order of lfr_batch_component_info) of the latest backward: 0 differentiated, 1 not usable, 2 indefinite (zero
 * gradient), 3 differentiated with the Gauss-Newton matrix after the exact Hessian proved indefinite (only with
 * LFR_BACKWARD_FALLBACK_GAUSS_NEWTON).
 * Waits for that backward.  Returns the count (< 0: error, LFR_ERR_ARG before the first backward). */
int64_t lfr_batch_backward_status(lfr_batch *b, int32_t *status);

/* ---------------------------------------------------------------------------------------------
 * Forward-mode sensitivity of the refined positions: xdot = J thetadot, J = dx^/dtheta - the other half of lfr_batch_backward's
 * J^T ubar (input noise pushed to the positions, torch.autograd.forward_ad / torch.func.jvp, the first-order prediction
 * x^(theta + dtheta) ~ x^ + J dtheta).
 *
 * Contract.  lfr_batch_backward's, read the other way.  Take the batch after its latest solve; per usable component at x^, with the
 * structure held fixed (tracks, roots, components, edge kinds, the active set of the box):
 *   - free coordinates: those of the variable nodes with |x^| < 1;
 *   - H = exactly the matrix of lfr_batch_backward in the same mode: the exact Hessian of F over the free coordinates, or J^T J with
 *     LFR_JVP_GAUSS_NEWTON (as LFR_BACKWARD_GAUSS_NEWTON), bound coordinates as identity rows and columns;
 *   - b = -sum_e d/d eps [grad_x F_e(x^; theta_e + eps thetadot_e)] on the free coordinates, 0 on bound ones.  Per edge, with
 *     rdot_k = -sum_ij Lr_i Lc_j phidot_ijk, sdot = 2 r . rdot and Pdot = d/d eps P (the sums with dLr_i Lc_j and Lr_i dLc_j): the
 *     destination's rows take -[wdot rho' r + w (rho'' sdot r + rho' rdot)], the source's
 *     +[wdot rho' P^T r + w (rho'' sdot P^T r + rho' (Pdot^T r + P^T rdot))];
 *   - xdot = H^-1 b.
 * Its defining property is the adjoint identity with lfr_batch_backward in the same mode on the same solve:
 * ubar . (J thetadot) = (J^T ubar) . thetadot for every ubar and thetadot.
 * Inputs: the tangents in the MATCH layout of lfr_batch_backward / lfr_batch_set_inputs / lfr_batch_evaluate - tan_disp1 / tan_disp2:
 * n_matches x 18, tan_sim: n_matches, float32 (double with LFR_JVP_F64), DEVICE pointers; edge node1->node2 of match m reads
 * tan_disp2[m], node2->node1 reads tan_disp1[m], both read tan_sim[m].  tan_disp1 and tan_disp2: both given or both NULL (= a zero flow
 * tangent); tan_sim NULL = zero; all three NULL: LFR_ERR_ARG.  Only the rows of this shard's records are read, and only by work
 * enqueued in this call.  A tangent that is not finite makes only its own component's output not finite: the status stays 0 and no
 * other component - one in the same wavefront included - changes by a bit.
 * Output: tan_positions_device, 2 * n_nodes doubles, the whole array is overwritten: xdot for the free coordinates of usable
 * components; 0 for bound coordinates, roots and constant nodes, for nodes outside solved components or outside the shard, for
 * FAILURE components (status 1) and for components whose factorization meets a pivot that is not positive (status 2).
 * Errors and state: LFR_ERR_ARG before the first solve, between an lfr_batch_set_inputs and the next solve, for an unknown flag
 * bit and for LFR_JVP_GAUSS_NEWTON together with LFR_JVP_FALLBACK_GAUSS_NEWTON; LFR_ERR_UNSUPPORTED for a batch over one rank's connected components (lfr_problem_cc_sharded = 1) and for components above
 * 6144 rows.  Runs on `hip_stream` after the latest solve; asynchronous unless stats != NULL.  Changes nothing the solve, the backward
 * or the covariance read; lfr_batch_set_inputs waits by event for the latest jvp.  Results are bitwise repeatable from call to call
 * and identical for host- and device-assembled batches; no fp64 value goes through a global-memory atomic.
 * Kernels: lfr_batch_backward's launch plan - one workgroup per component (one wave for the classes of up to 32 rows in the exact
 * mode), the right-hand side summed owner-computes in record order, H in LDS up to 192 rows and in an HBM workspace above; in
 * Gauss-Newton mode the classes of up to 32 rows run ONE launch in the covariance's packed layout (xdot_row = C_row . b). */
typedef struct lfr_jvp_stats {
    int64_t n_differentiated;      /* components whose tangent was computed (status 0 and, in fallback mode, 3) */
    int64_t n_not_usable;          /* FAILURE components (zero tangent) */
    int64_t n_indefinite;          /* components whose H met a pivot that is not positive (zero tangent) */
    int64_t n_bound_coordinates;   /* coordinates of usable components held at the +-1 bound */
    double kernel_ms;              /* HIP-event time of the jvp's kernels (and its clearing of the output) */
} lfr_jvp_stats;
#define LFR_JVP_F64 1              /* the three tangent INPUTS are double instead of float32 */
#define LFR_JVP_GAUSS_NEWTON 2     /* H = J^T J over the free coordinates, as LFR_BACKWARD_GAUSS_NEWTON */
/* Gauss-Newton fallback, the H of LFR_BACKWARD_FALLBACK_GAUSS_NEWTON (may be combined with LFR_JVP_F64; with LFR_JVP_GAUSS_NEWTON in
 * the same call: LFR_ERR_ARG, nothing written).  Per usable component the exact Hessian is factored as with flags 0 - success: status
 * 0, xdot bit for bit the exact mode's - and where it meets a pivot that is not positive or not finite the same workgroup rebuilds H
 * as J^T J over the same free set and factors again: status 3, xdot = (J^T J)^-1 b with the exact b (built once); a second failure:
 * status 2, zeros.  Status 1 unchanged.  lfr_jvp_stats: n_differentiated counts status 0 and 3, n_indefinite status 2.  The statuses
 * equal those of lfr_batch_backward with LFR_BACKWARD_FALLBACK_GAUSS_NEWTON on the same solve, and the adjoint identity holds between
 * the two.  Repeatability, assemblies, errors (LFR_ERR_UNSUPPORTED for cc_sharded batches and above 6144 rows) as in the other modes.
 * A status-3 component of more than 32 rows has bit for bit the xdot of LFR_JVP_GAUSS_NEWTON; in the classes of up to 32 rows (one
 * wave per component and LDL^T here, an explicit inverse in the Gauss-Newton mode's packed launch) the two agree to rounding,
 * |difference| <= max(1e-8, 64 eps kappa_2(J^T J)) |xdot| per component. */
#define LFR_JVP_FALLBACK_GAUSS_NEWTON 32
int lfr_batch_jvp(lfr_batch *b, const void *tan_disp1_device, const void *tan_disp2_device, const void *tan_sim_device,
                  double *tan_positions_device, int flags, void *hip_stream, lfr_jvp_stats *stats);
/* Per component (order of lfr_batch_component_info) of the latest jvp: 0 differentiated, 1 not usable, 2 indefinite (zero tangent),
 * 3 differentiated with the Gauss-Newton matrix after the exact Hessian proved indefinite (only with LFR_JVP_FALLBACK_GAUSS_NEWTON).
 * Waits for that jvp.  Returns the count (< 0: error, LFR_ERR_ARG before the first jvp). */
int64_t lfr_batch_jvp_status(lfr_batch *b, int32_t *status);

/* ---------------------------------------------------------------------------------------------
 * New flows and similarities into a live batch: the forward-side counterpart of the backward's contract (a training loop solves the
 * same scenes thousands of times and only the network's outputs change; the reference re-reads its MatchingFile for every run).
 *
 * Contract.  The structure of the batch is held fixed: the kept edges, their kinds (Cauchy / Tukey), local indices, component
 * descriptors, incidence lists, kernel classes, batch order, hand-out order, tree plans and teams are those of lfr_batch_create.  Only
 * the 18 flow values and the similarity of every record change; the graph stage is not run again, so similarities that would have
 * produced other tracks or roots do not.
 *   - disp1/disp2: n_matches x 18 float32, sim: n_matches float32, DEVICE pointers on the batch's device, in the MATCH layout of the
 *     graph (exactly the layout lfr_batch_backward writes its gradients in: input order of lfr_graph_from_arrays*, banned pairs removed;
 *     edge node1->node2 of match m reads disp2[m], node2->node1 reads disp1[m], both read sim[m]);
 *   - disp1 and disp2: both given or both NULL (= keep the flows); sim NULL = keep the similarities; all three NULL: LFR_ERR_ARG;
 *   - only this shard's records are written: matches whose edges were dropped or lie outside the shard are not read;
 *   - stream-ordered and asynchronous: the call waits BY EVENT for the batch's latest solve, backward and covariance, whatever streams
 *     they ran on, and runs on `hip_stream`.  The inputs are read only by work enqueued in this call: the caller may overwrite or free
 *     them in stream order afterwards.  No host synchronisation and no allocation, except in the first call of a batch whose records do
 *     not carry their directed-edge ids: it maps records to edges from the graph (the map lfr_batch_backward makes; whichever of the two
 *     comes first builds it), and the graph must still be alive then (LFR_ERR_ARG otherwise);
 *   - the next lfr_batch_solve, on any stream, uses the new values, and so do lfr_batch_backward and lfr_batch_covariance after it.
 *     BETWEEN this call and the next solve the positions are still those of the earlier solve (downloads, views and
 *     lfr_batch_positions_to_device keep their meaning), but the records no longer belong to them: lfr_batch_backward and
 *     lfr_batch_covariance return LFR_ERR_ARG ("inputs changed since the latest solve");
 *   - undefined values follow the contract at the top of this file: a flow or similarity that is not finite fails its component only;
 *   - a batch over one rank's connected components (lfr_problem_build_hip_shard with lfr_problem_cc_sharded = 1) numbers its matches
 *     by itself: LFR_ERR_UNSUPPORTED.  Shards of lfr_batch_create(p, device, rank, world) are served.
 * Kernel: one launch over all records of the batch, one thread per (record, 16-byte chunk), coalesced 16-byte stores; the
 * similarity-only form is one 4-byte store per record and the flows-only form never touches the similarity. */
int lfr_batch_set_inputs(lfr_batch *b, const float *disp1_device, const float *disp2_device, const float *sim_device, void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * Per-keypoint covariance of the refined positions (the counterpart of ceres::Covariance with apply_loss_function = true; the
 * reference's `solve` never asks Ceres for it).
 *
 * Contract.  Take the batch after its latest lfr_batch_solve; x^ = the fp64 positions it produced.  Per solved component, with the
 * component structure of that solve held fixed:
 *   - A = J^T J over ALL coordinates of the component's variable nodes, J the loss-corrected Jacobian at x^ of the component's kept
 *     directed edges: corrector sqrt(rho') (both losses have rho'' <= 0), the similarity as the loss scale, the interpolant's
 *     derivative zeroed outside [-0.5, 0.5] (cost.cc:38-43) - the Gauss-Newton matrix of the LM loop, without damping and without
 *     Jacobi scaling.  Like Ceres it ignores the +-1 box bounds;
 *   - C = A^-1.  Per node n three numbers cov[3n + 0..2] = C(di,di), C(di,dj), C(dj,dj) of the node's own 2x2 diagonal block, in the
 *     axis order of `positions` and in the solver's unit squared;
 *   - roots, other constant nodes, nodes outside solved components and nodes outside this shard: 0;
 *   - usable components: termination CONVERGENCE or NO_CONVERGENCE.  FAILURE components: all zeros, status "not usable";
 *   - an elimination that meets a pivot that is not positive (a node tied in only by edges of weight 0 or by saturated Tukey edges):
 *     all zeros for that component, status "singular".  A zero diagonal can never be the covariance of a variable node, so a 0 is
 *     unambiguous: "no covariance for this node".  Every other component - also one in the same wavefront - is unaffected, bit for bit;
 *   - results are bitwise repeatable from call to call, and identical for the host-assembled and the device-assembled batch.
 * Kernels: components of up to 32 rows in ONE launch in the solve's packed layout (64/S components per wavefront, one lane per row,
 * one evaluation sweep at x^ and an in-register Gauss-Jordan inversion); above, one workgroup per component: A in LDS up to 192
 * rows, in an HBM workspace above; the backward's LDL^T and, per node, two forward substitutions.  Components above 6144 rows:
 * LFR_ERR_UNSUPPORTED. */
typedef struct lfr_covariance_stats {
    int64_t n_computed;            /* components whose covariance was computed */
    int64_t n_not_usable;          /* FAILURE components (zeros) */
    int64_t n_singular;            /* components whose A met a pivot that is not positive (zeros) */
    double kernel_ms;              /* HIP-event time of the covariance's kernels (and its clearing of the output) */
} lfr_covariance_stats;

#define LFR_COVARIANCE_F64 1       /* the output is double instead of float32 (the float32 output is the fp64 result rounded once) */

/* cov_device: 3 * n_nodes float32 (double with LFR_COVARIANCE_F64) of the whole graph; the whole array is overwritten.  Runs on
 * `hip_stream` after the latest solve; asynchronous unless stats != NULL.  LFR_ERR_ARG before the first solve, and between an
 * lfr_batch_set_inputs and the next solve.  Changes nothing the solve or the backward read. */
int lfr_batch_covariance(lfr_batch *b, void *cov_device, int flags, void *hip_stream, lfr_covariance_stats *stats);
/* Per component (order of lfr_batch_component_info) of the latest covariance: 0 computed, 1 not usable, 2 singular.  Waits for that
 * call.  Returns the count (< 0: error, LFR_ERR_ARG before the first lfr_batch_covariance). */
int64_t lfr_batch_covariance_status(lfr_batch *b, int32_t *status);
/* Covariance between matched keypoints: what ceres::Covariance gives for a list of parameter-block PAIRS, with the graph's matches as
 * the list.  The nodes of a component are strongly correlated through its root, so the uncertainty of a match's relative displacement
 * x_node2 - x_node1 is not the sum of the two node blocks but
 *     D = Cov(x_2 - x_1) = C_11 + C_22 - C_12 - C_12^T,
 * and forming it downstream from float32 pieces cancels most of its digits.  The contract is that of lfr_batch_covariance - the same
 * A, the same usable components, the same status codes, taken after the latest solve (LFR_ERR_ARG before the first solve and between
 * an lfr_batch_set_inputs and the next solve), float32 outputs or double with LFR_COVARIANCE_F64, float32 = the fp64 value rounded
 * once - and the three outputs come from ONE assembly and ONE inversion per component.  Everything is in the solver's unit squared
 * and in the axis order of `positions`; there is no pixel mapping of the per-match outputs.
 *   - cov_device (may be NULL): 3 per node, exactly what lfr_batch_covariance writes, bit for bit;
 *   - cross_device (may be NULL): n_matches x 4 in the MATCH layout of lfr_batch_backward / lfr_batch_set_inputs / lfr_batch_evaluate.
 *     Row m = Cov(x_node1, x_node2) row-major: C(1di,2di), C(1di,2dj), C(1dj,2di), C(1dj,2dj).  0 where the true value is 0 or where
 *     there is no covariance: an end that is a root or another constant node, the two ends in different components (a dropped edge:
 *     independent, so exactly 0), a match outside the shard, a component with status 1 or 2;
 *   - rel_device (may be NULL): n_matches x 3, D(di,di), D(di,dj), D(dj,dj), formed in fp64 inside the kernel before any rounding to
 *     float32.  A constant end contributes zeros: a match with one constant end gets the other end's node block bit for bit.  A match
 *     whose direction node1->node2 is no residual block of this shard - a dropped edge, two constant ends, a match outside the shard -
 *     gets (-1, 0, -1): a negative variance is the "not in the program" mark, as lfr_batch_evaluate's weight -1.  A match of a
 *     status 1 / 2 component gets zeros, "no covariance", as in the node output;
 *   - whole arrays are overwritten.  All three outputs NULL, or a flag bit other than LFR_COVARIANCE_F64: LFR_ERR_ARG.  A batch over
 *     one rank's connected components (lfr_problem_cc_sharded = 1) numbers its matches by itself: LFR_ERR_UNSUPPORTED when a per-match
 *     output is asked for; cov alone is served.  Components above 6144 rows: LFR_ERR_UNSUPPORTED;
 *   - every match row is written once by a fixed rule (the record of direction node1->node2 writes it), no fp64 value goes through a
 *     global-memory atomic; results are bitwise repeatable, identical for host- and device-assembled batches, and components that
 *     share a wavefront do not influence each other, bit for bit;
 *   - lfr_batch_covariance_status serves this call too (the two calls share one pass state: it reports whichever ran last); streams,
 *     events and the asynchronous-unless-stats rule are those of lfr_batch_covariance.  The first call on a batch whose records do not
 *     carry their directed-edge ids builds the record -> edge map (a synchronising step; the graph must still be alive).
 * Kernels: up to 32 rows ONE launch in the covariance's packed layout - after the in-register inversion every row lane puts its row
 * of C into the group's LDS, then the lanes re-read their records' words and the node1->node2 records write their match; above, one
 * workgroup per component: the node blocks as in lfr_batch_covariance, then per node a back substitution c = L^-T D^-1 w for its two
 * full columns of C and a walk over the node's incident records. */
int lfr_batch_covariance_matches(lfr_batch *b, void *cov_device, void *cross_device, void *rel_device, int flags, void *hip_stream,
                                 lfr_covariance_stats *stats);
/* Consumer side, the counterpart of lfr_apply_displacements (colmap_utils.py:126-137): per feature of `image_name` the 2x2 covariance
 * in PIXELS and in keypoint (x, y) order, (16 * fact)^2 * [[C(dj,dj), C(di,dj)], [C(di,dj), C(di,di)]], as out[3f + 0..2] = xx, xy,
 * yy.  cov: 3 * n_nodes doubles on the host.  Features the graph does not know, roots and unsolved nodes get 0.  Host code. */
int lfr_keypoint_covariances(const lfr_graph *g, const double *cov, const char *image_name, float *out, int64_t num_features);
/* Unit-level probe of the packed classes' in-register inversion: n_sys symmetric matrices placed in waves exactly as
 * lfr_debug_solve_damped places systems (solver 0-3: n_rows <= 8, 16, 24, 32, even; 0 = an empty group).  A: the lower triangles,
 * packed row by row; Cinv: the inverses' full lower triangles in the same layout (row i as lane i holds it); status[s] = 0, or 2 when
 * a pivot was not positive (Cinv of that system is then zero).  Test infrastructure, not part of the covariance path. */
int lfr_debug_invert_spd(int device, int solver, int64_t n_sys, const int32_t *n_rows, const double *A, double *Cinv, int32_t *status);

/* ---------------------------------------------------------------------------------------------
 * Objective, gradient, residuals and loss weights at given positions (the counterpart of ceres::Problem::Evaluate).
 *
 * Contract.  Per solved-program component c of this shard, whatever its termination:
 *   F_c(x) = sum over the component's kept directed edges of 1/2 w_e rho_kind(e)(|r_e|^2),  r_e = x_dst - x_src - f(x_src; phi_e)
 * - the F of lfr_batch_backward's contract - with the records as they are NOW: after the latest lfr_batch_set_inputs, whether or not a
 * solve followed.
 *   - positions_device: 2 * n_nodes doubles of the whole graph on the batch's device, or NULL = the batch's own position array (NULL
 *     before the first solve: LFR_ERR_ARG; NULL between an lfr_batch_set_inputs and the next solve is allowed: the new records at the
 *     held positions).  Only variable nodes of this shard's components are read; roots and other constant nodes evaluate at 0 whatever
 *     the array holds there; nodes outside solved components are ignored.  Nothing is clamped to the +-1 box (the interpolant clamps
 *     its own argument, so F is defined everywhere).  With explicit positions the call needs no earlier solve;
 *   - cost_device (may be NULL): one double per component in the order of lfr_batch_component_info.  A component whose evaluation is
 *     not finite gets that non-finite value and nothing else is affected;
 *   - grad_positions_device (may be NULL): 2 * n_nodes doubles, the whole array is overwritten: dF/dx per coordinate of the variable
 *     nodes - no projection onto the box, no free / bound distinction - and 0 for constant nodes, nodes outside solved components and
 *     nodes outside the shard.  Per edge the destination gets w rho' r, the source -w rho' P^T r, P = I + df/dx_src, the derivative
 *     of the interpolant zeroed outside [-0.5, 0.5] and kept at exactly +-0.5 (cost.cc:38-43);
 *   - residuals_device (n_matches x 4) and weights_device (n_matches x 2), float32 or double with LFR_EVALUATE_F64, either may be
 *     NULL, whole arrays are overwritten; the MATCH layout of lfr_batch_backward / lfr_batch_set_inputs.  Row m of the residuals:
 *     (r_di, r_dj) of edge node1->node2, then of edge node2->node1 - raw residuals in the solver's unit, not loss-corrected.  Row m of
 *     the weights: rho'(|r|^2) of the same two edges (1 at a zero residual, 0 for a saturated Tukey edge; the similarity is not folded
 *     in).  A direction that is no residual block of this shard - a dropped edge, an edge between two constant nodes, a match outside
 *     the shard - gets residual 0 and weight -1: "turned off by the loss" (0) differs from "not in the program" (-1);
 *   - all four outputs NULL, or a flag bit other than LFR_EVALUATE_F64: LFR_ERR_ARG.  A batch over one rank's connected components
 *     (lfr_problem_cc_sharded = 1) numbers its matches by itself: LFR_ERR_UNSUPPORTED when a per-match output is asked for; cost and
 *     gradient are served.  There is no row limit: nothing here needs a matrix;
 *   - outputs are bitwise repeatable from call to call, identical for host- and device-assembled batches and whether the records of
 *     a device-assembled whole batch were materialised by this call or by a second solve; components that share a wavefront do not
 *     influence each other, bit for bit.  No fp64 value goes through a global-memory atomic;
 *   - runs on `hip_stream`, asynchronous unless stats != NULL.  Waits BY EVENT for the latest lfr_batch_set_inputs and the latest
 *     solve, whatever streams they ran on; lfr_batch_set_inputs in turn waits for the latest evaluate.  Between a LATER solve and an
 *     evaluate the caller orders the streams, as for lfr_batch_backward / lfr_batch_covariance.  The first call that asks for a
 *     per-match output on a batch whose records do not carry their directed-edge ids builds the record -> edge map (a synchronising
 *     step; the graph must still be alive: LFR_ERR_ARG otherwise).
 * Kernels (lfr_evaluate.hip): components of up to 32 rows in ONE launch in the solve's packed layout (64/S components per wavefront,
 * every record read once, cost by a fixed-order lane reduction, gradient accumulated in the group's LDS); above, one workgroup per
 * component, owner computes: the thread of a node sums its gradient over the node's out- and in-edges in record order, the out-edge
 * visit stores the per-match outputs and the cost term, the cost is a fixed wave-then-block tree. */
typedef struct lfr_evaluate_stats {
    int64_t n_components;          /* components evaluated (every solved-program component of the shard, whatever its termination) */
    int64_t n_nonfinite;           /* components whose cost is not finite */
    double sum_cost;               /* sum of the finite component costs, in descriptor order */
    double kernel_ms;              /* HIP-event time of the call's kernels (and its clearing of the outputs) */
} lfr_evaluate_stats;

#define LFR_EVALUATE_F64 1         /* residuals / weights are double instead of float32 (float32 = the fp64 value rounded once) */

int lfr_batch_evaluate(lfr_batch *b, const double *positions_device, double *cost_device, double *grad_positions_device,
                       void *residuals_device, void *weights_device, int flags, void *hip_stream, lfr_evaluate_stats *stats);

/* ---------------------------------------------------------------------------------------------
 * The vector-Jacobian product of lfr_batch_evaluate's differentiable outputs: the objective differentiated in its inputs.
 *
 * Contract.  With bars cbar_c (per component), rbar_e (per raw residual) and wbar_e (per weight rho'_e), the call returns the
 * gradient of  sum_c cbar_c F_c + sum_e rbar_e . r_e + sum_e wbar_e rho'_e  with respect to the positions, the flows and the
 * similarities, at the given positions, with the records as they are NOW - the EXPLICIT partials; the dependence of the positions
 * on the flows is lfr_batch_backward's.  Per kept directed edge e of component c everything follows from one 2-vector
 *     q_e = cbar_c w_e rho'_e r_e  +  rbar_e  +  wbar_e 2 rho''_e r_e
 * where r, rho' and P = I + df/dx_src are exactly lfr_batch_evaluate's (the derivative of the interpolant zeroed outside [-0.5, 0.5]
 * and kept at exactly +-0.5; nothing is clamped to the +-1 box) and rho'' is lfr_batch_backward's: Cauchy -1 / (b (1 + s/b)^2), Tukey
 * -6 k / a^4 (1 - s/a^2) inside and 0 where saturated.
 *   - positions_device: as for lfr_batch_evaluate (NULL = the batch's own; NULL before the first solve: LFR_ERR_ARG; NULL between an
 *     lfr_batch_set_inputs and the next solve is allowed);
 *   - cost_bar_device: one double per component in the order of lfr_batch_component_info; residuals_bar_device (n_matches x 4) and
 *     weights_bar_device (n_matches x 2) in lfr_batch_evaluate's match layout.  Any bar may be NULL = zero; all three NULL:
 *     LFR_ERR_ARG.  The bars of a direction that is no residual block of this shard (a dropped edge, two constant ends, outside the
 *     shard) are not read;
 *   - grad_positions_device (may be NULL): 2 * n_nodes doubles, the whole array is overwritten.  Per edge the destination adds +q_e,
 *     the source -P_e^T q_e; only variable nodes receive a gradient: constants, unsolved nodes and nodes outside the shard get 0;
 *   - grad_disp1_device / grad_disp2_device (n_matches x 18, both or neither; one alone: LFR_ERR_ARG): the flow gradient of an edge,
 *     g[6 i + 2 j + k] = -Lr_i(x_src) Lc_j(x_src) q_k with the basis values of the clamped argument, in row m of grad_disp2 for the
 *     edge node1->node2 of match m and of grad_disp1 for node2->node1 - the layout of lfr_batch_backward's gradients.  A saturated
 *     Tukey edge gets nothing from cbar and wbar, but its rbar passes;
 *   - grad_sim_device (n_matches, may be NULL): the sum over the match's two directions of cbar_c 1/2 rho_e(s_e), node1->node2 first
 *     (residuals and weights do not depend on the similarity);
 *   - directions that are no residual block of this shard leave 0 in every per-match output; whole arrays are overwritten;
 *   - LFR_EVALUATE_F64: every per-match array - bars and gradients - is double; otherwise float32, each float32 output the fp64 value
 *     rounded once.  cost_bar and grad_positions are always double.  Any other flag bit: LFR_ERR_ARG.  All four outputs NULL:
 *     LFR_ERR_ARG.  Every argument error is raised before an output is touched;
 *   - a batch over one rank's connected components (lfr_problem_cc_sharded = 1): LFR_ERR_UNSUPPORTED as soon as a per-match bar or a
 *     per-match output is given; cost_bar -> grad_positions alone is served.  There is no row limit: nothing here needs a matrix;
 *   - a bar, flow or similarity that is not finite makes the outputs of its own component not finite and changes no other component
 *     by a bit, one in the same wavefront included; stats->n_nonfinite counts the components with a q that is not finite;
 *   - outputs are bitwise repeatable from call to call and identical for host- and device-assembled batches.  No fp64 value goes
 *     through a global-memory atomic; every match row is written by exactly one record; the two directions' similarity terms go
 *     through a per-direction scratch and one combine pass in a fixed order;
 *   - runs on `hip_stream`, asynchronous unless stats != NULL.  Waits BY EVENT for the latest solve and the latest
 *     lfr_batch_set_inputs; lfr_batch_set_inputs in turn waits for the latest lfr_batch_evaluate_vjp.  A device-assembled batch whose
 *     records are not yet written materialises them first, and the first call with a per-match argument builds the record -> edge
 *     map, both as lfr_batch_evaluate does.  Two calls in flight at once on different streams share the similarity scratch: the
 *     caller orders them.
 * Kernels (lfr_evaluate.hip): lfr_batch_evaluate's two launches run backwards.  Packed classes: each record lane forms q, stores its
 * own flow row and its direction's similarity term and accumulates the two position sides in the group's LDS in the evaluate's
 * order; no barriers.  Workgroup classes: the thread of a node forms q on its out-edges (flow row, similarity term, source side) and
 * again, from that record's bars, on its in-edges (destination side); constants walk their out-edges only. */
typedef struct lfr_evaluate_vjp_stats {
    int64_t n_components;          /* components swept (every solved-program component of the shard, whatever its termination) */
    int64_t n_nonfinite;           /* components with a q that is not finite */
    double kernel_ms;              /* HIP-event time of the call's kernels (and its clearing of the outputs) */
} lfr_evaluate_vjp_stats;

int lfr_batch_evaluate_vjp(lfr_batch *b, const double *positions_device,
                           const double *cost_bar_device,        /* per component, order of lfr_batch_component_info */
                           const void *residuals_bar_device,     /* n_matches x 4 */
                           const void *weights_bar_device,       /* n_matches x 2 */
                           double *grad_positions_device,        /* 2 * n_nodes */
                           void *grad_disp1_device, void *grad_disp2_device,   /* n_matches x 18 */
                           void *grad_sim_device,                /* n_matches */
                           int flags, void *hip_stream, lfr_evaluate_vjp_stats *stats);

/* ---------------------------------------------------------------------------------------------
 * Matrix-free products with the second-order matrix of the objective at given positions: H v per component, nothing assembled.
 *
 * Contract.  Per solved-program component c of this shard, whatever its termination, over ALL coordinates of its variable nodes:
 *   - the matrix.  Default: the exact Hessian of lfr_batch_evaluate's F_c at the given positions, with the records as they are NOW -
 *     per kept directed edge the block [[P^T M P - w rho' sum_k r_k d2f_k, -P^T M], [-M P, M]] over (x_src, x_dst), M = w (rho' I +
 *     2 rho'' r r^T), P = I + df/dx_src: the matrix lfr_batch_backward factors, without its row limit and at any positions.
 *     LFR_HVP_GAUSS_NEWTON: M = w rho' I and no second-derivative term, the J^T J of lfr_batch_covariance and of the LM loop, undamped
 *     and unscaled.  Both with the derivative of the interpolant zeroed outside [-0.5, 0.5] and kept at exactly +-0.5
 *     (cost.cc:38-43), the second derivative with it; rho' and rho'' are lfr_batch_backward's (Cauchy: rho' >= DBL_MIN);
 *   - positions_device: exactly lfr_batch_evaluate's - 2 * n_nodes doubles, or NULL = the batch's own array (NULL before the first
 *     solve: LFR_ERR_ARG; NULL between an lfr_batch_set_inputs and the next solve is allowed).  Nothing is clamped; constants evaluate
 *     at 0 whatever the array holds there;
 *   - vectors_device: n_vectors arrays of 2 * n_nodes doubles in the layout of the positions, one after the other,
 *     1 <= n_vectors <= LFR_HVP_MAX_VECTORS.  Only the coordinates of variable nodes of this shard's components are read; everything
 *     else is ignored and counts as 0;
 *   - the +-1 box is ignored (lfr_batch_covariance's and lfr_batch_evaluate's convention) unless LFR_HVP_FREE_SET is given: then the
 *     coordinates with |x| >= 1 at the given positions are identity rows and columns, as in lfr_batch_backward - at such an i
 *     (H v)_i = v_i, and v_i enters no other row;
 *   - products_device (n_vectors x 2 * n_nodes, may be NULL): the whole array is overwritten; constants, unsolved nodes and nodes
 *     outside the shard get 0;
 *   - curvature_device (n_vectors x n_components, may be NULL): curvature[k * n_components + c] = sum_i v_i (H v)_i of vector k over
 *     component c's variable coordinates, c in the order of lfr_batch_component_info, summed in a fixed order (packed classes: one
 *     term per lane through the group's butterfly; workgroup classes: a wave-then-block tree);
 *   - LFR_ERR_ARG, before any output is touched: both outputs NULL, vectors_device NULL, n_vectors out of range, a flag bit other
 *     than the two defined.  There is no row limit - nothing here needs a matrix - and batches over one rank's connected components
 *     (lfr_problem_cc_sharded = 1) are served: everything is per node;
 *   - a vector entry, flow or similarity that is not finite makes the outputs of its own component not finite and changes no other
 *     component by a bit, one in the same wavefront included; stats->n_nonfinite counts the components with a product entry that is
 *     not finite;
 *   - outputs are bitwise repeatable from call to call and identical for host- and device-assembled batches; the outputs of vector k
 *     are the same bits whether it is passed alone or among others, whatever the others hold.  No fp64 value goes through a
 *     global-memory atomic;
 *   - runs on `hip_stream`, asynchronous unless stats != NULL.  Waits BY EVENT for the latest solve and the latest
 *     lfr_batch_set_inputs; lfr_batch_set_inputs in turn waits for the latest product.  A device-assembled batch whose records are
 *     not yet written materialises them first, as lfr_batch_evaluate does.
 * Kernels (lfr_hessian_product.hip): lfr_batch_evaluate's two layouts, the per-edge arithmetic of lfr_batch_backward's assembly
 * (bwd_eval, bwd_blocks) done once per record for all vectors.  Packed classes: per record and vector t = M (v_dst - P v_src), the
 * destination adds t, the source -P^T t minus the second-derivative term times v_src, accumulated in the group's LDS.  Workgroup
 * classes: the thread of a variable node sums its two rows over the node's out- and in-edges in record order. */
typedef struct lfr_hessian_product_stats {
    int64_t n_components;          /* components swept (every solved-program component of the shard, whatever its termination) */
    int64_t n_nonfinite;           /* components with a product entry that is not finite */
    int64_t n_bound_coordinates;   /* with LFR_HVP_FREE_SET: coordinates treated as bound; else 0 */
    double kernel_ms;              /* HIP-event time of the call's kernels (and its clearing of the outputs) */
} lfr_hessian_product_stats;

#define LFR_HVP_GAUSS_NEWTON 2     /* the loss-corrected Gauss-Newton matrix instead of the exact Hessian */
#define LFR_HVP_FREE_SET 4         /* coordinates at the +-1 bound are identity rows and columns */
#define LFR_HVP_MAX_VECTORS 4

int lfr_batch_hessian_product(lfr_batch *b, const double *positions_device, const double *vectors_device, int n_vectors,
                              double *products_device,      /* n_vectors x 2 * n_nodes, may be NULL */
                              double *curvature_device,     /* n_vectors x n_components, may be NULL */
                              int flags, void *hip_stream, lfr_hessian_product_stats *stats);

/* ---------------------------------------------------------------------------------------------
 * Matrix-free linear solves with that matrix: (H + damping I) y = b per component by preconditioned conjugate gradients, the whole
 * iteration inside the kernel, every component stopping on its own.
 *
 * Contract.  Per solved-program component c of this shard, whatever its termination:
 *   - the matrix.  A = H + damping I, H exactly the matrix of lfr_batch_hessian_product under the same flags (the exact Hessian, or
 *     J^T J with LFR_HSOLVE_GAUSS_NEWTON; LFR_HSOLVE_FREE_SET makes the coordinates with |x| >= 1 identity rows and columns), with
 *     the records as they are NOW and lfr_batch_hessian_product's rules for positions_device (NULL = the batch's own array; NULL
 *     before the first solve: LFR_ERR_ARG).  With the free set a bound coordinate gets y_i = b_i, the very bits: it enters no other
 *     row and no norm, and the damping is not added there;
 *   - the method.  Preconditioned conjugate gradients from y = 0.  The preconditioner is the inverse of every variable node's own
 *     2x2 diagonal block of A: M summed over the node's in-edges, P^T M P minus the second-derivative term over its out-edges, plus
 *     the damping; a bound coordinate is the identity's in its block.  A block that is not finite, or has a00 <= 0 or det <= 0
 *     (the exact mode can), is replaced by the identity for that node;
 *   - the stop.  After every step the residual r of the recurrence is tested: LFR_HSOLVE_OK when |r|_2 <= rel_tolerance |b|_2, both
 *     norms over the component's variable coordinates that are not bound.  b = 0 there: y = 0, LFR_HSOLVE_OK, 0 iterations.
 *     LFR_HSOLVE_MAX_ITERATIONS after max_iterations steps: y is the last iterate;
 *   - negative curvature.  LFR_HSOLVE_NEGATIVE_CURVATURE when a search direction p has p . A p <= 0: y is the iterate reached BEFORE
 *     that direction (zeros when it was the first), the rule of a truncated Newton step.  LFR_HSOLVE_OK does NOT certify that H is
 *     positive definite: conjugate gradients only ever see the Krylov space of b;
 *   - LFR_HSOLVE_NONFINITE when b (off the bound coordinates), a record or an intermediate of the component is not finite; its
 *     outputs may be non-finite.  No other component changes by a bit, one in the same wavefront included;
 *   - rhs_device / solutions_device: n_rhs arrays of 2 * n_nodes doubles in the layout of the positions, 1 <= n_rhs <=
 *     LFR_HVP_MAX_VECTORS.  The whole solutions array is overwritten; constants, unsolved nodes and nodes outside the shard get 0;
 *   - status_device, iterations_device, residual_device (each may be NULL): n_rhs x n_components, entry [k * n_components + c], c in
 *     the order of lfr_batch_component_info: the status above, the steps taken, the final |r|_2 / |b|_2 of the recurrence (0 for
 *     b = 0);
 *   - LFR_ERR_ARG, before any output is touched: no batch, rhs_device or solutions_device NULL, n_rhs out of range, a flag bit other
 *     than the two defined, damping negative or not finite, rel_tolerance negative or NaN, max_iterations < 1, NULL positions before
 *     the first solve.  There is no row limit and batches over one rank's connected components are served;
 *   - every sum has a fixed order (packed classes: the group's butterfly; workgroup classes: a wave-then-block tree and rows summed
 *     by their owner in record order) and no fp64 value goes through a global-memory atomic: outputs are bitwise repeatable from
 *     call to call and identical for host- and device-assembled batches; the outputs of right-hand side k are the same bits whether
 *     it is passed alone or among others, whatever the others hold - one that is done is frozen while the others go on;
 *   - runs on `hip_stream`, asynchronous unless stats != NULL; waits by event as lfr_batch_hessian_product does, and
 *     lfr_batch_set_inputs waits for the latest solve of this kind.  All calls on a batch iterate in one workspace: a call on
 *     another stream waits by event for the latest call, so calls of one batch run one after the other, in the order they were made.
 * Kernels (lfr_hessian_solve.hip): every record's blocks M, P, S are formed once per call.  Packed classes: in the registers of the
 * record's lane, p and A p in the group's LDS.  Workgroup classes: one persistent workgroup per component, the blocks in an 80-byte
 * slot per record of the pass's workspace, r, p, A p by global node id there, y in solutions_device. */
typedef struct lfr_hessian_solve_stats {
    int64_t n_components;          /* components swept */
    int64_t n_converged, n_max_iterations, n_negative_curvature, n_nonfinite;   /* over all (rhs, component) pairs */
    int64_t sum_iterations, max_iterations_used;
    int64_t n_bound_coordinates;   /* with LFR_HSOLVE_FREE_SET: coordinates treated as bound; else 0 */
    double kernel_ms;              /* HIP-event time of the call's kernels (and its clearing of the solutions) */
} lfr_hessian_solve_stats;

#define LFR_HSOLVE_GAUSS_NEWTON 2  /* same bit values as LFR_HVP_* */
#define LFR_HSOLVE_FREE_SET 4
#define LFR_HSOLVE_OK 0
#define LFR_HSOLVE_MAX_ITERATIONS 1
#define LFR_HSOLVE_NEGATIVE_CURVATURE 2
#define LFR_HSOLVE_NONFINITE 3

int lfr_batch_hessian_solve(lfr_batch *b, const double *positions_device,
                            const double *rhs_device, int n_rhs,          /* n_rhs x 2 * n_nodes, 1..LFR_HVP_MAX_VECTORS */
                            double damping, double rel_tolerance, int max_iterations,
                            double *solutions_device,                     /* n_rhs x 2 * n_nodes, required */
                            int32_t *status_device, int32_t *iterations_device, double *residual_device, /* n_rhs x n_components, each may be NULL */
                            int flags, void *hip_stream, lfr_hessian_solve_stats *stats);

/* Unit-level probe of the device arithmetic (cost.cc:13-48,78-90 + the loss / corrector of solve.cc:111,120): for
 * each of n edges (flows n x 18 float32, sim, kind 0 = intra-track/Cauchy 1 = inter-track/Tukey, x1 = source and
 * x2 = destination position) the kernels' eval_edge on the GPU: out8[8i..] = 0.5*rho, corrected residual r0 r1,
 * corrected d r / d x1 (j00 j01 j10 j11), sqrt(rho') (= d r / d x2 diagonal); cost_only[i] = 0.5*rho from the
 * cost-only variant the line search uses.  Test infrastructure for parity at 1e-12, not part of the solve path. */
int lfr_debug_eval_edges(int device, int64_t n, const float *flows, const float *sim, const int32_t *kind, const double *x1,
                         const double *x2, int tukey_variant, double *out8, double *cost_only);

/* Unit-level probe of the Armijo line search's step contraction (Ceres line_search.cc ArmijoLineSearch::DoSearch +
 * polynomial.cc MinimizeInterpolatingPolynomial): for each of n cases, samples holds 15 doubles = (x, value, gradient,
 * value_valid, gradient_valid) of the initial, the previous and the current sample; step[i] = the next step size the kernels
 * compute (negative: the search gives up); register_version 0 = the loop version the packed kernel calls, 1 = the unrolled
 * version of the workgroup-per-component kernel, 2 = the wave-cooperative form of the elimination-tree kernel (the pieces of the
 * root isolation a lane each; one case per wave).  Test infrastructure, not part of the solve path. */
int lfr_debug_ls_next_step(int device, int64_t n, const double *samples, const double *dir_max, int register_version, double *step);
/* Unit-level probe of the LM step solves: for each of n_sys systems (A + D) y = g, the solve of one solver kernel on the GPU.  solver
 * 0-3 = the packed classes' Gauss-Jordan elimination <8,1,3>, <16,1,6>, <32,1,6>, <32,2,5> (n_rows <= 8, 16, 24, 32; 0 = an empty group;
 * the groups of a wave take consecutive systems - 8, 4, 2, 1 per wave - exactly as the packed kernel places components, so the caller
 * decides which systems share a wave); 4-6 = the blocked LDL^T and back substitution of the workgroup classes of up to 88, 130, 192 rows
 * (n_rows >= 2; one workgroup per system, all in one launch, the class's full LDS).  n_rows even.  A: the lower triangles, packed row
 * by row (element (i, j), j <= i, at i (i + 1) / 2 + j), one system after the other; damp, g, y: n_rows[s] doubles per system.  The
 * damping goes onto the diagonal as each kernel adds it: a_ii + damp_i (packed: the kernels' dd) or a_ii + damp_i * damp_i with one
 * rounding (workgroup classes: the kernels' D / s, a fused multiply-add).  y solves (A + D) y = g: the LM step the kernels take is -y.
 * status[s] = 0 for a valid solve; bit 0: the kernel found a pivot that is not positive (its y is NaN), bit 1: a bounded spin-wait of
 * the factorization ran out.  Test infrastructure, not part of the solve path. */
int lfr_debug_solve_damped(int device, int solver, int64_t n_sys, const int32_t *n_rows, const double *A, const double *damp, const double *g,
                           double *y, int32_t *status);
/* Unit-level probe of the LM step solve of the elimination-tree kernel (components above 192 rows: the level-scheduled sparse LDL^T of
 * solve_tree_component): for each of n_sys systems (A + D) y = g, ONE factorization and back substitution by the device code of the
 * solve - the column tasks with their left-looking updates on the matrix cores, the barrier-free schedule of thin plans with the tiles
 * finished behind the elimination, the barrier schedule with its tile and extra-row tasks, the back substitution - on the caller's
 * matrix instead of a sweep's.  One workgroup per system (a team of one), all systems in one launch; a system's workspace behind the
 * plan's words is filled with NaN before the kernel's own prologue runs.  blobs: the plans as lfr_debug_tree_plan returns them, one
 * after the other, blob_words[s] words each (at most 4096 blocks).  tiles: the values of A in the plan's tile layout, n_tiles x 16 x 16
 * doubles per system (tile t = rows of block rowsof[t], columns of the block whose colptr range holds t, row-major; the diagonal tile
 * first in each column, its lower triangle read; tiles that are fill only: zero).  damp, g, y: n_pad = 16 x blocks doubles per system
 * in MATRIX order (row 2 p + c of node position p), zero at padding rows.  The damping goes onto the diagonal tiles as the LM loop puts
 * it there: damp is the kernels' D / s, the column task adds damp_i * damp_i (a product and a sum, each rounded).  y solves
 * (A + D) y = g (the LM step is -y) and is exactly 0 at padding rows.  status[s] = 0 for a valid solve; bit 0: a pivot was not positive
 * (y of that system is NaN), bit 1: a bounded spin-wait ran out.  Test infrastructure, not part of the solve path. */
int lfr_debug_solve_tree(int device, int64_t n_sys, const int64_t *blob_words, const uint32_t *blobs, const double *tiles, const double *damp,
                         const double *g, double *y, int32_t *status);
/* The library's persistent host workers (they make the elimination-tree plans of a batch, solve.cc:79-143 for components above 192 rows:
 * the reference builds one problem per pool thread, solve.cc:617-635): `items` increments of one counter dealt to `threads` threads, the
 * caller among them, `reps` times.  Returns the number of increments performed (items * reps when nothing was lost).  Callable from
 * several threads at once (a caller that finds the workers busy runs on threads of its own).  Test infrastructure. */
int64_t lfr_debug_pool_selftest(int threads, int64_t items, int reps);

/* The pipeline's stable device sort of (key, value) pairs (graph stage: matches by similarity, solve.cc:489-497; assembly: nodes and
 * edges by component, solve.cc:563-597 - the reference sorts on the host with std::sort / visits in order): n pairs of key_bytes (4 or 8)
 * byte unsigned keys and 32-bit values, ascending by key bits [begin_bit, end_bit), equal keys in input order.  use_library 0 = the
 * library's driver (one-sweep radix passes with ONE clearing fill per sort above 256 K pairs, lfr_sort.hpp), 1 = rocprim::radix_sort_pairs.
 * Test infrastructure, not part of the solve path. */
int lfr_debug_sort_pairs(int device, int64_t n, int key_bytes, const void *keys, const uint32_t *vals, int begin_bit, int end_bit,
                         int use_library, void *keys_out, uint32_t *vals_out);

/* The pipeline's one-launch exclusive prefix sum (lfr_sort.hpp: decoupled look-back over states that lie in a stage's zero block): n items
 * of item_bytes (4 or 8) byte unsigned integers; out[i] = in[0] + ... + in[i-1] (32-bit sums wrap, 64-bit sums must stay below 2^62).
 * Test infrastructure, not part of the solve path. */
int lfr_debug_exclusive_sum(int device, int64_t n, int item_bytes, const void *in, void *out);

/* Keeps `workgroups` CUs of the device busy for `milliseconds` (512-thread workgroups at the elimination-tree kernel's register budget, on
 * a stream of their own; returns when they have started): the tests take CUs away from a solve with it (lfr_batch_team_fallbacks).
 * Test infrastructure, not part of the solve path. */
int lfr_debug_occupy(int device, int workgroups, double milliseconds);

/* Where the time of this thread's latest lfr_graph_from_device_arrays went, in ms, into ms[0..n): expand, sort, head flags + prefix
 * sums, heads + scatter (device time between events; 0 unless the environment held LFR_GRAPHBUILD_SPANS=1 at the process's first such
 * call - the switch puts one more stream wait into the call, in front of the host mirror, and changes no result), then host mirror,
 * finish() and the host's pair table (host clock, always).  Diagnostic only (scripts/bench_graph_from_device.py): neither the
 * function nor the switch is part of the producer contract. */
int lfr_debug_graph_build_spans(double *ms, int n);

/* One-call convenience used by the `solve` launcher: upload, solve, download on one device. */
int lfr_solve_hip(const lfr_problem *p, int device, int tukey_variant, double *positions,
                  lfr_solve_stats *stats);

/* The same over several GPUs of one node from ONE process: the solvable components are dealt to
 * `n_devices` shards (lfr_problem_shard_components), one host thread per device assembles (on its GPU, for a
 * labels-only problem) or uploads (host-assembled problem), solves and downloads its shard; shards write
 * disjoint node sets of `positions` (the thread pool of solve.cc:617-635 with GPUs as workers). */
int lfr_solve_hip_multi(const lfr_problem *p, const int *devices, int n_devices, int tukey_variant, double *positions,
                        lfr_solve_stats *stats);

/* solve.cc:487-641 over several GPUs from ONE process, the graph stage included: device k runs tracks / roots / components, the assembly
 * and the solve over the connected components of the match graph dealt to shard k (lfr_problem_build_hip_shard) - nothing is computed
 * on one GPU for the others.  problem_stats: what the stdout lines of solve.cc:534-606 need, summed / maximised over the shards.
 * A graph that is one connected component cannot be dealt out: every device then holds the whole problem and solves its share of the
 * components (as lfr_solve_hip_multi).  positions: 2 * n_nodes doubles, every node written (zeros where nothing is solved). */
int lfr_solve_graph_hip_multi(const lfr_graph *g, const int *devices, int n_devices, int64_t max_nodes_in_component, int tukey_variant,
                              double *positions, lfr_problem_stats *problem_stats, lfr_solve_stats *stats);

/* ---------------------------------------------------------------------------------------------
 * A12  SolutionFile emit.                                                     solve.cc:644-679
 * ------------------------------------------------------------------------------------------- */
/* Writes types.proto:30-46; returns through n_outside the count printed at solve.cc:666-670. */
int lfr_write_solution(const lfr_graph *g, const double *positions, const char *path, int64_t *n_outside);

/* The consumer's arithmetic as a library call (colmap_utils.py:126-137) — lets a caller skip the
 * SolutionFile round trip: for every node of `image_name`, keypoints[feature_idx][0] += dj*fact*16,
 * keypoints[feature_idx][1] += di*fact*16 (float32, same operation order), then +0.5 on both
 * coordinates of all `num_features` rows.  An image the graph does not know only gets the +0.5
 * (colmap_utils.py:127-128).  keypoints: num_features rows of `stride` floats (x, y, ...). */
int lfr_apply_displacements(const lfr_graph *g, const double *positions, const char *image_name, float *keypoints,
                            int64_t num_features, int64_t stride);

#ifdef __cplusplus
}
#endif
#endif /* LFR_H */
