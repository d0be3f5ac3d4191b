"""ctypes binding of liblfr_hip.so (C ABI: include/lfr.h).

This is the host-side mirror of the reference's solver stages (``solve.cc`` main():
ingest -> tracks/roots/components -> batched LM -> SolutionFile).  There is no CPU
fallback: if the HIP library is missing, importing the binding raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LFR_LIB_OVERRIDE") or os.path.join(_HERE, "liblfr_hip.so")   # override: A/B of kernel variants

TUKEY = {"ceres1": 1, "ceres2": 2}
TERM_CONVERGENCE, TERM_NO_CONVERGENCE, TERM_FAILURE = 0, 1, 2


class LfrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("lfr error %d: %s" % (code, msg))
        self.code = code


NUM_KERNEL_CLASSES = 9          # LFR_NUM_KERNEL_CLASSES


class ProblemStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in (
        "n_tracks", "max_track_size", "n_components", "max_component_size", "n_cut_components",
        "n_solved_components", "n_solved_tracks", "n_solved_edges", "n_solved_nodes")] + \
        [(n, C.c_double) for n in ("tracks_ms", "roots_ms", "graph_cut_ms", "assemble_ms", "kruskal_rounds", "tie_resorts")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SolveStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in (
        "n_components", "n_edges", "n_nodes", "n_tracks", "n_converged", "n_no_convergence", "n_failed",
        "sum_iterations", "ref_jacobian_passes_edges", "ref_cost_passes_edges", "exec_passes_edges",
        "ref_passes_nodes")] + \
        [("sum_final_cost", C.c_double), ("kernel_ms", C.c_double), ("h2d_ms", C.c_double),
         ("d2h_ms", C.c_double), ("dominant_kernel_ms", C.c_double),
         ("dominant_kernel_edges", C.c_int64), ("dominant_kernel_nodes", C.c_int64),
         ("dominant_ref_passes_edges", C.c_int64), ("dominant_ref_passes_nodes", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BackwardStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_differentiated", "n_not_usable", "n_indefinite", "n_bound_coordinates")] + \
        [("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CovarianceStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_computed", "n_not_usable", "n_singular")] + [("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class EvaluateStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_components", "n_nonfinite")] + [("sum_cost", C.c_double), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class EvaluateVjpStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_components", "n_nonfinite")] + [("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class HessianProductStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_components", "n_nonfinite", "n_bound_coordinates")] + [("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class HessianSolveStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_components", "n_converged", "n_max_iterations", "n_negative_curvature", "n_nonfinite",
                                         "sum_iterations", "max_iterations_used", "n_bound_coordinates")] + [("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class JvpStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_differentiated", "n_not_usable", "n_indefinite", "n_bound_coordinates")] + [("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


BACKWARD_F64 = 1                # LFR_BACKWARD_F64
BACKWARD_GAUSS_NEWTON = 2       # LFR_BACKWARD_GAUSS_NEWTON
BACKWARD_FALLBACK_GAUSS_NEWTON = 32      # LFR_BACKWARD_FALLBACK_GAUSS_NEWTON
BACKWARD_OK, BACKWARD_NOT_USABLE, BACKWARD_INDEFINITE, BACKWARD_FALLBACK = 0, 1, 2, 3      # lfr_batch_backward_status
JVP_F64 = 1                     # LFR_JVP_F64
JVP_GAUSS_NEWTON = 2            # LFR_JVP_GAUSS_NEWTON
JVP_FALLBACK_GAUSS_NEWTON = 32  # LFR_JVP_FALLBACK_GAUSS_NEWTON
JVP_OK, JVP_NOT_USABLE, JVP_INDEFINITE, JVP_FALLBACK = 0, 1, 2, 3      # lfr_batch_jvp_status
COVARIANCE_F64 = 1              # LFR_COVARIANCE_F64
COVARIANCE_OK, COVARIANCE_NOT_USABLE, COVARIANCE_SINGULAR = 0, 1, 2     # lfr_batch_covariance_status
EVALUATE_F64 = 1                # LFR_EVALUATE_F64
HVP_GAUSS_NEWTON = 2            # LFR_HVP_GAUSS_NEWTON
HVP_FREE_SET = 4                # LFR_HVP_FREE_SET
HVP_MAX_VECTORS = 4             # LFR_HVP_MAX_VECTORS
HSOLVE_GAUSS_NEWTON = 2         # LFR_HSOLVE_GAUSS_NEWTON
HSOLVE_FREE_SET = 4             # LFR_HSOLVE_FREE_SET
HSOLVE_OK, HSOLVE_MAX_ITERATIONS, HSOLVE_NEGATIVE_CURVATURE, HSOLVE_NONFINITE = 0, 1, 2, 3      # status of lfr_batch_hessian_solve


_lib = None


def lib():
    """Load liblfr_hip.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s not found: build it with `python __graft_entry__.py` "
                          "(there is no CPU fallback for the solver path)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    pp = C.POINTER(C.c_void_p)
    cpp = C.POINTER(C.c_char_p)
    sig = {
        "lfr_version": (C.c_int, []),
        "lfr_last_error": (C.c_char_p, []),
        "lfr_graph_from_files": (C.c_int, [cpp, C.c_int, cpp, C.c_int, pp]),
        "lfr_graph_from_matches_file": (C.c_int, [C.c_char_p, cpp, C.c_int, pp]),
        "lfr_graph_from_matches_file_device": (C.c_int, [C.c_char_p, cpp, C.c_int, C.c_int, pp]),
        "lfr_graph_from_arrays": (C.c_int, [i32, cpp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, cpp, C.c_int, pp]),
        "lfr_graph_from_arrays_device_flows": (C.c_int, [i32, cpp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, cpp, C.c_int, pp]),
        "lfr_graph_from_device_arrays": (C.c_int, [i32, cpp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, cpp, C.c_int, pp]),
        "lfr_debug_graph_build_spans": (C.c_int, [vp, C.c_int]),
        "lfr_graph_to_device": (C.c_int, [vp, C.c_int]),
        "lfr_graph_evict_device": (C.c_int, [vp]),
        "lfr_graph_free": (None, [vp]),
        "lfr_graph_num_nodes": (i64, [vp]),
        "lfr_graph_num_edges": (i64, [vp]),
        "lfr_graph_num_images": (i32, [vp]),
        "lfr_graph_get_nodes": (C.c_int, [vp, vp, vp]),
        "lfr_graph_image_name": (C.c_char_p, [vp, i32]),
        "lfr_graph_image_fact": (C.c_float, [vp, i32]),
        "lfr_write_matching_file": (C.c_int, [C.c_char_p, i32, cpp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
        "lfr_problem_build": (C.c_int, [vp, i64, vp, pp]),
        "lfr_problem_build_labels": (C.c_int, [vp, i64, vp, pp]),
        "lfr_problem_build_hip": (C.c_int, [vp, C.c_int, i64, vp, pp]),
        "lfr_problem_build_hip_ex": (C.c_int, [vp, C.c_int, i64, vp, C.c_int, pp]),
        "lfr_problem_build_hip_shard": (C.c_int, [vp, C.c_int, i64, C.c_int, C.c_int, C.c_int, pp]),
        "lfr_problem_cc_sharded": (C.c_int, [vp]),
        "lfr_problem_free": (None, [vp]),
        "lfr_bisect_graph": (i64, [i64, vp, vp, vp, vp, vp]),
        "lfr_debug_recursive_cut": (i64, [i64, vp, vp, vp, i64, vp, i64, vp, vp]),
        "lfr_problem_get_stats": (C.c_int, [vp, C.POINTER(ProblemStats)]),
        "lfr_problem_get_labels": (C.c_int, [vp, vp, vp, vp]),
        "lfr_problem_shard_components": (i64, [vp, C.c_int, C.c_int, vp, vp]),
        "lfr_hip_warmup": (C.c_int, [C.c_int]),
        "lfr_hip_reserve": (C.c_int, [C.c_int, i64, i64]),
        "lfr_hip_trim": (C.c_int, [C.c_int]),
        "lfr_hip_synchronize": (C.c_int, [C.c_int]),
        "lfr_batch_create": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, pp]),
        "lfr_batch_free": (None, [vp]),
        "lfr_batch_solve": (C.c_int, [vp, vp, C.POINTER(SolveStats)]),
        "lfr_batch_solve_from": (C.c_int, [vp, vp, vp, C.POINTER(SolveStats)]),
        "lfr_batch_download": (C.c_int, [vp, vp]),
        "lfr_batch_positions_view": (C.c_int, [vp, pp]),
        "lfr_batch_positions_view_f32": (C.c_int, [vp, pp]),
        "lfr_batch_timing": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), vp, vp]),
        "lfr_batch_component_info": (i64, [vp, vp, vp, vp, vp, vp, vp]),
        "lfr_batch_positions_to_device": (C.c_int, [vp, vp, vp]),
        "lfr_batch_backward": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp, C.POINTER(BackwardStats)]),
        "lfr_batch_backward_status": (i64, [vp, vp]),
        "lfr_batch_jvp": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp, C.POINTER(JvpStats)]),
        "lfr_batch_jvp_status": (i64, [vp, vp]),
        "lfr_batch_set_inputs": (C.c_int, [vp, vp, vp, vp, vp]),
        "lfr_batch_covariance": (C.c_int, [vp, vp, C.c_int, vp, C.POINTER(CovarianceStats)]),
        "lfr_batch_covariance_matches": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, C.POINTER(CovarianceStats)]),
        "lfr_batch_covariance_status": (i64, [vp, vp]),
        "lfr_batch_evaluate": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, vp, C.POINTER(EvaluateStats)]),
        "lfr_batch_evaluate_vjp": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, C.POINTER(EvaluateVjpStats)]),
        "lfr_batch_hessian_product": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, C.POINTER(HessianProductStats)]),
        "lfr_batch_hessian_solve": (C.c_int, [vp, vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, vp, vp, vp, vp, C.c_int, vp,
                                              C.POINTER(HessianSolveStats)]),
        "lfr_keypoint_covariances": (C.c_int, [vp, vp, C.c_char_p, vp, i64]),
        "lfr_debug_invert_spd": (C.c_int, [C.c_int, C.c_int, i64, vp, vp, vp, vp]),
        "lfr_batch_spin_timeouts": (i64, [vp]),
        "lfr_batch_team_runs": (i64, [vp]),
        "lfr_batch_team_fallbacks": (i64, [vp]),
        "lfr_debug_occupy": (C.c_int, [C.c_int, C.c_int, C.c_double]),
        "lfr_batch_tree_stats": (i64, [vp, vp, vp, vp, vp, vp]),
        "lfr_debug_eval_edges": (C.c_int, [C.c_int, i64, vp, vp, vp, vp, vp, C.c_int, vp, vp]),
        "lfr_debug_ls_next_step": (C.c_int, [C.c_int, i64, vp, vp, C.c_int, vp]),
        "lfr_debug_solve_damped": (C.c_int, [C.c_int, C.c_int, i64, vp, vp, vp, vp, vp, vp]),
        "lfr_debug_tree_plan": (i64, [i32, i64, vp, vp, i64, vp]),
        "lfr_debug_solve_tree": (C.c_int, [C.c_int, i64, vp, vp, vp, vp, vp, vp, vp]),
        "lfr_debug_pool_selftest": (i64, [C.c_int, i64, C.c_int]),
        "lfr_debug_sort_pairs": (C.c_int, [C.c_int, i64, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
        "lfr_debug_exclusive_sum": (C.c_int, [C.c_int, i64, C.c_int, vp, vp]),
        "lfr_solve_hip": (C.c_int, [vp, C.c_int, C.c_int, vp, C.POINTER(SolveStats)]),
        "lfr_solve_hip_multi": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.POINTER(SolveStats)]),
        "lfr_solve_graph_hip_multi": (C.c_int, [vp, vp, C.c_int, i64, C.c_int, vp, C.POINTER(ProblemStats), C.POINTER(SolveStats)]),
        "lfr_write_solution": (C.c_int, [vp, vp, C.c_char_p, C.POINTER(i64)]),
        "lfr_apply_displacements": (C.c_int, [vp, vp, C.c_char_p, vp, i64, i64]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)       # AttributeError here = the .so does not export the ABI
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


EXPORTS = ["lfr_version", "lfr_last_error", "lfr_graph_from_files", "lfr_graph_from_matches_file", "lfr_graph_from_matches_file_device",
           "lfr_graph_from_arrays", "lfr_graph_from_arrays_device_flows", "lfr_graph_from_device_arrays", "lfr_debug_graph_build_spans", "lfr_graph_to_device", "lfr_graph_evict_device",
           "lfr_problem_build_hip_ex", "lfr_problem_build_hip_shard", "lfr_problem_cc_sharded", "lfr_hip_reserve", "lfr_hip_trim", "lfr_batch_positions_view", "lfr_batch_positions_view_f32", "lfr_bisect_graph", "lfr_debug_eval_edges", "lfr_debug_ls_next_step", "lfr_debug_solve_damped", "lfr_debug_tree_plan", "lfr_debug_solve_tree", "lfr_debug_pool_selftest", "lfr_debug_sort_pairs", "lfr_debug_exclusive_sum", "lfr_debug_recursive_cut", "lfr_hip_synchronize", "lfr_graph_free", "lfr_graph_num_nodes", "lfr_graph_num_edges",
           "lfr_graph_num_images", "lfr_graph_get_nodes", "lfr_graph_image_name", "lfr_graph_image_fact",
           "lfr_write_matching_file", "lfr_problem_build", "lfr_problem_build_labels", "lfr_problem_build_hip", "lfr_problem_free", "lfr_problem_get_stats",
           "lfr_problem_get_labels", "lfr_problem_shard_components", "lfr_hip_warmup", "lfr_batch_create", "lfr_batch_free", "lfr_batch_solve", "lfr_batch_solve_from",
           "lfr_batch_download", "lfr_batch_timing", "lfr_batch_spin_timeouts", "lfr_batch_team_runs", "lfr_batch_team_fallbacks", "lfr_debug_occupy", "lfr_batch_tree_stats", "lfr_batch_component_info", "lfr_batch_positions_to_device", "lfr_batch_backward", "lfr_batch_backward_status", "lfr_batch_jvp", "lfr_batch_jvp_status", "lfr_batch_set_inputs", "lfr_batch_covariance", "lfr_batch_covariance_matches", "lfr_batch_covariance_status", "lfr_batch_evaluate", "lfr_batch_evaluate_vjp", "lfr_batch_hessian_product", "lfr_batch_hessian_solve", "lfr_keypoint_covariances", "lfr_debug_invert_spd", "lfr_solve_hip", "lfr_solve_hip_multi", "lfr_solve_graph_hip_multi", "lfr_write_solution", "lfr_apply_displacements"]


def _check(rc):
    if rc != 0:
        raise LfrError(rc, lib().lfr_last_error().decode("utf-8", "replace"))


def _f64_device_tensor(caller, t, name, shapes, dev):
    """Argument check of Batch.hessian_product / Batch.hessian_solve: t is a contiguous float64 torch tensor on `dev` with one of
    `shapes` (None = any extent, printed as K); returns its address for the C call.  ValueError otherwise, in the caller's name."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: %s must be a torch tensor" % (caller, name))
    if not t.is_cuda or t.device != dev:
        raise ValueError("%s: %s is on %s, the batch on %s" % (caller, name, t.device, dev))
    if t.dtype != torch.float64:
        raise ValueError("%s: %s is %s, need torch.float64" % (caller, name, t.dtype))
    if not t.is_contiguous() or not any(t.dim() == len(s) and all(w is None or w == h for w, h in zip(s, t.shape)) for s in shapes):
        raise ValueError("%s: %s has shape %s, need a contiguous %s"
                         % (caller, name, tuple(t.shape), " or ".join("[%s]" % ", ".join("K" if w is None else str(w) for w in s) for s in shapes)))
    return C.c_void_p(t.detach().data_ptr() or 1)      # (no nodes: an empty tensor has no address, and nothing is read)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cstrs(strings):
    arr = (C.c_char_p * max(len(strings), 1))()
    for i, s in enumerate(strings):
        arr[i] = s.encode("utf-8") if isinstance(s, str) else s
    return arr


def hip_warmup_async(device=0, n_nodes=0, n_matches=0):
    """Start creating the HIP context on a side thread (ctypes releases the GIL); returns the thread.
    n_nodes / n_matches > 0 also pre-populates the slab caches for a graph of (about) that size."""
    import threading
    L = lib()

    def work():
        L.lfr_hip_warmup(device)
        if n_matches > 0:
            L.lfr_hip_reserve(device, n_nodes, n_matches)
    t = threading.Thread(target=work, daemon=True)
    t.start()
    return t


FLOWS_STAY_ON_HOST = 1      # LFR_BUILD_FLOWS_STAY_ON_HOST


class Graph:
    """Parsed match graph (solve.cc:405-481)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_matches_file(cls, path, banned=(), device=None):
        """device: ingest straight to that GPU (lfr_graph_from_matches_file_device: the flows' upload overlaps the node numbering)."""
        h = C.c_void_p()
        if device is None:
            _check(lib().lfr_graph_from_matches_file(os.fsencode(path), _cstrs(list(banned)), len(banned), C.byref(h)))
        else:
            _check(lib().lfr_graph_from_matches_file_device(os.fsencode(path), _cstrs(list(banned)), len(banned), int(device), C.byref(h)))
        return cls(h)

    @classmethod
    def from_files(cls, paths, banned=()):
        h = C.c_void_p()
        _check(lib().lfr_graph_from_files(_cstrs([os.fsencode(p) for p in paths]), len(paths),
                                          _cstrs(list(banned)), len(banned), C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, ma, banned=()):
        """ma: :class:`lfr_amd.synthetic.MatchArrays`."""
        h = C.c_void_p()
        a = _contig(ma)
        _check(lib().lfr_graph_from_arrays(len(ma.image_names), _cstrs(ma.image_names), _ptr(a["facts"]),
                                           len(a["p1"]), _ptr(a["p1"]), _ptr(a["p2"]), _ptr(a["off"]),
                                           _ptr(a["f1"]), _ptr(a["f2"]), _ptr(a["sim"]), _ptr(a["d1"]),
                                           _ptr(a["d2"]), _cstrs(list(banned)), len(banned), C.byref(h)))
        return cls(h)

    @classmethod
    def from_device_flows(cls, ma, disp1_ptr, disp2_ptr, device=0, banned=()):
        """ma: MatchArrays (its disp1/disp2 are ignored); disp*_ptr: device addresses (int) of float32
        [n_matches, 18] arrays on HIP device `device`, e.g. tensor.data_ptr().  The caller keeps them alive
        until the Batch exists."""
        h = C.c_void_p()
        a = _contig(ma, flows=False)
        _check(lib().lfr_graph_from_arrays_device_flows(
            len(ma.image_names), _cstrs(ma.image_names), _ptr(a["facts"]), len(a["p1"]), _ptr(a["p1"]), _ptr(a["p2"]),
            _ptr(a["off"]), _ptr(a["f1"]), _ptr(a["f2"]), _ptr(a["sim"]), C.c_void_p(disp1_ptr), C.c_void_p(disp2_ptr),
            device, _cstrs(list(banned)), len(banned), C.byref(h)))
        return cls(h)

    @classmethod
    def from_device_arrays(cls, ma, feat1_ptr, feat2_ptr, sim_ptr, disp1_ptr, disp2_ptr, device=0, banned=()):
        """lfr_graph_from_device_arrays: the nodes are numbered on the GPU.  ma: MatchArrays of which only the host-side fields are
        read (image_names, facts, pair_img1, pair_img2, pair_off); feat*_ptr / sim_ptr / disp*_ptr: device addresses (int, e.g.
        tensor.data_ptr(); 0 = NULL) of uint32 [n_matches], float32 [n_matches] and float32 [n_matches, 18] arrays on HIP device
        `device`, complete when the call is made.  The caller keeps the flows alive until the Batch exists; the other three are read
        inside the call only.  The graph is resident on `device` afterwards."""
        h = C.c_void_p()
        facts = np.ascontiguousarray(ma.facts, np.float32)
        p1, p2 = np.ascontiguousarray(ma.pair_img1, np.int32), np.ascontiguousarray(ma.pair_img2, np.int32)
        off = np.ascontiguousarray(ma.pair_off, np.int64)
        if len(off) != len(p1) + 1 or len(p2) != len(p1):
            raise ValueError("from_device_arrays: pair_off needs one entry more than pair_img1 / pair_img2")
        _check(lib().lfr_graph_from_device_arrays(
            len(ma.image_names), _cstrs(ma.image_names), _ptr(facts), len(p1), _ptr(p1), _ptr(p2), _ptr(off),
            C.c_void_p(feat1_ptr), C.c_void_p(feat2_ptr), C.c_void_p(sim_ptr), C.c_void_p(disp1_ptr), C.c_void_p(disp2_ptr),
            int(device), _cstrs(list(banned)), len(banned), C.byref(h)))
        return cls(h)

    @staticmethod
    def build_spans():
        """Spans (ms) of this thread's latest from_device_arrays (lfr_debug_graph_build_spans); the four device spans are 0 unless
        LFR_GRAPHBUILD_SPANS=1 was set when the library first built such a graph."""
        ms = np.zeros(7, np.float64)
        _check(lib().lfr_debug_graph_build_spans(_ptr(ms), 7))
        return dict(zip(("expand", "sort", "scans", "scatter", "host_mirror", "finish", "host_pair_table"), ms.tolist()))

    def close(self):
        if self._h:
            lib().lfr_graph_free(self._h)
            self._h = None

    __del__ = close

    def to_device(self, device=0):
        """Start the asynchronous upload of the graph (endpoints, similarities, flows) to HBM."""
        _check(lib().lfr_graph_to_device(self._h, device))

    def evict_device(self):
        """Drop the graph's cached copy in HBM (the next device pipeline run uploads it again)."""
        _check(lib().lfr_graph_evict_device(self._h))

    @property
    def n_nodes(self):
        return lib().lfr_graph_num_nodes(self._h)

    @property
    def n_edges(self):
        return lib().lfr_graph_num_edges(self._h)

    @property
    def n_images(self):
        return lib().lfr_graph_num_images(self._h)

    def nodes(self):
        n = self.n_nodes
        img = np.zeros(n, np.int32)
        feat = np.zeros(n, np.uint32)
        _check(lib().lfr_graph_get_nodes(self._h, _ptr(img), _ptr(feat)))
        return img, feat

    def image_names(self):
        return [lib().lfr_graph_image_name(self._h, i).decode("utf-8") for i in range(self.n_images)]

    def image_facts(self):
        return [lib().lfr_graph_image_fact(self._h, i) for i in range(self.n_images)]

    def apply_displacements(self, positions, image_name, keypoints):
        """In-place consumer arithmetic of colmap_utils.py:126-137 on a float32 [num_features, >=2] array."""
        assert keypoints.dtype == np.float32 and keypoints.ndim == 2 and keypoints.flags.c_contiguous
        pos = np.ascontiguousarray(positions, np.float64)
        _check(lib().lfr_apply_displacements(self._h, _ptr(pos), image_name.encode("utf-8"), _ptr(keypoints),
                                             keypoints.shape[0], keypoints.shape[1]))
        return keypoints

    def keypoint_covariances(self, cov, image_name, num_features):
        """Per feature of `image_name` the 2x2 covariance in pixels and keypoint (x, y) order (lfr_keypoint_covariances): a float32
        [num_features, 3] array of (xx, xy, yy) from the [n_nodes, 3] covariance of Batch.covariance (on the host); 0 where the graph
        has no node, for roots and for unsolved nodes."""
        c = np.ascontiguousarray(cov, np.float64)
        if c.size != 3 * self.n_nodes:
            raise ValueError("keypoint_covariances: need a [%d, 3] array" % self.n_nodes)
        out = np.zeros((int(num_features), 3), np.float32)
        _check(lib().lfr_keypoint_covariances(self._h, _ptr(c), image_name.encode("utf-8"), _ptr(out), int(num_features)))
        return out

    def write_solution(self, positions, path):
        """SolutionFile emit (solve.cc:644-679); returns the '> 0.5' count of solve.cc:666-670."""
        pos = np.ascontiguousarray(positions, np.float64)
        n_out = C.c_int64(0)
        _check(lib().lfr_write_solution(self._h, _ptr(pos), os.fsencode(path), C.byref(n_out)))
        return n_out.value


def _contig(ma, flows=True):
    M = ma.n_matches
    if not flows:
        return {"facts": np.ascontiguousarray(ma.facts, np.float32),
                "p1": np.ascontiguousarray(ma.pair_img1, np.int32), "p2": np.ascontiguousarray(ma.pair_img2, np.int32),
                "off": np.ascontiguousarray(ma.pair_off, np.int64),
                "f1": np.ascontiguousarray(ma.feat1, np.uint32), "f2": np.ascontiguousarray(ma.feat2, np.uint32),
                "sim": np.ascontiguousarray(ma.sim, np.float32)}
    return {"facts": np.ascontiguousarray(ma.facts, np.float32),
            "p1": np.ascontiguousarray(ma.pair_img1, np.int32), "p2": np.ascontiguousarray(ma.pair_img2, np.int32),
            "off": np.ascontiguousarray(ma.pair_off, np.int64),
            "f1": np.ascontiguousarray(ma.feat1, np.uint32), "f2": np.ascontiguousarray(ma.feat2, np.uint32),
            "sim": np.ascontiguousarray(ma.sim, np.float32),
            "d1": np.ascontiguousarray(ma.disp1, np.float32).reshape(M, 18),
            "d2": np.ascontiguousarray(ma.disp2, np.float32).reshape(M, 18)}


def eval_edges_hip(flows, sim, kind, x1, x2, tukey_variant="ceres1", device=0):
    """The kernels' per-edge arithmetic on the GPU (lfr_debug_eval_edges): returns (out[n, 8], cost_only[n])."""
    flows = np.ascontiguousarray(flows, np.float32).reshape(-1, 18)
    n = flows.shape[0]
    sim = np.ascontiguousarray(sim, np.float32)
    kind = np.ascontiguousarray(kind, np.int32)
    x1 = np.ascontiguousarray(x1, np.float64).reshape(n, 2)
    x2 = np.ascontiguousarray(x2, np.float64).reshape(n, 2)
    out = np.zeros((n, 8), np.float64)
    cost = np.zeros(n, np.float64)
    _check(lib().lfr_debug_eval_edges(device, n, _ptr(flows), _ptr(sim), _ptr(kind), _ptr(x1), _ptr(x2), TUKEY[tukey_variant],
                                      _ptr(out), _ptr(cost)))
    return out, cost


def ls_next_step_hip(samples, dir_max, register_version=False, device=0):
    """The kernels' line-search contraction on the GPU (lfr_debug_ls_next_step): samples[n, 3, 5] = (x, value, gradient,
    value_valid, gradient_valid) of the initial / previous / current sample.  Returns the next step sizes (negative: give up)."""
    samples = np.ascontiguousarray(samples, np.float64).reshape(-1, 15)
    n = samples.shape[0]
    dir_max = np.ascontiguousarray(dir_max, np.float64)
    a = np.zeros(n, np.float64)
    _check(lib().lfr_debug_ls_next_step(device, n, _ptr(samples), _ptr(dir_max), int(register_version), _ptr(a)))
    return a


SOLVERS = {"g8": 0, "g16": 1, "g64_2": 2, "g64_4": 3, "block_s": 4, "block_m": 5, "block_l": 6}
SOLVER_MAX_ROWS = {"g8": 8, "g16": 16, "g64_2": 24, "g64_4": 32, "block_s": 88, "block_m": 130, "block_l": 192}


def solve_damped_hip(solver, n_rows, A, damp, g, device=0):
    """The kernels' LM step solve (A + D) y = g on the GPU (lfr_debug_solve_damped).  solver: a key of SOLVERS; n_rows[s] per system;
    A, damp, g: the systems' packed lower triangles and vectors concatenated (see lfr.h).  Returns (y, status): the LM step is -y;
    status bit 0 = not positive definite (y NaN), bit 1 = a spin-wait of the factorization ran out."""
    n_rows = np.ascontiguousarray(n_rows, np.int32)
    A = np.ascontiguousarray(A, np.float64)
    damp = np.ascontiguousarray(damp, np.float64)
    g = np.ascontiguousarray(g, np.float64)
    n_vec = int(n_rows.astype(np.int64).sum())
    if A.size != int((n_rows.astype(np.int64) * (n_rows + 1) // 2).sum()) or damp.size != n_vec or g.size != n_vec:
        raise ValueError("A, damp, g do not match n_rows")
    y = np.zeros(n_vec, np.float64)
    status = np.zeros(n_rows.size, np.int32)
    _check(lib().lfr_debug_solve_damped(device, SOLVERS[solver], n_rows.size, _ptr(n_rows), _ptr(A), _ptr(damp), _ptr(g), _ptr(y), _ptr(status)))
    return y, status


def solve_tree_hip(blobs, tiles, damp, g, device=0):
    """The elimination-tree kernel's LM step solve (A + D) y = g on the GPU (lfr_debug_solve_tree), one workgroup per system, all in
    one launch.  Per system: blobs[s] the plan (tree_plan), tiles[s] A in the plan's tile layout [n_tiles, 16, 16], damp[s], g[s] of
    n_pad doubles in matrix order (see lfr.h).  Returns (list of y, status): status bit 0 = a pivot was not positive (y NaN), bit 1 =
    a spin-wait ran out."""
    blobs = [np.ascontiguousarray(b, np.uint32) for b in blobs]
    words = np.array([b.size for b in blobs], np.int64)
    n_pad = [16 * int(b[0]) for b in blobs]
    for b, t, d, gg, n in zip(blobs, tiles, damp, g, n_pad):
        if np.size(t) != 256 * int(b[1]) or np.size(d) != n or np.size(gg) != n:
            raise ValueError("tiles, damp, g do not match the plan")
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate([np.zeros(0, dt)] + [np.asarray(x, dt).reshape(-1) for x in xs]))
    B, T, D, G = cat(blobs, np.uint32), cat(tiles, np.float64), cat(damp, np.float64), cat(g, np.float64)
    y = np.zeros(D.size, np.float64)
    status = np.zeros(len(blobs), np.int32)
    _check(lib().lfr_debug_solve_tree(device, len(blobs), _ptr(words), _ptr(B), _ptr(T), _ptr(D), _ptr(G), _ptr(y), _ptr(status)))
    o = np.r_[0, np.cumsum(n_pad)]
    return [y[o[i]:o[i + 1]] for i in range(len(blobs))], status


def invert_spd_hip(solver, n_rows, A, device=0):
    """The packed classes' in-register inversion on the GPU (lfr_debug_invert_spd).  solver: "g8", "g16", "g64_2" or "g64_4";
    n_rows[s] per system; A: the packed lower triangles concatenated (see lfr.h).  Returns (Cinv, status): the inverses' lower
    triangles in the same layout, status 0 or COVARIANCE_SINGULAR (a pivot was not positive; that system's Cinv is zero)."""
    n_rows = np.ascontiguousarray(n_rows, np.int32)
    A = np.ascontiguousarray(A, np.float64)
    if SOLVERS[solver] > 3:
        raise ValueError("invert_spd_hip: a packed solver")
    if A.size != int((n_rows.astype(np.int64) * (n_rows + 1) // 2).sum()):
        raise ValueError("A does not match n_rows")
    Cinv = np.zeros(A.size, np.float64)
    status = np.zeros(n_rows.size, np.int32)
    _check(lib().lfr_debug_invert_spd(device, SOLVERS[solver], n_rows.size, _ptr(n_rows), _ptr(A), _ptr(Cinv), _ptr(status)))
    return Cinv, status


def sort_pairs_hip(keys, vals, begin_bit, end_bit, use_library=False, device=0):
    """The pipeline's stable device sort (lfr_debug_sort_pairs): uint32 / uint64 keys, uint32 values -> (sorted keys, values)."""
    keys = np.ascontiguousarray(keys)
    assert keys.dtype in (np.uint32, np.uint64)
    vals = np.ascontiguousarray(vals, np.uint32)
    ko, vo = np.empty_like(keys), np.empty_like(vals)
    _check(lib().lfr_debug_sort_pairs(device, keys.size, keys.dtype.itemsize, _ptr(keys), _ptr(vals), int(begin_bit), int(end_bit),
                                      int(bool(use_library)), _ptr(ko), _ptr(vo)))
    return ko, vo


def exclusive_sum_hip(values, device=0):
    """The pipeline's one-launch exclusive prefix sum (lfr_debug_exclusive_sum) of a uint32 / uint64 array."""
    values = np.ascontiguousarray(values)
    assert values.dtype in (np.uint32, np.uint64)
    out = np.empty_like(values)
    _check(lib().lfr_debug_exclusive_sum(device, values.size, values.dtype.itemsize, _ptr(values), _ptr(out)))
    return out


def occupy_hip(workgroups, milliseconds, device=0):
    """Keeps `workgroups` CUs busy for `milliseconds` on a stream of their own (lfr_debug_occupy); returns when they have started."""
    _check(lib().lfr_debug_occupy(device, int(workgroups), float(milliseconds)))


def bisect_graph(edges, weights):
    """The library's substitute for colmap::ComputeNormalizedMinGraphCut(edges, weights, 2) (solve.cc:192):
    {node id: side}."""
    e = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
    a, b = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
    w = np.ascontiguousarray(weights, np.int32)
    nodes = np.zeros(2 * len(w) + 1, np.int32)
    part = np.zeros(2 * len(w) + 1, np.int32)
    n = lib().lfr_bisect_graph(len(w), _ptr(a), _ptr(b), _ptr(w), _ptr(nodes), _ptr(part))
    if n < 0:
        _check(int(n))
    return {int(nodes[i]): int(part[i]) for i in range(n)}


def recursive_cut(edges, weights, node_weights, max_weight):
    """The product's size-cap recursion (lfr_debug_recursive_cut): (nodes ascending, subset of each)."""
    e = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
    a, b = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
    w = np.ascontiguousarray(weights, np.int32)
    nw = np.ascontiguousarray(node_weights, np.int64)
    nodes = np.zeros(2 * len(w) + 1, np.int32)
    sub = np.zeros(2 * len(w) + 1, np.int32)
    n = lib().lfr_debug_recursive_cut(len(w), _ptr(a), _ptr(b), _ptr(w), len(nw), _ptr(nw), int(max_weight), _ptr(nodes), _ptr(sub))
    if n < 0:
        _check(int(n))
    return nodes[:n].copy(), sub[:n].copy()


def write_matching_file(path, ma):
    """Native MatchingFile writer (compute_match_graph.py:163-205 equivalent)."""
    a = _contig(ma)
    _check(lib().lfr_write_matching_file(os.fsencode(path), len(ma.image_names), _cstrs(ma.image_names),
                                         _ptr(a["facts"]), len(a["p1"]), _ptr(a["p1"]), _ptr(a["p2"]),
                                         _ptr(a["off"]), _ptr(a["f1"]), _ptr(a["f2"]), _ptr(a["sim"]),
                                         _ptr(a["d1"]), _ptr(a["d2"])))


class Problem:
    """Tracks, roots, components and the device batch layout (solve.cc:487-606, 79-143)."""

    def __init__(self, graph, max_nodes_in_component=0, component_override=None, device_assembly=False,
                 device_graph_stage=None, flags=0, shard=None):
        """device_assembly=True: graph stage only; the batch is assembled on the GPU by Batch / solve_hip.
        device_graph_stage=<device ordinal>: tracks/roots/components on that GPU too (implies device_assembly);
        flags=FLOWS_STAY_ON_HOST: do not stage the flows in HBM (sharded batches gather their rows zero-copy);
        shard=(rank, world): the graph stage over the connected components of the match graph dealt to `rank` only."""
        self.graph = graph
        h = C.c_void_p()
        co = None if component_override is None else np.ascontiguousarray(component_override, np.int64)
        self.cc_sharded = False
        if shard is not None and device_graph_stage is None:
            raise ValueError("Problem(shard=...) needs device_graph_stage: the host graph stage is not sharded (deal the components with Batch(p, dev, rank, world))")
        if shard is not None and component_override is not None:
            raise ValueError("Problem(shard=...) cannot be combined with component_override (lfr_problem_build_hip_shard has no override)")
        if device_graph_stage is not None and shard is not None and shard[1] > 1:
            # multi-GPU: this rank's connected components only (lfr_problem_build_hip_shard); cc_sharded False = the whole graph after all
            _check(lib().lfr_problem_build_hip_shard(graph._h, int(device_graph_stage), int(max_nodes_in_component), int(flags),
                                                     int(shard[0]), int(shard[1]), C.byref(h)))
            self.cc_sharded = bool(lib().lfr_problem_cc_sharded(h))
        elif device_graph_stage is not None:
            _check(lib().lfr_problem_build_hip_ex(graph._h, int(device_graph_stage), int(max_nodes_in_component), _ptr(co),
                                                  int(flags), C.byref(h)))
        else:
            fn = lib().lfr_problem_build_labels if device_assembly else lib().lfr_problem_build
            _check(fn(graph._h, int(max_nodes_in_component), _ptr(co), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().lfr_problem_free(self._h)
            self._h = None

    __del__ = close

    def stats(self):
        s = ProblemStats()
        _check(lib().lfr_problem_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    def labels(self):
        n = self.graph.n_nodes
        track = np.zeros(n, np.int64)
        root = np.zeros(n, np.uint8)
        comp = np.zeros(n, np.int64)
        _check(lib().lfr_problem_get_labels(self._h, _ptr(track), _ptr(root), _ptr(comp)))
        return track, root.astype(bool), comp

    def shard_components(self, rank, world):
        """(component ids, edge counts) of the solvable components dealt to shard rank/world."""
        n = lib().lfr_problem_shard_components(self._h, rank, world, None, None)
        if n < 0:
            _check(int(n))
        comps = np.zeros(n, np.int64)
        edges = np.zeros(n, np.int64)
        lib().lfr_problem_shard_components(self._h, rank, world, _ptr(comps), _ptr(edges))
        return comps, edges

    def solve_hip(self, device=0, tukey_variant="ceres1", want_stats=True):
        """Upload + solve + download on one GPU.  Returns (positions[n,2], stats dict or None).  want_stats=False skips the statistics
        (they fetch every descriptor and per-component record to the host: 15-20 ms for 147 k components, several times the solve)."""
        n = self.graph.n_nodes
        pos = np.empty((n, 2), np.float64)                  # (fully written by the download: every node, zeros where nothing was solved)
        st = SolveStats()
        _check(lib().lfr_solve_hip(self._h, device, TUKEY[tukey_variant], _ptr(pos), C.byref(st) if want_stats else None))
        return pos, (st.as_dict() if want_stats else None)


def solve_graph_hip_multi(graph, devices, max_nodes_in_component=0, tukey_variant="ceres1"):
    """Graph stage, assembly and solve sharded over several GPUs from this process (lfr_solve_graph_hip_multi): device k takes the
    connected components of the match graph dealt to shard k.  Returns (positions[n, 2], problem stats, solve stats)."""
    n = graph.n_nodes
    pos = np.zeros((n, 2), np.float64)
    pst, st = ProblemStats(), SolveStats()
    dev = np.ascontiguousarray(devices, np.int32)
    _check(lib().lfr_solve_graph_hip_multi(graph._h, _ptr(dev), len(dev), int(max_nodes_in_component), TUKEY[tukey_variant], _ptr(pos),
                                          C.byref(pst), C.byref(st)))
    return pos, pst.as_dict(), st.as_dict()


def solve_hip_multi(problem, devices, tukey_variant="ceres1"):
    """Shard a host-assembled problem over several GPUs from this process (one host thread per device)."""
    n = problem.graph.n_nodes
    pos = np.zeros((n, 2), np.float64)
    st = SolveStats()
    dev = np.ascontiguousarray(devices, np.int32)
    _check(lib().lfr_solve_hip_multi(problem._h, _ptr(dev), len(dev), TUKEY[tukey_variant], _ptr(pos), C.byref(st)))
    return pos, st.as_dict()


class Batch:
    """A problem (or one LPT shard of it) resident in HBM."""

    def __init__(self, problem, device=0, shard_rank=0, shard_world=1, tukey_variant="ceres1"):
        self.problem = problem
        h = C.c_void_p()
        _check(lib().lfr_batch_create(problem._h, device, shard_rank, shard_world, TUKEY[tukey_variant], C.byref(h)))
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib().lfr_batch_free(self._h)
            self._h = None

    __del__ = close

    def solve(self, stream=None, want_stats=True):
        """stream: a hipStream_t as int (e.g. torch.cuda.current_stream().cuda_stream) or None."""
        st = SolveStats()
        _check(lib().lfr_batch_solve(self._h, C.c_void_p(stream) if stream else None,
                                     C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def solve_from(self, initial=None, stream=None, want_stats=True):
        """The solve started at given positions (lfr_batch_solve_from, include/lfr.h): `initial` is a contiguous [n_nodes, 2] float64
        tensor on the batch's device, read by work enqueued in this call only, or None = the batch's own positions, in place (the
        latest solve's result; zeros before the first).  Every coordinate is clamped to [-1, 1], a NaN reads as 0; from there on the
        loop is solve()'s.  stream: a hipStream_t as int, or None = the default stream as for solve()."""
        ptr = None
        if initial is not None:
            import torch
            n = self.problem.graph.n_nodes
            if (not isinstance(initial, torch.Tensor) or not initial.is_cuda or initial.device != torch.device("cuda", self.device)
                    or initial.dtype != torch.float64 or not initial.is_contiguous() or tuple(initial.shape) != (n, 2)):
                raise ValueError("solve_from: need a contiguous [%d, 2] float64 tensor on cuda:%d" % (n, self.device))
            ptr = C.c_void_p(initial.data_ptr() or 1)       # (no nodes: an empty tensor has no address, and nothing is read)
        st = SolveStats()
        _check(lib().lfr_batch_solve_from(self._h, ptr, C.c_void_p(stream) if stream else None,
                                          C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def timing(self, solves_back=0):
        """HIP-event times of one of the last 64 solves: (total_ms, per-kernel-class ms, per-class edges)."""
        tot = C.c_double(0.0)
        cls = np.zeros(NUM_KERNEL_CLASSES, np.float64)
        edges = np.zeros(NUM_KERNEL_CLASSES, np.int64)
        _check(lib().lfr_batch_timing(self._h, solves_back, C.byref(tot), _ptr(cls), _ptr(edges)))
        return tot.value, cls, edges

    def download(self, positions=None):
        n = self.problem.graph.n_nodes
        if positions is None:
            positions = np.zeros((n, 2), np.float64)
        _check(lib().lfr_batch_download(self._h, _ptr(positions)))
        return positions

    def positions_view(self):
        """Zero-copy [n, 2] float64 view of the batch's pinned staging buffer (valid until the next solve /
        download / close of this batch; nodes outside the shard read 0)."""
        n = self.problem.graph.n_nodes
        p = C.c_void_p()
        _check(lib().lfr_batch_positions_view(self._h, C.byref(p)))
        if n == 0:
            return np.zeros((0, 2), np.float64)
        buf = (C.c_double * (2 * n)).from_address(p.value)
        return np.frombuffer(buf, dtype=np.float64).reshape(n, 2)

    def positions_view_f32(self):
        """The same as [n, 2] float32 - the precision of the reference's SolutionFile (solve.cc:661-664) - converted on the device:
        half the bytes over PCIe."""
        n = self.problem.graph.n_nodes
        p = C.c_void_p()
        _check(lib().lfr_batch_positions_view_f32(self._h, C.byref(p)))
        if n == 0:
            return np.zeros((0, 2), np.float32)
        buf = (C.c_float * (2 * n)).from_address(p.value)
        return np.frombuffer(buf, dtype=np.float32).reshape(n, 2)

    def positions_to(self, tensor, stream=None):
        """Stream-ordered device copy of the latest solve's positions into `tensor` ([n_nodes, 2] float64, contiguous, on the batch's
        device); stream: a hipStream_t as int, None = torch's current stream.  Returns `tensor`."""
        import torch
        n = self.problem.graph.n_nodes
        if tensor.dtype != torch.float64 or not tensor.is_cuda or not tensor.is_contiguous() or tensor.numel() != 2 * n:
            raise ValueError("positions_to: need a contiguous [%d, 2] float64 device tensor" % n)
        if stream is None:
            stream = torch.cuda.current_stream(tensor.device).cuda_stream
        if n:
            _check(lib().lfr_batch_positions_to_device(self._h, C.c_void_p(tensor.data_ptr()), C.c_void_p(stream) if stream else None))
        return tensor

    def set_inputs(self, disp1=None, disp2=None, sim=None, stream=None):
        """New flows and / or similarities into the live batch (lfr_batch_set_inputs, include/lfr.h): contiguous float32 tensors on
        the batch's device in the graph's match layout - disp1, disp2: [n_matches, 18] or [n_matches, 9, 2], given together or not
        at all (None = keep); sim: [n_matches] (None = keep).  The structure of the batch stays that of its creation.  Stream-ordered
        on `stream` (a hipStream_t as int, None = torch's current stream) without a host synchronisation: the tensors may be
        overwritten or freed in stream order afterwards.  The next solve() uses the new values."""
        import torch
        m = self.problem.graph.n_edges // 2
        dev = torch.device("cuda", self.device)

        def ptr(t, name, shapes):
            if t is None:
                return None
            if not isinstance(t, torch.Tensor):
                raise ValueError("set_inputs: %s must be a torch tensor" % name)
            if not t.is_cuda or t.device != dev:
                raise ValueError("set_inputs: %s is on %s, the batch on %s" % (name, t.device, dev))
            if t.dtype != torch.float32:
                raise ValueError("set_inputs: %s is %s, need float32" % (name, t.dtype))
            if tuple(t.shape) not in shapes or not t.is_contiguous():
                raise ValueError("set_inputs: %s has shape %s, need a contiguous %s" % (name, tuple(t.shape), " or ".join(map(str, shapes))))
            return C.c_void_p(t.data_ptr() or 1)          # (no matches: an empty tensor has no address, and nothing is read)

        flow_shapes = ((m, 18), (m, 9, 2))
        p1, p2, ps = ptr(disp1, "disp1", flow_shapes), ptr(disp2, "disp2", flow_shapes), ptr(sim, "sim", ((m,),))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().lfr_batch_set_inputs(self._h, p1, p2, ps, C.c_void_p(stream) if stream else None))

    def backward(self, grad_positions, f64=False, stream=None, want_stats=False, gauss_newton=False, gn_fallback=False):
        """Implicit gradient of the latest solve (lfr_batch_backward, include/lfr.h): grad_positions = dL/dx, [n_nodes, 2] float64 on
        the batch's device.  Returns (grad_disp1, grad_disp2, grad_sim) as device tensors in the graph's match layout ([n_matches, 18],
        [n_matches, 18], [n_matches]; float32, or float64 with f64=True), and the stats dict when want_stats (that waits).
        gauss_newton=True: H = J^T J instead of the exact Hessian (LFR_BACKWARD_GAUSS_NEWTON): positive definite where the exact one
        is not, so those components get a gradient too; BACKWARD_INDEFINITE then means singular.
        gn_fallback=True: the exact Hessian, and J^T J for the components where it is indefinite (LFR_BACKWARD_FALLBACK_GAUSS_NEWTON):
        backward_status() reads BACKWARD_FALLBACK for those, BACKWARD_INDEFINITE where J^T J is singular too.  With gauss_newton=True:
        ValueError."""
        import torch
        if gauss_newton and gn_fallback:
            raise ValueError("backward: gauss_newton and gn_fallback exclude each other")
        n = self.problem.graph.n_nodes
        m = self.problem.graph.n_edges // 2
        g = grad_positions.detach().to(dtype=torch.float64).contiguous()
        if not g.is_cuda or g.numel() != 2 * n:
            raise ValueError("backward: need a [%d, 2] float64 device tensor" % n)
        dt = torch.float64 if f64 else torch.float32
        g1 = torch.empty((m, 18), dtype=dt, device=g.device)
        g2 = torch.empty((m, 18), dtype=dt, device=g.device)
        gs = torch.empty((m,), dtype=dt, device=g.device)
        if stream is None:
            stream = torch.cuda.current_stream(g.device).cuda_stream
        st = BackwardStats()
        _check(lib().lfr_batch_backward(self._h, C.c_void_p(g.data_ptr() or 1), C.c_void_p(g1.data_ptr() or 1), C.c_void_p(g2.data_ptr() or 1), C.c_void_p(gs.data_ptr() or 1),
                                        (BACKWARD_F64 if f64 else 0) | (BACKWARD_GAUSS_NEWTON if gauss_newton else 0)
                                        | (BACKWARD_FALLBACK_GAUSS_NEWTON if gn_fallback else 0),
                                        C.c_void_p(stream) if stream else None,
                                        C.byref(st) if want_stats else None))
        if want_stats:
            return g1, g2, gs, st.as_dict()
        return g1, g2, gs

    def backward_status(self):
        """Per component (order of component_info) of the latest backward: BACKWARD_OK / _NOT_USABLE / _INDEFINITE / _FALLBACK."""
        n = lib().lfr_batch_component_info(self._h, None, None, None, None, None, None)
        out = np.zeros(max(n, 0), np.int32)
        rc = lib().lfr_batch_backward_status(self._h, _ptr(out))
        if rc < 0:
            _check(rc)
        return out

    def jvp(self, tan_disp1=None, tan_disp2=None, tan_sim=None, f64=False, gauss_newton=False, stream=None, want_stats=False,
            gn_fallback=False):
        """Forward-mode sensitivity of the latest solve (lfr_batch_jvp, include/lfr.h): the tangent of the positions for the tangents
        of the flows and similarities - contiguous tensors on the batch's device in the graph's match layout, tan_disp1 / tan_disp2:
        [n_matches, 18] or [n_matches, 9, 2], given together or not at all (None = zero); tan_sim: [n_matches] (None = zero); float32,
        or float64 with f64=True.  Returns the [n_nodes, 2] float64 device tensor J thetadot (0 for roots, bound coordinates, unsolved
        nodes and the nodes of components that are not usable or indefinite), and the stats dict when want_stats (that waits).
        gauss_newton=True: H = J^T J instead of the exact Hessian (LFR_JVP_GAUSS_NEWTON), the mode of backward(gauss_newton=True).
        gn_fallback=True: the exact Hessian, and J^T J where it is indefinite (LFR_JVP_FALLBACK_GAUSS_NEWTON, jvp_status() JVP_FALLBACK),
        the mode of backward(gn_fallback=True).  With gauss_newton=True: ValueError."""
        import torch
        if gauss_newton and gn_fallback:
            raise ValueError("jvp: gauss_newton and gn_fallback exclude each other")
        n = self.problem.graph.n_nodes
        m = self.problem.graph.n_edges // 2
        dev = torch.device("cuda", self.device)
        dt = torch.float64 if f64 else torch.float32

        def ptr(t, name, shapes):
            if t is None:
                return None
            if not isinstance(t, torch.Tensor):
                raise ValueError("jvp: %s must be a torch tensor" % name)
            if not t.is_cuda or t.device != dev:
                raise ValueError("jvp: %s is on %s, the batch on %s" % (name, t.device, dev))
            if t.dtype != dt:
                raise ValueError("jvp: %s is %s, need %s" % (name, t.dtype, dt))
            if tuple(t.shape) not in shapes or not t.is_contiguous():
                raise ValueError("jvp: %s has shape %s, need a contiguous %s" % (name, tuple(t.shape), " or ".join(map(str, shapes))))
            return C.c_void_p(t.data_ptr() or 1)          # (no matches: an empty tensor has no address, and nothing is read)

        flow_shapes = ((m, 18), (m, 9, 2))
        p1, p2, ps = ptr(tan_disp1, "tan_disp1", flow_shapes), ptr(tan_disp2, "tan_disp2", flow_shapes), ptr(tan_sim, "tan_sim", ((m,),))
        out = torch.empty((n, 2), dtype=torch.float64, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        st = JvpStats()
        _check(lib().lfr_batch_jvp(self._h, p1, p2, ps, C.c_void_p(out.data_ptr() or 1),
                                   (JVP_F64 if f64 else 0) | (JVP_GAUSS_NEWTON if gauss_newton else 0)
                                   | (JVP_FALLBACK_GAUSS_NEWTON if gn_fallback else 0),
                                   C.c_void_p(stream) if stream else None, C.byref(st) if want_stats else None))
        if want_stats:
            return out, st.as_dict()
        return out

    def jvp_status(self):
        """Per component (order of component_info) of the latest jvp: JVP_OK / _NOT_USABLE / _INDEFINITE / _FALLBACK."""
        n = lib().lfr_batch_component_info(self._h, None, None, None, None, None, None)
        out = np.zeros(max(n, 0), np.int32)
        rc = lib().lfr_batch_jvp_status(self._h, _ptr(out))
        if rc < 0:
            _check(rc)
        return out

    def covariance(self, f64=False, stream=None, want_stats=False):
        """Per-keypoint covariance of the latest solve (lfr_batch_covariance, include/lfr.h): a [n_nodes, 3] device tensor of
        C(di,di), C(di,dj), C(dj,dj) per node in the solver's unit squared (float32, or float64 with f64=True); 0 for roots, unsolved
        nodes and the nodes of components that are not usable or singular.  With want_stats also the stats dict (that waits)."""
        import torch
        n = self.problem.graph.n_nodes
        dev = torch.device("cuda", self.device)
        cov = torch.empty((n, 3), dtype=torch.float64 if f64 else torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        st = CovarianceStats()
        _check(lib().lfr_batch_covariance(self._h, C.c_void_p(cov.data_ptr() or 1), COVARIANCE_F64 if f64 else 0,
                                          C.c_void_p(stream) if stream else None, C.byref(st) if want_stats else None))
        if want_stats:
            return cov, st.as_dict()
        return cov

    def covariance_matches(self, f64=True, want=("cov", "cross", "relative"), stream=None, want_stats=False):
        """Covariance between matched keypoints of the latest solve (lfr_batch_covariance_matches, include/lfr.h), from one assembly
        and one inversion per component.  Returns a dict of device tensors, one per name in `want`: "cov" [n_nodes, 3] exactly as
        covariance() gives it; "cross" [n_matches, 2, 2] = Cov(x_node1, x_node2) in the graph's match layout (0 for a constant end, a
        dropped edge, a match outside the batch, a component without covariance); "relative" [n_matches, 3] = D(di,di), D(di,dj),
        D(dj,dj) of D = Cov(x_node2 - x_node1), formed in fp64 ((-1, 0, -1): the match is no residual block of this batch; zeros: its
        component has no covariance).  float64, or float32 with f64=False; the solver's unit squared.  With want_stats also "stats"
        (that waits)."""
        import torch
        want = tuple(want)
        if not want or any(w not in ("cov", "cross", "relative") for w in want):
            raise ValueError("covariance_matches: want takes \"cov\", \"cross\", \"relative\" (at least one), got %r" % (want,))
        n = self.problem.graph.n_nodes
        m = self.problem.graph.n_edges // 2
        dev = torch.device("cuda", self.device)
        dt = torch.float64 if f64 else torch.float32
        shapes = {"cov": (n, 3), "cross": (m, 2, 2), "relative": (m, 3)}
        out = {k: torch.empty(shapes[k], dtype=dt, device=dev) for k in ("cov", "cross", "relative") if k in want}
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream

        def ptr(name):
            return C.c_void_p(out[name].data_ptr() or 1) if name in out else None

        st = CovarianceStats()
        _check(lib().lfr_batch_covariance_matches(self._h, ptr("cov"), ptr("cross"), ptr("relative"), COVARIANCE_F64 if f64 else 0,
                                                  C.c_void_p(stream) if stream else None, C.byref(st) if want_stats else None))
        if want_stats:
            out["stats"] = st.as_dict()
        return out

    def covariance_status(self):
        """Per component (order of component_info) of the latest covariance: COVARIANCE_OK / _NOT_USABLE / _SINGULAR."""
        n = lib().lfr_batch_component_info(self._h, None, None, None, None, None, None)
        out = np.zeros(max(n, 0), np.int32)
        rc = lib().lfr_batch_covariance_status(self._h, _ptr(out))
        if rc < 0:
            _check(rc)
        return out

    def evaluate(self, positions=None, *, cost=True, grad=True, residuals=True, weights=True, f64=True, stream=None, want_stats=False):
        """Objective, gradient, residuals and loss weights at `positions` (lfr_batch_evaluate, include/lfr.h): a [n_nodes, 2] float64
        tensor on the batch's device, or None = the batch's own positions (after a solve).  Returns a dict of device tensors, one per
        output asked for: "cost" [n_components] float64 in the order of component_info, "grad" [n_nodes, 2] float64 (dF/dx; 0 for
        constant and unsolved nodes), "residuals" [n_matches, 2, 2] (per match the raw (r_di, r_dj) of edge node1->node2, then of
        node2->node1) and "weights" [n_matches, 2] (rho' of the two edges; -1: the direction is no residual block of this batch),
        float64 or float32 with f64=False; with want_stats also "stats" (that waits)."""
        import torch
        n = self.problem.graph.n_nodes
        m = self.problem.graph.n_edges // 2
        dev = torch.device("cuda", self.device)
        pos = None
        if positions is not None:
            if not isinstance(positions, torch.Tensor) or not positions.is_cuda or positions.device != dev or positions.numel() != 2 * n:
                raise ValueError("evaluate: need a [%d, 2] float64 tensor on %s" % (n, dev))
            pos = positions.detach().to(dtype=torch.float64).contiguous()
        dt = torch.float64 if f64 else torch.float32
        out = {}
        if cost:
            nc = lib().lfr_batch_component_info(self._h, None, None, None, None, None, None)
            if nc < 0:
                _check(int(nc))
            out["cost"] = torch.empty((nc,), dtype=torch.float64, device=dev)
        if grad:
            out["grad"] = torch.empty((n, 2), dtype=torch.float64, device=dev)
        if residuals:
            out["residuals"] = torch.empty((m, 2, 2), dtype=dt, device=dev)
        if weights:
            out["weights"] = torch.empty((m, 2), dtype=dt, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream

        def ptr(name):
            return C.c_void_p(out[name].data_ptr() or 1) if name in out else None

        st = EvaluateStats()
        _check(lib().lfr_batch_evaluate(self._h, None if pos is None else C.c_void_p(pos.data_ptr() or 1), ptr("cost"), ptr("grad"),
                                        ptr("residuals"), ptr("weights"), EVALUATE_F64 if f64 else 0,
                                        C.c_void_p(stream) if stream else None, C.byref(st) if want_stats else None))
        if want_stats:
            out["stats"] = st.as_dict()
        return out

    def evaluate_vjp(self, positions=None, *, cost_bar=None, residuals_bar=None, weights_bar=None, want=("positions", "disp", "sim"),
                     f64=True, stream=None, want_stats=False):
        """Vector-Jacobian product of evaluate()'s differentiable outputs (lfr_batch_evaluate_vjp, include/lfr.h): the gradient of
        sum cost_bar * cost + sum residuals_bar * residuals + sum weights_bar * weights with respect to the positions, the flows and
        the similarities, at `positions` ([n_nodes, 2] float64 on the batch's device, None = the batch's own) with the records as they
        are now - the explicit partials, to be added to backward()'s implicit ones.  cost_bar: [n_components] float64 in the order of
        component_info; residuals_bar: [n_matches, 2, 2]; weights_bar: [n_matches, 2] - float64, or float32 with f64=False; None =
        zero, at least one is needed.  Returns a dict of device tensors, one per name in `want`: "positions" [n_nodes, 2] float64 (0
        for nodes that are not variable), "disp1" / "disp2" [n_matches, 18] for "disp" and "sim" [n_matches], float64 or float32
        with f64=False (0 for directions that are no residual block of this batch); with want_stats also "stats" (that waits)."""
        import torch
        want = tuple(want)
        if not want or any(w not in ("positions", "disp", "sim") for w in want):
            raise ValueError("evaluate_vjp: want takes \"positions\", \"disp\", \"sim\" (at least one), got %r" % (want,))
        n = self.problem.graph.n_nodes
        m = self.problem.graph.n_edges // 2
        dev = torch.device("cuda", self.device)
        dt = torch.float64 if f64 else torch.float32

        def ptr(t, name, shapes, dtype):
            if t is None:
                return None
            if not isinstance(t, torch.Tensor):
                raise ValueError("evaluate_vjp: %s must be a torch tensor" % name)
            if not t.is_cuda or t.device != dev:
                raise ValueError("evaluate_vjp: %s is on %s, the batch on %s" % (name, t.device, dev))
            if t.dtype != dtype:
                raise ValueError("evaluate_vjp: %s is %s, need %s" % (name, t.dtype, dtype))
            if tuple(t.shape) not in shapes or not t.is_contiguous():
                raise ValueError("evaluate_vjp: %s has shape %s, need a contiguous %s" % (name, tuple(t.shape), " or ".join(map(str, shapes))))
            return C.c_void_p(t.data_ptr() or 1)          # (no matches: an empty tensor has no address, and nothing is read)

        nc = lib().lfr_batch_component_info(self._h, None, None, None, None, None, None)
        if nc < 0:
            _check(int(nc))
        pp = ptr(positions, "positions", ((n, 2), (2 * n,)), torch.float64)
        pc = ptr(cost_bar, "cost_bar", ((nc,),), torch.float64)
        pr = ptr(residuals_bar, "residuals_bar", ((m, 2, 2), (m, 4)), dt)
        pw = ptr(weights_bar, "weights_bar", ((m, 2),), dt)
        out = {}
        if "positions" in want:
            out["positions"] = torch.empty((n, 2), dtype=torch.float64, device=dev)
        if "disp" in want:
            out["disp1"] = torch.empty((m, 18), dtype=dt, device=dev)
            out["disp2"] = torch.empty((m, 18), dtype=dt, device=dev)
        if "sim" in want:
            out["sim"] = torch.empty((m,), dtype=dt, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream

        def optr(name):
            return C.c_void_p(out[name].data_ptr() or 1) if name in out else None

        st = EvaluateVjpStats()
        _check(lib().lfr_batch_evaluate_vjp(self._h, pp, pc, pr, pw, optr("positions"), optr("disp1"), optr("disp2"), optr("sim"),
                                            EVALUATE_F64 if f64 else 0, C.c_void_p(stream) if stream else None,
                                            C.byref(st) if want_stats else None))
        if want_stats:
            out["stats"] = st.as_dict()
        return out

    def hessian_product(self, vectors, positions=None, *, gauss_newton=False, free_set=False, products=True, curvature=False,
                        stream=None, want_stats=False):
        """Matrix-free H v at `positions` (lfr_batch_hessian_product, include/lfr.h): H the exact Hessian of evaluate()'s objective,
        or the loss-corrected Gauss-Newton matrix with gauss_newton=True, per component over the coordinates of its variable nodes,
        with the records as they are now.  vectors: a contiguous [K, n_nodes, 2] (1 <= K <= HVP_MAX_VECTORS) or [n_nodes, 2] float64
        tensor on the batch's device, in the layout of the positions; entries of nodes that are not variable are ignored.  positions:
        a contiguous [n_nodes, 2] float64 tensor, or None = the batch's own (after a solve).  free_set=True: coordinates with
        |x| >= 1 are identity rows and columns, as in backward().  Returns a dict of device tensors: "products" with the shape of
        `vectors` (0 for nodes that are not variable) and / or "curvature" [K, n_components] ([n_components] for one [n_nodes, 2]
        vector), v . H v per component in the order of component_info; with want_stats also "stats" (that waits)."""
        import torch
        n = self.problem.graph.n_nodes
        dev = torch.device("cuda", self.device)

        def check(t, name, shapes):
            return _f64_device_tensor("hessian_product", t, name, shapes, dev)

        pv = check(vectors, "vectors", ((None, n, 2), (n, 2)))
        single = vectors.dim() == 2
        k = 1 if single else int(vectors.shape[0])
        if not 1 <= k <= HVP_MAX_VECTORS:
            raise ValueError("hessian_product: %d vectors, need 1 to %d" % (k, HVP_MAX_VECTORS))
        pp = None if positions is None else check(positions, "positions", ((n, 2),))
        out = {}
        if products:
            out["products"] = torch.empty(tuple(vectors.shape), dtype=torch.float64, device=dev)
        if curvature:
            nc = lib().lfr_batch_component_info(self._h, None, None, None, None, None, None)
            if nc < 0:
                _check(int(nc))
            out["curvature"] = torch.empty((nc,) if single else (k, nc), dtype=torch.float64, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream

        def optr(name):
            return C.c_void_p(out[name].data_ptr() or 1) if name in out else None

        st = HessianProductStats()
        flags = (HVP_GAUSS_NEWTON if gauss_newton else 0) | (HVP_FREE_SET if free_set else 0)
        _check(lib().lfr_batch_hessian_product(self._h, pp, pv, k, optr("products"), optr("curvature"), flags,
                                               C.c_void_p(stream) if stream else None, C.byref(st) if want_stats else None))
        if want_stats:
            out["stats"] = st.as_dict()
        return out

    def hessian_solve(self, rhs, positions=None, *, gauss_newton=False, free_set=False, damping=0.0, rel_tolerance=1e-10,
                      max_iterations=None, want_info=True, want_stats=False, stream=None):
        """Matrix-free (H + damping I) y = rhs per component by block-Jacobi preconditioned conjugate gradients inside the kernel
        (lfr_batch_hessian_solve, include/lfr.h), H the matrix of hessian_product() under the same gauss_newton / free_set at
        `positions` (a contiguous [n_nodes, 2] float64 tensor, or None = the batch's own after a solve).  rhs: a contiguous
        [K, n_nodes, 2] (1 <= K <= HVP_MAX_VECTORS) or [n_nodes, 2] float64 tensor on the batch's device.  A component stops when
        |r|_2 <= rel_tolerance |rhs|_2 (status HSOLVE_OK), after max_iterations steps (HSOLVE_MAX_ITERATIONS; None = 4 x the rows of
        the largest component), at a direction of non-positive curvature (HSOLVE_NEGATIVE_CURVATURE: the iterate before it) or at a
        value that is not finite (HSOLVE_NONFINITE).  Returns a dict of device tensors: "solutions" with the shape of `rhs` and, with
        want_info, "status", "iterations" (int32) and "residual" (float64), [K, n_components] ([n_components] for one [n_nodes, 2]
        right-hand side) in the order of component_info; with want_stats also "stats" (that waits)."""
        import torch
        n = self.problem.graph.n_nodes
        dev = torch.device("cuda", self.device)

        def check(t, name, shapes):
            return _f64_device_tensor("hessian_solve", t, name, shapes, dev)

        pr = check(rhs, "rhs", ((None, n, 2), (n, 2)))
        single = rhs.dim() == 2
        k = 1 if single else int(rhs.shape[0])
        if not 1 <= k <= HVP_MAX_VECTORS:
            raise ValueError("hessian_solve: %d right-hand sides, need 1 to %d" % (k, HVP_MAX_VECTORS))
        pp = None if positions is None else check(positions, "positions", ((n, 2),))
        damping, rel_tolerance = float(damping), float(rel_tolerance)
        if not (0.0 <= damping < float("inf")):
            raise ValueError("hessian_solve: damping %r, need a finite value >= 0" % damping)
        if not rel_tolerance >= 0.0:
            raise ValueError("hessian_solve: rel_tolerance %r, need a value >= 0" % rel_tolerance)
        nc = lib().lfr_batch_component_info(self._h, None, None, None, None, None, None)
        if nc < 0:
            _check(int(nc))
        if max_iterations is None:
            nvar = np.zeros(nc, np.int32)
            lib().lfr_batch_component_info(self._h, None, None, None, None, _ptr(nvar), None)
            max_iterations = max(1, 8 * int(nvar.max(initial=0)))          # 4 x the rows (two per node) of the largest component
        max_iterations = int(max_iterations)
        if max_iterations < 1:
            raise ValueError("hessian_solve: max_iterations %d, need at least 1" % max_iterations)
        out = {"solutions": torch.empty(tuple(rhs.shape), dtype=torch.float64, device=dev)}
        if want_info:
            shape = (nc,) if single else (k, nc)
            out["status"] = torch.empty(shape, dtype=torch.int32, device=dev)
            out["iterations"] = torch.empty(shape, dtype=torch.int32, device=dev)
            out["residual"] = torch.empty(shape, dtype=torch.float64, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream

        def optr(name):
            return C.c_void_p(out[name].data_ptr() or 1) if name in out else None

        st = HessianSolveStats()
        flags = (HSOLVE_GAUSS_NEWTON if gauss_newton else 0) | (HSOLVE_FREE_SET if free_set else 0)
        _check(lib().lfr_batch_hessian_solve(self._h, pp, pr, k, damping, rel_tolerance, max_iterations, optr("solutions"), optr("status"),
                                             optr("iterations"), optr("residual"), flags, C.c_void_p(stream) if stream else None,
                                             C.byref(st) if want_stats else None))
        if want_stats:
            out["stats"] = st.as_dict()
        return out

    def tree_stats(self):
        """Per component (order of component_info): columns / tiles / 16x16x16 updates per factorization / levels / sweep items of the
        elimination-tree plan (zeros for components of the other kernel classes)."""
        n = lib().lfr_batch_tree_stats(self._h, None, None, None, None, None)
        if n < 0:
            _check(int(n))
        out = {k: np.zeros(n, np.int64) for k in ("columns", "tiles", "updates", "levels", "items")}
        lib().lfr_batch_tree_stats(self._h, _ptr(out["columns"]), _ptr(out["tiles"]), _ptr(out["updates"]), _ptr(out["levels"]), _ptr(out["items"]))
        return out

    def spin_timeouts(self):
        """Bounded spin-waits of the workgroup kernels that ran out during the latest solve (0 on a healthy run)."""
        n = lib().lfr_batch_spin_timeouts(self._h)
        if n < 0:
            _check(int(n))
        return int(n)

    def team_runs(self):
        """Components the latest solve handed to a team of two or more workgroups (elimination-tree class)."""
        n = lib().lfr_batch_team_runs(self._h)
        if n < 0:
            _check(int(n))
        return int(n)

    def team_fallbacks(self):
        """Components the latest solve's teams could not serve at their size (CUs not resident together) and one workgroup solved."""
        n = lib().lfr_batch_team_fallbacks(self._h)
        if n < 0:
            _check(int(n))
        return int(n)

    def component_info(self):
        n = lib().lfr_batch_component_info(self._h, None, None, None, None, None, None)
        if n < 0:
            _check(int(n))
        comp = np.zeros(n, np.int64)
        it = np.zeros(n, np.int32)
        term = np.zeros(n, np.int32)
        cost = np.zeros(n, np.float64)
        nvar = np.zeros(n, np.int32)
        ne = np.zeros(n, np.int32)
        lib().lfr_batch_component_info(self._h, _ptr(comp), _ptr(it), _ptr(term), _ptr(cost), _ptr(nvar), _ptr(ne))
        return {"component": comp, "iterations": it, "termination": term, "final_cost": cost,
                "n_var_nodes": nvar, "n_edges": ne}


def tree_plan(n_var, words):
    """Elimination-tree plan of one large component (lfr_debug_tree_plan): (blob of uint32 words as the kernel reads it, info dict)."""
    w = np.ascontiguousarray(words, np.uint32)
    info = np.zeros(8, np.int64)
    n = lib().lfr_debug_tree_plan(int(n_var), int(w.shape[0]), _ptr(w), None, 0, _ptr(info))
    if n < 0:
        _check(int(n))
    blob = np.zeros(int(n), np.uint32)
    lib().lfr_debug_tree_plan(int(n_var), int(w.shape[0]), _ptr(w), _ptr(blob), int(n), _ptr(info))
    keys = ("blocks", "tiles", "levels", "items", "updates", "tracks", "segments", "column_rounds")
    return blob, {k: int(v) for k, v in zip(keys, info)}
