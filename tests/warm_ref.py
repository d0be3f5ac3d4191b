"""Reference of lfr_batch_solve_from (include/lfr.h): ceres::Solve started at given parameter values.  Not a test.

`solve_from` RESTATES oracle/lfr_ref.py's `solve_problem` - the same statements in the same order - with three differences, the ones
the header names: the start is `problem.project(x0)` with every NaN of x0 read as 0 beforehand (solve_problem: project(zeros)), so
x_norm starts at |project(x0)|; and a FAILURE returns that projected start (solve_problem: zeros; Ceres itself would leave the
caller's unprojected values).  tests/test_warm_ref.py pins the restatement to solve_problem bit for bit, trace entry for trace entry,
at x0 = 0.  It is written out here because oracle/ does not change.

`components` builds the per-component `Problem`s of a MatchArrays the way lfr_ref.solve_pairs does and keeps, per component, the graph
nodes of its variable rows; `solve_graph` runs solve_from over them from a [n_nodes, 2] start array."""
import math

import numpy as np

import lfr_ref as R


def solve_from(problem, x0, trace=None):
    """Returns (x, info) like lfr_ref.solve_problem; x0: 2 * nv start values (any floats)."""
    nv2 = 2 * problem.nv
    info = {"iterations": 0, "termination": R.TERM_CONVERGENCE, "final_cost": 0.0,
            "n_ls_evals": 0, "n_successful": 0}
    if nv2 == 0:
        return np.zeros(0), info
    x0 = np.array(x0, np.float64).reshape(nv2)
    x0[np.isnan(x0)] = 0.0
    x = problem.project(x0)               # IterationZero: project onto the bounds
    x_start = x.copy()
    x_norm = float(np.linalg.norm(x))
    cost, r, J, g = problem.evaluate(x, True)
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(axis=0)))      # jacobi scaling, computed once
    Js = J * scale[None, :]

    def _gmax(x_, g_):
        return float(np.max(np.abs(x_ - problem.project(x_ - g_))))

    gmax = _gmax(x, g)
    best_x = x.copy()
    min_cost = cost
    radius = R.INITIAL_RADIUS
    decrease_factor = 2.0
    reuse_diagonal = False
    diagonal = None
    n_invalid = 0
    step_successful = True
    iteration = 0
    if trace is not None:
        trace.append({"it": 0, "cost": cost, "gmax": gmax, "radius": radius, "ok": True})

    while True:
        if iteration >= R.MAX_NUM_ITERATIONS:
            info["termination"] = R.TERM_NO_CONVERGENCE
            break
        if step_successful and gmax <= R.GRADIENT_TOLERANCE:
            info["termination"] = R.TERM_CONVERGENCE
            break
        if radius <= R.MIN_RADIUS:
            info["termination"] = R.TERM_CONVERGENCE
            break
        iteration += 1
        step_successful = False

        if not reuse_diagonal:
            diagonal = np.clip((Js * Js).sum(axis=0), R.MIN_LM_DIAGONAL, R.MAX_LM_DIAGONAL)
        D = np.sqrt(diagonal / radius)
        reuse_diagonal = True
        H = Js.T @ Js + np.diag(D * D)
        rhs = Js.T @ r
        valid = True
        try:
            L = np.linalg.cholesky(H)
            y = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
            step = -y
            if not np.all(np.isfinite(step)):
                valid = False
        except np.linalg.LinAlgError:
            valid = False
        model_cost_change = 0.0
        if valid:
            mr = Js @ step
            model_cost_change = float(-mr @ (r + mr / 2.0))
            valid = model_cost_change > 0.0
        if not valid:
            n_invalid += 1
            if n_invalid >= R.MAX_CONSECUTIVE_INVALID:
                info["termination"] = R.TERM_FAILURE
                break
            radius = radius / decrease_factor
            decrease_factor *= 2.0
            reuse_diagonal = True
            if trace is not None:
                trace.append({"it": iteration, "invalid": True, "radius": radius})
            continue
        n_invalid = 0
        delta = step * scale

        ok, alpha, n_ev = R.armijo_line_search(problem, x, delta, cost, float(g @ delta))
        info["n_ls_evals"] += n_ev
        if ok:
            delta = delta * alpha

        x_cand = problem.project(x + delta)
        cost_cand, _, _, _ = problem.evaluate(x_cand, False)
        if not math.isfinite(cost_cand):
            cost_cand = R.DBL_MAX

        step_norm = float(np.linalg.norm(x - x_cand))
        if step_norm <= R.PARAMETER_TOLERANCE * (x_norm + R.PARAMETER_TOLERANCE):
            info["termination"] = R.TERM_CONVERGENCE
            if trace is not None:
                trace.append({"it": iteration, "stop": "parameter", "step_norm": step_norm})
            break
        cost_change = cost - cost_cand
        if abs(cost_change) <= R.FUNCTION_TOLERANCE * cost:
            info["termination"] = R.TERM_CONVERGENCE
            if trace is not None:
                trace.append({"it": iteration, "stop": "function", "cost_change": cost_change})
            break

        rel = cost_change / model_cost_change
        if rel > R.MIN_RELATIVE_DECREASE:
            x = x_cand
            x_norm = float(np.linalg.norm(x))
            cost, r, J, g = problem.evaluate(x, True)
            Js = J * scale[None, :]
            gmax = _gmax(x, g)
            step_successful = True
            info["n_successful"] += 1
            radius = radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3)
            radius = min(R.MAX_RADIUS, radius)
            decrease_factor = 2.0
            reuse_diagonal = False
            if cost < min_cost:
                min_cost = cost
                best_x = x.copy()
        else:
            radius = radius / decrease_factor
            decrease_factor *= 2.0
            reuse_diagonal = True
        if trace is not None:
            trace.append({"it": iteration, "cost": cost, "cost_cand": cost_cand, "rel": rel,
                          "ok": step_successful, "radius": radius, "alpha": alpha if ok else None,
                          "gmax": gmax, "model_cost_change": model_cost_change})

    info["iterations"] = iteration
    info["final_cost"] = min_cost
    info["n_cost_evals"] = problem.n_cost_evals
    info["n_jac_evals"] = problem.n_jac_evals
    if info["termination"] == R.TERM_FAILURE:
        return x_start, info
    return best_x, info


def components(ma, tukey_variant="ceres1", bisect_fn=None, banned=()):
    """{component id: (graph nodes of the variable rows, lfr_ref.Problem)} of a MatchArrays, built as lfr_ref.solve_pairs builds them
    (components of one node are skipped, solve.cc:619-622); also returns the number of graph nodes."""
    g = R.MatchGraph(ma.to_pairs(), banned)
    out = {}
    if g.n_nodes == 0:
        return out, 0
    track, n_tracks = R.build_tracks(g)
    is_root = R.select_roots(g, track, n_tracks)
    comp, n_comp, _ = R.split_components(g, track, n_tracks, len(g.images_set), bisect_fn)
    nodes_in = [[] for _ in range(n_comp)]
    for i in range(g.n_nodes):
        nodes_in[comp[i]].append(i)
    for c in range(n_comp):
        if len(nodes_in[c]) == 1:
            continue
        var_nodes, edges = R.assemble_component(g, track, is_root, comp, nodes_in[c])
        out[c] = (np.array(var_nodes, np.int64), R.Problem(len(var_nodes), edges, tukey_variant))
    return out, g.n_nodes


def fresh(problem):
    """the same Problem with its evaluation counters at zero (solve_from counts into them)"""
    return R.Problem(problem.nv, problem.edges, problem.tukey_variant)


def solve_graph(comps, n_nodes, start, want_trace=False):
    """solve_from on every component from the [n_nodes, 2] array `start` (None: zeros) -> (positions [n_nodes, 2] - nodes that are no
    variable of a component stay 0 -, {component: info})."""
    pos = np.zeros((n_nodes, 2))
    infos = {}
    start = np.zeros((n_nodes, 2)) if start is None else np.asarray(start, np.float64)
    for c, (var_nodes, prob) in comps.items():
        tr = [] if want_trace else None
        p = fresh(prob)
        x, info = solve_from(p, start[var_nodes].reshape(-1), tr)
        if want_trace:
            info["trace"] = tr
        info["n_edges"] = len(p.edges)
        info["n_var_nodes"] = p.nv
        infos[c] = info
        pos[var_nodes] = x.reshape(-1, 2)
    return pos, infos
