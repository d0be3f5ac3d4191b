"""PyTorch autograd through the batched LM solve: the two-view network's flows (and the similarities) in, refined positions out, and
the implicit-function-theorem gradient back (lfr_batch_backward, include/lfr.h) - or, in forward mode, the tangent
of the positions for tangents of the flows and similarities (lfr_batch_jvp).

    pos, node_image, node_feature = refine(disp1, disp2, sim, image_names=..., pair_img1=..., pair_img2=..., pair_off=...,
                                           feat1=..., feat2=...)
    loss(pos).backward()        # fills disp1.grad, disp2.grad, sim.grad

A training loop solves the same scenes again and again and only the network's outputs change: `Refiner` runs the graph stage and the
assembly ONCE and gives every later forward new flows (and similarities) into the live batch (lfr_batch_set_inputs):

    r = Refiner(disp1, disp2, sim, image_names=..., pair_img1=..., pair_img2=..., pair_off=..., feat1=..., feat2=...)
    for step in ...:
        pos = r(disp1, disp2)           # set_inputs + solve + positions on torch's current stream, no host synchronisation
        loss(pos).backward()

Refiner(..., warm_start=True) starts every forward after the first at the previous forward's positions (lfr_batch_solve_from) instead
of the origin: flows that moved a little need fewer LM iterations.  reset_start() makes the next forward a cold one again.

hessian="gauss_newton" (refine and Refiner) takes the implicit gradient with H = J^T J instead of the exact Hessian
(LFR_BACKWARD_GAUSS_NEWTON): components whose exact Hessian is indefinite - zero gradient in the default mode - get one too.
hessian="exact_or_gauss_newton" keeps the exact Hessian wherever its factorization succeeds and takes J^T J only for the components
where it does not (LFR_BACKWARD_FALLBACK_GAUSS_NEWTON / LFR_JVP_FALLBACK_GAUSS_NEWTON; Batch.backward_status() tells which).

One device.  First order in both modes: reverse (backward()) and forward (torch.autograd.forward_ad, Refiner.jvp) - the tangent J
thetadot comes from lfr_batch_jvp with the H of `hessian`, so ubar . (J thetadot) = (J^T ubar) . thetadot holds between the two.  Neither
pass is itself differentiable: no double backward, no forward-over-reverse through the solve.  The graph stage (tracks, roots, components, the cut) is
discrete and the box's active set piecewise constant: the gradient holds them fixed.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import capi
from .synthetic import MatchArrays


_HESSIANS = ("exact", "gauss_newton", "exact_or_gauss_newton")


def _check_hessian(who, hessian):
    if hessian not in _HESSIANS:
        raise ValueError("%s: hessian must be one of %s, got %r" % (who, ", ".join(map(repr, _HESSIANS)), hessian))
    return hessian


def _hessian_flags(hessian):
    """the mode of _check_hessian as the keywords of Batch.backward / Batch.jvp"""
    return {"gauss_newton": hessian == "gauss_newton", "gn_fallback": hessian == "exact_or_gauss_newton"}


def _kept_rows(pair_img1, pair_img2, pair_off, image_names, banned):
    """Input rows of the matches the graph keeps (pairs touching a banned image are skipped, solve.cc:444-446), in graph order."""
    if not banned:
        return None
    bad = np.array([n in set(banned) for n in image_names], bool)
    keep = ~(bad[pair_img1] | bad[pair_img2])
    rows = [np.arange(pair_off[p], pair_off[p + 1], dtype=np.int64) for p in np.nonzero(keep)[0]]
    return np.concatenate(rows) if rows else np.zeros(0, np.int64)


def _all_on(device, *tensors):
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == device for t in tensors)


def _device_indices(t):
    """Feature indices as a contiguous int32 tensor on their device holding the uint32 bit patterns (a wider integer type wraps)."""
    t = t.detach().reshape(-1)
    t = t.view(torch.int32) if t.dtype in (torch.int32, torch.uint32) else t.to(torch.int64).to(torch.int32)
    return t.contiguous()


def _build_graph(who, d1, d2, sim, dev, *, image_names, facts, pair_img1, pair_img2, pair_off, feat1, feat2, banned):
    """The match graph of refine() / Refiner from the flows d1, d2 ([n, 18] float32, contiguous, on HIP device `dev`).  feat1, feat2
    and sim all torch tensors on that device: the nodes are numbered there (lfr_graph_from_device_arrays) and nothing comes to the
    host; anything else: the host numbering over host copies (lfr_graph_from_arrays_device_flows).  Call inside
    torch.cuda.device(dev)."""
    ma = MatchArrays(image_names=list(image_names), facts=facts, pair_img1=pair_img1, pair_img2=pair_img2, pair_off=pair_off,
                     feat1=None, feat2=None, sim=None, disp1=None, disp2=None)
    if _all_on(d1.device, feat1, feat2, sim):
        f1, f2 = _device_indices(feat1), _device_indices(feat2)
        s = sim.detach().to(torch.float32).reshape(-1).contiguous()
        n = int(pair_off[-1]) if len(pair_off) else 0
        if not (f1.numel() == f2.numel() == s.numel() == d1.shape[0] == d2.shape[0] == n):
            raise ValueError("%s: pair_off ends at %d, feat1 / feat2 / sim / disp1 / disp2 have %d / %d / %d / %d / %d rows"
                             % (who, n, f1.numel(), f2.numel(), s.numel(), d1.shape[0], d2.shape[0]))
        # the library reads the arrays on its own streams: they must be complete before the graph takes them
        torch.cuda.current_stream(d1.device).synchronize()
        return capi.Graph.from_device_arrays(ma, f1.data_ptr(), f2.data_ptr(), s.data_ptr(), d1.data_ptr(), d2.data_ptr(), device=dev,
                                             banned=tuple(banned))       # (f1, f2, s are read inside the call only)
    ma.feat1, ma.feat2 = np.ascontiguousarray(feat1, np.uint32), np.ascontiguousarray(feat2, np.uint32)
    ma.sim = sim.detach().to(torch.float32).cpu().numpy()
    # the library reads the flows on its own streams: they must be complete before the graph takes them
    torch.cuda.current_stream(d1.device).synchronize()
    return capi.Graph.from_device_flows(ma, d1.data_ptr(), d2.data_ptr(), device=dev, banned=tuple(banned))


def _tangent_rows(who, tangents, n_rows, idx, device):
    """The tangents of (disp1, disp2, sim) in the caller's rows -> what Batch.jvp takes: the graph's rows (banned pairs dropped
    through idx), contiguous on `device`, float32 or - when one of them is float64 - float64; None stays None (= zero)."""
    t1, t2, ts = tangents
    if t1 is None and t2 is None and ts is None:
        raise ValueError("%s: no tangent (all three are None)" % who)
    f64 = any(t is not None and t.dtype == torch.float64 for t in tangents)
    dt = torch.float64 if f64 else torch.float32

    def rows(t, shape):
        t = t.detach().to(device=device, dtype=dt).reshape(shape)
        if t.shape[0] != n_rows:
            raise ValueError("%s: %d rows, the forward saw %d" % (who, t.shape[0], n_rows))
        return (t if idx is None else t.index_select(0, idx)).contiguous()

    if (t1 is None) != (t2 is None):         # one flow tangent alone: the other is zero
        t1 = torch.zeros_like(t2) if t1 is None else t1
        t2 = torch.zeros_like(t1) if t2 is None else t2
    return (None if t1 is None else rows(t1, (-1, 18)), None if t2 is None else rows(t2, (-1, 18)),
            None if ts is None else rows(ts, (-1,)), f64)


class _Refine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp1, disp2, sim, meta):
        device = disp1.device
        d1 = disp1.detach().to(torch.float32).reshape(-1, 18).contiguous()
        d2 = disp2.detach().to(torch.float32).reshape(-1, 18).contiguous()
        dev = device.index if device.index is not None else torch.cuda.current_device()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(device).cuda_stream
            g = _build_graph("refine", d1, d2, sim, dev, image_names=meta["image_names"], facts=meta["facts"], pair_img1=meta["pair_img1"],
                             pair_img2=meta["pair_img2"], pair_off=meta["pair_off"], feat1=meta["feat1"], feat2=meta["feat2"],
                             banned=meta["banned"])
            p = capi.Problem(g, device_graph_stage=dev)
            b = capi.Batch(p, dev, tukey_variant=meta["tukey_variant"])      # (gathers its records: d1 / d2 may go after this)
            b.solve(stream=stream, want_stats=False)
            pos = torch.empty((g.n_nodes, 2), dtype=torch.float64, device=device)
            b.positions_to(pos, stream=stream)
            if meta["return_covariance"]:      # not an output of the Function: the covariance is not differentiated
                meta["covariance"] = b.covariance(f64=True, stream=stream)
        node_image, node_feature = g.nodes()
        ctx.batch = b
        ctx.meta = meta
        ctx.n_in = (disp1.shape, disp2.shape, sim.shape, disp1.dtype, disp2.dtype, sim.dtype)
        return pos, node_image, node_feature

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_pos, *_):
        b, meta = ctx.batch, ctx.meta
        s1, s2, ss, t1, t2, ts = ctx.n_in
        if grad_pos is None:
            return None, None, None, None
        g1, g2, gs = b.backward(grad_pos, f64=False, **_hessian_flags(meta["hessian"]))
        rows = meta["kept_rows"]
        if rows is not None:        # back to the caller's rows (matches of banned pairs get 0)
            idx = torch.as_tensor(rows, device=g1.device)
            f1 = torch.zeros((ss[0], 18), dtype=g1.dtype, device=g1.device)
            f2 = torch.zeros_like(f1)
            fs = torch.zeros((ss[0],), dtype=gs.dtype, device=gs.device)
            f1[idx], f2[idx], fs[idx] = g1, g2, gs
            g1, g2, gs = f1, f2, fs
        return (g1.reshape(s1).to(t1) if ctx.needs_input_grad[0] else None,
                g2.reshape(s2).to(t2) if ctx.needs_input_grad[1] else None,
                gs.reshape(ss).to(device=gs.device, dtype=ts) if ctx.needs_input_grad[2] else None, None)

    @staticmethod
    def jvp(ctx, tan_disp1, tan_disp2, tan_sim, *_):
        """forward mode (torch.autograd.forward_ad): the tangent of the positions; the node maps have none"""
        b, meta = ctx.batch, ctx.meta
        pos_dev = torch.device("cuda", b.device)
        if tan_disp1 is None and tan_disp2 is None and tan_sim is None:
            return torch.zeros((b.problem.graph.n_nodes, 2), dtype=torch.float64, device=pos_dev), None, None
        rows = meta["kept_rows"]
        idx = None if rows is None else torch.as_tensor(rows, device=pos_dev)
        with torch.cuda.device(pos_dev):
            t1, t2, ts, f64 = _tangent_rows("refine", (tan_disp1, tan_disp2, tan_sim), int(np.prod(ctx.n_in[2])), idx, pos_dev)
            return b.jvp(t1, t2, ts, f64=f64, **_hessian_flags(meta["hessian"])), None, None


def refine(disp1, disp2, sim, *, image_names, pair_img1, pair_img2, pair_off, feat1, feat2, image_facts=None, banned=(),
           tukey_variant="ceres1", return_covariance=False, hessian="exact"):
    """Multi-view refinement of the matches as a differentiable function of the flows and similarities.

    disp1, disp2: [n_matches, 18] (or [n_matches, 9, 2]) float32 tensors on one HIP device - disp2 = flow image1 -> image2, disp1 =
    flow image2 -> image1 (lfr_graph_from_arrays); sim: [n_matches] similarities (any device); the rest as lfr_graph_from_arrays.
    feat1, feat2 (integer tensors) and sim all on the device of disp1: they stay there and the graph is numbered on the GPU
    (lfr_graph_from_device_arrays) - same graph, same results, no copy of the similarities to the host.
    Returns (positions, node_image, node_feature): [n_nodes, 2] float64 device positions (di, dj per node, the solver's unit) and the
    node -> (image index, feature index) map as numpy arrays.  Gradients reach disp1, disp2 and sim; the matches of banned pairs
    get 0.
    return_covariance=True: a fourth value, the [n_nodes, 3] float64 device tensor of lfr_batch_covariance (C(di,di), C(di,dj),
    C(dj,dj) per node, the solver's unit squared; 0 = no covariance for this node).  It is detached: the covariance is not
    differentiated.
    hessian: "exact" (the default), "gauss_newton" or "exact_or_gauss_newton" (exact where the exact Hessian is positive definite,
    Gauss-Newton for the other components) - the H of the backward pass and of forward mode (lfr_batch_backward, lfr_batch_jvp);
    anything else: ValueError."""
    hessian = _check_hessian("refine", hessian)
    pair_img1 = np.ascontiguousarray(pair_img1, np.int32)
    pair_img2 = np.ascontiguousarray(pair_img2, np.int32)
    pair_off = np.ascontiguousarray(pair_off, np.int64)
    facts = np.ones(len(image_names), np.float32) if image_facts is None else np.ascontiguousarray(image_facts, np.float32)
    if not disp1.is_cuda or disp2.device != disp1.device:
        raise ValueError("refine: disp1 and disp2 must be on the same HIP device")
    if not _all_on(disp1.device, feat1, feat2, sim):         # (all three on the flows' device: they stay there, _build_graph)
        feat1, feat2 = np.ascontiguousarray(feat1, np.uint32), np.ascontiguousarray(feat2, np.uint32)
    meta = {"image_names": list(image_names), "facts": facts, "pair_img1": pair_img1, "pair_img2": pair_img2, "pair_off": pair_off,
            "feat1": feat1, "feat2": feat2,
            "banned": tuple(banned), "tukey_variant": tukey_variant, "return_covariance": bool(return_covariance),
            "hessian": hessian,
            "kept_rows": _kept_rows(pair_img1, pair_img2, pair_off, list(image_names), tuple(banned))}
    pos, node_image, node_feature = _Refine.apply(disp1, disp2, sim, meta)
    if return_covariance:
        return pos, node_image, node_feature, meta.pop("covariance").detach()
    return pos, node_image, node_feature


class _RefinerStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp1, disp2, sim, refiner):
        ctx.refiner = refiner
        ctx.epoch = refiner._forward(disp1, disp2, sim)
        ctx.n_in = (disp1.shape, disp2.shape, None if sim is None else sim.shape, disp1.dtype, disp2.dtype,
                    None if sim is None else (sim.dtype, sim.device))
        pos = torch.empty((refiner.n_nodes, 2), dtype=torch.float64, device=refiner.device)
        refiner._batch.positions_to(pos)
        return pos

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_pos):
        r = ctx.refiner
        if r._batch is None:
            raise RuntimeError("Refiner: backward after close()")
        if ctx.epoch != r._epoch:
            raise RuntimeError("Refiner: this forward (step %d) is stale - the shared batch holds only its latest solve (step %d); "
                               "run backward before the next forward" % (ctx.epoch, r._epoch))
        s1, s2, ss, t1, t2, ts = ctx.n_in
        g1, g2, gs = r._batch.backward(grad_pos, f64=False, **_hessian_flags(r._hessian))
        if r._idx is not None:      # back to the caller's rows (matches of banned pairs get 0)
            f1 = torch.zeros((r.n_rows, 18), dtype=g1.dtype, device=g1.device)
            f2 = torch.zeros_like(f1)
            fs = torch.zeros((r.n_rows,), dtype=gs.dtype, device=gs.device)
            f1[r._idx], f2[r._idx], fs[r._idx] = g1, g2, gs
            g1, g2, gs = f1, f2, fs
        return (g1.reshape(s1).to(t1) if ctx.needs_input_grad[0] else None,
                g2.reshape(s2).to(t2) if ctx.needs_input_grad[1] else None,
                gs.reshape(ss).to(device=ts[1], dtype=ts[0]) if ss is not None and ctx.needs_input_grad[2] else None, None)

    @staticmethod
    def jvp(ctx, tan_disp1, tan_disp2, tan_sim, *_):
        """forward mode (torch.autograd.forward_ad): the tangent of the positions of THIS forward"""
        r = ctx.refiner
        if r._batch is None:
            raise RuntimeError("Refiner: jvp after close()")
        if ctx.epoch != r._epoch:
            raise RuntimeError("Refiner: this forward (step %d) is stale - the shared batch holds only its latest solve (step %d)"
                               % (ctx.epoch, r._epoch))
        if tan_disp1 is None and tan_disp2 is None and tan_sim is None:
            return torch.zeros((r.n_nodes, 2), dtype=torch.float64, device=r.device)
        return r.jvp(tan_disp1, tan_disp2, tan_sim)


class _Objective(torch.autograd.Function):
    """Refiner.objective: Batch.evaluate forward, Batch.evaluate_vjp backward (the explicit partials of the cost, the residuals and the
    weights with respect to the positions, the flows and the similarities)."""

    @staticmethod
    def forward(ctx, positions, disp1, disp2, sim, refiner, want_res, want_w):
        r = refiner
        ctx.refiner, ctx.epoch = r, r._epoch
        ctx.set_materialize_grads(False)
        ctx.n_in = (positions.shape, positions.dtype, disp1.shape, disp1.dtype, disp2.shape, disp2.dtype,
                    None if sim is None else (sim.shape, sim.dtype, sim.device))
        with torch.cuda.device(r.device):
            pos = positions.detach().to(device=r.device, dtype=torch.float64).reshape(-1, 2).contiguous()
            out = r._batch.evaluate(pos, cost=True, grad=False, residuals=want_res, weights=want_w, f64=True)
            ctx.pos = pos
            res = [out["cost"]]
            for name, fill in (("residuals", 0.0), ("weights", -1.0)):      # the caller's rows, as Refiner.evaluate gives them
                if name in out:
                    t = out[name]
                    if r._idx is not None:
                        full = torch.full((r.n_rows,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
                        full[r._idx] = t
                        t = full
                    res.append(t)
        ctx.names = ("cost",) + (("residuals",) if want_res else ()) + (("weights",) if want_w else ())
        return tuple(res)

    @staticmethod
    @once_differentiable
    def backward(ctx, *bars):
        r = ctx.refiner
        bars = dict(zip(ctx.names, bars))
        if all(b is None for b in bars.values()):
            return (None,) * 7
        if r._batch is None:
            raise RuntimeError("Refiner: backward after close()")
        if ctx.epoch != r._epoch:
            raise RuntimeError("Refiner: this forward (step %d) is stale - the shared batch holds only its latest solve (step %d); "
                               "run backward before the next forward" % (ctx.epoch, r._epoch))
        sp, tp, s1, t1, s2, t2, ss = ctx.n_in
        need = ctx.needs_input_grad
        want = (("positions",) if need[0] else ()) + (("disp",) if need[1] or need[2] else ()) + (("sim",) if ss is not None and need[3] else ())
        if not want:
            return (None,) * 7
        with torch.cuda.device(r.device):
            def rows(t):       # a bar in the caller's rows -> the graph's rows, float64 (the bars of banned pairs are not read)
                if t is None:
                    return None
                t = t.detach().to(device=r.device, dtype=torch.float64)
                return (t if r._idx is None else t.index_select(0, r._idx)).contiguous()
            cbar = bars["cost"]
            g = r._batch.evaluate_vjp(ctx.pos, cost_bar=None if cbar is None else cbar.detach().to(device=r.device, dtype=torch.float64).contiguous(),
                                      residuals_bar=rows(bars.get("residuals")), weights_bar=rows(bars.get("weights")), want=want, f64=True)
            if r._idx is not None:      # back to the caller's rows (matches of banned pairs get 0)
                for name in ("disp1", "disp2", "sim"):
                    if name in g:
                        full = torch.zeros((r.n_rows,) + tuple(g[name].shape[1:]), dtype=g[name].dtype, device=r.device)
                        full[r._idx] = g[name]
                        g[name] = full
        return (g["positions"].reshape(sp).to(tp) if need[0] else None,
                g["disp1"].reshape(s1).to(t1) if need[1] else None,
                g["disp2"].reshape(s2).to(t2) if need[2] else None,
                g["sim"].reshape(ss[0]).to(device=ss[2], dtype=ss[1]) if ss is not None and need[3] else None, None, None, None)


class Refiner:
    """refine() for a loop over the same scenes: the graph stage (tracks, roots, components) and the batch assembly run once, in the
    constructor, from the values given there; every call gives the live batch new flows - and similarities, if passed - and solves
    it again.  The structure stays that of the constructor's values: similarities that would have produced other tracks or roots do
    not (the gradient holds the structure fixed anyway).

    r(disp1, disp2, sim=None) -> [n_nodes, 2] float64 device positions, differentiable with respect to what was passed (sim=None:
    the similarities stay, no gradient).  Tensors as for refine(), in the caller's rows (banned pairs included).  The forward issues
    set_inputs, solve and the positions' copy on torch's current stream and does not synchronise the host.  The batch is shared and
    holds only its latest solve: backward() of an older forward raises RuntimeError; several backwards of the latest one are fine.
    warm_start=True: every forward after the first starts LM at the previous forward's positions (Batch.solve_from(None)) instead of
    the origin; reset_start() makes the next forward cold again.  The backward is the same either way: the implicit gradient is taken
    at the solution and does not know where LM started.
    hessian: as for refine().  node_image, node_feature, n_nodes: as refine() returns them.  covariance(f64=True): lfr_batch_covariance of the latest solve.
    match_covariance(f64=True): lfr_batch_covariance_matches of the latest solve (cross blocks and relative covariance per match).
    evaluate(positions=None, **kw): lfr_batch_evaluate (cost, dF/dx, residuals, loss weights), detached.
    objective(positions, disp1, disp2, sim=None): the same cost, residuals and weights, differentiable (lfr_batch_evaluate_vjp).
    jvp(tan_disp1, tan_disp2, tan_sim=None): lfr_batch_jvp of the latest forward (the tangent of the positions), detached;
    torch.autograd.forward_ad through r(...) calls it."""

    def __init__(self, disp1, disp2, sim, *, image_names, pair_img1, pair_img2, pair_off, feat1, feat2, image_facts=None, banned=(),
                 tukey_variant="ceres1", hessian="exact", warm_start=False):
        self._hessian = _check_hessian("Refiner", hessian)
        self._warm_start = bool(warm_start)
        self._have_start = False        # the batch's positions are a forward's result
        pair_img1 = np.ascontiguousarray(pair_img1, np.int32)
        pair_img2 = np.ascontiguousarray(pair_img2, np.int32)
        pair_off = np.ascontiguousarray(pair_off, np.int64)
        facts = np.ones(len(image_names), np.float32) if image_facts is None else np.ascontiguousarray(image_facts, np.float32)
        if not disp1.is_cuda or disp2.device != disp1.device:
            raise ValueError("Refiner: disp1 and disp2 must be on the same HIP device")
        device = disp1.device
        dev = device.index if device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", dev)
        d1 = disp1.detach().to(torch.float32).reshape(-1, 18).contiguous()
        d2 = disp2.detach().to(torch.float32).reshape(-1, 18).contiguous()
        self.n_rows = int(d1.shape[0])
        rows = _kept_rows(pair_img1, pair_img2, pair_off, list(image_names), tuple(banned))
        self._idx = None if rows is None else torch.as_tensor(rows, device=self.device)
        with torch.cuda.device(dev):
            self._graph = _build_graph("Refiner", d1, d2, sim, dev, image_names=image_names, facts=facts, pair_img1=pair_img1,
                                       pair_img2=pair_img2, pair_off=pair_off, feat1=feat1, feat2=feat2, banned=banned)
            self._problem = capi.Problem(self._graph, device_graph_stage=dev)
            self._batch = capi.Batch(self._problem, dev, tukey_variant=tukey_variant)     # (gathers its records: d1 / d2 may go after this)
        self.n_nodes = self._graph.n_nodes
        self.node_image, self.node_feature = self._graph.nodes()
        self._epoch = 0
        self._latest = None

    def _forward(self, disp1, disp2, sim):
        if self._batch is None:
            raise RuntimeError("Refiner: called after close()")
        if disp1.device != self.device or disp2.device != self.device:
            raise ValueError("Refiner: disp1 and disp2 must be on %s" % self.device)
        with torch.cuda.device(self.device):
            def rows(t, shape):
                t = t.detach().to(device=self.device, dtype=torch.float32).reshape(shape)
                if t.shape[0] != self.n_rows:
                    raise ValueError("Refiner: %d rows, the constructor saw %d" % (t.shape[0], self.n_rows))
                return (t if self._idx is None else t.index_select(0, self._idx)).contiguous()
            d1, d2 = rows(disp1, (-1, 18)), rows(disp2, (-1, 18))
            s = None if sim is None else rows(sim, (-1,))
            # (d1, d2, s may be temporaries: they are read by work enqueued here, and torch reuses their memory in stream order)
            self._batch.set_inputs(d1, d2, s)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if self._warm_start and self._have_start:
                self._batch.solve_from(None, stream=stream, want_stats=False)
            else:
                self._batch.solve(stream=stream, want_stats=False)
            self._have_start = True
        self._epoch += 1
        return self._epoch

    def __call__(self, disp1, disp2, sim=None):
        pos = _RefinerStep.apply(disp1, disp2, sim, self)
        self._latest = (disp1, disp2, sim)          # objective() checks that it is given these very tensors
        return pos

    def reset_start(self):
        """warm_start=True: the next forward starts at the origin, like the first one (the ones after it are warm again)."""
        self._have_start = False

    def covariance(self, f64=True):
        """[n_nodes, 3] device tensor of lfr_batch_covariance for the latest forward (detached: the covariance is not differentiated)."""
        if self._epoch == 0:
            raise RuntimeError("Refiner: covariance before the first forward")
        with torch.cuda.device(self.device):
            return self._batch.covariance(f64=f64)

    def match_covariance(self, f64=True):
        """Covariance between the matched keypoints of the latest forward (Batch.covariance_matches, lfr_batch_covariance_matches):
        {"cross": [rows, 2, 2] = Cov(x_node1, x_node2), "relative": [rows, 3] = D(di,di), D(di,dj), D(dj,dj) of Cov(x_node2 - x_node1)}
        in the caller's rows and the solver's unit squared: the rows of banned pairs read cross 0 and relative (-1, 0, -1), "not in the
        program".  Detached: the covariance is not differentiated."""
        if self._batch is None:
            raise RuntimeError("Refiner: match_covariance after close()")
        if self._epoch == 0:
            raise RuntimeError("Refiner: match_covariance before the first forward")
        with torch.cuda.device(self.device):
            out = self._batch.covariance_matches(f64=f64, want=("cross", "relative"))
            if self._idx is not None:
                full = torch.zeros((self.n_rows, 2, 2), dtype=out["cross"].dtype, device=self.device)
                full[self._idx] = out["cross"]
                out["cross"] = full
                full = torch.tensor([-1.0, 0.0, -1.0], dtype=out["relative"].dtype, device=self.device).repeat(self.n_rows, 1)
                full[self._idx] = out["relative"]
                out["relative"] = full
        return {k: v.detach() for k, v in out.items()}

    def jvp(self, tan_disp1, tan_disp2, tan_sim=None):
        """Forward-mode sensitivity of the latest forward (Batch.jvp, lfr_batch_jvp): the [n_nodes, 2] float64 tangent of the positions
        for tangents of the flows and / or the similarities in the caller's rows (banned pairs included: their rows are not read; a
        None is a zero tangent, all three None: ValueError).  float32 tangents, or float64 when one of them is.  The H is the
        Refiner's `hessian`, so ubar . r.jvp(t) equals the sum of backward()'s gradients times t.  Detached."""
        if self._batch is None:
            raise RuntimeError("Refiner: jvp after close()")
        if self._epoch == 0:
            raise RuntimeError("Refiner: jvp before the first forward")
        with torch.cuda.device(self.device):
            t1, t2, ts, f64 = _tangent_rows("Refiner.jvp", (tan_disp1, tan_disp2, tan_sim), self.n_rows, self._idx, self.device)
            # (t1, t2, ts may be temporaries: they are read by work enqueued here, and torch reuses their memory in stream order)
            return self._batch.jvp(t1, t2, ts, f64=f64, **_hessian_flags(self._hessian)).detach()

    def evaluate(self, positions=None, **kw):
        """Batch.evaluate (lfr_batch_evaluate) on the shared batch: cost, dF/dx, raw residuals and loss weights at `positions`
        ([n_nodes, 2], None = the latest forward's), with the records of the latest forward - or of the constructor before the first.
        "residuals" and "weights" come back in the caller's rows: the rows of banned pairs read residual 0 and weight -1.  Every
        tensor is detached: F is not differentiated here, neither with respect to the positions (that is "grad") nor to the flows -
        objective() is the differentiable form."""
        if self._batch is None:
            raise RuntimeError("Refiner: evaluate after close()")
        with torch.cuda.device(self.device):
            out = self._batch.evaluate(None if positions is None else positions.detach().to(self.device), **kw)
            if self._idx is not None:
                for name, fill in (("residuals", 0.0), ("weights", -1.0)):
                    if name in out:
                        t = out[name]
                        full = torch.full((self.n_rows,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
                        full[self._idx] = t
                        out[name] = full
        return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}

    def hessian_product(self, vectors, positions=None, **kw):
        """Batch.hessian_product (lfr_batch_hessian_product) on the shared batch: H v of the objective's exact Hessian (or, with
        gauss_newton=True, its Gauss-Newton matrix) at `positions` ([n_nodes, 2], None = the latest forward's) for `vectors`
        ([K, n_nodes, 2] or [n_nodes, 2] float64), with the records of the latest forward - or of the constructor before the first.
        Everything is per node, so nothing is mapped to the caller's rows.  Every tensor is detached: this is no double backward."""
        if self._batch is None:
            raise RuntimeError("Refiner: hessian_product after close()")
        with torch.cuda.device(self.device):
            out = self._batch.hessian_product(vectors.detach() if isinstance(vectors, torch.Tensor) else vectors,
                                              positions.detach() if isinstance(positions, torch.Tensor) else positions, **kw)
        return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}

    def hessian_solve(self, rhs, positions=None, **kw):
        """Batch.hessian_solve (lfr_batch_hessian_solve) on the shared batch: (H + damping I) y = rhs per component by preconditioned
        conjugate gradients, H the matrix of hessian_product() at `positions` ([n_nodes, 2], None = the latest forward's) with the
        records of the latest forward - or of the constructor before the first.  Everything is per node, so nothing is mapped to the
        caller's rows.  Every tensor is detached: this is no double backward."""
        if self._batch is None:
            raise RuntimeError("Refiner: hessian_solve after close()")
        with torch.cuda.device(self.device):
            out = self._batch.hessian_solve(rhs.detach() if isinstance(rhs, torch.Tensor) else rhs,
                                            positions.detach() if isinstance(positions, torch.Tensor) else positions, **kw)
        return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}

    def objective(self, positions, disp1, disp2, sim=None, *, residuals=False, weights=False):
        """The objective of the latest forward as a differentiable function of (positions, disp1, disp2, sim): `cost` [n_components]
        float64 in the order of Batch.component_info - and, when asked for, `residuals` [rows, 2, 2] and `weights` [rows, 2] (float64,
        the caller's rows; banned pairs read residual 0 and weight -1) - returned as a dict.  The forward is Batch.evaluate at
        positions.detach(), the backward Batch.evaluate_vjp (lfr_batch_evaluate_vjp): the EXPLICIT partials.  With `positions` the
        output of the latest r(...), autograd adds them to J^T dL/dx from lfr_batch_backward: the gradient that reaches the flows is
        the total derivative.  The records are those of the latest forward, so disp1, disp2 and sim must be the very tensors the
        latest r(...) received (anything else: ValueError; a missing sim is None in both), and a backward after a later forward
        raises RuntimeError.  First order only."""
        if self._batch is None:
            raise RuntimeError("Refiner: objective after close()")
        if self._epoch == 0 or self._latest is None:
            raise RuntimeError("Refiner: objective before the first forward")
        for name, given, seen in zip(("disp1", "disp2", "sim"), (disp1, disp2, sim), self._latest):
            if given is not seen:
                raise ValueError("Refiner.objective: %s is not the tensor the latest forward received - the batch holds that forward's "
                                 "records, and the gradient would go to a tensor they were not made from" % name)
        if not isinstance(positions, torch.Tensor) or positions.numel() != 2 * self.n_nodes:
            raise ValueError("Refiner.objective: positions must be a [%d, 2] tensor" % self.n_nodes)
        out = _Objective.apply(positions, disp1, disp2, sim, self, bool(residuals), bool(weights))
        names = ("cost",) + (("residuals",) if residuals else ()) + (("weights",) if weights else ())
        return dict(zip(names, out))

    def close(self):
        self._latest = None
        for name in ("_batch", "_problem", "_graph"):
            h = getattr(self, name, None)
            if h is not None:
                h.close()
            setattr(self, name, None)
