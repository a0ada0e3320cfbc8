"""One step of the open-loop EVAL rollout on the engine (reference src/dynamics/rollout/rollout.py:108-260, the body of
`rollout_from_start_graph`'s loop): predict -> bounding planes from the prediction -> rule-based graph rebuild with the max_nR
back-off -> history shift (with `store_rest_state` the rest frame stays in slot 0) -> the next step's graph dictionary.

This closes SURVEY §8(f) rank 3: the single-graph builder, its tool rules and the back-off loop (graph.py) were there; this is
the step loop they live in.  What stays out, as in §8: the dataset side of rollout.py (ground-truth lookup, error bookkeeping,
visualisation) - the caller passes the tool keypoints of the next frame pair.

Everything numeric runs on the device: the model forward (ag_forward), the plane bounds (torch reductions; SIX scalars come back to
the host because the reference forms its thresholds from them as Python / numpy scalars, rollout.py:132-139, graph.py:134), the
edge builder and its tool rules (ag_build_edges_single, ag_edges_apply_tool_rule), the history shift.  The back-off's retry
decision (does the graph fit max_nR?) is one integer read per attempt, where the reference catches pad_torch's exception.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .context import current_stream
from .graph import EdgeList, BackoffPlan, attempt_with_backoff, construct_edges_with_backoff, rule_graphs_limit, surface_graphs_limit

_GRAPH_KEYS = ("attrs", "p_rigid", "p_instance", "obj_mask", "eef_mask", "state_mask", "material_index")   # rollout.py:242-248


def surface_bounds(obj_kp_vis, ratio):
    """rollout.py:132-139: the six plane bounds of the predicted object keypoints (N_fps, 3), written as the reference writes them
    on numpy float32 scalars (`np.max(...) * ratio` etc., so the products round as they do there under the installed numpy).
    obj_kp_vis may be a device tensor: max / min run where it lives and six floats are read back."""
    if isinstance(obj_kp_vis, torch.Tensor):
        ext = torch.stack([obj_kp_vis.amax(0), obj_kp_vis.amin(0)]).to(torch.float32).cpu().numpy()      # one read-back
    else:
        kp = np.asarray(obj_kp_vis, np.float32)
        ext = np.stack([kp.max(0), kp.min(0)])
    mx, mn = ext[0], ext[1]
    max_y = mx[1] * ratio
    min_y = mn[1]
    max_x = mx[0] * ratio
    max_z = mx[2] * ratio
    min_x = mn[0]
    min_x = (max_x - min_x) * (1 - ratio) + min_x
    min_z = mn[2]
    min_z = (max_z - min_z) * (1 - ratio) + min_z
    return dict(max_y=max_y, min_y=min_y, max_x=max_x, max_z=max_z, min_x=min_x, min_z=min_z)


@torch.no_grad()
def rollout_eval_step(model, graph, eef_kp_start, eef_kp_end, *, adj_thresh, topk, max_nR, connect_tool_all=False,
                      connect_tool_all_non_fixed=True, connect_tool_surface=False, connect_tool_surface_ratio=1.0,
                      knn_thresh=1.0, min_kNN=1.0, knn_increment=0.1, store_rest_state=False, dense=True, trail=None):
    """graph: the batched (B = 1) dictionary `model(**graph)` takes - 'state' (1,n_his,N+M,3), 'action' (1,N+M,3), 'attrs',
    'p_instance', 'obj_mask' (1,N) bool, 'eef_mask', 'state_mask' (1,N+M) bool, '<material>_physics_param', and the edges either
    as dense one-hot 'Rr' / 'Rs' (1,n_rel,N+M) like the reference or as 'edges' (an EdgeList).  eef_kp_start / eef_kp_end (M,3):
    the tool keypoints at the next frame pair (rollout.py:158-161).  The keyword arguments are the dataset config's entries
    rollout.py:27-51 reads.  Returns (new_graph, pred_state (1,N,3), pred_motion): new_graph holds 'Rr' / 'Rs' padded to max_nR
    (dense=True: what rollout.py:237-248 builds, so truncate_graph + model(**graph) run on it unchanged) or 'edges' (dense=False).
    trail (list): receives the back-off's (kNN, topk, n_rel) per attempt, first attempt included."""
    dev = graph["state"].device
    if "edges" in graph:
        fwd = {k: v for k, v in graph.items() if k not in ("Rr", "Rs")}
    else:
        fwd = graph
    pred_state, pred_motion = model(**fwd)                                                # rollout.py:112
    obj_mask = graph["obj_mask"][0].to(dev).to(torch.bool)
    obj_kp = pred_state[0][obj_mask]                                                      # :121, :127 (obj_kp_num = obj_mask.sum())
    bounds = surface_bounds(obj_kp, connect_tool_surface_ratio)                           # :132-139
    eef_start = torch.as_tensor(eef_kp_start, dtype=torch.float32).to(dev)
    eef_end = torch.as_tensor(eef_kp_end, dtype=torch.float32).to(dev)
    n_obj = pred_state.shape[1]
    states = torch.cat([pred_state[0], eef_start], 0).contiguous()                        # :163  (N+M, 3)
    states_delta = torch.zeros_like(states)
    states_delta[n_obj:n_obj + eef_start.shape[0]] = eef_end - eef_start                  # :165-166
    edges = construct_edges_with_backoff(states, adj_thresh, graph["state_mask"][0], graph["eef_mask"][0], topk, max_nR,
                                         knn_thresh=knn_thresh, min_kNN=min_kNN, knn_increment=knn_increment, as_index=not dense,
                                         trail=trail, connect_tools_all=connect_tool_all, connect_tools_surface=connect_tool_surface,
                                         connect_tool_all_non_fixed=connect_tool_all_non_fixed, **bounds)            # :168-222
    hist = graph["state"][0]
    if store_rest_state:                                                                  # :224-229 the rest frame stays
        hist = torch.cat([hist[:1], hist[2:], states[None]], 0)
    else:                                                                                 # :231-232
        hist = torch.cat([hist[1:], states[None]], 0)
    new_graph = {"state": hist[None].to(torch.float32), "action": states_delta[None].to(torch.float32)}
    if dense:
        new_graph["Rr"], new_graph["Rs"] = edges[0][None].to(torch.float32), edges[1][None].to(torch.float32)
    else:
        new_graph["edges"] = edges
    for k in _GRAPH_KEYS:
        if k in graph:
            new_graph[k] = graph[k]
    for k in graph:
        if k.endswith("_physics_param"):                                                  # :249-253
            new_graph[k] = graph[k]
    return new_graph, pred_state, pred_motion


@torch.no_grad()
def rollout_eval(model, graph, eef_pos, start_frame, n_steps, **cfg):
    """n_steps of rollout_eval_step along a tool trajectory eef_pos (T, M, 3): step i uses the frame pair (start_frame + i - 1,
    start_frame + i) the way rollout.py:158-161 looks it up from the next pair (n_future = 1).  -> (final graph, [pred_state (N,3)
    per step], [back-off trail per step]).  The predictions stay on the device; nothing but the step's own decisions is read back."""
    preds, trails = [], []
    for i in range(1, n_steps + 1):
        tr = []
        graph, pred, _ = rollout_eval_step(model, graph, eef_pos[start_frame + i - 1], eef_pos[start_frame + i], trail=tr, **cfg)
        preds.append(pred[0])
        trails.append(tr)
    return graph, preds, trails


# ================================================================================================ batched eval rollout
def eval_schedule(frames, first, n_his, n_frames, rollout_steps=100):
    """The frame pairs one open-loop rollout visits: what rollout_from_start_graph records in idx_list (rollout.py:105, 152-160).
    frames: the (P, n_his + n_future) frame table of ONE episode as dataset.frame_table returns it - with store_rest_state and
    short pairs the rest frame is already in front, so the reference's n_his - 1 column shift (rollout/graph.py:675-676) is
    "always columns n_his - 1 and n_his"; first: the row the rollout starts from; n_frames: frames of the episode.
    -> [(start_0, end_0), ..., (start_{L-1}, end_{L-1})]: (start_0, end_0) = (first[n_his-1], first[n_his]); after prediction i
    the next pair is the MIDDLE one of the rows with column n_his-1 == end_i and column n_his > end_i
    (get_next_pair_or_break_episode_pushes, rollout/graph.py:672-687); the rollout ends when there is none or after
    rollout_steps predictions.  L = len(result) predictions; prediction i is compared with frame end_i.  Pure host function."""
    frames = np.asarray(frames, np.int64)
    first = np.asarray(first, np.int64).reshape(-1)
    if frames.ndim != 2 or frames.shape[1] <= n_his or first.shape[0] != frames.shape[1]:
        raise ValueError(f"eval_schedule: frames {frames.shape}, first {first.shape}, n_his {n_his}")
    if frames.min() < 0 or frames.max() >= n_frames or first.min() < 0 or first.max() >= n_frames:
        raise ValueError(f"eval_schedule: a frame outside [0, {n_frames})")
    a, b = frames[:, n_his - 1], frames[:, n_his]
    out = [(int(first[n_his - 1]), int(first[n_his]))]
    while len(out) < rollout_steps:
        end = out[-1][1]
        valid = np.nonzero((a == end) & (b > end))[0]
        if len(valid) == 0:
            break
        row = frames[valid[int(len(valid) / 2)]]                                          # pick the middle one
        out.append((int(row[n_his - 1]), int(row[n_his])))
    return out[:max(0, int(rollout_steps))]


@dataclass
class EvalResult:
    """What rollout_eval_batch returns, rollout by rollout in the caller's order."""
    errors: torch.Tensor          # (L_max, B) float32 on the device; NaN behind each rollout's length
    lengths: np.ndarray           # (B,) predictions per rollout
    schedule: list                # per rollout: [(start_i, end_i)] (eval_schedule)
    trails: list                  # per rollout, per step: the back-off's [(kNN, topk, n_rel)] of the graph prediction i ran on
    pred: torch.Tensor | None = None   # (L_max, B, max_nobj, 3) with keep_pred; NaN behind each rollout's length
    edges: list | None = None     # with keep_pred: per step an EdgeList over the B graphs prediction i ran on (ended: 0 edges)
    host_waits: int = 0           # read-backs of the step loop: one per step (the counts; after the last step the status word)
                                  # plus one per back-off round.  The start batch's own waits are DeviceDynDataset.batch's.

    def step_error(self):
        """rollout.py:439-444: the (min_step, B) float64 matrix of the steps every rollout reached (what error_short.txt holds)."""
        min_step = int(np.min(self.lengths)) if len(self.lengths) else 0
        return self.errors[:min_step].cpu().numpy().astype(np.float64)

    def summary(self):
        """rollout.py:451-453: per step the median, the 25th and the 75th percentile over the rollouts."""
        e = self.step_error()
        return dict(median=np.median(e, axis=1), p25=np.percentile(e, 25, axis=1), p75=np.percentile(e, 75, axis=1))


def _eval_step_args(ds, B, topk, edge_cap):
    sp = ds.spec
    a = _lib.AgEvalStepArgs()
    a.d_obj_pos, a.d_eef_pos = ds._obj.data_ptr(), ds._eef.data_ptr()
    a.obj_points, a.eef_points = ds._obj.shape[0], ds._eef.shape[0] - 1                  # (the tool buffer ends with a spare row)
    a.B, a.max_nobj, a.n_eef, a.n_inst, a.edge_cap, a.edge_rows = B, sp.max_nobj, ds.n_eef, 1, edge_cap, max(1, sp.max_nR)
    a.topk, a.connect_tools_all, a.store_rest_state = int(topk), int(sp.connect_tool_all), int(sp.store_rest_state)
    return a


def eval_error(ds, engine, pred, fps_idx, n_obj, gt_first):
    """The error half of ag_eval_step alone (pred_given): pred (B, max_nobj, 3) against the frames whose first object points are
    gt_first (B,) int64 -> (B,) float32 on the device.  Enqueue only.  The engine must be one of the model's n_his."""
    dev = pred.device
    B, N = pred.shape[0], ds.N
    tab = torch.stack([gt_first.to(dev), torch.full_like(gt_first, -1, device=dev), torch.zeros_like(gt_first, device=dev)], 1).contiguous()
    err = torch.empty((B,), dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    mask = torch.zeros((B, N), dtype=torch.uint8, device=dev)
    thr = torch.zeros((B,), dtype=torch.float32, device=dev)
    scratch = (torch.empty((B, 1), **i32), torch.empty((B, 1), **i32), torch.empty((B, N + 1), **i32), torch.empty((B,), **i32))
    status = torch.zeros(4, **i32)
    a = _eval_step_args(ds, B, 1, 1)
    pred = pred.contiguous()
    # (every graph "ended": no state is read and none written; the builder sees B empty graphs over a zero frame)
    nxt = torch.zeros((B, ds.spec.n_his, N, 3), dtype=torch.float32, device=dev)
    a.d_state, a.d_state_next, a.d_action_next = pred.data_ptr(), nxt.data_ptr(), thr.data_ptr()
    a.d_fps_idx, a.d_n_obj, a.d_frames = fps_idx.data_ptr(), n_obj.data_ptr(), tab.data_ptr()
    a.d_state_mask, a.d_eef_mask, a.d_thr2, a.d_cull = mask.data_ptr(), mask.data_ptr(), thr.data_ptr(), thr.data_ptr()
    a.pred_given, a.step, a.err_stride = 1, 0, B
    a.d_pred, a.d_err, a.d_status = pred.data_ptr(), err.data_ptr(), status.data_ptr()
    a.d_recv_next, a.d_send_next, a.d_row_ptr_next, a.d_n_edges_next = (t.data_ptr() for t in scratch)
    engine.check(engine.lib.ag_eval_step(engine.ctx, current_stream(dev), C.byref(a)))
    return err


def _take(dr, order):
    """BatchDraws rows in another order."""
    o = torch.from_numpy(np.asarray(order)).to(dr.fps_start.device)
    return type(dr)(*[None if t is None else t[o].contiguous() for t in
                      (dr.fps_start, dr.fps_radius, dr.rad_start, dr.phys_noise, dr.state_noise, dr.rot, dr.adj_thresh, dr.knn_thresh)])


@torch.no_grad()
def rollout_eval_batch(model, ds, idx, rollout_steps=100, draws=None, keep_pred=False, per_graph=False):
    """The reference's eval script (src/dynamics/rollout/rollout.py: rollout_dataset -> rollout_episode_pushes ->
    rollout_from_start_graph) for B rollouts that advance together.  ds: a DeviceDynDataset (any phase); idx: the pair indices
    the rollouts start from.  Start graphs: ds.batch(idx, draws or ds.eval_draws(idx), with_fps=True), their own back-off
    included (rollout/graph.py:513-543); schedules: eval_schedule per rollout over the pair rows of its own episode.

    The rollouts are sorted by length internally, so the live ones are a prefix and step s launches on B_s rows; everything is
    returned in the caller's order.  Per step: ONE ag_eval_step (forward, error against the ground-truth frame, next model
    input, next graphs at top-k into the other half of a double-buffered edge pair), ONE read-back of the counts of the graphs
    that go on, the sub-batch back-off at top-k - 1, ... for those over max_nR (Exception("Exceeds max dims") at top-k < 1), the
    swap.  A graph beyond max_nR never reaches a forward; the status word ag_eval_step raises if one did is checked at the end.

    Configs with the non-fixed rule and / or a kNN range take the same loop (_eval_batched): after ag_eval_step the rule launch
    ag_edges_nonfixed_rule_graphs, fed from d_state_next, and the back-off in rounds (host_waits = steps + extra rounds).
    Configs with connect_tool_surface chain ag_edges_surface_rule_graphs behind (or in place of) the non-fixed rule, and their
    START graphs get the eval script's own rule: both tool rules with construct_graph's six bounds from
    the padded rows of frame n_his - 1 (rollout/graph.py:446-458, 508-512) - ds.batch as the public calls it follows the training
    path, which never fires the surface rule.  Configs beyond the rule kernels' size limits, or per_graph=True, take the same start
    batch through rollout_eval_step graph by graph, the error from the same kernel at B = 1: correct and slow (several waits per
    step and graph).  keep_pred: also return every prediction and every step's edge lists.  keep_prev_fps and hetero of the reference's
    script are out of scope: every start pair samples its own points, the physics parameter is the episode's."""
    sp, dev = ds.spec, ds.device
    idx = np.asarray(idx, np.int64).reshape(-1)
    B = len(idx)
    if B < 1 or idx.min() < 0 or idx.max() >= len(ds):
        raise IndexError(f"rollout indices outside [0, {len(ds)})")
    scheds = []
    for i in idx:
        ep = int(ds._episode[i])
        scheds.append(eval_schedule(ds._frames[ds._episode == ep], ds._frames[i], sp.n_his, int(ds._t_e[ep]), rollout_steps))
    lengths = np.array([len(s) for s in scheds], np.int64)
    L_max = int(lengths.max())
    if L_max < 1:
        raise ValueError("rollout_eval_batch: rollout_steps < 1")
    order = np.argsort(-lengths, kind="stable")                                          # sorted position -> caller's position
    dr = draws if draws is not None else ds.eval_draws(idx)
    data = ds.batch(idx[order], _take(dr, order), with_fps=True, _eval_start=True)       # (raises before any step if a start graph cannot fit)
    aux = ds._last_build
    eng = model.engine(dev)
    N, No = ds.N, sp.max_nobj
    kw = {k: v for k, v in data.items() if k.endswith("_physics_param")}
    inp = model._inputs(dev, data["state"], data["attrs"], None, None, data["p_instance"], data["action"], data["edges"], kw)
    f32 = dict(dtype=torch.float32, device=dev)
    errors = torch.full((L_max, B), float("nan"), **f32)
    pred = torch.full((L_max if keep_pred else 1, B, No, 3), float("nan"), **f32)
    kept = [] if keep_pred else None
    trails = [[list(t)] for t in ds.last_trail]                                          # sorted order; step 0: the start graph's
    # per-step frame table (L_max, B, 3), uploaded once
    ep_s = ds._episode[idx[order]]
    tab = np.zeros((L_max, B, 3), np.int64)
    tab[:, :, 1] = -1
    for j, r in enumerate(order):
        sch, e = scheds[r], int(ep_s[j])
        for i, (_, end) in enumerate(sch):
            tab[i, j, 0] = ds._obj_off[e] + end * ds._n_e[e]
            if i + 1 < len(sch):
                tab[i, j, 1] = ds._eef_off[e] + sch[i + 1][0] * ds.n_eef
                tab[i, j, 2] = ds._eef_off[e] + sch[i + 1][1] * ds.n_eef
    waits = [0]
    # connect_tool_surface can fire in the eval rollout: all six bounds are passed on (rollout.py:168-222)
    limit = (sp.connect_tool_all_non_fixed and rule_graphs_limit(N, ds.n_eef)) or (sp.connect_tool_surface and surface_graphs_limit(N, ds.n_eef))
    if per_graph or limit:
        _eval_per_graph(model, ds, eng, data, aux, dr, order, scheds, tab, errors, pred, kept, trails, keep_pred)
    else:
        _eval_batched(ds, eng, data, aux, inp, lengths[order], tab, errors, pred, kept, trails, keep_pred, waits)
    # ---- back to the caller's order
    o = torch.from_numpy(order).to(dev)
    out_err = torch.empty_like(errors)
    out_err[:, o] = errors
    out_pred = out_edges = None
    if keep_pred:
        out_pred = torch.empty_like(pred)
        out_pred[:, o] = pred
        out_edges = []
        for e in kept:
            t = [torch.empty_like(x) for x in (e.recv, e.send, e.row_ptr, e.n_edges)]
            for dst, src in zip(t, (e.recv, e.send, e.row_ptr, e.n_edges)):
                dst[o] = src
            out_edges.append(EdgeList(*t, N))
    out_trails = [None] * B
    for j, r in enumerate(order):
        out_trails[r] = trails[j]
    return EvalResult(out_err, lengths, scheds, out_trails, out_pred, out_edges, waits[0])


def _eval_batched(ds, eng, data, aux, inp, len_s, tab, errors, pred, kept, trails, keep_pred, waits):
    """rollout_eval_batch's step loop, for every config that advances together.
    Per step: ag_eval_step - it writes the BASE next graphs at top-k into the second edge buffer -, then
    graph.attempt_with_backoff on the graphs that go on: ag_edges_nonfixed_rule_graphs and / or ag_edges_surface_rule_graphs
    (chained when the config has both, the step loop's bound order), fed from d_state_next (bounds: the predicted rows of its last
    frame, pad_rows 0, rollout.py:125-139; kNN: the start graph's draw, the config's midpoint), back into the first edge buffer,
    which the next step's forward reads; one read-back of their counts, then graph.BackoffPlan's rounds on those over max_nR.
    With a rule both edge buffers are max(max_nR, structural bound) wide - the rule can remove edges, so its input may exceed
    max_nR - and ag_eval_step is told edge_rows = max_nR.  A config with neither rule keeps the max_nR-wide double buffer: no
    launch follows the step, the base graphs are the next step's graphs and the two buffers swap roles."""
    sp, dev, N, nh = ds.spec, ds.device, ds.N, ds.spec.n_his
    attrs, action, phys, group, edges = inp.attrs, inp.action, inp.phys, inp.group, inp.edges
    L_max, B = errors.shape
    rule, cap = sp.connect_tool_all_non_fixed, max(1, sp.max_nR)
    cfg = ds._rule_config(sp.connect_tool_surface, 0)
    ruled = rule or cfg.surface                                                          # a launch follows ag_eval_step
    k = min(N, sp.topk)
    ecap = max(cap, N * (k + ds.n_eef) if k < N else N * N) if ruled else cap
    i32 = dict(dtype=torch.int32, device=dev)
    el = [EdgeList(torch.zeros((B, ecap), **i32), torch.zeros((B, ecap), **i32), edges.row_ptr.clone(), edges.n_edges.clone(), N),
          EdgeList(torch.zeros((B, ecap), **i32), torch.zeros((B, ecap), **i32), torch.zeros_like(edges.row_ptr),
                   torch.zeros_like(edges.n_edges), N)]
    el[0].recv[:, :cap], el[0].send[:, :cap] = edges.recv, edges.send
    knn_host = [t[0][0][0] for t in trails]                                              # the start graphs' own kNN draws
    if ruled:
        knn_dev = torch.tensor(knn_host, dtype=torch.float64).to(dev)
        first = torch.arange(B, dtype=torch.int64, device=dev) * (nh * N) + (nh - 1) * N # last frame of d_state_next, in points
    view = (lambda e, n: EdgeList(e.recv[:n], e.send[:n], e.row_ptr[:n], e.n_edges[:n], N))
    tab_d = torch.from_numpy(tab).to(dev)
    status = torch.zeros(4, **i32)
    state = [data["state"], data["state"].clone()]
    act = [action, action.clone()]
    cur = ec = 0                                                                          # state / action half, edge buffer read
    for s in range(L_max):
        Bs, Bn = int((len_s > s).sum()), int((len_s > s + 1).sum())
        nxt, en = 1 - cur, 1 - ec
        if keep_pred:
            kept.append(EdgeList(el[ec].recv[:, :cap].clone(), el[ec].send[:, :cap].clone(), el[ec].row_ptr.clone(), el[ec].n_edges.clone(), N))
            kept[-1].n_edges[Bs:] = 0
        a = _eval_step_args(ds, Bs, sp.topk, ecap)
        a.d_state, a.d_action, a.d_attrs, a.d_phys, a.d_group = (t.data_ptr() for t in (state[cur], act[cur], attrs, phys, group))
        a.d_recv, a.d_send, a.d_row_ptr, a.d_n_edges = (t.data_ptr() for t in (el[ec].recv, el[ec].send, el[ec].row_ptr, el[ec].n_edges))
        a.d_fps_idx, a.d_n_obj, a.d_frames = data["fps_idx"].data_ptr(), data["n_obj"].data_ptr(), tab_d[s].data_ptr()
        a.d_state_mask, a.d_eef_mask = aux["state_mask"].data_ptr(), aux["eef_mask"].data_ptr()
        a.d_thr2, a.d_cull = aux["thr2"].data_ptr(), aux["cull"].data_ptr()
        a.pred_given, a.step, a.err_stride = 0, s, B
        a.d_pred, a.d_err = pred[s if keep_pred else 0].data_ptr(), errors.data_ptr()
        a.d_state_next, a.d_action_next = state[nxt].data_ptr(), act[nxt].data_ptr()
        a.d_recv_next, a.d_send_next, a.d_row_ptr_next, a.d_n_edges_next = (
            t.data_ptr() for t in (el[en].recv, el[en].send, el[en].row_ptr, el[en].n_edges))
        a.d_status = status.data_ptr()
        eng.check(eng.lib.ag_eval_step(eng.ctx, current_stream(dev), C.byref(a)))
        if Bn > 0:
            knn = bnd = out = None
            if ruled:                                                                     # (the forward that read el[ec] is ahead of the
                knn, out = knn_dev[:Bn], view(el[ec], Bn)                                 # rule on the stream: its buffer is free)
                bnd = (state[nxt].view(-1, 3), first[:Bn], None, data["n_obj"][:Bn], 0)
            plan = BackoffPlan(knn_host[:Bn], sp.topk, sp.max_nR, sp.min_kNN, sp.knn_increment, has_rule=rule)
            attempt_with_backoff(cfg, plan, state[nxt].data_ptr() + (nh - 1) * N * 3 * 4, nh * N * 3, view(el[en], Bn), knn,
                                 state[nxt][:Bn, -1], aux["state_mask"][:Bn], aux["eef_mask"][:Bn], aux["thr2"][:Bn], aux["cull"][:Bn],
                                 bnd, ecap, out=out)                                      # the step's one wait, and one per round
            waits[0] += plan.rounds
            for j in range(Bn):
                trails[j].append(plan.trail[j])
            if not ruled:
                ec = en
        cur = nxt
    seen = int(status[:1].cpu()[0])                                                      # the last step's wait: the status word
    waits[0] += 1
    if seen > 0:
        raise Exception("Exceeds max dims")


def _eval_per_graph(model, ds, eng, data, aux, dr, order, scheds, tab, errors, pred, kept, trails, keep_pred):
    """rollout_eval_batch's graph-by-graph path: rollout_eval_step per step and graph on the rows of the same start batch, the
    error from ag_eval_step's kernel at B = 1.  Fills errors / pred / kept / trails in the sorted order."""
    sp, dev, N, No = ds.spec, ds.device, ds.N, ds.spec.max_nobj
    L_max, B = errors.shape
    adj = dr.adj_thresh.cpu().numpy()[order]
    knn = dr.knn_thresh.cpu().numpy()[order]
    tab_d = torch.from_numpy(tab).to(dev)
    cfg = dict(topk=sp.topk, max_nR=sp.max_nR, connect_tool_all=sp.connect_tool_all, connect_tool_all_non_fixed=sp.connect_tool_all_non_fixed,
               connect_tool_surface=sp.connect_tool_surface, connect_tool_surface_ratio=sp.connect_tool_surface_ratio,
               min_kNN=sp.min_kNN, knn_increment=sp.knn_increment, store_rest_state=sp.store_rest_state, dense=False)
    if keep_pred:
        for s in range(L_max):
            i32 = dict(dtype=torch.int32, device=dev)
            kept.append(EdgeList(torch.zeros((B, max(1, sp.max_nR)), **i32), torch.zeros((B, max(1, sp.max_nR)), **i32),
                                 torch.zeros((B, N + 1), **i32), torch.zeros((B,), **i32), N))
    e0 = data["edges"]
    for j, r in enumerate(order):
        sl = slice(j, j + 1)
        graph = {k: data[k][sl] for k in ("state", "action", "attrs", "p_rigid", "p_instance", "obj_mask", "material_index")}
        graph["state_mask"], graph["eef_mask"] = aux["state_mask"][sl].view(torch.bool), aux["eef_mask"][sl].view(torch.bool)
        for k in data:
            if k.endswith("_physics_param"):
                graph[k] = data[k][sl]
        graph["edges"] = EdgeList(e0.recv[sl].contiguous(), e0.send[sl].contiguous(), e0.row_ptr[sl].contiguous(), e0.n_edges[sl].contiguous(), N)
        L = len(scheds[r])
        for i in range(L):
            if keep_pred:
                g, n = graph["edges"], int(graph["edges"].n_edges[0])
                kept[i].recv[j, :n], kept[i].send[j, :n] = g.recv[0, :n], g.send[0, :n]
                kept[i].row_ptr[j], kept[i].n_edges[j] = g.row_ptr[0], n
            if i + 1 < L:
                es, ee = int(tab[i, j, 1]), int(tab[i, j, 2])
                tr = []
                graph, p, _ = rollout_eval_step(model, graph, ds._eef[es:es + ds.n_eef], ds._eef[ee:ee + ds.n_eef], adj_thresh=float(adj[j]),
                                                knn_thresh=float(knn[j]), trail=tr, **cfg)
                trails[j].append([tuple(t) for t in tr])
            else:
                p, _ = model(**graph)
            if keep_pred:
                pred[i, j] = p[0]
            errors[i, j:j + 1] = eval_error(ds, eng, p, data["fps_idx"][sl], data["n_obj"][sl], tab_d[i, j:j + 1, 0])
