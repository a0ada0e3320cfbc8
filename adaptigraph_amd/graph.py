"""Graph construction on the GPU.  Mirrors reference src/dynamics/dataset/graph.py:233-298
(construct_edges_from_states_batch) and src/dynamics/utils.py:49-69,150-160 (pad_torch, truncate_graph).

The native representation is an index-list graph (EdgeList: recv/send/row_ptr, CSR by receiver).  The dense one-hot
(Rr, Rs) pair the reference returns is produced on request for callers that still want it.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .context import default_engine, ptr, current_stream, _require_gpu


@dataclass
class EdgeList:
    """Edges of a batch of graphs, per batch element sorted by (receiver, sender) = the reference's nonzero order."""
    recv: torch.Tensor      # (B, edge_cap) int32
    send: torch.Tensor      # (B, edge_cap) int32
    row_ptr: torch.Tensor   # (B, N+1) int32 CSR offsets by receiver
    n_edges: torch.Tensor   # (B,) int32
    N: int

    @property
    def edge_cap(self):
        return self.recv.shape[1]

    def to_dense(self, n_rel=None):
        """(Rr, Rs) exactly as graph.py:288-298 builds them: (B, max_b n_edges, N) one-hot fp32, zero-padded rows."""
        B = self.recv.shape[0]
        n_rel = int(self.n_edges.max().item()) if n_rel is None else n_rel
        dev = self.recv.device
        Rr = torch.zeros((B, n_rel, self.N), device=dev, dtype=torch.float32)
        Rs = torch.zeros((B, n_rel, self.N), device=dev, dtype=torch.float32)
        e = torch.arange(n_rel, device=dev)[None, :].expand(B, n_rel)
        valid = e < self.n_edges[:, None]
        b_idx = torch.arange(B, device=dev)[:, None].expand(B, n_rel)[valid]
        e_idx = e[valid]
        Rr[b_idx, e_idx, self.recv[:, :n_rel][valid].long()] = 1
        Rs[b_idx, e_idx, self.send[:, :n_rel][valid].long()] = 1
        return Rr, Rs

    @staticmethod
    def from_dense(Rr, Rs):
        """Dense one-hot (B,E,N) -> index lists.  Zero rows are padding (the convention of pad_torch/truncate_graph and
        of the reference's viz, src/dynamics/rollout/graph.py:215-217).  Rows are re-sorted by receiver (stable) when
        the caller's order is not CSR; this only changes the summation order of the scatter (model.py:324)."""
        B, E, N = Rr.shape
        valid = Rr.sum(-1) > 0
        recv = Rr.argmax(-1).to(torch.int32)
        send = Rs.argmax(-1).to(torch.int32)
        key = torch.where(valid, recv.long(), torch.full_like(recv, N, dtype=torch.long))
        order = torch.argsort(key, dim=1, stable=True)
        recv = torch.gather(recv, 1, order).contiguous()
        send = torch.gather(send, 1, order).contiguous()
        n_edges = valid.sum(1).to(torch.int32)
        key_sorted = torch.gather(key, 1, order)
        counts = torch.zeros((B, N + 1), device=Rr.device, dtype=torch.long)
        counts.scatter_add_(1, key_sorted, torch.ones_like(key_sorted))
        row_ptr = torch.zeros((B, N + 1), device=Rr.device, dtype=torch.int32)
        row_ptr[:, 1:] = torch.cumsum(counts[:, :N], 1).to(torch.int32)
        if E == 0:
            recv = torch.zeros((B, 1), device=Rr.device, dtype=torch.int32)
            send = torch.zeros((B, 1), device=Rr.device, dtype=torch.int32)
        return EdgeList(recv, send, row_ptr.contiguous(), n_edges.contiguous(), N)


def construct_edges_index(states, adj_thresh, mask, tool_mask, topk=10, connect_tools_all=False, edge_cap=None,
                          engine=None):
    """Index-list form of construct_edges_from_states_batch.  Same arguments as graph.py:233; returns EdgeList.

    edge_cap: capacity per batch element (default: the structural bound N*(min(topk,N)+M)).  If a graph has more edges
    than edge_cap nothing is written for it and n_edges still reports the true count.
    """
    dev = _require_gpu(states.device)
    eng = engine or default_engine(dev)
    states = states.to(torch.float32).contiguous()
    B, N, sd = states.shape
    assert sd == 3, "state_dim must be 3"
    mask_u8 = mask.to(torch.bool).contiguous().view(torch.uint8)
    tool_u8 = tool_mask.to(torch.bool).contiguous().view(torch.uint8)
    thr_vec = None
    if isinstance(adj_thresh, torch.Tensor):
        thr_vec = adj_thresh.to(device=dev, dtype=torch.float32).contiguous()
        assert thr_vec.numel() == B
        thr = 0.0
    else:
        thr = float(adj_thresh)
    if edge_cap is None:
        k = min(N, int(topk))
        m = int(tool_mask.to(torch.bool).sum(1).max().item())
        edge_cap = N * (k + m) if k < N else N * N
    edge_cap = max(1, int(edge_cap))
    recv = torch.empty((B, edge_cap), device=dev, dtype=torch.int32)
    send = torch.empty((B, edge_cap), device=dev, dtype=torch.int32)
    row_ptr = torch.empty((B, N + 1), device=dev, dtype=torch.int32)
    n_edges = torch.empty((B,), device=dev, dtype=torch.int32)
    eng.check(eng.lib.ag_build_edges(eng.ctx, current_stream(dev), ptr(states), ptr(mask_u8), ptr(tool_u8), B, N, thr,
                                     ptr(thr_vec), int(topk), int(bool(connect_tools_all)), edge_cap, ptr(recv),
                                     ptr(send), ptr(row_ptr), ptr(n_edges)))
    return EdgeList(recv, send, row_ptr, n_edges, N)


CELLS_MAX_PARTICLES = 1 << 20   # ag_build_edges_cells (csrc/ag_cells.h)
CELLS_MAX_TOPK = 128


def construct_edges_cells(states, adj_thresh, mask, tool_mask, topk=10, connect_tools_all=False, edge_cap=None, single=False,
                          engine=None):
    """construct_edges_index from the cell-list builder (ag_build_edges_cells): the same EdgeList bit for bit, for graphs of up
    to CELLS_MAX_PARTICLES particles and 1 <= topk <= CELLS_MAX_TOPK (NotImplementedError beyond, and for an edge_cap that does
    not fit int32).  single: the single-graph builder's rule for every graph of the batch - the threshold squared in double and
    then rounded, as construct_edges_from_states squares it, connect_tools_all unconditional and without tool<->tool edges.
    Enqueue only; n_edges[b] is the TRUE count even above edge_cap, and then nothing else is written for graph b."""
    dev = _require_gpu(states.device)
    eng = engine or default_engine(dev)
    states = states.to(torch.float32).contiguous()
    B, N, sd = states.shape
    assert sd == 3, "state_dim must be 3"
    mask_u8 = mask.to(torch.bool).contiguous().view(torch.uint8)
    tool_u8 = tool_mask.to(torch.bool).contiguous().view(torch.uint8)
    thr, thr_vec, thr2_vec = 0.0, None, None
    if isinstance(adj_thresh, torch.Tensor):
        assert adj_thresh.numel() == B
        if single:
            thr2_vec = (adj_thresh.to(device=dev, dtype=torch.float64) ** 2).to(torch.float32).contiguous()
        else:
            thr_vec = adj_thresh.to(device=dev, dtype=torch.float32).contiguous()
    elif single:
        t = float(adj_thresh)
        thr2_vec = torch.full((B,), float(np.float32(t * t)), device=dev, dtype=torch.float32)   # double product, one fp32 rounding
    else:
        thr = float(adj_thresh)
    if edge_cap is None:
        k = min(N, int(topk))
        m = int(tool_mask.to(torch.bool).sum(1).max().item())
        edge_cap = N * (k + m) if k < N else N * N
    edge_cap = max(1, int(edge_cap))
    if edge_cap > 2 ** 31 - 1:
        raise NotImplementedError(f"construct_edges_cells: edge_cap={edge_cap} does not fit the int32 edge offsets (at most {2 ** 31 - 1})")
    recv = torch.empty((B, edge_cap), device=dev, dtype=torch.int32)
    send = torch.empty((B, edge_cap), device=dev, dtype=torch.int32)
    row_ptr = torch.empty((B, N + 1), device=dev, dtype=torch.int32)
    n_edges = torch.empty((B,), device=dev, dtype=torch.int32)
    rule = (2 if single else 1) if connect_tools_all else 0
    eng.check(_lib.load_cells().ag_build_edges_cells(eng.ctx, current_stream(dev), ptr(states), 0, ptr(mask_u8), ptr(tool_u8), B, N, thr,
                                                     ptr(thr_vec), ptr(thr2_vec), int(topk), rule, edge_cap, ptr(recv), ptr(send),
                                                     ptr(row_ptr), ptr(n_edges)))
    return EdgeList(recv, send, row_ptr, n_edges, N)


def construct_edges_from_states_batch(states, adj_thresh, mask, tool_mask, topk=10, connect_tools_all=False):
    """Drop-in for graph.py:233-298: returns dense one-hot (Rr, Rs) of shape (B, n_rel, N)."""
    el = construct_edges_index(states, adj_thresh, mask, tool_mask, topk, connect_tools_all)
    if int((el.n_edges > el.edge_cap).any().item()):
        raise RuntimeError("internal: structural edge bound exceeded")
    return el.to_dense()


_PLANES = ["max_y", "min_x", "max_x", "min_z", "max_z"]            # graph.py:38 order


def _plane_side(name, pos, max_y, max_x, max_z, min_x, min_z):
    """graph.py:45-66 on particle vectors: which particles lie beyond the named bounding plane (torch's own
    tensor-vs-scalar comparison, so the scalar is rounded exactly as in the reference)."""
    if name == "max_y":
        return pos[:, 1] >= max_y
    if name == "max_x":
        return pos[:, 0] >= max_x
    if name == "max_z":
        return pos[:, 2] >= max_z
    if name == "min_x":
        return pos[:, 0] <= min_x
    if name == "min_z":
        return pos[:, 2] <= min_z
    raise Exception("Unknown plane for connecting tool to surface object particles!!")


def _apply_tool_rule(eng, dev, el, pos, mask_u8, tool_u8, n_tools, subset, kNN):
    """ag_edges_apply_tool_rule on a single-graph EdgeList -> new EdgeList."""
    N = el.N
    edge_cap = max(1, min(el.edge_cap, N * N) + N * n_tools)                # every rule adds at most N*M tool edges (no read-back)
    recv = torch.empty((1, edge_cap), device=dev, dtype=torch.int32)
    send = torch.empty((1, edge_cap), device=dev, dtype=torch.int32)
    row_ptr = torch.empty((1, N + 1), device=dev, dtype=torch.int32)
    n_edges = torch.empty((1,), device=dev, dtype=torch.int32)
    sub_u8 = subset.to(dev).to(torch.bool).contiguous().view(torch.uint8)
    eng.check(eng.lib.ag_edges_apply_tool_rule(eng.ctx, current_stream(dev), ptr(pos), ptr(mask_u8), ptr(tool_u8), N, n_tools,
                                               ptr(el.send), ptr(el.row_ptr), ptr(sub_u8), float(kNN), edge_cap, ptr(recv),
                                               ptr(send), ptr(row_ptr), ptr(n_edges)))
    return EdgeList(recv, send, row_ptr, n_edges, N)        # (n_edges < 0 = tool count mismatch: checked where n_edges is next read)


def _tool_sender_edges(el, tool_b):
    """adj[obj_tool_mask_2].sum() (graph.py:128-129, :178-179): edges whose sender is a tool particle.  (Receivers of
    edges are valid particles by construction, which is the other half of obj_tool_mask_2.)"""
    live = torch.arange(el.edge_cap, device=el.send.device) < el.n_edges[0]          # one read-back instead of two
    return int((tool_b[el.send[0].clamp(0, el.N - 1).long()] & live).sum().item())


def construct_edges_from_states(states, adj_thresh, mask, tool_mask, topk=10, connect_tools_all=False, max_y=None,
                                min_y=None, max_x=None, max_z=None, min_x=None, min_z=None, connect_tools_surface=False,
                                connect_tool_all_non_fixed=True, kNN=1.0, as_index=False):
    """Drop-in for the single-graph builder (graph.py:68-231): states (N,3), mask/tool_mask (N,) -> dense one-hot
    (Rr, Rs) of shape (n_rel, N) (or an EdgeList with as_index=True).

    The radius / top-k / connect_tools_all part runs in ag_build_edges_single.  The two optional tool rules
    (graph.py:125-171 'tool to all non-fixed particles' with its flat kNN filter, :173-221 'tool to the two closest
    surface planes') are scalar decisions here - the same Python expressions as the reference, so thresholds round
    the same way - followed by ag_edges_apply_tool_rule on the device.  Like the reference this path synchronises
    (graph.py:129, :223)."""
    dev = _require_gpu(states.device)
    eng = default_engine(dev)
    pos = states.to(torch.float32).contiguous()
    N = pos.shape[0]
    thr = float(adj_thresh)
    thr2 = float(np.float32(thr * thr))                                     # double product, one fp32 rounding (:86,101)
    cull = float(np.nextafter(np.float32(abs(thr)), np.float32(np.inf)))    # cull^2 >= thr2 whatever the rounding did
    mask_b = mask.to(dev).to(torch.bool).contiguous()
    tool_b = tool_mask.to(dev).to(torch.bool).contiguous()
    mask_u8, tool_u8 = mask_b.view(torch.uint8), tool_b.view(torch.uint8)
    k = min(N, int(topk))
    m = int(tool_b.sum().item())
    edge_cap = max(1, N * (k + m) if k < N else N * N)
    recv = torch.empty((1, edge_cap), device=dev, dtype=torch.int32)
    send = torch.empty((1, edge_cap), device=dev, dtype=torch.int32)
    row_ptr = torch.empty((1, N + 1), device=dev, dtype=torch.int32)
    n_edges = torch.empty((1,), device=dev, dtype=torch.int32)
    eng.check(eng.lib.ag_build_edges_single(eng.ctx, current_stream(dev), ptr(pos), ptr(mask_u8), ptr(tool_u8), N, thr2,
                                            cull, int(topk), int(bool(connect_tools_all)), edge_cap, ptr(recv), ptr(send),
                                            ptr(row_ptr), ptr(n_edges)))
    el = EdgeList(recv, send, row_ptr, n_edges, N)

    if connect_tool_all_non_fixed and max_y is not None and min_y is not None:          # graph.py:125
        check = _tool_sender_edges(el, tool_b)                                          # :128-129
        threshold = (max_y - min_y) * 0.1 + min_y                                       # :134 bottom 10 % is fixed
        if check > 0:
            subset = (pos[:, 1] > threshold) & mask_b                                   # :138-143
            el = _apply_tool_rule(eng, dev, el, pos, mask_u8, tool_u8, m, subset, kNN)  # :144-170

    if connect_tools_surface and max_y is not None and max_x is not None and min_x is not None and max_z is not None \
            and min_z is not None:                                                      # graph.py:173
        check = _tool_sender_edges(el, tool_b)                                          # :178-179
        if check > 0:
            # :190-194 index s_receiv with the 0/1 VALUES of adj[obj_tool_mask_2]: each of its entries selects particle
            # 0 or particle 1, broadcast over N senders.  Reproduced as written: n0 zeros, n1 ones.
            n1 = check
            n0 = int(mask_b.sum().item()) * m - check
            p01 = pos[:2].cpu()
            def plane_dist(axis, bound):
                d = (p01[:, axis] - bound) ** 2                                         # fp32, like the reference
                return N * (n0 * float(d[0]) + n1 * float(d[min(1, N - 1)]))
            values = [plane_dist(1, max_y), plane_dist(0, min_x), plane_dist(0, max_x), plane_dist(2, min_z),
                      plane_dist(2, max_z)]                                             # :36-37
            order = np.argsort(values)                                                  # :39
            first, second = _PLANES[order[0]], _PLANES[order[1]]
            subset = _plane_side(first, pos, max_y, max_x, max_z, min_x, min_z) & \
                _plane_side(second, pos, max_y, max_x, max_z, min_x, min_z) & mask_b     # :197-207
            el = _apply_tool_rule(eng, dev, el, pos, mask_u8, tool_u8, m, subset, 1.0)  # :208-218

    if as_index:
        return el
    if int(el.n_edges[0].item()) < 0:
        raise RuntimeError("internal: tool count passed to ag_edges_apply_tool_rule does not match tool_mask")
    Rr, Rs = el.to_dense()
    return Rr[0], Rs[0]


def construct_edges_with_backoff(states, adj_thresh, mask, tool_mask, topk, max_nR, knn_thresh=1.0, min_kNN=1.0,
                                 knn_increment=0.1, as_index=False, trail=None, **rules):
    """The max_nR back-off loop the reference repeats around construct_edges_from_states (rollout.py:173-222,
    rollout/graph.py:508-543, dataset.py:310-350): if the graph does not fit max_nR, first shrink the tool's kNN
    fraction by knn_increment down to min_kNN, then lower top-k by one per attempt.  `rules` are the remaining keyword
    arguments of construct_edges_from_states (connect_tools_all, max_y, ...).  Returns (Rr, Rs) padded to max_nR, or with
    as_index the EdgeList of the graph that fitted (the fit test is then one integer read per attempt instead of the dense
    pad_torch).  trail (list): receives (kNN, topk, n_rel) of every attempt."""
    kNN = knn_thresh
    decrease_topK = topk
    k_now = topk
    while True:
        el = construct_edges_from_states(states, adj_thresh, mask, tool_mask, topk=k_now, kNN=kNN, as_index=True, **rules)
        n_rel = int(el.n_edges[0].item())
        if n_rel < 0:
            raise RuntimeError("internal: tool count passed to ag_edges_apply_tool_rule does not match tool_mask")
        if trail is not None:
            trail.append((float(kNN), int(k_now), n_rel))
        if n_rel <= max_nR:                                                             # rollout.py:192-194 pad_torch fits
            if as_index:
                return el
            Rr, Rs = el.to_dense(n_rel)
            return pad_torch(Rr[0], max_nR), pad_torch(Rs[0], max_nR)
        if kNN <= min_kNN:                                                              # rollout.py:199-211
            decrease_topK = decrease_topK - 1
            if decrease_topK < 1:
                raise Exception("Exceeds max dims")                                     # (the reference would loop on: utils.py:63-65)
            k_now = decrease_topK
        else:                                                                           # rollout.py:212-222
            kNN = kNN - knn_increment
            k_now = topk


def construct_edges_graphs(pos, pos_bstride, mask_u8, tool_u8, thr2, cull, topk, connect_tools_all=False, edge_cap=None, engine=None):
    """ag_build_edges_graphs: B independent graphs under the single-graph builder's rule in one launch -> EdgeList.  pos: a float32
    tensor (B, N, 3) or a device address with pos_bstride floats between graphs (0: N * 3); thr2 / cull (B,) float32: the squared
    threshold fp32(adj * adj in double) and a culling radius with cull^2 >= thr2; edge_cap defaults to the structural bound
    N * (min(topk, N) + tools).  Enqueue only; n_edges[b] is the TRUE count even above edge_cap."""
    dev = mask_u8.device
    eng = engine or default_engine(dev)
    B, N = mask_u8.shape
    if edge_cap is None:
        k = min(N, int(topk))
        edge_cap = N * (k + int(tool_u8[0].sum().item())) if k < N else N * N
    edge_cap = max(1, int(edge_cap))
    recv = torch.empty((B, edge_cap), device=dev, dtype=torch.int32)
    send = torch.empty((B, edge_cap), device=dev, dtype=torch.int32)
    row_ptr = torch.empty((B, N + 1), device=dev, dtype=torch.int32)
    n_edges = torch.empty((B,), device=dev, dtype=torch.int32)
    eng.check(eng.lib.ag_build_edges_graphs(eng.ctx, current_stream(dev), pos if isinstance(pos, int) else pos.data_ptr(),
                                            int(pos_bstride), ptr(mask_u8), ptr(tool_u8), B, N, ptr(thr2), ptr(cull), int(topk),
                                            int(bool(connect_tools_all)), edge_cap, ptr(recv), ptr(send), ptr(row_ptr), ptr(n_edges)))
    return EdgeList(recv, send, row_ptr, n_edges, N)


RULE_GRAPHS_MAX_PAIRS = 8192   # ag_edges_nonfixed_rule_graphs keeps a graph's (N, n_tools) pair tables in LDS
RULE_GRAPHS_MAX_TOOLS = 64


def rule_graphs_limit(N, n_tools):
    """None when ag_edges_nonfixed_rule_graphs takes graphs of N particles with n_tools tool points, else the limit in words."""
    if N > 4096:
        return f"N = {N} exceeds 4096"
    if n_tools > RULE_GRAPHS_MAX_TOOLS or N * n_tools > RULE_GRAPHS_MAX_PAIRS:
        return (f"N * n_tools = {N} * {n_tools} exceeds the LDS-resident pair tables (at most {RULE_GRAPHS_MAX_TOOLS} tool points and "
                f"{RULE_GRAPHS_MAX_PAIRS} pairs)")
    return None


def _rule_graphs(export, a, own, pos, pos_bstride, mask_u8, tool_u8, base, n_tools, bounds_pos, bounds_first, bounds_idx, bounds_n, pad_rows,
                 ratio, edge_cap, engine, out):
    """What the two rule launches share: the checks on the common tensors, the `out` allocation and the common fields of `a` (an
    AgRuleGraphsArgs or AgSurfaceRuleGraphsArgs; the two structs name them alike); own: the rule's own (field, tensor or None)
    pairs.  Launches eng.lib.<export> -> out."""
    import ctypes as C
    dev = mask_u8.device
    eng = engine or default_engine(dev)
    B, N = mask_u8.shape
    for t, dt, shape in ((mask_u8, torch.uint8, (B, N)), (tool_u8, torch.uint8, (B, N)), (bounds_first, torch.int64, (B,)),
                         (bounds_n, torch.int32, (B,)), (base.n_edges, torch.int32, (B,)), (base.row_ptr, torch.int32, (B, N + 1))):
        assert t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev, (t.dtype, tuple(t.shape), shape)
    assert base.send.dtype == torch.int32 and base.send.shape[0] == B and base.send.is_contiguous()
    assert bounds_pos.dtype == torch.float32 and bounds_pos.is_contiguous() and bounds_pos.shape[-1] == 3
    assert bounds_idx is None or (bounds_idx.dtype == torch.int32 and bounds_idx.shape[0] == B and bounds_idx.is_contiguous())
    edge_cap = max(1, int(edge_cap))
    if out is None:
        out = EdgeList(torch.empty((B, edge_cap), device=dev, dtype=torch.int32), torch.empty((B, edge_cap), device=dev, dtype=torch.int32),
                       torch.empty((B, N + 1), device=dev, dtype=torch.int32), torch.empty((B,), device=dev, dtype=torch.int32), N)
    assert out.edge_cap == edge_cap and out.recv.shape[0] == B
    a.d_pos = pos if isinstance(pos, int) else pos.data_ptr()
    a.pos_bstride = int(pos_bstride)
    for name, t in (("d_mask", mask_u8), ("d_tool_mask", tool_u8), ("d_send_in", base.send), ("d_row_ptr_in", base.row_ptr),
                    ("d_n_edges_in", base.n_edges), ("d_bounds_pos", bounds_pos), ("d_bounds_first", bounds_first),
                    ("d_bounds_idx", bounds_idx), ("d_bounds_n", bounds_n), ("d_recv", out.recv), ("d_send", out.send),
                    ("d_row_ptr", out.row_ptr), ("d_n_edges_out", out.n_edges)) + tuple(own):
        setattr(a, name, t.data_ptr() if t is not None else None)
    a.bounds_points = bounds_pos.numel() // 3
    a.ratio = float(ratio)
    a.B, a.N, a.n_tools, a.base_cap, a.edge_cap = B, N, int(n_tools), base.edge_cap, edge_cap
    a.idx_stride = bounds_idx.shape[1] if bounds_idx is not None else 0
    a.pad_rows = int(pad_rows)
    eng.check(getattr(eng.lib, export)(eng.ctx, current_stream(dev), C.byref(a)))
    return out


def nonfixed_rule_graphs(pos, pos_bstride, mask_u8, tool_u8, base, n_tools, kNN, bounds_pos, bounds_first, bounds_idx, bounds_n,
                         pad_rows, ratio, edge_cap, engine=None, out=None, thr_out=None):
    """ag_edges_nonfixed_rule_graphs: the non-fixed rule (graph.py:125-171) and its kNN filter on the B base graphs `base` (an
    EdgeList as ag_build_edges_graphs wrote it) -> new EdgeList of capacity edge_cap.  Enqueue only.
    pos: a float32 tensor (B, N, 3) or a device address, graph b at + b * pos_bstride floats (0: N * 3); mask_u8 / tool_u8 (B, N)
    uint8; kNN (B,) float64; the bounds source: bounds_pos flat (P, 3) float32, bounds_first (B,) int64, bounds_idx (B, stride) int32
    or None, bounds_n (B,) int32, pad_rows, ratio (include/adaptigraph_amd.h).  out: an EdgeList to write into; thr_out: (B,)
    float32 that receives the thresholds.  n_edges[b] = -1 marks a refused graph: raise where the counts are read."""
    from . import _lib
    B = mask_u8.shape[0]
    assert kNN.dtype == torch.float64 and tuple(kNN.shape) == (B,) and kNN.is_contiguous() and kNN.device == mask_u8.device, \
        (kNN.dtype, tuple(kNN.shape), (B,))
    return _rule_graphs("ag_edges_nonfixed_rule_graphs", _lib.AgRuleGraphsArgs(), (("d_kNN", kNN), ("d_thr", thr_out)), pos, pos_bstride,
                        mask_u8, tool_u8, base, n_tools, bounds_pos, bounds_first, bounds_idx, bounds_n, pad_rows, ratio, edge_cap, engine, out)


def surface_graphs_limit(N, n_tools):
    """None when ag_edges_surface_rule_graphs takes graphs of N particles with n_tools tool points, else the limit in words."""
    if N > 4096:
        return f"N = {N} exceeds 4096"
    if n_tools > RULE_GRAPHS_MAX_TOOLS:
        return f"n_tools = {n_tools} exceeds the LDS-resident tool list (at most {RULE_GRAPHS_MAX_TOOLS} tool points)"
    return None


def surface_rule_graphs(pos, pos_bstride, mask_u8, tool_u8, base, n_tools, bounds_pos, bounds_first, bounds_idx, bounds_n, pad_rows,
                        ratio, bounds_order, edge_cap, engine=None, out=None, bounds_out=None, planes_out=None):
    """ag_edges_surface_rule_graphs: the two-closest-planes rule (graph.py:175-221) on the B graphs `base` (an EdgeList as
    ag_build_edges_graphs or ag_edges_nonfixed_rule_graphs wrote it) -> new EdgeList of capacity edge_cap.  Enqueue only.
    Arguments as nonfixed_rule_graphs (no kNN: this rule has no filter).  bounds_order 0: the eval step loop's bounds
    (rollout.surface_bounds), 1: construct_graph's (min_x / min_z from the unscaled maxima).  out: an EdgeList to write into;
    bounds_out (B, 6) float32: max_y, min_y, max_x, max_z, min_x, min_z as the rule used them; planes_out (B, 2) int32: the chosen
    planes as indices into max_y, min_x, max_x, min_z, max_z (-1 without contact).  n_edges[b] = -1 marks a refused graph: raise
    where the counts are read."""
    from . import _lib
    B = mask_u8.shape[0]
    assert bounds_out is None or (bounds_out.dtype == torch.float32 and tuple(bounds_out.shape) == (B, 6) and bounds_out.is_contiguous())
    assert planes_out is None or (planes_out.dtype == torch.int32 and tuple(planes_out.shape) == (B, 2) and planes_out.is_contiguous())
    a = _lib.AgSurfaceRuleGraphsArgs()
    a.bounds_order = int(bounds_order)
    return _rule_graphs("ag_edges_surface_rule_graphs", a, (("d_bounds", bounds_out), ("d_planes", planes_out)), pos, pos_bstride, mask_u8,
                        tool_u8, base, n_tools, bounds_pos, bounds_first, bounds_idx, bounds_n, pad_rows, ratio, edge_cap, engine, out)


class BackoffPlan:
    """The max_nR back-off of construct_edges_with_backoff (dataset.py:317-349, rollout.py:173-222) for B graphs at once, as a
    pure host state machine: it is told the edge counts of an attempt and says which graphs need another one, and with what.

        plan = BackoffPlan(knn, topk, max_nR, min_kNN, knn_increment)
        while plan.active:                      # graph indices of this round's attempt
            counts = <attempt: graph b at plan.kNN[b] and top-k plan.k_now[b]; plan.rebuild[b]: its base graph changes too>
            plan.record(counts)

    Per graph: while kNN > min_kNN, kNN -= knn_increment (Python doubles) at the ORIGINAL top-k - the base graph is unchanged, only
    the rule reruns; after that top-k goes down by one per attempt with kNN left where it stopped; below top-k 1 it raises
    Exception('Exceeds max dims').  trail[b] holds (kNN, topk, n_rel) of every attempt.  has_rule=False (a kNN range without the
    non-fixed rule): a kNN attempt rebuilds nothing, so it is recorded with the unchanged count and costs no round.
    rounds: the number of record() calls = read-backs."""

    def __init__(self, knn, topk, max_nR, min_kNN=1.0, knn_increment=0.1, has_rule=True):
        self.kNN = list(map(float, knn))
        B = len(self.kNN)
        self.topk, self.max_nR, self.min_kNN, self.knn_increment = int(topk), int(max_nR), float(min_kNN), float(knn_increment)
        self.has_rule = bool(has_rule)
        self.k_now = [self.topk] * B
        self._decrease_topK = [self.topk] * B
        self.rebuild = [True] * B
        self.trail = [[] for _ in range(B)]
        self.active = list(range(B))
        self.rounds = 0

    def record(self, counts):
        """counts[j]: the edge count of graph self.active[j] in the attempt just made.  Returns the graphs of it that now fit."""
        assert len(counts) == len(self.active)
        self.rounds += 1
        counts = np.asarray(counts, np.int64).tolist()
        kNN, k_now, trail = self.kNN, self.k_now, self.trail
        if counts and min(counts) >= 0 and max(counts) <= self.max_nR:                   # every graph fits: no state to advance
            for b, c in zip(self.active, counts):
                trail[b].append((kNN[b], k_now[b], c))
            fits, self.active = self.active, []
            return fits
        nxt, fits = [], []
        for b, c in zip(self.active, counts):
            if c < 0:
                raise RuntimeError("internal: ag_edges_nonfixed_rule_graphs refused a graph (base edge list or tool count inconsistent)")
            while True:
                self.trail[b].append((self.kNN[b], self.k_now[b], c))
                if c <= self.max_nR:
                    fits.append(b)
                    break
                if self.kNN[b] <= self.min_kNN:
                    self._decrease_topK[b] -= 1
                    if self._decrease_topK[b] < 1:
                        raise Exception("Exceeds max dims")                              # (the reference would loop on: utils.py:63-65)
                    self.k_now[b], self.rebuild[b] = self._decrease_topK[b], True
                    nxt.append(b)
                    break
                self.kNN[b] = self.kNN[b] - self.knn_increment
                self.k_now[b], self.rebuild[b] = self.topk, False
                if self.has_rule:
                    nxt.append(b)
                    break
        self.active = nxt
        return fits


@dataclass
class RuleConfig:
    """What an attempt of the batched back-off needs besides its graphs: is the non-fixed rule on (else only the base graphs are
    built), the tool points per graph, connect_tool_surface_ratio, connect_tool_all, the engine; surface: the two-closest-planes
    rule follows (chained behind the non-fixed rule when both are on), with its bounds in bounds_order (surface_rule_graphs)."""
    rule: bool
    n_tools: int
    ratio: float
    connect_tools_all: bool = False
    engine: object = None
    surface: bool = False
    bounds_order: int = 0


def rule_attempt(cfg, pos, bstride, mask, tool, base, knn, bnd, cap, out=None):
    """The non-fixed rule on the base graphs, then the surface rule on its output (each only if the config has it; the base graphs
    themselves for a config with neither) -> EdgeList of capacity cap.  Both rules read the same bounds source bnd: (flat points,
    first (B,) int64, gather (B, stride) int32 or None, rows (B,) int32, pad_rows).  When both run, the graphs between them live in
    a buffer as wide as the base graphs' - the surface rule removes edges too, so cap is no capacity for its input."""
    if not cfg.rule and not cfg.surface:
        return base
    pts, first, idx, n, pad_rows = bnd
    el = base
    if cfg.rule:
        mid = max(base.edge_cap, cap) if cfg.surface else cap
        el = nonfixed_rule_graphs(pos, bstride, mask, tool, base, cfg.n_tools, knn, pts, first, idx, n, pad_rows, cfg.ratio, mid,
                                  engine=cfg.engine, out=None if cfg.surface else out)
    if cfg.surface:
        el = surface_rule_graphs(pos, bstride, mask, tool, el, cfg.n_tools, pts, first, idx, n, pad_rows, cfg.ratio, cfg.bounds_order,
                                 cap, engine=cfg.engine, out=out)
    return el


def attempt_with_backoff(cfg, plan, pos, bstride, base, knn, last, mask, tool, thr2, cull, bnd, cap, out=None, read_knn=False):
    """The whole batched build behind the base graphs, for every config: rule_attempt on `base` (the graphs at plan.topk; pos /
    bstride as construct_edges_graphs took them, knn (B,) float64 on the device), ONE read-back of the counts, plan.record, then
    backoff_rounds -> EdgeList of capacity cap, every graph within plan.max_nR (or Exception('Exceeds max dims')).  read_knn: the
    plan's kNN values are the draws `knn`, which only the device holds; they come back in the same transfer as the counts.
    A config with neither rule launches nothing here: the counts are the base graphs' own, a lower top-k rebuilds into buffers of
    their capacity, and knn / bnd may be None."""
    el = rule_attempt(cfg, pos, bstride, mask, tool, base, knn, bnd, cap, out=out)
    if read_knn:
        host = torch.cat([knn, el.n_edges.to(torch.float64)]).cpu().numpy()                  # the one wait
        plan.kNN, counts = host[:len(knn)].tolist(), host[len(knn):].astype(np.int64)
    else:
        counts = el.n_edges.cpu().numpy()                                                    # the one wait
    plan.record(counts)
    backoff_rounds(cfg, plan, el, base, last, mask, tool, thr2, cull, bnd)
    return el


def backoff_rounds(cfg, plan, el, base, last, mask, tool, thr2, cull, bnd):
    """BackoffPlan's rounds after the first attempt: per round the sub-batch plan.active, one group per top-k (the kNN group reruns
    the rule on its rows of `base`, a lower top-k rebuilds the base graphs from `last`, the (B, N, 3) positions), ONE read-back of
    the round's counts, and the graphs that now fit are copied into their rows of `el`.  Rows of el / base / last / mask / tool /
    thr2 / cull / bnd correspond; a graph fits when its count is within plan.max_nR, whatever el's capacity.  The kNN values and the
    bounds rows of a sub-batch are gathered only for a config whose rules read them (bnd may be None otherwise)."""
    N, dev = el.N, mask.device
    ruled = cfg.rule or cfg.surface
    while plan.active:
        groups = {}
        for b in plan.active:
            groups.setdefault(plan.k_now[b], []).append(b)
        groups = [groups[kk] for kk in sorted(groups, reverse=True)]                         # graphs that share a top-k share a launch
        parts = []
        for g in groups:
            kk = plan.k_now[g[0]]
            sub = torch.tensor(g, dtype=torch.int64).to(dev)
            pos, m, t = last[sub].contiguous(), mask[sub].contiguous(), tool[sub].contiguous()
            if kk == plan.topk:                                                              # kNN went down: the base graph stands
                b_el = EdgeList(base.recv[sub], base.send[sub], base.row_ptr[sub], base.n_edges[sub], N)
            else:
                b_el = construct_edges_graphs(pos, 0, m, t, thr2[sub].contiguous(), cull[sub].contiguous(), kk, cfg.connect_tools_all,
                                              edge_cap=base.edge_cap, engine=cfg.engine)
            knn = sub_bnd = None
            if ruled:
                pts, first, idx, n_rows, pad_rows = bnd
                knn = torch.tensor([plan.kNN[b] for b in g], dtype=torch.float64).to(dev)
                sub_bnd = (pts, first[sub], None if idx is None else idx[sub], n_rows[sub], pad_rows)
            parts.append((sub, rule_attempt(cfg, pos, 0, m, t, b_el, knn, sub_bnd, el.edge_cap)))
        counts = [se.n_edges for _, se in parts]
        counts = (counts[0] if len(counts) == 1 else torch.cat(counts)).cpu().numpy()        # one wait per round
        plan.active = [b for g in groups for b in g]                                         # the order of `counts`
        plan.record(counts)
        off = 0
        for sub, se in parts:
            c = counts[off:off + len(sub)]
            off += len(sub)
            fit = (c <= plan.max_nR).nonzero()[0]
            if len(fit):
                src = torch.from_numpy(fit).to(dev)
                dst = sub[src]
                el.recv[dst], el.send[dst], el.row_ptr[dst], el.n_edges[dst] = se.recv[src], se.send[src], se.row_ptr[src], se.n_edges[src]


def pad_torch(x, max_dim, dim=0):
    """src/dynamics/utils.py:49-69: zero-pad `dim` to max_dim, raise Exception('Exceeds max dims') when larger."""
    if dim == 0:
        x_dim = x.shape[0]
        out = torch.zeros((max_dim, x.shape[1]), dtype=x.dtype, device=x.device)
        if x_dim > max_dim:
            raise Exception("Exceeds max dims")
        out[:x_dim] = x
    elif dim == 1:
        x_dim = x.shape[1]
        out = torch.zeros((x.shape[0], max_dim, x.shape[2]), dtype=x.dtype, device=x.device)
        if x_dim > max_dim:
            raise Exception("Exceeds max dims")
        out[:, :x_dim] = x
    else:
        raise ValueError("pad_torch supports dim 0 or 1")
    return out


def truncate_graph(data):
    """src/dynamics/utils.py:150-160: cut Rr/Rs back to the largest non-zero row count in the batch."""
    Rr, Rs = data["Rr"], data["Rs"]
    n_Rr = int((Rr.sum(-1) > 0).sum(1).max().item())
    n_Rs = int((Rs.sum(-1) > 0).sum(1).max().item())
    n = max(n_Rr, n_Rs)
    data["Rr"] = Rr[:, :n, :]
    data["Rs"] = Rs[:, :n, :]
    return data
