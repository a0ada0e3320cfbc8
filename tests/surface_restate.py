"""ag_edges_surface_rule_graphs restated in plain numpy for ONE graph: the "tool to the two closest surface planes" rule of
construct_edges_from_states (reference src/dynamics/dataset/graph.py:175-221) as the kernel forms it - the six bounds from a set of
rows in either order, the contact check on the INPUT edge list, the plane values in closed form, the subset, the merge.  The CPU
yardstick of the batched rule, pinned to the reference's own graphs by tests/test_surface_rule_host.py (fixture from
tests/golden/make_golden_eval_batch_surface.py).  The base graph and the non-fixed rule in front of it are the oracle's
(oracle.adaptigraph_oracle.construct_edges_from_states without connect_tools_surface)."""
import numpy as np

from oracle import adaptigraph_oracle as O

F32 = np.float32
PLANES = ["max_y", "min_x", "max_x", "min_z", "max_z"]                  # graph.py:40 order = the kernel's plane indices 0 .. 4
BOUND_KEYS = ("max_y", "min_y", "max_x", "max_z", "min_x", "min_z")     # the order of the kernel's d_bounds


def bounds6(rows, pad_rows, ratio, order):
    """The six bounds of the rows (n, 3) fp32, a zero row added iff pad_rows > n, as (6,) fp32 in BOUND_KEYS order.  Every operation
    is one separately rounded fp32 operation on fp32(ratio) and fp32(1 - ratio in double).  order 0: rollout.py:132-139 (min_x / min_z
    from the SCALED maxima), order 1: rollout/graph.py:446-458 (from the UNSCALED maxima, the maxima scaled afterwards).  No row
    at all: NaN."""
    rows = np.asarray(rows, F32).reshape(-1, 3)
    if pad_rows > len(rows):
        rows = np.concatenate([rows, np.zeros((1, 3), F32)])
    if len(rows) == 0:
        return np.full(6, np.nan, F32)
    r, q = F32(ratio), F32(1.0 - float(ratio))
    with np.errstate(invalid="ignore"):
        mx, mn = rows.max(0), rows.min(0)                                # np.max propagates NaN per column
        max_y, max_x, max_z = mx[1] * r, mx[0] * r, mx[2] * r
        hx, hz = (mx[0], mx[2]) if order else (max_x, max_z)
        min_x = (hx - mn[0]) * q + mn[0]
        min_z = (hz - mn[2]) * q + mn[2]
    out = np.array([max_y, mn[1], max_x, max_z, min_x, min_z])
    assert out.dtype == F32
    return out


def plane_values(pos, n0, n1, bd):
    """value_k = N * (n0 * d_0 + n1 * d_1) in fp64, d the fp32 squared distance of particles 0 and min(1, N - 1) to plane k's bound."""
    pos = np.asarray(pos, F32)
    N = len(pos)
    k1 = min(1, N - 1)
    bound = [bd[0], bd[4], bd[2], bd[5], bd[3]]
    axis = [1, 0, 0, 2, 2]
    vals = []
    with np.errstate(invalid="ignore", over="ignore"):
        for ax, b in zip(axis, bound):
            e0, e1 = F32(pos[0, ax] - F32(b)), F32(pos[k1, ax] - F32(b))
            d0, d1 = float(F32(e0 * e0)), float(F32(e1 * e1))
            vals.append(N * (n0 * d0 + n1 * d1))
    return np.array(vals, np.float64)


def side(plane, pos, bd):
    pos = np.asarray(pos, F32)
    with np.errstate(invalid="ignore"):
        return [pos[:, 1] >= bd[0], pos[:, 0] <= bd[4], pos[:, 0] >= bd[2], pos[:, 2] <= bd[5], pos[:, 2] >= bd[3]][plane]


def surface_rule(pos, mask, tool, recv, send, bd):
    """The rule on an edge list sorted by (receiver, sender) -> (recv, send, planes, S, check).  planes: (-1, -1) and the list copied
    through when no input edge has a tool sender."""
    pos = np.asarray(pos, F32)
    mask, tool = np.asarray(mask, bool), np.asarray(tool, bool)
    recv, send = np.asarray(recv, np.int64), np.asarray(send, np.int64)
    N, M = len(pos), int(tool.sum())
    check = int(tool[send].sum())
    if check == 0:
        return recv.astype(np.int32), send.astype(np.int32), (-1, -1), np.zeros(N, bool), 0
    vals = plane_values(pos, int(mask.sum()) * M - check, check, bd)
    order = np.argsort(vals, kind="stable")                              # (value, index), NaN last
    p1, p2 = int(order[0]), int(order[1])
    S = side(p1, pos, bd) & side(p2, pos, bd) & mask
    adj = np.zeros((N, N), bool)
    adj[recv, send] = True
    adj[tool[:, None] & S[None, :]] = False                              # graph.py:217 tool receiver, sender in S
    adj[S[:, None] & tool[None, :]] = True                               # :218 receiver in S, tool sender
    adj[tool[:, None] & tool[None, :]] = False                           # :219
    r, s = np.nonzero(adj)
    return r.astype(np.int32), s.astype(np.int32), (p1, p2), S, check


def chained(pos, adj_thresh, mask, tool, topk, connect_tools_all, nonfixed, kNN, rows, pad_rows, ratio, order, surface=True):
    """The base graph, the non-fixed rule (the oracle's, with max_y / min_y of the same rows) and the surface rule behind it, as
    graph.rule_attempt chains the two launches.  -> dict(recv, send, mid (the list between the rules), planes, S, check, bounds)."""
    bd = bounds6(rows, pad_rows, ratio, order)
    kw = dict(max_y=bd[0], min_y=bd[1]) if nonfixed else {}
    r0, s0 = O.construct_edges_from_states(pos, adj_thresh, mask, tool, topk=topk, connect_tools_all=connect_tools_all,
                                           connect_tool_all_non_fixed=bool(nonfixed), kNN=kNN, **kw)
    if not surface:
        return dict(recv=r0, send=s0, mid=(r0, s0), planes=(-1, -1), S=np.zeros(len(pos), bool), check=0, bounds=bd)
    r, s, planes, S, check = surface_rule(pos, mask, tool, r0, s0, bd)
    return dict(recv=r, send=s, mid=(r0, s0), planes=planes, S=S, check=check, bounds=bd)
