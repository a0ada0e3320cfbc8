"""Degenerate-graph batches for the backward tests (tests/test_backward_shapes.py on the CPU, tests/test_gpu_backward_shapes.py
on the GPU), and the float64 / fp32 torch restatement of their gradients (tests/train_restate.py) on any device.

A batch holds graphs over the same N particles, kinds cycling through KINDS:
  dense  12 random distinct senders per receiver (12 N edges).
  empty  n_edges = 0.
  hub    node N-1 sends to every other node and receives from every other node: sorted by receiver, edges 0 .. N-2 all have the
         sender N-1 (one sender's edges fill a whole 64-edge sweep and run into the next), and the receiver row N-1 holds N-1 edges.
  half   nodes N//2 .. N-1 have no incident edge; nodes 0 .. N//2-1 each receive three edges from the senders [0, 0, 1]: every edge
         but the third of a row is a duplicate, sender 0 has 2 (N//2) edges (64 or more) spread over every sweep, and the edges
         0 -> 0 (twice) and 1 -> 1 are self edges.
Lists are sorted by receiver; tests/test_gpu_train.py::_edge_list builds row_ptr from them.
"""
from __future__ import annotations

import numpy as np
import torch

import train_restate as TR

KINDS = ["dense", "empty", "hub", "half"]
# name -> (N, n_p, n_his, pstep): a tool row / no tool row at pstep's lower bound / two tool rows at its upper bound
CONFIGS = {"tool_row": (97, 96, 4, 3), "no_tool_row": (97, 97, 4, 1), "pstep7": (65, 63, 5, 7)}
NAMES = TR.KEYS + ["state", "phys", "action"]
# the all-real-rows split-K case: 4 x 300 x 28 = 33,600 edge rows.  With ~10^7 ReLU inputs some sit within fp32 rounding of zero, and
# at most seeds one of them decides the comparison for ANY fp32 implementation: perturbing the weights by fp32 rounding (6e-8
# relative) moves the float64 gradients themselves by 3e-5 .. 1.4e-3 of a tensor's max at 11 of the 17 seeds tried (57: 4.7e-4 on
# relation_propagator.linear.weight, exactly what the engine then shows against float64).  At 54, 71, 72, 74 and 75 they move by 2e-7;
# 54 also leaves the fp32 restatement on the CPU 3e-6 from float64.  tests/test_backward_shapes.py holds both conditions.
SPLITK_CONFIG = (300, 299, 4, 3)
SPLITK_SEED = 54


def graph(kind, N, rng):
    """-> (recv, send) int32, sorted by receiver."""
    if kind == "dense":
        recv = np.repeat(np.arange(N), 12)
        send = np.concatenate([rng.choice(N, 12, replace=False) for _ in range(N)])
    elif kind == "empty":
        recv = send = np.zeros(0)
    elif kind == "hub":
        recv = np.concatenate([np.arange(N - 1), np.full(N - 1, N - 1)])
        send = np.concatenate([np.full(N - 1, N - 1), np.arange(N - 1)])
    elif kind == "half":
        recv = np.repeat(np.arange(N // 2), 3)
        send = np.tile([0, 0, 1], N // 2)
    else:
        raise ValueError(kind)
    return recv.astype(np.int32), send.astype(np.int32)


def make_batch(N, n_p, n_his, B=4, seed=1, kinds=None):
    """B graphs (kinds: KINDS cycled) with states, per-particle physics parameters and upstream gradients of their own.  Graphs
    beyond the fourth repeat the edge lists of graph b - 4 on a perturbed copy of its state; the first four do not depend on B.
    seed 1: with seed 0 the pstep7 configuration puts a particle-encoder ReLU input within fp32 rounding of zero (the fp32
    restatement's dphys is 1.3e-4 of the tensor's max off float64; 2e-6 at seeds 1 to 3), which tests/test_backward_shapes.py refuses."""
    rng = np.random.default_rng(seed)
    B0 = min(B, 4) if kinds is None else B
    kinds = [KINDS[b % len(KINDS)] for b in range(B0)] if kinds is None else list(kinds)
    edges = [graph(k, N, rng) for k in kinds]
    state = np.zeros((B0, n_his, N, 3), np.float32)
    for b in range(B0):
        cloud = rng.uniform(-1, 1, (N, 3)) * [1.0, 0.2, 1.0]
        for t in range(n_his):
            state[b, t] = cloud + rng.normal(0, 0.01, (N, 3))
    action = np.zeros((B0, N, 3), np.float32)
    action[:, n_p:] = rng.normal(0, 0.05, (B0, N - n_p, 3))
    phys = rng.uniform(0.2, 0.8, (B0, n_p)).astype(np.float32)
    gp, gm = (rng.normal(0, 1, (B0, n_p, 3)).astype(np.float32) for _ in range(2))
    if B > B0:
        more = np.arange(B0, B) - 4
        rng = np.random.default_rng(seed + 1000)
        kinds, edges = kinds + [kinds[b] for b in more], edges + [edges[b] for b in more]
        state = np.concatenate([state, (state[more] + rng.normal(0, 0.01, state[more].shape)).astype(np.float32)])
        action = np.concatenate([action, action[more]])
        phys = np.concatenate([phys, rng.uniform(0.2, 0.8, (len(more), n_p)).astype(np.float32)])
        gp = np.concatenate([gp, rng.normal(0, 1, (len(more), n_p, 3)).astype(np.float32)])
        gm = np.concatenate([gm, rng.normal(0, 1, (len(more), n_p, 3)).astype(np.float32)])
    attrs = np.zeros((B, N, 2), np.float32)
    attrs[:, :n_p, 0] = 1
    attrs[:, n_p:, 1] = 1
    return dict(kinds=kinds, N=N, n_p=n_p, n_his=n_his, state=state, attrs=attrs, action=action,
                p_instance=np.ones((B, n_p, 1), np.float32), phys=phys, recv_l=[e[0] for e in edges], send_l=[e[1] for e in edges],
                gp=gp, gm=gm)


def dense_batch(N, n_p, n_his, B, per_recv, seed):
    """B dense random graphs of per_recv distinct senders per receiver (the split-K cases)."""
    bt = make_batch(N, n_p, n_his, B=B, seed=seed, kinds=["empty"] * B)
    rng = np.random.default_rng(seed + 1)
    bt["kinds"] = ["dense"] * B
    bt["recv_l"] = [np.repeat(np.arange(N), per_recv).astype(np.int32) for _ in range(B)]
    bt["send_l"] = [np.concatenate([rng.choice(N, per_recv, replace=False) for _ in range(N)]).astype(np.int32) for _ in range(B)]
    return bt


def rounding_sensitivity(bt, W, pstep, g64, names, draws=3):
    """How far the float64 gradients themselves move, as a fraction of each tensor's max, when the weights are perturbed by fp32
    rounding (6e-8 relative, `draws` seeded draws): above ~1e-6 a ReLU input within rounding of zero decides, and agreement of
    any fp32 run with float64 is luck.  -> the worst over names and draws."""
    worst = 0.0
    for d in range(draws):
        rng = np.random.default_rng(100 + d)
        Wp = {k: v.astype(np.float64) * (1 + 6e-8 * rng.uniform(-1, 1, v.shape)) for k, v in W.items()}
        gp, _, _ = restate(bt, Wp, pstep, torch.float64)
        worst = max([worst] + [float(np.abs(gp[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in names])
    return worst


def restate(bt, W, pstep, dtype, device="cpu", loss=None):
    """Gradients of sum(pos * gp) + sum(motion * gm) (or loss(step) if given) in `dtype` on `device` ->
    ({name: float64 numpy array} over NAMES, pred_pos, pred_motion as float64 numpy)."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(device=device, dtype=dtype)   # noqa: E731
    B, N, n_p = len(bt["recv_l"]), bt["N"], bt["n_p"]
    Wd = {k: t(W[k]).requires_grad_(True) for k in TR.KEYS}
    state, action, pp = t(bt["state"]).requires_grad_(True), t(bt["action"]).requires_grad_(True), t(bt["phys"]).requires_grad_(True)
    phys = torch.cat([pp, torch.zeros(B, N - n_p, dtype=dtype, device=device)], 1)
    group = torch.cat([t(bt["p_instance"]), torch.zeros(B, N - n_p, 1, dtype=dtype, device=device)], 1)
    recv = torch.from_numpy(np.concatenate([r.astype(np.int64) + b * N for b, r in enumerate(bt["recv_l"])])).to(device)
    send = torch.from_numpy(np.concatenate([s.astype(np.int64) + b * N for b, s in enumerate(bt["send_l"])])).to(device)
    step = lambda s, a: TR.forward(Wd, s, t(bt["attrs"]), a, phys, group, recv, send, n_p, pstep)   # noqa: E731
    if loss is None:
        pos, mot = step(state, action)
        ((pos * t(bt["gp"])).sum() + (mot * t(bt["gm"])).sum()).backward()
    else:
        pos, mot = loss(step, state, action, t)
    g = {k: Wd[k].grad for k in TR.KEYS}
    g.update(state=state.grad, phys=pp.grad, action=action.grad)
    g = {k: (v.detach().double().cpu().numpy() if v is not None else None) for k, v in g.items()}
    return g, pos.detach().double().cpu().numpy(), mot.detach().double().cpu().numpy()


def bar(ref, err32):
    """The project's gradient bar: max|g - g64| <= max(3e-4 max|g64| + 1e-7, 4 err32), err32 = the fp32 restatement's own error."""
    return max(3e-4 * float(np.abs(ref).max()) + 1e-7, 4.0 * float(err32))
