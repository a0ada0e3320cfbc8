"""Torch restatement of DynamicsPredictor.forward (reference src/dynamics/gnn/model.py:130-342) on index-list graphs, for
autograd in any dtype on any device: index gathers for Rr.bmm / Rs.bmm and index_add for Rr_t.bmm.  The tests use it in
float64 as the gradient yardstick; tools/bench_train.py runs it in fp32 on the GPU as the torch baseline.

Also: the training-fixture loaders shared by tests/test_train.py and tests/test_gpu_train.py.
"""
from __future__ import annotations

import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ORDER = ["particle_encoder.model.0", "particle_encoder.model.2", "particle_encoder.model.4",
         "relation_encoder.model.0", "relation_encoder.model.2", "relation_encoder.model.4",
         "particle_propagator.linear", "relation_propagator.linear",
         "non_rigid_predictor.linear_0", "non_rigid_predictor.linear_1", "non_rigid_predictor.linear_2"]
KEYS = [b + s for b in ORDER for s in (".weight", ".bias")]


def make_weights(seed, n_his=4, nf=150):
    """Seeded parameters (nn.Linear's U(-1/sqrt(fan_in), 1/sqrt(fan_in)) ranges, numpy RNG): the training fixtures store the
    seed, not the 250k floats."""
    rel = 5 + 3 * n_his
    shapes = [(nf, 6), (nf, nf), (nf, nf), (nf, rel), (nf, nf), (nf, nf), (nf, 2 * nf), (nf, 3 * nf), (nf, nf), (nf, nf), (3, nf)]
    rng = np.random.default_rng(seed)
    W = {}
    for base, (o, i) in zip(ORDER, shapes):
        bound = 1.0 / np.sqrt(i)
        W[base + ".weight"] = rng.uniform(-bound, bound, (o, i)).astype(np.float32)
        W[base + ".bias"] = rng.uniform(-bound, bound, (o,)).astype(np.float32)
    return W


def fixture_weights(f):
    """The fixture's parameters: make_weights(w_seed), non_rigid_predictor.linear_2 rescaled as recorded (train_clamp)."""
    W = make_weights(int(f["w_seed"]), n_his=f["state"].shape[1])
    W["non_rigid_predictor.linear_2.weight"] = W["non_rigid_predictor.linear_2.weight"] * np.float32(f["l2_scale"])
    W["non_rigid_predictor.linear_2.bias"] = (W["non_rigid_predictor.linear_2.bias"] * np.float32(f["l2_scale"])
                                              + f["l2_shift"].astype(np.float32))
    return W


def _mlp(x, W, pre, idx, relu_last=True):
    for j, i in enumerate(idx):
        x = x @ W[f"{pre}{i}.weight"].T + W[f"{pre}{i}.bias"]
        if relu_last or j < len(idx) - 1:
            x = torch.relu(x)
    return x


def forward(W, state, attrs, action, phys, group, recv, send, n_p, pstep, clamp=100.0):
    """state (B,n_his,N,3); attrs (B,N,2); action (B,N,3); phys (B,N) (zero for tools); group (B,N,n_inst) = [p_instance; 0];
    recv / send: flat node ids b*N + i of every edge (LongTensor).  Returns pred_pos, pred_motion (B,n_p,3)."""
    B, n_his, N, _ = state.shape
    res = state[:, 1:] - state[:, :-1]                                           # :156
    snt = torch.cat([res, state[:, -1:]], 1).transpose(1, 2).reshape(B * N, n_his * 3)   # :165-166
    p_in = torch.cat([attrs, phys[..., None], action], 2).reshape(B * N, 6)       # :169,210,223
    at = attrs.reshape(B * N, 2)
    g = group.reshape(B * N, -1)
    gd = (g[recv] - g[send]).abs().sum(1, keepdim=True)                          # :264-267
    rel_in = torch.cat([at[recv], at[send], gd, snt[recv] - snt[send]], 1)       # :257,270,282
    p_enc = _mlp(p_in, W, "particle_encoder.model.", (0, 2, 4))                 # :297
    r_enc = _mlp(rel_in, W, "relation_encoder.model.", (0, 2, 4))               # :303
    eff = p_enc
    for _ in range(pstep):                                                       # :307-330
        er = torch.relu(torch.cat([r_enc, eff[recv], eff[send]], 1) @ W["relation_propagator.linear.weight"].T
                        + W["relation_propagator.linear.bias"])
        agg = torch.zeros_like(eff).index_add(0, recv, er)
        eff = torch.relu(torch.cat([p_enc, agg], 1) @ W["particle_propagator.linear.weight"].T
                         + W["particle_propagator.linear.bias"] + eff)
    eff = eff.reshape(B, N, -1)[:, :n_p].reshape(B * n_p, -1)
    mot = _mlp(eff, W, "non_rigid_predictor.linear_", (0, 1, 2), relu_last=False).reshape(B, n_p, 3)   # :335
    pos = state[:, -1, :n_p] + torch.clamp(mot, min=-clamp, max=clamp)            # :338
    return pos, mot


# ------------------------------------------------------------------------------------------------ training fixtures
def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name))
    return {k: z[k] for k in z.files}


def fixture_edges(f, B, N, device="cpu"):
    """Per-graph index lists of a fixture -> flat (recv, send) node ids and padded per-graph arrays."""
    cnt = f["n_edges"].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)])
    recv = np.concatenate([f["recv"][off[b]:off[b + 1]].astype(np.int64) + b * N for b in range(B)])
    send = np.concatenate([f["send"][off[b]:off[b + 1]].astype(np.int64) + b * N for b in range(B)])
    return torch.from_numpy(recv).to(device), torch.from_numpy(send).to(device)


def fixture_inputs(f, dtype=torch.float64, device="cpu"):
    """(state0, attrs, action steps, phys (B,N), group (B,N,n_inst), state_future, eef_future) as tensors."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(device=device, dtype=dtype)   # noqa: E731
    attrs = t(f["attrs"])
    B, N = attrs.shape[:2]
    p_inst = t(f["p_instance"])
    n_p = p_inst.shape[1]
    phys = torch.zeros(B, N, dtype=dtype, device=device)
    pp = t(f["physics_param"]).reshape(B, -1)
    phys[:, :n_p] = pp if pp.shape[1] == n_p else pp[:, :1]
    group = torch.cat([p_inst, torch.zeros(B, N - n_p, p_inst.shape[2], dtype=dtype, device=device)], 1)
    return dict(state=t(f["state"]), attrs=attrs, action=t(f["action"]), phys=phys, group=group, n_p=n_p,
                state_future=t(f["state_future"]), eef_future=t(f["eef_future"]), action_future=t(f["action_future"]))


def weights(f, dtype=torch.float64, device="cpu", requires_grad=True):
    W = fixture_weights(f)
    return {k: torch.from_numpy(W[k]).to(device=device, dtype=dtype).requires_grad_(requires_grad) for k in KEYS}


def chain_loss(step, inp, n_future):
    """train.py:86-124 loop body: n_future chained forwards, MSE on pred_state, next state assembled from the prediction.
    step(state, action) -> (pred_pos, pred_motion)."""
    state, action = inp["state"], inp["action"]
    n_p = inp["n_p"]
    loss = 0
    for fi in range(n_future):
        gt = inp["state_future"][:, fi]
        pred, _ = step(state, action)
        loss = loss + torch.nn.functional.mse_loss(pred[:, :gt.shape[1], :3], gt)
        if fi < n_future - 1:
            nxt = inp["eef_future"][:, fi].clone().unsqueeze(1)
            nxt[:, -1, :n_p] = pred[:, :n_p]
            state = torch.cat([state[:, 1:], nxt], 1)
            action = inp["action_future"][:, fi]
    return loss
