"""Shared by tests/test_ppm_grad.py and tests/test_gpu_ppm_grad.py: the ppm_grad_*.npz loaders, the gradient bar, and a torch
restatement of the masked rollout + chamfer loss on the fixture's edge lists (any dtype, CPU), built on tests/train_restate.py."""
from __future__ import annotations

import json
import types

import numpy as np
import torch

import train_restate as TR

MATERIALS = ["rope", "granular", "cloth"]
LAYOUTS = ["shared", "rows", "particles"]


def load(material):
    return TR.load_fixture(f"ppm_grad_{material}.npz")


def task_of(f):
    return json.loads(bytes(f["task_json"]).decode())


def ppm_of(task, material):
    return types.SimpleNamespace(task_config=task, eef_num=task["eef_num"], material=material,
                                 material_dims=task["material_dims"], material_indices=task["material_indices"],
                                 physics_param={material: torch.tensor([0.5])}, adj_thresh=task["adj_thresh"])


def bar(ref64, ref32):
    """max|g - ref64| allowed: max(3e-4 max|ref64| + 1e-7, 4 err32), err32 = the reference's own fp32 error against float64."""
    ref64 = np.asarray(ref64, np.float64)
    err32 = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    return max(3e-4 * float(np.abs(ref64).max()) + 1e-7, 4.0 * err32)


def step_edges(f, prefix, i):
    cnt = f[f"{prefix}step{i}::n_edges"]
    off = np.concatenate([[0], np.cumsum(cnt)])
    recv, send = f[f"{prefix}step{i}::recv"], f[f"{prefix}step{i}::send"]
    return [(recv[off[b]:off[b + 1]], send[off[b]:off[b + 1]]) for b in range(len(cnt))]


def chamfer_restated(x, y):
    """losses.py:4-10 on x (B,N,3), y (B,M,3) without the repeats."""
    dis = (x[:, None, :, :] - y[:, :, None, :]).norm(2, dim=-1)             # (B, M, N)
    return dis.min(dim=2).values.mean(dim=1) + dis.min(dim=1).values.mean(dim=1)


def restated_loss(f, material, layout, dtype=torch.float64):
    """forward_dynamics.py:209-399 + the mean masked chamfer on the fixture's edges.  -> (loss, per-row chamfer, state_seqs,
    phys leaf, state_init leaf); call loss.backward() for the gradients."""
    from adaptigraph_amd.plan_utils import decode_action
    from adaptigraph_amd.forward_dynamics import _tool_layout
    task = task_of(f)
    n_his, max_n = int(task["n_his"]), int(task["max_n"])
    W = {k: torch.from_numpy(v).to(dtype) for k, v in TR.make_weights(int(f["w_seed"]), n_his=n_his).items()}
    state = torch.from_numpy(f["state_init"]).to(dtype).requires_grad_(True)
    mask = torch.from_numpy(f["state_mask"])
    B, N_o, _ = state.shape
    M = int(task["eef_num"])
    N = N_o + M
    action = torch.from_numpy(f["action"])[:, None]
    decoded, repeat = decode_action(action, push_length=task["push_length"])
    xz, delta = _tool_layout(decoded, action[:, :, 2], task)
    xz, delta, repeat = xz[:, 0].to(dtype), delta[:, 0].to(dtype), repeat[:, 0]
    maskf, cnt = mask.to(dtype), mask.sum(1).to(dtype)
    grip = 0.01 * task["sim_real_ratio"] if task["gripper_enable"] else 0.0

    def tools_at(x, z, pos):
        y = (pos[:, :, 1] * maskf).sum(1) / cnt + grip
        return torch.stack([x, y[:, None].expand(B, M), z], -1)

    states = torch.cat([state[:, None].expand(B, n_his, N_o, 3), tools_at(xz[..., 0], xz[..., 1], state)[:, None].expand(B, n_his, M, 3)], 2)
    act = torch.cat([torch.zeros(B, N_o, 3, dtype=dtype), delta], 1)
    attrs = torch.zeros(B, N, 2, dtype=dtype)
    attrs[:, :N_o, 0] = maskf
    attrs[:, N_o:, 1] = 1
    group = torch.zeros(B, N, max_n, dtype=dtype)
    group[:, :N_o, 0] = (torch.arange(N_o)[None] < mask.sum(1)[:, None]).to(dtype)
    p = torch.from_numpy(f[f"{layout}::phys"]).to(dtype).requires_grad_(True)
    pp = p[None].expand(B, 1) if p.dim() == 1 else p
    phys = torch.cat([pp.expand(B, N_o), torch.zeros(B, M, dtype=dtype)], 1)
    seqs = torch.zeros(B, N_o, 3, dtype=dtype)
    for i in range(int(f[f"{layout}::n_steps"])):
        edges = step_edges(f, f"{layout}::", i)
        recv = torch.from_numpy(np.concatenate([r.astype(np.int64) + b * N for b, (r, _) in enumerate(edges)]))
        send = torch.from_numpy(np.concatenate([s.astype(np.int64) + b * N for b, (_, s) in enumerate(edges)]))
        pred, _ = TR.forward(W, states, attrs, act, phys, group, recv, send, N_o, int(f["pstep"]))
        seqs = torch.where((repeat == i + 1)[:, None, None], pred, seqs)
        last = states[:, -1, N_o:] + act[:, N_o:]
        cur = torch.cat([pred, tools_at(last[..., 0], last[..., 2], pred)], 1)
        states = torch.cat([states[:, 1:], cur[:, None]], 1)
    real, rmask = torch.from_numpy(f["state_real"]).to(dtype), torch.from_numpy(f["real_mask"])
    ch = torch.stack([chamfer_restated(seqs[b][mask[b]][None], real[b][rmask[b]][None])[0] for b in range(B)])
    return ch.mean(), ch, seqs, p, state
