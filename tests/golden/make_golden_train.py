#!/usr/bin/env python3
"""Generate the TRAINING fixtures from the real reference (jhyau/AdaptiGraph): gradients of its own autograd.

Runs only where the reference checkout exists (like make_golden.py, whose import recipe it reuses); the GPU tests see
only the .npz files written here.  What is driven (reference file:line):
  * DynamicsPredictor.forward + torch autograd     src/dynamics/gnn/model.py:130-342
  * construct_edges_from_states_batch              src/dynamics/dataset/graph.py:233-298
  * the train loop body, restated                  src/dynamics/train/train.py:86-124 (model(**data) at :97, next-state
                                                   assembly :104-119, loss_sum.backward() / optimizer.step() at :123-124)
on CPU, with seeded weights and synthetic clouds.

Each file holds: the weight seed (w_seed; tests/train_restate.py:make_weights) and, for train_clamp, the rescale of
non_rigid_predictor.linear_2 (l2_scale, l2_shift: |motion| passes 100 on about half of the rows, both signs); the data batch
(state, attrs, p_instance, physics_param, action, state_future, eef_future, action_future; edges as index lists recv / send /
n_edges); the inputs every future step saw (step<k>::state, step<k>::action); loss_sum and the 22 gradients after
loss_sum.backward() (g::<key>, rounded to 14 mantissa bits); dstate0 = dloss/d(first step's state); the loss curve of 5 Adam
steps (lr 1e-3, train.py:67); and, when model.double() runs, the reference's own fp32 error against its float64 gradients
(err64::<key>, dstate0_64, loss_sum_64).  train_clamp.npz is one forward (n_future 1) and records its pred_motion.

Usage:  python tests/golden/make_golden_train.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
import train_restate as TR  # noqa: E402

OUT = HERE


def rope_cloud(n, rng):
    t = np.linspace(0, 1, n)
    return (np.stack([-2 + 3 * t, 0 * t, 0.5 * np.sin(6 * t)], 1) + rng.normal(0, 0.01, (n, 3))).astype(np.float32)


def cloth_cloud(side, rng, pitch=0.25):
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) * pitch
    return np.stack([g[:, 0] - 1.0, rng.normal(0, 0.01, len(g)), g[:, 1] - 1.0], 1).astype(np.float32)


def trim(g):
    """fp32 gradient rounded to 14 mantissa bits (relative 3e-5, below the tests' 1e-4 bar): keeps each file under 1 MiB."""
    u = np.ascontiguousarray(g, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + (1 << 8)) & ~np.uint64((1 << 9) - 1)).astype(np.uint32)
    return u.view(np.float32)


def make_batch(cloud, tools, B, n_his, rng, noise=0.02):
    """Synthetic training batch shaped like DynDataset's (dataset.py): history of n_his frames, n_future = 3."""
    n_p, n_s = cloud.shape[0], tools.shape[0]
    N = n_p + n_s
    base = np.concatenate([cloud, tools], 0)
    state = np.zeros((B, n_his, N, 3), np.float32)
    for b in range(B):
        drift = rng.normal(0, 0.01, (1, 3)).astype(np.float32)
        for t in range(n_his):
            state[b, t] = base + drift * t + rng.normal(0, noise, (N, 3)).astype(np.float32)
    attrs = np.zeros((B, N, 2), np.float32)
    attrs[:, :n_p, 0] = 1
    attrs[:, n_p:, 1] = 1
    p_instance = np.ones((B, n_p, 1), np.float32)
    phys = rng.uniform(0.2, 0.8, (B, 1)).astype(np.float32)
    action = np.zeros((B, N, 3), np.float32)
    action[:, n_p:] = rng.normal(0, 0.05, (B, n_s, 3))
    state_future = (state[:, -1:, :n_p] + rng.normal(0, 0.02, (B, 3, n_p, 3))).astype(np.float32)
    eef_future = np.zeros((B, 2, N, 3), np.float32)
    eef_future[:, :, n_p:] = state[:, -1:, n_p:] + rng.normal(0, 0.03, (B, 2, n_s, 3))
    action_future = np.zeros((B, 2, N, 3), np.float32)
    action_future[:, :, n_p:] = rng.normal(0, 0.05, (B, 2, n_s, 3))
    return dict(state=state, attrs=attrs, p_instance=p_instance, physics_param=phys, action=action,
                state_future=state_future, eef_future=eef_future, action_future=action_future)


def train_loss(model, data, n_future, pkey, record=None, dtype=torch.float32):
    """train.py:86-121 for one batch (store_rest_state False): returns loss_sum; record collects every step's inputs."""
    d = {k: (v.to(dtype) if torch.is_floating_point(v) else v) for k, v in data.items()}
    future_state, future_eef, future_action = d["state_future"], d["eef_future"], d["action_future"]
    graph = dict(state=d["state"], attrs=d["attrs"], Rr=d["Rr"], Rs=d["Rs"], p_instance=d["p_instance"],
                 action=d["action"], **{pkey: d["physics_param"]})
    loss_sum = 0
    mse = torch.nn.MSELoss()
    for fi in range(n_future):
        gt_state = future_state[:, fi].clone()
        if record is not None:
            record.append((graph["state"].detach().numpy().copy(), graph["action"].detach().numpy().copy()))
        pred_state, pred_motion = MG.quiet(model, **graph)
        pred_state_p = pred_state[:, :gt_state.shape[1], :3].clone()
        loss_sum = loss_sum + mse(pred_state_p, gt_state)
        if fi < n_future - 1:
            next_state = future_eef[:, fi].clone().unsqueeze(1)
            next_state[:, -1, :pred_state_p.shape[1]] = pred_state_p
            graph["state"] = torch.cat([graph["state"][:, 1:], next_state], dim=1)
            graph["action"] = future_action[:, fi].clone()
    return loss_sum, pred_motion


def gen_case(name, refs, material, cloud, tools, B, topk, adj_thresh, connect_tools_all, seed, n_future=3, clamp_case=False):
    DynamicsPredictor, construct_edges, _, _ = refs
    dyn, _ = MG.load_cfg(material)
    rng = np.random.default_rng(seed)
    n_his = dyn["dataset_config"]["n_his"]
    model = MG.make_model(DynamicsPredictor, dyn, seed)
    W = TR.make_weights(seed, n_his=n_his)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    l2_scale, l2_shift = 1.0, np.zeros(3, np.float32)
    np_data = make_batch(cloud, tools, B, n_his, rng)
    n_p = cloud.shape[0]
    N = n_p + tools.shape[0]
    states = torch.from_numpy(np_data["state"][:, -1])
    mask = torch.ones(B, N, dtype=torch.bool)
    tool_mask = torch.zeros(B, N, dtype=torch.bool)
    tool_mask[:, n_p:] = True
    MG.assert_no_topk_boundary_tie(states, mask, tool_mask, adj_thresh, topk)
    Rr, Rs = MG.quiet(construct_edges, states, adj_thresh, mask, tool_mask, topk=topk, connect_tools_all=connect_tools_all)
    data = {k: torch.from_numpy(v) for k, v in np_data.items()}
    data.update(Rr=Rr, Rs=Rs)
    pkey = f"{material}_physics_param"
    if clamp_case:
        # scale + shift non_rigid_predictor.linear_2 so that |motion| passes 100 on about half of the rows, both signs
        with torch.no_grad():
            _, mo = MG.quiet(model, state=data["state"], attrs=data["attrs"], Rr=Rr, Rs=Rs, p_instance=data["p_instance"],
                             action=data["action"], **{pkey: data["physics_param"]})
        mo = mo.reshape(-1, 3).numpy().astype(np.float64)
        med = np.median(mo, 0)
        l2_scale = np.float32(100.0 / np.quantile(np.abs(mo - med), 0.5))
        l2_shift = (-med * l2_scale).astype(np.float32)
        with torch.no_grad():
            model.non_rigid_predictor.linear_2.weight.mul_(torch.tensor(l2_scale))
            model.non_rigid_predictor.linear_2.bias.mul_(torch.tensor(l2_scale)).add_(torch.from_numpy(l2_shift))
    store = {"w_seed": np.int64(seed), "l2_scale": np.float32(l2_scale), "l2_shift": l2_shift}
    store.update(np_data)
    MG.pack_edges("", MG.edges_from_R(Rr, Rs), store)
    store["n_future"] = np.int32(n_future)
    store["pstep"] = np.int32(dyn["model_config"]["pstep"])

    model.train()
    d0 = dict(data)
    d0["state"] = data["state"].clone().requires_grad_(True)
    steps = []
    loss, motion = train_loss(model, d0, n_future, pkey, record=steps)
    loss.backward()
    store["loss_sum"] = np.float64(loss.item())
    g32 = {k: p.grad.numpy().copy() for k, p in model.named_parameters()}
    for k, g in g32.items():
        store["g::" + k] = trim(g)
    store["dstate0"] = d0["state"].grad.numpy().copy()
    for i, (s, a) in enumerate(steps):
        store[f"step{i}::state"] = s
        store[f"step{i}::action"] = a
    store["pred_motion"] = motion.detach().numpy().copy()

    # float64 gradients of the same model (the yardstick of both fp32 implementations)
    try:
        m64 = copy.deepcopy(model).double()
        m64.zero_grad()
        d64 = dict(data)
        d64["state"] = data["state"].double().clone().requires_grad_(True)
        l64, _ = train_loss(m64, d64, n_future, pkey, dtype=torch.float64)
        l64.backward()
        for k, p in m64.named_parameters():   # the reference's own fp32 error per tensor (the float64 gradients themselves
            store["err64::" + k] = np.float64(np.abs(g32[k] - p.grad.numpy()).max())   # are recomputed by the tests)
        store["dstate0_64"] = d64["state"].grad.numpy().copy()
        store["loss_sum_64"] = np.float64(l64.item())
    except Exception as e:  # noqa: BLE001
        print(f"{name}: model.double() did not run ({type(e).__name__}: {e}); no float64 gradients recorded")

    # loss curve of 5 Adam steps on this batch (train.py:67,93-124)
    m = copy.deepcopy(MG.make_model(DynamicsPredictor, dyn, seed))
    m.load_state_dict(model.state_dict())
    opt = torch.optim.Adam(m.parameters(), lr=0.001)
    curve = []
    m.train()
    for _ in range(5):
        opt.zero_grad()
        ls, _ = train_loss(m, data, n_future, pkey)
        ls.backward()
        opt.step()
        curve.append(ls.item())
    store["adam_losses"] = np.array(curve, np.float64)

    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **store)
    extra = ""
    if clamp_case:
        mo = store["pred_motion"]
        extra = f", motions > 100: {(mo > 100).sum()}, < -100: {(mo < -100).sum()}, inside: {(np.abs(mo) <= 100).sum()}"
    print(f"{name}: B={B} N={N} edges/graph={store['n_edges'].tolist()} loss={store['loss_sum']:.6g} "
          f"adam={np.round(curve, 6).tolist()} -> {os.path.getsize(path) / 1e6:.2f} MB{extra}")


def main():
    refs = MG.import_reference()
    torch.set_num_threads(8)
    rng = np.random.default_rng(7)
    cloud = rope_cloud(100, rng)
    tool = np.array([[cloud[50, 0], 0.02, cloud[50, 2] + 0.15]], np.float32)
    gen_case("train_rope", refs, "rope", cloud, tool, B=4, topk=10, adj_thresh=0.5, connect_tools_all=False, seed=11)
    cc = cloth_cloud(8, rng)
    tools = np.array([[cc[27, 0], 0.05, cc[27, 2]], [cc[36, 0], 0.05, cc[36, 2]]], np.float32)
    gen_case("train_cloth", refs, "cloth", cc, tools, B=3, topk=8, adj_thresh=0.3, connect_tools_all=True, seed=12)
    gen_case("train_clamp", refs, "rope", cloud, tool, B=2, topk=10, adj_thresh=0.5, connect_tools_all=False, seed=13,
             n_future=1, clamp_case=True)


if __name__ == "__main__":
    main()
