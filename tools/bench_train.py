#!/usr/bin/env python3
"""Training-iteration benchmark: ms per iteration of the reference's training configuration (src/dynamics/train/train.py:86-124
with config/dynamics/rope.yaml: batch 128, 100 object particles + 1 tool, topk 10, max_nR 1000, n_future 3), i.e. three chained
forwards, loss_sum.backward() and one Adam step (lr 1e-3).

Three variants on the same GPU in the same process, alternated round by round:
  engine   adaptigraph_amd.DynamicsPredictor under autograd (ag_forward + ag_backward) + torch.optim.Adam
  fused    adaptigraph_amd.TrainStep.step with max_edges given (ag_train_step + ag_adam_step: enqueue only)
  torch    tests/train_restate.py in fp32 under torch autograd (index gathers + index_add; the reference itself stays on the host)
and the model FLOPs per iteration from the shapes (forward as the reference computes it: the relation propagator on the
concatenated 450-wide input; backward = 2x forward, plus one recomputed forward for the engine and the fused step).  Host
waits per iteration are DECLARED, not observed: the tool counts its calls of the C-ABI entries and multiplies by what the blocking
table of include/adaptigraph_amd.h says each one waits (ag_forward 1, ag_backward 2, ag_ctx_load_weights 1, the fused entries 0).
That the fused step really does not wait is what tests/test_gpu_train_step.py::test_step_returns_while_the_stream_is_busy shows.

  python tools/bench_train.py [--rounds 5] [--iters 5] [--warmup 3] [--out FILE]
  python tools/bench_train.py --only engine --rounds 1 --iters 3    (e.g. under rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adaptigraph_amd as ag  # noqa: E402
import train_restate as TR  # noqa: E402

CFG = dict(verbose=False, nf_particle=150, nf_relation=150, nf_effect=150, nf_physics=10, attr_dim=2, state_dim=0, offset_dim=0,
           action_dim=3, density_dim=0, pstep=3, sequence_len=4, rel_particle_dim=0, rel_attr_dim=2, rel_group_dim=1,
           rel_distance_dim=3, rel_density_dim=0)


def make_batch(dev, B=128, n_p=100, n_his=4, seed=0):
    """A rope batch shaped like DynDataset's (fps radius ~0.2, adjacency radius 0.5, rope.yaml)."""
    rng = np.random.default_rng(seed)
    N = n_p + 1
    t = np.linspace(0, 1, n_p)
    state = np.zeros((B, n_his, N, 3), np.float32)
    for b in range(B):
        cloud = np.stack([-10 + 20 * t, 0 * t, 2.0 * np.sin(6 * t + rng.uniform(0, 6))], 1) + rng.normal(0, 0.02, (n_p, 3))
        tool = cloud[rng.integers(n_p)] + np.array([0, 0.1, 0.2])
        for k in range(n_his):
            state[b, k] = np.concatenate([cloud, tool[None]], 0) + rng.normal(0, 0.01, (N, 3)) + 0.01 * k
    attrs = np.zeros((B, N, 2), np.float32)
    attrs[:, :n_p, 0] = 1
    attrs[:, n_p:, 1] = 1
    action = np.zeros((B, N, 3), np.float32)
    action[:, n_p:] = rng.normal(0, 0.05, (B, 1, 3))
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)   # noqa: E731
    mask = torch.ones(B, N, dtype=torch.bool, device=dev)
    tool = torch.zeros(B, N, dtype=torch.bool, device=dev)
    tool[:, n_p:] = True
    edges = ag.construct_edges_index(tt(state[:, -1]), 0.5, mask, tool, topk=10, edge_cap=1000)
    ne = edges.n_edges.cpu().numpy()
    assert ne.max() <= 1000, ne.max()
    future = state[:, -1:, :n_p] + rng.normal(0, 0.02, (B, 3, n_p, 3))
    eef = np.zeros((B, 2, N, 3), np.float32)
    eef[:, :, n_p:] = state[:, -1:, n_p:]
    return dict(state=tt(state), attrs=tt(attrs), action=tt(action), p_instance=tt(np.ones((B, n_p, 1))),
                phys_physics_param=tt(rng.uniform(0.2, 0.8, (B, 1))), edges=edges, state_future=tt(future),
                eef_future=tt(eef), action_future=tt(np.zeros((B, 2, N, 3))), n_p=n_p, ne=ne)


def engine_variant(dev, data, W):
    model = ag.DynamicsPredictor(CFG, {"material_index": {"rope": 0}, "rope": {"physics_params": [{"name": "s", "use": True}]}},
                                 {"n_his": 4, "materials": ["rope"]}, dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    model.to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=0.001)
    g = {k: data[k] for k in ("attrs", "p_instance", "phys_physics_param", "edges")}

    def it():
        opt.zero_grad()
        loss = TR.chain_loss(lambda s, a: model(state=s, action=a, **g), data, 3)
        loss.backward()
        opt.step()
        return loss
    return it


def fused_variant(dev, data, W):
    model = ag.DynamicsPredictor(CFG, {"material_index": {"rope": 0}, "rope": {"physics_params": [{"name": "s", "use": True}]}},
                                 {"n_his": 4, "materials": ["rope"]}, dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    ts = ag.TrainStep(model.to(dev), lr=0.001, n_future=3)
    batch = {k: data[k] for k in ("state", "attrs", "action", "p_instance", "phys_physics_param", "edges", "state_future",
                                  "eef_future", "action_future")}
    max_edges = int(data["ne"].max())

    def it():
        return ts.step(batch, max_edges=max_edges)
    return it


WAITS = {"ag_forward": 1, "ag_backward": 2, "ag_ctx_load_weights": 1, "ag_train_step": 0, "ag_adam_step": 0,
         "ag_ctx_load_weights_device": 0}
CALLS = {k: 0 for k in WAITS}


def count_calls():
    """Wrap the C-ABI entries of the loaded library with call counters (the library object is shared by every Engine)."""
    from adaptigraph_amd import _lib
    lib = _lib.load()
    for name in WAITS:
        fn = getattr(lib, name)

        def wrapped(*a, _fn=fn, _name=name):
            CALLS[_name] += 1
            return _fn(*a)
        setattr(lib, name, wrapped)


def torch_variant(dev, data, W):
    Wt = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in W.items()}
    opt = torch.optim.Adam(list(Wt.values()), lr=0.001)
    B, N = data["attrs"].shape[:2]
    n_p = data["n_p"]
    e = data["edges"]
    ne = data["ne"]
    recv = torch.cat([e.recv[b, :ne[b]].long() + b * N for b in range(B)])
    send = torch.cat([e.send[b, :ne[b]].long() + b * N for b in range(B)])
    phys = torch.zeros(B, N, device=dev)
    phys[:, :n_p] = data["phys_physics_param"]
    group = torch.zeros(B, N, 1, device=dev)
    group[:, :n_p] = 1

    def it():
        opt.zero_grad()
        loss = TR.chain_loss(lambda s, a: TR.forward(Wt, s, data["attrs"], a, phys, group, recv, send, n_p, 3), data, 3)
        loss.backward()
        opt.step()
        return loss
    return it


def model_flops(B, N, n_p, E, n_his=4, pstep=3, nf=150):
    R = 5 + 3 * n_his
    n, e = B * N, B * E
    enc = 2 * n * (6 * nf + 2 * nf * nf) + 2 * e * (R * nf + 2 * nf * nf)
    prop = pstep * (2 * e * 3 * nf * nf + 2 * n * 2 * nf * nf)
    head = 2 * B * n_p * (2 * nf * nf + 3 * nf)
    return enc + prop + head


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--only", choices=["engine", "fused", "torch"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    data = make_batch(dev, B=a.batch)
    W = TR.make_weights(0)
    count_calls()
    makers = {"engine": engine_variant, "fused": fused_variant, "torch": torch_variant}
    variants = {k: mk(dev, data, W) for k, mk in makers.items() if a.only in (None, k)}
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    losses = {}
    waits = {k: 0 for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            before = dict(CALLS)
            t0 = time.perf_counter()
            for _ in range(a.iters):
                loss = fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
            waits[k] += sum((CALLS[n] - before[n]) * WAITS[n] for n in WAITS)
            losses[k] = float(loss)
    B, N = data["attrs"].shape[:2]
    E = float(data["ne"].mean())
    fwd = model_flops(B, N, data["n_p"], E)
    flops = {"engine": 3 * (4 * fwd), "fused": 3 * (4 * fwd), "torch": 3 * (3 * fwd)}   # n_future forwards; backward 2x; the engine paths recompute once more
    res = {"tool": "bench_train", "config": dict(B=B, N=N, n_p=data["n_p"], topk=10, max_nR=1000, edges_mean=E,
                                                 edges_max=int(data["ne"].max()), n_future=3, pstep=3, optimizer="Adam lr 1e-3"),
           "device": torch.cuda.get_device_name(dev), "rounds": a.rounds, "iters_per_round": a.iters,
           "model_gflop_per_forward": fwd / 1e9,
           "note": "FLOPs from shapes: forward as the reference computes it (relation propagator on the 450-wide concatenation); "
                   "backward 2x forward; the engine and the fused step also recompute one forward inside the backward; host_waits_per_iter_declared = calls x the header's blocking table, not a measurement"}
    for k in variants:
        ms = float(np.median(times[k]))
        res[k] = {"ms_per_iter_median": ms, "ms_per_iter_rounds": [round(x, 3) for x in times[k]], "last_loss": losses[k],
                  "gflop_per_iter": flops[k] / 1e9, "achieved_tflops": flops[k] / (ms * 1e-3) / 1e12}
        if k != "torch":
            res[k]["host_waits_per_iter_declared"] = waits[k] / (a.rounds * a.iters)
    if "engine" in res and "torch" in res:
        res["torch_over_engine"] = res["torch"]["ms_per_iter_median"] / res["engine"]["ms_per_iter_median"]
    if "fused" in res and "torch" in res:
        res["torch_over_fused"] = res["torch"]["ms_per_iter_median"] / res["fused"]["ms_per_iter_median"]
    if "fused" in res and "engine" in res:
        res["engine_over_fused"] = res["engine"]["ms_per_iter_median"] / res["fused"]["ms_per_iter_median"]
        r = res["engine"]["ms_per_iter_rounds"]
        res["engine_round_spread_ms"] = max(r) - min(r)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
