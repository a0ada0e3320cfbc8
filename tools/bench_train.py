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
  python tools/bench_train.py --parts 1,2,4 --out FILE
      the parts leg INSTEAD of the three variants: TrainStep.step on the batch (the one-call step, the base every other figure
      is compared with) alternated in the same process with the same batch as K equal parts through accumulate ... apply, for
      every K given; and a mixed-size batch (half the graphs built with topk 10, half with topk 5) as one call with the common
      max_edges against two buckets with their own.  --parts 4 --no-mixed --only-parts under rocprofv3 gives the 4-part kernel table.
  python tools/bench_train.py --losses mse:1,chamfer:0.5,hausdorff:0.25 --out FILE
      the loss-list leg INSTEAD of the three variants, four legs alternated in the same process on the same batch: fused_default
      (TrainStep(), the MSE step as it always was), fused_losses (TrainStep(losses=...): ag_train_step_losses), engine_default and
      engine_losses (the autograd path with MSE alone and with the same list, its set terms being adaptigraph_amd.ChamferLoss /
      HausdorffLoss).  --only-losses NAME runs one of them (for a kernel trace).
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


def make_batch(dev, B=128, n_p=100, n_his=4, seed=0, topk=10):
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
    edges = ag.construct_edges_index(tt(state[:, -1]), 0.5, mask, tool, topk=topk, edge_cap=1000)
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


BATCH_KEYS = ("state", "attrs", "action", "p_instance", "phys_physics_param", "state_future", "eef_future", "action_future")


def slice_batch(data, lo, hi):
    """Graphs [lo, hi) of a make_batch dict as a TrainStep data dict, and their largest edge count."""
    from adaptigraph_amd.graph import EdgeList
    e = data["edges"]
    d = {k: data[k][lo:hi].contiguous() for k in BATCH_KEYS}
    d["edges"] = EdgeList(e.recv[lo:hi].contiguous(), e.send[lo:hi].contiguous(), e.row_ptr[lo:hi].contiguous(),
                          e.n_edges[lo:hi].contiguous(), e.N)
    return d, int(data["ne"][lo:hi].max())


def concat_batches(a, b):
    """Two make_batch dicts (same N and edge capacity) as one batch, a's graphs first."""
    from adaptigraph_amd.graph import EdgeList
    d = {k: torch.cat([a[k], b[k]]) for k in BATCH_KEYS}
    ea, eb = a["edges"], b["edges"]
    d["edges"] = EdgeList(*[torch.cat([getattr(ea, k), getattr(eb, k)]) for k in ("recv", "send", "row_ptr", "n_edges")], ea.N)
    d["ne"], d["n_p"] = np.concatenate([a["ne"], b["ne"]]), a["n_p"]
    return d


def parts_variants(dev, data, W, ks, mixed):
    """name -> (callable of one iteration, description).  Every leg has a TrainStep of its own from the same weights."""
    def new_ts():
        model = ag.DynamicsPredictor(CFG, {"material_index": {"rope": 0}, "rope": {"physics_params": [{"name": "s", "use": True}]}},
                                     {"n_his": 4, "materials": ["rope"]}, dev)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
        return ag.TrainStep(model.to(dev), lr=0.001, n_future=3)
    B = data["attrs"].shape[0]
    out = {}
    whole, bound = slice_batch(data, 0, B)
    ts0 = new_ts()
    out["step"] = (lambda: ts0.step(whole, max_edges=bound), f"TrainStep.step, 1 x {B}, max_edges {bound}")
    for k in ks:
        cuts = [slice_batch(data, i * B // k, (i + 1) * B // k) for i in range(k)]
        ts = new_ts()
        out[f"parts_{k}"] = (lambda ts=ts, cuts=cuts: ts.step_parts([c[0] for c in cuts], max_edges=[c[1] for c in cuts]),
                             f"accumulate x {k} + apply, {k} x {B // k}, max_edges {[c[1] for c in cuts]}")
    if mixed:
        a, b = make_batch(dev, B=B // 2, seed=1, topk=10), make_batch(dev, B=B - B // 2, seed=2, topk=5)
        mix = concat_batches(a, b)
        whole_m, bound_m = slice_batch(mix, 0, B)
        buckets = [slice_batch(mix, 0, B // 2), slice_batch(mix, B // 2, B)]
        ts1, ts2 = new_ts(), new_ts()
        out["mixed_common"] = (lambda: ts1.step(whole_m, max_edges=bound_m),
                               f"mixed batch (topk 10 | topk 5) as one call, max_edges {bound_m}, mean edges {float(mix['ne'].mean()):.1f}")
        out["mixed_buckets"] = (lambda: ts2.step_parts([c[0] for c in buckets], max_edges=[c[1] for c in buckets]),
                                f"the same batch as two buckets, max_edges {[c[1] for c in buckets]}")
    return out


def run_parts(a, dev, data, W):
    ks = [int(x) for x in a.parts.split(",")]
    legs = parts_variants(dev, data, W, ks, not a.no_mixed)
    if a.only_parts:
        legs = {k: v for k, v in legs.items() if k.startswith("parts_")}
    for fn, _ in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times, losses = {k: [] for k in legs}, {}
    for _ in range(a.rounds):
        for k, (fn, _) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                loss = fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
            losses[k] = float(loss)
    res = {"tool": "bench_train --parts", "device": torch.cuda.get_device_name(dev), "rounds": a.rounds, "iters_per_round": a.iters,
           "config": dict(B=int(data["attrs"].shape[0]), N=int(data["attrs"].shape[1]), n_p=data["n_p"], n_future=3, pstep=3,
                          optimizer="Adam lr 1e-3", edges_mean=float(data["ne"].mean()), edges_max=int(data["ne"].max())),
           "note": "every leg in one process, alternated round by round; ms per optimiser step, median over the rounds; "
                   "'step' is the one-call TrainStep.step (ag_train_step + ag_adam_step), the base of every ratio"}
    for k, (_, what) in legs.items():
        r = times[k]
        res[k] = {"what": what, "ms_per_iter_median": float(np.median(r)), "ms_per_iter_rounds": [round(x, 3) for x in r],
                  "ms_min": min(r), "ms_max": max(r), "last_loss": losses[k]}
    if "step" in res:
        base = res["step"]
        for k in legs:
            if k.startswith("parts_"):
                res[k]["over_step"] = res[k]["ms_per_iter_median"] / base["ms_per_iter_median"]
        if "parts_1" in res:
            res["parts_1"]["inside_step_spread"] = bool(base["ms_min"] <= res["parts_1"]["ms_per_iter_median"] <= base["ms_max"])
    if "mixed_common" in res and "mixed_buckets" in res:
        res["mixed_buckets_over_common"] = res["mixed_buckets"]["ms_per_iter_median"] / res["mixed_common"]["ms_per_iter_median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def parse_losses(text):
    """'mse:1,chamfer:0.5' -> [("mse", 1.0), ("chamfer", 0.5)]; checked by LossSpec."""
    out = [(t.split(":")[0].strip(), float(t.split(":")[1])) for t in text.split(",")]
    ag.LossSpec(out)
    return out


def chain_loss_funcs(step, inp, n_future, loss_funcs):
    """TR.chain_loss with train.py:100-102's loss = sum(weight * func(pred, gt))."""
    state, action, n_p = inp["state"], inp["action"], inp["n_p"]
    loss = 0
    for fi in range(n_future):
        gt = inp["state_future"][:, fi]
        pred, _ = step(state, action)
        p = pred[:, :gt.shape[1], :3].clone()
        loss = loss + sum([w * func(p, gt) for func, w in loss_funcs])
        if fi < n_future - 1:
            nxt = inp["eef_future"][:, fi].clone().unsqueeze(1)
            nxt[:, -1, :n_p] = pred[:, :n_p]
            state = torch.cat([state[:, 1:], nxt], 1)
            action = inp["action_future"][:, fi]
    return loss


def run_losses(a, dev, data, W):
    losses = parse_losses(a.losses)
    mods = {"mse": torch.nn.MSELoss(), "chamfer": ag.ChamferLoss(), "hausdorff": ag.HausdorffLoss()}

    def new_model():
        model = ag.DynamicsPredictor(CFG, {"material_index": {"rope": 0}, "rope": {"physics_params": [{"name": "s", "use": True}]}},
                                     {"n_his": 4, "materials": ["rope"]}, dev)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
        return model.to(dev)
    batch = {k: data[k] for k in BATCH_KEYS + ("edges",)}
    max_edges = int(data["ne"].max())

    def fused(spec):
        ts = ag.TrainStep(new_model(), lr=0.001, n_future=3, losses=spec)
        return lambda: ts.step(batch, max_edges=max_edges)

    def engine(funcs):
        model = new_model().train()
        opt = torch.optim.Adam(model.parameters(), lr=0.001)
        g = {k: data[k] for k in ("attrs", "p_instance", "phys_physics_param", "edges")}

        def it():
            opt.zero_grad()
            loss = chain_loss_funcs(lambda s, x: model(state=s, action=x, **g), data, 3, funcs)
            loss.backward()
            opt.step()
            return loss
        return it
    legs = {"fused_default": fused(None), "fused_losses": fused(losses), "engine_default": engine([(mods["mse"], 1)]),
            "engine_losses": engine([(mods[n], w) for n, w in losses])}
    if a.only_losses:
        legs = {a.only_losses: legs[a.only_losses]}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times, last = {k: [] for k in legs}, {}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                loss = fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
            last[k] = float(loss.detach())
    res = {"tool": "bench_train --losses", "device": torch.cuda.get_device_name(dev), "rounds": a.rounds, "iters_per_round": a.iters,
           "losses": [[n, w] for n, w in losses],
           "config": dict(B=int(data["attrs"].shape[0]), N=int(data["attrs"].shape[1]), n_p=data["n_p"], n_future=3, pstep=3,
                          optimizer="Adam lr 1e-3", edges_mean=float(data["ne"].mean()), edges_max=int(data["ne"].max())),
           "note": "every leg in one process, alternated round by round; ms per optimiser step, median over the rounds"}
    for k, r in times.items():
        res[k] = {"ms_per_iter_median": float(np.median(r)), "ms_per_iter_rounds": [round(x, 3) for x in r], "ms_min": min(r),
                  "ms_max": max(r), "last_loss": last[k]}
    med = lambda k: res[k]["ms_per_iter_median"]   # noqa: E731
    if "fused_default" in res and "fused_losses" in res:
        res["set_terms_add_ms_fused"] = med("fused_losses") - med("fused_default")
    if "engine_default" in res and "engine_losses" in res:
        res["set_terms_add_ms_engine"] = med("engine_losses") - med("engine_default")
    if "fused_losses" in res and "engine_losses" in res:
        res["engine_losses_over_fused_losses"] = med("engine_losses") / med("fused_losses")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


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
    ap.add_argument("--parts", default=None, help="K[,K...]: the parts leg (see the module docstring)")
    ap.add_argument("--no-mixed", action="store_true", help="with --parts: leave the mixed-size batch out")
    ap.add_argument("--only-parts", action="store_true", help="with --parts: the K-part legs alone (for a kernel trace)")
    ap.add_argument("--losses", default=None, help="term:weight[,term:weight...]: the loss-list leg (see the module docstring)")
    ap.add_argument("--only-losses", choices=["fused_default", "fused_losses", "engine_default", "engine_losses"], default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    data = make_batch(dev, B=a.batch)
    W = TR.make_weights(0)
    if a.parts:
        return run_parts(a, dev, data, W)
    if a.losses:
        return run_losses(a, dev, data, W)
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
