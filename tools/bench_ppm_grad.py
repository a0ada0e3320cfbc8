#!/usr/bin/env python3
"""Physics-parameter fit benchmark: ms per optimize_grad iteration (one stacked masked rollout + one backward over
n_starts x 20 rows) at n_starts 1 and 8 on a 20-interaction rope problem (clouds and pushes drawn like the
ppm_dynamics_error fixture's), and for scale one dynamics_error call on the same problem (the gradient-free path: the fused
rollout + chamfer).  Reported, not asserted: the per-call host synchronisations of ag_forward / ag_backward_inputs (DESIGN.md
section 3.10) are part of the number.  fit1 / fit8: one PhysParamFit.step() (ag_ppm_grad_step + ag_ppm_adam_step, enqueue only;
the timed window ends in a device synchronise) on the same problem, alternated with grad1 / grad8 in the same process.

  python tools/bench_ppm_grad.py [--rounds 5] [--iters 5] [--warmup 2] [--out FILE]
  python tools/bench_ppm_grad.py --only fit8 --rounds 1 --iters 3     (e.g. under rocprofv3 --kernel-trace --stats)
  python tools/bench_ppm_grad.py --only fit8 --edge-rows 1100         (fit legs with PhysParamFit.edge_rows = 1100 instead of
                                                                       the builder's structural bound N * (topk + M))
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adaptigraph_amd as ag  # noqa: E402
from adaptigraph_amd import physics_param_optimizer as PPO  # noqa: E402
import train_restate as TR  # noqa: E402
from test_train import CFG  # noqa: E402


def rope_cloud(n, rng):
    t = np.linspace(0.0, 1.0, n)
    p = np.stack([-2.0 + 3.0 * t, np.zeros(n), 0.5 * np.sin(6.0 * t)], 1)
    return (p + rng.normal(0, 0.01, p.shape)).astype(np.float32)


def make_problem(dev, n=20, seed=41):
    rng = np.random.default_rng(seed)
    task = dict(adj_thresh=0.5, topk=10, connect_tools_all=False, sim_real_ratio=10, push_length=0.1, gripper_enable=False,
                max_n=1, max_nR=4000, n_his=4, eef_num=1, material="rope", pusher_points=[[0.0, 0.0, 0.12]],
                material_dims={"rope": 1}, material_indices={"rope": 0}, max_nobj=110)
    mat = {"material_index": {"rope": 0}, "rope": {"physics_params": [{"name": "p", "use": True}]}}
    model = ag.DynamicsPredictor(CFG, mat, {"n_his": 4, "materials": ["rope"]}, dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in TR.make_weights(seed).items()})
    ppm = types.SimpleNamespace(task_config=task, eef_num=1, material="rope", material_dims=task["material_dims"],
                                material_indices=task["material_indices"], physics_param={"rope": torch.tensor([0.5])},
                                adj_thresh=0.5, model=model.to(dev), device=dev)
    inits = [rope_cloud(int(c), rng) for c in rng.integers(70, 111, n)]
    reals = [(rope_cloud(int(c), rng) + np.float32([0.05, 0.0, 0.03])).astype(np.float32) for c in rng.integers(70, 111, n)]
    acts = []
    for cloud in inits:
        c = cloud.mean(0)
        acts.append(np.float32([c[0] + rng.uniform(-0.6, 0.6), c[2] + rng.uniform(-0.6, 0.6), rng.uniform(-3.14, 3.14),
                                rng.uniform(2.2, 4.8)]))
    return ppm, inits, reals, acts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["grad1", "grad8", "fit1", "fit8", "error"])
    ap.add_argument("--edge-rows", type=int)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ppm, inits, reals, acts = make_problem(dev)
    problem = PPO._problem(ppm, inits, reals, acts)
    fits = {}

    def fit_step(k):                                # the fit object is built once: the upload is not part of an iteration
        if k not in fits:
            fits[k] = ag.PhysParamFit(ppm, acts, inits, reals, n_starts=k, iterations=0)
            fits[k].edge_rows = a.edge_rows
        fits[k].step()

    legs = {"grad1": lambda: PPO._stacked_eval(PPO._starting_points([0.5], 1), ppm, problem),
            "fit1": lambda: fit_step(1),
            "grad8": lambda: PPO._stacked_eval(PPO._starting_points([0.5], 8), ppm, problem),
            "fit8": lambda: fit_step(8),
            "error": lambda: ag.dynamics_error([0.5], ppm, inits, reals, acts)}
    if a.only:
        legs = {a.only: legs[a.only]}
    times = {k: [] for k in legs}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    for _ in range(a.rounds):                       # legs alternated round by round: drift hits all of them alike
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / a.iters * 1e3)
    for fit in fits.values():
        fit.result()                                # raises if a step was skipped (a graph beyond max_nR)
    res = {"interactions": len(acts), "edge_rows": a.edge_rows, "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "ms": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
