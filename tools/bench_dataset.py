#!/usr/bin/env python3
"""Batch-build benchmark: ms per DeviceDynDataset.batch() of the reference's rope training configuration (config/dynamics/
rope.yaml: batch 128, max_nobj 100, one tool point, topk 10, max_nR 1000, noise and rotation on) on synthetic episodes of 600
and of 2000 raw points, in one process:

  batch          ds.batch(idx) alone, wall time per call (a call ends with its own wait for the edge counts, so nothing of it
                 is still in flight when the next begins), and the HIP-event time of each kernel family inside it (ag_ctx_kernel_stats: fps, assemble,
                 edge_count, edge_emit), measured in a separate pass
  step           TrainStep.step on a fixed batch (the iteration a loader has to keep up with)
  loop           next(loader) + TrainStep.step per iteration, with prefetch (batch k+1 is built on the dataset's side stream while
                 step k runs) and without
  cpu            tests/dataset_restate.py (numpy) on the same samples and draws, on this machine's CPU: the reference itself is not
                 where the GPU is

A second leg ("softbody") follows config/dynamics/softbody.yaml's dataset entries (n_his 5, rest frame, max_nobj 300, five tool
points, topk 10, max_nR 3500, tool-to-non-fixed rule, knn_range [0.4, 1.0]): ds.batch on the batched rule path
(ag_edges_nonfixed_rule_graphs, back-off in rounds) against ds.batch(..., per_sample_edges=True), the graph-by-graph path,
alternated round by round in one process on the same samples and draws; ms per call, the ratio, the read-backs of a batch and the
HIP-event time of the kernel families, "rule" among them.

There is no pass / fail threshold.  The claim to confirm or refute: a batch builds in less than one TrainStep iteration, so that
prefetch hides it ("loop_prefetch_minus_step_ms" is then about zero); if not, "kernels" says which phase dominates.

  python tools/bench_dataset.py [--rounds 5] [--iters 10] [--warmup 3] [--batch 128] [--points 600,2000] [--out FILE]
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
import dataset_restate as DR  # noqa: E402
import train_restate as TR  # noqa: E402
from bench_train import CFG  # noqa: E402

DATASET = {"n_his": 4, "n_future": 3, "materials": ["rope"],
           "datasets": [{"name": "rope", "max_nobj": 100, "max_nR": 1000, "fps_radius_range": [0.18, 0.22],
                         "adj_radius_range": [0.48, 0.52], "topk": 10, "connect_tool_all": False}],
           "randomness": {"use": True, "state_noise": {"train": 0.05, "valid": 0.0}, "phys_noise": {"train": 0.0, "valid": 0.0}}}
MATERIAL = {"material_index": {"rope": 0}, "rope": {"physics_params": [{"name": "stiffness", "use": True}]}}
FAMILIES = ["fps", "assemble", "edge_count", "edge_emit"]
SOFT_DATASET = {"n_his": 5, "n_future": 3, "store_rest_state": True, "materials": ["softbody"],
                "datasets": [{"name": "softbody", "max_nobj": 300, "max_nR": 3500, "fps_radius_range": [0.2, 0.24],
                              "adj_radius_range": [0.48, 0.52], "topk": 10, "connect_tool_all": False, "connect_tool_surface": False,
                              "connect_tool_surface_ratio": 1.0, "connect_tool_all_non_fixed": True, "knn_range": [0.4, 1.0],
                              "min_knn": 0.4, "knn_increment": 0.1}],
                "randomness": {"use": False, "state_noise": {"train": 0.05, "valid": 0.0}, "phys_noise": {"train": 0.0, "valid": 0.0}}}
SOFT_MATERIAL = {"material_index": {"softbody": 0}, "softbody": {"physics_params": [{"name": "stiffness", "use": True}]}}


def make_episodes(points, n_epis=8, T=38, seed=0):
    """Ropes of `points` raw particles about 20 units long (so that ~100 samples at radius 0.2 cover them, as in training).
    8 episodes x 32 windows = 256 pairs: an epoch is whole batches of 128 (main() refuses a batch size that leaves a short one,
    which would make a loader iteration cheaper than the step it is compared with)."""
    rng = np.random.default_rng(seed)
    obj, eef, phys, pairs = [], [], [], []
    for e in range(n_epis):
        t = np.sort(rng.uniform(0, 1, points))
        base = np.stack([-10 + 20 * t, 0.02 + 0 * t, 2.0 * np.sin(6 * t + rng.uniform(0, 6))], 1) + rng.normal(0, 0.02, (points, 3))
        drift = rng.normal(0, 0.01, (1, 3))
        obj.append(np.stack([base + drift * k + rng.normal(0, 0.004, base.shape) for k in range(T)]).astype(np.float32))
        tool = base[rng.integers(points)] + np.array([0, 0.1, 0.2])
        eef.append(np.stack([tool[None] + 0.03 * k for k in range(T)]).astype(np.float32))
        phys.append({"rope": np.array([rng.uniform(0.2, 0.8)], np.float32)})
        pairs += [[e] + list(range(s, s + 7)) for s in range(T - 6)]
    return np.array(pairs), phys, obj, eef


def make_soft_episodes(points=600, n_epis=8, T=38, seed=0):
    """Blocks of `points` raw particles (2.4 x 0.7 x 2.4 units) that sag a little frame by frame, five tool points in a row that
    come down on the top face: farthest-point sampling at radius ~0.22 keeps a few hundred of them."""
    rng = np.random.default_rng(seed)
    obj, eef, phys, pairs = [], [], [], []
    for e in range(n_epis):
        base = rng.uniform(0, 1, (points, 3)) * [2.4, 0.7, 2.4] - [1.2, 0.0, 1.2]
        drift = rng.normal(0, 0.004, (1, 3))
        obj.append(np.stack([base + drift * k + rng.normal(0, 0.003, base.shape) for k in range(T)]).astype(np.float32))
        row = np.array([[0.5, 0.9, 0.0], [-0.5, 0.9, 0.0], [0.0, 0.9, 0.0], [0.25, 0.9, 0.0], [-0.25, 0.9, 0.0]]) + [rng.uniform(-0.5, 0.5), 0, rng.uniform(-0.5, 0.5)]
        eef.append(np.stack([row - [0.0, 0.008 * k, 0.0] for k in range(T)]).astype(np.float32))
        phys.append({"softbody": np.array([rng.uniform(0.2, 0.8)], np.float32)})
        pairs += [[e] + list(range(s, s + 8)) for s in range(T - 7)]
    return np.array(pairs), phys, obj, eef


def run_softbody(a, dev):
    pairs, phys, obj, eef = make_soft_episodes()
    ds = ag.DeviceDynDataset(SOFT_DATASET, SOFT_MATERIAL, pairs, phys, obj, eef, dev)
    B = a.batch
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    idx = np.random.default_rng(1).integers(0, len(ds), B)
    dr = ds.draws(idx, generator=g)
    sync = torch.cuda.synchronize
    variants = {"batched": lambda: ds.batch(idx, draws=dr), "per_sample": lambda: ds.batch(idx, draws=dr, per_sample_edges=True)}
    data = {k: fn() for k, fn in variants.items()}                                       # warm-up, and the two agree
    na, nb = data["batched"]["edges"].n_edges.cpu().numpy(), data["per_sample"]["edges"].n_edges.cpu().numpy()
    same = bool(np.array_equal(na, nb)) and all(
        torch.equal(data["batched"]["edges"].send[b, :na[b]], data["per_sample"]["edges"].send[b, :na[b]]) for b in range(B))
    variants["batched"]()
    res = {"points": 600, "pairs": len(ds), "B": B, "N": ds.N, "n_obj_mean": float(data["batched"]["obj_mask"].sum(1).float().mean()),
           "edges_mean": float(na.mean()), "edges_max": int(na.max()), "edges_equal": same, "last_waits": ds.last_waits,
           "attempts_per_graph_mean": float(np.mean([len(t) for t in ds.last_trail])),
           "attempts_per_graph_max": int(max(len(t) for t in ds.last_trail)),
           "graphs_backed_off": int(sum(len(t) > 1 for t in ds.last_trail))}
    times = {k: [] for k in variants}
    iters = {"batched": a.iters, "per_sample": 1}
    for _ in range(a.rounds):
        for k, fn in variants.items():                                                   # alternated within the round
            sync()
            t0 = time.perf_counter()
            for _ in range(iters[k]):
                fn()
            sync()
            times[k].append((time.perf_counter() - t0) * 1e3 / iters[k])
    for k, v in times.items():
        res[k] = {"ms_median": float(np.median(v)), "ms_rounds": [round(x, 3) for x in v], "calls_per_round": iters[k]}
    res["per_sample_over_batched"] = res["per_sample"]["ms_median"] / res["batched"]["ms_median"]
    fams = FAMILIES + ["rule"]
    ds.engine.set_profiling(fams)
    ds.engine.reset_stats()
    for _ in range(a.iters):
        variants["batched"]()
    sync()
    res["kernels"] = {}
    for f in fams:
        ms, n = ds.engine.kernel_stats(f)
        res["kernels"][f] = {"ms_per_batch": ms / a.iters, "launches_per_batch": n / a.iters}
    ds.engine.set_profiling([])
    return res


def timed(fn, rounds, iters, sync):
    out = []
    for _ in range(rounds):
        sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return {"ms_median": float(np.median(out)), "ms_rounds": [round(x, 3) for x in out]}


def run_config(a, dev, points):
    pairs, phys, obj, eef = make_episodes(points)
    ds = ag.DeviceDynDataset(DATASET, MATERIAL, pairs, phys, obj, eef, dev)
    model = ag.DynamicsPredictor(CFG, MATERIAL, {"n_his": 4, "materials": ["rope"]}, dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in TR.make_weights(0).items()})
    ts = ag.TrainStep(model.to(dev), lr=0.001, n_future=3)
    B = a.batch
    if len(ds) % B:
        raise SystemExit(f"{len(ds)} pairs do not divide into batches of {B}: the loop legs would time short batches")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rng = np.random.default_rng(1)
    idx = rng.integers(0, len(ds), B)
    sync = torch.cuda.synchronize
    res = {"points": points, "pairs": len(ds), "B": B}
    # ---- batch() alone
    for _ in range(a.warmup):
        data = ds.batch(idx, generator=g)
    ne = data["edges"].n_edges.cpu().numpy()
    res["edges_mean"], res["edges_max"] = float(ne.mean()), int(ne.max())
    res["n_obj_mean"] = float(data["obj_mask"].sum(1).float().mean())
    res["backoff_graphs"] = int(sum(len(t) > 1 for t in ds.last_trail))
    fast = a.iters * a.fast_factor                          # sub-millisecond calls: enough of them per timed window
    res["batch"] = timed(lambda: ds.batch(idx, generator=g), a.rounds, fast, sync)
    dr = ds.draws(idx, generator=g)
    res["batch_given_draws"] = timed(lambda: ds.batch(idx, draws=dr), a.rounds, fast, sync)
    res["draws"] = timed(lambda: ds.draws(idx, generator=g), a.rounds, fast, sync)
    ds.engine.set_profiling(FAMILIES)
    ds.engine.reset_stats()
    n_prof = fast
    for _ in range(n_prof):
        ds.batch(idx, draws=dr)
    sync()
    res["kernels"] = {}
    for f in FAMILIES:
        ms, n = ds.engine.kernel_stats(f)
        res["kernels"][f] = {"ms_per_batch": ms / n_prof, "launches_per_batch": n / n_prof}
    ds.engine.set_profiling([])
    # ---- the training iteration on a fixed batch
    for _ in range(a.warmup):
        ts.step(data, max_edges=data["max_edges"])
    res["step"] = timed(lambda: ts.step(data, max_edges=data["max_edges"]), a.rounds, a.iters, sync)
    # ---- loader + step
    for name, prefetch in (("loop_prefetch", True), ("loop_no_prefetch", False)):
        it = ds.loader(B, True, generator=g, prefetch=prefetch)

        def one(it=it):
            d = next(it)
            ts.step(d, max_edges=d["max_edges"])
        for _ in range(a.warmup):
            one()
        res[name] = timed(one, a.rounds, a.iters, sync)
        it.close()
    ts.check()
    # ---- the numpy restatement on this machine's CPU, same samples and draws
    npd = {k: (None if getattr(dr, k) is None else getattr(dr, k).cpu().numpy()) for k in DR.DRAW_KEYS}
    n_cpu = min(B, a.cpu_samples)
    t0 = time.perf_counter()
    DR.restate_batch(DATASET, MATERIAL, pairs, phys, obj, eef, idx[:n_cpu], {k: (None if v is None else v[:n_cpu]) for k, v in npd.items()})
    res["cpu_restate"] = {"ms_per_batch_scaled": (time.perf_counter() - t0) * 1e3 * B / n_cpu, "samples_timed": n_cpu,
                          "threads": torch.get_num_threads()}
    res["batch_over_step"] = res["batch"]["ms_median"] / res["step"]["ms_median"]
    for name in ("loop_prefetch", "loop_no_prefetch"):     # every loop iteration is a full batch of B: comparable with "step"
        res[name + "_minus_step_ms"] = res[name]["ms_median"] - res["step"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--points", default="600,2000")
    ap.add_argument("--cpu-samples", type=int, default=32)
    ap.add_argument("--fast-factor", type=int, default=40, help="the sub-millisecond rows run iters x this many calls per round")
    ap.add_argument("--out", default=None)
    ap.add_argument("--softbody", choices=["also", "only", "no"], default="also", help="the softbody leg: with the rope configs, alone, or not")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"tool": "bench_dataset", "device": torch.cuda.get_device_name(dev), "rounds": a.rounds, "iters_per_round": a.iters,
           "config": "rope.yaml dataset entries, B %d, synthetic episodes" % a.batch,
           "note": "one process; ms per call, median over the rounds; batch() ends with its own wait for the edge counts; the batch / "
                   "draws rows time iters x fast_factor calls per round; 'kernels' are HIP-event times from a separate pass; every "
                   "loop iteration is a full batch (shuffled with the device generator); cpu_restate is the numpy restatement on this "
                   "machine, not the reference", "fast_factor": a.fast_factor,
           "configs": [] if a.softbody == "only" else [run_config(a, dev, int(p)) for p in a.points.split(",")]}
    if a.softbody != "no":
        res["softbody"] = run_softbody(a, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
