#!/usr/bin/env python3
"""Eval-rollout benchmark: the open-loop validation rollout of the reference's rope configuration (100 + 1 particles, topk 10,
max_nR 1000) for 64 rollouts of 30 steps on synthetic episodes, three ways in one process, alternated round by round:

  batched      rollout_eval_batch(model, ds, idx): one ag_eval_step and one read-back per step for all 64
  sequential   64 rollout_eval calls on the rows of the same start batch, the caller doing the ground-truth lookup and the error
               with torch ops on the device - how this work was done before rollout_eval_batch
  per_graph    rollout_eval_batch(..., per_graph=True)

--config softbody runs softbody.yaml's entries instead (n_his 5, rest frame, pstep 4, max_nobj 300, five tool points, topk 10,
max_nR 3500, tool-to-non-fixed rule, kNN range): the batched variant then advances the rule graphs together
(ag_edges_nonfixed_rule_graphs per step, back-off in rounds), per_graph is the graph-by-graph path these configs took before; the
sequential variant is the rope leg's only.  --config surface is the softbody leg with connect_tool_surface: True at ratio 0.8: the
batched variant chains ag_edges_surface_rule_graphs behind the non-fixed rule in every step and every back-off attempt (kernel
family "surface"), and the start graphs get the eval script's own rule.

All three include building the start batch.  Reported: ms per variant (median of the rounds), per step and per rollout, the ratio
to the sequential path, and - from a separate pass - the HIP-event time of each kernel family inside the batched path
(ag_ctx_kernel_stats) next to one plain forward at B = 64.  No pass / fail threshold.  The expectation to confirm or refute: a
batched step costs about one forward at B = 64 plus one read-back.

  python tools/bench_eval.py [--rounds 5] [--rollouts 64] [--steps 30] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import adaptigraph_amd as ag  # noqa: E402
import train_restate as TR  # noqa: E402
from bench_dataset import DATASET, MATERIAL, SOFT_DATASET, SOFT_MATERIAL, make_episodes, make_soft_episodes  # noqa: E402
from bench_train import CFG  # noqa: E402

FAMILIES = ["fps", "assemble", "edge_count", "edge_emit", "rule", "surface", "prep", "node_enc", "edge_enc", "node_prop", "node_final", "roll_update"]


def sequential(model, ds, idx, steps):
    """The same rollouts one graph at a time through rollout_eval; -> (L, B) errors on the device."""
    sp, N = ds.spec, ds.N
    dr = ds.eval_draws(idx)
    data = ds.batch(idx, dr, with_fps=True)
    aux = ds._last_build
    adj = float(dr.adj_thresh[0])
    cfg = dict(adj_thresh=adj, topk=sp.topk, max_nR=sp.max_nR, connect_tool_all=sp.connect_tool_all,
               connect_tool_all_non_fixed=sp.connect_tool_all_non_fixed, store_rest_state=sp.store_rest_state, dense=False)
    errors = torch.empty((steps, len(idx)), dtype=torch.float32, device=ds.device)
    e0 = data["edges"]
    for j, i in enumerate(idx):
        ep, t0 = int(ds._episode[i]), int(ds._frames[i, sp.n_his - 1])
        sl = slice(j, j + 1)
        graph = {k: data[k][sl] for k in ("state", "action", "attrs", "p_rigid", "p_instance", "obj_mask", "material_index", "rope_physics_param")}
        graph["state_mask"], graph["eef_mask"] = aux["state_mask"][sl].view(torch.bool), aux["eef_mask"][sl].view(torch.bool)
        graph["edges"] = ag.EdgeList(e0.recv[sl].contiguous(), e0.send[sl].contiguous(), e0.row_ptr[sl].contiguous(), e0.n_edges[sl].contiguous(), N)
        o, n_e = int(ds._obj_off[ep]), int(ds._n_e[ep])
        eef = ds._eef[int(ds._eef_off[ep]):int(ds._eef_off[ep]) + int(ds._t_e[ep]) * ds.n_eef].view(-1, ds.n_eef, 3)
        _, preds, _ = ag.rollout_eval(model, graph, eef, t0 + 1, steps, **cfg)
        n = int(data["n_obj"][j])
        sel = data["fps_idx"][j, :n].long()
        for s, p in enumerate(preds):
            gt = ds._obj[o + (t0 + 1 + s) * n_e:o + (t0 + 2 + s) * n_e][sel]
            errors[s, j] = (p[:n] - gt).norm(dim=-1).mean()
    return errors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--config", choices=["rope", "softbody", "surface"], default="rope")
    a = ap.parse_args()
    soft = a.config in ("softbody", "surface")
    dev = torch.device("cuda:0")
    T = a.steps + 15
    n_epis, per = 8, a.rollouts // 8
    assert per * n_epis == a.rollouts and per <= 8, "rollouts: a multiple of 8, at most 64"
    if soft:
        pairs, phys, obj, eef = make_soft_episodes(600, n_epis=n_epis, T=T)
        dcfg = SOFT_DATASET
        if a.config == "surface":
            import copy
            dcfg = copy.deepcopy(SOFT_DATASET)
            dcfg["datasets"][0].update(connect_tool_surface=True, connect_tool_surface_ratio=0.8)
        ds = ag.DeviceDynDataset(dcfg, SOFT_MATERIAL, pairs, phys, obj, eef, dev, phase="valid")
        model = ag.DynamicsPredictor(dict(CFG, pstep=4), SOFT_MATERIAL, {"n_his": 5, "materials": ["softbody"]}, dev)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in TR.make_weights(0, n_his=5).items()})
    else:
        pairs, phys, obj, eef = make_episodes(600, n_epis=n_epis, T=T)
        ds = ag.DeviceDynDataset(DATASET, MATERIAL, pairs, phys, obj, eef, dev, phase="valid")
        model = ag.DynamicsPredictor(CFG, MATERIAL, {"n_his": 4, "materials": ["rope"]}, dev)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in TR.make_weights(0).items()})
    model = model.to(dev)
    idx = np.array([e * (len(pairs) // n_epis) + s for e in range(n_epis) for s in range(per)])
    sync = torch.cuda.synchronize
    variants = {"batched": lambda: ag.rollout_eval_batch(model, ds, idx, rollout_steps=a.steps).errors,
                "sequential": lambda: sequential(model, ds, idx, a.steps),
                "per_graph": lambda: ag.rollout_eval_batch(model, ds, idx, rollout_steps=a.steps, per_graph=True).errors}
    if soft:
        del variants["sequential"]
    base = "per_graph" if soft else "sequential"
    out = {k: fn() for k, fn in variants.items()}                                    # warm-up, and the three agree
    sync()
    res0 = ag.rollout_eval_batch(model, ds, idx, rollout_steps=a.steps)
    assert res0.lengths.tolist() == [a.steps] * a.rollouts
    agree = {k: float((out[k] - out["batched"]).abs().max()) for k in variants if k != "batched"}
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times[k].append((time.perf_counter() - t0) * 1e3)
    res = {"tool": "bench_eval", "device": torch.cuda.get_device_name(dev), "rounds": a.rounds, "rollouts": a.rollouts, "steps": a.steps,
           "config": ("surface: softbody with connect_tool_surface at ratio 0.8; " if a.config == "surface" else "") +
                     ("softbody: max_nobj 300 + 5 tool points, topk 10, max_nR 3500, non-fixed rule, kNN range [0.4, 1.0], n_his 5, pstep 4, "
                      "synthetic episodes of 600 points") if soft else
                     "rope: max_nobj 100 + 1 tool point, topk 10, max_nR 1000, synthetic episodes of 600 points",
           "n_obj_mean": float(ds.batch(idx, ds.eval_draws(idx), with_fps=True)["n_obj"].float().mean()),
           "edges_start_mean": float(np.mean([tr[0][-1][2] for tr in res0.trails])),
           "backoff_attempts_in_loop": int(sum(len(t) - 1 for tr in res0.trails for t in tr[1:])), "host_waits": res0.host_waits,
           "max_abs_error_difference_to_batched": agree, "variants": {}}
    for k, v in times.items():
        med = float(np.median(v))
        res["variants"][k] = {"ms_median": med, "ms_rounds": [round(x, 2) for x in v], "ms_per_step": med / a.steps,
                              "ms_per_rollout": med / a.rollouts, "us_per_rollout_step": med * 1e3 / (a.steps * a.rollouts)}
    seq = res["variants"][base]["ms_median"]
    for k in variants:
        res["variants"][k]["speedup_over_" + base] = seq / res["variants"][k]["ms_median"]
    # ---- kernel table of the batched path, and one plain forward at the same B, in a separate pass
    eng = model.engine(dev)
    for e in (eng, ds.engine):
        e.set_profiling(FAMILIES)
        e.reset_stats()
    variants["batched"]()
    sync()
    res["kernels_batched_ms_per_step"] = {}
    for f in FAMILIES:
        ms = sum(e.kernel_stats(f)[0] for e in (eng, ds.engine))
        n = sum(e.kernel_stats(f)[1] for e in (eng, ds.engine))
        res["kernels_batched_ms_per_step"][f] = {"ms": ms / a.steps, "launches": n / a.steps}
    res["kernels_batched_ms_per_step_total"] = sum(v["ms"] for v in res["kernels_batched_ms_per_step"].values())
    for e in (eng, ds.engine):
        e.set_profiling([])
    data = ds.batch(idx, ds.eval_draws(idx))
    fwd = {k: v for k, v in data.items() if k in ("state", "attrs", "p_instance", "action", "edges") or k.endswith("_physics_param")}
    for _ in range(3):
        model(**fwd)
    sync()
    t0 = time.perf_counter()
    for _ in range(20):
        model(**fwd)                                                                # (ag_forward waits for its flag: wall time per call)
    res["forward_B%d_ms" % a.rollouts] = (time.perf_counter() - t0) * 1e3 / 20
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
