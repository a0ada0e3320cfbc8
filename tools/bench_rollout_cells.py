"""The rollout over cell-list graphs (adaptigraph_amd.dynamics_cells) in numbers -> profiles/r25_rollout_cells.json.

  scaling   ms per rollout step at B = 1, cloth (top-k 5, connect_tools_all), 128^2 / 256^2 / 512^2 object rows + 1 tool: one call =
            one look-ahead step x repeat 5, enqueue only; HIP events around back-to-back calls after a warm-up, median of the
            rounds, divided by 5 (the look-ahead step's init and particle encoder are in it).  GATE: step(65,536) <= 8 x step(16,384)
            - linear growth is 4 x, a quadratic term 16 x.  Exit status 1 when it is missed.
  split     per step from the engine's kernel_stats: edge build (cell-list builder), guard + self-loop pass, chains, glue
            (tool height + row kernels, init included)
  ratio     dynamics_cells over dynamics on the 45 x 45 cloth at B = 64 and B = 1 (2 look-ahead x repeat 10, bench.py's shape)
  planner   one Planner call (64 samples, MPPI, chamfer target) on the 4096 + 1 cloth through partial(dynamics_cells, ...)
One GPU.  Diagnostic: the contract line is bench.py's."""
import json, os, sys, types
from functools import partial
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B
import adaptigraph_amd as ag

dev = torch.device("cuda", 0)
CHAINS = ["node_enc", "edge_enc", "node_prop", "node_final"]


def model_and_ppm(max_nR):
    task = B.make_task(max_nR, limits=False)
    m = ag.DynamicsPredictor(*B.model_cfg(), dev)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in B.random_weights(0).items()})
    ppm = types.SimpleNamespace(task_config=task, eef_num=1, material="cloth", material_dims=task["material_dims"],
                                material_indices=task["material_indices"], physics_param={"cloth": torch.tensor([0.5])},
                                adj_thresh=task["adj_thresh"])
    return m, ppm, task


def timed(fn, calls, rounds, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return float(np.median(out)), [round(v, 4) for v in out]


def scaling(side, repeat=5):
    rng = np.random.default_rng(side)
    cloud = B.cloth_cloud(side, rng)
    N = cloud.shape[0] + 1
    m, ppm, _ = model_and_ppm(int(1.2 * 6 * N) + 64)
    eng = m.engine(dev)
    a = torch.from_numpy(B.make_actions(1, 1, repeat, cloud, rng))
    s0 = torch.from_numpy(cloud).to(dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    fn = lambda: ag.dynamics_cells(s0, a, m, dev, ppm, _sync=False, _overflow_flag=flag)
    calls = 10 if N < 100000 else 4
    ms, rounds = timed(fn, calls, 5)
    assert int(flag[0]) == 0
    fams = ["edge_count", "edge_emit", "roll_init", "roll_update"] + CHAINS
    eng.set_profiling(fams)
    eng.reset_stats()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    st = {f: eng.kernel_stats(f)[0] / (3 * repeat) for f in fams}
    eng.set_profiling([])
    split = {"edge_build_ms": st["edge_count"], "guard_and_self_loops_ms": st["edge_emit"], "chains_ms": sum(st[f] for f in CHAINS),
             "glue_ms": st["roll_init"] + st["roll_update"]}
    split["glue_share"] = split["glue_ms"] / sum(v for k, v in split.items() if k.endswith("_ms"))
    return {"rows": N, "repeat": repeat, "calls_per_round": calls, "ms_per_call_rounds": rounds, "ms_per_step": ms / repeat,
            "split_per_step": split}


def ratio(Bn):
    rng = np.random.default_rng(0)
    cloud = B.cloth_cloud(45, rng)
    m, ppm, _ = model_and_ppm(int(1.2 * 6 * (cloud.shape[0] + 1)) + 64)
    a = torch.from_numpy(B.make_actions(Bn, 2, 10, cloud, rng))
    s0 = torch.from_numpy(cloud).to(dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    out = {}
    for name, f in (("dynamics", ag.dynamics), ("dynamics_cells", ag.dynamics_cells)):
        ms, rounds = timed(lambda: f(s0, a, m, dev, ppm, _sync=False, _overflow_flag=flag), 5, 5)
        out[name + "_ms"] = ms
    assert torch.equal(ag.dynamics(s0, a, m, dev, ppm)["state_seqs"], ag.dynamics_cells(s0, a, m, dev, ppm)["state_seqs"])
    out["cells_over_dynamics"] = out["dynamics_cells_ms"] / out["dynamics_ms"]
    return out


def planner_call(n_sample=64):
    from adaptigraph_amd.planner import Planner
    rng = np.random.default_rng(4097)
    cloud = B.cloth_cloud(64, rng)
    m, ppm, t = model_and_ppm(int(1.2 * 6 * (cloud.shape[0] + 1)) + 64)
    lo_l, hi_l = [-11.5, -8.5, -3.14, 2.0], [7.5, 10.5, 3.14, 6.0]     # pushes over the sheet, 2..5 steps
    lo, hi = torch.tensor(lo_l, device=dev), torch.tensor(hi_l, device=dev)
    s0 = torch.from_numpy(cloud).to(dev)
    target = torch.from_numpy(cloud + np.float32([0.4, 0, 0.3])).to(dev)
    bbox = np.array([[-12.0, 8.0], [-9.0, 11.0]])
    cfg = {"action_dim": 4, "model_rollout_fn": partial(ag.dynamics_cells, model=m, device=dev, ppm_optimizer=ppm),
           "evaluate_traj_fn": partial(ag.running_cost, error_func=partial(ag.chamfer, y=target[None]),
                                       penalty_func=partial(ag.cloth_penalty, sim_real_ratio=10.0), bbox=bbox),
           "sampling_action_seq_fn": partial(ag.sample_action_seq, action_lower_lim=lo, action_upper_lim=hi, n_sample=n_sample,
                                             device=dev, noise_level=1.0, push_length=t["push_length"]),
           "clip_action_seq_fn": partial(ag.clip_actions, action_lower_lim=lo, action_upper_lim=hi),
           "optimize_action_mppi_fn": partial(ag.optimize_action_mppi, reward_weight=500.0, action_lower_lim=lo,
                                              action_upper_lim=hi, push_length=t["push_length"]),
           "n_sample": n_sample, "n_look_ahead": 1, "n_update_iter": 1, "reward_weight": 500.0, "action_lower_lim": lo,
           "action_upper_lim": hi, "planner_type": "MPPI", "device": dev, "verbose": False, "noise_level": 1.0, "rollout_best": True}
    pl = Planner(cfg)
    act = torch.tensor([[-2.0, 1.0, 0.0, 3.5]], device=dev)
    ms, rounds = timed(lambda: pl.trajectory_optimization(s0, act), 1, 3, warm=1)
    return {"rows": cloud.shape[0] + 1, "n_sample": n_sample, "ms_per_planner_call": ms, "rounds": rounds}


def main():
    res = {"tool": "bench_rollout_cells", "device": torch.cuda.get_device_name(0),
           "timing": "HIP events around back-to-back enqueue-only calls after 2 warm-up calls; median of 5 rounds",
           "scaling": {}, "ratio": {}}
    out_path = os.path.join(ROOT, "profiles", "r25_rollout_cells.json")
    for side in (128, 256, 512):
        res["scaling"][str(side * side)] = scaling(side)
        print(json.dumps({side * side: res["scaling"][str(side * side)]}), flush=True)
    s = res["scaling"]
    res["step_65536_over_16384"] = s["65536"]["ms_per_step"] / s["16384"]["ms_per_step"]
    res["step_262144_over_65536"] = s["262144"]["ms_per_step"] / s["65536"]["ms_per_step"]
    res["gate_step_65536_within_8x"] = res["step_65536_over_16384"] <= 8.0
    for Bn in (64, 1):
        res["ratio"][str(Bn)] = ratio(Bn)
        print(json.dumps({"ratio_B": Bn, **res["ratio"][str(Bn)]}), flush=True)
    try:
        res["planner"] = planner_call()
    except Exception as e:                                               # reported, not hidden: the rest of the file stands
        res["planner"] = {"error": f"{type(e).__name__}: {e}"}
    print(json.dumps(res["planner"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("step_65536_over_16384", "step_262144_over_65536", "gate_step_65536_within_8x")}))
    return 0 if res["gate_step_65536_within_8x"] else 1


if __name__ == "__main__":
    sys.exit(main())
