#!/usr/bin/env python
"""A/B of builds of the library for Options::zero_skip (docs/EXPERIMENTS.md): alternating runs, one process at a time.

  headline   python tools/zero_skip_ab.py bench --libs parent=PATH,change=PATH [--runs 3] --out profiles/zero_skip_ab.json
             runs `bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline` per library in turn (ADAPTIGRAPH_AMD_LIB) and
             keeps every run's ms per step and reward_sha256
  kernels    python tools/zero_skip_ab.py kernels --libs ... --weights bench|all_live [--runs 3] --out ...
             the bench's cloth batch on ONE stream with share_first off (every k_edge_enc launch a full 128-candidate one),
             HIP events around every launch of the three chain kernels: ms per launch, per run.  --weights all_live sets every
             hidden bias to +10, so that no ReLU unit is ever off and zero_skip finds nothing to skip: what the mask and the
             branches cost where they cannot pay
  (one)      the worker of `kernels`: one library (the one ADAPTIGRAPH_AMD_LIB names), one JSON line
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMS = ["edge_enc", "node_prop", "node_final"]
HIDDEN = ["relation_encoder.model.0", "relation_encoder.model.2", "relation_encoder.model.4",
          "particle_encoder.model.0", "particle_encoder.model.2", "particle_encoder.model.4",
          "relation_propagator.linear", "particle_propagator.linear",
          "non_rigid_predictor.linear_0", "non_rigid_predictor.linear_1"]


def worker(args):
    sys.path.insert(0, ROOT)
    import types
    import numpy as np
    import torch
    import bench
    import adaptigraph_amd as ag
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    cloud = bench.cloth_cloud(45, rng)
    task = bench.make_task(max_nR=int(1.2 * 6 * (cloud.shape[0] + 1)) + 64)
    W = bench.random_weights(0)
    if args.weights == "all_live":
        for name in HIDDEN:
            W[name + ".bias"][:] = 10.0
    model = ag.DynamicsPredictor(*bench.model_cfg(), dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    ppm = types.SimpleNamespace(task_config=task, eef_num=1, material="cloth", material_dims=task["material_dims"],
                                material_indices=task["material_indices"], physics_param={"cloth": torch.tensor([0.5])},
                                adj_thresh=task["adj_thresh"])
    a = torch.from_numpy(bench.make_actions(1024, 2, 10, cloud, rng)).to(dev)
    s0 = torch.from_numpy(cloud).to(dev)
    eng = model.engine(dev)
    out = {"weights": args.weights, "lib": os.environ.get("ADAPTIGRAPH_AMD_LIB", "product"), "passes": []}
    try:
        out["zero_skip_active"] = eng.get_option("zero_skip_active")
    except AssertionError:
        out["zero_skip_active"] = None                        # a build from before the option
    ag.dynamics(s0, a, model, dev, ppm)                       # warm-up: allocations, graphs of the first call
    torch.cuda.synchronize()
    with eng.options(share_first=0):
        for _ in range(args.passes):
            eng.reset_stats()
            eng.set_profiling(FAMS)
            seq = ag.dynamics(s0, a, model, dev, ppm)["state_seqs"]
            torch.cuda.synchronize()
            eng.set_profiling([])
            p = {}
            for f in FAMS:
                ms, n = eng.kernel_stats(f)
                p[f] = {"ms": ms, "launches": n, "ms_per_launch": ms / max(1, n)}
            out["passes"].append(p)
    out["finite"] = bool(torch.isfinite(seq).all())
    print("ZS_AB " + json.dumps(out))


def run_child(cmd, lib, tag, limit):
    env = dict(os.environ, ADAPTIGRAPH_AMD_LIB=os.path.abspath(lib))
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit(f"{tag}: exit status {r.returncode}; nothing more is started")
    return r.stdout


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["bench", "kernels", "one"])
    ap.add_argument("--libs", default="")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--weights", default="bench", choices=["bench", "all_live"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode == "one":
        return worker(args)
    libs = [kv.split("=", 1) for kv in args.libs.split(",")]
    res = {"mode": args.mode, "weights": args.weights, "order": "alternating, " + " -> ".join(n for n, _ in libs), "runs": []}
    for i in range(args.runs):
        for name, path in libs:
            if args.mode == "bench":
                txt = run_child([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"],
                                path, name, 600)
                line = [ln for ln in txt.splitlines() if ln.startswith("{")][-1]
                d = json.loads(line)
                rec = {"lib": name, "run": i, "ms_per_step": d["ms_per_step"], "rollout_steps_per_s": d["value"],
                       "reward_sha256": d.get("reward_sha256")}
            else:
                txt = run_child([sys.executable, os.path.abspath(__file__), "one", "--weights", args.weights, "--passes", str(args.passes)],
                                path, name, 600)
                d = json.loads([ln for ln in txt.splitlines() if ln.startswith("ZS_AB ")][-1][6:])
                rec = {**d, "lib": name, "run": i}
            res["runs"].append(rec)
            print(json.dumps(rec), flush=True)
    if args.mode == "bench":
        res["summary"] = {n: sorted(r["ms_per_step"] for r in res["runs"] if r["lib"] == n) for n, _ in libs}
    else:
        res["summary"] = {n: {f: sorted(round(p[f]["ms_per_launch"], 5) for r in res["runs"] if r["lib"] == n for p in r["passes"])
                              for f in FAMS} for n, _ in libs}
    print(json.dumps(res["summary"]))
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
