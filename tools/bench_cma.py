#!/usr/bin/env python3
"""CMA-ES benchmark: what a generation of the device-side search (ag_cma.hip) costs, and the planner type next to MPPI.

  kernels  device time of one generation - ask, then rank + tell - of CmaSearch at (n, popsize) = (4, 500), (4, 20000), (8, 1024),
           (64, 1024) and, the cap of both, (64, 32768): seeded draws, the sphere as fitness.  Every timed generation is the SAME
           valid one: the state is restored from a copy taken after three real generations (one device-to-device copy, timed on
           its own as restore_copy and included in the two figures named restore_*), then ask(z) and tell(v) with v computed once
           for that state and z - the timed region holds the copy and the library's three kernels only.
  planner  the rope configuration of the reference's random_interact.py planner call (tools/bench_interact.py: 200 particles,
           n_sample 1000, n_update_iter 5, n_look_ahead 1): one planner call with planner_type 'MPPI' and one with 'CMA', same
           n_sample x n_update_iter, alternating; ms per call (wall time around a call that ends in a synchronise) and the best
           reward of each, over `seeds` seeds.  Whether CMA-ES reaches MPPI's reward on this task is what this section records.

Each section runs in a child process of its own under a time limit of its own; the first child that fails ends the run (nothing
more is started on the device).  Device times are HIP events around `calls` back-to-back calls after a warm-up, per call = elapsed
/ calls, median over `rounds`.  No pass / fail threshold.

  python tools/bench_cma.py [--rounds 7] [--seeds 5] [--out profiles/r23_cma.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = {"kernels": 240, "planner": 420}


def timed(run, calls, rounds):
    """Median per-call milliseconds by device events, and the spread."""
    import numpy as np
    import torch
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return {"ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "calls_per_round": calls}


def child(section, rounds, seeds):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import adaptigraph_amd as ag
    dev = torch.device("cuda:0")
    res = {"section": section, "rounds": rounds, "device": torch.cuda.get_device_name(dev)}
    if section == "kernels":
        for n, pop in ((4, 500), (4, 20000), (8, 1024), (64, 1024), (64, 32768)):
            gen = torch.Generator(device=dev).manual_seed(n * 100003 + pop)
            z = torch.randn((pop, n), dtype=torch.float64, device=dev, generator=gen)
            s = ag.CmaSearch(np.full(n, 0.5), 0.3, -1.0, 2.0, popsize=pop, device=dev)
            for _ in range(3):                                   # a few real generations: C is no longer the identity
                s.tell((s.ask() ** 2).sum(dim=1))
            start = s._state.clone()
            v = (s.ask(z) ** 2).sum(dim=1)

            def restore():
                s._state.copy_(start)

            def tell():
                restore()
                s.tell(v)

            def generation():
                restore()
                s.ask(z)
                s.tell(v)
            calls = 20 if pop <= 20000 else 4
            r = {"ask": timed(lambda: s.ask(z), calls, rounds), "restore_copy": timed(restore, calls, rounds),
                 "restore_rank_tell": timed(tell, calls, rounds), "restore_generation": timed(generation, calls, rounds)}
            st = s.state()
            r.update(status=st["status"], generations_told=st["g"], sigma=st["sigma"])
            res[f"n{n}_pop{pop}"] = r
    elif section == "planner":
        import bench_interact as BI
        import bench_planner as BP
        from adaptigraph_amd.planner import Planner
        base, m, s0, lo, hi, cloud, task = BI.make_interact_planner("rope", 1000, np.random.default_rng(0))
        planners = {"MPPI": base, "CMA": Planner(dict(base.config, planner_type="CMA"))}
        torch.manual_seed(0)
        act_seq = torch.rand((1, 4), device=dev) * (hi - lo) + lo
        out = {k: {"ms": [], "best_reward": []} for k in planners}
        for k, p in planners.items():
            for _ in range(2):
                torch.manual_seed(1)
                BP.loop_call(p, s0, act_seq, 1)
        torch.cuda.synchronize()
        for seed in range(seeds):
            for k, p in planners.items():                        # alternating
                torch.manual_seed(100 + seed)
                t0 = time.perf_counter()
                r = BP.loop_call(p, s0, act_seq, 1)
                torch.cuda.synchronize()
                out[k]["ms"].append((time.perf_counter() - t0) * 1e3)
                out[k]["best_reward"].append(float(r["best_eval_output"]["reward_seqs"].mean()))
        for k, o in out.items():
            res[k] = {"ms_per_planner_call": float(np.median(o["ms"])), "ms_all": o["ms"], "best_reward_per_seed": o["best_reward"],
                      "best_reward_median": float(np.median(o["best_reward"]))}
        # the search's own share of a CMA call: its five generations without the rollout and the cost
        s = planners["CMA"].last_cma
        v = torch.zeros(s.popsize, device=dev)
        res["CMA"]["search_ms_per_call"] = 5 * timed(lambda: (s.ask(), s.tell(v)), 10, rounds)["ms"]
        res["config"] = (f"rope {cloud.shape[0]}+{task['eef_num']} particles, random_interact.py planner call: n_sample 1000, "
                         "n_update_iter 5, n_look_ahead 1, one chunk")
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--sections", nargs="*", default=["kernels", "planner"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_cma.json"))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rounds, a.seeds)
    out = {"rounds": a.rounds, "seeds": a.seeds, "results": []}
    for section in a.sections:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", section, "--rounds", str(a.rounds), "--seeds",
                            str(a.seeds)], capture_output=True, text=True, timeout=LIMIT_S[section])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            raise SystemExit(f"bench_cma: section {section} failed with exit code {p.returncode}; nothing more is started")
        r = json.loads(line[0][7:])
        out["results"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
