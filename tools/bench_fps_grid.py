#!/usr/bin/env python3
"""Cell-pruned farthest-point sampling benchmark: per-call time of fps_cloud_grid (ag_fps_cloud_grid) next to fps_cloud where both
apply - n in {8192, 131072, 1048576} x max_nobj in {100, 1024} - and alone beyond fps_cloud's 1024 samples: (131072, 4096),
(1048576, 4096), (1048576, 16384), (1048576, 65536) and four clouds per launch at (131072, 4096).  Cloud and radius are those of
tools/bench_cloud.py.

Two cell policies are timed side by side: "p64" - the library's default, about 64 points per cell, at most 16,384 cells (above
2048 cells the selection's per-cell tables live in the workspace) - and "lds" - the same, capped at the 2048 cells whose tables fit
LDS, passed as a forced `cells`.  They differ only above 131,072 points.  (`cells` forces stage 2's cell count too; the policies
are compared on binning + stage 1.)

The split of a call is measured by whole calls that leave a part out, timed in the same rounds:
    binning  = the call at max_nobj 1 and a radius above the cloud (pass 1's binning; stage 1 has no pick to make),
    stage 1  = the call at a radius above the cloud - binning (includes the binning of the max_nobj stage-1 points),
    stage 2  = the call - the call at a radius above the cloud.
Time per selected point: stage 1 over its min(max_nobj, n) - 1 sweeps, stage 2 over the points it keeps.

Timing: HIP events around back-to-back enqueue-only calls after a warm-up, every variant of a configuration alternating inside a
round, median of the rounds.  Every group of configurations runs in a child process under a time limit of its own; the first child
that fails ends the run (nothing more is started on the device).

Gate (exit status): outputs equal wherever two paths or two policies run, and at (1048576, 1024) the default policy is not slower
than fps_cloud measured beside it.

  python tools/bench_fps_grid.py [--rounds 7] [--out profiles/r27_fps_grid.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS = 0.6
FAR = 1e30                                                   # a radius above every cloud: stage 2 keeps its start alone
M = 1 << 20
GROUPS = {                                                   # name: ([(n, max_nobj, B)], time limit of the child in seconds)
    "both_small": ([(8192, 100, 1), (8192, 1024, 1), (131072, 100, 1), (131072, 1024, 1)], 300),
    "both_1m": ([(M, 100, 1), (M, 1024, 1)], 400),
    "beyond_131072": ([(131072, 4096, 1), (131072, 4096, 4)], 400),
    "beyond_1m": ([(M, 4096, 1), (M, 16384, 1)], 400),
    "beyond_1m_65536": ([(M, 65536, 1)], 500),
}
HOST_SHAPE = (131072, 4096, 1)                               # the numpy restatement is timed (once) on this one


def clouds_for(n, B):
    import numpy as np
    rng = np.random.default_rng(n + B)
    return [(rng.normal(size=(n, 3)) * [1.0, 0.1, 0.6]).astype(np.float32) for _ in range(B)]


def lds_cells(n):
    c = 1
    while c < 2048 and c * 64 < n:
        c *= 2
    return c


def group(name, rounds):
    """The child: every configuration of one group; prints one JSON line."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import adaptigraph_amd as ag
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "configs": []}
    for n, max_nobj, B in GROUPS[name][0]:
        clouds = clouds_for(n, B)
        starts = [(int(n // 3 + b), int(7 + b)) for b in range(B)]
        pos = torch.from_numpy(np.concatenate(clouds)).to(dev)
        tab = torch.tensor([[b * n for b in range(B)], [n] * B], dtype=torch.int64).to(dev)
        st = torch.tensor([[s for s, _ in starts], [r for _, r in starts]], dtype=torch.int32).to(dev)
        rad = torch.full((B,), RADIUS, dtype=torch.float32, device=dev)
        far = torch.full((B,), FAR, dtype=torch.float32, device=dev)
        zero = torch.zeros_like(st[1])
        policies = {"p64": None}
        if lds_cells(n) * 64 < n:
            policies["lds"] = lds_cells(n)
        variants = {}
        if max_nobj <= 1024:
            variants["fps_cloud"] = lambda: ag.fps_cloud(pos, tab[0], tab[1], st[0], rad, st[1], max_nobj, n)
        for pol, cells in policies.items():
            variants[pol] = lambda cells=cells: ag.fps_cloud_grid(pos, tab[0], tab[1], st[0], rad, st[1], max_nobj, n, cells=cells)
            variants[pol + "_no_stage2"] = lambda cells=cells: ag.fps_cloud_grid(pos, tab[0], tab[1], st[0], far, st[1], max_nobj, n, cells=cells)
            variants[pol + "_binning"] = lambda cells=cells: ag.fps_cloud_grid(pos, tab[0], tab[1], st[0], far, zero, 1, n, cells=cells)
        results = {}
        for k, fn in variants.items():                       # warm-up: the code objects, the workspace
            results[k] = fn()
            fn()
        torch.cuda.synchronize(dev)
        full = [k for k in variants if k in ("fps_cloud", "p64", "lds")]
        equal = all(torch.equal(results[k][0], results[full[0]][0]) and torch.equal(results[k][1], results[full[0]][1]) for k in full)
        kept = results["p64"][1].cpu().tolist()
        est = {}
        for k, fn in variants.items():                       # size the timed window: about 50 ms of calls, at least one
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            est[k] = max(1, min(20, int(50.0 / max(e0.elapsed_time(e1), 1e-3))))
        ms = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():                   # the variants alternate inside a round
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(est[k]):
                    fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / est[k])
        med = {k: float(np.median(v)) for k, v in ms.items()}
        cfg = {"points": n, "max_nobj": max_nobj, "clouds": B, "kept": kept, "equal": bool(equal), "compared": full,
               "calls_per_round": est, "ms_per_call_median": med, "ms_per_call_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
        picks1, picks2 = min(max_nobj, n) - 1, max(kept)
        for pol in policies:
            b, s1, s2 = med[pol + "_binning"], med[pol + "_no_stage2"] - med[pol + "_binning"], med[pol] - med[pol + "_no_stage2"]
            cfg[pol + "_split_ms"] = {"binning": b, "stage1": s1, "stage2": s2, "stage1_us_per_pick": 1e3 * s1 / max(picks1, 1),
                                      "stage2_us_per_pick": 1e3 * s2 / max(picks2, 1)}
        if "fps_cloud" in med:
            cfg["fps_cloud_over_grid"] = {pol: med["fps_cloud"] / med[pol] for pol in policies}
        if (n, max_nobj, B) == HOST_SHAPE:
            import dataset_restate as DR
            import fps_grid_restate as GR
            t0 = time.perf_counter()
            want = DR.fps_indices(clouds[0], max_nobj, starts[0][0], RADIUS, starts[0][1])
            cfg["host_brute_force_restatement_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            again = GR.fps_indices(clouds[0], max_nobj, starts[0][0], RADIUS, starts[0][1])
            cfg["host_pruned_restatement_s"] = time.perf_counter() - t0
            got = results["p64"][0][0, :kept[0]].cpu().numpy()
            cfg["equal_host_restatement"] = bool(kept[0] == len(want) and np.array_equal(got, want) and np.array_equal(again, want))
        out["configs"].append(cfg)
        print(f"{name}: ({n}, {max_nobj}) x {B} done", file=sys.stderr, flush=True)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--group", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.group is not None:
        return group(a.group, a.rounds)
    res = {"tool": "bench_fps_grid", "fps_radius": RADIUS, "cloud": "normal(0, 1) * [1.0, 0.1, 0.6], fp32, seeded (tools/bench_cloud.py)",
           "timing": "HIP events around calls_per_round back-to-back enqueue-only calls after 2 warm-up calls; the variants of a "
                     "configuration alternate inside a round; median of the rounds",
           "policies": {"p64": "about 64 points per cell, at most 16384 cells (the default)",
                        "lds": "about 64 points per cell, at most the 2048 cells whose tables fit LDS (forced cells)"},
           "split": "binning = call at max_nobj 1, radius above the cloud; stage1 = call at a radius above the cloud - binning; "
                    "stage2 = call - call at a radius above the cloud",
           "rounds": a.rounds, "groups": {}}
    for name, (_, limit) in GROUPS.items():
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--group", name, "--rounds", str(a.rounds)],
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            res["stopped"] = f"{name}: no result within {limit} s; nothing further was started"
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            res["stopped"] = f"{name}: exit status {p.returncode}; nothing further was started"
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            break
        res["groups"][name] = json.loads(lines[-1][len("RESULT "):])
        sys.stderr.write(p.stderr[-600:])
    cfgs = [c for g in res["groups"].values() for c in g["configs"]]
    gate = {"outputs_equal": all(c["equal"] and c.get("equal_host_restatement", True) for c in cfgs) and bool(cfgs)}
    at = [c for c in cfgs if (c["points"], c["max_nobj"], c["clouds"]) == (M, 1024, 1)]
    gate["not_slower_at_1048576_x_1024"] = bool(at) and at[0]["ms_per_call_median"]["p64"] <= at[0]["ms_per_call_median"]["fps_cloud"]
    gate["ran_1048576_x_65536_to_the_end"] = any((c["points"], c["max_nobj"]) == (M, 65536) for c in cfgs)
    res["gate"] = gate
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ok = "stopped" not in res and gate["outputs_equal"] and gate["not_slower_at_1048576_x_1024"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
