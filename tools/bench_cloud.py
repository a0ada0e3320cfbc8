#!/usr/bin/env python3
"""Cloud-sampling benchmark: per-call time of fps_cloud (ag_fps_cloud, both farthest-point stages of a perceived cloud) at
max_nobj 100 for clouds of 8192, 32,768, 131,072 and 1,048,576 points, one cloud per launch and four, next to the two paths that
existed before it: the numpy restatement on the host (tests/dataset_restate.py: fps_indices - what a caller of the reference's
construct_graph runs today, minus dgl's own implementation of stage 1) for the same clouds, and fps_batch (the LDS-resident
kernel) at 8192 points, its limit.

Each size runs in a child process of its own under a time limit of its own; the first child that fails ends the run (nothing more
is started on the device).  Device times are HIP events around `calls` back-to-back calls after a warm-up, per-call = elapsed /
calls, median over `rounds`; host times are wall time of the restatement, median over its repeats.  In every child the device's
indices are compared with the restatement's on the timed clouds ("equal").  No pass / fail threshold on time.

  python tools/bench_cloud.py [--rounds 7] [--out profiles/r19_cloud_fps.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [8192, 32768, 131072, 1048576]
BATCHES = [1, 4]
MAX_NOBJ = 100
RADIUS = 0.6
LIMIT_S = {8192: 240, 32768: 240, 131072: 300, 1048576: 480}      # per child: torch's first import, the host restatement, the device


def clouds_for(n, B):
    import numpy as np
    rng = np.random.default_rng(n + B)
    return [(rng.normal(size=(n, 3)) * [1.0, 0.1, 0.6]).astype(np.float32) for _ in range(B)]


def one(n, rounds):
    """The child: everything at one cloud size; prints one JSON line."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import adaptigraph_amd as ag
    import dataset_restate as DR
    from adaptigraph_amd.dataset import fps_batch
    dev = torch.device("cuda:0")
    calls = 20 if n <= 32768 else 10 if n <= 131072 else 4
    res = {"points": n, "calls_per_round": calls, "rounds": rounds, "device": torch.cuda.get_device_name(dev)}
    for B in BATCHES:
        clouds = clouds_for(n, B)
        starts = [(int(n // 3 + b), int(7 + b)) for b in range(B)]
        pos = torch.from_numpy(np.concatenate(clouds)).to(dev)
        tab = torch.tensor([[b * n for b in range(B)], [n] * B], dtype=torch.int64).to(dev)
        st = torch.tensor([[s for s, _ in starts], [r for _, r in starts]], dtype=torch.int32).to(dev)
        rad = torch.full((B,), RADIUS, dtype=torch.float32, device=dev)
        variants = {"fps_cloud": ag.fps_cloud}
        if n <= 8192:
            variants["fps_batch"] = fps_batch
        # host: the restatement, cloud after cloud
        reps = 3 if n <= 131072 else 1
        host, want = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            want = [DR.fps_indices(c, MAX_NOBJ, s, RADIUS, r) for c, (s, r) in zip(clouds, starts)]
            host.append((time.perf_counter() - t0) * 1e3)
        entry = {"host_restatement_ms": float(np.median(host)), "host_repeats": reps, "n_obj": [len(w) for w in want]}
        for name, fn in variants.items():
            run = lambda: fn(pos, tab[0], tab[1], st[0], rad, st[1], MAX_NOBJ, n)   # noqa: E731
            for _ in range(3):
                idx, n_obj = run()
            torch.cuda.synchronize(dev)
            got = idx.cpu().numpy()
            equal = all(int(n_obj[b]) == len(want[b]) and np.array_equal(got[b, :len(want[b])], want[b]) for b in range(B))
            ms = []
            for _ in range(rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    run()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / calls)
            entry[name] = {"ms_per_call_median": float(np.median(ms)), "ms_per_call_rounds": [round(x, 4) for x in ms], "equal": bool(equal)}
        entry["host_over_fps_cloud"] = entry["host_restatement_ms"] / entry["fps_cloud"]["ms_per_call_median"]
        if "fps_batch" in entry:
            entry["fps_cloud_over_fps_batch"] = entry["fps_cloud"]["ms_per_call_median"] / entry["fps_batch"]["ms_per_call_median"]
        res["B%d" % B] = entry
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one is not None:
        return one(a.one, a.rounds)
    res = {"tool": "bench_cloud", "max_nobj": MAX_NOBJ, "fps_radius": RADIUS, "cloud": "normal(0, 1) * [1.0, 0.1, 0.6], fp32, seeded",
           "timing": "HIP events around calls_per_round back-to-back calls after 3 warm-up calls; median of the rounds; host: wall time",
           "sizes": {}}
    for n in SIZES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), "--rounds", str(a.rounds)],
                               capture_output=True, text=True, timeout=LIMIT_S[n])
        except subprocess.TimeoutExpired:
            res["stopped"] = f"{n} points: no result within {LIMIT_S[n]} s; nothing further was started"
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            res["stopped"] = f"{n} points: exit status {p.returncode}; nothing further was started"
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            break
        res["sizes"][str(n)] = json.loads(lines[-1][len("RESULT "):])
        print(f"{n} points: done", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    sys.exit(main())
