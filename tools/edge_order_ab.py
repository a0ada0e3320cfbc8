#!/usr/bin/env python
"""A/B of builds of the library for Options::edge_order (docs/EXPERIMENTS.md): alternating runs, one process at a time.  The
sibling of tools/zero_skip_ab.py; a library is given as name=path:order, and `order` goes to the child as AG_EDGE_ORDER (a
library from before the option ignores it).

  headline   python tools/edge_order_ab.py bench --libs parent=PATH:0,change=PATH:1 [--runs 3] --out profiles/edge_order_ab.json
             runs `bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline` per library in turn (ADAPTIGRAPH_AMD_LIB) and keeps
             every run's ms per step and reward_sha256
  kernels    python tools/edge_order_ab.py kernels --libs ... --weights bench|all_live [--runs 1] [--passes 4] --out ...
             the bench's cloth batch on ONE stream with share_first off (every k_edge_enc launch a full 128-candidate one), HIP
             events around every launch of k_edge_enc, k_ell_index (family edge_emit) and the propagate chains: ms per launch,
             per pass.  --weights all_live sets every hidden bias to +10: no k-step of the relation encoder is dead, what the
             mask and the branches cost where they cannot pay
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import zero_skip_ab as zs  # noqa: E402

FAMS = ["edge_enc", "edge_emit", "node_prop", "node_final"]


def run_child(cmd, lib, order, tag, limit):
    env = dict(os.environ, ADAPTIGRAPH_AMD_LIB=os.path.abspath(lib), AG_EDGE_ORDER=str(order))
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
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--weights", default="bench", choices=["bench", "all_live"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode == "one":
        zs.FAMS = FAMS
        return zs.worker(args)
    libs = []
    for kv in args.libs.split(","):
        name, rest = kv.split("=", 1)
        path, order = rest.rsplit(":", 1)
        libs.append((name, path, int(order)))
    res = {"mode": args.mode, "weights": args.weights, "order": "alternating, " + " -> ".join(n for n, _, _ in libs),
           "edge_order": {n: o for n, _, o in libs}, "runs": []}
    for i in range(args.runs):
        for name, path, order in libs:
            if args.mode == "bench":
                txt = run_child([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"],
                                path, order, name, 600)
                d = json.loads([ln for ln in txt.splitlines() if ln.startswith("{")][-1])
                rec = {"lib": name, "run": i, "ms_per_step": d["ms_per_step"], "rollout_steps_per_s": d["value"],
                       "reward_sha256": d.get("reward_sha256")}
            else:
                txt = run_child([sys.executable, os.path.abspath(__file__), "one", "--weights", args.weights, "--passes", str(args.passes)],
                                path, order, name, 600)
                d = json.loads([ln for ln in txt.splitlines() if ln.startswith("ZS_AB ")][-1][6:])
                rec = {**d, "lib": name, "run": i}
            res["runs"].append(rec)
            print(json.dumps(rec), flush=True)
    if args.mode == "bench":
        res["summary"] = {n: sorted(r["ms_per_step"] for r in res["runs"] if r["lib"] == n) for n, _, _ in libs}
        res["reward_sha256"] = sorted({str(r["reward_sha256"]) for r in res["runs"]})
    else:
        res["summary"] = {n: {f: sorted(round(p[f]["ms_per_launch"], 5) for r in res["runs"] if r["lib"] == n for p in r["passes"])
                              for f in FAMS} for n, _, _ in libs}
    print(json.dumps(res["summary"]))
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
