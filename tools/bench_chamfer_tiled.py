#!/usr/bin/env python3
"""Tiled Chamfer benchmark: per-call time of chamfer_tiled (forward) and of chamfer_tiled_diff + backward (forward + backward) at
seven shapes (R, N, M) - below the LDS limit of chamfer() beside chamfer() / chamfer_diff() measured in the same process, alternating
with them, and beyond it alone - plus the default tile against 512, 1024 and 4096 at (1, 65536, 65536).

Seeded N(0,1) / N(0.2,1) clouds, By = R, no masks.  Device times are HIP events around `calls` back-to-back calls after a warm-up,
per-call = elapsed / calls, median over `rounds`.  `evals` is the number of distance evaluations a call needs (2 R N M forward: both
directions); Gevals_per_s = evals / time.  growth_65536_over_16384 is the ratio of the (1, 65536, 65536) and (1, 16384, 16384)
times: the work grows 16x.  Where both apply the outputs are compared bit for bit.  No pass / fail threshold on time.

  python tools/bench_chamfer_tiled.py [--rounds 7] [--out profiles/r26_chamfer_tiled.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1, 6739, 6741), (128, 2025, 2025), (20, 4096, 4096), (128, 16385, 33), (1, 16384, 16384), (1, 65536, 65536),
          (8, 65536, 65536)]
BESIDE = 3                                   # the first three shapes fit chamfer()
TILES = (512, 1024, 2048, 4096)


def clocks():
    """What the device reports about its clocks, read only; None where the tool is missing."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30)
        return json.loads(r.stdout) if r.returncode == 0 else None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_chamfer_tiled.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import adaptigraph_amd as ag
    if not torch.cuda.is_available():
        sys.exit("bench_chamfer_tiled: no GPU; nothing is measured on the CPU")
    dev = torch.device("cuda:0")

    def timed(fns, calls):
        """fns: name -> callable.  Per round every fn in turn (alternating), `calls` back-to-back calls each: median ms per call."""
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    fn()
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b) / calls)
        return {k: {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}

    def fwd_bwd(fn, x, y, **kw):
        def run():
            xg = x.detach().requires_grad_(True)
            fn(xg, y, **kw).sum().backward()
            return xg.grad
        return run

    result = {"device": torch.cuda.get_device_name(0), "clocks_before": clocks(), "rounds": args.rounds, "shapes": []}
    by_shape = {}
    for si, (R, N, M) in enumerate(SHAPES):
        rng = np.random.default_rng([26, R, N, M])
        x = torch.from_numpy(rng.normal(0.0, 1.0, (R, N, 3)).astype(np.float32)).to(dev)
        y = torch.from_numpy(rng.normal(0.2, 1.0, (R, M, 3)).astype(np.float32)).to(dev)
        evals = 2.0 * R * N * M
        calls = max(2, min(50, int(2e11 / evals)))
        fns = {"tiled_fwd": lambda: ag.chamfer_tiled(x, y), "tiled_fwd_bwd": fwd_bwd(ag.chamfer_tiled_diff, x, y)}
        row = {"R": R, "N": N, "M": M, "evals_fwd": evals, "calls": calls}
        if si < BESIDE:
            fns["lds_fwd"] = lambda: ag.chamfer(x, y)
            fns["lds_fwd_bwd"] = fwd_bwd(ag.chamfer_diff, x, y)
            row["fwd_bits_equal"] = bool(torch.equal(ag.chamfer_tiled(x, y).view(torch.int32), ag.chamfer(x, y).view(torch.int32)))
            row["grad_bits_equal"] = bool(torch.equal(fns["tiled_fwd_bwd"]().view(torch.int32), fns["lds_fwd_bwd"]().view(torch.int32)))
        row.update(timed(fns, calls))
        row["tiled_fwd"]["Gevals_per_s"] = evals / row["tiled_fwd"]["ms"] / 1e6
        if si < BESIDE:
            row["lds_fwd"]["Gevals_per_s"] = evals / row["lds_fwd"]["ms"] / 1e6
            row["lds_over_tiled_fwd"] = row["lds_fwd"]["ms"] / row["tiled_fwd"]["ms"]
            row["lds_over_tiled_fwd_bwd"] = row["lds_fwd_bwd"]["ms"] / row["tiled_fwd_bwd"]["ms"]
        if (R, N, M) == (1, 65536, 65536):
            tiles = timed({str(t): (lambda t=t: ag.chamfer_tiled(x, y, tile=t)) for t in TILES}, calls)
            row["fwd_ms_by_tile"] = {k: v["ms"] for k, v in tiles.items()}
        by_shape[(R, N, M)] = row
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del x, y
    a, b = by_shape[(1, 16384, 16384)], by_shape[(1, 65536, 65536)]
    result["growth_65536_over_16384"] = {"work": 16.0, "fwd": b["tiled_fwd"]["ms"] / a["tiled_fwd"]["ms"],
                                         "fwd_bwd": b["tiled_fwd_bwd"]["ms"] / a["tiled_fwd_bwd"]["ms"]}
    result["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result["growth_65536_over_16384"]))


if __name__ == "__main__":
    main()
