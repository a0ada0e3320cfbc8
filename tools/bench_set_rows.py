#!/usr/bin/env python3
"""Set losses over real rows (AG_LOSS_ROWS): what the flagged kinds cost, and that the plain kinds cost what they did.

  loss    B = 128, N = M = 100, seeded random clouds: forward + backward (ag_set_loss, then ag_set_loss_backward on its tables) of
          Chamfer, Hausdorff and Earth-mover, the plain kinds and - where the library knows the flag - the flagged kinds with counts
          uniform in [50, 100].
  train   a TrainStep iteration at B = 128 rope (the training fixture's graphs repeated, n_p = 40) with
          [mse, chamfer, hausdorff] and with [mse, earth_mover], plain and - where known - real_rows=True on the same batch with
          live prefixes uniform in [20, 40] marked in attrs.

Every variant is a library: "change" is the product library, every name=path given with --libs another build of the same exports
(the parent commit's, built from a clean checkout) loaded through ADAPTIGRAPH_AMD_LIB; a library that refuses the flag is measured
on the plain kinds only.  The variants alternate, --runs times each, one child process per run under a time limit of its own; the
first child that fails ends the run.  Device times are HIP events around `calls` back-to-back calls after a warm-up, per call =
elapsed / calls, median over `rounds`.  No pass / fail threshold.

  python tools/bench_set_rows.py --libs parent=/path/to/parent/libadaptigraph_hip.so [--runs 3] [--out profiles/r22_set_rows.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_emd import random_clouds, timed  # noqa: E402

LIMIT_S = 300
KINDS = {"chamfer": 1, "hausdorff": 2, "earth_mover": 3}
ROWS = 16


def fwd_bwd(ag, x, y, kind, counts=None):
    """-> (callable, return code of one trial call)"""
    import torch
    from adaptigraph_amd.context import ptr, current_stream
    eng = ag.default_engine(x.device)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    out, g, go = torch.empty((), device=x.device), torch.empty_like(x), torch.ones(1, device=x.device)
    work = torch.zeros(B * (N + M) + 4 + 2 * B, device=x.device, dtype=torch.int32)
    if counts is not None:
        work[B * (N + M) + 4:] = counts.reshape(-1)
        kind |= ROWS
    st = current_stream(x.device)

    def run():
        rc = eng.lib.ag_set_loss(eng.ctx, st, ptr(x), ptr(y), B, N, M, B, kind, ptr(out), ptr(work))
        return rc or eng.lib.ag_set_loss_backward(eng.ctx, st, ptr(x), ptr(y), B, N, M, B, kind, ptr(go), ptr(g), ptr(work))
    return run, run()


def child(rounds):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import adaptigraph_amd as ag
    import train_restate as TR
    from test_gpu_train_step import _data, _train_step, _max_edges
    dev = torch.device("cuda:0")
    res = {"rounds": rounds, "device": torch.cuda.get_device_name(dev), "lib": ag._lib.LIB_PATH, "loss": {}, "train": {}}
    B, N = 128, 100
    xn, yn = random_clouds(B, N, N)
    x, y = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)
    rng = np.random.default_rng(22)
    counts = torch.from_numpy(rng.integers(50, 101, (2, B)).astype(np.int32)).to(dev)
    for name, kind in KINDS.items():
        for tag, c in (("plain", None), ("rows", counts)):
            run, rc = fwd_bwd(ag, x, y, kind, c)
            res["loss"][f"{name}_{tag}"] = timed(run, 20, rounds) if rc == 0 else {"refused": rc}
    res["has_rows"] = "refused" not in res["loss"]["chamfer_rows"]
    f = TR.load_fixture("train_losses_rope.npz")
    f = {k: np.array(f[k]) for k in f.keys()}
    idx = np.arange(B) % f["attrs"].shape[0]
    data = _data(f, dev, idx=idx)
    n_p = f["p_instance"].shape[1]
    live = torch.from_numpy(rng.integers(n_p // 2, n_p + 1, B)).to(dev)
    padded = dict(data)
    padded["attrs"] = data["attrs"].clone()
    padded["attrs"][:, :n_p, 0] = (torch.arange(n_p, device=dev)[None] < live[:, None]).float()
    k = _max_edges(data)
    lists = {"mse_chamfer_hausdorff": [("mse", 1.0), ("chamfer", 0.5), ("hausdorff", 0.25)],
             "mse_earth_mover": [("mse", 1.0), (ag.EarthMoverLoss(), 0.5)]}
    for name, losses in lists.items():
        ts, _ = _train_step(dev, f, losses=losses)
        res["train"][name + "_plain"] = timed(lambda: ts.step(data, max_edges=k), 10, rounds)
        ts.check()
        if res["has_rows"]:
            tr, _ = _train_step(dev, f, losses=losses, real_rows=True)
            res["train"][name + "_rows"] = timed(lambda: tr.step(padded, max_edges=k), 10, rounds)
            tr.check()
    res["shape"] = {"loss": [B, N, N], "train": [B, int(n_p), int(f["n_future"])]}
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--libs", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_set_rows.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.rounds)
    libs = [tuple(s.split("=", 1)) for s in a.libs] + [("change", None)]
    out = {"rounds": a.rounds, "runs": a.runs, "results": []}
    for run in range(a.runs):
        for name, path in libs:                                  # alternating
            env = dict(os.environ)
            if path:
                env["ADAPTIGRAPH_AMD_LIB"] = os.path.abspath(path)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds)], env=env,
                               capture_output=True, text=True, timeout=LIMIT_S)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                raise SystemExit(f"bench_set_rows: run {run} of {name} failed with exit code {p.returncode}; nothing more is started")
            r = json.loads(line[0][7:])
            r.update(variant=name, run=run, lib=os.path.basename(r["lib"]))
            out["results"].append(r)
            print(json.dumps(r), flush=True)
    # the table: per measurement and variant the runs' medians, and whether the change's plain kinds lie inside the parent's own range
    table = {}
    for r in out["results"]:
        for sec in ("loss", "train"):
            for key, t in r[sec].items():
                if "ms" in t:
                    table.setdefault(f"{sec}.{key}", {}).setdefault(r["variant"], []).append(round(t["ms"], 5))
    out["table_ms"] = table
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    for key, v in table.items():
        print(key, v)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
