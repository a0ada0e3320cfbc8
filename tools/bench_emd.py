#!/usr/bin/env python3
"""Earth-mover benchmark: what the device-side assignment solve (ag_emd.hip) costs, next to the host route it replaces.

  loss    B = 128, N = M = 40, 100, 300, seeded random clouds: EarthMoverLoss forward + backward on the device, and the host route
          in the same process - the distance matrix on the device, one copy out, scipy.optimize.linear_sum_assignment per graph
          (the numpy restatement tests/emd_restate.py where scipy is not importable), the gather and the mean on the device.
          The device's assignments are compared with the host's ("equal").
  shape   (B, N, M) = (128, 100, 100), forward only, under every library given with --libs (name=path; the product library is
          always "wg256"): the launch-shape comparison of k_emd_assign (docs/EXPERIMENTS.md).  The children alternate.
  chain   one graph of the adversarial "chain" layout (two parallel lines, the label shifted by K/2 along them: the search of row
          r scans all r matched columns, K (K + 1) / 2 steps in all) at K = 128, 256, 512: what one launch can cost at the cap.
  train   a TrainStep iteration at B = 128 rope (the training fixture's graphs repeated) with and without the term.

Each section runs in a child process of its own under a time limit of its own; the first child that fails ends the run (nothing
more is started on the device).  Device times are HIP events around `calls` back-to-back calls after a warm-up, per call = elapsed
/ calls, median over `rounds`; host-route times are wall time around work that ends in a synchronise.  No pass / fail threshold.

  python tools/bench_emd.py [--rounds 7] [--libs wave64=adaptigraph_amd/csrc/libadaptigraph_hip_emdwave.so] [--out profiles/r21_emd.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = {"loss": 420, "shape": 240, "chain": 240, "train": 420}


def random_clouds(B, N, M, seed=0):
    import numpy as np
    rng = np.random.default_rng([seed, B, N, M])
    x = rng.normal(0, 0.3, (B, N, 3)).astype(np.float32)
    y = (x[:, rng.integers(0, N, M)] + rng.normal(0, 0.1, (B, M, 3))).astype(np.float32)
    return x, y


def chain_clouds(K):
    import numpy as np
    rng = np.random.default_rng(K)
    x = np.stack([np.arange(K) * 1.0, np.zeros(K), np.zeros(K)], 1)
    y = np.stack([np.arange(K) * 1.0 + K / 2, np.full(K, 0.5), np.zeros(K)], 1)
    return ((x + rng.normal(0, 0.01, x.shape))[None] * 0.05).astype(np.float32), ((y + rng.normal(0, 0.01, y.shape))[None] * 0.05).astype(np.float32)


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


def forward_only(ag, x, y):
    import torch
    from adaptigraph_amd.context import ptr, current_stream
    eng = ag.default_engine(x.device)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    out = torch.empty((), device=x.device)
    work = torch.empty(B * (N + M) + 4, device=x.device, dtype=torch.int32)
    return lambda: eng.check(eng.lib.ag_set_loss(eng.ctx, current_stream(x.device), ptr(x), ptr(y), B, N, M, B, 3, ptr(out), ptr(work)))


def child(section, rounds):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import adaptigraph_amd as ag
    import emd_restate as ER
    dev = torch.device("cuda:0")
    res = {"section": section, "rounds": rounds, "device": torch.cuda.get_device_name(dev)}
    if section == "loss":
        try:
            from scipy.optimize import linear_sum_assignment as lsa
            res["host_solver"] = "scipy.optimize.linear_sum_assignment"
        except ImportError:
            lsa = lambda c: ER.solve(c)[:2]   # noqa: E731
            res["host_solver"] = "tests/emd_restate.py"
        loss = ag.EarthMoverLoss()
        for n in (40, 100, 300):
            xn, yn = random_clouds(128, n, n)
            y = torch.from_numpy(yn).to(dev)
            x = torch.from_numpy(xn).to(dev).requires_grad_(True)

            def device():
                x.grad = None
                loss(x, y).backward()

            def host():
                x.grad = None
                dis = torch.cdist(x.detach(), y).cpu().numpy()          # the copy out waits for the device
                idx = [lsa(d) for d in dis]
                i1 = torch.from_numpy(np.stack([i[0] for i in idx])).to(dev)
                i2 = torch.from_numpy(np.stack([i[1] for i in idx])).to(dev)
                b = torch.arange(x.shape[0], device=dev)[:, None]
                torch.linalg.vector_norm(x[b, i1] - y[b, i2], dim=2).mean().backward()
                torch.cuda.synchronize()
                return i1, i2
            d = timed(device, 10, rounds)
            g_dev = x.grad.clone()
            wall = []
            for _ in range(max(3, rounds // 2)):
                t0 = time.perf_counter()
                i1, i2 = host()
                wall.append((time.perf_counter() - t0) * 1e3)
            a1, a2 = ag.earth_mover_assignment(x, y)
            res[f"N{n}"] = {"B": 128, "device_fwd_bwd": d, "host_route_ms": float(np.median(wall)), "host_route_min_ms": float(min(wall)),
                            "equal": bool(torch.equal(a1, i1) and torch.equal(a2, i2)),
                            "grad_max_diff": float((g_dev - x.grad).abs().max())}
    elif section == "shape":
        xn, yn = random_clouds(128, 100, 100)
        run = forward_only(ag, torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev))
        res["B128_N100_forward"] = timed(run, 20, rounds)
        for K in (128, 256, 512):
            xc, yc = chain_clouds(K)
            res[f"chain_K{K}"] = timed(forward_only(ag, torch.from_numpy(xc).to(dev), torch.from_numpy(yc).to(dev)), 2, rounds)
        res["lib"] = os.path.basename(ag._lib.LIB_PATH)
    elif section == "chain":
        for K in (128, 256, 512):
            xc, yc = chain_clouds(K)
            steps = int(ER.solve(ER.cost_matrix(xc[0], yc[0], np.float32))[2].sum())
            x, y = torch.from_numpy(xc).to(dev), torch.from_numpy(yc).to(dev)
            t = timed(forward_only(ag, x, y), 2, rounds)
            i1, i2 = ag.earth_mover_assignment(x, y)
            r1, r2 = ER.assignment(xc, yc, np.float32)
            # the layout is built for its step count, not for a unique optimum: compare the cost, not the indices
            cost = ER.cost_matrix(xc[0], yc[0], np.float32)
            t.update(search_steps=steps, worst_case_steps=K * (K + 1) // 2,
                     cost_device=float(cost[i1[0].cpu().numpy(), i2[0].cpu().numpy()].sum()), cost_restatement=float(cost[r1[0], r2[0]].sum()))
            res[f"K{K}"] = t
    elif section == "train":
        import train_restate as TR
        from test_gpu_train_step import _data, _train_step, _max_edges
        f = TR.load_fixture("train_emd_rope.npz")
        data = _data(f, dev, idx=np.arange(128) % f["attrs"].shape[0])
        k = _max_edges(data)
        for name, losses in (("mse", [("mse", 1.0)]), ("mse_emd", [("mse", 1.0), (ag.EarthMoverLoss(), 0.5)]),
                             ("mse_chamfer", [("mse", 1.0), ("chamfer", 0.5)])):
            ts, _ = _train_step(dev, f, losses=losses)
            res[name] = timed(lambda: ts.step(data, max_edges=k), 10, rounds)
            ts.check()
        res["B"], res["n_p"], res["n_future"] = 128, int(f["p_instance"].shape[1]), int(f["n_future"])
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--libs", nargs="*", default=[])
    ap.add_argument("--sections", nargs="*", default=["loss", "chain", "train", "shape"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_emd.json"))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rounds)
    libs = [("wg256", None)] + [tuple(s.split("=", 1)) for s in a.libs]
    jobs = [(s, "wg256", None) for s in a.sections if s != "shape"]
    if "shape" in a.sections:
        jobs += [("shape", name, path) for _ in range(2) for name, path in libs]          # alternating, twice each
    out = {"rounds": a.rounds, "results": []}
    for section, name, path in jobs:
        env = dict(os.environ)
        if path:
            env["ADAPTIGRAPH_AMD_LIB"] = os.path.abspath(path)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", section, "--rounds", str(a.rounds)], env=env,
                           capture_output=True, text=True, timeout=LIMIT_S[section])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            raise SystemExit(f"bench_emd: section {section} ({name}) failed with exit code {p.returncode}; nothing more is started")
        r = json.loads(line[0][7:])
        r["variant"] = name
        out["results"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
