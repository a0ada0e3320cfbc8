#!/usr/bin/env python3
"""Cell-list edge builder benchmark: per-call time of construct_edges_cells (ag_build_edges_cells) on two clouds of constant
density - a jittered sheet of pitch 0.3 (thr 0.75, topk 5, one tool above the centre, connect_tools_all) and a uniform pile of
125 particles per unit volume (thr 0.4, topk 20, 5 tools) - at N = 4096 next to the LDS-resident builder (construct_edges_index),
whose limit that is, and alone at 16,384, 65,536 and 262,144.  At 16,384 and 65,536 a chunked torch brute force over all N^2 pairs
(the same fp32 operations, one torch kernel each, so nothing is contracted; top-k by the (distance, index) key) is timed as the
baseline and must produce the same edge lists: the large-N equality check, here because it takes longer than a test may.

"pair tests" is the number of (receiver, sender) distance evaluations the cell builder executes: per receiver, the particles in the
27 cells around its own, counted on the host from the restated grid (tests/cells_restate.py).  scaling_65536_over_16384 is the
ratio of the per-graph times: 4 if the work is linear in N, 16 if quadratic.

Each size runs in a child process of its own under a time limit of its own; the first child that fails ends the run (nothing more is
started on the device).  Device times are HIP events around `calls` back-to-back calls after a warm-up, per-call = elapsed / calls,
median over `rounds`.  No pass / fail threshold on time.

  python tools/bench_cells.py [--rounds 7] [--out profiles/r24_cells.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [4096, 16384, 65536, 262144]
BRUTE = (16384, 65536)
LIMIT_S = {4096: 240, 16384: 300, 65536: 420, 262144: 300}


def cloud(kind, n):
    import numpy as np
    rng = np.random.default_rng(n + len(kind))
    if kind == "sheet":
        side = int(round(n ** 0.5))
        assert side * side == n
        ii, jj = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
        pos = np.stack([ii.ravel() * 0.3, np.zeros(n), jj.ravel() * 0.3], 1) + rng.normal(0, 0.02, (n, 3))
        pos[-1] = [(side - 1) * 0.15, 0.1, (side - 1) * 0.15]
        tool = np.zeros(n, bool)
        tool[-1] = True
        return pos.astype(np.float32), tool, 0.75, 5, True
    edge = (n / 125.0) ** (1.0 / 3.0)
    pos = rng.uniform(0, edge, (n, 3))
    tool = np.zeros(n, bool)
    tool[-5:] = True
    return pos.astype(np.float32), tool, 0.4, 20, False


def pair_tests(pos, thr):
    """Distance evaluations of k_cells_rows: per binned receiver, the members of the 27 cells around its own."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cells_restate as R
    g = R.make_grid(pos, np.float32(thr) * np.float32(thr), R.cells_cap_for(len(pos)))
    c = R.cells_of(pos, g)
    n = g["n"]
    cnt = np.zeros(tuple(n + 2), np.int64)
    np.add.at(cnt, (c[:, 0] + 1, c[:, 1] + 1, c[:, 2] + 1), 1)
    around = np.zeros_like(cnt)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                around += np.roll(cnt, (dx, dy, dz), (0, 1, 2))        # (the one-cell rim is empty, so nothing wraps)
    return int((cnt * around).sum()), [int(x) for x in n]


def brute_force(torch, pos, tool, thr, topk, cta, chunk=1024):
    """All N^2 pairs on the device, `chunk` receivers at a time -> (recv, send) int64, sorted by (receiver, sender)."""
    N = pos.shape[0]
    thr2 = torch.tensor(thr, dtype=torch.float32, device=pos.device) ** 2
    big = torch.iinfo(torch.int64).max
    idx = torch.arange(N, device=pos.device)
    recv, send, flag = [], [], False
    for r0 in range(0, N, chunk):
        p = pos[r0:r0 + chunk]
        d = p[:, None, :] - pos[None, :, :]
        sq = d * d
        dis = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        within = ((dis - thr2) < 0) & ~(tool[r0:r0 + chunk, None] & tool[None, :])
        key = torch.where(within, (dis.view(torch.int32).to(torch.int64) << 32) | idx[None, :], torch.full_like(idx, big)[None, :])
        kept = torch.topk(key, min(topk, N), dim=1, largest=False).values
        ok = kept != big
        r = (idx[r0:r0 + chunk, None].expand_as(kept))[ok]
        s = (kept & 0xffffffff)[ok]
        if cta:                                                         # the batch rule: tool rows and tool senders leave ...
            flag = flag or bool((tool[r] & ~tool[s]).any())
            keep = ~tool[r] & ~tool[s]
            r, s = r[keep], s[keep]
        recv.append(r)
        send.append(s)
    recv, send = torch.cat(recv), torch.cat(send)
    if cta and flag:                                                    # ... and every tool sends to every particle
        t = idx[tool]
        recv = torch.cat([recv, idx.repeat_interleave(len(t))])
        send = torch.cat([send, t.repeat(N)])
    order = torch.argsort(recv * N + send)
    return recv[order], send[order]


def one(n, rounds):
    """The child: everything at one size; prints one JSON line."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import adaptigraph_amd as ag
    dev = torch.device("cuda:0")
    calls = 20 if n <= 65536 else 10
    res = {"particles": n, "calls_per_round": calls, "rounds": rounds, "device": torch.cuda.get_device_name(dev)}

    def timed(run, calls):
        for _ in range(3):
            out = run()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                run()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / calls)
        return out, {"ms_per_call_median": float(np.median(ms)), "ms_per_call_rounds": [round(x, 4) for x in ms]}

    for kind in ("sheet", "pile"):
        pos_h, tool_h, thr, topk, cta = cloud(kind, n)
        pos, tool = torch.from_numpy(pos_h).to(dev), torch.from_numpy(tool_h).to(dev)
        mask = torch.ones(n, dtype=torch.bool, device=dev)
        cap = n * (topk + int(tool_h.sum()))
        tests, cells = pair_tests(pos_h, thr)
        entry = {"thr": thr, "topk": topk, "connect_tools_all": cta, "pair_tests": tests, "cells_per_axis": cells}
        el, t = timed(lambda: ag.construct_edges_cells(pos[None], thr, mask[None], tool[None], topk, cta, edge_cap=cap), calls)
        E = int(el.n_edges[0].item())
        t["pair_tests_per_s"] = tests / (t["ms_per_call_median"] * 1e-3)
        entry["cells"], entry["edges"] = t, E
        if n <= 4096:
            lds, t = timed(lambda: ag.construct_edges_index(pos[None], thr, mask[None], tool[None], topk, cta, edge_cap=cap), calls)
            t["equal"] = bool(torch.equal(lds.n_edges, el.n_edges) and torch.equal(lds.row_ptr, el.row_ptr) and
                              torch.equal(lds.recv[0, :E], el.recv[0, :E]) and torch.equal(lds.send[0, :E], el.send[0, :E]))
            entry["lds"] = t
            entry["cells_over_lds"] = entry["cells"]["ms_per_call_median"] / t["ms_per_call_median"]
        if n in BRUTE:
            (r, s), t = timed(lambda: brute_force(torch, pos, tool, thr, topk, cta), 1)
            t["equal"] = bool(len(r) == E and torch.equal(r.to(torch.int32), el.recv[0, :E]) and torch.equal(s.to(torch.int32), el.send[0, :E]))
            entry["torch_brute_force"] = t
            entry["brute_force_over_cells"] = t["ms_per_call_median"] / entry["cells"]["ms_per_call_median"]
        res[kind] = entry
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one is not None:
        return one(a.one, a.rounds)
    res = {"tool": "bench_cells", "clouds": "sheet: jittered grid, pitch 0.3, N(0, 0.02^2); pile: uniform, 125 per unit volume; fp32, seeded",
           "timing": "HIP events around calls_per_round back-to-back calls after 3 warm-up calls (brute force: 1 call); median of the rounds",
           "sizes": {}}
    for n in SIZES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), "--rounds", str(a.rounds)],
                               capture_output=True, text=True, timeout=LIMIT_S[n])
        except subprocess.TimeoutExpired:
            res["stopped"] = f"{n} particles: no result within {LIMIT_S[n]} s; nothing further was started"
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            res["stopped"] = f"{n} particles: exit status {p.returncode}; nothing further was started"
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            break
        res["sizes"][str(n)] = json.loads(lines[-1][len("RESULT "):])
        print(f"{n} particles: done", file=sys.stderr, flush=True)
    s = res["sizes"]
    if "16384" in s and "65536" in s:
        res["scaling_65536_over_16384"] = {k: s["65536"][k]["cells"]["ms_per_call_median"] / s["16384"][k]["cells"]["ms_per_call_median"]
                                          for k in ("sheet", "pile")}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    sys.exit(main())
