#!/usr/bin/env python
"""Does one work list per launch chunk beat one per candidate?  A CPU census for Options::edge_order = 2 (csrc/ag_edges.hip:
k_chunk_count / k_chunk_scan / k_chunk_fill), the sibling of tools/zero_skip_census.py and built on its layers_of_forward.

numpy only, no GPU.  `--candidates N` consecutive candidates of bench.py's batch (from --first on) are stepped by the oracle for
the first forwards of look-ahead step 0.  For every forward the hidden activations of the relation encoder (the inputs of L2, L3
and W1) are laid out twice:
  * candidate order (Options::edge_order = 1, what ships): every candidate's own class-major list, tiles of 128 rows and
    wavefronts of 32 inside it, the candidates one after the other;
  * chunk order (Options::edge_order = 2): ONE list over the N candidates, sorted by chunk_keys below - the numpy restatement of
    the device key - and inside a key by candidate.
Printed per layer, for the tiles that start among the object-object entries and for the others (tool) separately: the shares of
(wavefront, k-step) pairs that are dead / half-dead / live and the mean MFMA issue cycles per k-step they stand for (dead 0,
half-dead 192, live 320), with the quarter barriers modelled as in zero_skip_census.py.

The key (all comparisons, no transcendental; a NaN compares false and lands in a defined bin):
  * object-object slot (receiver i, position t in the receiver's row): the transposed slot index t * N + i.  The candidates of a
    chunk start from one cloth and stay close to it, so the same slot of 32 candidates is as alike as 32 rows can be; and the
    senders of a row ascend, so consecutive keys - one position, consecutive receivers - are mostly one direction on a grid, and
    the four wavefronts of a tile are alike too (--oo-key slot: the receiver-major slot index i * stride + t, for comparison);
  * a slot with a tool at either end: n_slots + sector * TOOL_BINS + bin of d = pos_r - pos_s at the frame the builder read, with
    sector = ((d.x < 0) + 2 (d.z < 0) + 4 (|d.z| > |d.x|)) * 4 + #{k : min(|d.x|, |d.z|) >= TAN[k] * max(|d.x|, |d.z|)}
    (32 sectors of 11.25 degrees in the x-z plane) and bin = #{k : |d|^2 >= RING[k] * thr^2} (16 rings).
--sectors / --bins try other counts (sectors 8, 16, 32; bins 1..16 as every (16 / bins)-th ring): how the counts were chosen.

  python tools/chunk_order_census.py [--candidates 32] [--first 0] [--forwards 3] [--sectors 32] [--bins 16] [--oo-key position|slot]
                                     [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import zero_skip_census as Z  # noqa: E402

F32 = np.float32
TOOL_SECTORS, TOOL_BINS = 32, 16
# tan(11.25), tan(22.5), tan(33.75 degrees), rounded to fp32 (the device holds the same three literals)
TAN = np.asarray([0.19891237, 0.41421357, 0.66817864], F32)
# rings of |d|^2 / thr^2: radii 1, 2, ... 15 adjacency thresholds
RING = np.asarray([float(k * k) for k in range(1, TOOL_BINS)], F32)


def tool_keys(d, thr2, sectors=TOOL_SECTORS, bins=TOOL_BINS):
    """0 .. sectors * bins - 1 for every row of d (n, 3) = pos_r - pos_s in fp32; thr2 = fl(thr * thr)"""
    d = np.asarray(d, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        ax, az = np.abs(d[:, 0]), np.abs(d[:, 2])
        swap = az > ax
        mn, mx = np.where(swap, ax, az), np.where(swap, az, ax)
        fine = np.zeros(len(d), np.int64)
        for t in TAN:
            fine += mn >= (t * mx).astype(F32)
        sector = ((d[:, 0] < 0) * 1 + (d[:, 2] < 0) * 2 + swap * 4) * 4 + fine
        sector //= TOOL_SECTORS // sectors
        d2 = ((d[:, 0] * d[:, 0]).astype(F32) + (d[:, 1] * d[:, 1]).astype(F32)).astype(F32)
        d2 = (d2 + (d[:, 2] * d[:, 2]).astype(F32)).astype(F32)
        ring = np.zeros(len(d), np.int64)
        for k, c in enumerate(RING):
            if (k + 1) % (TOOL_BINS // bins) == 0:
                ring += d2 >= (c * F32(thr2)).astype(F32)
    return sector * bins + ring


def chunk_keys(slot, tool, d, thr2, n_slots, sectors=TOOL_SECTORS, bins=TOOL_BINS):
    """key of every entry: slot (object-object) or n_slots + tool key"""
    key = np.asarray(slot, np.int64).copy()
    tool = np.asarray(tool, bool)
    key[tool] = n_slots + tool_keys(np.asarray(d, F32)[tool], thr2, sectors, bins)
    return key


def chunk_list(per_cand, thr2, n_slots, sectors=TOOL_SECTORS, bins=TOOL_BINS):
    """per_cand: one (slot, tool, d) triple of arrays per live candidate, over its non-self slots.  Returns (cand, index into the
    candidate's arrays, key) of the chunk list in order, and the number of entries in front of the first tool key."""
    cand = np.concatenate([np.full(len(s), b, np.int64) for b, (s, _, _) in enumerate(per_cand)])
    idx = np.concatenate([np.arange(len(s), dtype=np.int64) for s, _, _ in per_cand])
    key = np.concatenate([chunk_keys(s, t, d, thr2, n_slots, sectors, bins) for s, t, d in per_cand])
    order = np.lexsort((idx, cand, key))                      # by key, inside a key by candidate
    return cand[order], idx[order], key[order], int((key < n_slots).sum())


def slots_of(recv, n_particles):
    """slot index (receiver * stride + position in the receiver's row) of a receiver-major edge list; also returns the stride"""
    recv = np.asarray(recv, np.int64)
    assert (np.diff(recv) >= 0).all(), "edges must be receiver-major"
    first = np.searchsorted(recv, np.arange(n_particles))
    pos_in_row = np.arange(len(recv)) - first[recv]
    return recv, pos_in_row


def accumulate(tot, name, layer, act, n_oo):
    for scope, mask in (("object-object tiles", lambda e0: e0 < n_oo), ("tool tiles", lambda e0: e0 >= n_oo)):
        h = Z.step_shares(act, 0, mask)
        k = (name, layer, scope)
        tot[k] = tuple(x + y for x, y in zip(tot.get(k, (0,) * 8), h))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--candidates", type=int, default=32)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--forwards", type=int, default=3)
    ap.add_argument("--sectors", type=int, default=TOOL_SECTORS, choices=[8, 16, 32])
    ap.add_argument("--bins", type=int, default=TOOL_BINS, choices=[1, 2, 4, 8, 16])
    ap.add_argument("--oo-key", default="position", choices=["position", "slot"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import bench
    from oracle import adaptigraph_oracle as O

    rng = np.random.default_rng(0)
    cloud = bench.cloth_cloud(45, rng)
    N_o = cloud.shape[0]
    task = bench.make_task(max_nR=int(1.2 * 6 * (N_o + 1)) + 64)
    W = bench.random_weights(0)
    actions = bench.make_actions(1024, 2, 10, cloud, rng)
    picks = list(range(args.first, args.first + args.candidates))
    a = actions[picks, :1].copy()
    a[..., 3] = args.forwards + 0.5
    trace = []
    O.dynamics(W, 3, cloud, a, task, trace=trace)
    dec, _ = O.decode_action(a, task["push_length"])
    _, delta = O.tool_keypoints(dec, a[..., 2], task)
    N = N_o + 1
    attrs = np.zeros((N, 2), F32); attrs[:N_o, 0] = 1; attrs[N_o:, 1] = 1
    group = np.zeros((N, 1), F32); group[:N_o] = 1
    phys = np.zeros(N, F32); phys[:N_o] = 0.5
    thr2 = F32(task["adj_thresh"]) * F32(task["adj_thresh"])
    stride = max(int(np.bincount(rec["recv"], minlength=N).max()) for recs in trace for rec in recs)
    n_slots = N * stride
    tot = {}
    entries = [0, 0]
    for k in range(args.forwards):
        acts = {"L2": [], "L3": [], "W1": []}
        per_cand = []
        for ci, recs in enumerate(trace):
            rec = recs[k]
            states = [recs[0]["state_last"]] * 3 + [r["state_last"] for r in recs[:k + 1]]
            hist = np.stack(states[-4:], 0).astype(F32)
            action = np.zeros((N, 3), F32); action[N_o:] = delta[ci, 0]
            recv, send = rec["recv"], rec["send"]
            ns = np.flatnonzero(recv != send)
            r_all, t_all = slots_of(recv, N)
            slot = (r_all * stride + t_all)[ns] if args.oo_key == "slot" else (t_all * N + r_all)[ns]
            tool = (recv[ns] >= N_o) | (send[ns] >= N_o)
            d = hist[-1][recv[ns]] - hist[-1][send[ns]]
            per_cand.append((slot, tool, d))
            perm, n_oo = Z.work_list_order(recv[ns], send[ns], hist[-1], N_o, "class")
            layers = Z.layers_of_forward(O, W, hist, attrs, recv, send, group, action, phys, 3, "slot", N_o)
            for chain, layer, act in layers:
                if chain != "edge":
                    break
                live = act != 0
                acts[layer].append(live)
                accumulate(tot, "candidate", layer, live[perm], n_oo)
        cand, idx, key, n_oo = chunk_list(per_cand, thr2, n_slots, args.sectors, args.bins)
        entries[0] += n_oo; entries[1] += len(key) - n_oo
        base = np.concatenate([[0], np.cumsum([len(s) for s, _, _ in per_cand])])
        rows = base[cand] + idx
        for layer, parts in acts.items():
            accumulate(tot, "chunk", layer, np.concatenate(parts, 0)[rows], n_oo)
    print(f"chunk-order census: bench batch, candidates {picks[0]}..{picks[-1]}, forwards 1..{args.forwards} of look-ahead step 0; "
          f"stride {stride}, object-object key by {args.oo_key}, tool key {args.sectors} sectors x {args.bins} rings; "
          f"{entries[0]} object-object and {entries[1]} tool entries")
    print(f"{'order':10s} {'layer':6s} {'tiles':20s} {'dead':>7s} {'half':>7s} {'live':>7s} {'cyc now':>8s} {'cyc half':>9s} "
          f"{'half, barriers':>15s}")
    out = {"first": picks[0], "candidates": args.candidates, "forwards": args.forwards, "sectors": args.sectors, "bins": args.bins,
           "stride": stride, "rows": []}
    for (name, layer, scope), (de, ha, li, n, c0, c1, b0, b1) in sorted(tot.items(), key=lambda kv: (kv[0][2], kv[0][1], kv[0][0])):
        if n == 0:
            continue
        print(f"{name:10s} {layer:6s} {scope:20s} {100 * de / n:6.2f}% {100 * ha / n:6.2f}% {100 * li / n:6.2f}% {c0 / n:8.1f} "
              f"{c1 / n:9.1f} {b1 / n:15.1f}")
        out["rows"].append({"order": name, "layer": layer, "tiles": scope, "dead": de / n, "half": ha / n, "live": li / n, "pairs": n,
                            "cycles_now": c0 / n, "cycles_half_step": c1 / n, "cycles_half_step_barriers": b1 / n})
    for name in ("candidate", "chunk"):
        cyc = sum(v[5] for k_, v in tot.items() if k_[0] == name)
        n = sum(v[3] for k_, v in tot.items() if k_[0] == name and k_[1] == "L2")
        print(f"{name:10s} L2 + L3 + W1, all tiles: {cyc / n:7.1f} issue cycles per k-step triple")
        out[f"{name}_cycles_per_triple"] = cyc / n
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
