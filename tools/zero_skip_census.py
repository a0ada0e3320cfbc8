#!/usr/bin/env python
"""How many k-steps of the fp32 chains are all zero?  A CPU census for Options::zero_skip (csrc/ag_mlp.hip: mma_act).

numpy only, no GPU.  Inputs are bench.py's own: random_weights(0), the jittered 45 x 45 cloth, the first draw of the 1024
actions.  A few candidates of that batch are stepped by the oracle for the first forwards of look-ahead step 0; for every
forward the hidden activations of the model are recomputed with the oracle's feature assembly (model_forward_single) and
laid out as the engine sees them:
  * relation-encoder chain (k_edge_enc): the candidate's edges in the reference's order (receiver-major), self-loops left
    out (they take a constant C row), 32 consecutive ones per wavefront;
  * propagate chains (k_node_prop): dense rows candidate * N + particle, 32 consecutive ones per wavefront (a wavefront that
    straddles two candidates is counted with the rows of the simulated candidate only);
  * k-step s of a 160-wide layer = features (lo, lo + 4), lo = 32 t + (r & 3) + 8 (r >> 2), (t, r) = (s / 16, s % 16) for
    s < 64 and (4, s - 64) above: the packed K order.  Slot 150 is the bias slot (always 1.0), 151 is padding (always 0).
Printed per layer: the share of (wavefront, k-step) pairs whose two features are zero in all rows of the wavefront - the
MFMAs zero_skip leaves out - and the share of (wavefront, 4-step chunk) pairs that are dead as a whole (their weight-fragment
reads go too).  Not modelled: the shared first forward (its object-object edges are encoded once per call, not per candidate).

--order: the order of the relation encoder's work list (Options::edge_order, csrc/ag_edges.hip: k_ell_index).  `slot` is the
receiver-major slot order; `tool-last` moves the edges with a tool at either end behind the object-object ones; `class` is the
engine's class-major list: object-object edges by (d.x < 0, d.y < 0, d.z < 0) x argmax(|d.x|, |d.y|, |d.z|) of d = pos_r - pos_s
at the current frame (ties to the lower axis, a NaN compares false), the tool class last, slot order inside a class
(work_list_order below is the numpy restatement of that key).  The propagate chains do not depend on it.

Behind that output (its format is a prefix of this tool's output) comes the census for Options::half_step: a k-step with exactly ONE
of its two features zero in all rows of the wavefront takes 3 MFMAs (192 issue cycles) instead of 5 (320).  Per layer the shares of
(wavefront, k-step) pairs that are dead / half-dead / live - for the relation encoder also over the tiles (128 rows) that start among
the object-object classes and over the others, which is the gate of the engine's skip - and the mean MFMA issue cycles per k-step
they stand for, with the skip alone and with half-steps.  The quarter barriers are modelled as the slowest of a workgroup's four
wavefronts per quarter (k-steps 0-19, 20-39, 40-59, 60-75).

  python tools/zero_skip_census.py [--forwards 3] [--candidates 0,341,682,1023] [--order slot|tool-last|class] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32 = np.float32
NSTEP = 76


def step_features():
    lo = []
    for s in range(NSTEP):
        t, r = (s // 16, s % 16) if s < 64 else (4, s - 64)
        lo.append(32 * t + (r & 3) + 8 * (r >> 2))
    return np.asarray(lo)


LO = step_features()


def dead_share(act, first_row=0):
    """act (rows, 150) ReLU outputs in engine row order -> (dead k-steps, dead chunks, wavefront x k-step pairs, wavefront x chunk pairs)"""
    rows = act.shape[0]
    a = np.zeros((rows, 160), bool)
    a[:, :150] = act != 0
    a[:, 150] = True                                          # bias slot
    step_live_row = a[:, LO] | a[:, LO + 4]                   # (rows, 76)
    wave = (first_row + np.arange(rows)) // 32
    wave -= wave[0]
    n_wave = int(wave[-1]) + 1
    live = np.zeros((n_wave, NSTEP), bool)
    np.logical_or.at(live, wave, step_live_row)
    chunk_live = live.reshape(n_wave, NSTEP // 4, 4).any(2)
    return int((~live).sum()), int((~chunk_live).sum()), live.size, chunk_live.size


CYC_FULL, CYC_HALF = 320, 192                                 # 5 MFMAs of 64 cycles; 2 two-block MFMAs + 1


def step_shares(act, first_row=0, tile_mask=None):
    """act as for dead_share -> (dead, half-dead, live, wavefront x k-step pairs, issue cycles today, issue cycles with half-steps,
    the same two with every quarter of a 4-wavefront workgroup taking as long as its slowest wavefront).  tile_mask(first row of
    a 128-row tile) -> bool selects the tiles that are counted (None: all)."""
    rows = act.shape[0]
    a = np.zeros((rows, 160), bool)
    a[:, :150] = act != 0
    a[:, 150] = True
    wave = (first_row + np.arange(rows)) // 32
    wave -= wave[0]
    n_wave = int(wave[-1]) + 1
    lo = np.zeros((n_wave, NSTEP), bool)
    hi = np.zeros((n_wave, NSTEP), bool)
    np.logical_or.at(lo, wave, a[:, LO])
    np.logical_or.at(hi, wave, a[:, LO + 4])
    keep = np.ones(n_wave, bool)
    if tile_mask is not None:
        keep = np.asarray([bool(tile_mask((w // 4) * 128)) for w in range(n_wave)])
    lo, hi = lo[keep], hi[keep]
    n_live = lo.astype(int) + hi
    dead, half, live = int((n_live == 0).sum()), int((n_live == 1).sum()), int((n_live == 2).sum())
    cyc_now = np.where(n_live == 0, 0, CYC_FULL)
    cyc_hs = np.where(n_live == 0, 0, np.where(n_live == 1, CYC_HALF, CYC_FULL))
    bar = [0, 0]
    wg = np.flatnonzero(keep) // 4
    for i, cyc in enumerate((cyc_now, cyc_hs)):
        for q0, q1 in ((0, 20), (20, 40), (40, 60), (60, 76)):
            per_wave = cyc[:, q0:q1].sum(1)
            for g in np.unique(wg):
                sel = per_wave[wg == g]
                bar[i] += int(sel.max()) * len(sel)
    return dead, half, live, lo.size, int(cyc_now.sum()), int(cyc_hs.sum()), bar[0], bar[1]


N_CLASSES = 25


def edge_classes(recv, send, pos, n_obj):
    """class 0..24 of every edge (receiver, sender): k_ell_index's key, in fp32 like the kernel"""
    pos = np.asarray(pos, F32)
    d = pos[recv] - pos[send]
    ad = np.abs(d)
    ax = np.zeros(len(recv), np.int64)
    m = ad[:, 0].copy()
    up = ad[:, 1] > m
    ax[up] = 1
    m[up] = ad[up, 1]
    ax[ad[:, 2] > m] = 2
    cls = ((d[:, 0] < 0) * 1 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 4) * 3 + ax
    cls[(recv >= n_obj) | (send >= n_obj)] = N_CLASSES - 1
    return cls


def work_list_order(recv, send, pos, n_obj, order):
    """Permutation of the slot-order work list (the edges given, self-loops already left out): entry t of the engine's list is edge
    perm[t].  Also returns the number of entries in front of the tool class (the whole list for `slot`)."""
    n = len(recv)
    if order == "slot":
        return np.arange(n), n
    assert order in ("tool-last", "class"), order
    cls = edge_classes(recv, send, pos, n_obj)
    tool = cls == N_CLASSES - 1
    if order == "tool-last":
        cls = tool.astype(np.int64)
    return np.argsort(cls, kind="stable"), int((~tool).sum())


def layers_of_forward(O, W, hist, attrs, recv, send, group, action, phys, pstep, order="slot", n_obj=None):
    """the hidden activations of one forward, as model_forward_single computes them; yields (chain, layer, rows x 150)"""
    n_his, N, _ = hist.shape
    res = hist[1:] - hist[:-1]
    snt = np.ascontiguousarray(np.concatenate([res, hist[-1:]], 0).transpose(1, 0, 2)).reshape(N, n_his * 3)
    p_inputs = np.concatenate([attrs, phys[:, None], action], 1).astype(F32)
    gdiff = np.abs(group[recv] - group[send]).sum(1, keepdims=True)
    rel_inputs = np.concatenate([attrs[recv], attrs[send], gdiff, snt[recv] - snt[send]], 1).astype(F32)
    ns = np.flatnonzero(recv != send)                         # the relation encoder's work list
    ns = ns[work_list_order(recv[ns], send[ns], hist[-1], N if n_obj is None else n_obj, order)[0]]

    def enc(x, pre):
        hs = []
        for i in (0, 2, 4):
            x = O._relu(O._linear(x, W[f"{pre}.model.{i}.weight"], W[f"{pre}.model.{i}.bias"]))
            hs.append(x)
        return hs
    r1, r2, r_enc = enc(rel_inputs, "relation_encoder")
    yield "edge", "L2", r1[ns]
    yield "edge", "L3", r2[ns]
    yield "edge", "W1", r_enc[ns]
    p_enc = enc(p_inputs, "particle_encoder")[2]
    eff = p_enc
    Wrp, brp = W["relation_propagator.linear.weight"], W["relation_propagator.linear.bias"]
    Wpp, bpp = W["particle_propagator.linear.weight"], W["particle_propagator.linear.bias"]
    for ps in range(pstep):
        eff_rel = O._relu(O._linear(np.concatenate([r_enc, eff[recv], eff[send]], 1), Wrp, brp))
        agg = np.zeros((N, eff_rel.shape[1]), F32)
        np.add.at(agg, recv, eff_rel)
        eff = O._relu(O._linear(np.concatenate([p_enc, agg], 1), Wpp, bpp) + eff)
        last = ps + 1 == pstep
        yield "node_last" if last else "node", "Wb", agg
        yield ("node_last", "P0", eff) if last else ("node", "W2,W3", eff)
    h = O._relu(O._linear(eff, W["non_rigid_predictor.linear_0.weight"], W["non_rigid_predictor.linear_0.bias"]))
    yield "node_last", "P1", h


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--forwards", type=int, default=3)
    ap.add_argument("--candidates", default="0,341,682,1023")
    ap.add_argument("--order", default="slot", choices=["slot", "tool-last", "class"])
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
    picks = [int(c) for c in args.candidates.split(",")]
    a = actions[picks, :1].copy()
    a[..., 3] = args.forwards + 0.5                           # the first forwards of look-ahead step 0 are the same ones
    trace = []
    O.dynamics(W, 3, cloud, a, task, trace=trace)
    dec, _ = O.decode_action(a, task["push_length"])
    _, delta = O.tool_keypoints(dec, a[..., 2], task)
    N = N_o + 1
    attrs = np.zeros((N, 2), F32); attrs[:N_o, 0] = 1; attrs[N_o:, 1] = 1
    group = np.zeros((N, 1), F32); group[:N_o] = 1
    phys = np.zeros(N, F32); phys[:N_o] = 0.5
    tot = {}
    half = {}
    per_forward = []
    for ci, (cand, recs) in enumerate(zip(picks, trace)):
        action = np.zeros((N, 3), F32); action[N_o:] = delta[ci, 0]
        states = [recs[0]["state_last"]] * 3
        for k, rec in enumerate(recs):
            states.append(rec["state_last"])
            hist = np.stack(states[-4:], 0).astype(F32)
            n_ns = int((rec["recv"] != rec["send"]).sum())
            n_tool = int(((rec["recv"] != rec["send"]) & ((rec["recv"] >= N_o) | (rec["send"] >= N_o))).sum())
            row = {"candidate": cand, "forward": k + 1, "edges": n_ns, "tool_edges": n_tool}
            for chain, layer, act in layers_of_forward(O, W, hist, attrs, rec["recv"], rec["send"], group, action, phys, 3,
                                                        args.order, N_o):
                d = dead_share(act, 0 if chain == "edge" else cand * N)
                key = (chain, layer)
                tot[key] = tuple(x + y for x, y in zip(tot.get(key, (0, 0, 0, 0)), d))
                row[f"{chain}.{layer}"] = round(d[0] / d[2], 4)
                scopes = [("all tiles", None)]
                if chain == "edge":
                    ns_i = np.flatnonzero(rec["recv"] != rec["send"])
                    n_oo = work_list_order(rec["recv"][ns_i], rec["send"][ns_i], hist[-1], N_o, args.order)[1]
                    scopes += [("object-object tiles", lambda e0: e0 < n_oo), ("tool tiles", lambda e0: e0 >= n_oo)]
                for scope, mask in scopes:
                    h = step_shares(act, 0 if chain == "edge" else cand * N, mask)
                    hk = (chain, layer, scope)
                    half[hk] = tuple(x + y for x, y in zip(half.get(hk, (0,) * 8), h))
            per_forward.append(row)
    print(f"zero-skip census: bench batch, candidates {picks}, forwards 1..{args.forwards} of look-ahead step 0, "
          f"work list in {args.order} order")
    print(f"{'chain':10s} {'layer':6s} {'dead k-steps':>13s} {'dead chunks':>12s}   (wavefront x k-step pairs)")
    out = {"candidates": picks, "forwards": args.forwards, "order": args.order, "layers": [], "per_forward": per_forward}
    chains = {}
    for (chain, layer), (ds, dc, ns_, nc) in tot.items():
        print(f"{chain:10s} {layer:6s} {100 * ds / ns_:12.2f}% {100 * dc / nc:11.2f}%   ({ns_})")
        out["layers"].append({"chain": chain, "layer": layer, "dead_steps": ds / ns_, "dead_chunks": dc / nc, "pairs": ns_})
        c = chains.setdefault(chain, [0, 0])
        w = 2 if layer == "W2,W3" else 1                      # one mask, two layers
        c[0] += w * ds; c[1] += w * ns_
    for chain, (ds, ns_) in chains.items():
        print(f"{chain:10s} all    {100 * ds / ns_:12.2f}%")
        out[f"{chain}_dead_steps"] = ds / ns_
    for row in per_forward:
        print(json.dumps(row))
    print("half-step census: share of (wavefront, k-step) pairs, and mean MFMA issue cycles per k-step "
          f"(dead 0, half-dead {CYC_FULL} today / {CYC_HALF} as a half-step, live {CYC_FULL})")
    print(f"{'chain':10s} {'layer':6s} {'tiles':20s} {'dead':>7s} {'half':>7s} {'live':>7s} {'cyc now':>8s} {'cyc half':>9s} "
          f"{'now, barriers':>14s} {'half, barriers':>15s}")
    out["half_step"] = []
    for (chain, layer, scope), (de, ha, li, n, c0, c1, b0, b1) in half.items():
        if n == 0:
            continue
        print(f"{chain:10s} {layer:6s} {scope:20s} {100 * de / n:6.2f}% {100 * ha / n:6.2f}% {100 * li / n:6.2f}% {c0 / n:8.1f} {c1 / n:9.1f} "
              f"{b0 / n:14.1f} {b1 / n:15.1f}")
        out["half_step"].append({"chain": chain, "layer": layer, "tiles": scope, "dead": de / n, "half": ha / n, "live": li / n,
                                 "pairs": n, "cycles_now": c0 / n, "cycles_half_step": c1 / n, "cycles_now_barriers": b0 / n,
                                 "cycles_half_step_barriers": b1 / n})
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
