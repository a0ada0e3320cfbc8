#!/usr/bin/env python3
"""Generate the BATCHED EVAL-ROLLOUT fixtures from the real reference (jhyau/AdaptiGraph): its own construct_graph and
rollout_from_start_graph on synthetic episodes.

Runs only where the reference checkout exists (the import recipe of make_golden.py, the farthest-point stand-in of
make_golden_dataset.py: dgl is not installed, stage 1 is tests/dataset_restate.py:fps_stage1); the tests see only the .npz files.
What is driven (reference file:line):
  * construct_graph                              src/dynamics/rollout/graph.py:342-650   (start graph, its own back-off)
  * rollout_from_start_graph                     src/dynamics/rollout/rollout.py:21-270  (viz=False, no images)
  * get_next_pair_or_break_episode_pushes        src/dynamics/rollout/graph.py:672-687
Both are CALLED, not restated.  rollout_from_start_graph keeps idx_list to itself, so the pair function handed to it is a wrapper
that records what the reference's own function returns; idx_list is the start pair plus those, by rollout.py:154-160.  The
model's forward and construct_edges_from_states (in both modules) are wrapped to record, per step: the model input, the
prediction, the cloud the builder was fed, every attempt's (kNN, topk, n_rel).  np.random.randint is wrapped to record the two
farthest-point start indices.  natsort / h5py / cv2 / moviepy are absent and only used by the visualisation: empty stand-ins.

Config: the reference's rope.yaml with max_nobj 24, topk 5, fps radius range [0.125, 0.25], adj range [0.375, 0.625] (midpoints exact
in fp32), connect_tool_all false, connect_tool_all_non_fixed false, knn_range [1, 1]; eval_batch_rope: n_his 4, no rest frame;
eval_batch_rest: n_his 5, store_rest_state, short pairs.  3 episodes of 37 / 50 / 64 points, 2 tool points, 14 frames; 4 start
pairs with schedules of 6, 3, 2 and 8 predictions.  max_nR is the largest first-attempt edge count among the graphs a free run
REBUILDS, minus one: at least one graph backs off inside the loop (a denser start graph does too) and the others fit.

Margins: over every builder call of every step, the smallest |distance - radius| of an unmasked pair and the smallest gap
between the k-th and (k+1)-th neighbour distance inside the radius (k = the attempt's top-k), in distance units.  Seeds are tried
until both are >= 1e-4, ten times the position bar of the GPU test: a prediction within the bar moves a distance by at most
2 sqrt(3) 1e-5 and a gap by twice that, so it cannot flip an edge.

Usage:  python tests/golden/make_golden_eval_batch.py          (rewrites both files; a second run reproduces them bit for bit)
"""
import copy
import json
import os
import sys
import types

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_dataset as MD  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
import train_restate as TR  # noqa: E402

OUT = HERE
MARGIN = 1e-4
MAX_NOBJ, TOPK, T_FRAMES = 24, 5, 14
STARTS = [(0, 3, 1), (0, 9, 1), (1, 10, 2), (2, 5, 1)]          # (episode, start frame, stride of the start pair)
STRIDES = {0: (1, 2, 3), 1: (1, 2), 2: (1,)}


def import_rollout():
    D, G = MD.import_dataset()
    for name in ("natsort", "h5py"):
        sys.modules.setdefault(name, types.ModuleType(name))
    import dynamics.rollout.graph as RG
    import dynamics.rollout.rollout as RR
    return G, RG, RR


def pair_rows(ep):
    rows = []
    for t in range(3, T_FRAMES - 1):
        for d in STRIDES[ep]:
            if t + d <= T_FRAMES - 1:
                rows.append([ep, t - 3, t - 2, t - 1, t, t + d, min(t + 2 * d, T_FRAMES - 1), min(t + 3 * d, T_FRAMES - 1)])
    return rows


def episodes(rng):
    eps = []
    for n, scale in ((37, 0.7), (50, 1.0), (64, 1.4)):
        base = MD.rope_base(n, rng) * [scale, 1.0, scale]
        tools = base[n // 2][None] + np.array([[0.05, 0.03, 0.12], [-0.08, 0.03, 0.15]])
        obj, eef = MD.episode(base, tools, T_FRAMES, rng, drift=0.01, jitter=0.004, tool_step=0.02)
        eps.append((obj, eef, [rng.uniform(0.2, 0.8)]))
    return eps


def margins(cloud, adj, mask, tool, k):
    """(radius margin, top-k gap) of one builder call, in distance units."""
    p = cloud.astype(np.float64)
    d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
    dead = ~(mask[:, None] & mask[None, :]) | (tool[:, None] & tool[None, :])
    rad = np.abs(np.where(dead, np.inf, d) - adj).min()
    s = np.sort(np.where(dead, np.inf, d), axis=1)
    gap = np.inf
    if k < len(p):
        both = s[:, k] < adj
        if both.any():
            gap = (s[both, k] - s[both, k - 1]).min()
    return rad, gap


class Tape:
    """Everything one rollout records, in call order."""

    def __init__(self):
        self.model_in, self.pred, self.builds, self.pairs, self.randint = [], [], [], [], []


def run_rollout(mods, model, dcfg, mcfg, eps, pairs_all, start):
    G, RG, RR = mods
    ep, t0, d0 = start
    obj, eef, phys = eps[ep]
    n_his, rest = dcfg["n_his"], dcfg["store_rest_state"]
    rows = np.array([r[1:] for r in pairs_all if r[0] == ep])
    pair = np.array([t0 - 3, t0 - 2, t0 - 1, t0, t0 + d0, min(t0 + 2 * d0, T_FRAMES - 1), min(t0 + 3 * d0, T_FRAMES - 1)])
    assert any((r == pair).all() for r in rows)
    tape = Tape()
    orig_fwd, orig_ri = model.forward, np.random.randint
    orig_b = {m: m.construct_edges_from_states for m in (RG, RR)}

    def fwd(**g):
        tape.model_in.append({k: g[k].clone() for k in ("state", "action", "Rr", "Rs")})
        tape.builds.append([])                                  # builder calls from here on belong to the NEXT graph
        out = orig_fwd(**g)
        tape.pred.append(out[0].detach().clone())
        return out

    def builder(states, *a, **k):
        Rr, Rs = orig_b[RG](states, *a, **k)
        topk = k["topk"] if "topk" in k else a[3]
        if not tape.builds:
            tape.builds.append([])                              # the start graph's attempts
        tape.builds[-1].append((states.numpy().copy(), float(k.get("kNN", 1.0)), int(topk), int(Rr.shape[0])))
        return Rr, Rs

    def randint(*a, **k):
        v = orig_ri(*a, **k)
        tape.randint.append(int(v))
        return v

    def next_pair(*a, **k):
        p = RG.get_next_pair_or_break_episode_pushes(*a, **k)
        tape.pairs.append(None if p is None else np.array(p))
        return p

    model.forward = fwd
    RG.construct_edges_from_states = RR.construct_edges_from_states = builder
    np.random.randint = randint
    try:
        graph, fps_idx, _ = MG.quiet(RG.construct_graph, dcfg, mcfg, eef, obj, n_his, pair, {dcfg["materials"][0]: np.asarray(phys, np.float32)},
                                     store_rest_state=rest)
        start_builds = tape.builds.pop() if tape.builds else []
        assert len(tape.randint) == 2, tape.randint
        s, e = (pair[n_his - 2], pair[n_his - 1]) if rest else (pair[n_his - 1], pair[n_his])          # rollout.py:300-305
        errors = MG.quiet(RR.rollout_from_start_graph, graph, fps_idx, dcfg, mcfg, model, torch.device("cpu"), eef, obj, int(s), int(e),
                          next_pair, rows, None, False, None, None, None, None, False)
    finally:
        del model.forward
        RG.construct_edges_from_states, RR.construct_edges_from_states = orig_b[RG], orig_b[RR]
        np.random.randint = orig_ri
    idx_list = [[int(s), int(e)]]
    c = n_his - 1 if rest else n_his                            # rollout.py:154-159 on the short pairs
    for p in tape.pairs:
        if p is not None:
            idx_list.append([int(p[c - 1]), int(p[c])])
    L = len(tape.pred)
    assert len(errors) == L and len(idx_list) == L, (len(errors), len(idx_list), L)
    builds = [start_builds] + tape.builds[:L - 1]
    assert all(len(b) >= 1 for b in builds) and len(tape.builds[L - 1]) == 0
    fps_idx = np.asarray(fps_idx, np.int64)
    obj_mask = graph["obj_mask"].numpy()
    err64 = []
    for i in range(L):
        gt = np.zeros((MAX_NOBJ, 3), np.float32)
        gt[:len(fps_idx)] = obj[idx_list[i][1]][fps_idx]
        p = tape.pred[i][0].numpy()
        err64.append(np.sqrt(((p[obj_mask].astype(np.float64) - gt[obj_mask].astype(np.float64)) ** 2).sum(-1)).mean())
    return dict(L=L, idx_list=np.array(idx_list, np.int64), error_list=np.array(errors, np.float32), error64=np.array(err64, np.float64),
                pred=np.stack([p[0].numpy() for p in tape.pred]), state=np.stack([m["state"][0].numpy() for m in tape.model_in]),
                action=np.stack([m["action"][0].numpy() for m in tape.model_in]),
                edges=[MG.edges_from_R(m["Rr"], m["Rs"])[0] for m in tape.model_in], builds=builds, fps_idx=fps_idx,
                fps_start=tape.randint[0], rad_start=tape.randint[1], state_mask=graph["state_mask"].numpy(), eef_mask=graph["eef_mask"].numpy())


def gen_case(name, mods, n_his, rest, seed0):
    with open(f"{MG.REF}/config/dynamics/rope.yaml") as f:
        dyn = yaml.safe_load(f)
    dyn = copy.deepcopy(dyn)
    dcfg, mcfg = dyn["dataset_config"], dyn["material_config"]
    dcfg["n_his"], dcfg["store_rest_state"] = n_his, rest
    dcfg["datasets"][0].update(max_nobj=MAX_NOBJ, topk=TOPK, fps_radius_range=[0.125, 0.25], adj_radius_range=[0.375, 0.625],
                               connect_tool_all=False, connect_tool_all_non_fixed=False, knn_range=[1.0, 1.0], max_nR=10000)
    assert dcfg["n_future"] == 3
    adj = 0.5
    DynamicsPredictor = MG.import_reference()[0]
    pairs_all = [r for ep in range(3) for r in pair_rows(ep)]
    for attempt in range(60):
        seed = seed0 + 100 * attempt
        rng = np.random.default_rng(seed)
        eps = episodes(rng)
        model = MG.make_model(DynamicsPredictor, dyn, seed)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in TR.make_weights(seed, n_his=n_his).items()})

        def run_all(max_nR):
            dcfg["datasets"][0]["max_nR"] = int(max_nR)
            np.random.seed(seed)
            return [run_rollout(mods, model, dcfg, mcfg, eps, pairs_all, st) for st in STARTS]
        free = run_all(10000)
        if [r["L"] for r in free] != [6, 3, 2, 8]:
            raise SystemExit(f"{name}: schedule lengths {[r['L'] for r in free]}")
        max_nR = max(b[0][3] for r in free for b in r["builds"][1:]) - 1          # the densest REBUILT graph backs off
        try:
            runs = run_all(max_nR)
        except Exception as e:                                  # (a top-k that reaches zero loops in the reference: guarded by the assert below)
            print(f"{name}: seed {seed}: {e}")
            continue
        n_obj = [len(r["fps_idx"]) for r in runs]
        backed = sum(len(b) > 1 for r in runs for b in r["builds"][1:])
        fits = sum(len(b) == 1 for r in runs for b in r["builds"])
        if min(b[-1][2] for r in runs for b in r["builds"]) < 1 or backed < 1 or fits < 1 or len(set(n_obj)) < 3 or min(n_obj) >= MAX_NOBJ:
            print(f"{name}: seed {seed}: n_obj {n_obj}, backed off {backed}, fit {fits}: conditions not met")
            continue
        m_rad, m_gap = np.inf, np.inf
        for r in runs:
            for b in r["builds"]:
                for cloud, _, k, _ in b:
                    a, g = margins(cloud, adj, r["state_mask"], r["eef_mask"], k)
                    m_rad, m_gap = min(m_rad, a), min(m_gap, g)
        if min(m_rad, m_gap) < MARGIN:
            print(f"{name}: seed {seed}: margins radius {m_rad:.2e}, top-k {m_gap:.2e}: below {MARGIN}")
            continue
        break
    else:
        raise SystemExit(f"{name}: no seed met the conditions")
    material = dcfg["materials"][0]
    meta = dict(reference="construct_graph and rollout_from_start_graph called directly (viz=False); idx_list rebuilt from the pairs "
                          "the reference's get_next_pair_or_break_episode_pushes returned to it, by rollout.py:154-160",
                fps_stage1="tests/dataset_restate.py:fps_stage1 in place of dgl", seed=int(seed), max_nR=int(max_nR))
    store = {"dataset_config_json": np.frombuffer(json.dumps(dcfg).encode(), np.uint8),
             "material_config_json": np.frombuffer(json.dumps(mcfg).encode(), np.uint8),
             "meta_json": np.frombuffer(json.dumps(meta).encode(), np.uint8),
             "pair_lists": np.asarray(pairs_all, np.int64), "n_episodes": np.int64(3), "w_seed": np.int64(seed),
             "samples": np.array([pairs_all.index([ep, t - 3, t - 2, t - 1, t, t + d, min(t + 2 * d, T_FRAMES - 1), min(t + 3 * d, T_FRAMES - 1)])
                                  for ep, t, d in STARTS], np.int64),
             "margin_radius": np.float64(m_rad), "margin_topk": np.float64(m_gap)}
    for e, (o, f, p) in enumerate(eps):
        store[f"ep{e}::obj"], store[f"ep{e}::eef"], store[f"ep{e}::phys"] = o, f, np.asarray(p, np.float32)
    store["draw::fps_start"] = np.array([r["fps_start"] for r in runs], np.int32)
    store["draw::rad_start"] = np.array([r["rad_start"] for r in runs], np.int32)
    fps = np.full((len(runs), MAX_NOBJ), -1, np.int32)
    for j, r in enumerate(runs):
        fps[j, :len(r["fps_idx"])] = r["fps_idx"]
    store["fps_idx"], store["n_obj"] = fps, np.array([len(r["fps_idx"]) for r in runs], np.int32)
    gap = 0.0
    for j, r in enumerate(runs):
        pre = f"r{j}::"
        for k in ("idx_list", "error_list", "error64", "pred", "state", "action"):
            store[pre + k] = r[k]
        MG.pack_edges(pre, r["edges"], store)
        store[pre + "cloud"] = np.stack([b[0][0] for b in r["builds"][1:]]) if r["L"] > 1 else np.zeros((0, MAX_NOBJ + 2, 3), np.float32)
        store[pre + "trail"] = np.array([len(b) for b in r["builds"]], np.int32)
        store[pre + "trail::rows"] = np.array([[a[1], a[2], a[3]] for b in r["builds"] for a in b], np.float64).reshape(-1, 3)
        gap = max(gap, float(np.abs(r["error_list"].astype(np.float64) - r["error64"]).max()))
    store["ref_gap"] = np.float64(gap)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **store)
    print(f"{name}: seed {seed} max_nR {max_nR} n_obj {store['n_obj'].tolist()} L {[r['L'] for r in runs]} "
          f"attempts {[[len(b) for b in r['builds']] for r in runs]} margins {m_rad:.2e} {m_gap:.2e} ref_gap {gap:.2e} "
          f"-> {os.path.getsize(path) / 1e3:.0f} KB")
    return store


def main():
    torch.set_num_threads(8)
    mods = import_rollout()
    gen_case("eval_batch_rope", mods, 4, False, seed0=31)
    gen_case("eval_batch_rest", mods, 5, True, seed0=32)


if __name__ == "__main__":
    main()
