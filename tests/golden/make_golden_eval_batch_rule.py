#!/usr/bin/env python3
"""Generate the BATCHED EVAL-ROLLOUT fixture of a RULE config from the real reference (jhyau/AdaptiGraph): its own construct_graph
and rollout_from_start_graph, driven exactly as make_golden_eval_batch.py drives them (run_rollout and its helpers are imported
from there, that file is not edited), on the reference's softbody.yaml.

Config: softbody.yaml (n_his 5, store_rest_state, pstep 4, connect_tool_all_non_fixed, knn_range [0.4, 1.0], min_knn 0.4,
knn_increment 0.1, connect_tool_surface off) with max_nobj 24, topk 5, fps radius range [0.125, 0.25], adj range [0.375, 0.625].
3 ragged episodes of 37 / 50 / 64 points with a y extent (the rule's threshold is the bottom 10 % of the y range), 2 tool points,
14 frames, short pairs; the 4 start pairs of make_golden_eval_batch.py (schedules of 6, 3, 2 and 8 predictions).  max_nR is searched
downwards from the densest rebuilt graph until, among the graphs a free run REBUILDS, at least one backs off by kNN only, one by kNN
and then top-k, and one fits at once.

Margins, each >= 1e-4 = ten times the position bar of the GPU test, over every builder call of every step (seeds are tried until
all hold): radius and top-k as in make_golden_eval_batch.py; |y - thr| of every valid particle (thr = (max_y - min_y) * 0.1 + min_y
on the float32 scalars the reference passed); the gap between the keepK-th and the (keepK+1)-th pair distance of the flat kNN
filter (receiver above thr, tool sender; keepK = int(kNN * #pairs)).  A prediction within the bar moves y and thr by at most
1e-5 each and a distance by at most 2 sqrt(3) 1e-5, so none of these decisions can flip.

Usage:  python tests/golden/make_golden_eval_batch_rule.py      (rewrites eval_batch_softbody.npz; a second run reproduces it bit
for bit, which the script checks itself)
"""
import copy
import json
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_dataset as MD  # noqa: E402
import make_golden_eval_batch as EB  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
import train_restate as TR  # noqa: E402

NAME = "eval_batch_softbody"
MARGIN = EB.MARGIN
ADJ, KNN_MID = 0.5, 0.7


def episodes(rng):
    eps = []
    for n, scale in ((37, 0.7), (50, 1.0), (64, 1.4)):
        base = MD.rope_base(n, rng) * [scale, 1.0, scale]
        base[:, 1] += rng.uniform(0.0, 0.3, n)
        tools = base[n // 2][None] + np.array([[0.05, 0.03, 0.12], [-0.08, 0.03, 0.15]])
        tools[:, 1] = 0.36
        obj, eef = MD.episode(base, tools, EB.T_FRAMES, rng, drift=0.01, jitter=0.004, tool_step=0.02)
        eps.append((obj, eef, [rng.uniform(0.2, 0.8)]))
    return eps


def rule_margins(cloud, mask, tool, max_y, min_y, kNN):
    """(smallest |y - thr| of a valid particle, gap around the kNN filter's cut) of one builder call, in distance units."""
    thr = (max_y - min_y) * 0.1 + min_y
    assert isinstance(thr, np.float32)
    y = cloud[:, 1].astype(np.float64)
    m_y = np.abs(y[mask] - float(thr)).min()
    S = mask & (cloud[:, 1] > thr)
    gap = np.inf
    if 0.0 < kNN < 1.0 and S.any():
        p = cloud.astype(np.float64)
        d = np.sqrt(((p[S][:, None] - p[tool][None]) ** 2).sum(-1))
        d[tool[S]] = 1e5                                       # tool receivers: the reference's 1e10 squared distance
        flat = np.sort(d.reshape(-1))
        keepK = int(kNN * len(flat))
        if 0 < keepK < len(flat):
            gap = flat[keepK] - flat[keepK - 1]
    return m_y, gap


def kinds_of(runs, topk):
    out = []
    for r in runs:
        for b in r["builds"][1:]:
            out.append("fits" if len(b) == 1 else "topk" if b[-1][2] < topk else "knn")
    return out


def generate(mods):
    G, RG, RR = mods
    with open(f"{MG.REF}/config/dynamics/softbody.yaml") as f:
        dyn = copy.deepcopy(yaml.safe_load(f))
    dcfg, mcfg = dyn["dataset_config"], dyn["material_config"]
    assert dcfg["n_his"] == 5 and dcfg["store_rest_state"] and dcfg["n_future"] == 3 and dyn["model_config"]["pstep"] == 4
    dcfg["datasets"][0].update(max_nobj=EB.MAX_NOBJ, topk=EB.TOPK, fps_radius_range=[0.125, 0.25], adj_radius_range=[0.375, 0.625],
                               connect_tool_all=False, connect_tool_surface=False, connect_tool_surface_ratio=1.0,
                               connect_tool_all_non_fixed=True, knn_range=[0.4, 1.0], min_knn=0.4, knn_increment=0.1, max_nR=10000)
    DynamicsPredictor = MG.import_reference()[0]
    pairs_all = [r for ep in range(3) for r in EB.pair_rows(ep)]
    calls = []
    real = RG.construct_edges_from_states

    def logging_builder(states, *a, **k):
        calls.append((k.get("max_y"), k.get("min_y"), float(k.get("kNN", 1.0))))
        return real(states, *a, **k)

    RG.construct_edges_from_states = RR.construct_edges_from_states = logging_builder     # run_rollout wraps whatever is installed
    try:
        for attempt in range(80):
            seed = 41 + 100 * attempt
            rng = np.random.default_rng(seed)
            eps = episodes(rng)
            model = MG.make_model(DynamicsPredictor, dyn, seed)
            model.load_state_dict({k: torch.from_numpy(v) for k, v in TR.make_weights(seed, n_his=5).items()})

            def run_all(max_nR):
                dcfg["datasets"][0]["max_nR"] = int(max_nR)
                np.random.seed(seed)
                runs, logs = [], []
                for st in EB.STARTS:
                    del calls[:]
                    runs.append(EB.run_rollout(mods, model, dcfg, mcfg, eps, pairs_all, st))
                    logs.append(list(calls))
                return runs, logs
            free, _ = run_all(10000)
            if [r["L"] for r in free] != [6, 3, 2, 8]:
                raise SystemExit(f"{NAME}: schedule lengths {[r['L'] for r in free]}")
            top = max(b[0][3] for r in free for b in r["builds"][1:])
            found = None
            for max_nR in range(top - 1, int(0.6 * top), -1):
                try:
                    runs, logs = run_all(max_nR)
                except Exception as e:                          # (a top-k that reaches zero: pad_torch's 'Exceeds max dims')
                    print(f"{NAME}: seed {seed} max_nR {max_nR}: {e}")
                    break
                ks = kinds_of(runs, EB.TOPK)
                if min(b[-1][2] for r in runs for b in r["builds"]) >= 1 and {"fits", "knn", "topk"} <= set(ks):
                    found = (max_nR, runs, logs)
                    break
            if found is None:
                print(f"{NAME}: seed {seed}: no max_nR with all three kinds among the rebuilt graphs")
                continue
            max_nR, runs, logs = found
            n_obj = [len(r["fps_idx"]) for r in runs]
            if len(set(n_obj)) < 3 or min(n_obj) >= EB.MAX_NOBJ:
                print(f"{NAME}: seed {seed}: n_obj {n_obj}: not ragged")
                continue
            m = dict(radius=np.inf, topk=np.inf, y=np.inf, knn=np.inf)
            for r, log in zip(runs, logs):
                flat = [a for b in r["builds"] for a in b]
                assert len(flat) == len(log)
                for (cloud, kNN, k, _), (max_y, min_y, kNN_l) in zip(flat, log):
                    assert kNN == kNN_l and isinstance(max_y, np.float32) and isinstance(min_y, np.float32)
                    a, g = EB.margins(cloud, ADJ, r["state_mask"], r["eef_mask"], k)
                    y, c = rule_margins(cloud, r["state_mask"], r["eef_mask"], max_y, min_y, kNN)
                    m = dict(radius=min(m["radius"], a), topk=min(m["topk"], g), y=min(m["y"], y), knn=min(m["knn"], c))
            if min(m.values()) < MARGIN:
                print(f"{NAME}: seed {seed} max_nR {max_nR}: margins " + ", ".join(f"{k} {v:.2e}" for k, v in m.items()) + f": below {MARGIN}")
                continue
            break
        else:
            raise SystemExit(f"{NAME}: no seed met the conditions")
    finally:
        RG.construct_edges_from_states = RR.construct_edges_from_states = real
    T = EB.T_FRAMES
    meta = dict(reference="construct_graph and rollout_from_start_graph called directly (viz=False), as make_golden_eval_batch.py does",
                fps_stage1="tests/dataset_restate.py:fps_stage1 in place of dgl", seed=int(seed), max_nR=int(max_nR), pstep=4,
                kinds=kinds_of(runs, EB.TOPK))
    store = {"dataset_config_json": np.frombuffer(json.dumps(dcfg).encode(), np.uint8),
             "material_config_json": np.frombuffer(json.dumps(mcfg).encode(), np.uint8),
             "meta_json": np.frombuffer(json.dumps(meta).encode(), np.uint8),
             "pair_lists": np.asarray(pairs_all, np.int64), "n_episodes": np.int64(3), "w_seed": np.int64(seed),
             "samples": np.array([pairs_all.index([ep, t - 3, t - 2, t - 1, t, t + d, min(t + 2 * d, T - 1), min(t + 3 * d, T - 1)])
                                  for ep, t, d in EB.STARTS], np.int64),
             "margin_radius": np.float64(m["radius"]), "margin_topk": np.float64(m["topk"]), "margin_y": np.float64(m["y"]),
             "margin_knn": np.float64(m["knn"])}
    for e, (o, f, p) in enumerate(eps):
        store[f"ep{e}::obj"], store[f"ep{e}::eef"], store[f"ep{e}::phys"] = o, f, np.asarray(p, np.float32)
    store["draw::fps_start"] = np.array([r["fps_start"] for r in runs], np.int32)
    store["draw::rad_start"] = np.array([r["rad_start"] for r in runs], np.int32)
    fps = np.full((len(runs), EB.MAX_NOBJ), -1, np.int32)
    for j, r in enumerate(runs):
        fps[j, :len(r["fps_idx"])] = r["fps_idx"]
    store["fps_idx"], store["n_obj"] = fps, np.array([len(r["fps_idx"]) for r in runs], np.int32)
    gap = 0.0
    for j, r in enumerate(runs):
        pre = f"r{j}::"
        for k in ("idx_list", "error_list", "error64", "pred", "state", "action"):
            store[pre + k] = r[k]
        MG.pack_edges(pre, r["edges"], store)
        store[pre + "cloud"] = np.stack([b[0][0] for b in r["builds"][1:]]) if r["L"] > 1 else np.zeros((0, EB.MAX_NOBJ + 2, 3), np.float32)
        store[pre + "trail"] = np.array([len(b) for b in r["builds"]], np.int32)
        store[pre + "trail::rows"] = np.array([[a[1], a[2], a[3]] for b in r["builds"] for a in b], np.float64).reshape(-1, 3)
        gap = max(gap, float(np.abs(r["error_list"].astype(np.float64) - r["error64"]).max()))
    store["ref_gap"] = np.float64(gap)
    print(f"{NAME}: seed {seed} max_nR {max_nR} n_obj {store['n_obj'].tolist()} L {[r['L'] for r in runs]} "
          f"attempts {[[len(b) for b in r['builds']] for r in runs]} kinds {meta['kinds']} margins "
          + ", ".join(f"{k} {v:.2e}" for k, v in m.items()) + f" ref_gap {gap:.2e}")
    return store


def main():
    torch.set_num_threads(8)
    mods = EB.import_rollout()
    path = os.path.join(HERE, NAME + ".npz")
    first = generate(mods)
    np.savez_compressed(path, **first)
    again = generate(mods)
    assert sorted(first) == sorted(again) and all(np.array_equal(first[k], again[k]) for k in first), "a second run differs"
    size = os.path.getsize(path)
    assert size < 2_000_000
    print(f"{NAME}: second run identical -> {size / 1e3:.0f} KB")


if __name__ == "__main__":
    main()
