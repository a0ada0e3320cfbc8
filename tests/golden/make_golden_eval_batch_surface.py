#!/usr/bin/env python3
"""Generate the BATCHED EVAL-ROLLOUT fixture of a SURFACE config from the real reference (jhyau/AdaptiGraph): its own
construct_graph and rollout_from_start_graph, driven exactly as make_golden_eval_batch.py drives them (run_rollout and its helpers
are imported from there, that file is not edited), on the reference's softbody.yaml with connect_tool_surface switched on.

Config: softbody.yaml (n_his 5, store_rest_state, pstep 4, connect_tool_all_non_fixed, knn_range [0.4, 1.0], min_knn 0.4,
knn_increment 0.1) with connect_tool_surface True at connect_tool_surface_ratio 0.8 - so both tool rules chain -, max_nobj 24,
topk 5, fps radius range [0.125, 0.25], adj range [0.375, 0.625].  3 ragged episodes of 37 / 50 / 64 points in boxes of three
different sizes away from the origin (the planes are RATIOS of the extreme coordinates, so a corner beyond two planes holds
particles), 2 tool points low beside the +x +z corner, 14 frames, short pairs; the tool of episode 0 starts out of reach and
closes in, the others touch throughout.  The 4 start pairs of make_golden_eval_batch.py (schedules of 6, 3, 2 and 8 predictions).
max_nR is searched downwards from the densest rebuilt graph.

Conditions the script asserts (seeds are tried until all hold):
  1. the surface rule fires (check > 0) on at least one start graph and at least one rebuilt graph;
  2. on at least one of each kind its subset S holds a non-tool particle and the rule both adds and removes an edge;
  3. at least one builder call has check == 0 (the graph is copied through);
  4. among the rebuilt graphs at least one fits at once and one backs off to a lower top-k;
  5. at least one start graph's bounds differ between the two bound orders (construct_graph forms min_x / min_z from the unscaled
     maxima, the step loop from the scaled ones);
  6. the numpy restatement of the batched rule (tests/surface_restate.py) reproduces every recorded edge list, every chosen plane
     pair and all six bounds of every builder call.
Margins, each >= 1e-4 = ten times the position bar of the GPU test, over every builder call of every step: radius, top-k,
y threshold and kNN cut as in make_golden_eval_batch_rule.py; |coordinate - bound| of every valid particle for each of the two
chosen planes.  Plane ranking: only the SET of the two smallest values matters, so the margin is between the 2nd and the 3rd
smallest: with every (p - bound) difference moved by +-1e-4 the 2nd's upper value stays below the 3rd's lower value (a prediction
within the 1e-5 bar cannot swap them), and their relative gap is >= 1e-3 (the reference sums at most 52 * 26 fp32 terms with
torch.sum, worst case 1352 * 2^-24 ~ 8e-5, where the restatement and the kernel use the closed fp64 form).

Usage:  python tests/golden/make_golden_eval_batch_surface.py      (rewrites eval_batch_surface.npz; a second run reproduces it
bit for bit, which the script checks itself)
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
import make_golden_eval_batch_rule as EBR  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import surface_restate as SR  # noqa: E402
import train_restate as TR  # noqa: E402

NAME = "eval_batch_surface"
MARGIN = EB.MARGIN
ADJ, KNN_MID, RATIO = 0.5, 0.7, 0.8
F32 = np.float32
BOUND_KEYS = SR.BOUND_KEYS


def episodes(rng):
    """Boxes of three sizes with their low corner at (0.9, 0, 0.9), a third of the points in a layer on the floor (a body at
    rest on a table).  At ratio 0.8 the max_x / max_z planes cut through the upper part of each box, so a corner between an x and a
    z plane runs through the whole height and holds FIXED particles (the bottom 10 % of the non-fixed rule): only those keep an
    edge TO a tool behind the non-fixed rule, which this rule then removes, and only those lack the tool as a sender, which it
    adds.  The tool sits low beside the +x +z corner; in episode 0 it starts out of reach and closes in, the others touch
    throughout."""
    eps = []
    for e, (n, size) in enumerate(((37, 0.45), (50, 0.6), (64, 0.8))):
        u = rng.uniform(0, 1, (n, 3))
        u[:, 1] = np.where(rng.uniform(0, 1, n) < 0.35, rng.uniform(0, 0.04, n), u[:, 1])
        base = np.array([0.9, 0.0, 0.9]) + u * [size, 0.6 * size, size]
        corner = np.array([base[:, 0].max(), base[:, 1].min(), base[:, 2].max()])
        gap0, closer = ((0.50, 0.03) if e == 0 else (0.12, 0.0))
        tools = corner[None] + np.array([[gap0, 0.02, gap0 - 0.05], [gap0 - 0.06, 0.10, gap0 + 0.03]])
        T = EB.T_FRAMES
        v = rng.normal(0, 0.008, (1, 3))
        obj = np.stack([base + v * t + rng.normal(0, 0.004, base.shape) for t in range(T)]).astype(F32)
        step = np.array([-closer, 0.004, -closer]) if e == 0 else np.array([-0.010, 0.004, -0.006])
        eef = np.stack([tools + step * t + rng.normal(0, 0.003, tools.shape) for t in range(T)]).astype(F32)
        eps.append((obj, eef, [rng.uniform(0.2, 0.8)]))
    return eps


def plane_margins(cloud, mask, bd, planes):
    """The smallest |coordinate - bound| of a valid particle over the two chosen planes."""
    axis = dict(max_y=1, min_x=0, max_x=0, min_z=2, max_z=2)
    p = cloud.astype(np.float64)
    side = min(np.abs(p[mask][:, axis[SR.PLANES[k]]] - float(bd[SR.PLANES[k]])).min() for k in planes)
    return side


def ranking_margin(cloud, n0, n1, bd):
    """(lower value of the 3rd smallest plane value minus upper value of the 2nd with every |p - bound| moved by 1e-4, their relative
    gap), the values from the closed form in fp64."""
    p = cloud.astype(np.float64)
    N = len(p)
    lo, hi, mid = [], [], []
    for name in SR.PLANES:
        ax = dict(max_y=1, min_x=0, max_x=0, min_z=2, max_z=2)[name]
        e0, e1 = abs(p[0, ax] - float(bd[name])), abs(p[1, ax] - float(bd[name]))
        mid.append(N * (n0 * e0 ** 2 + n1 * e1 ** 2))
        hi.append(N * (n0 * (e0 + MARGIN) ** 2 + n1 * (e1 + MARGIN) ** 2))
        lo.append(N * (n0 * max(e0 - MARGIN, 0.0) ** 2 + n1 * max(e1 - MARGIN, 0.0) ** 2))
    order = np.argsort(mid)
    second, third = order[1], order[2]
    return lo[third] - hi[second], (mid[third] - mid[second]) / mid[third]


def generate(mods):
    G, RG, RR = mods
    with open(f"{MG.REF}/config/dynamics/softbody.yaml") as f:
        dyn = copy.deepcopy(yaml.safe_load(f))
    dcfg, mcfg = dyn["dataset_config"], dyn["material_config"]
    assert dcfg["n_his"] == 5 and dcfg["store_rest_state"] and dcfg["n_future"] == 3 and dyn["model_config"]["pstep"] == 4
    dcfg["datasets"][0].update(max_nobj=EB.MAX_NOBJ, topk=EB.TOPK, fps_radius_range=[0.125, 0.25], adj_radius_range=[0.375, 0.625],
                               connect_tool_all=False, connect_tool_surface=True, connect_tool_surface_ratio=RATIO,
                               connect_tool_all_non_fixed=True, knn_range=[0.4, 1.0], min_knn=0.4, knn_increment=0.1, max_nR=10000)
    DynamicsPredictor = MG.import_reference()[0]
    pairs_all = [r for ep in range(3) for r in EB.pair_rows(ep)]
    calls = []
    real, real_planes = RG.construct_edges_from_states, G.determine_closest_plane

    def logging_planes(*a):
        out = real_planes(*a)
        calls[-1]["planes"] = (SR.PLANES.index(out[0]), SR.PLANES.index(out[2]))
        return out

    def logging_builder(states, *a, **k):
        assert k["connect_tools_surface"] and k["connect_tool_all_non_fixed"]
        calls.append(dict(bd={n: k[n] for n in BOUND_KEYS}, kNN=float(k.get("kNN", 1.0)), planes=(-1, -1)))
        return MG.quiet(real, states, *a, **k)

    RG.construct_edges_from_states = RR.construct_edges_from_states = logging_builder     # run_rollout wraps whatever is installed
    G.determine_closest_plane = logging_planes
    try:
        for attempt in range(200):
            seed = 51 + 100 * attempt
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
                    logs.append([dict(c) for c in calls])
                return runs, logs
            free, _ = run_all(10000)
            if [r["L"] for r in free] != [6, 3, 2, 8]:
                raise SystemExit(f"{NAME}: schedule lengths {[r['L'] for r in free]}")
            n_obj = [len(r["fps_idx"]) for r in free]
            if len(set(n_obj)) < 3 or min(n_obj) >= EB.MAX_NOBJ:
                print(f"{NAME}: seed {seed}: n_obj {n_obj}: not ragged")
                continue
            top = max(b[0][3] for r in free for b in r["builds"][1:])
            found = None
            for max_nR in range(top - 1, int(0.6 * top), -1):
                try:
                    runs, logs = run_all(max_nR)
                except Exception as e:                          # (a top-k that reaches zero: pad_torch's 'Exceeds max dims')
                    print(f"{NAME}: seed {seed} max_nR {max_nR}: {e}")
                    break
                ks = EBR.kinds_of(runs, EB.TOPK)
                if min(b[-1][2] for r in runs for b in r["builds"]) >= 1 and {"fits", "topk"} <= set(ks):
                    found = (max_nR, runs, logs)
                    break
            if found is None:
                print(f"{NAME}: seed {seed}: no max_nR with a fitting and a top-k back-off among the rebuilt graphs")
                continue
            max_nR, runs, logs = found
            # ---- margins, conditions, and the restatement on every builder call
            m = dict(radius=np.inf, topk=np.inf, y=np.inf, knn=np.inf, side=np.inf, rank_abs=np.inf, rank_rel=np.inf)
            fired = dict(start=0, rebuilt=0)
            both = dict(start=0, rebuilt=0)
            copied = orders_differ = 0
            why = None
            for j, (r, log) in enumerate(zip(runs, logs)):
                flat = [(bi, ai, a) for bi, b in enumerate(r["builds"]) for ai, a in enumerate(b)]
                assert len(flat) == len(log)
                mask, tool = r["state_mask"], r["eef_mask"]
                ep, t0, _ = EB.STARTS[j]
                n = len(r["fps_idx"])
                for (bi, ai, (cloud, kNN, k, n_rel)), c in zip(flat, log):
                    bd = c["bd"]
                    assert kNN == c["kNN"] and all(isinstance(bd[x], np.float32) for x in BOUND_KEYS)
                    kind = "start" if bi == 0 else "rebuilt"
                    rows = eps[ep][0][t0][r["fps_idx"]] if bi == 0 else cloud[:n]           # frame n_his - 1 of the start pair
                    order, pad = (1, EB.MAX_NOBJ) if bi == 0 else (0, 0)
                    got = SR.chained(cloud, ADJ, mask, tool, k, False, True, kNN, rows, pad, RATIO, order)
                    want_bd = np.array([bd[x] for x in BOUND_KEYS], F32)
                    if not np.array_equal(got["bounds"], want_bd):
                        raise SystemExit(f"{NAME}: seed {seed} run {j} build {bi}.{ai}: bounds {got['bounds']} != reference {want_bd}")
                    if bi == 0 and not np.array_equal(SR.bounds6(rows, pad, RATIO, 0), want_bd):
                        orders_differ += 1
                    if set(got["planes"]) != set(c["planes"]) or len(got["recv"]) != n_rel:
                        why = f"run {j} build {bi}.{ai}: planes {got['planes']} vs reference {c['planes']}, {len(got['recv'])} vs {n_rel} edges"
                        break
                    if ai == len(r["builds"][bi]) - 1:                                       # the graph the forward ran on
                        if not (np.array_equal(got["recv"], r["edges"][bi][0]) and np.array_equal(got["send"], r["edges"][bi][1])):
                            why = f"run {j} build {bi}: the restatement's edge list differs from the reference's"
                            break
                    a, g = EB.margins(cloud, ADJ, mask, tool, k)
                    y, cut = EBR.rule_margins(cloud, mask, tool, bd["max_y"], bd["min_y"], kNN)
                    m.update(radius=min(m["radius"], a), topk=min(m["topk"], g), y=min(m["y"], y), knn=min(m["knn"], cut))
                    if got["check"] == 0:
                        copied += 1
                        continue
                    fired[kind] += 1
                    before = set(zip(*got["mid"]))
                    after = set(zip(got["recv"].tolist(), got["send"].tolist()))
                    before = set((int(x), int(y_)) for x, y_ in before)
                    if (got["S"] & ~tool).any() and (after - before) and (before - after):
                        both[kind] += 1
                    n1 = got["check"]
                    n0 = int(mask.sum()) * int(tool.sum()) - n1
                    ra, rr = ranking_margin(cloud, n0, n1, bd)
                    m.update(side=min(m["side"], plane_margins(cloud, mask, bd, got["planes"])), rank_abs=min(m["rank_abs"], ra),
                             rank_rel=min(m["rank_rel"], rr))
                if why:
                    break
            if why:
                raise SystemExit(f"{NAME}: seed {seed}: {why}")
            cond = dict(fired=fired, adds_and_removes=both, copied=copied, orders_differ=orders_differ)
            if min(fired.values()) < 1 or min(both.values()) < 1 or copied < 1 or orders_differ < 1:
                print(f"{NAME}: seed {seed} max_nR {max_nR}: conditions not met: {cond}")
                continue
            small = {k: v for k, v in m.items() if v < (1e-3 if k == "rank_rel" else 0.0 if k == "rank_abs" else MARGIN)}
            if small or m["rank_abs"] <= 0:
                print(f"{NAME}: seed {seed} max_nR {max_nR}: margins " + ", ".join(f"{k} {v:.2e}" for k, v in m.items()) + ": too small")
                continue
            break
        else:
            raise SystemExit(f"{NAME}: no seed met the conditions")
    finally:
        RG.construct_edges_from_states = RR.construct_edges_from_states = real
        G.determine_closest_plane = real_planes
    T = EB.T_FRAMES
    meta = dict(reference="construct_graph and rollout_from_start_graph called directly (viz=False), as make_golden_eval_batch.py does",
                fps_stage1="tests/dataset_restate.py:fps_stage1 in place of dgl", seed=int(seed), max_nR=int(max_nR), pstep=4,
                kinds=EBR.kinds_of(runs, EB.TOPK), conditions=cond, planes=SR.PLANES, bound_keys=list(BOUND_KEYS))
    store = {"dataset_config_json": np.frombuffer(json.dumps(dcfg).encode(), np.uint8),
             "material_config_json": np.frombuffer(json.dumps(mcfg).encode(), np.uint8),
             "meta_json": np.frombuffer(json.dumps(meta).encode(), np.uint8),
             "pair_lists": np.asarray(pairs_all, np.int64), "n_episodes": np.int64(3), "w_seed": np.int64(seed),
             "samples": np.array([pairs_all.index([ep, t - 3, t - 2, t - 1, t, t + d, min(t + 2 * d, T - 1), min(t + 3 * d, T - 1)])
                                  for ep, t, d in EB.STARTS], np.int64)}
    for k, v in m.items():
        store["margin_" + k] = np.float64(v)
    for e, (o, f, p) in enumerate(eps):
        store[f"ep{e}::obj"], store[f"ep{e}::eef"], store[f"ep{e}::phys"] = o, f, np.asarray(p, np.float32)
    store["draw::fps_start"] = np.array([r["fps_start"] for r in runs], np.int32)
    store["draw::rad_start"] = np.array([r["rad_start"] for r in runs], np.int32)
    fps = np.full((len(runs), EB.MAX_NOBJ), -1, np.int32)
    for j, r in enumerate(runs):
        fps[j, :len(r["fps_idx"])] = r["fps_idx"]
    store["fps_idx"], store["n_obj"] = fps, np.array([len(r["fps_idx"]) for r in runs], np.int32)
    gap = 0.0
    for j, (r, log) in enumerate(zip(runs, logs)):
        pre = f"r{j}::"
        for k in ("idx_list", "error_list", "error64", "pred", "state", "action"):
            store[pre + k] = r[k]
        MG.pack_edges(pre, r["edges"], store)
        store[pre + "cloud"] = np.stack([b[0][0] for b in r["builds"][1:]]) if r["L"] > 1 else np.zeros((0, EB.MAX_NOBJ + 2, 3), np.float32)
        store[pre + "trail"] = np.array([len(b) for b in r["builds"]], np.int32)
        store[pre + "trail::rows"] = np.array([[a[1], a[2], a[3]] for b in r["builds"] for a in b], np.float64).reshape(-1, 3)
        store[pre + "call::bounds"] = np.array([[c["bd"][x] for x in BOUND_KEYS] for c in log], np.float32).reshape(-1, 6)
        store[pre + "call::planes"] = np.array([c["planes"] for c in log], np.int32).reshape(-1, 2)
        gap = max(gap, float(np.abs(r["error_list"].astype(np.float64) - r["error64"]).max()))
    store["ref_gap"] = np.float64(gap)
    print(f"{NAME}: seed {seed} max_nR {max_nR} n_obj {store['n_obj'].tolist()} L {[r['L'] for r in runs]} "
          f"attempts {[[len(b) for b in r['builds']] for r in runs]} kinds {meta['kinds']} conditions {cond} margins "
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
    assert size < 1_000_000
    print(f"{NAME}: second run identical -> {size / 1e3:.0f} KB")


if __name__ == "__main__":
    main()
