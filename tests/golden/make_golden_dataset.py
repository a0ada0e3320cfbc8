#!/usr/bin/env python3
"""Generate the DATASET fixtures from the real reference (jhyau/AdaptiGraph): DynDataset.__getitem__ on synthetic episodes.

Runs only where the reference checkout exists (like make_golden.py, whose import recipe it reuses); the tests see only the
.npz files written here.  What is driven (reference file:line):
  * DynDataset.__getitem__                      src/dynamics/dataset/dataset.py:117-383
  * fps (stage 2 = fps_rad_idx, utils.py:10-24) src/dynamics/dataset/graph.py:8-36
  * construct_edges_from_states + back-off      src/dynamics/dataset/graph.py:68-231, dataset.py:310-349
The dataset object is made with object.__new__ and its attributes set by hand from the reference's own yaml (its __init__ reads
files from disk; keys the upstream yaml lacks - connect_tool_all_non_fixed, knn_range, min_knn, ... - take off / 1.0 / 0.1).
dgl is not installed: after the import, dynamics.dataset.graph.farthest_point_sampler is set to the numpy statement of stage 1 in
tests/dataset_restate.py (fps_stage1) - so stage 1 in these fixtures is that statement, not dgl's code.

np.random.randint / uniform are wrapped to record each sample's draws in call order (fps_start, fps_radius, rad_start,
phys_noise, [state_noise, rot], adj_thresh, [knn_thresh]); fps_radius is handed on already rounded to float32, so the float32
distances compare with it alike under every numpy version.  physics_params is deep-copied before each item (the reference adds
the noise in place).  The reference's edge builder is wrapped to record (kNN, topk, n_rel) of every back-off attempt.

Each case is re-seeded until (checked with the oracle's numpy builder): no top-k boundary tie inside the radius at any attempt;
in the augmented case (rope) every unmasked pair distance is more than 1e-4 relative away from the squared radius and every
top-k boundary gap inside the radius is more than 1e-4 relative.

Files (flags: none - every run rewrites all five): dataset_rope, dataset_cloth, dataset_granular, dataset_backoff,
dataset_softbody (.npz).  Usage:  python tests/golden/make_golden_dataset.py
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
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dataset_restate as DR  # noqa: E402
from oracle import adaptigraph_oracle as O  # noqa: E402

OUT = HERE
MARGIN = 1e-4


def import_dataset():
    MG.import_reference()
    import dynamics.dataset.dataset as D
    import dynamics.dataset.graph as G

    def sampler(x, npoints, start_idx=0):
        return torch.from_numpy(DR.fps_stage1(x[0].numpy(), npoints, start_idx))[None]
    G.farthest_point_sampler = sampler
    return D, G


def make_dataset(D, dcfg, mcfg, pair_lists, physics_params, obj_pos, eef_pos, phase="train"):
    """dataset.py:18-112 without the disk."""
    ds = object.__new__(D.DynDataset)
    d = dcfg["datasets"][0]
    ds.phase, ds.dataset_config, ds.material_config, ds.verbose = phase, dcfg, mcfg, False
    ds.n_his, ds.n_future = dcfg["n_his"], dcfg["n_future"]
    ds.store_rest_state = dcfg.get("store_rest_state", False)
    ds.add_randomness = dcfg["randomness"]["use"]
    ds.state_noise = dcfg["randomness"]["state_noise"][phase]
    ds.phys_noise = dcfg["randomness"]["phys_noise"][phase]
    ds.lazy_loading = False
    ds.obj_config, ds.dataset = dcfg["datasets"], d
    ds.max_nobj, ds.fps_radius_range, ds.max_nR = d["max_nobj"], d["fps_radius_range"], d["max_nR"]
    ds.adj_radius_range, ds.topk = d["adj_radius_range"], d["topk"]
    ds.knn_range = d.get("knn_range", [1.0, 1.0])
    ds.min_kNN, ds.knn_increment = d.get("min_knn", 1.0), d.get("knn_increment", 0.1)
    ds.connect_tool_all = d["connect_tool_all"]
    ds.connect_tool_all_non_fixed = d.get("connect_tool_all_non_fixed", False)
    ds.connect_tool_surface = d.get("connect_tool_surface", False)
    ds.connect_tool_surface_ratio = d.get("connect_tool_surface_ratio", 1.0)
    ds.pair_lists = np.array(pair_lists)
    ds.physics_params = physics_params
    ds.materials = {k: v.shape[0] for k, v in physics_params[0].items()}
    ds.eef_pos, ds.obj_pos = eef_pos, obj_pos
    ds.pos_dim, ds.eef_dim = obj_pos[0].shape[-1], eef_pos[0].shape[1]
    ds.obj_dim = ds.max_nobj
    ds.state_dim = ds.obj_dim + ds.eef_dim
    return ds


class Draws:
    """Records the numpy draws of one __getitem__ in call order."""

    def __init__(self):
        self.calls = []
        self._ri, self._un = np.random.randint, np.random.uniform

    def __enter__(self):
        def randint(*a, **k):
            v = self._ri(*a, **k)
            self.calls.append(("randint", v))
            return v

        def uniform(*a, **k):
            v = self._un(*a, **k)
            if len(self.calls) == 1 and np.ndim(v) == 0:          # the second draw of an item is fps_radius (graph.py:22)
                v = float(np.float32(v))
            self.calls.append(("uniform", v))
            return v
        np.random.randint, np.random.uniform = randint, uniform
        return self

    def __exit__(self, *a):
        np.random.randint, np.random.uniform = self._ri, self._un


def run_item(D, ds, i, trail):
    """The real __getitem__ on sample i -> (graph, draws dict)."""
    orig = D.construct_edges_from_states

    def builder(*a, **k):
        Rr, Rs = orig(*a, **k)
        trail.append([float(k.get("kNN", 1.0)), int(a[4]), int(Rr.shape[0])])
        return Rr, Rs
    D.construct_edges_from_states = builder
    ds.physics_params = copy.deepcopy(ds._stored_physics)
    try:
        with Draws() as rec:
            g = MG.quiet(ds.__getitem__, i)
    finally:
        D.construct_edges_from_states = orig
    c = [v for _, v in rec.calls]
    kinds = [k for k, _ in rec.calls]
    assert kinds[:4] == ["randint", "uniform", "randint", "uniform"], kinds
    d = dict(fps_start=int(c[0]), fps_radius=np.float32(c[1]), rad_start=int(c[2]), phys_noise=np.asarray(c[3], np.float64),
             state_noise=None, rot=None)
    k = 4
    if ds.add_randomness:
        d["state_noise"], d["rot"] = np.asarray(c[k], np.float64), float(c[k + 1])
        k += 2
    d["adj_thresh"] = float(c[k])
    d["knn_thresh"] = float(c[k + 1]) if ds.min_kNN < 1.0 else 1.0
    assert len(c) == k + (2 if ds.min_kNN < 1.0 else 1), (len(c), k)
    return g, d


def margins_ok(pos, adj, mask, tool, k):
    """Every unmasked pair distance is MARGIN relative away from the squared radius, every top-k gap inside the radius too."""
    thr2 = np.float32(float(adj) * float(adj))
    dis = O.pairwise_dis(pos)
    dead = ~(mask[:, None] & mask[None, :]) | (tool[:, None] & tool[None, :])
    if (np.abs(np.where(dead, np.inf, dis) - thr2) <= MARGIN * thr2).any():
        return False
    d = np.sort(np.where(dead, O.BIG, dis), axis=1)
    k = min(len(pos), k)
    if k < len(pos):
        both = d[:, k] < thr2
        if (d[both, k] - d[both, k - 1] <= MARGIN * d[both, k]).any():
            return False
    return True


def gen_case(name, D, material, episodes, pairs, samples, seed, over=None, want=None, augmented=False):
    """episodes: list of (obj (T,N,3), eef (T,M,3), phys vector); pairs: (P, 1 + n_frames); samples: indices into pairs."""
    with open(f"{MG.REF}/config/dynamics/{material}.yaml") as f:
        dyn = yaml.safe_load(f)
    dcfg, mcfg = copy.deepcopy(dyn["dataset_config"]), dyn["material_config"]
    dcfg["datasets"][0].update(over or {})
    obj_pos = [e[0] for e in episodes]
    eef_pos = [e[1] for e in episodes]
    phys = [{material: np.asarray(e[2], np.float32)} for e in episodes]
    ds = make_dataset(D, dcfg, mcfg, pairs, phys, obj_pos, eef_pos)
    ds._stored_physics = phys
    spec = DR.parse_config(dcfg, mcfg)
    for attempt in range(200):
        np.random.seed(seed + 1000 * attempt)
        items, draws, trails, ok = [], [], [], True
        for i in samples:
            trail = []
            g, d = run_item(D, ds, i, trail)
            items.append(g), draws.append(d), trails.append(trail)
            pos = g["state"][-1].numpy()
            N = pos.shape[0]
            mask = np.zeros(N, bool)
            mask[:int(g["obj_mask"].sum())] = True
            mask[spec.max_nobj:] = True
            tool = np.zeros(N, bool)
            tool[spec.max_nobj:] = True
            for kNN, k, _ in trail:
                try:
                    O.construct_edges_from_states(pos, d["adj_thresh"], mask, tool, topk=k, connect_tools_all=spec.connect_tool_all,
                                                  connect_tool_all_non_fixed=False, check_ties=True)
                except O.TopkTie:
                    ok = False
                if augmented and not margins_ok(pos, d["adj_thresh"], mask, tool, k):
                    ok = False
        if ok and (want is None or want(trails)):
            break
    else:
        raise SystemExit(f"{name}: no seed met the conditions")
    store = {"dataset_config_json": np.frombuffer(json.dumps(dcfg).encode(), np.uint8),
             "material_config_json": np.frombuffer(json.dumps(mcfg).encode(), np.uint8),
             "pair_lists": np.asarray(pairs, np.int64), "samples": np.asarray(samples, np.int64),
             "n_episodes": np.int64(len(episodes)), "seed": np.int64(seed + 1000 * attempt)}
    for e, (o, f, p) in enumerate(episodes):
        store[f"ep{e}::obj"], store[f"ep{e}::eef"], store[f"ep{e}::phys"] = o, f, np.asarray(p, np.float32)
    pkey = material + "_physics_param"
    for k in ("state", "action", "eef_future", "action_future", "state_future", "attrs", "p_rigid", "p_instance", "obj_mask",
              "material_index", pkey):
        store["out::" + k] = np.stack([g[k].numpy() for g in items])
    Rr, Rs = torch.stack([g["Rr"] for g in items]), torch.stack([g["Rs"] for g in items])
    assert Rr.shape[1] == ds.max_nR
    MG.pack_edges("out::", MG.edges_from_R(Rr, Rs), store)
    for k in ("fps_start", "rad_start"):
        store["draw::" + k] = np.array([d[k] for d in draws], np.int32)
    store["draw::fps_radius"] = np.array([d["fps_radius"] for d in draws], np.float32)
    for k in ("phys_noise", "adj_thresh", "knn_thresh") + (("state_noise", "rot") if ds.add_randomness else ()):
        store["draw::" + k] = np.stack([np.asarray(d[k], np.float64) for d in draws])
    store["trail"] = np.array([len(t) for t in trails], np.int32)
    store["trail::rows"] = np.array([r for t in trails for r in t], np.float64).reshape(-1, 3)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **store)
    print(f"{name}: seed {int(store['seed'])} B={len(samples)} n_obj={[int(g['obj_mask'].sum()) for g in items]} "
          f"edges={store['out::n_edges'].tolist()} attempts={[[r[1] for r in t] for t in trails]} -> {os.path.getsize(path) / 1e3:.0f} KB")


# ---------------------------------------------------------------------------------------------- synthetic episodes
def episode(base, tools, T, rng, drift=0.01, jitter=0.002, tool_step=0.03):
    """A cloud that drifts and jitters over T frames, tool points that advance along x."""
    v = rng.normal(0, drift, (1, 3))
    obj = np.stack([base + v * t + rng.normal(0, jitter, base.shape) for t in range(T)]).astype(np.float32)
    step = np.array([tool_step, 0.0, 0.3 * tool_step])
    eef = np.stack([tools + step * t + rng.normal(0, jitter, tools.shape) for t in range(T)]).astype(np.float32)
    return obj, eef


def rope_base(n, rng):
    t = np.sort(rng.uniform(0, 1, n))
    return np.stack([-1.5 + 3 * t, 0.02 * np.ones(n), 0.4 * np.sin(5 * t)], 1) + rng.normal(0, 0.01, (n, 3))


def sheet_base(n, rng, half=0.8):
    return np.stack([rng.uniform(-half, half, n), rng.normal(0.05, 0.005, n), rng.uniform(-half, half, n)], 1)


def pile_base(n, rng, half):
    return np.stack([rng.uniform(-half, half, n), rng.uniform(0, 0.08, n), rng.uniform(-half, half, n)], 1)


def block_base(n, rng):
    return np.stack([rng.uniform(-0.7, 0.7, n), rng.uniform(0.0, 0.6, n), rng.uniform(-0.7, 0.7, n)], 1)


def windows(ep, T, n_frames, count, rng):
    starts = rng.choice(T - n_frames + 1, count, replace=False)
    return [[ep] + list(range(s, s + n_frames)) for s in sorted(starts)]


def main():
    D, _ = import_dataset()
    torch.set_num_threads(8)
    rng = np.random.default_rng(20)
    T = 12
    # rope: augmentation on, one tool point, episodes of 600, 601 and 37 raw points (the last below max_nobj)
    eps, pairs = [], []
    for e, n in enumerate((600, 601, 37)):
        base = rope_base(n, rng)
        obj, eef = episode(base, base[n // 2][None] + np.array([[0.0, 0.03, 0.12]]), T, rng)
        eps.append((obj, eef, [rng.uniform(0.2, 0.8)]))
        pairs += windows(e, T, 7, 2, rng)
    gen_case("dataset_rope", D, "rope", eps, pairs, list(range(6)), seed=1, augmented=True)
    # cloth: no augmentation, connect_tool_all, top-k 5, two tool points
    eps, pairs = [], []
    for e, n in enumerate((600, 450)):
        base = sheet_base(n, rng)
        obj, eef = episode(base, np.array([[0.1, 0.08, -0.1], [0.1, 0.08, 0.1]]), T, rng)
        eps.append((obj, eef, [rng.uniform(0.2, 0.8)]))
        pairs += windows(e, T, 7, 2, rng)
    gen_case("dataset_cloth", D, "cloth", eps, pairs, list(range(4)), seed=2)
    # granular: top-k 20, five tool points
    tools5 = np.array([[0.5, 0.045, 0.2], [-0.5, 0.045, 0.2], [0.0, 0.045, 0.2], [0.25, 0.045, 0.2], [-0.25, 0.0, 0.2]]) * [0.6, 1, 1]
    eps, pairs = [], []
    for e, (n, half) in enumerate(((600, 0.6), (520, 0.5))):
        obj, eef = episode(pile_base(n, rng, half), tools5, T, rng)
        eps.append((obj, eef, [rng.uniform(0.1, 0.3)]))
        pairs += windows(e, T, 7, 2, rng)
    gen_case("dataset_granular", D, "granular", eps, pairs, list(range(4)), seed=3)
    # back-off: granular piles of different density under a lowered max_nR - at least two graphs back off, at least one does not
    eps, pairs = [], []
    for e, (n, half) in enumerate(((600, 0.45), (600, 0.9))):
        obj, eef = episode(pile_base(n, rng, half), tools5, T, rng)
        eps.append((obj, eef, [rng.uniform(0.1, 0.3)]))
        pairs += windows(e, T, 7, 2, rng)

    def want(trails):
        steps = [len(t) - 1 for t in trails]
        return sum(s >= 1 for s in steps) >= 2 and sum(s == 0 for s in steps) >= 1
    gen_case("dataset_backoff", D, "granular", eps, pairs, list(range(4)), seed=4, over={"max_nR": BACKOFF_MAX_NR}, want=want)
    # softbody: n_his 5, rest state in front of a 7-frame pair, the non-fixed tool rule with its kNN range: the per-sample path
    eps, pairs = [], []
    for e, n in enumerate((600, 500)):
        tools = tools5 * [1, 0, 1] + [0.0, 0.62, -0.2]
        obj, eef = episode(block_base(n, rng), tools, T, rng)
        eps.append((obj, eef, [rng.uniform(0.2, 0.8)]))
        pairs += windows(e, T, 7, 2, rng)
    gen_case("dataset_softbody", D, "softbody", eps, pairs, [0, 1, 2], seed=5)


BACKOFF_MAX_NR = 260


if __name__ == "__main__":
    main()
