#!/usr/bin/env python3
"""Generate the EARTH-MOVER fixtures from the real reference (jhyau/AdaptiGraph): its own EarthMoverLoss values, the gradients of
its own autograd and the assignments its scipy.optimize.linear_sum_assignment picks.

Runs only where the reference checkout and scipy exist (make_golden.py's import recipe is reused for the model; loss.py is loaded
by path); the tests see only the .npz files written here.  What is driven (reference file:line):
  * EarthMoverLoss                                 src/dynamics/gnn/loss.py:25-60 (the host solve at :42)
  * DynamicsPredictor.forward + torch autograd     src/dynamics/gnn/model.py:130-342
  * the train loop body with a loss list           src/dynamics/train/train.py:65, 86-124 (loss at :100-102)
on CPU, with seeded weights and synthetic clouds.

emd.npz - standalone cases c<k>:: with x (B,N,3), y (B,M,3), emd (fp32 value of the reference), g_emd (its autograd gradient
toward x), emd_64 (the same module in float64), ind1 / ind2 (B,K) (scipy's assignment per graph on the reference's fp32 distance
matrix), gap (B), seed.
train_emd_rope.npz - make_golden_train.py's layout (batch, edges, w_seed, loss_sum, g::<key> rounded to 14 mantissa bits, dstate0,
err64::<key>, loss_sum_64, adam_losses) for loss_funcs = [(MSELoss, 1), (EarthMoverLoss, 0.5)], plus loss_names, loss_weights,
loss_terms (n_future, 2) = every step's terms before weighting, loss_terms_64, step_gaps (n_future, B), adam_gaps (5), seed.

CONDITIONS (enforced here, recorded in the files; not measurements).
  * uniqueness: gap = float64 cost of the second-best assignment minus the best (tests/emd_restate.py:gap - every matched pair
    forbidden in turn, the problem solved again) >= 1e-4 in every graph of every case, at every step of the chain and at every
    step of the Adam curve.  Two correct implementations then cannot pick different assignments, and gradients compare
    element by element.
  * the reference's fp32 run and a float64 run pick the same assignment.
  * shortcuts fail: in every case with K >= 5 the row-order greedy matching differs from the optimum and the nearest-neighbour
    table is not one-to-one (every graph).  (2,2,2) is built so that both x points' nearest y point is the same one.
  * chain case: the numpy restatement counts, for at least one row, a search of at least K/2 steps.
Seeds are walked from a fixed start up to MAX_TRIES; the first that meets the conditions is stored, nothing is written if none does.

Usage:  python tests/golden/make_golden_emd.py
"""
import copy
import importlib.util
import os
import sys

import numpy as np
import scipy.optimize  # noqa: F401  (loss.py says `import scipy` and uses scipy.optimize)
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_train as MT  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
import emd_restate as ER  # noqa: E402
import train_restate as TR  # noqa: E402

OUT = HERE
MAX_TRIES = 64
GAP = 1e-4
LOSSES = [("mse", 1.0), ("earth_mover", 0.5)]
# (B, N, M), what the case is for
CASES = [((1, 1, 1), "degenerate size"), ((2, 2, 2), "smallest size at which a matching can be wrong"),
         ((3, 7, 5), "y is the row side, unmatched x rows"), ((3, 5, 7), "x is the row side"), ((2, 64, 64), "one wave exactly"),
         ((2, 65, 70), "one column past a wave"), ((2, 100, 100), "the training size"), ((1, 257, 300), "past the 256 threads of a block"),
         ((2, 9, 9), "coincident pair x[0,2] == y[0,4]"), ((1, 48, 48), "chain")]


def load_reference_losses():
    spec = importlib.util.spec_from_file_location("reference_loss", os.path.join(MG.REF, "dynamics", "gnn", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_assignment(x, y):
    """What loss.py:32-42 hands to scipy and gets back, per graph, in the clouds' dtype."""
    xt, yt = torch.as_tensor(x), torch.as_tensor(y)
    x_ = xt[:, :, None, :].repeat(1, 1, yt.size(1), 1)
    y_ = yt[:, None, :, :].repeat(1, xt.size(1), 1, 1)
    dis = torch.norm(torch.add(x_, -y_), 2, dim=3)
    out = [scipy.optimize.linear_sum_assignment(d.numpy(), maximize=False) for d in dis]
    return np.stack([o[0] for o in out]).astype(np.int64), np.stack([o[1] for o in out]).astype(np.int64)


def clouds(shape, rng):
    B, N, M = shape
    if shape == (2, 2, 2):        # both x points are nearest to y_0; the row-order greedy matching is the wrong one
        x = np.array([[0, 0, 0], [1, 0, 0]], np.float64)[None] + rng.normal(0, 0.02, (B, 2, 3))
        y = np.array([[0.6, 0, 0], [-1, 0, 0]], np.float64)[None] + rng.normal(0, 0.02, (B, 2, 3))
        return x.astype(np.float32), y.astype(np.float32)
    if shape == (1, 48, 48):      # chain: x_i at i, y_i at i + 0.4 but the last at -10 - the last row's path moves every match
        K = 48
        x = np.stack([np.arange(K, dtype=np.float64), np.zeros(K), np.zeros(K)], 1)[None] * 0.05
        y = np.stack([np.concatenate([np.arange(K - 1) + 0.4, [-10.0]]), np.zeros(K), np.zeros(K)], 1)[None] * 0.05
        return (x + rng.normal(0, 1e-3, x.shape)).astype(np.float32), (y + rng.normal(0, 1e-3, y.shape)).astype(np.float32)
    x = rng.normal(0, 0.3, (B, N, 3)).astype(np.float32)
    y = (x[:, rng.integers(0, N, M)] + rng.normal(0, 0.1, (B, M, 3))).astype(np.float32)
    if shape == (2, 9, 9):
        y[0, 4] = x[0, 2]
    return x, y


def standalone_case(L, shape, k, seed):
    B, N, M = shape
    K = min(N, M)
    x, y = clouds(shape, np.random.default_rng(seed))
    i32 = reference_assignment(x, y)
    i64 = reference_assignment(x.astype(np.float64), y.astype(np.float64))
    if not (np.array_equal(i32[0], i64[0]) and np.array_equal(i32[1], i64[1])):
        return None
    gaps = ER.batch_gaps(x, y)
    if not (gaps >= GAP).all():
        return None
    costs = [ER.cost_matrix(a, b) for a, b in zip(x, y)]
    if K >= 5 and not all(ER.shortcuts_fail(c) for c in costs):
        return None
    if shape == (2, 2, 2) and not all((c.argmin(1) == c.argmin(1)[0]).all() for c in costs):
        return None
    if shape == (1, 48, 48) and not ER.solve(costs[0])[2].max() >= K / 2:
        return None
    if shape == (2, 9, 9) and not (i32[1][0][list(i32[0][0]).index(2)] == 4):        # the coincident pair is matched
        return None
    mod = L.EarthMoverLoss()
    xt = torch.from_numpy(x).requires_grad_(True)
    v = mod(xt, torch.from_numpy(y))
    v.backward()
    out = {"x": x, "y": y, "gap": gaps, "seed": np.int64(seed), "ind1": i32[0], "ind2": i32[1], "emd": np.float32(v.item()),
           "g_emd": xt.grad.numpy().copy(),
           "emd_64": np.float64(mod(torch.from_numpy(x).double(), torch.from_numpy(y).double()).item())}
    assert np.isfinite(out["g_emd"]).all()
    return {f"c{k}::{key}": val for key, val in out.items()}


def gen_standalone(L):
    store = {"n_cases": np.int32(len(CASES)), "gap_bar": np.float64(GAP)}
    for k, (shape, what) in enumerate(CASES):
        for t in range(MAX_TRIES):
            got = standalone_case(L, shape, k, 100 * (k + 1) + t)
            if got is not None:
                break
        else:
            raise SystemExit(f"emd case {shape}: no seed in {MAX_TRIES} tries met the conditions; nothing written")
        store.update(got)
        print(f"emd c{k} {shape} ({what}): seed {int(got[f'c{k}::seed'])}, gap {got[f'c{k}::gap']}, emd {got[f'c{k}::emd']:.6g}")
    path = os.path.join(OUT, "emd.npz")
    np.savez_compressed(path, **store)
    print(f"emd.npz: {os.path.getsize(path) / 1e6:.3f} MB")


def train_loss(L, model, data, n_future, pkey, dtype=torch.float32):
    """make_golden_train.train_loss with loss_funcs = [(MSELoss, 1), (EarthMoverLoss, 0.5)] (train.py:65): returns loss_sum, the
    per-step terms (unweighted) and every step's (prediction, label)."""
    d = {k: (v.to(dtype) if torch.is_floating_point(v) else v) for k, v in data.items()}
    graph = dict(state=d["state"], attrs=d["attrs"], Rr=d["Rr"], Rs=d["Rs"], p_instance=d["p_instance"], action=d["action"],
                 **{pkey: d["physics_param"]})
    funcs = {"mse": torch.nn.MSELoss(), "earth_mover": L.EarthMoverLoss()}
    loss_funcs = [(funcs[name], w) for name, w in LOSSES]
    loss_sum, table, pairs = 0, [], []
    for fi in range(n_future):
        gt_state = d["state_future"][:, fi].clone()
        pred_state, _ = MG.quiet(model, **graph)
        pred_state_p = pred_state[:, :gt_state.shape[1], :3].clone()
        vals = [func(pred_state_p, gt_state) for func, _ in loss_funcs]
        loss_sum = loss_sum + sum([weight * v for (_, weight), v in zip(loss_funcs, vals)])     # train.py:100-102
        table.append([v.item() for v in vals])
        pairs.append((pred_state_p.detach().numpy().copy(), gt_state.numpy().copy()))
        if fi < n_future - 1:
            next_state = d["eef_future"][:, fi].clone().unsqueeze(1)
            next_state[:, -1, :pred_state_p.shape[1]] = pred_state_p
            graph["state"] = torch.cat([graph["state"][:, 1:], next_state], dim=1)
            graph["action"] = d["action_future"][:, fi].clone()
    return loss_sum, np.array(table, np.float64), pairs


def same_assignment(p32, p64):
    a, b = reference_assignment(*p32), reference_assignment(*p64)
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def train_case(L, refs, seed, B=3, n_p=40, topk=10, adj_thresh=0.5, n_future=3):
    DynamicsPredictor, construct_edges, _, _ = refs
    dyn, _ = MG.load_cfg("rope")
    rng = np.random.default_rng(seed)
    n_his = dyn["dataset_config"]["n_his"]
    cloud = MT.rope_cloud(n_p, rng)
    tool = np.array([[cloud[n_p // 2, 0], 0.02, cloud[n_p // 2, 2] + 0.15]], np.float32)
    model = MG.make_model(DynamicsPredictor, dyn, seed)
    W = TR.make_weights(seed, n_his=n_his)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    np_data = MT.make_batch(cloud, tool, B, n_his, rng)
    N = n_p + 1
    states = torch.from_numpy(np_data["state"][:, -1])
    mask = torch.ones(B, N, dtype=torch.bool)
    tool_mask = torch.zeros(B, N, dtype=torch.bool)
    tool_mask[:, n_p:] = True
    try:
        MG.assert_no_topk_boundary_tie(states, mask, tool_mask, adj_thresh, topk)
    except AssertionError:
        return None
    Rr, Rs = MG.quiet(construct_edges, states, adj_thresh, mask, tool_mask, topk=topk, connect_tools_all=False)
    data = {k: torch.from_numpy(v) for k, v in np_data.items()}
    data.update(Rr=Rr, Rs=Rs)
    pkey = "rope_physics_param"

    model.train()
    d0 = dict(data)
    d0["state"] = data["state"].clone().requires_grad_(True)
    loss, table, pairs = train_loss(L, model, d0, n_future, pkey)
    m64 = copy.deepcopy(model).double()
    m64.zero_grad()
    d64 = dict(data)
    d64["state"] = data["state"].double().clone().requires_grad_(True)
    l64, table64, pairs64 = train_loss(L, m64, d64, n_future, pkey, dtype=torch.float64)
    step_gaps = np.stack([ER.batch_gaps(p, g) for p, g in pairs64])
    if not (step_gaps >= GAP).all():
        return None
    if not all(same_assignment(a, b) for a, b in zip(pairs, pairs64)):
        return None

    store = {"w_seed": np.int64(seed), "seed": np.int64(seed), "l2_scale": np.float32(1.0), "l2_shift": np.zeros(3, np.float32)}
    store.update(np_data)
    MG.pack_edges("", MG.edges_from_R(Rr, Rs), store)
    store["n_future"] = np.int32(n_future)
    store["pstep"] = np.int32(dyn["model_config"]["pstep"])
    store["loss_names"] = np.array([n for n, _ in LOSSES])
    store["loss_weights"] = np.array([w for _, w in LOSSES], np.float64)
    store["loss_terms"], store["loss_terms_64"] = table, table64
    store["step_gaps"], store["gap_bar"] = step_gaps, np.float64(GAP)
    loss.backward()
    l64.backward()
    store["loss_sum"], store["loss_sum_64"] = np.float64(loss.item()), np.float64(l64.item())
    g32 = {k: p.grad.numpy().copy() for k, p in model.named_parameters()}
    for k, g in g32.items():
        store["g::" + k] = MT.trim(g)
    for k, p in m64.named_parameters():
        store["err64::" + k] = np.float64(np.abs(g32[k] - p.grad.numpy()).max())
    store["dstate0"] = d0["state"].grad.numpy().copy()
    store["dstate0_64"] = d64["state"].grad.numpy().copy()

    m = copy.deepcopy(MG.make_model(DynamicsPredictor, dyn, seed))
    m.load_state_dict(model.state_dict())
    opt = torch.optim.Adam(m.parameters(), lr=0.001)
    curve, adam_gaps = [], []
    m.train()
    for _ in range(5):
        opt.zero_grad()
        ls, _, prs = train_loss(L, m, data, n_future, pkey)
        adam_gaps.append(min(ER.batch_gaps(p, g).min() for p, g in prs))
        ls.backward()
        opt.step()
        curve.append(ls.item())
    if not min(adam_gaps) >= GAP:
        return None
    store["adam_losses"], store["adam_gaps"] = np.array(curve, np.float64), np.array(adam_gaps, np.float64)
    return store


def gen_train(L, refs):
    for t in range(MAX_TRIES):
        store = train_case(L, refs, 31 + t)
        if store is not None:
            break
        print(f"train_emd_rope: seed {31 + t} does not meet the conditions")
    else:
        raise SystemExit(f"train_emd_rope: no seed in {MAX_TRIES} tries met the conditions; nothing written")
    path = os.path.join(OUT, "train_emd_rope.npz")
    np.savez_compressed(path, **store)
    print(f"train_emd_rope: seed {int(store['seed'])}, edges/graph {store['n_edges'].tolist()}, loss {store['loss_sum']:.6g}, "
          f"terms {np.round(store['loss_terms'], 6).tolist()}, gaps {store['step_gaps'].min(1)}, adam gaps {store['adam_gaps']}, "
          f"adam {np.round(store['adam_losses'], 6).tolist()} -> {os.path.getsize(path) / 1e6:.2f} MB")


def main():
    refs = MG.import_reference()
    L = load_reference_losses()
    torch.set_num_threads(8)
    gen_standalone(L)
    gen_train(L, refs)


if __name__ == "__main__":
    main()
