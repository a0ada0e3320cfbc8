#!/usr/bin/env python3
"""Generate the PHYSICS-PARAMETER GRADIENT fixtures from the real reference (jhyau/AdaptiGraph): its own autograd through its
own masked rollout.

Runs only where the reference checkout exists (like make_golden.py, whose import recipe it reuses); the tests see only the
.npz files written here.  What is driven (reference file:line), on CPU:
  * planning.forward_dynamics.dynamics_masked.__wrapped__   src/planning/forward_dynamics.py:209-399 - the body that
                                                            @torch.no_grad() wraps, so that it runs under autograd
  * planning.losses.chamfer                                 src/planning/losses.py:4-10
  * DynamicsPredictor.forward + torch autograd              src/dynamics/gnn/model.py:130-342 (the single-forward case)
Nothing of the reference is restated: the float64 runs call the same function on model.double() with float64 as the default
dtype (dynamics_masked allocates its tensors with the default dtype); the few tensors it creates as float32 regardless (attrs,
p_instance, Rr, Rs: exact 0 / 1 values) are cast to the model's dtype where they enter model.forward (GraphRecorder).

Per material (rope: 1-point pusher; granular: 5-point pusher, connect_tools_all; cloth: gripper offset) one file with: the
weight seed (w_seed; tests/train_restate.py:make_weights), padded clouds and masks before the push (state_init, state_mask),
the pushes (action), the observed clouds (state_real, real_mask), the task scalars (task_json), pstep, and for each of three
parameter layouts K in
    shared     the reference's (1,) tensor, one value for all rows             one call on the whole batch
    rows       (B,1): a different value per row                                one call per row (the reference's
    particles  (B,n_p): a value per particle                                   dynamics_masked broadcasts ONE tensor over
                                                                               its batch, so a row-specific parameter is fed
                                                                               row by row; rows never interact)
  K::phys, K::n_steps, K::row_steps (model calls that row b went through: all of the batch's for `shared`, action_repeat[b] when
  fed row by row), K::step<i>::{n_edges,recv,send} (the edge lists every model call saw), K::state_seqs, K::chamfer (per
  interaction), K::loss = mean chamfer, K::dphys, K::dstate_init and their float64 counterparts K::*_64 (the reference's own
  fp32 error is the difference).  dphys / dphys_rows / dphys_particles of the tests are shared::dphys, rows::dphys,
  particles::dphys.
Single-forward case (fwd::*): the graph the first model call of the `rows` run saw, seeded output gradients g_pos / g_motion,
and d(sum(g_pos pred_pos) + sum(g_motion pred_motion)) / d(action, physics parameter) in fp32 and float64.

Two conditions are asserted for every run, and the seeds below are chosen so that the reference meets them: no top-k boundary
tie at any step (make_golden.assert_no_topk_boundary_tie), and identical edge lists at every step between the fp32 and the
float64 run (else the two gradients belong to different graphs).

Usage:  python tests/golden/make_golden_ppm_grad.py [--search]     (--search: print the first seed per material that passes)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
import train_restate as TR  # noqa: E402

OUT = HERE
SEEDS = {"rope": 1, "granular": 1, "cloth": 1}
COUNTS, REAL_COUNTS, MAX_NOBJ = [120, 80, 101], [110, 80, 95], 120


class GraphRecorder:
    """Wraps model.forward: the edges and last-frame positions of every call, and the whole graph of the first one.  Floating
    tensors of another dtype than the model's are cast at this boundary: dynamics_masked builds attrs / p_instance (exact 0 / 1
    constants) and the one-hot Rr / Rs as float32 whatever the default dtype, which model.double() refuses."""

    def __init__(self, model):
        self.steps, self.first = [], None
        self._model, self._orig = model, model.forward
        model.forward = self._fwd

    def _fwd(self, **graph):
        if self.first is None:
            self.first = {k: v.detach().clone() for k, v in graph.items() if torch.is_tensor(v)}
        self.steps.append({"edges": MG.edges_from_R(graph["Rr"], graph["Rs"]),
                           "state_last": graph["state"][:, -1].detach().to(torch.float32),
                           "mask": graph["state_mask"].clone(), "tool": graph["eef_mask"].clone()})
        dtype = next(self._model.parameters()).dtype
        graph = {k: (v.to(dtype) if torch.is_tensor(v) and torch.is_floating_point(v) else v) for k, v in graph.items()}
        return self._orig(**graph)

    def close(self):
        self._model.forward = self._orig


def run(fn, chamfer, model, task, material, case, phys, dtype):
    """One gradient evaluation of loss = mean_b chamfer(pred_b[mask_b], real_b[real_mask_b]).  phys (1,): one batch call;
    (B,k): one call per row with phys[b].  -> dict(loss, chamfer, state_seqs, dphys, dstate_init), steps per call, first graph"""
    B = case["state_init"].shape[0]
    mask, rmask = torch.from_numpy(case["state_mask"]), torch.from_numpy(case["real_mask"])
    st = torch.from_numpy(case["state_init"]).to(dtype).requires_grad_(True)
    real = torch.from_numpy(case["state_real"]).to(dtype)
    action = torch.from_numpy(case["action"]).to(dtype)
    p = torch.from_numpy(phys).to(dtype).requires_grad_(True)
    calls = [slice(0, B)] if p.dim() == 1 else [slice(b, b + 1) for b in range(B)]
    seqs, steps, first = [], [], None
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        for sl in calls:
            rec = GraphRecorder(model)
            np.random.seed(0)
            ppm = MG.make_ppm(task, material)
            out = MG.quiet(fn, st[sl], mask[sl], action[sl], model, torch.device("cpu"), ppm,
                           physics_param={material: p if p.dim() == 1 else p[sl.start]})
            rec.close()
            seqs.append(out["state_seqs"])
            steps.append(rec.steps)
            first = first or rec.first
    finally:
        torch.set_default_dtype(old)
    s = torch.cat(seqs, 0)
    ch = torch.stack([chamfer(s[b][mask[b]][None], real[b][rmask[b]][None])[0] for b in range(B)])
    loss = ch.mean()
    loss.backward()
    for call in steps:
        for stp in call:
            MG.assert_no_topk_boundary_tie(stp["state_last"], stp["mask"], stp["tool"], task["adj_thresh"], task["topk"])
    res = dict(loss=loss.item(), chamfer=ch.detach().numpy(), state_seqs=s.detach().numpy(), dphys=p.grad.numpy().copy(),
               dstate_init=st.grad.numpy().copy())
    return res, steps, first


def step_edges(steps, B):
    """per-call step records -> per global step the (recv, send) of all B rows (a row that its call no longer steps: empty)"""
    n = max(len(c) for c in steps)
    out = []
    for i in range(n):
        rows = []
        for c in steps:
            rows += c[i]["edges"] if i < len(c) else [(np.zeros(0, np.int32), np.zeros(0, np.int32))] * (B // len(steps))
        out.append(rows)
    return out


def same_edges(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(np.array_equal(r0, r1) and np.array_equal(s0, s1)
                                                                for (r0, s0), (r1, s1) in zip(x, y)) for x, y in zip(a, b))


def gen_case(material, seed, refs, write=True):
    DynamicsPredictor, _, _, dynamics_masked = refs
    from planning.losses import chamfer
    fn = dynamics_masked.__wrapped__
    rng = np.random.default_rng(seed)
    dyn, task = MG.load_cfg(material)
    task = dict(task)
    task["max_nR"] = 4000
    n_his = dyn["dataset_config"]["n_his"]
    W = TR.make_weights(seed, n_his=n_his)
    B = len(COUNTS)
    case = dict(state_init=np.zeros((B, MAX_NOBJ, 3), np.float32), state_mask=np.zeros((B, MAX_NOBJ), bool),
                state_real=np.zeros((B, MAX_NOBJ, 3), np.float32), real_mask=np.zeros((B, MAX_NOBJ), bool))
    for b, c in enumerate(COUNTS):
        cloud = MG.rope_cloud(c, rng) if material == "rope" else \
            MG.grid_cloud(11, 0.12 if material == "granular" else 0.3, 0.02, rng)[:c]
        case["state_init"][b, :c] = cloud
        case["state_mask"][b, :c] = True
        r = REAL_COUNTS[b]
        case["state_real"][b, :r] = (cloud + rng.normal(0, 0.05, cloud.shape).astype(np.float32))[:r]
        case["real_mask"][b, :r] = True
    case["action"] = MG.actions_near(case["state_init"][0, :80], B, 1, rng, 2.2, 4.8)[:, 0]
    case["action"][:, 3] = np.float32([2.4, 4.3, 3.3])          # action_repeat 2, 4, 3: every row is captured at another step
    layouts = {"shared": np.float32([0.5]), "rows": np.float32([[0.3], [0.5], [0.8]]),
               "particles": rng.uniform(0.2, 0.8, (B, MAX_NOBJ)).astype(np.float32)}
    store = {"w_seed": np.int64(seed), "pstep": np.int32(dyn["model_config"]["pstep"]),
             "task_json": np.frombuffer(json.dumps(MG.task_scalars(task)).encode(), dtype=np.uint8)}
    store.update(case)

    def model_of(dtype):
        m = MG.make_model(DynamicsPredictor, dyn, seed)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
        return m.double() if dtype == torch.float64 else m

    m32, m64 = model_of(torch.float32), model_of(torch.float64)
    first_rows = None
    for name, phys in layouts.items():
        r32, s32, f32 = run(fn, chamfer, m32, task, material, case, phys, torch.float32)
        r64, s64, _ = run(fn, chamfer, m64, task, material, case, phys, torch.float64)
        e32, e64 = step_edges(s32, B), step_edges(s64, B)
        assert same_edges(e32, e64), f"{material} seed {seed} {name}: the fp32 and the float64 run built different graphs"
        if name == "rows":
            first_rows = f32
        store[f"{name}::phys"] = phys
        store[f"{name}::n_steps"] = np.int32(len(e32))
        store[f"{name}::row_steps"] = np.int32([len(c) for c in s32 for _ in range(B // len(s32))])
        for i, rows in enumerate(e32):
            MG.pack_edges(f"{name}::step{i}::", rows, store)
        for k in ("state_seqs", "chamfer", "dphys", "dstate_init"):
            store[f"{name}::{k}"] = r32[k].astype(np.float32)
            store[f"{name}::{k}_64"] = r64[k].astype(np.float64)
        store[f"{name}::loss"], store[f"{name}::loss_64"] = np.float64(r32["loss"]), np.float64(r64["loss"])
        print(f"  {material} {name}: loss {r32['loss']:.6f} |dphys| max {np.abs(r64['dphys']).max():.3e} "
              f"err32 {np.abs(r32['dphys'] - r64['dphys']).max():.2e}  dstate max {np.abs(r64['dstate_init']).max():.3e} "
              f"err32 {np.abs(r32['dstate_init'] - r64['dstate_init']).max():.2e}  steps {len(e32)}")

    # ---- single forward: the first graph of row 0 of the `rows` run, stacked for all rows would need three graphs; one is enough
    g = first_rows
    pkey = f"{material}_physics_param"
    n_p = g["p_instance"].shape[1]
    g_pos = rng.normal(0, 1, (1, n_p, 3)).astype(np.float32)
    g_mot = rng.normal(0, 1, (1, n_p, 3)).astype(np.float32)
    act = (g["action"].numpy() + rng.normal(0, 0.02, g["action"].shape)).astype(np.float32)   # object rows too
    fphys = rng.uniform(0.2, 0.8, (1, n_p)).astype(np.float32)
    store.update({"fwd::state": g["state"].numpy(), "fwd::attrs": g["attrs"].numpy(), "fwd::p_instance": g["p_instance"].numpy(),
                  "fwd::action": act, "fwd::phys": fphys, "fwd::g_pos": g_pos, "fwd::g_motion": g_mot})
    MG.pack_edges("fwd::", MG.edges_from_R(g["Rr"], g["Rs"]), store)
    for dtype, model, suf in ((torch.float32, m32, ""), (torch.float64, m64, "_64")):
        a = torch.from_numpy(act).to(dtype).requires_grad_(True)
        ph = torch.from_numpy(fphys).to(dtype).requires_grad_(True)
        graph = {k: (v.to(dtype) if torch.is_floating_point(v) else v) for k, v in g.items()}
        graph.update({"action": a, pkey: ph})
        pos, mot = MG.quiet(model, **graph)
        ((pos * torch.from_numpy(g_pos).to(dtype)).sum() + (mot * torch.from_numpy(g_mot).to(dtype)).sum()).backward()
        store["fwd::daction" + suf] = a.grad.numpy().copy()
        store["fwd::dphys" + suf] = ph.grad.numpy().copy()
        store["fwd::pred_pos" + suf] = pos.detach().numpy()
    if write:
        path = os.path.join(OUT, f"ppm_grad_{material}.npz")
        np.savez_compressed(path, **store)
        print(f"ppm_grad_{material}: seed {seed} -> {os.path.getsize(path) / 1e6:.2f} MB")


def main():
    refs = MG.import_reference()
    for material in ("rope", "granular", "cloth"):
        if "--search" in sys.argv:
            for seed in range(1, 40):
                try:
                    gen_case(material, seed, refs, write=False)
                    print(f"{material}: seed {seed} passes")
                    break
                except AssertionError as e:
                    print(f"{material}: seed {seed}: {e}")
        else:
            gen_case(material, SEEDS[material], refs)


if __name__ == "__main__":
    main()
