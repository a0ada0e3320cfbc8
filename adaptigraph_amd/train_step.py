"""TrainStep: the reference's training iteration (src/dynamics/train/train.py:86-124) resident on the GPU.

step() enqueues ag_train_step (n_future chained forwards, MSE, next-state assembly, backward through the chain) and ag_adam_step
(torch.optim.Adam's formula over the 22 tensors, then the device re-pack of the engine's weight images) and returns: nothing
between two iterations waits for the GPU, no weight travels through the host.  Master weights, Adam's m and v, the gradients and
the status words live on the device for the life of the object.  The autograd path (DynamicsPredictor.forward + loss.backward()
+ torch.optim) is untouched; this is a second way next to it.
"""
from __future__ import annotations

import ctypes as C

import torch

from .autograd import _vp_array
from .context import Engine, ptr, current_stream, _require_gpu

_ADAM_FIXED = {"amsgrad": False, "maximize": False}


def adam_state_to_torch(step, exp_avg, exp_avg_sq, hyper, order):
    """torch.optim.Adam(model.parameters()).state_dict() from TrainStep's state.  Pure host function.
    step: applied steps; exp_avg / exp_avg_sq: 22 tensors in ag_ctx_load_weights order; hyper: lr, betas, eps, weight_decay;
    order[i] = position in ag_ctx_load_weights order of the optimiser's parameter i (model.parameters() order)."""
    dummies = [torch.zeros(1, requires_grad=True) for _ in order]
    group = torch.optim.Adam(dummies, lr=hyper["lr"], betas=tuple(hyper["betas"]), eps=hyper["eps"],
                             weight_decay=hyper["weight_decay"]).state_dict()["param_groups"][0]   # the installed torch's keys
    group["params"] = list(range(len(order)))
    state = {}
    if step > 0:
        for i, k in enumerate(order):
            state[i] = {"step": torch.tensor(float(step)), "exp_avg": exp_avg[k].detach().clone(),
                        "exp_avg_sq": exp_avg_sq[k].detach().clone()}
    return {"state": state, "param_groups": [group]}


def adam_state_from_torch(sd, order):
    """Inverse of adam_state_to_torch: (step, exp_avg[22] or None, exp_avg_sq[22] or None, hyper).  Pure host function."""
    groups = sd["param_groups"]
    if len(groups) != 1 or len(groups[0]["params"]) != len(order):
        raise ValueError("TrainStep: expected one param group over the model's 22 parameters")
    g = groups[0]
    for k, v in _ADAM_FIXED.items():
        if g.get(k, v) != v:
            raise NotImplementedError(f"TrainStep: Adam with {k}={g[k]} is not implemented")
    hyper = dict(lr=float(g["lr"]), betas=(float(g["betas"][0]), float(g["betas"][1])), eps=float(g["eps"]),
                 weight_decay=float(g["weight_decay"]))
    state = sd["state"]
    if not state:
        return 0, None, None, hyper
    if sorted(state.keys()) != list(range(len(order))):
        raise ValueError("TrainStep: optimizer state does not cover the 22 parameters")
    steps = {int(float(state[i]["step"])) for i in range(len(order))}
    if len(steps) != 1:
        raise ValueError(f"TrainStep: parameters at different steps {sorted(steps)}")
    m, v = [None] * len(order), [None] * len(order)
    for i, k in enumerate(order):
        m[k], v[k] = state[i]["exp_avg"], state[i]["exp_avg_sq"]
    return steps.pop(), m, v, hyper


class TrainStep:
    """ts = TrainStep(model, lr=1e-3, n_future=3); loss = ts.step(data, max_edges=k); ...; ts.check(); ts.sync_to_module()."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, n_future=3, store_rest_state=False):
        params = model.ordered_parameters()
        dev = _require_gpu(params[0].device)                     # no CPU fallback, as every other op
        self.model, self.device = model, dev
        self.hyper = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay))
        self.n_future, self.store_rest_state = int(n_future), bool(store_rest_state)
        assert self.n_future >= 1
        ids = {id(p): k for k, p in enumerate(params)}
        self._order = [ids[id(p)] for p in model.parameters()]  # optimiser index -> ag_ctx_load_weights position
        # an engine of its own: model.engine() keeps serving every other caller from the nn.Parameters
        self.engine = Engine(dev, pstep=model.model_config["pstep"], n_his=model.n_his, rel_dim=model.rel_input_dim,
                             motion_clamp=float(model.motion_clamp))
        if model._precision is not None:
            self.engine.set_precision(model._precision)
        self.w = [p.detach().to(dev, torch.float32).clone().contiguous() for p in params]
        self.exp_avg = [torch.zeros_like(w) for w in self.w]
        self.exp_avg_sq = [torch.zeros_like(w) for w in self.w]
        self.grad = [torch.zeros_like(w) for w in self.w]
        self._status = torch.zeros(4, dtype=torch.int32, device=dev)   # [0] overflow flag, [1] applied steps
        self._loss = torch.zeros(self.n_future + 1, device=dev)
        self._step = 0                                                  # host counter of enqueued optimiser steps
        self.last_pred = None
        self._w_arr, self._g_arr = _vp_array(self.w), _vp_array(self.grad)
        self._m_arr, self._v_arr = _vp_array(self.exp_avg), _vp_array(self.exp_avg_sq)
        self._upload()

    def _upload(self):
        eng = self.engine
        eng.check(eng.lib.ag_ctx_load_weights_device(eng.ctx, current_stream(self.device), self._w_arr))

    def _run(self, data, max_edges, want_grad):
        model, dev, eng = self.model, self.device, self.engine
        kw = {k: v for k, v in data.items() if k.endswith("_physics_param")}
        with torch.no_grad():
            state = data["state"].to(device=dev, dtype=torch.float32).contiguous()
            attrs, action, phys, group, edges, n_p = model._inputs(dev, state, data["attrs"], data.get("Rr"), data.get("Rs"),
                                                                   data["p_instance"], data["action"], data.get("edges"), kw)
            B, N = attrs.shape[:2]
            assert state.shape == (B, model.n_his, N, 3)
            nf = self.n_future
            fut = data["state_future"].to(device=dev, dtype=torch.float32)[:, :nf].contiguous()
            assert fut.shape == (B, nf, n_p, 3), tuple(fut.shape)
            eef = act_f = None
            if nf > 1:
                eef = data["eef_future"].to(device=dev, dtype=torch.float32)[:, :nf - 1].contiguous()
                act_f = data["action_future"].to(device=dev, dtype=torch.float32)[:, :nf - 1].contiguous()
                assert eef.shape == (B, nf - 1, N, 3) and act_f.shape == (B, nf - 1, N, 3)
            if max_edges is None:
                max_edges = int(edges.n_edges.max().item())                 # the one wait of the call
            pred = torch.empty((nf, B, n_p, 3), device=dev, dtype=torch.float32)
        eng.check(eng.lib.ag_train_step(
            eng.ctx, current_stream(dev), ptr(state), ptr(attrs), ptr(action), ptr(phys), ptr(group), group.shape[2],
            ptr(edges.recv), ptr(edges.send), ptr(edges.row_ptr), ptr(edges.n_edges), edges.edge_cap, B, N, n_p, self._w_arr,
            nf, ptr(fut), ptr(eef), ptr(act_f), int(self.store_rest_state), max(1, int(max_edges)), int(want_grad), self._g_arr,
            ptr(self._loss), ptr(pred), ptr(self._status)))
        self.last_pred = pred
        return self._loss[nf].clone()

    def step(self, data, max_edges=None):
        """One training iteration on `data` (the dict train.py passes to model(**data): state, attrs, p_instance, action,
        <material>_physics_param, state_future, eef_future, action_future and either edges (an EdgeList) or dense Rr / Rs).
        Returns loss_sum as a 0-d DEVICE tensor.  max_edges: the caller's bound on the largest edge count of the batch (a data
        loader knows it: it built the edges); with it the call only enqueues.  None reads edges.n_edges.max() back once, which is
        then the step's only wait.  A batch with a graph beyond max_edges (or the EdgeList's capacity) is skipped on the device -
        weights, m and v stay as they were - and check() reports it."""
        loss = self._run(data, max_edges, True)
        self._step += 1
        h, eng = self.hyper, self.engine
        eng.check(eng.lib.ag_adam_step(eng.ctx, current_stream(self.device), self._w_arr, self._g_arr, self._m_arr, self._v_arr,
                                       self._step, h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"],
                                       ptr(self._status)))
        return loss

    def evaluate(self, data, max_edges=None):
        """The valid phase: forwards and loss only, no backward, no update.  Returns loss_sum (0-d device tensor); the n_future
        predictions are in .last_pred (n_future, B, n_p, 3).  A batch with a graph beyond max_edges raises the same sticky flag as in
        step(): its loss is then that of the guarded (empty) graph, and every following step() is skipped until check() has
        reported it."""
        return self._run(data, max_edges, False)

    def check(self):
        """One 16-byte read-back (waits for the enqueued steps).  Raises Exception("Exceeds max dims"), as the reference's
        pad_torch does, when a step since the last check was skipped; the step counter is then back at the number of applied
        steps and the flag is cleared, so the object is exactly where it was before the first skipped step."""
        st = self._status.cpu()
        if int(st[0]) != 0:
            self._step = int(st[1])
            self._status[0] = 0
            raise Exception("Exceeds max dims")                  # src/dynamics/utils.py:63-65 raises a bare Exception

    def sync_to_module(self):
        """Device master weights -> the model's nn.Parameters (state_dict / torch.save as before).  Bumps the parameters'
        versions, so a later plain model(...) re-uploads them.  A skipped step never touches the weights, so this needs no check()."""
        with torch.no_grad():
            for p, w in zip(self.model.ordered_parameters(), self.w):
                p.copy_(w)

    def optimizer_state_dict(self):
        """torch.optim.Adam's state_dict layout (the reference's latest_optim.pth), loadable into torch.optim.Adam(model.parameters()).
        Calls check() first (one read-back; raises for a skipped step): the `step` it reports is then the number of applied steps."""
        self.check()
        return adam_state_to_torch(self._step, self.exp_avg, self.exp_avg_sq, self.hyper, self._order)

    def load_optimizer_state_dict(self, sd):
        step, m, v, hyper = adam_state_from_torch(sd, self._order)
        with torch.no_grad():
            for k in range(len(self.w)):
                if m is None:
                    self.exp_avg[k].zero_()
                    self.exp_avg_sq[k].zero_()
                else:
                    self.exp_avg[k].copy_(m[k])
                    self.exp_avg_sq[k].copy_(v[k])
            self._status[1] = step
        self.hyper, self._step = hyper, step
